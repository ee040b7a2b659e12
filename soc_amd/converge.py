"""converge -- how much the dust emission changed from one re-emission iteration to the next: the criterion of `convergence eps [kmin]`
in soc_amd.driver (not a key of the reference, whose users look at the maps and run again).

The quantity is the frequency-integrated luminosity of every cell, so one plane of CELLS doubles is carried from iteration to
iteration, not a second emission array.  For the emission E[CELLS, NFREQ] of an iteration:

    w[c] = (double)(float)(COEFF[level(c)] * DENS[c])      the float product of the cell-emission launches (soc_set_emission_column)
    B[c] = sum_f (double)E[c][f] * W[f]                    in double, f ascending, every product and every sum rounded
    L[c] = B[c] * w[c];  0 in a link or an empty cell (DENS < 1e-10) whatever its row holds;  a live cell whose L is negative or not
           finite is counted as bad and gives 0

and with Lp the luminosities of the iteration before (zeros before the first)

    S_abs = sum |L - Lp|,  S_new = sum L,  S_old = sum Lp,  M = max |L - Lp| / max(L, Lp) over the cells where max(L, Lp) > 0

These are the host statements of soc_emitted_change (soc_amd/csrc/soc_reemit.hip), which makes the same L to the bit from the
emission resident on the device; they serve engines without that call, `emission_source='host'` and runs on several ranks, where
every rank holds the whole emission.  figures() turns the statistics of either path into the three numbers reported:

    d_l1    = S_abs / S_new            the luminosity-weighted relative change: the criterion
    d_total = |S_new - S_old| / S_new  the change of the total luminosity
    d_max   = M                        the largest relative change of a cell (dominated by the Monte Carlo noise of single cells)
"""
import numpy as np


def luminosity(E, W, DENS, OFF, LCELLS, COEFF):
    """E[CELLS, NFREQ] float32, W[NFREQ] (launch.trapezoid_weight), the hierarchy's DENS[CELLS], OFF[LEVELS], LCELLS[LEVELS] and
    COEFF[LEVELS] (rounded to float32 as the engine takes them) -> (L[CELLS] float64, bad)"""
    E = np.asarray(E)
    CELLS, NFREQ = E.shape
    W = np.asarray(W, np.float64)
    DENS = np.asarray(DENS, np.float32)
    COEFF = np.asarray(COEFF, np.float32)
    if W.shape != (NFREQ,) or DENS.shape != (CELLS,):
        raise ValueError("luminosity: E[%d, %d] needs W[%d] and DENS[%d]" % (CELLS, NFREQ, NFREQ, CELLS))
    w = np.zeros(CELLS, np.float32)
    for level in range(len(COEFF)):
        a, b = int(OFF[level]), int(OFF[level]) + int(LCELLS[level])
        w[a:b] = COEFF[level] * DENS[a:b]                                  # float32 x float32, rounded to float32
    B = np.zeros(CELLS, np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        for f in range(NFREQ):                                             # (the order of the device's sum; not a dot product)
            B = B + E[:, f].astype(np.float64) * W[f]
        L = B * w.astype(np.float64)
        dead = DENS < np.float32(1.0e-10)
        fine = np.isfinite(L) & (L >= 0.0)
    bad = int(np.count_nonzero(~dead & ~fine))
    return np.where(dead | ~fine, 0.0, L), bad


def change(L, Lp):
    """dict(S_abs, S_new, S_old, M) of two planes of luminosities (both finite and >= 0, as luminosity() leaves them)"""
    L, Lp = np.asarray(L, np.float64), np.asarray(Lp, np.float64)
    diff, top = np.abs(L - Lp), np.maximum(L, Lp)
    some = top > 0.0
    M = float(np.max(diff[some] / top[some])) if some.any() else 0.0
    return dict(S_abs=float(np.sum(diff)), S_new=float(np.sum(L)), S_old=float(np.sum(Lp)), M=M)


def figures(stats):
    """dict(d_l1, d_total, d_max) from the statistics of change() or of Engine.emitted_change()"""
    S_abs, S_new, S_old = float(stats["S_abs"]), float(stats["S_new"]), float(stats["S_old"])

    def ratio(a):
        if S_new > 0.0:
            return a / S_new
        return 0.0 if a == 0.0 else float("inf")
    return dict(d_l1=ratio(S_abs), d_total=ratio(abs(S_new - S_old)), d_max=float(stats["M"]))
