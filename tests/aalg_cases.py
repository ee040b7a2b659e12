"""Polarised emission of aligned grains (`aalg`): the numpy restatement that tests/test_aalg.py (CPU) and tests/test_gpu_aalg.py
(GPU) hold the code to, and the inputs they share.  The restatement follows the reference line by line -- A2E.py:413-429, 533-539
(the per-size weights and the sum over sizes and batches), A2E_MABU.py:615-637 (an equilibrium dust's table <dust>.rpol),
:1139-1147, :1182 (the abundance-weighted sum and the ratio) -- with its loops over sizes, batches and cells, and is built from the
per-size emissions the engine's solvers return, which the existing suite pins to the oracle.  It is no test module."""
import os

import numpy as np

from soc_amd import a2e, mabu
from soc_amd.launch import FACTOR
from soc_amd.synth import a2e_absorption_fraction

f32 = np.float32


# ---- A2E.py ---------------------------------------------------------------------------------------------------------
def literal_weight(ASIZE, isize, aalg):
    """W[cells] of one size, cell by cell: A2E.py:417 (hard cutoff), :423-425 (the partial arm), in numpy float32 scalars"""
    ASIZE = np.asarray(ASIZE, f32)
    NSIZE = len(ASIZE)
    W = np.zeros(len(aalg), f32)
    for c, a in enumerate(np.asarray(aalg, f32)):
        if ASIZE[isize] >= a:
            W[c] = 1.0
        elif isize < (NSIZE - 1):
            if (ASIZE[isize] < a) & (ASIZE[isize + 1] > a):
                W[c] = (np.log10(a) - np.log10(ASIZE[isize])) / (np.log10(ASIZE[isize + 1]) - np.log10(ASIZE[isize]))
    return W


def per_size_emissions(engine, sol, ABSORBED, NSTOCH=999):
    """emit[isize][CELLS, NFREQ] as the solvers return it: a2e_solve for a stochastic size, a2e_eqtemp (on ABSORBED * AF, with the
    tables of soc_amd.a2e.eq_table) for an equilibrium one; None for an equilibrium size the program skips (A2E.py:466).
    ABSORBED with its last channel clipped (A2E.py:184-185)."""
    CELLS, NFREQ = ABSORBED.shape
    out = []
    for isize in range(sol["NSIZE"]):
        AF = a2e_absorption_fraction(sol, isize)
        if isize >= NSTOCH or isize >= len(sol["sizes"]):
            if sol["S_FRAC"][isize] < 1.0e-30:
                out.append(None)
                continue
            Emin, kE, oplgkE, TTT, KABS = a2e.eq_table(sol, isize)
            _, emit = engine.a2e_eqtemp(0, CELLS, a2e.NIP, FACTOR, kE, oplgkE, Emin, sol["FREQ"], KABS, TTT, np.asarray(ABSORBED * AF, f32))
        else:
            engine.a2e_set_size(sol["NE"], NFREQ, sol["sizes"][isize], AF)
            emit = engine.a2e_solve(ABSORBED)
        out.append(np.array(emit, f32))
    return out


def clipped(ABSORBED):
    A = np.array(ABSORBED, f32)
    A[:, -1] = np.clip(A[:, -1], 0.0, 0.2 * A[:, -2])
    return A


def restated_pemitted(sol, aalg_all, emits, NSTOCH=999, IFREQ=-1, BATCH=8192):
    """PEMITTED of A2E.py from the per-size emissions: the loop over the sizes, inside it the loop over the batches with the aalg
    file read batch by batch (:387, :415; :534), the masks and the weight on the batch's cells."""
    ASIZE, NSIZE, GD, S_FRAC = np.asarray(sol["SIZE_A"], f32), sol["NSIZE"], sol["GD"], sol["S_FRAC"]
    CELLS, NFREQ = emits[0].shape
    PEMITTED = np.zeros((CELLS, 1 if IFREQ >= 0 else NFREQ), f32)
    log10, nonzero = np.log10, np.nonzero
    with np.errstate(all="ignore"):
        for isize in range(NSIZE):
            if emits[isize] is None:
                continue
            for icell in range(0, CELLS, BATCH):
                batch = min([BATCH, CELLS - icell])
                emit = emits[isize][icell:icell + batch]
                aalg = np.asarray(aalg_all[icell:icell + batch], f32)
                if isize >= NSTOCH or isize >= len(sol["sizes"]):                          # A2E.py:533-539
                    m = np.nonzero(ASIZE[isize] >= aalg)
                    if IFREQ >= 0:
                        PEMITTED[icell + m[0], 0] += emit[m[0], IFREQ] * GD * S_FRAC[isize]
                    else:
                        PEMITTED[icell + m[0], :] += emit[m[0], :] * GD * S_FRAC[isize]
                    continue
                m = nonzero(ASIZE[isize] >= aalg)                                          # A2E.py:417-421
                if IFREQ >= 0:
                    PEMITTED[icell + m[0], 0] += emit[m[0], IFREQ]
                else:
                    PEMITTED[icell + m[0], :] += emit[m[0], :]
                if isize < (NSIZE - 1):                                                    # A2E.py:423-429
                    m = nonzero((ASIZE[isize] < aalg) & (ASIZE[isize + 1] > aalg))
                    w = (log10(aalg[m]) - log10(ASIZE[isize])) / (log10(ASIZE[isize + 1]) - log10(ASIZE[isize]))
                    if IFREQ >= 0:
                        PEMITTED[icell + m[0], 0] += w * emit[m[0], IFREQ]
                    else:
                        PEMITTED[icell + m[0], :] += w[:, None] * emit[m[0], :]            # (one weight per cell, for its row)
    return PEMITTED


def edge_aalg(ASIZE, n):
    """n values that walk through every arm of every size, neighbours in different arms: 0 (log10 = -inf: every size aligned, the
    logarithm not used), each size itself (>=: aligned), a value between each pair of sizes (the partial arm of the lower, the
    upper aligned), the next float above and below each size, and a value above the largest size (nothing aligned)"""
    ASIZE = np.asarray(ASIZE, f32)
    v = [f32(0.0)]
    for k, s in enumerate(ASIZE):
        v += [s, np.nextafter(s, f32(np.inf)), np.nextafter(s, f32(0.0))]
        if k + 1 < len(ASIZE):
            v += [f32(np.sqrt(np.float64(s) * np.float64(ASIZE[k + 1]))), f32(0.75 * s + 0.25 * ASIZE[k + 1])]
    v += [f32(2.0) * ASIZE[-1]]
    v = np.asarray(v, f32)
    return v[np.arange(n) % len(v)]


def write_aalg(path, aalg, cells=None):
    with open(path, "wb") as fp:
        np.asarray([len(aalg) if cells is None else cells], np.int32).tofile(fp)
        np.asarray(aalg, f32).tofile(fp)
    return path


# ---- A2E_MABU.py ----------------------------------------------------------------------------------------------------
def write_rpol(path, apol, fpol, R):
    """<dust>.rpol: the first row the frequencies (behind a corner value), the first column the sizes, R[size, frequency]"""
    d = np.zeros((len(apol) + 1, len(fpol) + 1))
    d[0, 1:], d[1:, 0], d[1:, 1:] = fpol, apol, R
    np.savetxt(path, d, fmt="%.17e")
    return path


def synthetic_rpol(path, FREQ, amin, amax, NA=9, seed=21):
    """a table on sizes amin..amax whose frequency columns lie strictly inside FREQ (so that frequencies fall outside the columns
    on both sides: below the first, the weight wj is negative -- an extrapolation; above the last, the last column is taken)"""
    rng = np.random.default_rng(seed)
    FREQ = np.asarray(FREQ, np.float64)
    fpol = np.geomspace(FREQ[2] * 1.07, FREQ[-3] * 0.93, 5)
    apol = np.geomspace(amin, amax, NA).astype(f32).astype(np.float64)             # (sizes a float32 aalg can hit exactly)
    R = np.sort(rng.uniform(0.0, 1.0, (NA, len(fpol))), axis=0)[::-1].copy()       # falls with the minimum aligned size
    write_rpol(path, apol, fpol, R)
    return np.loadtxt(path)[1:, 0]                                                 # the sizes as the file holds them


def literal_rpol_column(d, freq):
    """A2E_MABU.py:622-633 for one frequency (a float32 scalar, as SolveEquilibriumDust's FREQ[ifreq]): (apol, tmp)"""
    from numpy import argmin, log
    Rpol = d[1:, 1:]
    apol = d[1:, 0]
    fpol = d[0, 1:]
    i = argmin(abs(fpol - freq))
    if (fpol[i] > freq):
        i = max([i - 1, 0])
    j = min([i + 1, len(fpol) - 1])
    if (i == j):
        wj = 0.0
    else:
        wj = (log(freq) - log(fpol[i])) / (log(fpol[j]) - log(fpol[i]))
    tmp = (1.0 - wj) * Rpol[:, i] + wj * Rpol[:, j]
    return apol, tmp


def literal_ipR(apol, tmp, aalg):
    """the linear interpolation of A2E_MABU.py:635 cell by cell in Python floats (IEEE doubles, one operation at a time): the node
    value on a node, slope = (y1 - y0) / (x1 - x0) and slope * (x - x0) + y0 between nodes, 0 outside"""
    apol, tmp = [float(x) for x in apol], [float(y) for y in tmp]
    out = np.zeros(len(aalg), np.float64)
    for c, x in enumerate(float(a) for a in np.asarray(aalg, f32)):
        if x < apol[0] or x > apol[-1]:
            continue
        j = max(k for k in range(len(apol)) if apol[k] <= x)
        if j == len(apol) - 1 or apol[j] == x:
            out[c] = tmp[j]
        else:
            slope = (tmp[j + 1] - tmp[j]) / (apol[j + 1] - apol[j])
            out[c] = slope * (x - apol[j]) + tmp[j]
    return out


def restated_R(engine, dusts, kinds, FABS, ABU, aalg_of, c0=0, CELLS=None):
    """<emitted>.R of A2E_MABU.py for the rows of FABS (cells c0.. of a model of CELLS cells): per dust the split
    (mabu.split_absorbed, pinned by the existing suite), the solver's emission -- an equilibrium dust from engine.eqsolver, a
    stochastic one size by size --, its polarised emission (:615-637, or A2E.py via restated_pemitted), both summed in steps of
    1024 cells weighted by the abundances (:1131-1147), and FPEP /= (FPE + 1e-32) (:1182).  aalg_of: per dust aalg[cells] or None.
    Returns (R, FPE)."""
    n, NFREQ = FABS.shape
    CELLS = n if CELLS is None else CELLS
    RABS, _ = mabu.relative_cross_sections(dusts, kinds)
    FPE, FPEP = np.zeros((n, NFREQ), f32), np.zeros((n, NFREQ), f32)
    with np.errstate(all="ignore"):
        for IDUST, (dust, kind) in enumerate(zip(dusts, kinds)):
            part = mabu.split_absorbed(FABS, RABS, ABU, IDUST)
            PEMITTED = None
            if kind == 'eqdust':
                FREQ, KABS, Emin, kE, oplgkE, TTT = mabu.eq_dust_table(dust)
                _, EMITTED = engine.eqsolver(c0, CELLS, mabu.NE_EQ, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, part)
                if aalg_of[IDUST] is not None:
                    d = np.loadtxt('%s.rpol' % (dust.replace('.dust', '')))
                    PEMITTED = np.zeros((n, NFREQ), f32)
                    for ifreq in range(NFREQ):
                        apol, tmp = literal_rpol_column(d, FREQ[ifreq])
                        PEMITTED[:, ifreq] = EMITTED[:, ifreq] * literal_ipR(apol, tmp, aalg_of[IDUST])
            else:
                from soc_amd import files
                sol = files.read_solver(mabu.solver_name(dust))
                emits = per_size_emissions(engine, sol, clipped(part))
                EMITTED = np.zeros((n, NFREQ), f32)
                for e in emits:
                    EMITTED += e
                if aalg_of[IDUST] is not None:
                    PEMITTED = restated_pemitted(sol, aalg_of[IDUST], emits)
            a = 0
            while (a < n):
                b = min(a + 1024, n)
                FPE[a:b, :] += EMITTED[a:b] * ABU[a:b, IDUST].reshape(b - a, 1)
                if PEMITTED is not None:
                    FPEP[a:b, :] += PEMITTED[a:b] * ABU[a:b, IDUST].reshape(b - a, 1)
                a += 1024
        FPEP /= (FPE + 1.0e-32)
    return FPEP, FPE


class Batches:
    """an engine without the resident calls: soc_amd.a2e.run then works in batches, as tools/exp_a2e.py makes it"""

    def __init__(self, engine):
        self.engine = engine

    def __getattr__(self, name):
        if name.startswith("a2e_resident"):
            raise AttributeError(name)
        return getattr(self.engine, name)


def pol_ini_lines(d, eq_aalg, st_aalg):
    return "polarisation %s/sil.dust %s\npolarisation %s/gs_pah %s\n" % (d, eq_aalg, d, st_aalg)


def stage_inputs(d, CELLS, NFREQ, seed=31):
    """Inputs of the multi-dust stage on the three dusts of tests/test_mabu.py (sil.dust: equilibrium, with sil.rpol; gs_pah.dust:
    stochastically heated; carb.dust: no polarisation): absorptions with parent-cell rows (-1e20) and all-zero rows (emission 0 at
    the frequencies where the Planck function underflows: 0 / (0 + 1e-32)), abundances, and the two aalg arrays -- the
    equilibrium dust's below, on and above the nodes of sil.rpol, the stochastic dust's through every arm of its sizes."""
    from soc_amd import files
    rng = np.random.default_rng(seed)
    sol = files.read_solver(os.path.join(d, "pah.solver"))
    FABS = (rng.uniform(0.0, 1.0, (CELLS, NFREQ)) * 10.0 ** rng.uniform(-9, -5, (CELLS, 1))).astype(f32)
    FABS[rng.uniform(size=CELLS) < 0.1] = f32(-1.0e20)
    FABS[3:CELLS:97] = 0.0
    ABU = rng.uniform(0.2, 1.5, (CELLS, 3)).astype(f32)
    apol = synthetic_rpol(os.path.join(d, "sil.rpol"), sol["FREQ"], 2.0e-7, 6.0e-5)
    a_eq = (10.0 ** rng.uniform(np.log10(apol[0]) - 0.3, np.log10(apol[-1]) + 0.3, CELLS)).astype(f32)
    nodes = np.asarray(apol, f32)
    assert np.array_equal(nodes.astype(np.float64), apol)                           # (a float32 aalg can hit every node exactly)
    a_eq[1:1 + 7 * len(nodes):7] = nodes
    a_eq[0], a_eq[2] = f32(apol[0] * 0.5), f32(apol[-1] * 2.0)
    a_st = edge_aalg(sol["SIZE_A"], CELLS)[rng.permutation(CELLS)]
    return FABS, ABU, a_eq, a_st, sol


def driver_case(d, cloud, IF=5):
    """tests/test_driver.py::write_case with `polarisation` lines for both dusts, the three B files of `polmap` and `mapum` at
    frequency IF alone, as two ini files in their own directories: 'mem' without `polred`, 'file' with `polred <d>/R.bin`"""
    from soc_amd import files, launch, synth
    from test_driver import write_case
    ini, sol, abu = write_case(d, cloud)
    apol = synthetic_rpol(os.path.join(d, "sil.rpol"), sol["FREQ"], 2.0e-7, 6.0e-5)
    rng = np.random.default_rng(17)
    write_aalg(os.path.join(d, "sil.aalg"), (10.0 ** rng.uniform(np.log10(apol[0]), np.log10(apol[-1]), cloud.CELLS)).astype(f32))
    write_aalg(os.path.join(d, "pah.aalg"), edge_aalg(sol["SIZE_A"], cloud.CELLS)[rng.permutation(cloud.CELLS)])
    for name, b in zip("xyz", synth.magnetic_field(cloud, seed=2)):
        files.write_temperature(os.path.join(d, "b%s.bin" % name), cloud, b)
    um = 1.0e4 * launch.C_LIGHT / float(f32(sol["FREQ"][IF]))
    extra = "polmap %s/bx.bin %s/by.bin %s/bz.bin\nmapum %.4f\n" % (d, d, d, um) + pol_ini_lines(d, d + "/sil.aalg", d + "/pah.aalg")
    with open(ini) as fp:
        text = fp.read()
    inis = {}
    for tag, more in (("mem", ""), ("file", "polred %s/R.bin\n" % d)):
        os.makedirs(os.path.join(d, tag))
        inis[tag] = os.path.join(d, tag + ".ini")
        with open(inis[tag], "w") as fp:
            fp.write(text + extra + more)
    return inis, sol
