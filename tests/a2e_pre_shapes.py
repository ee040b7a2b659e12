"""Inputs of the solver-preprocessing shape tests (tests/test_a2e_pre_shapes.py on the CPU, tests/test_gpu_a2e_pre_shapes.py on the
GPU): the sizes at which soc_pre_weights_kernel takes a second and later pass of upper bins, soc_pre_cooling_kernel a second and
later pass of frequency intervals, the launcher its LDS attribute and its limit -- and grids with uneven frequencies, a narrow bin,
pairs no frequency feeds, no window at all.  The oracle's result is computed once per case and shared (read-only)."""
import functools

import numpy as np

from soc_amd import a2e_pre, launch

FACTOR = launch.kernel_literals(1.0)[0]
PRE_T = 64                         # lanes of the weights workgroup = upper bins per pass; lanes of the cooling wave = intervals per pass
LDS_LIMIT = 160 * 1024             # of a workgroup
LDS_DEFAULT = 64 * 1024            # dynamic LDS a kernel may ask for without the attribute
NFREQ_MAX = 639                    # the largest NFREQ whose columns fit: (639 * 64 + 64) * 4 = 160 KB

# name -> (NFREQ, NE, isize) on the standard grid (that of make_golden.a2e_pre_cases with AnalyticDust(NSIZE=3))
STANDARD = {
    "ne65": (50, 65, 1),           # the last size with one pass of upper bins
    "ne66": (50, 66, 1),           # a second pass of one lane
    "ne128": (50, 128, 1),         # the sizes README quotes
    "ne256": (50, 256, 0),
    "ne130": (70, 130, 1),         # three passes
    "ne280": (50, 280, 1),         # five passes at the largest NE the solver accepts
    "nf130": (130, 24, 0),         # three passes of the cooling kernel's interval loop
    "nf255": (255, 12, 0),         # the last size without the LDS attribute
    "nf256": (256, 12, 0),         # the first with it
    "nf639": (639, 8, 0),          # the LDS limit
    "nf2": (2, 3, 1),              # the smallest NFREQ
    "ne2": (3, 2, 1),              # the smallest NE: one workgroup, one pair
}
# name -> (NFREQ, NE): the recipe of test_a2e_pre.py::test_oracle_live_vs_reference_other_grids
RANDOM = {"rnd150": (90, 150), "rnd70": (140, 70), "rnd30": (300, 30)}
EMPTY = "empty"                    # no window meets the frequencies
NAMES = tuple(STANDARD) + tuple(RANDOM) + (EMPTY,)
OTHER = {"small": (24, 16, 0), "nf640": (640, 8, 0)}     # a golden case of test_a2e_pre.py to come back to; one frequency too many
SOLVER_NE = (128, 256)             # device-built tables through DoSolve: four cells and one cell per workgroup at NFREQ = 50
SOLVER_SCALES = (1e-6, 1e-3, 1.0, 30.0, 1e3, 1e5, 0.0)


def lds_bytes(NFREQ):
    """dynamic LDS of soc_pre_weights_kernel: a column of NFREQ floats per lane and the scan (soc_launch_a2e_pre)"""
    return (NFREQ * PRE_T + PRE_T) * 4


def standard_freq(NFREQ):
    return np.logspace(np.log10(1.5e11), np.log10(2.0e15), NFREQ).astype(np.float32)


def _grid(dust, isize, NE):
    T = dust.TMIN[isize] + (dust.TMAX[isize] - dust.TMIN[isize]) * (np.arange(NE + 1) / float(NE)) ** 2.0    # A2E_pre.py:206-207
    return np.asarray(dust.T2E(isize, T), np.float32), np.asarray(T, np.float32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(FREQ, Ef, SKABS per grain, E, T) of a case, read-only"""
    if name in STANDARD or name in OTHER:
        NFREQ, NE, isize = STANDARD[name] if name in STANDARD else OTHER[name]
        dust = a2e_pre.AnalyticDust(NSIZE=3)
        FREQ = standard_freq(NFREQ)
        E, T = _grid(dust, isize, NE)
        SK = np.asarray(dust.SKabs(isize, FREQ), np.float32)
    elif name in RANDOM:
        NFREQ, NE = RANDOM[name]
        rng = np.random.default_rng(3)
        FREQ = np.unique(np.sort(np.exp(rng.uniform(np.log(3e11), np.log(5e14), NFREQ))).astype(np.float32))
        E = np.cumsum(np.exp(rng.uniform(np.log(1e-16), np.log(3e-12), NE + 1)))
        E[3] = E[2] * (1 + 3e-6)                               # one very narrow bin
        E = np.sort(E).astype(np.float32)
        T = np.sort(rng.uniform(5.0, 900.0, NE + 1)).astype(np.float32)
        SK = (1e-12 * (FREQ / 1e13) ** 1.3).astype(np.float32)
    elif name == EMPTY:
        dust = a2e_pre.AnalyticDust(NSIZE=3)
        E, T = _grid(dust, 2, 10)
        FREQ = np.logspace(np.log10(10.0 * E[-1] / a2e_pre.PLANCK), np.log10(1000.0 * E[-1] / a2e_pre.PLANCK), 8).astype(np.float32)
        SK = np.asarray(dust.SKabs(2, FREQ), np.float32)
    else:
        raise KeyError(name)
    Ef = np.asarray(a2e_pre.PLANCK * FREQ, np.float32)
    out = (FREQ, Ef, SK, E, T)
    for a in out:
        a.setflags(write=False)
    return out


def shape(name):
    """(NFREQ, NE) of a case"""
    FREQ, _, _, E, _ = inputs(name)
    return FREQ.size, E.size - 1


def _frozen(k):
    for a in k.values():
        a.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def oracle(orc, name):
    """a2e_oracle_pre of a case, computed once and shared (read-only)"""
    from oracle.pyoracle import a2e_oracle_pre
    return _frozen(a2e_oracle_pre(orc, *inputs(name), FACTOR))


class OracleEngine:
    """stand-in for the engine in a2e_pre.make_solver: the oracle's preprocessing"""

    def __init__(self, orc):
        self.orc = orc

    def a2e_pre(self, FREQ, Ef, SKABS, E, T, FACTOR):
        from oracle.pyoracle import a2e_oracle_pre
        return a2e_oracle_pre(self.orc, FREQ, Ef, SKABS, E, T, FACTOR)


@functools.lru_cache(maxsize=None)
def oracle_solver(orc, NE):
    """make_solver(AnalyticDust(NSIZE=3), FREQ(50), NE) with the oracle's preprocessing, and the absorption fractions of its sizes"""
    from soc_amd import synth
    sol = a2e_pre.make_solver(a2e_pre.AnalyticDust(NSIZE=3), standard_freq(50), NE, OracleEngine(orc))
    return sol, [synth.a2e_absorption_fraction(sol, isize) for isize in range(3)]


@functools.lru_cache(maxsize=None)
def solver_absorptions():
    """[7, 50]: lognormal rows around 1e-3 (nu / 1e13)^-1 scaled from 1e-6 to 1e5, the last row zero"""
    FREQ = standard_freq(50)
    rng = np.random.default_rng(1)
    ABS = rng.lognormal(0, 1, (len(SOLVER_SCALES), 50)) * 1e-3 * (FREQ[None, :] / 1e13) ** -1.0
    ABS = (ABS * np.asarray(SOLVER_SCALES)[:, None]).astype(np.float32)
    ABS.setflags(write=False)
    return ABS


def windows(k, NE):
    """(l, u, length) of the pairs l < u in the order of the packed weights; length 0 where no frequency feeds the pair"""
    L1, L2 = np.asarray(k["L1"]).reshape(NE, NE), np.asarray(k["L2"]).reshape(NE, NE)
    l, u = np.triu_indices(NE, 1)
    return l, u, np.where(L1[l, u] >= 0, L2[l, u] - L1[l, u] + 1, 0)


def passes(k, NE):
    """(non-empty windows per pass (u - l - 1) // 64 of the weights kernel, the number of lower bins with a non-empty window both
    in pass 0 and in a later pass)"""
    l, u, n = windows(k, NE)
    p = (u - l - 1) // PRE_T
    counts = [int(((p == i) & (n > 0)).sum()) for i in range((NE - 2) // PRE_T + 1)]
    spans = len(set(l[(p == 0) & (n > 0)]) & set(l[(p > 0) & (n > 0)]))
    return counts, spans


def interval_passes(name):
    """per upper bin u = 1 .. NE-1 the passes the cooling kernel's loop `for (i = lane; i <= whole && i < NFREQ - 1; i += 64)` takes:
    `whole` counts the frequency intervals that end below the bin centre Eu"""
    _, Ef, _, E, _ = inputs(name)
    Eu = 0.5 * (E[1:-1].astype(np.float64) + E[2:].astype(np.float64))
    whole = np.searchsorted(Ef[1:].astype(np.float64), Eu, "left")
    return np.minimum(whole, Ef.size - 2) // PRE_T + 1


def first_difference(got, want, NE):
    """the first pair (l, u) whose weights differ in bits (the windows are those of `want`), or None"""
    l, u, n = windows(want, NE)
    off = np.cumsum(n) - n
    a, b = np.asarray(got["Iw"], np.float32).view(np.uint32), np.asarray(want["Iw"], np.float32).view(np.uint32)
    if a.size == b.size and np.array_equal(a, b):
        return None
    m = min(a.size, b.size)
    bad = np.nonzero(a[:m] != b[:m])[0]
    at = int(bad[0]) if bad.size else m
    i = int(np.searchsorted(off + n, at, side="right"))
    return (int(l[i]), int(u[i])) if i < len(l) else (NE - 2, NE - 1)
