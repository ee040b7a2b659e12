"""Inputs of the DoSolve launch-shape tests (tests/test_a2e_shapes.py on the CPU, tests/test_gpu_a2e_shapes.py on the GPU) and a
finder for them: a numpy fp32 restatement of the heating sums, the suffix sums and the forward substitution of
oracle/a2e_oracle.c that says at which rows a cell rescales.  The finder picks test inputs; it is no second oracle (its first
test holds it to the oracle's bits, so that its row lists can be trusted)."""
import functools

import numpy as np

from soc_amd import synth

# NE -> (cells per workgroup, threads per workgroup) at NFREQ = 50, as the launcher chooses today.  The GPU test asserts every
# entry through Engine.a2e_launch_shape(): after a retuning of the rule it names the sizes to move.
TABLE = {
    3: (4, 256),                   # smallest accepted size: NE - 3 = 0 columns in the suffix sums
    65: (4, 256), 70: (4, 256),    # 256 threads with a second row block of 1 or 6 rows
    71: (4, 1024),                 # first size with 1024 threads
    100: (4, 1024),                # second block partly filled
    129: (4, 1024),                # a third block of one row
    142: (4, 1024), 143: (2, 1024),    # last C = 4, first C = 2
    193: (2, 1024),                # a fourth block of one row
    201: (2, 1024), 202: (1, 1024),    # last C = 2, first C = 1
    256: (1, 1024),                # the size README quotes
    280: (1, 1024),                # largest accepted: five blocks, the last of 24 rows
}
# (NE, NFREQ) -> C: 2 (smallest), 64 and 65 (the emission loop's one full and one one-lane round), 130
NFREQ_EDGES = {(ne, nf): c for ne, c in ((143, 2), (64, 4)) for nf in (2, 64, 65, 130)}
OVERFLOW_NE = 280                  # the case "overflow": rows base * 10**k, k = 11 .. 16, whose oracle output may be non-finite
OVERFLOW_K = tuple(range(11, 17))
K_TOP = 10                         # every row up to here is finite and non-negative in the oracle at every size of TABLE
K_TOP_AT = {(143, 130): 9, (280, 810): 9}      # (NE, NFREQ) -> top of the grid where base * 10**10 (more frequencies, more absorbed
                                   # energy) is not finite in the oracle, both at size 1; test_a2e_shapes.py shows that 10 fails there


@functools.lru_cache(maxsize=None)
def solver(NE, NFREQ=50):
    sol = synth.synth_solver(NFREQ=NFREQ, NE=NE, NSIZE=2, seed=5)
    return sol, [synth.a2e_absorption_fraction(sol, isize) for isize in range(2)]


def base_row(NFREQ):
    return np.random.default_rng(4).lognormal(0, 2, NFREQ) * 1e-2


def k_grid(C, top=K_TOP):
    """the exponents k of the rows base * 10**k of a case with 4*C + 3 cells: -14 .. top, as many as leave room for the
    all-zero row and at least one lognormal row"""
    return tuple(int(k) for k in np.round(np.linspace(-14, top, {4: 13, 2: 8, 1: 5}[C])))


@functools.lru_cache(maxsize=None)
def absorptions(NE, NFREQ, C):
    """[4*C + 3, NFREQ] (the last workgroup holds 3 of 4 or 1 of 2 cells): the k grid, one all-zero row, the rest lognormal as in
    make_golden.a2e_case.  Returns (ABS, ks): ks[c] is the exponent of cell c, None for the other rows."""
    sol, _ = solver(NE, NFREQ)
    n, ks = 4 * C + 3, k_grid(C, K_TOP_AT.get((NE, NFREQ), K_TOP))
    rng = np.random.default_rng(1)
    ABS = (rng.lognormal(0, 1, (n, NFREQ)) * 1e-3 * (sol["FREQ"][None, :] / 1e13) ** -1.0).astype(np.float32)
    with np.errstate(over="ignore"):
        for c, k in enumerate(ks):
            ABS[c] = (base_row(NFREQ) * 10.0 ** k).astype(np.float32)
    ABS[len(ks)] = 0.0
    ABS.setflags(write=False)
    return ABS, ks + (None,) * (n - len(ks))


RESIDENT = {160: 2, 256: 1}        # NE -> C of the cases of the resident (accumulate) path


@functools.lru_cache(maxsize=None)
def resident_absorptions(NE):
    """8*C + 5 cells: the case's own rows and the first 4*C + 2 of the 19 rows of a C = 4 case (a finer k grid)"""
    C = RESIDENT[NE]
    ABS = np.concatenate([absorptions(NE, 50, C)[0], absorptions(NE, 50, 4)[0][:4 * C + 2]])
    ABS.setflags(write=False)
    return ABS


@functools.lru_cache(maxsize=None)
def overflow_absorptions():
    ABS = np.stack([(base_row(50) * 10.0 ** k).astype(np.float32) for k in OVERFLOW_K])
    ABS.setflags(write=False)
    return ABS


@functools.lru_cache(maxsize=None)
def oracle_emission(orc, NE, NFREQ, C, isize, overflow=False):
    """the oracle's emission for one case and size, computed once and shared (read-only)"""
    from oracle.pyoracle import a2e_oracle_dosolve
    sol, AF = solver(NE, NFREQ)
    ABS = overflow_absorptions() if overflow else absorptions(NE, NFREQ, C)[0]
    e = a2e_oracle_dosolve(orc, NE, NFREQ, sol["sizes"][isize], AF[isize], ABS)
    e.setflags(write=False)
    return e


def find_rows(NE, NFREQ, size, AF, ABS):
    """oracle/a2e_oracle.c:44-67 in numpy fp32, the cells side by side, every sum in the oracle's order (one fp32 multiplication,
    one fp32 addition per term).  Returns (rows, XLraw, XL): rows[c] the sorted rows j at which cell c rescales, XLraw [cells, NE]
    as the forward substitution leaves it, XL normalised."""
    f32 = np.float32
    ABS, AF = np.asarray(ABS, f32), np.asarray(AF, f32)
    Iw, Tdown = np.asarray(size["Iw"], f32), np.asarray(size["Tdown"], f32)
    L1, L2 = np.asarray(size["L1"]).reshape(NE, NE), np.asarray(size["L2"]).reshape(NE, NE)
    n = ABS.shape[0]
    lo, up = np.triu_indices(NE, 1)                          # the pairs in the oracle's (l, u) loop order
    first, cnt = L1[lo, up].astype(np.int64), np.maximum(L2[lo, up] - L1[lo, up] + 1, 0).astype(np.int64)
    off = np.cumsum(cnt) - cnt
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        I = np.zeros((n, len(lo)), f32)
        for t in range(int(cnt.max()) if len(cnt) else 0):
            m = np.nonzero(t < cnt)[0]
            i = first[m] + t
            I[:, m] += (ABS[:, i] * Iw[off[m] + t][None, :]) * AF[i][None, :]
        L = np.zeros((n, NE, NE), f32)                       # L[c, u, l]
        L[:, up, lo] = np.maximum(I, f32(0.0))
        for j in range(NE - 3, 0, -1):
            L[:, j, :j] += L[:, j + 1, :j]
        XL = np.zeros((n, NE), f32)
        XL[:, 0] = f32(1.0e-20)
        rows = [[] for _ in range(n)]
        for j in range(1, NE):
            s = np.zeros(n, f32)
            for i in range(j):
                s += L[:, j, i] * XL[:, i]
            s = np.maximum(s / (Tdown[j] + f32(1.0e-30)), f32(0.0))      # (fmaxf(NaN, 0) = 0 as well)
            s[np.isnan(s)] = 0.0
            XL[:, j] = s
            for c in np.nonzero(s > f32(1.0e20))[0]:
                XL[c, :j + 1] *= f32(1.0e-20)
                rows[c].append(j)
        raw = XL.copy()
        nrm = np.zeros(n, f32)
        for i in range(NE):
            nrm += XL[:, i]
        XL = XL * (f32(1.0) / nrm)[:, None]
    return rows, raw, XL


def emission(NE, NFREQ, size, XL):
    """oracle/a2e_oracle.c:72-76 in numpy fp32 from the normalised XL of find_rows"""
    EA, Ibeg = np.asarray(size["EA"], np.float32).reshape(NFREQ, NE), np.asarray(size["Ibeg"])
    out = np.zeros((XL.shape[0], NFREQ), np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i in range(NE):
            m = np.nonzero(Ibeg <= i)[0]
            out[:, m] += EA[m, i][None, :] * XL[:, i:i + 1]
    return out


@functools.lru_cache(maxsize=None)
def case_rows(NE, NFREQ, C, isize, overflow=False):
    sol, AF = solver(NE, NFREQ)
    ABS = overflow_absorptions() if overflow else absorptions(NE, NFREQ, C)[0]
    return find_rows(NE, NFREQ, sol["sizes"][isize], AF[isize], ABS)
