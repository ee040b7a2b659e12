"""Inputs of the library-method tests, regenerated from seeded numpy.random.Generator(PCG64): synthetic libraries with cells to
look up (tests/golden/library.npz holds what the reference's LibrarySolve gives for them), and absorptions to build a grid from.
Nothing here depends on a math mode: the values are drawn in double and stored as float32."""
import numpy as np

SEED = 20240611


def _rng(tag):
    return np.random.Generator(np.random.PCG64([SEED, sum(ord(ch) * (i + 1) for i, ch in enumerate(tag))]))


def _library(rng, N, NFREQ, empty=0.0, spread=0.5):
    """a grid with its own origin and width per i and per (i, j), the representative of bin (i, j, k) within `spread` of the bin
    centre, a positive emission row per bin; a fraction `empty` of the bins without one (1e32 rows)"""
    I0, dI0 = np.float32(-13.0 + rng.random()), np.float32(0.15 + 0.2 * rng.random())
    I1 = (-12.0 + rng.random(N)).astype(np.float32)
    dI1 = (0.1 + 0.2 * rng.random(N)).astype(np.float32)
    I2 = (-11.0 + rng.random((N, N))).astype(np.float32)
    dI2 = (0.1 + 0.2 * rng.random((N, N))).astype(np.float32)
    idx = np.indices((N, N, N)).astype(np.float64)
    X, Y, Z = ((idx[a] + spread * (2.0 * rng.random((N, N, N)) - 1.0)).astype(np.float32) for a in range(3))
    E = (10.0 ** (-20.0 + 10.0 * rng.random((N ** 3, NFREQ)))).astype(np.float32)
    if empty > 0.0:
        E[rng.random(N ** 3) < empty, :] = 1.0e32
    return dict(N=N, I0=I0, dI0=dI0, I1=I1, dI1=dI1, I2=I2, dI2=dI2, X=X, Y=Y, Z=Z, E=E)


def _cells(lib, x, y, z):
    """absorptions that land near the coordinates (x, y, z) of the library's grid (the bins are taken from the rounded
    coordinates in double; a cell on a half-integer may land on either side once the float arithmetic has spoken)"""
    N = lib["N"]
    i = np.clip(np.rint(x).astype(int), 0, N - 1)
    j = np.clip(np.rint(y).astype(int), 0, N - 1)
    a0 = 10.0 ** (float(lib["I0"]) + x * float(lib["dI0"]))
    a1 = 10.0 ** (lib["I1"][i].astype(np.float64) + y * lib["dI1"][i])
    a2 = 10.0 ** (lib["I2"][i, j].astype(np.float64) + z * lib["dI2"][i, j])
    return np.stack([a0, a1, a2], axis=1).astype(np.float32)


def _uniform(rng, n, lo, hi):
    return lo + (hi - lo) * rng.random(n)


# name: (N, NFREQ, n, kind)
SOLVE = {
    "n2_f1_c1": (2, 1, 1, "mixed"),
    "n3_f7_c63": (3, 7, 63, "mixed"),
    "n30_f65_c64": (30, 65, 64, "mixed"),
    "n3_f65_c65": (3, 65, 65, "mixed"),
    "n30_f7_c1000": (30, 7, 1000, "mixed"),
    "ocol": (3, 7, 1000, "mixed"),
    "all_miss": (3, 7, 65, "all_miss"),
    "no_miss": (30, 7, 1000, "no_miss"),
    "clamped": (3, 7, 1000, "clamped"),
    "empty_bins": (3, 7, 1000, "empty"),
    "halves": (3, 1, 64, "halves"),
}


def solve_case(name):
    """dict(lib, ABS3[n, 3], ocol or None)"""
    N, NFREQ, n, kind = SOLVE[name]
    rng = _rng("solve_" + name)
    ocol = None
    if kind == "no_miss":                                      # cells and representatives both within 0.3 of a bin centre
        lib = _library(rng, N, NFREQ, spread=0.3)
        x, y, z = (rng.integers(0, N, n) + _uniform(rng, n, -0.3, 0.3) for _ in range(3))
    elif kind == "all_miss":                                   # every representative two bins away on axis 1
        lib = _library(rng, N, NFREQ, spread=0.3)
        lib["Y"] = (lib["Y"] + np.float32(2.0)).astype(np.float32)
        x, y, z = (rng.integers(0, N, n) + _uniform(rng, n, -0.3, 0.3) for _ in range(3))
    elif kind == "clamped":                                    # every cell beyond the first or the last bin of one axis at least
        lib = _library(rng, N, NFREQ)
        x, y, z = (_uniform(rng, n, -0.4, N - 0.6) for _ in range(3))
        out = np.where(rng.random(n) < 0.5, _uniform(rng, n, -1.6, -0.6), _uniform(rng, n, N - 0.4, N + 0.6))
        axis = rng.integers(0, 3, n)
        x, y, z = np.where(axis == 0, out, x), np.where(axis == 1, out, y), np.where(axis == 2, out, z)
        every = rng.random(n) < 0.2                            # and some beyond on all three
        x, y, z = (np.where(every, out, v) for v in (x, y, z))
    elif kind == "empty":                                      # four bins in ten hold no emission
        lib = _library(rng, N, NFREQ, empty=0.4, spread=0.3)
        x, y, z = (rng.integers(0, N, n) + _uniform(rng, n, -0.3, 0.3) for _ in range(3))
    elif kind == "halves":
        # absorption 1 has the logarithm 0 in every math mode; with I = -0.5 * dI and dI a power of two the coordinate is 0.5
        # exactly: the look-up rounds it away from zero, to bin 1 (halves to even would give bin 0)
        lib = _library(rng, N, NFREQ, spread=0.0)
        lib["I0"], lib["dI0"] = np.float32(-0.25), np.float32(0.5)
        lib["I1"][:], lib["dI1"][:] = np.float32(-0.125), np.float32(0.25)
        lib["I2"][:], lib["dI2"][:] = np.float32(-0.5), np.float32(1.0)
        ABS3 = np.ones((n, 3), np.float32)
        ABS3[1::2, 1] = np.float32(10.0 ** (-0.125 + 0.25 * 1.2))             # every other cell off the half on axis 1
        return dict(lib=lib, ABS3=ABS3, ocol=None)
    else:
        lib = _library(rng, N, NFREQ, empty=0.1)
        x, y, z = (_uniform(rng, n, -2.0, N + 1.0) for _ in range(3))
    ABS3 = _cells(lib, x, y, z)
    if kind == "mixed" and n >= 63:                            # values the clamp of the look-up catches
        ABS3[5, 0], ABS3[6, 1], ABS3[7, 2], ABS3[8, :] = 0.0, 1.0e20, 0.0, 1.0e-35
    if name == "ocol":
        ocol = np.asarray([5, 0, 6, 2], np.int32)
    return dict(lib=lib, ABS3=ABS3, ocol=ocol)


def _cloud(rng, cells, lo=-14.0, hi=-9.0):
    """correlated absorptions over (hi - lo) decades: what a model's cells look like on the three axes"""
    u = _uniform(rng, cells, lo, hi)
    v = u + 0.8 + 0.4 * rng.standard_normal(cells)
    w = v + 0.5 + 0.3 * rng.standard_normal(cells)
    return (10.0 ** np.stack([u, v, w], axis=1)).astype(np.float32)


# name: (N, cells)
BUILD = {
    "one_cell": (4, 1),
    "two_cells": (4, 2),                  # far apart: every window of axis 2 holds one cell (the `< 2` rule), all of I2 is filled in
    "c70": (3, 70),
    "c5000": (6, 5000),
    "c5000_n30": (30, 5000),
    "two_clumps": (8, 400),               # the windows of axis 0 between the clumps are empty
    "clipped": (5, 300),                  # absorptions of 0 and above 1
    "twins": (4, 200),                    # identical cells: the lower index represents the bin
    "c300000": (30, 300000),
    "halves": (4, 8),                     # a planted cell at x = 2.5 and y = 2.5 exactly: the build rounds to even, into bin (2, 2, .)
}

# The planted case, found by a search over float32 values and stored as bit patterns.  In libm's log10f and in soc_log10f alike:
# log10(HALF_LO0) and log10(1) = 0 span axis 0 so that (log10(HALF_X) - I0) / dI0 is 2.5 exactly; HALF_IN2 lies in window 2 of
# axis 0; log10(HALF_LO1) and 0 span axis 1 of that window so that (log10(HALF_Y) - I1[2]) / dI1[2] is 2.5 exactly.
HALF_LO0, HALF_X, HALF_IN2, HALF_LO1, HALF_Y = (np.asarray([u], np.uint32).view(np.float32)[0]
                                                for u in (730640676, 1024747257, 961060655, 772007244, 1029862131))
HALF_CELL = 7                             # the planted cell's index


def build_case(name):
    """dict(N, ABS3[cells, 3])"""
    N, cells = BUILD[name]
    rng = _rng("build_" + name)
    if name == "halves":
        # four cells at the minimum of axis 0: two of them share window (0, 2) and give axis 2 its only grid, which the raster fill
        # hands to every later (i, j); one cell at the maximum; two in window 2 of axis 0 that span its axis 1; the planted cell
        ABS3 = np.asarray([[HALF_LO0, 1e-5, 1e-11], [HALF_LO0, 1e-5, 1e-3], [HALF_LO0, 1e-8, 1e-6], [HALF_LO0, 1e-4, 1e-6],
                           [1.0, 1e-5, 1e-6], [HALF_IN2, 1.0, 1e-6], [HALF_IN2, HALF_LO1, 1e-6], [HALF_X, HALF_Y, 1e-6]], np.float32)
        return dict(N=N, ABS3=ABS3)
    if name == "two_cells":
        ABS3 = np.asarray([[1e-14, 1e-13, 1e-12], [1e-8, 3e-8, 2e-7]], np.float32)
    elif name == "two_clumps":
        ABS3 = np.concatenate([_cloud(rng, cells // 2, -14.0, -13.5), _cloud(rng, cells - cells // 2, -9.5, -9.0)])
    else:
        ABS3 = _cloud(rng, cells)
    if name == "clipped":
        ABS3[::7, 0] = 0.0
        ABS3[3::11, 1] = 0.0
        ABS3[5::13, 2] = 25.0
        ABS3[2::17, :] = 3.0
    if name == "twins":
        ABS3[100:200] = ABS3[0:100]
    return dict(N=N, ABS3=ABS3)


def meta():
    """what tests/golden/library.npz was recorded for"""
    return "library v1 seed %d solve %s" % (SEED, " ".join("%s:%d:%d:%d:%s" % ((k,) + SOLVE[k]) for k in sorted(SOLVE)))
