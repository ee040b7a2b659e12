"""Compile tests/csrc/library_host.c (the CPU restatement of the library method: LibrarySolve of kernel_soc_library.c and the
build of soc_library.py:127-217) in the oracle's two math modes and bind it."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "csrc", "library_host.c")
DEPS = [SRC, os.path.join(REPO, "soc_amd", "csrc", "soc_math.h")]

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
TABLES = ("I1", "dI1", "I2", "dI2", "X", "Y", "Z")

_libs = {}


def load(mode):
    """mode 'libm' (what the reference's x86 build computes) or 'soc' (what the HIP kernels compute)"""
    if mode in _libs:
        return _libs[mode]
    so = os.path.join(HERE, "csrc", "liblibrary_%s.so" % mode)
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        cmd = ["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-msse4.1", "-Wall",
               "-Wno-unused-function"] + (["-DSOC_ORACLE_LIBM"] if mode == "libm" else []) + [SRC, "-o", tmp, "-lm"]
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, so)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    lib = C.CDLL(so)
    lib.lh_solve.restype = None
    lib.lh_solve.argtypes = [C.c_int, C.c_int, C.c_int, _I, C.c_float, C.c_float] + [_F] * 8 + [C.c_long, _F, C.c_long, _I, _F, _I, _I,
                                                                                              C.POINTER(C.c_long)]
    lib.lh_build.restype = C.c_int
    lib.lh_build.argtypes = [C.c_int, C.c_long, _F, C.c_long, _I] + [_F] * 5 + [_I, _F, _F, _F]
    lib.lh_log10.restype = None
    lib.lh_log10.argtypes = [C.c_long, _F, _F]
    assert lib.lh_math_mode() == (1 if mode == "soc" else 0)
    _libs[mode] = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


def _i(a):
    return None if a is None else a.ctypes.data_as(_I)


def _columns(ABS, cols):
    ABS = np.ascontiguousarray(ABS, np.float32)
    assert ABS.ndim == 2
    cols = np.ascontiguousarray(np.arange(3) if cols is None else cols, np.int32)
    assert cols.size == 3 and cols.min() >= 0 and cols.max() < ABS.shape[1]
    return ABS, cols


def log10(mode, x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    load(mode).lh_log10(x.size, _f(x), _f(y))
    return y


def solve(mode, lib, ABS, cols=None, ocol=None):
    """lib: dict(N, I0, dI0, I1, dI1, I2, dI2, X, Y, Z, E[N^3, NFREQ]); ABS[n, >=3] with the reference columns cols (default
    0, 1, 2).  Returns (EMI[n, nout], ijkm[n, 4] = i, j, k, miss flag, the missed cells in ascending order)."""
    h = load(mode)
    ABS, cols = _columns(ABS, cols)
    N = int(lib["N"])
    t = [np.ascontiguousarray(lib[k], np.float32) for k in TABLES]
    E = np.ascontiguousarray(lib["E"], np.float32)
    assert [a.size for a in t] == [N, N, N * N, N * N, N ** 3, N ** 3, N ** 3] and E.shape[0] == N ** 3
    oc = None if ocol is None else np.ascontiguousarray(ocol, np.int32)
    nout = E.shape[1] if oc is None else oc.size
    n = ABS.shape[0]
    EMI = np.zeros((n, nout), np.float32)
    ijkm, miss, nmiss = np.zeros((n, 4), np.int32), np.zeros(n, np.int32), C.c_long(0)
    h.lh_solve(N, E.shape[1], nout, _i(oc), np.float32(lib["I0"]), np.float32(lib["dI0"]), *[_f(a) for a in t], _f(E), n, _f(ABS),
               ABS.shape[1], _i(cols), _f(EMI), _i(ijkm), _i(miss), C.byref(nmiss))
    return EMI, ijkm, miss[:nmiss.value].copy()


def build(mode, N, ABS, cols=None):
    """the grid and the representative cells: dict(N, I0, dI0, I1, dI1, I2, dI2, IND[N^3], X, Y, Z [N,N,N])"""
    h = load(mode)
    ABS, cols = _columns(ABS, cols)
    N = int(N)
    grid = np.zeros(2, np.float32)
    I1, dI1 = np.zeros(N, np.float32), np.zeros(N, np.float32)
    I2, dI2 = np.zeros((N, N), np.float32), np.zeros((N, N), np.float32)
    IND = np.zeros(N ** 3, np.int32)
    X, Y, Z = (np.zeros((N, N, N), np.float32) for _ in range(3))
    rc = h.lh_build(N, ABS.shape[0], _f(ABS), ABS.shape[1], _i(cols), _f(grid), _f(I1), _f(dI1), _f(I2), _f(dI2), _i(IND), _f(X), _f(Y), _f(Z))
    assert rc == 0
    return dict(N=N, I0=grid[0], dI0=grid[1], I1=I1, dI1=dI1, I2=I2, dI2=dI2, IND=IND, X=X, Y=Y, Z=Z)
