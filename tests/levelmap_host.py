"""Compile tests/csrc/levelmap_host.c (the CPU restatement of the per-level Mapping kernel of kernel_ASOC_map_H.c) in the
oracle's two math modes and bind it.  The recipe is tests/polmap_host.py's."""
import ctypes as C
import os
import subprocess

import numpy as np

from polmap_host import parents, same_bits                # noqa: F401  (same_bits: re-exported for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "levelmap_host.c")
DEPS = [SRC, os.path.join(HERE, "..", "soc_amd", "csrc", "soc_math.h")]

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


class LmArgs(C.Structure):
    _fields_ = [("NX", C.c_int), ("NY", C.c_int), ("NZ", C.c_int), ("LEVELS", C.c_int),
                ("OFF", _I), ("PAR", _I), ("DENS", _F), ("OPT", _F), ("EMIT", _F),
                ("NPIX_X", C.c_int), ("NPIX_Y", C.c_int), ("MAP_DX", C.c_float), ("ABS", C.c_float), ("SCA", C.c_float),
                ("DIR", C.c_float * 3), ("RA", C.c_float * 3), ("DE", C.c_float * 3), ("CENTRE", C.c_float * 3), ("INTOBS", C.c_float * 3),
                ("MAP", _F), ("NSTEPS", _I)]


_libs = {}


def load(mode):
    """mode 'libm' (what the reference's x86 build computes) or 'soc' (what the HIP kernel computes)"""
    if mode in _libs:
        return _libs[mode]
    so = os.path.join(HERE, "csrc", "liblevelmap_%s.so" % mode)
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        cmd = ["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-mfma",
               "-msse4.1", "-Wall", "-Wno-unused-function"] + (["-DPM_LIBM"] if mode == "libm" else []) + [SRC, "-o", tmp, "-lm"]
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, so)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    lib = C.CDLL(so)
    lib.lm_levelmap.restype = C.c_int
    lib.lm_levelmap.argtypes = [C.POINTER(LmArgs)]
    _libs[mode] = lib
    return lib


def _fp(a):
    return None if a is None else a.ctypes.data_as(_F)


def levelmap(mode, cloud, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, INTOBS=None, OPT=None, PAR=None, steps=False):
    """The images of one view: float32 [LEVELS, NPIX.y, NPIX.x] (and the cell steps per pixel with steps=True)"""
    lib = load(mode)
    keep = [np.ascontiguousarray(EMIT, np.float32).ravel(), np.ascontiguousarray(cloud.DENS, np.float32),
            np.ascontiguousarray(cloud.OFF, np.int32), np.ascontiguousarray(parents(cloud) if PAR is None else PAR, np.int32)]
    opt = None if OPT is None else np.ascontiguousarray(OPT, np.float32).ravel()
    assert keep[0].size == cloud.CELLS and keep[1].size == cloud.CELLS and (opt is None or opt.size == 2 * cloud.CELLS)
    nx, ny = int(NPIX[0]), int(NPIX[1])
    MAP = np.zeros((cloud.LEVELS, ny, nx), np.float32)
    NST = np.zeros((ny, nx), np.int32)
    a = LmArgs()
    a.NX, a.NY, a.NZ, a.LEVELS = cloud.NX, cloud.NY, cloud.NZ, cloud.LEVELS
    a.OFF, a.PAR, a.DENS, a.OPT, a.EMIT = keep[2].ctypes.data_as(_I), keep[3].ctypes.data_as(_I), _fp(keep[1]), _fp(opt), _fp(keep[0])
    a.NPIX_X, a.NPIX_Y = nx, ny
    a.MAP_DX, a.ABS, a.SCA = np.float32(MAP_DX), np.float32(ABS), np.float32(SCA)
    inside = INTOBS is not None and INTOBS[0] > -1e10
    zero = (0.0, 0.0, 0.0)
    for dst, src in ((a.DIR, DIR), (a.RA, RA), (a.DE, DE), (a.CENTRE, CENTRE), (a.INTOBS, INTOBS if inside else (-1.0e12, 0.0, 0.0))):
        for k in range(3):
            dst[k] = np.float32((zero if src is None else src)[k])
    a.MAP, a.NSTEPS = _fp(MAP), NST.ctypes.data_as(_I)
    if lib.lm_levelmap(C.byref(a)) != 0:
        raise ValueError("%d levels" % cloud.LEVELS)
    return (MAP, NST) if steps else MAP
