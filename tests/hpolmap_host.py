"""Compile tests/csrc/hpolmap_host.c (the CPU restatement of the reference's PolHealpixMapping kernel) in the oracle's two
math modes and bind it.  The recipe is the one of tests/polmap_host.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from polmap_host import parents, same_bits  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "hpolmap_host.c")
DEPS = [SRC, os.path.join(HERE, "..", "soc_amd", "csrc", "soc_math.h")]

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


class HpArgs(C.Structure):
    _fields_ = [("NX", C.c_int), ("NY", C.c_int), ("NZ", C.c_int), ("LEVELS", C.c_int),
                ("OFF", _I), ("PAR", _I), ("DENS", _F), ("OPT", _F),
                ("Bx", _F), ("By", _F), ("Bz", _F), ("EMIT", _F),
                ("NSIDE", C.c_int), ("polred", C.c_int), ("threshold", C.c_int), ("interpolate", C.c_int),
                ("p00", C.c_float), ("MINLOS", C.c_float), ("MAXLOS", C.c_float), ("Y_SHEAR", C.c_float),
                ("ABS", C.c_float), ("SCA", C.c_float), ("LENGTH", C.c_float), ("INTOBS", C.c_float * 3),
                ("MAP", _F), ("NSTEPS", _I)]


_libs = {}


def load(mode):
    """mode 'libm' (what the reference's x86 build computes) or 'soc' (what the HIP kernel computes)"""
    if mode in _libs:
        return _libs[mode]
    so = os.path.join(HERE, "csrc", "libhpolmap_%s.so" % mode)
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
    lib.hp_polmap.restype = C.c_int
    lib.hp_polmap.argtypes = [C.POINTER(HpArgs)]
    _libs[mode] = lib
    return lib


def _fp(a):
    return None if a is None else a.ctypes.data_as(_F)


def polmap(mode, cloud, B, EMIT, NSIDE, INTOBS, ABS, SCA, OPT=None, polred=0, threshold=0, p0=0.2, interpolate=0, minlos=-1.0,
           maxlos=1e10, y_shear=0.0, LENGTH=1.0, PAR=None, steps=False):
    """One all-sky map of the restatement: float32 [4, 12*NSIDE^2] (and the cell steps per pixel with steps=True)"""
    lib = load(mode)
    keep = [np.ascontiguousarray(b, np.float32).ravel() for b in B]
    keep.append(np.ascontiguousarray(EMIT, np.float32).ravel())
    keep.append(np.ascontiguousarray(cloud.DENS, np.float32))
    keep.append(np.ascontiguousarray(cloud.OFF, np.int32))
    keep.append(np.ascontiguousarray(parents(cloud) if PAR is None else PAR, np.int32))
    opt = None if OPT is None else np.ascontiguousarray(OPT, np.float32).ravel()
    assert all(k.size == cloud.CELLS for k in keep[:5]) and (opt is None or opt.size == 2 * cloud.CELLS)
    npix = 12 * int(NSIDE) ** 2
    MAP = np.zeros((4, npix), np.float32)
    NST = np.zeros(npix, np.int32)
    a = HpArgs()
    a.NX, a.NY, a.NZ, a.LEVELS = cloud.NX, cloud.NY, cloud.NZ, cloud.LEVELS
    a.OFF, a.PAR, a.DENS, a.OPT = keep[5].ctypes.data_as(_I), keep[6].ctypes.data_as(_I), _fp(keep[4]), _fp(opt)
    a.Bx, a.By, a.Bz, a.EMIT = _fp(keep[0]), _fp(keep[1]), _fp(keep[2]), _fp(keep[3])
    a.NSIDE, a.polred, a.threshold, a.interpolate = int(NSIDE), int(polred), int(threshold), int(interpolate)
    a.p00, a.MINLOS, a.MAXLOS, a.Y_SHEAR = np.float32(p0), np.float32(minlos), np.float32(maxlos), np.float32(y_shear)
    a.ABS, a.SCA, a.LENGTH = np.float32(ABS), np.float32(SCA), np.float32(LENGTH)
    for k in range(3):
        a.INTOBS[k] = np.float32(INTOBS[k])
    a.MAP, a.NSTEPS = _fp(MAP), NST.ctypes.data_as(_I)
    if lib.hp_polmap(C.byref(a)) != 0:
        raise ValueError("interpolate %d on a grid of %d levels is not restated" % (interpolate, cloud.LEVELS))
    return (MAP, NST) if steps else MAP
