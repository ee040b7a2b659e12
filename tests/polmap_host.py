"""Compile tests/csrc/polmap_host.c (the CPU restatement of the reference's PolMapping kernels) in the oracle's two math
modes and bind it.  The recipe is the one of oracle/build.py's build_oracle."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "polmap_host.c")
DEPS = [SRC, os.path.join(HERE, "..", "soc_amd", "csrc", "soc_math.h")]

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


class PmArgs(C.Structure):
    _fields_ = [("NX", C.c_int), ("NY", C.c_int), ("NZ", C.c_int), ("LEVELS", C.c_int),
                ("OFF", _I), ("PAR", _I), ("DENS", _F), ("OPT", _F),
                ("Bx", _F), ("By", _F), ("Bz", _F), ("EMIT", _F),
                ("polstat", C.c_int), ("polred", C.c_int), ("rho_weight", C.c_int), ("threshold", C.c_int),
                ("p00", C.c_float), ("NPIX_X", C.c_int), ("NPIX_Y", C.c_int),
                ("MAP_DX", C.c_float), ("ABS", C.c_float), ("SCA", C.c_float), ("LENGTH", C.c_float),
                ("DIR", C.c_float * 3), ("RA", C.c_float * 3), ("DE", C.c_float * 3), ("CENTRE", C.c_float * 3),
                ("MAP", _F), ("NSTEPS", _I)]


_libs = {}


def load(mode):
    """mode 'libm' (what the reference's x86 build computes) or 'soc' (what the HIP kernel computes)"""
    if mode in _libs:
        return _libs[mode]
    so = os.path.join(HERE, "csrc", "libpolmap_%s.so" % mode)
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
    lib.pm_polmap.restype = C.c_int
    lib.pm_polmap.argtypes = [C.POINTER(PmArgs)]
    lib.pm_fmod.argtypes = [_F, _F, _F, C.c_long]
    _libs[mode] = lib
    return lib


def parents(cloud):
    """PAR[CELLS - NX*NY*NZ]: for every cell above the root grid the index of its parent within the parent's level"""
    c = cloud
    PAR = np.zeros(max(1, c.CELLS - c.NX * c.NY * c.NZ), np.int32)
    for l in range(c.LEVELS - 1):
        d = c.DENS[c.OFF[l]:c.OFF[l] + c.LCELLS[l]]
        p = np.nonzero(d <= 0.0)[0]
        first = (-d[p]).view(np.int32).astype(np.int64) + int(c.OFF[l + 1]) - c.NX * c.NY * c.NZ
        for k in range(8):
            PAR[first + k] = p
    return PAR


def _fp(a):
    return None if a is None else a.ctypes.data_as(_F)


def polmap(mode, cloud, B, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, OPT=None, polstat=0, polred=0, rho_weight=0,
           threshold=0, p0=0.2, LENGTH=1.0, PAR=None, steps=False):
    """One map of the restatement: float32 [4, NPIX.y, NPIX.x] (and the cell steps per pixel with steps=True)"""
    lib = load(mode)
    keep = [np.ascontiguousarray(b, np.float32).ravel() for b in B]
    keep.append(np.ascontiguousarray(EMIT, np.float32).ravel())
    keep.append(np.ascontiguousarray(cloud.DENS, np.float32))
    keep.append(np.ascontiguousarray(cloud.OFF, np.int32))
    keep.append(np.ascontiguousarray(parents(cloud) if PAR is None else PAR, np.int32))
    opt = None if OPT is None else np.ascontiguousarray(OPT, np.float32).ravel()
    assert all(k.size == cloud.CELLS for k in keep[:5]) and (opt is None or opt.size == 2 * cloud.CELLS)
    nx, ny = int(NPIX[0]), int(NPIX[1])
    MAP = np.zeros((4, ny, nx), np.float32)
    NST = np.zeros((ny, nx), np.int32)
    a = PmArgs()
    a.NX, a.NY, a.NZ, a.LEVELS = cloud.NX, cloud.NY, cloud.NZ, cloud.LEVELS
    a.OFF, a.PAR, a.DENS, a.OPT = keep[5].ctypes.data_as(_I), keep[6].ctypes.data_as(_I), _fp(keep[4]), _fp(opt)
    a.Bx, a.By, a.Bz, a.EMIT = _fp(keep[0]), _fp(keep[1]), _fp(keep[2]), _fp(keep[3])
    a.polstat, a.polred, a.rho_weight, a.threshold = int(polstat), int(polred), int(rho_weight), int(threshold)
    a.p00, a.NPIX_X, a.NPIX_Y = np.float32(p0), nx, ny
    a.MAP_DX, a.ABS, a.SCA, a.LENGTH = np.float32(MAP_DX), np.float32(ABS), np.float32(SCA), np.float32(LENGTH)
    for dst, src in ((a.DIR, DIR), (a.RA, RA), (a.DE, DE), (a.CENTRE, CENTRE)):
        for k in range(3):
            dst[k] = np.float32(src[k])
    a.MAP, a.NSTEPS = _fp(MAP), NST.ctypes.data_as(_I)
    if lib.pm_polmap(C.byref(a)) != 0:
        raise ValueError("polstat %d is not restated" % polstat)
    return (MAP, NST) if steps else MAP


def fmod(mode, x, y):
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    r = np.zeros_like(x)
    load(mode).pm_fmod(_fp(x), _fp(y), _fp(r), x.size)
    return r


def same_bits(a, b):
    """equal bit for bit, NaNs compared by position (every element takes part)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))
