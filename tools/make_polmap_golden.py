#!/usr/bin/env python3
"""Record tests/golden/polmaps.npz: what the reference's PolMapping kernel (kernel_ASOC_map.c, compiled unmodified for
x86-64 where it lies) gives for the cases of tests/polmap_cases.py.

    python tools/make_polmap_golden.py [reference directory]

Run by hand on a machine that has the reference; nothing it compiles is kept (a temporary directory) and no test
imports it.  The compiler recipe is oracle/build.py's build_ref_map with POLSTAT, POLRED, POL_RHO_WEIGHT,
LEVEL_THRESHOLD and p00 substituted in its -D list (ASOC.py:344-362); the driver is tools/ref_polmap.cpp.
"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import build as obuild                     # noqa: E402
import polmap_cases as pc                              # noqa: E402
import polmap_host                                     # noqa: E402

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


class Args(C.Structure):
    _fields_ = [("NPIX_X", C.c_int), ("NPIX_Y", C.c_int), ("MAP_DX", C.c_float), ("ABS", C.c_float), ("SCA", C.c_float),
                ("DIR", C.c_float * 4), ("RA", C.c_float * 4), ("DE", C.c_float * 4), ("CENTRE", C.c_float * 4),
                ("LCELLS", _I), ("OFF", _I), ("PAR", _I),
                ("DENS", _F), ("EMIT", _F), ("OPT", _F), ("Bx", _F), ("By", _F), ("Bz", _F), ("MAP", _F)]


def build(tmp, reference, tag, cloud, WITH_ABU, POLSTAT, POLRED, POL_RHO_WEIGHT, LEVEL_THRESHOLD, p0):
    defs = obuild.ref_defs(NX=cloud.NX, NY=cloud.NY, NZ=cloud.NZ, LEVELS=cloud.LEVELS, CELLS=cloud.CELLS, WITH_ABU=WITH_ABU,
                           LEVEL_THRESHOLD=LEVEL_THRESHOLD, GL=pc.GL)
    sub = {"POLSTAT": POLSTAT, "POLRED": POLRED, "POL_RHO_WEIGHT": POL_RHO_WEIGHT, "p00": "%.4ff" % p0, "NSIDE": pc.NPIX[0]}
    defs = [d for d in defs if d[2:].split("=")[0] not in sub] + ["-D%s=%s" % kv for kv in sub.items()]
    ksrc = os.path.join(reference, "kernel_ASOC_map.c")
    kobj, dobj, so = (os.path.join(tmp, "%s.%s" % (tag, e)) for e in ("k.o", "d.o", "so"))
    common = ["-O2", "-fPIC", "-ffp-contract=off", "-target", "x86_64-unknown-linux-gnu"]
    subprocess.check_call([obuild.CLANG, "-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-ftrivial-auto-var-init=zero",
                           "-w", "-I", reference] + common + defs + ["-c", ksrc, "-o", kobj])
    subprocess.check_call([obuild.CLANG + "++", "-std=c++17", "-w"] + common + ["-c", os.path.join(REPO, "tools", "ref_polmap.cpp"), "-o", dobj])
    subprocess.check_call([obuild.CLANG + "++", "-shared", "-Wl,-z,defs", kobj, dobj, "-lm", "-lpthread", "-o", so])
    lib = C.CDLL(so)
    lib.ref_polmap.argtypes = [C.POINTER(Args)]
    return lib


def main(argv):
    reference = argv[1] if len(argv) > 1 else obuild.REFERENCE
    ODIR, RA, DE = pc.views()
    out = dict(ODIR=ODIR, RA=RA, DE=DE, NPIX=np.asarray(pc.NPIX, np.int32),
               meta=np.asarray(json.dumps(dict(cases=pc.CASES, views=pc.VIEWS, GL=pc.GL, p0=pc.P0))))
    with tempfile.TemporaryDirectory() as tmp:
        for name, (mname, polstat, polred, rhow, thr) in pc.CASES.items():
            m = pc.model(mname)
            c = m["cloud"]
            lib = build(tmp, reference, name, c, int(m["OPT"] is not None), polstat, polred, rhow, thr, pc.P0)
            PAR = polmap_host.parents(c)
            keep = [np.ascontiguousarray(c.LCELLS, np.int32), np.ascontiguousarray(c.OFF, np.int32), PAR,
                    np.ascontiguousarray(c.DENS, np.float32), m["EMIT"]] + list(m["B"])
            opt = None if m["OPT"] is None else np.ascontiguousarray(m["OPT"], np.float32)
            maps = np.zeros((len(pc.VIEWS), 4, pc.NPIX[1], pc.NPIX[0]), np.float32)
            for idir in range(len(pc.VIEWS)):
                a = Args()
                a.NPIX_X, a.NPIX_Y, a.MAP_DX, a.ABS, a.SCA = pc.NPIX[0], pc.NPIX[1], m["MAP_DX"], m["ABS"], m["SCA"]
                cen = pc.centre(c)
                for k in range(3):
                    a.DIR[k], a.RA[k], a.DE[k], a.CENTRE[k] = ODIR[idir, k], RA[idir, k], DE[idir, k], cen[k]
                a.LCELLS, a.OFF, a.PAR = (x.ctypes.data_as(_I) for x in keep[:3])
                a.DENS, a.EMIT = keep[3].ctypes.data_as(_F), keep[4].ctypes.data_as(_F)
                a.Bx, a.By, a.Bz = (x.ctypes.data_as(_F) for x in keep[5:8])
                a.OPT = None if opt is None else opt.ctypes.data_as(_F)
                one = np.zeros(4 * pc.NPIX[0] * pc.NPIX[1], np.float32)
                a.MAP = one.ctypes.data_as(_F)
                lib.ref_polmap(C.byref(a))
                maps[idir] = one.reshape(4, pc.NPIX[1], pc.NPIX[0])
            out["map_" + name] = maps
            out["fp_" + mname] = pc.fingerprint(m)
            print("%-16s  NaN pixels %4d   |sum| %.6e" % (name, int(np.isnan(maps).sum()), float(np.nansum(np.abs(maps)))))
    path = os.path.join(REPO, "tests", "golden", "polmaps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
