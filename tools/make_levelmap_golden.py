#!/usr/bin/env python3
"""Record tests/golden/levelmaps.npz: what the per-level Mapping kernel of the reference (kernel_ASOC_map_H.c, `mapping nx ny dx
999`; compiled unmodified for x86-64 where it lies) gives for the cases of tests/levelmap_cases.py.

    python tools/make_levelmap_golden.py [reference directory]

Run by hand on a machine that has the reference; nothing it compiles is kept (a temporary directory) and no test imports
it.  The compiler recipe is tools/make_hpolmap_golden.py's: the -D list of oracle.build.ref_defs (ASOC.py:344-362, POLSTAT = 0)
with NSIDE = NPIX.x (ASOC.py:3330); the driver is tools/ref_levelmap.cpp.  The models with abundances are built with
-D WITH_ABU=1 as ASOC.py does, and get their OPT array -- the kernel does not read it (its per-cell line is under "#ifdef
USE_ABU", which nothing defines), so their maps are those of the scalar ABS + SCA.

Before it calls the reference the script asks the CPU restatement's step counter whether every ray of the case ends (on a
hierarchy that file's walk can cycle without end).  Per case it prints how many pixels are non-zero on each level; every
level of oct8 must have some, and the cases named *_wide must miss the model on the whole outer ring of pixels.
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
import levelmap_cases as lc                            # noqa: E402
import levelmap_host                                   # noqa: E402
import polmap_host                                     # noqa: E402

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


class Args(C.Structure):
    _fields_ = [("NPIX_X", C.c_int), ("NPIX_Y", C.c_int), ("MAP_DX", C.c_float), ("ABS", C.c_float), ("SCA", C.c_float),
                ("DIR", C.c_float * 4), ("RA", C.c_float * 4), ("DE", C.c_float * 4), ("CENTRE", C.c_float * 4), ("INTOBS", C.c_float * 4),
                ("LCELLS", _I), ("OFF", _I), ("PAR", _I), ("DENS", _F), ("EMIT", _F), ("OPT", _F), ("MAP", _F)]


_built = {}


def build(tmp, reference, mname, cloud, WITH_ABU):
    if mname in _built:
        return _built[mname]
    defs = obuild.ref_defs(NX=cloud.NX, NY=cloud.NY, NZ=cloud.NZ, LEVELS=cloud.LEVELS, CELLS=cloud.CELLS, WITH_ABU=WITH_ABU, GL=lc.GL)
    defs = [d for d in defs if not d.startswith("-DNSIDE=")] + ["-DNSIDE=%d" % lc.NPIX[0]]
    ksrc = os.path.join(reference, "kernel_ASOC_map_H.c")
    kobj, dobj, so = (os.path.join(tmp, "%s.%s" % (mname, e)) for e in ("k.o", "d.o", "so"))
    common = ["-O2", "-fPIC", "-ffp-contract=off", "-target", "x86_64-unknown-linux-gnu"]
    subprocess.check_call([obuild.CLANG, "-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-ftrivial-auto-var-init=zero",
                           "-w", "-I", reference] + common + defs + ["-c", ksrc, "-o", kobj])
    subprocess.check_call([obuild.CLANG + "++", "-std=c++17", "-w"] + common + ["-c", os.path.join(REPO, "tools", "ref_levelmap.cpp"), "-o", dobj])
    subprocess.check_call([obuild.CLANG + "++", "-shared", "-Wl,-z,defs", kobj, dobj, "-lm", "-lpthread", "-o", so])
    lib = C.CDLL(so)
    lib.ref_levelmap.argtypes = [C.POINTER(Args)]
    _built[mname] = lib
    return lib


def main(argv):
    reference = argv[1] if len(argv) > 1 else obuild.REFERENCE
    ODIR, RA, DE = lc.views()
    nx, ny = lc.NPIX
    out = dict(NPIX=np.asarray(lc.NPIX, np.int32), ODIR=ODIR, RA=RA, DE=DE, meta=np.asarray(json.dumps(dict(cases=lc.CASES, GL=lc.GL))))
    with tempfile.TemporaryDirectory() as tmp:
        for name, k in lc.CASES.items():
            m, kw = lc.case_args(name, ODIR, RA, DE)
            c = m["cloud"]
            # the reference has no step limit, and on a hierarchy its walk can cycle: ask the restatement's counter first
            _, NST = levelmap_host.levelmap("libm", c, m["EMIT"], steps=True, **kw)
            assert NST.max() < 1 << 15, "%s: %d rays would not end in the reference" % (name, int((NST >= 1 << 15).sum()))
            lib = build(tmp, reference, k["model"], c, int(m["OPT"] is not None))
            keep = [np.ascontiguousarray(c.LCELLS, np.int32), np.ascontiguousarray(c.OFF, np.int32), polmap_host.parents(c),
                    np.ascontiguousarray(c.DENS, np.float32), m["EMIT"]]
            opt = None if m["OPT"] is None else np.ascontiguousarray(m["OPT"], np.float32)
            a = Args()
            a.NPIX_X, a.NPIX_Y, a.MAP_DX, a.ABS, a.SCA = nx, ny, kw["MAP_DX"], m["ABS"], m["SCA"]
            obs = kw["INTOBS"] if kw["INTOBS"] is not None else (-1.0e12, 0.0, 0.0)
            for dst, src in ((a.DIR, kw["DIR"]), (a.RA, kw["RA"]), (a.DE, kw["DE"]), (a.CENTRE, kw["CENTRE"]), (a.INTOBS, obs)):
                for i in range(3):
                    dst[i] = src[i]
            a.LCELLS, a.OFF, a.PAR = (x.ctypes.data_as(_I) for x in keep[:3])
            a.DENS, a.EMIT = keep[3].ctypes.data_as(_F), keep[4].ctypes.data_as(_F)
            a.OPT = None if opt is None else opt.ctypes.data_as(_F)
            one = np.full(c.LEVELS * ny * nx, np.nan, np.float32)
            a.MAP = one.ctypes.data_as(_F)
            lib.ref_levelmap(C.byref(a))
            MAP = one.reshape(c.LEVELS, ny, nx)
            assert np.isfinite(MAP).all(), "%s: %d values are not finite" % (name, int((~np.isfinite(MAP)).sum()))
            lit = [int((MAP[l] != 0.0).sum()) for l in range(c.LEVELS)]
            if k["model"] == "oct8":
                assert min(lit) > 0, "%s lights no pixel on some level: %s" % (name, lit)
            if name.endswith("_wide"):
                ring = np.ones((ny, nx), bool)
                ring[1:-1, 1:-1] = False
                assert (MAP[:, ring] == 0.0).all() and (MAP != 0.0).any(), "%s: the outer ring should miss the model" % name
            out["map_" + name] = MAP
            out["fp_" + k["model"]] = lc.fingerprint(m)
            print("%-12s  non-zero pixels per level %-18s  of %d   sum %.6e" % (name, lit, nx * ny, float(MAP.astype(np.float64).sum())))
    path = os.path.join(REPO, "tests", "golden", "levelmaps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
