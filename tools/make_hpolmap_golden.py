#!/usr/bin/env python3
"""Record tests/golden/hpolmaps.npz: what the reference's PolHealpixMapping kernel (kernel_ASOC_map_H.c, compiled unmodified
for x86-64 where it lies) gives for the cases of tests/hpolmap_cases.py.

    python tools/make_hpolmap_golden.py [reference directory]

Run by hand on a machine that has the reference; nothing it compiles is kept (a temporary directory) and no test
imports it.  The compiler recipe is tools/make_polmap_golden.py's with NSIDE, POLRED, LEVEL_THRESHOLD, INTERPOLATE, p00,
MINLOS and MAXLOS substituted in the -D list (ASOC.py:344-362, :3827); the driver is tools/ref_hpolmap.cpp.  Only
-D POLSTAT=0 compiles in that file.  The models with abundances are built with -D WITH_ABU=1 as ASOC.py does, and get their
OPT array -- the kernel does not read it (its per-cell line is under "#ifdef USE_ABU", which nothing defines), so their
maps are those of the scalar ABS + SCA.

Before it calls the reference the script asks the CPU restatement's step counter whether every ray of the case ends (on a
hierarchy that walk can cycle without end); before it writes, it checks what the tests rely on: no zero vector in the field, I, Q, U finite in every pixel of
every case, I > 0 wherever the column density is.
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
import hpolmap_cases as hc                             # noqa: E402
import hpolmap_host                                    # noqa: E402
import polmap_host                                     # noqa: E402

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


class Args(C.Structure):
    _fields_ = [("NSIDE", C.c_int), ("ABS", C.c_float), ("SCA", C.c_float), ("Y_SHEAR", C.c_float), ("INTOBS", C.c_float * 4),
                ("LCELLS", _I), ("OFF", _I), ("PAR", _I),
                ("DENS", _F), ("EMIT", _F), ("OPT", _F), ("Bx", _F), ("By", _F), ("Bz", _F), ("MAP", _F)]


def build(tmp, reference, tag, cloud, WITH_ABU, k):
    defs = obuild.ref_defs(NX=cloud.NX, NY=cloud.NY, NZ=cloud.NZ, LEVELS=cloud.LEVELS, CELLS=cloud.CELLS, WITH_ABU=WITH_ABU,
                           LEVEL_THRESHOLD=k["thr"], GL=hc.GL)
    sub = {"POLSTAT": 0, "POLRED": k["polred"], "p00": "%.4ff" % hc.P0, "NSIDE": hc.NSIDE, "INTERPOLATE": k["interp"],
           "MINLOS": "%.3ef" % k["minlos"], "MAXLOS": "%.3ef" % k["maxlos"]}
    defs = [d for d in defs if d[2:].split("=")[0] not in sub] + ["-D%s=%s" % kv for kv in sub.items()]
    ksrc = os.path.join(reference, "kernel_ASOC_map_H.c")
    kobj, dobj, so = (os.path.join(tmp, "%s.%s" % (tag, e)) for e in ("k.o", "d.o", "so"))
    common = ["-O2", "-fPIC", "-ffp-contract=off", "-target", "x86_64-unknown-linux-gnu"]
    subprocess.check_call([obuild.CLANG, "-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-ftrivial-auto-var-init=zero",
                           "-w", "-I", reference] + common + defs + ["-c", ksrc, "-o", kobj])
    subprocess.check_call([obuild.CLANG + "++", "-std=c++17", "-w"] + common + ["-c", os.path.join(REPO, "tools", "ref_hpolmap.cpp"), "-o", dobj])
    subprocess.check_call([obuild.CLANG + "++", "-shared", "-Wl,-z,defs", kobj, dobj, "-lm", "-lpthread", "-o", so])
    lib = C.CDLL(so)
    lib.ref_hpolmap.argtypes = [C.POINTER(Args)]
    return lib


def main(argv):
    reference = argv[1] if len(argv) > 1 else obuild.REFERENCE
    npix = 12 * hc.NSIDE ** 2
    out = dict(NSIDE=np.asarray(hc.NSIDE, np.int32), meta=np.asarray(json.dumps(dict(cases=hc.CASES, GL=hc.GL, p0=hc.P0))))
    with tempfile.TemporaryDirectory() as tmp:
        for name, k in hc.CASES.items():
            m = hc.model(k["model"])
            c = m["cloud"]
            B = m["B"]
            assert (B[0].astype(np.float64) ** 2 + B[1].astype(np.float64) ** 2 + B[2].astype(np.float64) ** 2 > 0.0).all(), "zero field vector"
            obs = hc.case_observer(name)
            # the reference has no step limit, and on a hierarchy its walk can cycle: ask the restatement's counter first
            _, NST = hpolmap_host.polmap("libm", c, B, m["EMIT"], hc.NSIDE, obs, m["ABS"], m["SCA"], steps=True, **hc.switches(name))
            assert NST.max() < 1 << 15, "%s: %d rays would not end in the reference" % (name, int((NST >= 1 << 15).sum()))
            lib = build(tmp, reference, name, c, int(m["OPT"] is not None), k)
            keep = [np.ascontiguousarray(c.LCELLS, np.int32), np.ascontiguousarray(c.OFF, np.int32), polmap_host.parents(c),
                    np.ascontiguousarray(c.DENS, np.float32), m["EMIT"]] + list(B)
            opt = None if m["OPT"] is None else np.ascontiguousarray(m["OPT"], np.float32)
            a = Args()
            a.NSIDE, a.ABS, a.SCA, a.Y_SHEAR = hc.NSIDE, m["ABS"], m["SCA"], k["yshear"]
            for i in range(3):
                a.INTOBS[i] = obs[i]
            a.LCELLS, a.OFF, a.PAR = (x.ctypes.data_as(_I) for x in keep[:3])
            a.DENS, a.EMIT = keep[3].ctypes.data_as(_F), keep[4].ctypes.data_as(_F)
            a.Bx, a.By, a.Bz = (x.ctypes.data_as(_F) for x in keep[5:8])
            a.OPT = None if opt is None else opt.ctypes.data_as(_F)
            one = np.full(4 * npix, np.nan, np.float32)
            a.MAP = one.ctypes.data_as(_F)
            lib.ref_hpolmap(C.byref(a))
            MAP = one.reshape(4, npix)
            assert np.isfinite(MAP).all(), "%s: %d values are not finite" % (name, int((~np.isfinite(MAP)).sum()))
            assert (MAP[0][MAP[3] > 0.0] > 0.0).all(), "%s: I <= 0 in %d pixels with N > 0" % (name, int((MAP[0][MAP[3] > 0.0] <= 0.0).sum()))
            if k["obs"] == "outside":
                assert (MAP == 0.0).all()
            elif k["minlos"] <= 0.0:
                assert (MAP[3] > 0.0).all(), "%s: %d pixels see no column" % (name, int((MAP[3] <= 0.0).sum()))
            else:                                      # a ray that leaves before MINLOS registers nothing
                assert (MAP[3] > 0.0).any()
            out["map_" + name] = MAP
            out["obs_" + name] = np.asarray(obs, np.float64)
            out["fp_" + k["model"]] = hc.fingerprint(m)
            print("%-16s  observer %-28s  sum I %.6e  max |Q|/I %.3f" % (name, str(tuple(round(v, 4) for v in obs)), float(MAP[0].sum()),
                                                                         float(np.max(np.abs(MAP[1]) / np.maximum(MAP[0], 1e-30)))))
    path = os.path.join(REPO, "tests", "golden", "hpolmaps.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
