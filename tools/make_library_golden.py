#!/usr/bin/env python3
"""Record tests/golden/library.npz: what the LibrarySolve kernel of the reference (kernel_soc_library.c:6-85 with METHOD 0;
compiled unmodified for x86-64 where it lies) gives for the look-up cases of tests/library_cases.py, its work items run one
after the other in id order.

    python tools/make_library_golden.py [reference directory]

Run by hand on a machine that has the reference; nothing it compiles is kept (a temporary directory) and no test imports it.
The compiler recipe is tools/make_split_golden.py's, with -DMETHOD=0 -DN= -DNFREQ= -DLOCAL= -DCELLS=; the driver is
tools/ref_library.cpp.

The file holds the reference's outputs only: per case column 0 of EMI for every cell (1e32 marks a cell the library has no
answer for) and the whole rows of the other cells, in cell order.  The kernel leaves the rest of a missed row as it finds it;
that part is not recorded.  The inputs come back from library_cases.py, the `meta` string says for which version of it.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle import build as obuild                     # noqa: E402
import library_cases as lc                             # noqa: E402
import library_host                                    # noqa: E402

_F = C.POINTER(C.c_float)


class Args(C.Structure):
    _fields_ = [("no", C.c_int), ("I0", C.c_float), ("dI0", C.c_float)] + \
               [(k, _F) for k in ("I1", "dI1", "I2", "dI2", "X", "Y", "Z", "E", "ABS", "EMI")]


def build(tmp, reference, name, N, NFREQ, cells):
    defs = ["-DMETHOD=0", "-DN=%d" % N, "-DNFREQ=%d" % NFREQ, "-DLOCAL=4", "-DCELLS=%d" % cells]
    ksrc = os.path.join(reference, "kernel_soc_library.c")
    kobj, dobj, so = (os.path.join(tmp, "%s.%s" % (name, e)) for e in ("k.o", "d.o", "so"))
    common = ["-O2", "-fPIC", "-ffp-contract=off", "-target", "x86_64-unknown-linux-gnu"]
    subprocess.check_call([obuild.CLANG, "-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-ftrivial-auto-var-init=zero",
                           "-w", "-I", reference] + common + defs + ["-c", ksrc, "-o", kobj])
    subprocess.check_call([obuild.CLANG + "++", "-std=c++17", "-w"] + common + ["-c", os.path.join(REPO, "tools", "ref_library.cpp"), "-o", dobj])
    subprocess.check_call([obuild.CLANG + "++", "-shared", "-Wl,-z,defs", kobj, dobj, "-lm", "-lpthread", "-o", so])
    lib = C.CDLL(so)
    lib.ref_library.argtypes = [C.POINTER(Args)]
    return lib


def main(argv):
    reference = argv[1] if len(argv) > 1 else obuild.REFERENCE
    out = dict(meta=np.asarray(lc.meta()))
    with tempfile.TemporaryDirectory() as tmp:
        for name in sorted(lc.SOLVE):
            case = lc.solve_case(name)
            L, ABS3 = case["lib"], np.ascontiguousarray(case["ABS3"], np.float32)
            N, NFREQ, n = L["N"], L["E"].shape[1], ABS3.shape[0]
            lib = build(tmp, reference, name, N, NFREQ, n)
            keep = [np.ascontiguousarray(L[k], np.float32) for k in ("I1", "dI1", "I2", "dI2", "X", "Y", "Z", "E")] + [ABS3]
            EMI = np.full((n, NFREQ), np.nan, np.float32)                 # (what a missed row keeps beyond its element 0)
            a = Args()
            a.no, a.I0, a.dI0 = n, L["I0"], L["dI0"]
            for k, v in zip(("I1", "dI1", "I2", "dI2", "X", "Y", "Z", "E", "ABS", "EMI"), keep + [EMI]):
                setattr(a, k, v.ctypes.data_as(_F))
            sys.stdout.flush()
            lib.ref_library(C.byref(a))
            hit = ~(EMI[:, 0] > 1.0e31)
            rest = EMI[~hit, 1:]                                         # untouched, or the 1e32 row of an empty bin copied whole
            assert np.isfinite(EMI[hit]).all() and (np.isnan(rest) | (rest > 1.0e31)).all(), name
            hE, _, hmiss = library_host.solve("libm", L, ABS3)
            same = np.array_equal(hE[:, 0].view(np.uint32), EMI[:, 0].view(np.uint32)) and np.array_equal(hE[hit].view(np.uint32), EMI[hit].view(np.uint32))
            print("%-14s cells %5d  misses %5d  restatement bit-equal: %s" % (name, n, int((~hit).sum()), same))
            out["EMI0_" + name], out["ROWS_" + name] = EMI[:, 0].copy(), EMI[hit].copy()
    path = os.path.join(REPO, "tests", "golden", "library.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv)
