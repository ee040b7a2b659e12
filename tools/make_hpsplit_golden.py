#!/usr/bin/env python3
"""Record tests/golden/hpsplit.npz: what the SimHpSplit kernel of the reference (kernel_ASOC.c:2871-3550, `split 1` with `hpbg`;
compiled unmodified for x86-64 where it lies) gives for the cases of tests/hpsplit_cases.py, its work items run one after the
other in id order.

    python tools/make_hpsplit_golden.py [reference directory]

Run by hand on a machine that has the reference; nothing it compiles is kept (a temporary directory) and no test imports
it.  The compiler recipe is tools/make_split_golden.py's: the -D list of oracle.build.ref_defs (ASOC.py:344-362) with
-DDO_SPLIT=1 and the case's -DMAX_SPLIT, -DHPBG_WEIGHTED, -DWITH_ABU, -DWITH_MSF, -DNDUST, -DSAVE_INTENSITY; the driver is
tools/ref_hpsplit.cpp.

Before it calls the reference the script runs the CPU restatement (tests/hpsplit_host.py, libm mode) over all cases and asserts
hpsplit_cases.coverage: every branch the cases are there for reached, no 30000-step return, and guard == 0 in every case -- no
root ray born too deep for its stack, where the reference writes 4^level entries without looking.  The restatement's counters
are stored with the tallies.
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
from oracle.pyoracle import Oracle                     # noqa: E402
import hpsplit_cases as hc                             # noqa: E402
import hpsplit_host                                    # noqa: E402

_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
STATS = hpsplit_host.COUNTERS + hpsplit_host.EXTRA
POINTERS = ("ABS", "SCA", "LCELLS", "OFF", "PAR", "DENS", "EMIT", "TABS", "DSC", "CSC", "INT", "INTX", "INTY", "INTZ", "OPT", "BG", "HPBGP",
            "ABU", "BUFFER")


class Args(C.Structure):
    _fields_ = [("PACKETS", C.c_int), ("BATCH", C.c_int), ("GLOBAL", C.c_int), ("SEED", C.c_float), ("TW", C.c_float)] + \
               [(k, _I if k in ("LCELLS", "OFF", "PAR") else _F) for k in POINTERS]


def build(tmp, reference, name, job, max_split):
    c = job.cloud
    ndust = 1 if job.MSF is None else len(job.MSF[1])
    defs = obuild.ref_defs(NX=c.NX, NY=c.NY, NZ=c.NZ, LEVELS=c.LEVELS, CELLS=c.CELLS, BINS=job.BINS, WITH_ABU=int(job.OPT is not None),
                           WITH_MSF=int(job.MSF is not None), NDUST=ndust, SAVE_INTENSITY=2 if job.WITH_INT == 2 else 1, NOABSORBED=0)
    defs = [d for d in defs if d.split("=")[0] not in ("-DDO_SPLIT", "-DSELEM", "-DMAX_SPLIT", "-DHPBG_WEIGHTED")]
    defs += ["-DDO_SPLIT=1", "-DSELEM=1", "-DMAX_SPLIT=%d" % max_split, "-DHPBG_WEIGHTED=%d" % int(job.HPBGP is not None)]
    ksrc = os.path.join(reference, "kernel_ASOC.c")
    kobj, dobj, so = (os.path.join(tmp, "%s.%s" % (name, e)) for e in ("k.o", "d.o", "so"))
    common = ["-O2", "-fPIC", "-ffp-contract=off", "-target", "x86_64-unknown-linux-gnu"]
    subprocess.check_call([obuild.CLANG, "-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header", "-ftrivial-auto-var-init=zero",
                           "-w", "-I", reference] + common + defs + ["-c", ksrc, "-o", kobj])
    subprocess.check_call([obuild.CLANG + "++", "-std=c++17", "-w"] + common + ["-c", os.path.join(REPO, "tools", "ref_hpsplit.cpp"), "-o", dobj])
    subprocess.check_call([obuild.CLANG + "++", "-shared", "-Wl,-z,defs", kobj, dobj, "-lm", "-lpthread", "-o", so])
    lib = C.CDLL(so)
    lib.ref_hpsplit.argtypes = [C.POINTER(Args)]
    return lib


def main(argv):
    reference = argv[1] if len(argv) > 1 else obuild.REFERENCE
    host = {}
    for name in hc.CASES:
        job, ms = hc.job(name)
        host[name] = hpsplit_host.sim_hp_split("libm", job, ms)
        print("%-13s restatement %s" % (name, host[name][3]))
    bad = hc.coverage({n: h[3] for n, h in host.items()})
    assert not bad, "; ".join(bad)
    assert all(h[3]["guard"] == 0 for h in host.values())
    orc = Oracle("libm")
    out = dict(meta=np.asarray(hc.meta()))
    all_same = True
    with tempfile.TemporaryDirectory() as tmp:
        for name in hc.CASES:
            job, ms = hc.job(name)
            c = job.cloud
            PAR = np.ascontiguousarray(orc.parents(job), np.int32)
            lib = build(tmp, reference, name, job, ms)
            z = lambda n=c.CELLS: np.zeros(n, np.float32)                               # noqa: E731
            TABS, INT, INTX, INTY, INTZ = z(), z(), z(), z(), z()
            if job.MSF is not None:
                ABS, SCA, CSC, ABU = job.MSF[0], job.MSF[1], np.ascontiguousarray(job.MSF[2], np.float32).ravel(), np.ascontiguousarray(job.MSF[3], np.float32).ravel()
            else:
                ABS, SCA, CSC, ABU = np.asarray([job.ABS], np.float32), np.asarray([job.SCA], np.float32), job.CSC, z(1)
            OPT = z(2) if job.OPT is None else np.ascontiguousarray(job.OPT, np.float32).ravel()
            DSC = np.ones(CSC.size, np.float32)
            HPBGP = z(49152) if job.HPBGP is None else job.HPBGP
            BUFFER = np.zeros(10 * ms * (job.GLOBAL + 1), np.float32)
            keep = [ABS, SCA, job.LCELLS, job.OFF, PAR, job.DENS, z(), TABS, DSC, CSC, INT, INTX, INTY, INTZ, OPT, job.HPBG, HPBGP, ABU, BUFFER]
            a = Args()
            a.PACKETS, a.BATCH, a.GLOBAL, a.SEED, a.TW = 0, job.BATCH, job.GLOBAL, job.SEED, job.TW
            for k, v in zip(POINTERS, keep):
                setattr(a, k, v.ctypes.data_as(_I if v.dtype == np.int32 else _F))
            lib.ref_hpsplit(C.byref(a))
            assert np.isfinite(TABS).all() and TABS.max() > 0, name
            hT, hI, hV, st = host[name]
            same = np.array_equal(TABS.view(np.uint32), hT.view(np.uint32)) and np.array_equal(INT.view(np.uint32), hI.view(np.uint32))
            all_same = all_same and same
            print("%-13s TABS sum %.6e  INT sum %.6e  restatement bit-equal: %s" % (name, float(TABS.astype(np.float64).sum()), float(INT.astype(np.float64).sum()), same))
            out["TABS_" + name], out["INT_" + name] = TABS, INT
            if job.WITH_INT == 2:
                out["INTV_" + name] = np.stack([INTX, INTY, INTZ])
            out["stats_" + name] = np.asarray([st[k] for k in STATS], np.int64)
    path = os.path.join(REPO, "tests", "golden", "hpsplit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", "all bit-equal" if all_same else "NOT all bit-equal")


if __name__ == "__main__":
    main(sys.argv)
