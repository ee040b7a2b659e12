"""Compile tests/csrc/hpsplit_host.c (the CPU restatement of SimHpSplit, kernel_ASOC.c:2871-3550) in the oracle's two math
modes and bind it.  The source includes tests/csrc/split_host.c and with it oracle/soc_oracle.c as a unit, so a launch is
described by the oracle's model structure (oracle.pyoracle.Job with HPBG / HPBGP) plus the split arguments."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle.pyoracle import Oracle, OrcModel

import split_host

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "csrc", "hpsplit_host.c")
DEPS = [SRC] + split_host.DEPS

COUNTERS = split_host.COUNTERS
EXTRA = ("max_depth", "guard", "initial", "stop20", "skipped_splits", "skipped_replicas")


class HsArgs(C.Structure):
    _fields_ = [("max_split", C.c_int), ("gid0", C.c_int), ("gid1", C.c_int),
                ("n", C.c_ulonglong * 6), ("guard", C.c_ulonglong), ("initial", C.c_ulonglong), ("stop20", C.c_ulonglong),
                ("skipped_splits", C.c_ulonglong), ("skipped_replicas", C.c_ulonglong), ("max_depth", C.c_int)]


_libs = {}
_oracles = {}


def load(mode):
    """mode 'libm' (what the reference's x86 build computes) or 'soc' (what the HIP kernel computes)"""
    if mode in _libs:
        return _libs[mode]
    so = os.path.join(HERE, "csrc", "libhpsplit_%s.so" % mode)
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS):
        tmp = "%s.%d.tmp" % (so, os.getpid())
        cmd = ["gcc", "-O2", "-std=gnu11", "-fPIC", "-shared", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "-mfma",
               "-msse4.1", "-Wall", "-Wno-unused-function", "-Wno-unused-variable"] \
            + (["-DSOC_ORACLE_LIBM"] if mode == "libm" else []) + [SRC, "-o", tmp, "-lm"]
        try:
            subprocess.check_call(cmd)
            os.replace(tmp, so)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    lib = C.CDLL(so)
    lib.hs_sim_hp_split.restype = C.c_int
    lib.hs_sim_hp_split.argtypes = [C.POINTER(OrcModel), C.POINTER(HsArgs)]
    assert lib.sp_math_mode() == (1 if mode == "soc" else 0)
    _libs[mode] = lib
    return lib


def sim_hp_split(mode, job, max_split, gid0=0, gid1=None, TABS=None, INT=None):
    """Work items [gid0, gid1) of the launch `job` (an oracle Job with HPBG and, weighted, HPBGP; GLOBAL = the work items launched)
    in id order.  Adds to TABS / INT when given.  Returns (TABS, INT, INTV or None, stats): stats holds COUNTERS and EXTRA."""
    lib = load(mode)
    if mode not in _oracles:
        _oracles[mode] = Oracle(mode)
    m = _oracles[mode]._model(job)
    cells = job.cloud.CELLS
    TABS = np.zeros(cells, np.float32) if TABS is None else TABS
    INT = np.zeros(cells, np.float32) if INT is None else INT
    m.TABS, m.INT = TABS.ctypes.data_as(C.POINTER(C.c_float)), INT.ctypes.data_as(C.POINTER(C.c_float))
    m.threaded = 0
    a = HsArgs()
    a.max_split = int(max_split if max_split > 0 else 4300)
    a.gid0, a.gid1 = int(gid0), int(job.GLOBAL if gid1 is None else gid1)
    if lib.hs_sim_hp_split(C.byref(m), C.byref(a)) != 0:
        raise ValueError("sim_hp_split: max_split %d, work items [%d, %d) of %d" % (max_split, a.gid0, a.gid1, job.GLOBAL))
    st = {k: int(a.n[i]) for i, k in enumerate(COUNTERS)}
    st.update({k: int(getattr(a, k)) for k in EXTRA})
    return TABS, INT, (job.INTV if job.WITH_INT == 2 else None), st
