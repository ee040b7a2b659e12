"""Helpers of the packet-splitting tests: OracleEngine with `sim_bg_split` (through the CPU restatement, tests/split_host.py),
and one oracle Job run through a HIP engine's sim_bg_split."""
import numpy as np

from oracle.pyoracle import Job
from oracle_engine import OracleEngine

import split_host


class SplitOracleEngine(OracleEngine):
    """OracleEngine plus the split launch: what `split 1` ini runs need from an engine"""

    def __init__(self, mode="soc"):
        OracleEngine.__init__(self, mode)
        self.split_mode = mode
        self.split_launches = []                   # (BATCH, SEED, BG, TW, SELEM, max_split, GLOBAL, first, count) of every launch
        self._split = {k: 0 for k in split_host.COUNTERS}
        self._split["max_depth"] = 0

    def sim_bg_split(self, PACKETS, BATCH, SEED, BG, TW, SELEM, max_split=0, GLOBAL=None, gid_first=0, gid_count=None):
        job = self._job(1, PACKETS, BATCH, SEED, BG, TW, GLOBAL)
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self.split_launches.append((int(BATCH), float(SEED), float(BG), float(TW), int(SELEM), int(max_split), int(GLOBAL),
                                    int(gid_first), int(gid_count)))
        _, _, _, st = split_host.sim_bg_split(self.split_mode, job, SELEM, max_split, gid_first, gid_first + gid_count,
                                              TABS=self.T[0], INT=self._int_target())
        for k in split_host.COUNTERS:
            self._split[k] += st[k]
        self._split["max_depth"] = max(self._split["max_depth"], st["max_depth"])

    def split_stats(self, reset=False):
        st = dict(self._split)
        if reset:
            for k in self._split:
                self._split[k] = 0
        return st


def setup_engine(eng, job):
    """the state a Job describes, on a HIP engine (tests/util.py: run_engine, without the launch)"""
    eng.set_cloud(job.cloud)
    eng.set_features(with_int=job.WITH_INT, ps_method=0, use_emweight=0)
    eng.set_optical(job.ABS, job.SCA)
    eng.set_step_weight(0, 0.0, 0.0)
    eng.set_mirror(0)
    eng.set_opt_half(False)
    if job.MSF is not None:
        ABS, SCA, CSC, ABU = job.MSF
        eng.set_abundances(ABU)
        eng.set_optical_abu(ABS, SCA)
        eng.set_scatter_tables(None, CSC)
    else:
        eng.set_scatter_table(job.DSC, job.CSC)
        eng.set_opt(job.OPT)
    eng.set_exec(0, 4)


def restore_engine(eng, job):
    if job.MSF is not None:
        eng.set_scatter_table(None, job.MSF[2][0])
        eng.set_opt(None)
        eng.set_abundances(None)


def assert_vector_sums_close(INTV, want_INTV, want_INT, rtol=1e-5, floor_frac=1e-6):
    """INTX, INTY, INTZ of runs with identical trajectories: signed sums of delta * u_k, so the order of the adds moves a sum by a
    fraction of the sum of the magnitudes of its terms, which is at most INT (|u_k| <= 1) -- not by a fraction of the sum itself,
    which cancels.  (Measured on the restatement alone, x104_int2 added up in another order: up to 3e-3 of |INTX|, 3e-7 of INT.)
    The bound is util.assert_tally_close's with the cell's INT as the magnitude."""
    I = np.asarray(want_INT, np.float64)
    tol = rtol * I + floor_frac * rtol * I.max()
    for k in range(3):
        d = np.abs(np.asarray(INTV[k], np.float64) - np.asarray(want_INTV[k], np.float64))
        assert not (d > tol).any(), "INTV[%d]: %d of %d cells differ; worst %.3e of INT" % (k, (d > tol).sum(), d.size, (d / np.maximum(I, 1e-300))[d > tol].max())


def run_split(eng, job, SELEM, max_split, gid_first=0, gid_count=None):
    """Returns (TABS, INT, INTV or None, split_stats) of one launch on zeroed tallies"""
    setup_engine(eng, job)
    eng.zero(0)
    eng.zero(1)
    eng.split_stats(reset=True)
    eng.sim_bg_split(0, job.BATCH, job.SEED, job.BG, job.TW, SELEM, max_split, GLOBAL=job.GLOBAL, gid_first=gid_first, gid_count=gid_count)
    eng.sync()
    st = eng.split_stats(reset=True)
    INTV = np.stack([eng.read_tally(3 + k) for k in range(3)]) if job.WITH_INT == 2 else None
    out = eng.read_tally(0), eng.read_tally(1), INTV, st
    restore_engine(eng, job)
    return out
