"""Helpers of the tests of packet splitting with a Healpix sky: SplitOracleEngine plus `sim_hp_split` (through the CPU
restatement, tests/hpsplit_host.py), and one oracle Job run through a HIP engine's sim_hp_split."""
import numpy as np

from split_engine import SplitOracleEngine, restore_engine, setup_engine

import hpsplit_host


class HpSplitOracleEngine(SplitOracleEngine):
    """SplitOracleEngine plus the Healpix split launch: what `split 1` + `hpbg` ini runs need from an engine"""

    def __init__(self, mode="soc"):
        SplitOracleEngine.__init__(self, mode)
        self.hp_split_launches = []                # (BATCH, SEED, TW, max_split, GLOBAL, first, count, HPBG, HPBGP) of every launch
        self._split["skipped_splits"] = 0

    def sim_hp_split(self, PACKETS, BATCH, SEED, TW, max_split=0, GLOBAL=None, gid_first=0, gid_count=None):
        job = self._job(1, PACKETS, BATCH, SEED, 0.0, TW, GLOBAL)
        job.HPBG, job.HPBGP = self.HPBG, self.HPBGP
        gid_count = (GLOBAL - gid_first) if gid_count is None else gid_count
        self.hp_split_launches.append((int(BATCH), float(SEED), float(TW), int(max_split), int(GLOBAL), int(gid_first), int(gid_count),
                                       self.HPBG.copy(), None if self.HPBGP is None else self.HPBGP.copy()))
        _, _, _, st = hpsplit_host.sim_hp_split(self.split_mode, job, max_split, gid_first, gid_first + gid_count,
                                                TABS=self.T[0], INT=self._int_target())
        for k in hpsplit_host.COUNTERS + ("skipped_splits",):
            self._split[k] += st[k]
        self._split["max_depth"] = max(self._split["max_depth"], st["max_depth"])


def run_hp_split(eng, job, max_split, gid_first=0, gid_count=None):
    """Returns (TABS, INT, INTV or None, split_stats) of one launch on zeroed tallies"""
    setup_engine(eng, job)
    eng.set_hpbg(job.HPBG, job.HPBGP)
    eng.zero(0)
    eng.zero(1)
    eng.split_stats(reset=True)
    eng.sim_hp_split(0, job.BATCH, job.SEED, job.TW, max_split, GLOBAL=job.GLOBAL, gid_first=gid_first, gid_count=gid_count)
    eng.sync()
    st = eng.split_stats(reset=True)
    INTV = np.stack([eng.read_tally(3 + k) for k in range(3)]) if job.WITH_INT == 2 else None
    out = eng.read_tally(0), eng.read_tally(1), INTV, st
    restore_engine(eng, job)
    return out
