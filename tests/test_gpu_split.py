"""Packet splitting on the GPU (`split 1`, soc_sim_bg_split) against the CPU restatement of SimBgSplit in soc mode (the math
header both sides compile): every lane follows the restatement's trajectory, so tallies differ only by the order of the
atomic adds (the project's rtol 1e-5; the signed sums INTX/Y/Z of `saveint 2` by that fraction of INT) and the counters and the
maximum stack depth are equal.  Reads only the repository."""
import os

import numpy as np
import pytest

import split_cases as sc
import split_host
from split_engine import SplitOracleEngine, assert_vector_sums_close, restore_engine, run_split, setup_engine
from soc_amd import lib as soclib
from util import assert_tally_close

pytestmark = pytest.mark.gpu

KEYS = split_host.COUNTERS + ("max_depth",)


@pytest.fixture(scope="module")
def want():
    """the restatement's result of every case, computed once"""
    out = {}
    for name in sc.CASES:
        job, SELEM, ms = sc.job(name)
        out[name] = split_host.sim_bg_split("soc", job, SELEM, ms)
    return out


def _same(got, ref, name):
    TABS, INT, INTV, st = got
    wT, wI, wV, wst = ref
    print(name, "gpu", st, "restatement", {k: wst[k] for k in KEYS})
    assert {k: st[k] for k in KEYS} == {k: wst[k] for k in KEYS}, name
    assert wT.max() > 0
    assert_tally_close(TABS, wT, rtol=1e-5)
    assert_tally_close(INT, wI, rtol=1e-5)
    if wV is not None:
        assert np.abs(wV).max() > 0
        assert_vector_sums_close(INTV, wV, wI, rtol=1e-5)      # signed sums: against INT, the sum of the magnitudes (split_engine.py)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_cases_equal_the_restatement(engine, want, name):
    job, SELEM, ms = sc.job(name)
    _same(run_split(engine, job, SELEM, ms), want[name], name)


def test_two_half_ranges_equal_the_whole_launch(engine, want):
    name = "oct6_selem3"
    job, SELEM, ms = sc.job(name)
    half = 64                                       # of GLOBAL 96: a whole wave and half a wave
    a = run_split(engine, job, SELEM, ms, 0, half)
    b = run_split(engine, job, SELEM, ms, half, job.GLOBAL - half)
    wT, wI, _, wst = want[name]
    assert_tally_close(a[0] + b[0], wT, rtol=1e-5)
    assert_tally_close(a[1] + b[1], wI, rtol=1e-5)
    for k in split_host.COUNTERS:
        assert a[3][k] + b[3][k] == wst[k], k
    assert max(a[3]["max_depth"], b[3]["max_depth"]) == wst["max_depth"]
    # and the halves are those of the restatement
    ha = split_host.sim_bg_split("soc", sc.job(name)[0], SELEM, ms, 0, half)
    assert {k: a[3][k] for k in KEYS} == {k: ha[3][k] for k in KEYS}
    assert_tally_close(a[0], ha[0], rtol=1e-5)


def test_small_stack_drops_as_the_restatement(engine, want):
    name = "nest5_ms16"
    job, SELEM, ms = sc.job(name)
    assert ms == 16 and want[name][3]["overflow_drops"] > 0
    _same(run_split(engine, job, SELEM, ms), want[name], name)
    # the same launch with room for every ray drops nothing and absorbs more
    big = run_split(engine, job, SELEM, 64)
    assert big[3]["overflow_drops"] == 0 and big[3]["splits"] > want[name][3]["splits"]


def test_cartesian_grid_never_splits(engine):
    from soc_amd import synth
    from oracle.pyoracle import Job
    c = synth.cartesian_cloud(5, seed=4, NY=4, NZ=3)
    job = Job(c, sc._CSC, ABS=1e-4, SCA=3e-4, SOURCE=1, BATCH=3, SEED=0.37, GLOBAL=sc.launch_shape(c.AREA, 2), WITH_INT=1)
    got = run_split(engine, job, 2, 14)
    ref = split_host.sim_bg_split("soc", Job(c, sc._CSC, ABS=1e-4, SCA=3e-4, SOURCE=1, BATCH=3, SEED=0.37, GLOBAL=job.GLOBAL, WITH_INT=1), 2, 14)
    _same(got, ref, "cartesian")
    assert got[3]["splits"] == 0 and got[3]["max_depth"] == 0 and got[3]["roots"] == 3 * c.AREA


def test_plain_launch_after_a_split_launch(engine):
    """soc_sim_pb after soc_sim_bg_split gives what it gives on a fresh context"""
    from util import run_engine
    job, SELEM, ms = sc.job("oct4b")
    fresh = soclib.Engine(0)
    try:
        want_T, want_I, want_st = run_engine(fresh, sc.job("oct4b")[0])
    finally:
        fresh.close()
    run_split(engine, job, SELEM, ms)
    got_T, got_I, got_st = run_engine(engine, sc.job("oct4b")[0])
    assert got_st == want_st
    assert_tally_close(got_T, want_T, rtol=1e-5)
    assert_tally_close(got_I, want_I, rtol=1e-5)


def test_refused_calls_leave_tallies_and_handle(engine, want):
    name = "kat"
    job, SELEM, ms = sc.job(name)
    setup_engine(engine, job)
    engine.zero(0)
    engine.zero(1)
    engine.split_stats(reset=True)
    engine.sim_bg_split(0, job.BATCH, job.SEED, job.BG, job.TW, SELEM, ms, GLOBAL=job.GLOBAL)
    before = engine.read_tally(0).copy()

    def refused(text, **kw):
        a = dict(PACKETS=0, BATCH=job.BATCH, SEED=job.SEED, BG=job.BG, TW=job.TW, SELEM=SELEM, max_split=ms, GLOBAL=job.GLOBAL)
        a.update(kw)
        with pytest.raises(soclib.SocError) as e:
            engine.sim_bg_split(**a)
        assert text in str(e.value), str(e.value)

    refused("max_split 13", max_split=13)
    refused("SELEM 0", SELEM=0)
    refused("outside GLOBAL", gid_first=100, gid_count=100)
    refused("GB of device memory", GLOBAL=1 << 30, max_split=1 << 24)
    engine.set_mirror(1)
    refused("reflecting faces")
    engine.set_mirror(0)
    engine.set_step_weight(1, 2.0, 0.5)
    refused("weighted free paths")
    engine.set_step_weight(0, 0.0, 0.0)
    engine.set_roi_save([1, 2, 1, 2, 1, 2], 1, 2)
    refused("region-of-interest")
    engine.set_roi_save(None)
    assert np.array_equal(engine.read_tally(0), before)
    assert engine.split_stats()["roots"] == want[name][3]["roots"]
    # the handle goes on: the same launch again doubles the tally
    engine.sim_bg_split(0, job.BATCH, job.SEED, job.BG, job.TW, SELEM, ms, GLOBAL=job.GLOBAL)
    assert_tally_close(engine.read_tally(0), 2.0 * want[name][0].astype(np.float64), rtol=1e-5)
    restore_engine(engine, job)
    # no grid: a fresh handle refuses, and works once it has one
    fresh = soclib.Engine(0)
    try:
        with pytest.raises(soclib.SocError) as e:
            fresh.sim_bg_split(0, 1, 0.5, 1.0, 1.0, 1, 14, GLOBAL=64)
        assert "soc_set_grid" in str(e.value)
        assert fresh.split_stats()["roots"] == 0
    finally:
        fresh.close()


def test_ini_run_equals_the_restatement_engine(engine, tmp_path):
    """one `split 1` ini run end to end: the absorbed file and packet.info of the HIP engine and of the restatement engine"""
    from split_ini import run_ini
    got = run_ini(engine, tmp_path / "gpu", split=1)
    ref = run_ini(SplitOracleEngine("soc"), tmp_path / "cpu", split=1)
    assert got["launches"] is None and len(ref["launches"]) == got["nfreq"]
    assert np.array_equal(got["packet_info"], ref["packet_info"])
    assert got["absorbed"].shape == ref["absorbed"].shape and ref["absorbed"].max() > 0
    for k in range(got["absorbed"].shape[1]):
        assert_tally_close(got["absorbed"][:, k], ref["absorbed"][:, k], rtol=1e-5)
    assert {k: got["stats"][k] for k in KEYS} == {k: ref["stats"][k] for k in KEYS}
