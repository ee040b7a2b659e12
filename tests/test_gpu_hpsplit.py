"""Packet splitting with a Healpix sky on the GPU (`split 1` + `hpbg`, soc_sim_hp_split) against the CPU restatement of SimHpSplit
in soc mode (the math header both sides compile): every lane follows the restatement's trajectory, so tallies differ only by the
order of the atomic adds (the project's rtol 1e-5; the signed sums INTX/Y/Z of `saveint 2` by that fraction of INT) and the
counters, the skipped splits and the maximum stack depth are equal.
Reads only the repository."""
import numpy as np
import pytest

import hpsplit_cases as hc
import hpsplit_host
import split_cases as sc
from hpsplit_engine import HpSplitOracleEngine, run_hp_split
from split_engine import assert_vector_sums_close, restore_engine, run_split, setup_engine
from soc_amd import lib as soclib
from util import assert_tally_close

pytestmark = pytest.mark.gpu

KEYS = hpsplit_host.COUNTERS + ("max_depth", "skipped_splits")


@pytest.fixture(scope="module")
def want():
    """the restatement's result of every case, computed once"""
    return {name: hpsplit_host.sim_hp_split("soc", *hc.job(name)) for name in hc.CASES}


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


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_cases_equal_the_restatement(engine, want, name):
    job, ms = hc.job(name)
    _same(run_hp_split(engine, job, ms), want[name], name)


def test_two_half_ranges_equal_the_whole_launch(engine, want):
    name = "oct4b_w"
    job, ms = hc.job(name)
    half = 64                                       # of GLOBAL 96: a whole wave and half a wave
    a = run_hp_split(engine, job, ms, 0, half)
    b = run_hp_split(engine, job, ms, half, job.GLOBAL - half)
    wT, wI, _, wst = want[name]
    assert_tally_close(a[0] + b[0], wT, rtol=1e-5)
    assert_tally_close(a[1] + b[1], wI, rtol=1e-5)
    for k in hpsplit_host.COUNTERS + ("skipped_splits",):
        assert a[3][k] + b[3][k] == wst[k], k
    assert max(a[3]["max_depth"], b[3]["max_depth"]) == wst["max_depth"]
    # and the halves are those of the restatement
    ha = hpsplit_host.sim_hp_split("soc", hc.job(name)[0], ms, 0, half)
    hb = hpsplit_host.sim_hp_split("soc", hc.job(name)[0], ms, half, None)
    assert {k: a[3][k] for k in KEYS} == {k: ha[3][k] for k in KEYS}
    assert {k: b[3][k] for k in KEYS} == {k: hb[3][k] for k in KEYS}
    assert_tally_close(a[0], ha[0], rtol=1e-5)
    assert_tally_close(b[0], hb[0], rtol=1e-5)


def test_small_stack_skips_and_drops_as_the_restatement(engine, want):
    name = "jump3_ms17"
    job, ms = hc.job(name)
    assert ms == 17 and want[name][3]["overflow_drops"] > 0 and want[name][3]["skipped_splits"] > 0
    _same(run_hp_split(engine, job, ms), want[name], name)
    # the same launch with room for every ray skips nothing, drops nothing and splits more often
    big = run_hp_split(engine, job, 64)
    assert big[3]["overflow_drops"] == 0 and big[3]["skipped_splits"] == 0 and big[3]["splits"] > want[name][3]["splits"]


def test_cartesian_grid_never_splits(engine):
    from soc_amd import synth
    from oracle.pyoracle import Job
    c = synth.cartesian_cloud(5, seed=4, NY=4, NZ=3)
    HPBG, HPBGP = hc.sky_inputs("oct4b_w")
    kw = dict(ABS=1e-4, SCA=3e-4, SOURCE=1, BATCH=3, SEED=0.37, BG=0.0, GLOBAL=hc.GLOBAL, WITH_INT=1, HPBG=HPBG, HPBGP=HPBGP)
    got = run_hp_split(engine, Job(c, sc._CSC, **kw), 14)
    ref = hpsplit_host.sim_hp_split("soc", Job(c, sc._CSC, **kw), 14)
    _same(got, ref, "cartesian")
    assert got[3]["splits"] == 0 and got[3]["max_depth"] == 0 and got[3]["roots"] == hc.GLOBAL * 3


def test_other_launches_after_a_healpix_split_launch(engine):
    """soc_sim_hp and soc_sim_bg_split after soc_sim_hp_split give what they give on a fresh handle, and the isotropic split never
    counts a skipped split"""
    from oracle.pyoracle import Job

    def others(eng):
        job, ms = hc.job("oct4b_w")
        setup_engine(eng, job)
        eng.set_hpbg(job.HPBG, job.HPBGP)
        eng.zero(0)
        eng.zero(1)
        eng.sim_hp(0, job.BATCH, job.SEED, job.TW, 128)
        eng.sync()
        hp = eng.read_tally(0), eng.read_tally(1)
        restore_engine(eng, job)
        bjob, SELEM, bms = sc.job("nest5_ms16")
        bg = run_split(eng, bjob, SELEM, bms)
        return hp, bg

    fresh = soclib.Engine(0)
    try:
        want_hp, want_bg = others(fresh)
    finally:
        fresh.close()
    job, ms = hc.job("jump3_ms17")
    assert run_hp_split(engine, job, ms)[3]["skipped_splits"] > 0
    got_hp, got_bg = others(engine)
    assert want_hp[0].max() > 0
    for g, w in zip(got_hp, want_hp):
        assert_tally_close(g, w, rtol=1e-5)
    assert got_bg[3] == want_bg[3] and got_bg[3]["overflow_drops"] > 0 and got_bg[3]["skipped_splits"] == 0
    assert_tally_close(got_bg[0], want_bg[0], rtol=1e-5)
    assert_tally_close(got_bg[1], want_bg[1], rtol=1e-5)


def test_refused_calls_leave_tallies_and_handle(engine, want):
    name = "kat"
    job, ms = hc.job(name)
    setup_engine(engine, job)
    engine.set_hpbg(job.HPBG, job.HPBGP)
    engine.zero(0)
    engine.zero(1)
    engine.split_stats(reset=True)
    engine.sim_hp_split(0, job.BATCH, job.SEED, job.TW, ms, GLOBAL=job.GLOBAL)
    before = engine.read_tally(0).copy()

    def refused(text, **kw):
        a = dict(PACKETS=0, BATCH=job.BATCH, SEED=job.SEED, TW=job.TW, max_split=ms, GLOBAL=job.GLOBAL)
        a.update(kw)
        with pytest.raises(soclib.SocError) as e:
            engine.sim_hp_split(**a)
        assert text in str(e.value), str(e.value)

    refused("max_split 13", max_split=13)
    refused("outside GLOBAL", gid_first=90, gid_count=10)
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
    st = engine.split_stats()
    assert {k: st[k] for k in KEYS} == {k: want[name][3][k] for k in KEYS}
    # the handle goes on: the same launch again doubles the tally
    engine.sim_hp_split(0, job.BATCH, job.SEED, job.TW, ms, GLOBAL=job.GLOBAL)
    assert_tally_close(engine.read_tally(0), 2.0 * want[name][0].astype(np.float64), rtol=1e-5)
    restore_engine(engine, job)
    # a fresh handle: no grid, then no sky; it works once it has both
    fresh = soclib.Engine(0)
    try:
        with pytest.raises(soclib.SocError) as e:
            fresh.sim_hp_split(0, 1, 0.5, 1.0, 14, GLOBAL=64)
        assert "soc_set_grid" in str(e.value)
        setup_engine(fresh, job)
        with pytest.raises(soclib.SocError) as e:
            fresh.sim_hp_split(0, job.BATCH, job.SEED, job.TW, ms, GLOBAL=job.GLOBAL)
        assert "call soc_set_hpbg first" in str(e.value)
        st = fresh.split_stats()
        assert st["roots"] == 0 and st["skipped_splits"] == 0
        assert not fresh.read_tally(0).any()
        _same(run_hp_split(fresh, job, ms), want[name], name)
    finally:
        fresh.close()


def test_ini_run_equals_the_restatement_engine(engine, tmp_path):
    """one `split 1` + `hpbg` ini run end to end (oct4b: 128 work items x 100 rays per frequency, weighted sky): the absorbed file,
    packet.info and the counters of the HIP engine and of the restatement engine"""
    from hpsplit_ini import run_hp_ini
    got = run_hp_ini(engine, tmp_path / "gpu", 1)
    ref = run_hp_ini(HpSplitOracleEngine("soc"), tmp_path / "cpu", 1)
    assert got["hp_launches"] is None and len(ref["hp_launches"]) == got["nfreq"]
    assert all(l[:1] + l[3:7] == (100, 0, 128, 0, 128) for l in ref["hp_launches"])
    assert np.array_equal(got["packet_info"], ref["packet_info"])
    assert got["absorbed"].shape == ref["absorbed"].shape and ref["absorbed"].max() > 0
    for k in range(got["absorbed"].shape[1]):
        assert_tally_close(got["absorbed"][:, k], ref["absorbed"][:, k], rtol=1e-5)
    assert {k: got["stats"][k] for k in KEYS} == {k: ref["stats"][k] for k in KEYS}
    assert ref["stats"]["splits"] > 0
