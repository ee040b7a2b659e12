"""Packet splitting of the isotropic background (`split 1`, SimBgSplit) without a GPU: the CPU restatement against the
recorded reference (tests/golden/split.npz, tools/make_split_golden.py), the launch arithmetic, the ini handling and the
driver on a test engine that runs split launches through the restatement."""
import os

import numpy as np
import pytest

import split_cases as sc
import split_host
from oracle_engine import OracleEngine
from split_engine import SplitOracleEngine
from split_ini import BG, FREQ, run_ini, write_model
from soc_amd import launch
from soc_amd.asoc import AbsorptionRun, UnsupportedOption
from soc_amd.ini import User

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split.npz")


@pytest.fixture(scope="module")
def libm():
    out = {}
    for name in sc.CASES:
        job, SELEM, ms = sc.job(name)
        out[name] = split_host.sim_bg_split("libm", job, SELEM, ms)
    return out


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_restatement_equals_the_reference_bit_for_bit(libm, name):
    g = np.load(GOLDEN)
    TABS, INT, INTV, st = libm[name]
    assert g["TABS_" + name].max() > 0
    assert _bits(TABS, g["TABS_" + name]) and _bits(INT, g["INT_" + name])
    if sc.CASES[name]["variant"] == "int2":
        assert _bits(INTV, g["INTV_" + name]) and np.abs(INTV).max() > 0
    assert [st[k] for k in split_host.COUNTERS] + [st["max_depth"]] == list(g["stats_" + name])


def test_golden_is_of_these_cases():
    assert str(np.load(GOLDEN)["meta"]) == sc.meta()


def test_cases_cover_every_branch(libm):
    assert sc.coverage({n: r[3] for n, r in libm.items()}) == []
    total = {k: sum(r[3][k] for r in libm.values()) for k in split_host.COUNTERS}
    assert all(total[k] > 0 for k in split_host.COUNTERS[:5]) and total["long_returns"] == 0
    assert libm["oct4b"][3]["initial"] > 0 and libm["kat"][3]["deep_splits"] > 0 and libm["oct4b_opaque"][3]["stop20"] > 0
    assert libm["nest5_ms16"][3]["overflow_drops"] > 0
    # SELEM 3 on AREA 216: work items 24..95 return at their third element, so every element is sent from exactly once
    job, SELEM, _ = sc.job("oct6_selem3")
    assert job.GLOBAL == 96 and libm["oct6_selem3"][3]["roots"] == job.cloud.AREA * job.BATCH


def test_soc_mode_follows_the_same_trajectories(libm):
    """the two math modes differ in the last bits of exp, log, sin, cos only: same events unless a free path lands within those"""
    for name in ("kat", "oct6_selem3"):
        job, SELEM, ms = sc.job(name)
        T, _, _, st = split_host.sim_bg_split("soc", job, SELEM, ms)
        assert {k: st[k] for k in split_host.COUNTERS} == {k: libm[name][3][k] for k in split_host.COUNTERS}
        assert np.allclose(T, libm[name][0], rtol=1e-4, atol=1e-6 * T.max())


def test_x104_tells_a_float_walk_from_a_double_one(monkeypatch):
    """The x104 case exists to catch a DBL kernel that walks in float: such a walk must move the tallies by more than the GPU
    tests' rtol 1e-5 in many cells.  Observed: 104 cells of the 4601 that carry signal, largest relative difference 3.2e-4."""
    import oracle.pyoracle
    job, SELEM, ms = sc.job("x104")
    assert oracle.pyoracle.double_index(job.cloud.NX, job.cloud.LEVELS) == 1
    n, of = sc.float_walk_differs(lambda: split_host.sim_bg_split("soc", sc.job("x104")[0], SELEM, ms)[0], monkeypatch)
    print("x104: %d of %d cells differ by more than 1e-5 when Index() runs in float" % (n, of))
    assert n >= 50


def test_half_ranges_sum_to_the_launch(libm):
    name = "oct6_selem3"
    job, SELEM, ms = sc.job(name)
    a = split_host.sim_bg_split("libm", job, SELEM, ms, 0, 40)
    TABS, INT, _, b = split_host.sim_bg_split("libm", sc.job(name)[0], SELEM, ms, 40, None, TABS=a[0], INT=a[1])
    assert _bits(TABS, libm[name][0])              # one thread, id order: the very same sequence of adds
    assert all(a[3][k] + b[k] == libm[name][3][k] for k in split_host.COUNTERS)


def test_launch_arithmetic():
    """ASOC.py:311-315 and :1067-1075 by hand"""
    # config-3-like: 256^3 roots, AREA = 6*256^2 = 393216 = 12 * 32768: SELEM 12, GLOBAL = Fix(32768 + 1, 32) = 32800
    L = launch.bg_split_launch(2000000, 393216)
    assert (L["SELEM"], L["GLOBAL"], L["BATCH"], L["PACKETS"]) == (12, 32800, 5, 1966080)
    assert L["SELEM"] * L["GLOBAL"] >= 393216 and L["WBG"] == np.pi / (launch.PLANCK * 5)
    # AREA not divisible by GLOBAL_0: 100 x 90 x 80 -> AREA = 2*(9000+7200+8000) = 48400; 48400 // 32768 = 1 -> GLOBAL = Fix(48401, 32) = 48416
    L = launch.bg_split_launch(100000, 48400)
    assert (L["SELEM"], L["GLOBAL"], L["BATCH"], L["PACKETS"]) == (1, 48416, 2, 96800)
    # 130^3: AREA = 101400; 101400 // 32768 = 3; 101400 // 3 + 1 = 33801 -> 33824; 3 * 33824 = 101472 >= AREA
    L = launch.bg_split_launch(50000, 101400)
    assert (L["SELEM"], L["GLOBAL"], L["BATCH"], L["PACKETS"]) == (3, 33824, 1, 101400)
    assert L["WBG"] == np.pi / launch.PLANCK
    # a small model: one element per work item, BATCH = int(BGPAC / AREA)
    L = launch.bg_split_launch(300, 96)
    assert (L["SELEM"], L["GLOBAL"], L["BATCH"], L["PACKETS"]) == (1, 128, 3, 288)
    L = launch.bg_split_launch(300, 96, LOCAL=8)
    assert L["GLOBAL"] == 104


def _refused(tmp_path, engine, extra, text, sub):
    ini = write_model(tmp_path / sub, sc.model("oct4b"), "split 1\n" + extra)
    with pytest.raises(UnsupportedOption) as e:
        AbsorptionRun(User(ini), engine, verbose=0)
    assert text in str(e.value), str(e.value)


def test_ini_refusals(tmp_path):
    eng = SplitOracleEngine("soc")
    _refused(tmp_path, OracleEngine("soc"), "", "the engine has no sim_bg_split", "a")
    np.ones((len(FREQ), 49152), np.float32).tofile(str(tmp_path / "sky.bin"))
    _refused(tmp_path, eng, "hpbg %s/sky.bin 1.0 0\n" % tmp_path, "SimHpSplit", "b")
    _refused(tmp_path, eng, "mirror xX\n", "split with mirror", "c")
    _refused(tmp_path, eng, "stepweight 2 0.5 1\n", "split with stepweight", "d")
    _refused(tmp_path, eng, "roi 1 2 1 2 1 2\nroisave %s/roi.save 1\n" % tmp_path, "split with roisave", "e")
    _refused(tmp_path, eng, "maxsplit 10\n", "maxsplit 10", "f")
    # `split 0` is the plain run on any engine, and maxsplit alone changes nothing
    r = run_ini(OracleEngine("soc"), tmp_path / "g", split=0, extra="maxsplit 20\n")
    assert list(r["packet_info"]) == [384, 0, 0, 0]


def test_ini_run_equals_tallies_composed_by_hand(tmp_path):
    """`split 1` on the test engine: the launches are the hand-worked ones, packet.info carries the corrected BGPAC, and the
    absorbed file holds the INT tallies of the same launches of the restatement, scaled as the plain run's"""
    from soc_amd import files
    c = sc.model("oct4b")
    eng = SplitOracleEngine("soc")
    r = run_ini(eng, tmp_path / "a", split=1, extra="maxsplit 40\n", bgpackets=300)
    L = launch.bg_split_launch(300, c.AREA)
    assert (L["SELEM"], L["GLOBAL"], L["BATCH"], L["PACKETS"]) == (1, 128, 3, 288)
    assert list(r["packet_info"]) == [288, 0, 0, 0]
    assert len(eng.split_launches) == len(FREQ)
    run = r["run"]
    want = np.zeros((c.CELLS, len(FREQ)), np.float32)
    from oracle.pyoracle import Job
    for k, (BATCH, SEED, BGk, TW, SELEM, ms, GLOBAL, first, count) in enumerate(eng.split_launches):
        assert (BATCH, SELEM, ms, GLOBAL, first, count) == (3, 1, 40, 128, 0, 128)
        assert SEED == pytest.approx(launch.launch_seed(0.7853981634, k))
        assert np.float32(BGk) == np.float32(float(np.float32(BG[k])) * L["WBG"] / FREQ[k])
        ABS = np.float32(run.AFABS[0][k])
        SCA = np.float32(run.AFSCA[0][k])
        job = Job(c, run.FCSC[0, k, :], ABS=ABS, SCA=SCA, SOURCE=1, BATCH=BATCH, SEED=SEED, BG=BGk, TW=TW, GLOBAL=GLOBAL, WITH_INT=1)
        want[:, k] = split_host.sim_bg_split("soc", job, SELEM, ms)[1]
    files.scale_absorbed(want, c, run.U.GL, run.U.NNNLIMIT, 1)
    assert want.max() > 0 and _bits(r["absorbed"], want)
    assert r["stats"]["splits"] > 0 and r["stats"]["max_depth"] <= 40


def test_split_normalisation_on_a_fully_refined_model(tmp_path):
    """Total absorbed energy of a `split 1` run against `split 0` runs on a uniform model whose root cells are all refined once:
    every root ray splits at birth into four of a quarter of its weight, so the two runs estimate the same energy.  The standard
    error comes from 8 seeds of the plain run; 5 sigma, since a wrong WBG or a lost factor 4 is off by tens of percent.
    Observed: split 9.4788e+00, plain mean 9.4386e+00 +- 4.2e-02 (one run), difference 0.95 sigma."""
    c = sc.model("full4")
    assert c.LEVELS == 2 and (c.DENS[:64] <= 0).all()

    def total(eng, sub, split, seed):
        r = run_ini(eng, tmp_path / sub, split=split, cloud=c, bgpackets=3000, seed=seed)
        lev = c.level_of_cells()
        leaf = c.DENS > 0
        # scale_absorbed divides by the cell volume: weigh the cells back to energies
        return float((r["absorbed"][leaf].astype(np.float64).sum(axis=1) * 8.0 ** (-lev[leaf])).sum())
    plain = [total(OracleEngine("soc"), "p%d" % k, 0, 0.05 + 0.11 * k) for k in range(8)]
    split = total(SplitOracleEngine("soc"), "s", 1, 0.4321)
    mean, sd = float(np.mean(plain)), float(np.std(plain, ddof=1))
    print("split %.4e  plain mean %.4e +- %.1e (one run)  difference %.2f sigma" % (split, mean, sd, (split - mean) / sd))
    # the difference of one split run and the mean of 8 plain ones: variance sd^2 (1 + 1/8), the split run's taken as the plain run's
    assert abs(split - mean) <= 5.0 * sd * np.sqrt(1.0 + 1.0 / 8.0)
