"""Packet splitting with a Healpix sky (`split 1` + `hpbg`, SimHpSplit) without a GPU: the CPU restatement against the recorded
reference (tests/golden/hpsplit.npz, tools/make_hpsplit_golden.py), the launch arithmetic, the ini handling and the driver on a
test engine that runs the launches through the restatement."""
import os

import numpy as np
import pytest

import hpsplit_cases as hc
import hpsplit_host
import split_cases as sc
from hpsplit_engine import HpSplitOracleEngine
from hpsplit_ini import SKY_SCALE, run_hp_ini, sky_rows
from oracle_engine import OracleEngine
from split_engine import SplitOracleEngine
from split_ini import FREQ, write_model
from soc_amd import files, launch
from soc_amd.asoc import AbsorptionRun, UnsupportedOption
from soc_amd.ini import User

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpsplit.npz")
STATS = hpsplit_host.COUNTERS + hpsplit_host.EXTRA


@pytest.fixture(scope="module")
def libm():
    return {name: hpsplit_host.sim_hp_split("libm", *hc.job(name)) for name in hc.CASES}


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_restatement_equals_the_reference_bit_for_bit(libm, name):
    g = np.load(GOLDEN)
    TABS, INT, INTV, st = libm[name]
    assert g["TABS_" + name].max() > 0
    assert _bits(TABS, g["TABS_" + name]) and _bits(INT, g["INT_" + name])
    if hc.CASES[name]["variant"] == "int2":
        assert _bits(INTV, g["INTV_" + name]) and np.abs(INTV).max() > 0
    assert [st[k] for k in STATS] == list(g["stats_" + name])
    assert st["guard"] == 0                        # the condition under which the reference stays inside its slab


def test_golden_is_of_these_cases():
    assert str(np.load(GOLDEN)["meta"]) == hc.meta()


def test_cases_cover_every_branch(libm):
    st = {n: r[3] for n, r in libm.items()}
    assert hc.coverage(st) == []
    assert st["oct4b"]["initial"] > 0 and st["kat"]["deep_splits"] > 0 and st["oct4b_opaque"]["stop20"] > 0
    assert all(s["ended_below_RL"] > 0 for s in st.values())
    assert st["jump3_ms17"]["skipped_splits"] > 0 and st["jump3_ms17"]["overflow_drops"] > 0
    assert st["kat_ms14"]["skipped_replicas"] > 0 and st["kat_ms14"]["guard"] == 0
    assert all(s["long_returns"] == 0 and s["guard"] == 0 for s in st.values())
    # every work item sends its BATCH rays: nobody returns at id >= 8*AREA or at an element >= AREA
    assert all(s["roots"] == hc.CASES[n]["GLOBAL"] * hc.CASES[n]["BATCH"] for n, s in st.items())
    assert {k["GLOBAL"] for n, k in hc.CASES.items() if k["model"] != "x104"} == {hc.GLOBAL} == {96}


def test_soc_mode_follows_the_same_trajectories(libm):
    """the two math modes differ in the last bits of exp, log, sin, cos only: same events unless a free path lands within those.
    Counters are equal in all cases.  The tallies are compared, at test_split.py's tolerance, on an unweighted case with a deep jump,
    a weighted one and the small-stack one; in two other cases (oct4b_abu, oct6_w) single cells that a ray only clips differ by up to
    1.4e-5 of the largest tally, since here the sine and cosine also set the direction of every root ray."""
    for name in hc.CASES:
        st = hpsplit_host.sim_hp_split("soc", *hc.job(name))[3]
        assert {k: st[k] for k in STATS} == {k: libm[name][3][k] for k in STATS}, name
    for name in ("kat", "oct4b_w", "jump3_ms17"):
        job, ms = hc.job(name)
        T, _, _, st = hpsplit_host.sim_hp_split("soc", job, ms)
        assert {k: st[k] for k in STATS} == {k: libm[name][3][k] for k in STATS}
        assert np.allclose(T, libm[name][0], rtol=1e-4, atol=1e-6 * T.max())


def test_x104_tells_a_float_walk_from_a_double_one(monkeypatch):
    """As test_split.py's: with Index() in float the x104 launch (1024 work items x 3 rays) must move many cells' tallies by more
    than the GPU tests' rtol 1e-5.  Observed: 148 cells of 4262, largest relative difference 9.6e-4."""
    import oracle.pyoracle
    job, ms = hc.job("x104")
    assert oracle.pyoracle.double_index(job.cloud.NX, job.cloud.LEVELS) == 1 and job.GLOBAL == 1024
    n, of = sc.float_walk_differs(lambda: hpsplit_host.sim_hp_split("soc", *hc.job("x104"))[0], monkeypatch)
    print("x104: %d of %d cells differ by more than 1e-5 when Index() runs in float" % (n, of))
    assert n >= 50


def test_half_ranges_sum_to_the_launch(libm):
    name = "oct4b_w"
    job, ms = hc.job(name)
    a = hpsplit_host.sim_hp_split("libm", job, ms, 0, 64)
    TABS, INT, _, b = hpsplit_host.sim_hp_split("libm", hc.job(name)[0], ms, 64, None, TABS=a[0], INT=a[1])
    assert _bits(TABS, libm[name][0]) and _bits(INT, libm[name][1])     # one thread, id order: the very same sequence of adds
    assert all(a[3][k] + b[k] == libm[name][3][k] for k in hpsplit_host.COUNTERS + ("skipped_splits", "skipped_replicas"))


def test_launch_arithmetic():
    """ASOC.py:311-315 and :1050-1059 by hand"""
    P = launch.PLANCK
    # config-3-like: 256^3 roots, AREA = 393216 = 12 * 32768: SELEM 12, GLOBAL_SPLIT = Fix(32769, 32) = 32800 = 1025 * 32, an odd multiple
    # of 32: the weight counts Fix(32800, 64) = 32832 work items, 32 more than are launched
    L = launch.hp_split_launch(2000000, 256, 256, 256, 393216)
    assert (L["GLOBAL"], L["GLOBAL_W"], L["BATCH"], L["PACKETS"]) == (32800, 32832, 100, 3283200)
    assert L["WBG"] == (np.pi / P) / ((32832 * 100) / (2 * 3 * 65536))
    # oct4b / full4: 4^3 roots, AREA 96: GLOBAL_SPLIT = Fix(97, 32) = 128 = GLOBAL_W
    L = launch.hp_split_launch(300, 4, 4, 4, 96)
    assert (L["GLOBAL"], L["GLOBAL_W"], L["BATCH"], L["PACKETS"]) == (128, 128, 100, 12800)
    assert L["WBG"] == (np.pi / P) / (12800 / 96)
    # 5 x 4 x 3: AREA 94 -> Fix(95, 32) = 96 launched, the weight counts 128
    L = launch.hp_split_launch(300, 5, 4, 3, 94)
    assert (L["GLOBAL"], L["GLOBAL_W"], L["PACKETS"]) == (96, 128, 12800) and L["WBG"] == (np.pi / P) / (12800 / 94)
    # LOCAL 8 (a CPU device): AREA 96 -> Fix(97, 8) = 104 launched, 128 counted
    L = launch.hp_split_launch(300, 4, 4, 4, 96, LOCAL=8)
    assert (L["GLOBAL"], L["GLOBAL_W"]) == (104, 128)
    # the work items launched are bg_split_launch's
    assert launch.bg_split_launch(2000000, 393216)["GLOBAL"] == 32800


@pytest.mark.parametrize("weighted", [0, 1])
def test_ini_run_equals_tallies_composed_by_hand(tmp_path, weighted):
    """`split 1` + `hpbg sky 1.0 <weighted>` on the test engine: the launches are the hand-worked ones, the sky is the plain Healpix
    run's with this launch's WBG, packet.info carries the rounded BGPAC (what ASOC.py:251 writes for this combination: the file is
    written before the launch loop recomputes BGPAC), and the absorbed file holds the INT tallies of the same launches of the
    restatement, scaled as the plain run's"""
    from oracle.pyoracle import Job
    c = sc.model("oct4b")
    eng = HpSplitOracleEngine("soc")
    r = run_hp_ini(eng, tmp_path / "a", weighted, extra="maxsplit 40\n", bgpackets=300)
    L = launch.hp_split_launch(384, 4, 4, 4, c.AREA)
    assert (L["GLOBAL"], L["GLOBAL_W"], L["BATCH"]) == (128, 128, 100)
    assert list(r["packet_info"]) == [launch.Fix(launch.Fix(300, 96), 32), 0, 0, 0] == [384, 0, 0, 0]
    assert len(eng.hp_split_launches) == len(FREQ) and eng.split_launches == []
    run = r["run"]
    rows = sky_rows()
    want = np.zeros((c.CELLS, len(FREQ)), np.float32)
    for k, (BATCH, SEED, TW, ms, GLOBAL, first, count, HPBG, HPBGP) in enumerate(eng.hp_split_launches):
        assert (BATCH, ms, GLOBAL, first, count) == (100, 40, 128, 0, 128)
        assert SEED == pytest.approx(launch.launch_seed(0.7853981634, k))
        sky = files.hpbg_for_frequency(rows[k], L["WBG"] / float(run.FFREQ[k]), weighted)
        assert _bits(HPBG, sky[0]) and ((HPBGP is None and sky[1] is None) if not weighted else _bits(HPBGP, sky[1]))
        job = Job(c, run.FCSC[0, k, :], ABS=np.float32(run.AFABS[0][k]), SCA=np.float32(run.AFSCA[0][k]), SOURCE=1, BATCH=BATCH, SEED=SEED,
                  BG=0.0, TW=TW, GLOBAL=GLOBAL, WITH_INT=1, HPBG=HPBG, HPBGP=HPBGP)
        want[:, k] = hpsplit_host.sim_hp_split("soc", job, ms)[1]
    files.scale_absorbed(want, c, run.U.GL, run.U.NNNLIMIT, 1)
    assert want.max() > 0 and _bits(r["absorbed"], want)
    assert r["stats"]["splits"] > 0 and r["stats"]["max_depth"] <= 40 and r["stats"]["roots"] == 3 * 12800


def test_an_empty_weighted_sky_skips_the_frequency(tmp_path):
    eng = HpSplitOracleEngine("soc")
    d = tmp_path / "e"
    os.makedirs(str(d))
    rows = sky_rows()
    rows[1] = 0.0
    path = os.path.join(str(d), "sky0.bin")
    rows.tofile(path)
    from split_ini import run_ini
    r = run_ini(eng, d, split=1, extra="hpbg %s 1.0 1\n" % path)
    assert len(eng.hp_split_launches) == len(FREQ) - 1
    assert r["absorbed"][:, 1].max() == 0 and r["absorbed"][:, 0].max() > 0


def _refused(tmp_path, engine, extra, text, sub):
    np.ones((len(FREQ), 49152), np.float32).tofile(str(tmp_path / "sky.bin"))
    ini = write_model(tmp_path / sub, sc.model("oct4b"), "split 1\nhpbg %s/sky.bin 1.0 0\n" % tmp_path + extra)
    with pytest.raises(UnsupportedOption) as e:
        AbsorptionRun(User(ini), engine, verbose=0)
    assert text in str(e.value), str(e.value)


def test_ini_refusals(tmp_path):
    eng = HpSplitOracleEngine("soc")
    _refused(tmp_path, eng, "mirror xX\n", "split with mirror", "c")
    _refused(tmp_path, eng, "stepweight 2 0.5 1\n", "split with stepweight", "d")
    _refused(tmp_path, eng, "roi 1 2 1 2 1 2\nroisave %s/roi.save 1\n" % tmp_path, "split with roisave", "e")
    _refused(tmp_path, eng, "maxsplit 10\n", "maxsplit 10", "f")
    _refused(tmp_path, SplitOracleEngine("soc"), "", "SimHpSplit", "g")
    _refused(tmp_path, SplitOracleEngine("soc"), "", "this engine has no sim_hp_split", "h")
    # and the same ini file runs on an engine that has the call
    AbsorptionRun(User(write_model(tmp_path / "i", sc.model("oct4b"), "split 1\nhpbg %s/sky.bin 1.0 0\n" % tmp_path)), eng, verbose=0)


def test_split_normalisation_on_a_fully_refined_model(tmp_path):
    """Total absorbed energy of a `split 1` run against `split 0` runs with the same uniform Healpix sky on a uniform model whose root
    cells are all refined once (GLOBAL_SPLIT = Fix(97, 32) = 128 = GLOBAL_W, and the plain launch has 64 <= 8*AREA work items, so nobody
    returns early): every root ray splits at birth into four of a quarter of its weight, so the two runs estimate the same energy.
    The standard error comes from 8 seeds of the plain run; 5 sigma x sqrt(1 + 1/8).
    Observed: split 6.4143e+00, plain mean 6.3836e+00 +- 4.0e-02 (one run), difference 0.77 sigma."""
    c = sc.model("full4")
    assert c.LEVELS == 2 and (c.DENS[:64] <= 0).all()
    L = launch.hp_split_launch(3000, 4, 4, 4, c.AREA)
    assert L["GLOBAL"] == L["GLOBAL_W"] == 128
    assert launch.hpbg_launch(launch.packet_counts(3000, 0, 0, 0, c.AREA, c.CELLS)["BGPAC"], 4, 4, 4)["GLOBAL"] <= 8 * c.AREA
    d = tmp_path / "sky"
    os.makedirs(str(d))
    path = os.path.join(str(d), "uniform.bin")
    np.full((len(FREQ), 49152), SKY_SCALE, np.float32).tofile(path)
    from split_ini import run_ini

    def total(eng, sub, split, seed):
        r = run_ini(eng, tmp_path / sub, split=split, cloud=c, extra="hpbg %s 1.0 0\n" % path, bgpackets=3000, seed=seed)
        lev = c.level_of_cells()
        leaf = c.DENS > 0
        # scale_absorbed divides by the cell volume: weigh the cells back to energies
        return float((r["absorbed"][leaf].astype(np.float64).sum(axis=1) * 8.0 ** (-lev[leaf])).sum())
    plain = [total(OracleEngine("soc"), "p%d" % k, 0, 0.05 + 0.11 * k) for k in range(8)]
    split = total(HpSplitOracleEngine("soc"), "s", 1, 0.4321)
    mean, sd = float(np.mean(plain)), float(np.std(plain, ddof=1))
    print("split %.4e  plain mean %.4e +- %.1e (one run)  difference %.2f sigma" % (split, mean, sd, (split - mean) / sd))
    # the difference of one split run and the mean of 8 plain ones: variance sd^2 (1 + 1/8), the split run's taken as the plain run's
    assert abs(split - mean) <= 5.0 * sd * np.sqrt(1.0 + 1.0 / 8.0)
