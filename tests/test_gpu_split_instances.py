"""Every compiled instance of the two packet-splitting kernels that a launch can reach, run once against the CPU restatement.

soc_split.hip compiles soc_sim_bg_split_kernel and soc_sim_hp_split_kernel as <OCT, DBL, ABU, WINT>: 16 instances each, picked by
soc_split_key (soc_dev.h).  Cartesian grids clear DBL, so 12 of each can run; REACHABLE lists them and CASES holds one launch per
entry.  soc_last_variant names the instance that ran (bit 14: a split launch).  Each case asserts the instance, all counters and the
largest stack depth equal to the restatement's in soc mode (tests/split_host.py, tests/hpsplit_host.py: pinned bit for bit to the
reference, on a hierarchy with Index() in double too -- tests/test_split.py, tests/test_hpsplit.py), and every tally the instance
writes equal to the restatement's to the order of the atomic adds (rtol 1e-5): the trajectories are the same, lane by lane.  The
tallies are what tells a DBL instance that walks in float from one that does not: the counters of such a walk stay the same
(test_x104_tells_a_float_walk_from_a_double_one in the two CPU modules).  Reads only the repository.

Observed on one MI355X (each case prints its figure): the largest relative tally difference over cells above 1e-3 of the largest
tally is 2.4e-7 to 8.4e-7 over the 24 instances (double hierarchy: background 4.1e-7 to 4.5e-7, sky 4.0e-7 to 8.3e-7), INT as TABS;
the module takes 2.8 s, 2.2 s of it the restatement's results of all cases."""
import numpy as np
import pytest

import hpsplit_cases as hc
import hpsplit_host
import split_cases as sc
import split_host
from hpsplit_engine import run_hp_split
from oracle.pyoracle import Job
from soc_amd import files, synth
from split_engine import run_split
from util import assert_tally_close, run_engine

BG, HP = "bg", "hp"                                     # soc_sim_bg_split_kernel (kind 0), soc_sim_hp_split_kernel (kind 1)
KIND = {BG: 0, HP: 1}
GRIDS = {(0, 0): "cart", (1, 0): "oct4b", (1, 1): "x104"}     # (octree, dbl): Cartesian, hierarchy with Index() in float / in double

# (kernel, octree, dbl, abu, wint).  Excluded: dbl without octree -- a Cartesian grid's Index() has no double arithmetic, soc_split_key clears it
REACHABLE = {(k, o, d, a, w) for k in (BG, HP) for (o, d) in GRIDS for a in (0, 1) for w in (0, 1)}

KEYS = split_host.COUNTERS + ("max_depth",)
HP_KEYS = hpsplit_host.COUNTERS + ("max_depth", "skipped_splits")

_MEMO = {}


def _cloud(grid):
    if grid not in _MEMO:
        _MEMO[grid] = synth.cartesian_cloud(5, seed=4, NY=4, NZ=3) if grid == "cart" else sc.model(grid)
    return _MEMO[grid]


def _case(kernel, octree, dbl, abu, wint):
    """The launch of one entry.  Cartesian: the model and SELEM of test_cartesian_grid_never_splits at opacities where packets
    scatter, the sky launch with one work item per surface element (94: a wave and a partial one); float hierarchy: oct4b with the
    launches of the shared case tables; double hierarchy: their x104 launches.  The sky is plain or weighted in turn."""
    grid = GRIDS[(octree, dbl)]
    k = dict(grid=grid, abu=abu, wint=wint, max_split=64, ABS=1e-4, SCA=3e-4, SEED=0.2891, SELEM=1, BATCH=2)
    if grid == "cart":
        k.update(max_split=14, ABS=1e-2, SCA=3e-2, SEED=0.37, SELEM=2, BATCH=3)
    elif grid == "x104":
        k.update(SELEM=2)
    if kernel == HP:
        k.update(BATCH=3, GLOBAL={"cart": _cloud("cart").AREA, "oct4b": 96, "x104": 1024}[grid], weighted=(abu + wint) % 2)
    else:
        k.update(GLOBAL=sc.launch_shape(_cloud(grid).AREA, k["SELEM"]))
    return k


CASES = {key: _case(*key) for key in REACHABLE}
# the double-Index() instances first: the ones nothing else runs
ORDER = sorted(CASES, key=lambda key: (-key[2], -key[1], key[0], key[3], key[4]))


def _job(key):
    k = CASES[key]
    c = _cloud(k["grid"])
    kw = dict(ABS=k["ABS"], SCA=k["SCA"], SOURCE=1, BATCH=k["BATCH"], SEED=k["SEED"], GLOBAL=k["GLOBAL"], WITH_INT=k["wint"])
    if k["abu"]:
        kw["OPT"] = sc.per_cell_opt(c, k["ABS"], k["SCA"])
    if key[0] == HP:
        HPBG, HPBGP = files.hpbg_for_frequency(hc.sky(2 + k["weighted"]), 1.0, k["weighted"])
        kw.update(BG=0.0, HPBG=HPBG, HPBGP=HPBGP)
    return Job(c, sc._CSC, **kw)


def _restatement(key):
    k = CASES[key]
    if key[0] == HP:
        return hpsplit_host.sim_hp_split("soc", _job(key), k["max_split"])
    return split_host.sim_bg_split("soc", _job(key), k["SELEM"], k["max_split"])


def _launch(engine, key, gid_first=0, gid_count=None):
    k = CASES[key]
    if key[0] == HP:
        return run_hp_split(engine, _job(key), k["max_split"], gid_first, gid_count)
    return run_split(engine, _job(key), k["SELEM"], k["max_split"], gid_first, gid_count)


def _worst(got, ref):
    """largest relative difference over the cells above 1e-3 of the largest tally"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = ref > 1e-3 * ref.max()
    return float((np.abs(got[m] - ref[m]) / ref[m]).max())


@pytest.fixture(scope="module")
def want():
    """the restatement's result of every case, computed once"""
    return {key: _restatement(key) for key in CASES}


def test_the_cases_are_the_reachable_instances():
    assert set(CASES) == REACHABLE and len(REACHABLE) == 24
    assert {k for k, *_ in REACHABLE} == {BG, HP} and not any(d and not o for _, o, d, _, _ in REACHABLE)
    # what makes the key on the host: the grids are the ones soc_grid_variant tells apart (soc_dev.h: NX > 100 with three levels or more)
    for (o, d), grid in GRIDS.items():
        c = _cloud(grid)
        assert (int(c.LEVELS > 1), int(c.LEVELS > 1 and c.NX > (399 if c.LEVELS < 3 else 100))) == (o, d), grid
    assert {CASES[k]["weighted"] for k in CASES if k[0] == HP and k[2]} == {0, 1}
    assert ORDER[0][2] == 1 and [k[2] for k in ORDER] == sorted((k[2] for k in ORDER), reverse=True)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ORDER, ids=["-".join(map(str, k)) for k in ORDER])
def test_instance_equals_the_restatement(engine, want, key):
    kernel, octree, dbl, abu, wint = key
    k = CASES[key]
    TABS, INT, _, st = _launch(engine, key)
    v = engine.last_variant()
    assert (v["split"], v["form"], v["kind"], v["wint"], v["octree"], v["dbl"], v["abu"]) == (1, 0, KIND[kernel], wint, octree, dbl, abu), v
    wT, wI, _, wst = want[key]
    keys = HP_KEYS if kernel == HP else KEYS
    print(key, "gpu", {n: st[n] for n in keys}, "restatement", {n: wst[n] for n in keys})
    assert {n: st[n] for n in keys} == {n: wst[n] for n in keys}
    assert wT.max() > 0
    print(key, "largest relative difference: TABS %.2e" % _worst(TABS, wT), ("INT %.2e" % _worst(INT, wI)) if wint else "")
    assert_tally_close(TABS, wT, rtol=1e-5)
    if wint:
        assert wI.max() > 0
        assert_tally_close(INT, wI, rtol=1e-5)
    else:
        assert not INT.any() and not wI.any()
    if dbl:
        assert st["splits"] >= (500 if kernel == HP else 1000)
    elif octree:
        assert st["splits"] >= 50
    else:
        assert st["splits"] == 0 and st["max_depth"] == 0 and st["roots"] == k["BATCH"] * _cloud("cart").AREA
        assert wst["stop20"] > 0                    # packets scatter: the walk's scattering branch runs on this grid too


@pytest.mark.gpu
def test_plain_launch_after_a_split_launch_reports_no_split(engine):
    for key in ((BG, 1, 0, 0, 1), (HP, 1, 0, 0, 1)):
        _launch(engine, key)
        assert engine.last_variant()["split"] == 1 and engine.last_variant()["kind"] == KIND[key[0]]
        job = sc.job("oct4b")[0]
        run_engine(engine, job)
        v = engine.last_variant()
        assert (v["split"], v["form"], v["kind"], v["octree"], v["wint"]) == (0, 0, 0, 1, 1), v


@pytest.mark.gpu
def test_split_launch_without_work_items_leaves_the_variant(engine):
    run_engine(engine, sc.job("oct4b")[0])
    plain = engine.last_variant()
    assert plain["split"] == 0
    for key in ((BG, 1, 0, 1, 0), (HP, 1, 0, 1, 0)):
        st = _launch(engine, key, 0, 0)[3]
        assert st["roots"] == 0 and engine.last_variant() == plain
    # and one split launch is not taken for the other's
    _launch(engine, (BG, 1, 0, 1, 0))
    bg = engine.last_variant()
    assert (bg["split"], bg["kind"], bg["abu"], bg["wint"]) == (1, 0, 1, 0)
    _launch(engine, (HP, 1, 0, 0, 1), 0, 0)
    assert engine.last_variant() == bg
