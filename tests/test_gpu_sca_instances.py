"""Every compiled instance of the direct scattered-light kernel, soc_sca_kernel<OCT, DBL, ABU, KIND> (soc_amd/csrc/soc_sca.hip: 32), run
once against the oracle in soc mode, and twelve more launches on the paths the 8^3 cases never took: a Healpix image seen from inside
a five-level hierarchy for every kind, reflecting faces on a hierarchy, and the boundary of soc_grid_variant's rule.  The cases, their
grids and what they must keep true are tests/sca_instance_cases.py; the oracle is pinned bit for bit to the reference's kernel on every
one of them (tests/test_sca_instances.py).  Each case runs with soc_set_exec(0) and asserts that no sweep ran, that soc_last_variant
names the instance (bit 15: a launch of this kernel), that image contributions, packets and scatterings equal the oracle's, and that
the image passes test_gpu_sca.assert_image_close at rtol 1e-5.  The instances with Index() in double run first: nothing else runs 15
of those 16.  What tells such an instance from one that walks in float is the image (and often the counts): sca_instance_cases.problems.
Reads only the repository.

Observed on one MI355X (each case prints its figure): every event count equal to the oracle's in all 44 cases; the largest relative
difference of a lit pixel is 1.6e-7 to 3.5e-6 over the 32 instances (the eight on the five-level hierarchy with Index() in double:
8.7e-7 to 2.8e-6) and 4.7e-7 to 1.9e-6 over the twelve further cases.  The float walk on the CPU moves 4 to 21 pixels of those eight
past the bar (sca_instance_cases' docstring has every figure).  The module takes 3.6 s, 2.0 s of it the oracle's results of all cases.
With all 1024 work items of the SimRAM_CL launches on that hierarchy (2e5 to 4e5 contributions, thousands per pixel) two cases missed
the bar by one pixel each, 1.1e-5 and 2.0e-5, with every count equal: the order of the fp32 sums, which moves the oracle's own image
by 7e-6 between one thread and eight.  Those four launches run their first 64 to 256 work items instead."""
import numpy as np
import pytest

import sca_instance_cases as si
from test_gpu_sca import assert_image_close, run_sca
from util import run_engine

pytestmark = pytest.mark.gpu

# the double-Index() instances first, the five-level hierarchy before the single-level grid
ORDER = sorted(si.REACHABLE, key=lambda k: (-k[2], -k[1], k[0], k[3]))


@pytest.fixture(scope="module")
def want():
    """the oracle's result of every case (soc mode, 8 threads), computed once"""
    return {key: si.expected(key) for key in si.CASES}


def _launch(engine, key, gid_count=None):
    g0, n = si.items(key)
    engine.set_exec(0, 4)
    try:
        got, st = run_sca(engine, si.job(key), si.view(key), si.CASES[key]["kind"], g0, n if gid_count is None else gid_count)
        assert engine.last_passes() == 0
    finally:
        engine.set_exec(-1, 4)
    return got, st


def _worst(got, ref):
    """largest relative difference over the lit pixels"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    m = ref > 0
    return float((np.abs(got[m] - ref[m]) / ref[m]).max())


def _check(engine, want, key):
    got, st = _launch(engine, key)
    v = engine.last_variant()
    assert (v["sca"], v["form"], v["kind"], v["octree"], v["dbl"], v["abu"]) == (1, 0) + si.instance(key), v
    assert (v["split"], v["rays"], v["wint"]) == (0, 0, 0)
    img, nadd, npkt, nscat = want[key]
    print(si.case_id(key), "gpu", st, "oracle", (nadd, npkt, nscat))
    assert (st["tally_events"], st["packets"], st["scatterings"]) == (nadd, npkt, nscat)
    assert nadd >= si.MIN_CONTRIBUTIONS and nscat >= si.MIN_SCATTERINGS
    print(si.case_id(key), "largest relative pixel difference %.2e" % _worst(got, img))
    assert_image_close(got, img)


@pytest.mark.parametrize("key", ORDER, ids=[si.case_id(k) for k in ORDER])
def test_instance_equals_the_oracle(engine, want, key):
    assert si.instance(key) == key
    _check(engine, want, key)


@pytest.mark.parametrize("key", list(si.EXTRA))
def test_further_paths_equal_the_oracle(engine, want, key):
    _check(engine, want, key)


def test_plain_launch_after_a_scattered_light_launch_reports_no_sca(engine):
    import split_cases as sc
    _launch(engine, (si.CL, 1, 0, 1))
    v = engine.last_variant()
    assert (v["sca"], v["kind"], v["octree"], v["abu"]) == (1, si.CL, 1, 1)
    run_engine(engine, sc.job("oct4b")[0])
    v = engine.last_variant()
    assert (v["sca"], v["split"], v["form"], v["kind"], v["octree"], v["wint"]) == (0, 0, 0, 0, 1, 1), v


def test_launch_without_work_items_leaves_the_variant(engine):
    import split_cases as sc
    run_engine(engine, sc.job("oct4b")[0])
    plain = engine.last_variant()
    assert plain["sca"] == 0
    for key in ((si.BG, 1, 0, 0), (si.HP, 0, 0, 1)):
        _, st = _launch(engine, key, gid_count=0)
        assert st["packets"] == 0 and engine.last_variant() == plain
    # and one scattered-light launch is not taken for another's
    _launch(engine, (si.PS, 1, 0, 1))
    ps = engine.last_variant()
    assert (ps["sca"], ps["kind"], ps["octree"], ps["dbl"], ps["abu"]) == (1, si.PS, 1, 0, 1)
    _launch(engine, (si.BG, 0, 0, 0), gid_count=0)
    assert engine.last_variant() == ps


def test_a_sweep_of_rays_reports_rays_not_sca(engine, want):
    key = (si.BG, 1, 1, 0)
    g0, n = si.items(key)
    _launch(engine, key)
    assert engine.last_variant()["sca"] == 1
    engine.set_exec(1, 4)
    try:
        got, st = run_sca(engine, si.job(key), si.view(key), si.BG, g0, n)
        v = engine.last_variant()
        assert engine.last_passes() > 0 and engine.last_form() == 3
    finally:
        engine.set_exec(-1, 4)
    assert (v["rays"], v["sca"], v["octree"], v["dbl"]) == (1, 0, 1, 1), v
    assert st["tally_events"] == want[key][1]
    assert_image_close(got, want[key][0])
