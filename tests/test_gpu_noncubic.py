"""The walk kernels on hierarchies whose three sides differ (synth.NONCUBIC): oct759 (7 x 5 x 9), oct104x6x5 (NX > 100: Index() in
double, the only one of the three the engine walks brick-locally) and oct6x104x5 (NY > 100 but NX is not: Index() stays in float).
The bar is the one of tests/test_gpu_ltree.py: identical trajectories (tally-event counts equal to the oracle's), tallies equal to
fp32 summation order (assert_tally_close, rtol 1e-5).  The oracle is pinned bit for bit to the reference on these grids
(tests/test_oracle_vs_ref.py, tests/golden/sims.npz).

Forms: the direct kernels (soc_set_exec 0, form 0) and the brick sweep (soc_set_exec 1): brick-local (form 3) where Index() runs in
double, the hierarchy in global memory (form 2) elsewhere and where `global_tree` asks for it.  Every case prints its event count
and the largest relative tally difference (over cells above 1e-3 of the largest tally)."""
import numpy as np
import pytest

import cases
import hpsplit_cases as hc
import hpsplit_host
import split_cases as sc
import split_host
from hpsplit_engine import run_hp_split
from oracle.pyoracle import Job, ScaView, oracle_sim_sca
from soc_amd import launch, synth
from split_engine import run_split
from test_gpu_sca import assert_image_close, run_sca
from util import assert_tally_close, run_engine

pytestmark = pytest.mark.gpu

MODELS = ["oct759", "oct104x6x5", "oct6x104x5"]
BRICK_LOCAL = {"oct759": False, "oct104x6x5": True, "oct6x104x5": False}     # soc_brick_local: Index() in double
_MEMO = {}


def cloud(name):
    if name not in _MEMO:
        _MEMO[name] = synth.noncubic_cloud(name)
    return _MEMO[name]


def oracle(orc, key, job, kind, **kw):
    """the oracle's (TABS, INT, events) of a launch: computed once per session, shared by the forms, never changed"""
    if key not in _MEMO:
        T, I, n = orc.sim(job, kind, nthreads=8, **kw)
        T.setflags(write=False)
        I.setflags(write=False)
        _MEMO[key] = (T, I, n)
    return _MEMO[key]


def opacities(cl):
    """about one optical depth of scattering along the shortest side, so that packets scatter a few times before they leave"""
    mean = float(cl.DENS[:cl.NX * cl.NY * cl.NZ][cl.DENS[:cl.NX * cl.NY * cl.NZ] > 0].mean())
    k = 1.0 / (min(cl.NX, cl.NY, cl.NZ) * mean)
    return np.float32(0.1 * k), np.float32(k)


def sources(name):
    """{source: (kind, Job, gid0, gid1)}: background (the whole launch of the slabs is 18 784 work items), a point source inside and one
    outside, cell emission"""
    cl = cloud(name)
    a, s = opacities(cl)
    N = np.asarray([cl.NX, cl.NY, cl.NZ], np.float32)
    ps = np.stack([N * np.asarray([0.52, 0.47, 0.55], np.float32), N * np.asarray([0.5, 0.5, 0.5], np.float32) + np.asarray([0, 0, 3.0 * cl.NZ], np.float32)])
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    G = 8 * cl.AREA
    return {
        "bg": (0, Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=1, BATCH=3, SEED=0.377), 0, min(G, 4000)),
        "bg_end": (0, Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=1, BATCH=2, SEED=0.52), max(0, G - 3000), G),
        "ps": (0, Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=0, BATCH=10, SEED=0.2, GLOBAL=512, PSPOS=ps, PS=[1.0, 2.5], PS_METHOD=0, WITH_INT=1, TW=1.5), 0, 512),
        "cl": (1, Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=2, BATCH=1, SEED=0.9, GLOBAL=1024, EMIT=emit), 0, 1024),
    }


def report(tag, got, want, n):
    want = np.asarray(want, np.float64)
    sig = want > 1e-3 * want.max()
    rel = float((np.abs(np.asarray(got, np.float64) - want)[sig] / want[sig]).max())
    print("%-40s events %8d   largest relative tally difference %.3e" % (tag, n, rel))


def check(engine, oracle_soc, name, src, exec_mode, form):
    kind, job, g0, g1 = sources(name)[src]
    T, I, n = oracle(oracle_soc, (name, src), job, kind, gid0=g0, gid1=g1)
    assert n > 1000 and (T > 0).sum() > 900                    # (oct759 has 1036 leaves)
    Tg, Ig, st = run_engine(engine, job, kind, gid_first=g0, gid_count=g1 - g0, exec_mode=exec_mode)
    assert engine.last_form() == form, (engine.last_form(), form)
    assert (engine.last_passes() > 0) == (form > 0)
    report("%s %s form %d" % (name, src, form), Tg, T, st["tally_events"])
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert_tally_close(Tg, T, rtol=1e-5)
    if job.WITH_INT:
        assert_tally_close(Ig, I, rtol=1e-5)
    engine.set_features(0, 0, 0)
    engine.set_exec(-1, 4)


@pytest.mark.parametrize("src", ["bg", "bg_end", "ps", "cl"])
@pytest.mark.parametrize("name", MODELS)
def test_direct_kernels(name, src, engine, oracle_soc):
    check(engine, oracle_soc, name, src, 0, 0)


@pytest.mark.parametrize("src", ["bg", "bg_end", "ps", "cl"])
@pytest.mark.parametrize("name", MODELS)
def test_sweep_with_the_hierarchy_in_global_memory(name, src, engine, oracle_soc, tuned):
    tuned(global_tree=1)
    check(engine, oracle_soc, name, src, 1, 2)


@pytest.mark.parametrize("src", ["bg", "bg_end", "ps", "cl"])
@pytest.mark.parametrize("name", MODELS)
def test_sweep_in_the_form_the_engine_chooses(name, src, engine, oracle_soc):
    """brick-local (form 3) for oct104x6x5; the other two grids evaluate Index() in float, which the brick-local walk does not restate"""
    check(engine, oracle_soc, name, src, 1, 3 if BRICK_LOCAL[name] else 2)


# brick_cells 100: the tiles of oct104x6x5 (16 x 6 x 5 root cells, 8 x 6 x 5 at the far x face) are halved along x, y and z down to
# bricks of 4 x 3 x 5, 4 x 3 x 2, 2 x 3 x 3 ... root cells, three different extents (tests/test_ltree.py asserts that on the host
# builder); 12288: every tile is one brick
@pytest.mark.parametrize("src", ["bg", "ps", "cl"])
@pytest.mark.parametrize("cells", [100, 12288])
def test_brick_local_walk_at_two_brick_sizes(cells, src, engine, oracle_soc, tuned):
    tuned(brick_cells=cells)
    check(engine, oracle_soc, "oct104x6x5", src, 1, 3)


@pytest.mark.parametrize("tune", [dict(), dict(brick_cells=100), dict(slow_every=3)], ids=["defaults", "cells100", "slow3"])
def test_per_cell_opacities_on_the_brick_local_walk(tune, engine, oracle_soc, tuned):
    """abu_local on oct104x6x5, as tests/test_gpu_ltree_abu.py has it on the cube"""
    cl = cloud("oct104x6x5")
    a, s = opacities(cl)
    rr = np.random.default_rng(11)
    opt = np.zeros((cl.CELLS, 2), np.float32)
    opt[:, 0] = a * rr.uniform(0.5, 2, cl.CELLS)
    opt[:, 1] = s * rr.uniform(0.5, 2, cl.CELLS)
    job = Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=1, BATCH=3, SEED=0.377, OPT=opt)
    g0, g1 = 2000, 6000
    T, _, n = oracle(oracle_soc, "abu", job, 0, gid0=g0, gid1=g1)
    n_scalar = oracle(oracle_soc, ("oct104x6x5", "abu_scalar"), Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=1, BATCH=3, SEED=0.377), 0, gid0=g0, gid1=g1)[2]
    assert n != n_scalar                                        # a walk that used the launch's scalars fails on the count
    tuned(abu_local=1, **tune)
    try:
        Tg, _, st = run_engine(engine, job, 0, gid_first=g0, gid_count=g1 - g0, exec_mode=1)
        v = engine.last_variant()
        assert engine.last_passes() > 0 and engine.last_form() == 3 and v["abu"] == 1 and v["form"] == 3
        report("oct104x6x5 abu_local %s" % (tune,), Tg, T, st["tally_events"])
        assert st["tally_events"] == n, "trajectories diverged from the oracle"
        assert_tally_close(Tg, T, rtol=1e-5)
    finally:
        engine.set_opt(None)
        engine.set_exec(-1, 4)


# ---- packet splitting: soc_sim_bg_split_kernel and soc_sim_hp_split_kernel on oct759 (Index() in float) and oct104x6x5 (in double) ----
KEYS = split_host.COUNTERS + ("max_depth",)
SPLIT_MODELS = ["oct759", "oct104x6x5"]


def _split_same(got, ref, keys):
    TABS, INT, _, st = got
    wT, wI, _, wst = ref
    print("gpu", {k: st[k] for k in keys}, "restatement", {k: wst[k] for k in keys})
    assert {k: st[k] for k in keys} == {k: wst[k] for k in keys}
    assert wT.max() > 0 and wst["splits"] > 100
    assert_tally_close(TABS, wT, rtol=1e-5)
    assert_tally_close(INT, wI, rtol=1e-5)


@pytest.mark.parametrize("SELEM", [1, 3])
@pytest.mark.parametrize("name", SPLIT_MODELS)
def test_split_background(name, SELEM, engine):
    cl = cloud(name)

    def job():
        return Job(cl, sc._CSC, ABS=1e-4, SCA=3e-4, SOURCE=1, BATCH=2, SEED=0.2891, GLOBAL=sc.launch_shape(cl.AREA, SELEM), WITH_INT=1)
    ref = split_host.sim_bg_split("soc", job(), SELEM, 64)
    got = run_split(engine, job(), SELEM, 64)
    _split_same(got, ref, KEYS)
    assert got[3]["roots"] == 2 * cl.AREA
    assert engine.last_variant()["split"] == 1 and engine.last_variant()["dbl"] == (1 if name == "oct104x6x5" else 0)


@pytest.mark.parametrize("name", SPLIT_MODELS)
def test_split_healpix_background(name, engine):
    cl = cloud(name)
    HPBG, HPBGP = hc.sky_inputs("oct4b_w")
    GLOBAL = 1024 if name == "oct104x6x5" else hc.GLOBAL        # (96 work items split some hundred times on the long model; 1024 a thousand)

    def job():
        return Job(cl, sc._CSC, ABS=1e-4, SCA=3e-4, SOURCE=1, BATCH=3, SEED=0.5772, BG=0.0, GLOBAL=GLOBAL, WITH_INT=1, HPBG=HPBG, HPBGP=HPBGP)
    ref = hpsplit_host.sim_hp_split("soc", job(), 64)
    got = run_hp_split(engine, job(), 64)
    _split_same(got, ref, hpsplit_host.COUNTERS + ("max_depth", "skipped_splits"))
    assert got[3]["roots"] == 3 * GLOBAL
    assert engine.last_variant()["split"] == 1 and engine.last_variant()["dbl"] == (1 if name == "oct104x6x5" else 0)


# ---- scattered light: soc_sca_kernel (direct) on oct759, the sweep of rays on oct104x6x5 ----
def _view(cl, NPIX, MAP_DX):
    import math
    angles = ((30.0, 40.0), (90.0, 0.0), (0.0, 0.0))
    _, OD, RA, DE = launch.set_observer_directions([math.radians(t) for t, _ in angles], [math.radians(p) for _, p in angles])
    return ScaView(OD, RA, DE, NPIX=NPIX, MAP_DX=MAP_DX, CENTRE=(0.5 * cl.NX, 0.5 * cl.NY, 0.5 * cl.NZ), FFS=1)


@pytest.mark.parametrize("name,rays", [("oct759", False), ("oct759", None), ("oct104x6x5", False), ("oct104x6x5", True)],
                         ids=["oct759-direct", "oct759-refused", "oct104x6x5-direct", "oct104x6x5-rays"])
def test_scattered_light(name, rays, engine, oracle_soc):
    """rays None: soc_set_exec(1) on a grid whose Index() runs in float -- the sweep of rays is refused (no quiet fall-back), and the
    direct kernel then gives the oracle's image as if nothing had been asked"""
    from soc_amd.lib import SocError
    cl = cloud(name)
    a, s = opacities(cl)
    job = Job(cl, cases._CSC, ABS=3.0 * a, SCA=s, SOURCE=1, BATCH=3, SEED=0.377, DSC=cases._DSC, BG=1.0)
    view = _view(cl, (14, 11), 1.0 if name == "oct759" else 0.8)
    g0, g1 = 0, min(job.GLOBAL, 3000)
    if ("sca", name) not in _MEMO:
        _MEMO[("sca", name)] = oracle_sim_sca(oracle_soc, job, view, 0, gid0=g0, gid1=g1, nthreads=8)
    want, n = _MEMO[("sca", name)]
    assert (want > 0).sum() > 30 and (want == 0).any()
    try:
        if rays is None:
            engine.set_exec(1, 4)
            with pytest.raises(SocError, match="not one the sweep of rays takes"):
                run_sca(engine, job, view, 0, g0, g1 - g0)
        engine.set_exec(1 if rays else 0, 4)
        got, st = run_sca(engine, job, view, 0, g0, g1 - g0)
        if rays:
            assert engine.last_passes() > 0 and engine.last_form() == 3 and engine.last_variant()["rays"] == 1
        else:
            assert engine.last_passes() == 0
    finally:
        engine.set_exec(-1, 4)
    print("%s: image contributions %d, packets %d, scatterings %d" % (name, st["tally_events"], st["packets"], st["scatterings"]))
    assert st["tally_events"] == n and st["packets"] == 3 * (g1 - g0) and st["scatterings"] > 100
    assert_image_close(got, want)
