"""The brick-local walk in its FLOAT form (soc_ltree.h: soc_lt_aim_flt / soc_lt_land_flt; soc_lbrick_pass_flt<WINT>,
soc_lbrick_pass_ali_flt<WINT>, soc_lray_pass<., ., 0, 1>) on the GPU: hierarchies on which the reference evaluates Index() with float3
POS (NX <= 100, or <= 399 with two levels), reached with Engine.set_tuning(float_local=1).  The bar is that of the other sweeps:
identical trajectories (tally-event counts equal to the oracle's), tallies equal to fp32 summation order, last_form() == 3 and
last_variant()["dbl"] == 0; the sweep that reads the hierarchy from global memory (`global_tree`) is the second witness, and the
slow-step queue -- soc_index<float> in the event workgroups -- is forced on every few steps."""
import os
import sys

import numpy as np
import pytest

import cases
from oracle.pyoracle import Job, oracle_sim_sca
from soc_amd import synth
from soc_amd.lib import SocError
from test_gpu_sca import assert_image_close, run_sca
from util import assert_tally_close, run_engine

pytestmark = pytest.mark.gpu

_MEMO = {}


def cloud(name):
    if name not in _MEMO:
        _MEMO[name] = {"oct64_l4": lambda: synth.octree_cloud(64, levels=4, frac=0.08, seed=3),
                       "oct104_l2": lambda: synth.octree_cloud(104, levels=2, frac=0.08, seed=3),
                       "oct104_l4": lambda: synth.octree_cloud(104, levels=4, frac=0.08, seed=3),
                       "oct759": lambda: synth.noncubic_cloud("oct759")}[name]()
    return _MEMO[name]


def oracle(orc, key, job, kind, **kw):
    """the oracle's (TABS, INT, events) of a launch and what it left in the job (XAB, ROI record, vector sums): computed once per
    session, shared by the tunings, never changed"""
    if key not in _MEMO:
        T, I, n = orc.sim(job, kind, nthreads=8, **kw)
        extra = {k: np.array(getattr(job, k), np.float32).copy() for k in ("XAB", "ROI_SAVE", "INTV") if getattr(job, k, None) is not None}
        for a in (T, I) + tuple(extra.values()):
            a.setflags(write=False)
        _MEMO[key] = (T, I, n, extra)
    return _MEMO[key]


def opacities(cl):
    """about one optical depth of scattering along the shortest side: packets scatter a few times before they leave"""
    root = cl.DENS[:cl.NX * cl.NY * cl.NZ]
    k = 1.0 / (min(cl.NX, cl.NY, cl.NZ) * float(root[root > 0].mean()))
    return np.float32(0.1 * k), np.float32(k)


def bg_job(name):
    """(Job, gid0, gid1): about 6000 work items of a background launch from an offset (oct759: the whole launch is 2288)"""
    cl = cloud(name)
    a, s = opacities(cl)
    G = 8 * cl.AREA
    g0 = 100000 if G > 106000 else 0
    return Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=1, BATCH=4, SEED=0.377), g0, min(G, g0 + 6000)


@pytest.fixture(autouse=True)
def float_local(engine):
    engine.set_tuning(float_local=1)
    yield
    engine.set_tuning(float_local=0)
    engine.set_exec(-1, 4)


@pytest.fixture(params=[0, 1], ids=["park4096", "nopark"])
def parking(request, engine):
    """short brick queues parked until they hold 4096 packets (the default), or never"""
    engine.set_tuning(park_below=request.param)
    yield
    engine.set_tuning(park_below=0)


def _sweep(engine, job, kind, form=3, **kw):
    T, I, st = run_engine(engine, job, kind, exec_mode=1, **kw)
    assert engine.last_passes() > 0
    assert engine.last_form() == form, (engine.last_form(), form)
    assert engine.last_variant()["dbl"] == 0 and engine.last_variant()["octree"] == 1
    return T, I, st


# ---- 1: the smallest case, alone: one launch on the 8^3-root hierarchy of three levels ----
def test_smallest_case_first(engine, oracle_soc):
    ref, kind, mk = cases.CASES["bg_oct8"]
    job = mk()
    T, I, n, _ = oracle(oracle_soc, "bg_oct8", job, kind)
    Tg, _, st = _sweep(engine, job, kind)
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert_tally_close(Tg, T, rtol=1e-5)


# ---- 2: background packets ----
@pytest.mark.parametrize("tune", [dict(), dict(brick_cells=700), dict(slow_every=3), dict(steps_per_visit=3, hash_slots=64), dict(chunk=64, threads=64)],
                         ids=["default", "cells700", "slow3", "visit3_hash64", "chunk64_t64"])
def test_background_packets_on_the_64_root_hierarchy(tune, engine, oracle_soc, tuned, parking):
    job, g0, g1 = bg_job("oct64_l4")
    T, _, n, _ = oracle(oracle_soc, "bg64", job, 0, gid0=g0, gid1=g1)
    assert n > 100000
    tuned(**tune)
    Tg, _, st = _sweep(engine, job, 0, gid_first=g0, gid_count=g1 - g0)
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert st["scatterings"] > 1000
    assert_tally_close(Tg, T, rtol=1e-5)


@pytest.mark.parametrize("name", ["oct104_l2", "oct759"])
@pytest.mark.parametrize("tune", [dict(brick_cells=200), dict(brick_cells=200, slow_every=3)], ids=["cells200", "cells200_slow3"])
def test_background_packets_across_small_bricks(name, tune, engine, oracle_soc, tuned, parking):
    """one level of climb onto a 104-cell root grid (float because LEVELS < 3), and the 7 x 5 x 9 grid; bricks of 200 cells, so that
    packets leave and arrive across bricks"""
    job, g0, g1 = bg_job(name)
    T, _, n, _ = oracle(oracle_soc, "bg" + name, job, 0, gid0=g0, gid1=g1)
    assert n > 10000
    tuned(**tune)
    Tg, _, st = _sweep(engine, job, 0, gid_first=g0, gid_count=g1 - g0)
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert_tally_close(Tg, T, rtol=1e-5)


# ---- 3: the oracle cases of tests/cases.py on oct8, through the sweep ----
OCT8 = ["bg_oct8", "ps_in_oct8", "cl_oct8", "hp_oct8", "hp_oct8_weighted_int", "bg_oct8_mirror", "cl_oct8_mirror", "cl_oct8_ali",
        "cl_oct8_int2", "hp_oct8_int2", "bg_oct8_sw2", "cl_oct8_roisave", "roi_oct8_load_save"]


@pytest.mark.parametrize("cells", [0, 200], ids=["one_brick", "cells200"])
@pytest.mark.parametrize("name", OCT8)
def test_oracle_cases_on_oct8_in_the_sweep(name, cells, engine, oracle_soc, tuned):
    ref, kind, mk = cases.CASES[name]
    job = mk()
    T, I, n, extra = oracle(oracle_soc, name, job, kind)
    tuned(brick_cells=cells)
    Tg, Ig, st = _sweep(engine, job, kind)
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert_tally_close(Tg, T, rtol=1e-5)
    if job.WITH_INT:
        assert_tally_close(Ig, I, rtol=1e-5)
    if job.WITH_INT == 2:
        V = extra["INTV"]
        assert np.abs(V).sum() > 0
        for k in range(3):      # signed sums: the error is measured against the sum of the absolute terms, INT (as tests/test_gpu_parity.py)
            assert np.abs(job.INTV_gpu[k] - V[k]).max() <= 2e-6 * np.abs(I).max()
            assert np.all(np.abs(job.INTV_gpu[k] - V[k]) <= 1e-5 * np.maximum(I, 1e-3 * I.max()))
    if job.WITH_ALI:
        assert extra["XAB"].sum() > 0 and engine.last_variant()["ali"] == 1
        assert_tally_close(job.XAB_gpu, extra["XAB"], rtol=1e-5)
    if job.ROI is not None:
        want = extra["ROI_SAVE"]
        assert want.sum() > 0 and np.array_equal(job.ROI_SAVE_gpu != 0, want != 0)
        assert_tally_close(job.ROI_SAVE_gpu, want, rtol=1e-5)
    engine.set_features(0, 0, 0)


# ---- 4: the sweep that reads the hierarchy from global memory as the second witness ----
def test_global_tree_sweep_is_a_second_witness(engine, tuned):
    job, _, _ = bg_job("oct64_l4")
    g0, g1 = 0, 40000
    Ta, _, sa = _sweep(engine, job, 0, gid_first=g0, gid_count=g1 - g0)
    tuned(global_tree=1)
    Tb, _, sb = _sweep(engine, job, 0, form=2, gid_first=g0, gid_count=g1 - g0)
    assert sa["tally_events"] == sb["tally_events"] and sa["packets"] == sb["packets"] and sa["scatterings"] == sb["scatterings"]
    assert sa["scatterings"] > 1000
    assert_tally_close(Ta, Tb, rtol=1e-5)


# ---- 5: routing ----
def test_without_the_key_the_grid_is_routed_as_before(engine, oracle_soc):
    ref, kind, mk = cases.CASES["bg_oct8"]
    job = mk()
    T, _, n, _ = oracle(oracle_soc, "bg_oct8", job, kind)
    engine.set_tuning(float_local=0)
    Tg, _, st = _sweep(engine, job, kind, form=2)
    assert st["tally_events"] == n
    assert_tally_close(Tg, T, rtol=1e-5)


def test_per_cell_opacities_keep_their_path(engine, oracle_soc):
    """no kernel combines the float form with per-cell opacities: with the key (and with abu_local beside it) such a launch is routed as without"""
    ref, kind, mk = cases.CASES["bg_oct8"]
    job = mk()
    job = Job(job.cloud, cases._CSC, SOURCE=1, BATCH=30, SEED=0.41, OPT=cases._opt(job.cloud.CELLS))
    T, _, n, _ = oracle(oracle_soc, "bg_oct8_opt", job, kind)
    engine.set_opt_half(False)                              # (the shared engine may come from a run with `optishalf`)
    for abu_local in (0, 1):
        engine.set_tuning(abu_local=abu_local)
        try:
            Tg, _, st = _sweep(engine, job, kind, form=2)
        finally:
            engine.set_tuning(abu_local=0)
            engine.set_opt(None)
        assert engine.last_variant()["abu"] == 1
        assert st["tally_events"] == n
        assert_tally_close(Tg, T, rtol=1e-5)


def test_the_key_changes_nothing_where_index_runs_in_double(engine, oracle_soc):
    cl = cloud("oct104_l4")
    job = Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=4, SEED=0.377)
    g0, g1 = 100000, 103000
    T, _, n, _ = oracle(oracle_soc, "bg104", job, 0, gid0=g0, gid1=g1)
    Tg, _, st = run_engine(engine, job, 0, exec_mode=1, gid_first=g0, gid_count=g1 - g0)
    v = engine.last_variant()
    assert engine.last_form() == 3 and v["dbl"] == 1
    assert st["tally_events"] == n
    assert_tally_close(Tg, T, rtol=1e-5)
    engine.set_tuning(float_local=0)
    run_engine(engine, job, 0, exec_mode=1, gid_first=g0, gid_count=g1 - g0)
    assert engine.last_variant() == v


# ---- 6: the sweep of rays of the scattered-light launches ----
def _rays(engine, job, view, kind, healpix, hpsky=0):
    engine.set_exec(1, 4)
    img, st = run_sca(engine, job, view, kind)
    v = engine.last_variant()
    assert engine.last_passes() > 0 and engine.last_form() == 3
    assert v["rays"] == 1 and v["dbl"] == 0 and v["octree"] == 1 and v["healpix"] == healpix and v["hpsky"] == hpsky
    assert engine.sca_ray_steps() > st["packets"]
    return img, st


def _ps_oct8():
    return ("oct8ps", 2, lambda: Job(cases._oct8(), cases._CSC, ABS=1e-4, SCA=3e-4, SOURCE=0, BATCH=20, SEED=0.2, GLOBAL=256,
                                     PSPOS=cases._ps_in_oct8(), PS=[1.0, 2.0], DSC=cases._DSC), {})


RAYS = ["sca_bg_oct8", "sca_cl_oct8", "sca_ps_oct8", "sca_hpx_bg_oct8_out", "sca_hpx_cl_oct8_in", "sca_hp_oct8_hpx"]


def _sca_oracle(orc, name):
    ref, kind, mk, vkw = _ps_oct8() if name == "sca_ps_oct8" else cases.SCA_CASES[name]
    job, view = mk(), cases.sca_view(**vkw)
    if ("sca", name) not in _MEMO:
        want, n = oracle_sim_sca(orc, job, view, kind)
        want.setflags(write=False)
        _MEMO[("sca", name)] = (want, n)
    return (job, view, kind, "healpix" in vkw) + _MEMO[("sca", name)]


@pytest.mark.parametrize("cells", [0, 300], ids=["one_brick", "cells300"])
@pytest.mark.parametrize("name", RAYS)
def test_rays_on_oct8(name, cells, engine, oracle_soc, tuned):
    job, view, kind, hpx, want, n = _sca_oracle(oracle_soc, name)
    tuned(brick_cells=cells)
    got, st = _rays(engine, job, view, kind, int(hpx), int(kind == 3))
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert_image_close(got, want)


def test_rays_through_the_slow_queue_and_against_the_direct_kernel(engine, oracle_soc, tuned):
    job, view, kind, hpx, want, n = _sca_oracle(oracle_soc, "sca_bg_oct8")
    tuned(slow_every=3, brick_cells=300)
    got, st = _rays(engine, job, view, kind, 0)
    assert st["tally_events"] == n
    assert_image_close(got, want)
    engine.set_exec(0, 4)
    direct, sd = run_sca(engine, job, view, kind)
    assert engine.last_passes() == 0
    assert sd == st
    assert_image_close(got, direct)


@pytest.mark.parametrize("name", ["sca_bg_oct8_msf", "sca_cl_oct8_msf"])
def test_rays_with_several_scattering_functions_stay_refused(name, engine):
    ref, kind, mk, vkw = cases.SCA_CASES[name]
    job, view = mk(), cases.sca_view(**vkw)
    engine.set_exec(1, 4)
    try:
        with pytest.raises(SocError, match=r"not applicable: several scattering functions \(WITH_MSF\)"):
            run_sca(engine, job, view, kind)
    finally:
        engine.set_scatter_table(None, job.MSF[2][0])          # (what run_sca undoes after a launch of WITH_MSF)
        engine.set_opt(None)
        engine.set_abundances(None)


# ---- 7: from an ini file, with the class switch of the drivers forced on and off ----
def test_absorbed_file_run_on_a_float_index_hierarchy(engine, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(__file__))
    from test_host import _write_model
    from soc_amd import files
    from soc_amd.asoc import AbsorptionRun
    from soc_amd.ini import User
    engine.set_tuning(float_local=0)                        # (the driver's business here)
    d = str(tmp_path)
    cl = cloud("oct64_l4")
    ini = _write_model(d, cl, nfreq=2, with_ps=True, extra="gridlength 2e-6\nbgpackets 300000\n")
    # (automatic mode sweeps launches of a batch from 65536 work items on, and a sweep on a hierarchy from two launches on)
    txt = open(ini).read().replace("pointsource 3.3 3.2 3.1", "pointsource 32.3 31.7 30.2").replace("pspackets 4000\nglobal 128\n", "pspackets 131072\nglobal 65536\n")
    assert "global 65536" in txt
    open(ini, "w").write(txt)
    os.chdir(d)
    forms = []
    real = engine.batch_end

    def spy():
        real()
        if engine.last_passes() > 0:
            forms.append((engine.last_form(), engine.last_variant()["dbl"]))
    engine.batch_end = spy
    try:
        monkeypatch.setattr(AbsorptionRun, "FLOAT_LOCAL", True)
        Cg, _ = AbsorptionRun(User(ini), engine, verbose=0).run()
        got = files.read_absorbed(os.path.join(d, "abs.data")).copy()
        on = list(forms)
        del forms[:]
        monkeypatch.setattr(AbsorptionRun, "FLOAT_LOCAL", False)
        Cw, _ = AbsorptionRun(User(ini), engine, verbose=0).run()
        want = files.read_absorbed(os.path.join(d, "abs.data")).copy()
        off = list(forms)
    finally:
        engine.batch_end = real
    assert on and all(f == (3, 0) for f in on), "with float_local the sweeps of the run are brick-local: %r" % (on,)
    assert off and all(f == (2, 0) for f in off), "with float_local forced off the run is routed as always: %r" % (off,)
    assert want.max() > 0
    assert_tally_close(Cg, Cw, rtol=1e-5)
    assert_tally_close(got, want, rtol=1e-5)
