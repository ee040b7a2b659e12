"""Per-cell opacities (-D WITH_ABU) on the brick-local walk: soc_lbrick_pass_abu<WINT>, reached with Engine.set_tuning(abu_local=1).

The bar is the one of tests/test_gpu_ltree.py: identical trajectories (tally-event counts equal to the oracle's), tallies equal to
fp32 summation order, on the smallest hierarchy that is brick-local at all (104^3 root cells, 4 levels).  Every case also asserts
that the sweep ran as form 3 with the abundance kernel (last_variant()["abu"]).  With scalar opacities the oracle counts other
events on these launches (3 135 005 against 3 182 632 for the background launch of test_background_packets, both from the oracle
on the CPU), so a walk that used the launch's scalars would fail on the count.  Without the feature every case that asks for form 3 fails: the tuning key is unknown.

The last tests guard what must not change: the key off (form 2, as always), with_int 2 and ALI with per-cell opacities."""
import os
import sys

import numpy as np
import pytest

import cases
from oracle.pyoracle import Job
from soc_amd import synth
from util import EMW, assert_tally_close, assert_zero_weights_skipped, cl_packets, emission_weights, run_engine

pytestmark = pytest.mark.gpu

_MEMO = {}


def cloud104():
    if "c" not in _MEMO:
        _MEMO["c"] = synth.octree_cloud(104, levels=4, frac=0.08, seed=3)
    return _MEMO["c"]


def opt104(f=1.0):
    """per-cell opacities as _opt() of tests/test_gpu_variants.py builds them; f: another 'frequency'"""
    cl = cloud104()
    if "opt" not in _MEMO:
        rr = np.random.default_rng(11)
        opt = np.zeros((cl.CELLS, 2), np.float32)
        opt[:, 0] = 3e-6 * rr.uniform(0.5, 2, cl.CELLS)
        opt[:, 1] = 3e-5 * rr.uniform(0.5, 2, cl.CELLS)
        _MEMO["opt"] = opt
    return _MEMO["opt"] if f == 1.0 else _MEMO["opt"] * np.float32(f)


def emit104(f=1.0):
    cl = cloud104()
    return (np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4) * f).astype(np.float32)


def oracle(orc, key, job, kind, **kw):
    """the oracle's (TABS, INT, events) of a launch, computed once per session and left unchanged"""
    if key not in _MEMO:
        T, I, n = orc.sim(job, kind, nthreads=8, **kw)
        T.setflags(write=False)
        I.setflags(write=False)
        _MEMO[key] = (T, I, n)
    return _MEMO[key]


@pytest.fixture(autouse=True)
def abu_local(engine):
    engine.set_tuning(abu_local=1)
    yield
    engine.set_tuning(abu_local=0)
    engine.set_opt(None)
    engine.set_abundances(None)
    engine.set_features(0, 0, 0)
    engine.set_mirror(0)
    engine.set_ali(0)
    engine.set_exec(-1, 4)


def ran_local(engine):
    v = engine.last_variant()
    assert engine.last_passes() > 0
    assert engine.last_form() == 3, "the launches did not take the brick-local walk"
    assert v["abu"] == 1 and v["form"] == 3


def _sweep(engine, job, kind, **kw):
    T, I, st = run_engine(engine, job, kind, exec_mode=1, **kw)
    ran_local(engine)
    return T, I, st


# ---- 1: background packets, the shapes of the walk ----
@pytest.mark.parametrize("tune", [dict(), dict(brick_cells=700), dict(slow_every=3), dict(chunk=64, threads=64)],
                         ids=["defaults", "cells700", "slow3", "chunk64"])
def test_background_packets(tune, engine, oracle_soc, tuned):
    cl = cloud104()
    job = Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=4, SEED=0.377, OPT=opt104())
    g0, g1 = 100000, 106000
    T, _, n = oracle(oracle_soc, "bg", job, 0, gid0=g0, gid1=g1)
    tuned(**tune)
    Tg, _, st = _sweep(engine, job, 0, gid_first=g0, gid_count=g1 - g0)
    print("tally events %d, oracle %d" % (st["tally_events"], n))
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert_tally_close(Tg, T, rtol=1e-5)


def test_the_scalars_of_the_launch_are_not_used(oracle_soc):
    """the same launch with the scalar opacities the job carries beside OPT: other trajectories, so the count above tells the two apart"""
    cl = cloud104()
    a = Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=4, SEED=0.377, OPT=opt104())
    b = Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=4, SEED=0.377)
    na = oracle(oracle_soc, "bg", a, 0, gid0=100000, gid1=106000)[2]
    nb = oracle(oracle_soc, "bg_scalar", b, 0, gid0=100000, gid1=106000)[2]
    assert na != nb


# ---- 2: point sources, TABS and INT side by side (WINT 1), then INT alone in LDS (WINT 3) ----
def _ps_job(seed=0.2, tw=1.5, f=1.0):
    ps = np.array([[52.3, 51.7, 50.2], [52.0, 52.0, 300.0]], np.float32)
    return Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=0, BATCH=30, SEED=seed, GLOBAL=512, PSPOS=ps, PS=[1.0, 2.5], PS_METHOD=0,
               WITH_INT=1, TW=tw, OPT=opt104(f))


def test_point_sources_inside_and_outside(engine, oracle_soc):
    """TABS and INT side by side in LDS (WINT 1): two launches that tally into one INT array with different weights TW.  Then INT alone
    in LDS (WINT 3), TABS = TW * INT at the flush: a launch by itself, and the same through an INT group."""
    cl = cloud104()
    jobs = [_ps_job(), _ps_job(seed=0.3, tw=0.7)]
    if "ps2" not in _MEMO:
        T2, I2 = np.zeros(cl.CELLS, np.float32), np.zeros(cl.CELLS, np.float32)
        _MEMO["ps2"] = (T2, I2, sum(oracle_soc.sim(j, 0, nthreads=8, TABS=T2, INT=I2)[2] for j in jobs))
    T2, I2, n2 = _MEMO["ps2"]
    e = engine
    e.set_cloud(cl)
    e.set_features(1, 0, 0)
    e.set_scatter_table(None, cases._CSC)
    e.set_optical(3e-6, 3e-5)
    e.set_opt(jobs[0].OPT)
    e.set_mirror(0)
    e.set_exec(1, 4)
    e.zero(0)
    e.zero(1)
    e.stats(reset=True)
    e.batch_begin_shared_int(0)
    for j in jobs:
        e.sim_pb(0, j.PACKETS, j.BATCH, j.SEED, j.BG, j.TW, PSPOS=j.PSPOS[:, :3], PS=j.PS, GLOBAL=j.GLOBAL)
    e.batch_end()
    ran_local(e)
    assert e.last_variant()["wint"] == 1
    assert e.stats()["tally_events"] == n2
    assert_tally_close(e.read_tally(0), T2, rtol=1e-5)
    assert_tally_close(e.read_tally(1), I2, rtol=1e-5)
    # one weight per INT array: the INT-only form
    job = jobs[0]
    T, I, n = oracle(oracle_soc, "ps", job, 0)
    Tg, Ig, st = _sweep(engine, job, 0)
    assert engine.last_variant()["wint"] == 3
    assert st["tally_events"] == n
    assert_tally_close(Tg, T, rtol=1e-5)
    assert_tally_close(Ig, I, rtol=1e-5)
    e.zero(0)
    e.stats(reset=True)
    e.batch_begin_int_groups(0)
    e.batch_next_int()
    e.sim_pb(0, job.PACKETS, job.BATCH, job.SEED, job.BG, job.TW, PSPOS=job.PSPOS[:, :3], PS=job.PS, GLOBAL=job.GLOBAL)
    e.batch_end()
    ran_local(e)
    assert e.last_variant()["wint"] == 3
    assert e.stats()["tally_events"] == n
    assert_tally_close(e.read_tally(0), T, rtol=1e-5)
    assert_tally_close(e.batch_read_int(0), I, rtol=1e-5)


# ---- 3: cell emission ----
@pytest.mark.parametrize("emw", EMW)
def test_cell_emission(emw, engine, oracle_soc, tuned):
    cl = cloud104()

    def mk(e):
        return Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=2, BATCH=1, SEED=0.9, GLOBAL=8192, EMIT=emit104(),
                   EMWEI=emission_weights(cl.CELLS, e), USE_EMWEIGHT=1 if e else 0, OPT=opt104())
    job = mk(emw)
    g0, g1 = 4000, 4096
    T, _, n = oracle(oracle_soc, ("cl", emw), job, 1, gid0=g0, gid1=g1)
    if emw == "zeros":                                   # (cells without weight are stepped over)
        assert_zero_weights_skipped(job, mk(1), g0, g1, n, oracle(oracle_soc, ("cl", 1), mk(1), 1, gid0=g0, gid1=g1)[2])
    tuned(slow_every=7)
    Tg, _, st = _sweep(engine, job, 1, gid_first=g0, gid_count=g1 - g0)
    assert st["tally_events"] == n
    if emw == "zeros":
        assert st["packets"] == cl_packets(job, g0, g1)
    assert_tally_close(Tg, T, rtol=1e-5)


# ---- 4: the Healpix background ----
def test_healpix_background(engine, oracle_soc):
    sky, P = cases.hp_sky(weighted=True)
    job = Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=8, SEED=0.11, GLOBAL=4096, HPBG=sky, HPBGP=P, TW=1.2, OPT=opt104())
    T, _, n = oracle(oracle_soc, "hp", job, 2)
    Tg, _, st = _sweep(engine, job, 2)
    assert st["tally_events"] == n
    assert_tally_close(Tg, T, rtol=1e-5)


# ---- 5: WITH_MSF, the scatterer drawn from the cell's species ----
def test_several_scattering_functions(engine, oracle_soc):
    cl = cloud104()
    job = Job(cl, None, SOURCE=1, BATCH=4, SEED=0.46, **cases.msf_inputs(cl))
    g0, g1 = 100000, 104000
    T, _, n = oracle(oracle_soc, "msf", job, 0, gid0=g0, gid1=g1)
    Tg, _, st = _sweep(engine, job, 0, gid_first=g0, gid_count=g1 - g0)
    print("scatterings %d" % st["scatterings"])
    assert st["tally_events"] == n and st["scatterings"] > 100
    assert_tally_close(Tg, T, rtol=1e-5)


# ---- 6: two frequencies x (point source, background, cell emission) in one sweep: groups by OPT, the shared copy of OPT ----
_FREQS = ((1.0, 1.0), (1.7, 0.6))                               # factor on OPT (and the emission), TW


def _six():
    """the six launches: (kind, job, gid0, gid1) by frequency"""
    out = []
    for k, (f, tw) in enumerate(_FREQS):
        kw = dict(ABS=3e-6, SCA=3e-5, WITH_INT=1, TW=tw, OPT=opt104(f))
        ps = np.array([[52.3, 51.7, 50.2]], np.float32)
        out.append([(0, Job(cloud104(), cases._CSC, SOURCE=0, BATCH=20, SEED=0.2 + 0.1 * k, GLOBAL=512, PSPOS=ps, PS=[1.0 + k], PS_METHOD=0, **kw), 0, 512),
                    (0, Job(cloud104(), cases._CSC, SOURCE=1, BATCH=2, SEED=0.3 + 0.1 * k, BG=1.0 + k, **kw), 200000, 202000),
                    (1, Job(cloud104(), cases._CSC, SOURCE=2, BATCH=1, SEED=0.6 + 0.1 * k, GLOBAL=8192, EMIT=emit104(1 + k), **kw), 4000, 4048)])
    return out


def _issue(e, kind, job, g0, g1):
    if kind == 0:
        e.sim_pb(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.BG, job.TW, PSPOS=job.PSPOS[:, :3], PS=job.PS, GLOBAL=job.GLOBAL,
                 gid_first=g0, gid_count=g1 - g0)
    else:
        e.set_emission(job.EMIT, None)
        e.sim_cl(2, job.PACKETS, job.BATCH, job.SEED, job.TW, job.GLOBAL, gid_first=g0, gid_count=g1 - g0)


def test_two_frequencies_in_one_sweep(engine, oracle_soc):
    freqs = _six()
    if "six" not in _MEMO:
        T = np.zeros(cloud104().CELLS, np.float32)
        ints, n = [], 0
        for launches in freqs:
            I = np.zeros(cloud104().CELLS, np.float32)
            for kind, job, g0, g1 in launches:
                n += oracle_soc.sim(job, kind, gid0=g0, gid1=g1, nthreads=8, TABS=T, INT=I)[2]
            ints.append(I)
        _MEMO["six"] = (T, ints, n)
    T, ints, n = _MEMO["six"]
    e = engine
    e.set_cloud(cloud104())
    e.set_scatter_table(None, cases._CSC)
    e.set_optical(3e-6, 3e-5)
    e.set_mirror(0)
    e.set_exec(1, 4)
    for with_int in (0, 1):
        e.set_features(with_int, 0, 0)
        e.zero(0)
        e.stats(reset=True)
        if with_int:
            e.batch_begin_int_groups(0)
        else:
            e.batch_begin(0)
        for k, launches in enumerate(freqs):
            if with_int:
                e.batch_next_int()
            e.set_opt(launches[0][1].OPT)                       # once per frequency: its three launches share the copy
            for la in launches:
                _issue(e, *la)
                assert e.last_passes() == 0, "a launch was not deferred"
        e.batch_end()
        ran_local(e)
        assert e.last_variant()["kind"] == 4 and e.last_variant()["wint"] == (3 if with_int else 0)
        st = e.stats()
        assert st["tally_events"] == n, "one sweep of six launches: the events of the oracle's six runs"
        assert_tally_close(e.read_tally(0), T, rtol=1e-5)
        if with_int:
            for k in range(2):
                assert_tally_close(e.batch_read_int(k), ints[k], rtol=1e-5)


def test_launches_after_new_opacities_do_not_share_the_earlier_copy(engine, oracle_soc):
    """Two background launches with the same seed, the second after another set_opt: were the copy of the first shared, both would
    tally the first frequency's absorptions.  Then 17 opacity arrays in one batch, which holds 16: the engine starts another sweep by
    itself, and every launch still runs once with its own array."""
    cl = cloud104()
    g0, g1 = 200000, 201000
    jobs = [Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=2, SEED=0.31, OPT=opt104(f)) for f in (1.0, 1.7)]
    T = np.zeros(cl.CELLS, np.float32)
    n = sum(oracle_soc.sim(j, 0, gid0=g0, gid1=g1, nthreads=8, TABS=T)[2] for j in jobs)
    T1, _, n1 = oracle_soc.sim(jobs[0], 0, gid0=g0, gid1=g1, nthreads=8)
    assert n != 2 * n1
    e = engine
    e.set_cloud(cl)
    e.set_features(0, 0, 0)
    e.set_scatter_table(None, cases._CSC)
    e.set_optical(3e-6, 3e-5)
    e.set_exec(1, 4)
    e.zero(0)
    e.stats(reset=True)
    e.batch_begin(0)
    for j in jobs:
        e.set_opt(j.OPT)
        e.sim_pb(1, 0, j.BATCH, j.SEED, j.BG, j.TW, GLOBAL=j.GLOBAL, gid_first=g0, gid_count=g1 - g0)
    e.batch_end()
    ran_local(e)
    assert e.stats()["tally_events"] == n
    assert_tally_close(e.read_tally(0), T, rtol=1e-5)
    # 17 arrays (the same values, set anew every time), 100 work items each: a batch holds 16
    e.zero(0)
    e.stats(reset=True)
    e.batch_begin(0)
    for k in range(17):
        e.set_opt(jobs[0].OPT)
        e.sim_pb(1, 0, 2, 0.31, 1.0, 1.0, GLOBAL=jobs[0].GLOBAL, gid_first=g0 + 100 * (k % 10), gid_count=100)
    e.batch_end()
    ran_local(e)
    Tw = np.zeros(cl.CELLS, np.float32)
    m = 0
    for k in range(10):
        Tk, _, nk = oracle_soc.sim(jobs[0], 0, gid0=g0 + 100 * k, gid1=g0 + 100 * (k + 1), nthreads=8)
        w = 2 if k < 7 else 1                                   # launches 10 .. 16 repeat the first seven ranges
        m += w * nk
        Tw += np.float32(w) * Tk
    assert e.stats()["tally_events"] == m
    assert_tally_close(e.read_tally(0), Tw, rtol=1e-5)


# ---- 7: reflecting faces: admitted to the sweep because the launch is brick-local ----
def test_reflecting_faces(engine, oracle_soc):
    job = Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=3, SEED=0.4177, MIRROR=25, OPT=opt104())
    g0, g1 = 200000, 204000
    T, _, n = oracle(oracle_soc, "mirror", job, 0, gid0=g0, gid1=g1)
    Tg, _, st = _sweep(engine, job, 0, gid_first=g0, gid_count=g1 - g0)
    assert st["tally_events"] == n
    assert_tally_close(Tg, T, rtol=1e-5)


# ---- 8: the key off: the sweep that reads the hierarchy and OPT from global memory, as always ----
def test_key_off_is_the_older_sweep_and_a_second_witness(engine):
    job = Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=2, SEED=0.91, OPT=opt104())
    g0, g1 = 0, 40000
    Ta, _, sa = _sweep(engine, job, 0, gid_first=g0, gid_count=g1 - g0)
    engine.set_tuning(abu_local=0)
    Tb, _, sb = run_engine(engine, job, 0, gid_first=g0, gid_count=g1 - g0, exec_mode=1)
    v = engine.last_variant()
    assert engine.last_passes() > 0 and engine.last_form() == 2 and v["abu"] == 1 and v["form"] == 2
    assert sa["tally_events"] == sb["tally_events"] and sa["packets"] == sb["packets"] and sa["scatterings"] == sb["scatterings"]
    assert_tally_close(Ta, Tb, rtol=1e-5)


# ---- 9: with_int 2 and ALI with per-cell opacities keep their paths ----
def test_with_int_2_keeps_its_path(engine, oracle_soc):
    job = Job(cloud104(), cases._CSC, ABS=3e-5, SCA=6e-5, SOURCE=1, BATCH=3, SEED=0.377, WITH_INT=2, TW=1.7, OPT=opt104())
    g0, g1 = 100000, 103000
    T, I, n = oracle_soc.sim(job, 0, gid0=g0, gid1=g1, nthreads=8)
    Tg, Ig, st = run_engine(engine, job, 0, gid_first=g0, gid_count=g1 - g0, exec_mode=-1)
    assert engine.last_form() != 3
    assert st["tally_events"] == n
    assert_tally_close(Tg, T, rtol=1e-5)
    assert_tally_close(Ig, I, rtol=1e-5)


def test_ali_keeps_its_path(engine, oracle_soc):
    job = Job(cloud104(), cases._CSC, ABS=3e-4, SCA=6e-4, SOURCE=2, BATCH=2, SEED=0.9, GLOBAL=8192, EMIT=emit104(), WITH_ALI=1, TW=1.3,
              OPT=opt104(100.0))
    g0, g1 = 4000, 4064
    T, _, n = oracle_soc.sim(job, 1, gid0=g0, gid1=g1, nthreads=8)
    want = np.array(job.XAB, np.float32).copy()
    assert want.sum() > 0
    Tg, _, st = run_engine(engine, job, 1, gid_first=g0, gid_count=g1 - g0, exec_mode=-1)
    assert engine.last_form() != 3
    assert st["tally_events"] == n
    assert_tally_close(Tg, T, rtol=1e-5)
    assert_tally_close(job.XAB_gpu, want, rtol=1e-5)


# ---- 10: from an ini file: an abundance file, optishalf, the absorbed file ----
def test_absorbed_file_run_with_an_abundance_file(engine, tmp_path, monkeypatch):
    sys.path.insert(0, os.path.dirname(__file__))
    from test_host import _write_model
    from soc_amd import files
    from soc_amd.asoc import AbsorptionRun
    from soc_amd.ini import User
    d = str(tmp_path)
    cloud = cloud104()
    np.random.default_rng(4).uniform(0.2, 1.0, cloud.CELLS).astype(np.float32).tofile(os.path.join(d, "a.abu"))
    ini = _write_model(d, cloud, nfreq=2, with_ps=True, extra="gridlength 2e-6\nbgpackets 300000\noptishalf\n")
    with open(os.path.join(d, "m2.dust"), "w") as fp:
        fp.write("eqdust\n 1.0e-7\n 0.7e-4\n2\n 4.00000e+14  0.6  2.0e-2  1.2e-1\n 4.67700e+14  0.6  2.5e-2  1.0e-1\n")
    txt = open(ini).read().replace("optical %s/m.dust\n" % d, "optical %s/m.dust %s/a.abu\noptical %s/m2.dust\n" % (d, d, d))
    # (automatic mode sweeps launches of a batch from 65536 work items on, and a sweep on a hierarchy from two launches on)
    txt = txt.replace("pointsource 3.3 3.2 3.1", "pointsource 52.3 51.7 50.2").replace("pspackets 4000\nglobal 128\n", "pspackets 131072\nglobal 65536\n")
    assert "global 65536" in txt
    open(ini, "w").write(txt)
    os.chdir(d)
    forms = []
    real = engine.batch_end

    def spy():
        real()
        if engine.last_passes() > 0:
            forms.append((engine.last_form(), engine.last_variant()["abu"]))
    engine.batch_end = spy
    try:
        monkeypatch.setattr(AbsorptionRun, "ABU_LOCAL", True)
        Cg, _ = AbsorptionRun(User(ini), engine, verbose=0).run()
        got = files.read_absorbed(os.path.join(d, "abs.data")).copy()
        on = list(forms)
        del forms[:]
        monkeypatch.setattr(AbsorptionRun, "ABU_LOCAL", False)
        Cw, _ = AbsorptionRun(User(ini), engine, verbose=0).run()
        want = files.read_absorbed(os.path.join(d, "abs.data")).copy()
        off = list(forms)
    finally:
        engine.batch_end = real
    assert on and all(f == (3, 1) for f in on), "with abu_local the sweeps of the run are brick-local: %r" % (on,)
    assert off and all(f == (2, 1) for f in off), "with abu_local forced off the run is routed as always: %r" % (off,)
    assert want.max() > 0
    assert_tally_close(Cg, Cw, rtol=1e-5)
    assert_tally_close(got, want, rtol=1e-5)
