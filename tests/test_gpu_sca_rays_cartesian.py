"""Scattered-light images through the sweep of rays on single-level (Cartesian) grids (soc_brick.hip: the CART arm of
soc_lbrick_walk<., RAY> + soc_sca_events; bricks of root cells from soc_cbricks_build) against the CPU oracle and the direct
kernel: identical trajectories (image contributions, packets, scatterings equal) and images equal to fp32 summation order -- the bar
of tests/test_gpu_sca_rays.py.  Two grids: one with three different edges, none a multiple of the brick edge of 16 (40 x 36 x 50),
and a 104^3 cube (6.5 bricks per edge); optical depth about 2 across either.  Without the feature every soc_set_exec(1) launch here
raises SocError ("brick sweep requested but not applicable")."""
import math
import os

import numpy as np
import pytest

import cases
from oracle.pyoracle import Job, ScaView, oracle_sim_sca
from soc_amd import files, launch, synth
from soc_amd.lib import SocError
from test_gpu_sca import assert_image_close, run_sca
from test_gpu_sca_rays import parking  # noqa: F401  (the three parking settings)
from util import EMW, assert_zero_weights_skipped, cl_packets, emission_weights

pytestmark = pytest.mark.gpu

_CLOUDS = {}


def cloud(name):
    if name not in _CLOUDS:
        _CLOUDS[name] = synth.cartesian_cloud(40, NY=36, NZ=50, seed=5) if name == "odd" else synth.cartesian_cloud(104, seed=7)
    return _CLOUDS[name]


def kappa(cl):
    """scattering cross section for an optical depth of 2 along the mean edge"""
    return 2.0 / ((cl.NX + cl.NY + cl.NZ) / 3.0 * float(cl.DENS.mean()))


def view(cl, FFS=1, angles=((30.0, 40.0), (90.0, 0.0), (0.0, 0.0)), NPIX=(40, 36)):
    th = [math.radians(a[0]) for a in angles]
    ph = [math.radians(a[1]) for a in angles]
    _, OD, RA, DE = launch.set_observer_directions(th, ph)
    n = max(cl.NX, cl.NY, cl.NZ)
    return ScaView(OD, RA, DE, NPIX=NPIX, MAP_DX=1.2 * n / 36.0, CENTRE=(cl.NX / 2.0, cl.NY / 2.0, cl.NZ / 2.0), FFS=FFS)


def hview(cl, where, FFS=1, nside=8):
    pos = (0.51 * cl.NX, 0.49 * cl.NY, 0.47 * cl.NZ) if where == "inside" else (2.3 * cl.NX, 0.4 * cl.NY, 0.55 * cl.NZ)
    return cases.sca_view(healpix=(nside, pos), FFS=FFS)


def job(cl, **kw):
    kw.setdefault("ABS", 0.3 * kappa(cl))
    kw.setdefault("SCA", kappa(cl))
    kw.setdefault("DSC", cases._DSC)
    return Job(cl, kw.pop("CSC", cases._CSC), **kw)


def _rays(engine, jb, vw, kind, g0, g1):
    engine.set_exec(1, 4)
    try:
        img, st = run_sca(engine, jb, vw, kind, g0, g1 - g0)
        _check_variant(engine, kind, vw)
        assert engine.sca_ray_steps() > st["packets"]
    finally:
        engine.set_exec(-1, 4)
    return img, st


def _check_variant(engine, kind, vw):
    assert engine.last_passes() > 0 and engine.last_form() != 0
    v = engine.last_variant()
    assert v["rays"] == 1 and v["octree"] == 0
    assert v["healpix"] == (1 if vw.nside else 0) and v["hpsky"] == (1 if kind == 3 else 0)


def _direct(engine, jb, vw, kind, g0, g1):
    engine.set_exec(0, 4)
    try:
        img, st = run_sca(engine, jb, vw, kind, g0, g1 - g0)
        assert engine.last_passes() == 0 and engine.last_form() == 0
    finally:
        engine.set_exec(-1, 4)
    return img, st


_WANT = {}


def _oracle(oracle_soc, key, jb, vw, kind, g0, g1):
    """the oracle's image and count of a case (kept: the tuning variants of a case share it)"""
    if key not in _WANT:
        _WANT[key] = oracle_sim_sca(oracle_soc, jb, vw, kind, gid0=g0, gid1=g1, nthreads=8)
    return _WANT[key]


def _parity(engine, oracle_soc, key, jb, vw, kind, g0, g1):
    """oracle, sweep of rays and direct kernel: counts equal, images to summation order"""
    want, n = _oracle(oracle_soc, key, jb, vw, kind, g0, g1)
    got, st = _rays(engine, jb, vw, kind, g0, g1)
    print("%s: image contributions %d (oracle %d), packets %d, scatterings %d" % (key, st["tally_events"], n, st["packets"], st["scatterings"]))
    assert st["tally_events"] == n and n > 0
    assert_image_close(got, want)
    ref, sd = _direct(engine, jb, vw, kind, g0, g1)
    assert sd == st
    assert_image_close(got, ref)
    return st


GRIDS = ["odd", "cube"]
# many brick crossings and short chunks: bricks of 9^3 and of 4^3 cells, few steps per visit, chunks of one packet per lane of one wave
TUNES = [dict(), dict(brick_cells=900, steps_per_visit=5), dict(brick_cells=64, steps_per_visit=2), dict(chunk=64, threads=64)]


@pytest.mark.parametrize("tune", TUNES, ids=["builtin", "bricks9", "bricks4", "chunk64"])
@pytest.mark.parametrize("ffs", [1, 0])
@pytest.mark.parametrize("grid", GRIDS)
def test_background_rays(grid, ffs, tune, engine, oracle_soc, tuned, parking):  # noqa: F811
    cl = cloud(grid)
    g0, g1 = (30000, 33000) if grid == "odd" else (100000, 103000)            # a work-item sub-range
    tuned(**tune)
    st = _parity(engine, oracle_soc, ("bg", grid, ffs), job(cl, SOURCE=1, BATCH=3, SEED=0.377, BG=1.0), view(cl, FFS=ffs), 0, g0, g1)
    assert st["packets"] == 3 * (g1 - g0) and st["scatterings"] > 1000


@pytest.mark.parametrize("meth", [0, 1, 2, 4, 5])
@pytest.mark.parametrize("grid", GRIDS)
def test_point_source_rays(grid, meth, engine, oracle_soc):
    cl = cloud(grid)
    inside = [0.503 * cl.NX, 0.497 * cl.NY, 0.48 * cl.NZ]
    outside = [0.5 * cl.NX, 0.5 * cl.NY, 2.9 * cl.NZ]
    ps = np.array([outside] if meth == 4 else [inside, outside], np.float32)                # (method 4: external sources only)
    lum = [2.5] if meth == 4 else [1.0, 2.5]
    xps = files.analyse_external_point_sources(cl.NX, cl.NY, cl.NZ, ps, len(ps), meth)
    jb = job(cl, SOURCE=0, BATCH=12, SEED=0.2, GLOBAL=512, PSPOS=ps, PS=lum, PS_METHOD=meth, XPS=xps)
    for kind in (2, 0):                                   # SimRAM_PS, and the point sources of SimRAM_PB
        st = _parity(engine, oracle_soc, ("ps", grid, meth, kind), jb, view(cl), kind, 0, 512)
        assert st["packets"] == 12 * 512


@pytest.mark.parametrize("emw", EMW)
@pytest.mark.parametrize("grid", GRIDS)
def test_cell_emission_rays(grid, emw, engine, oracle_soc, parking):  # noqa: F811
    cl = cloud(grid)
    emit = (cl.DENS * 1e-3).astype(np.float32)

    def mk(e):
        return job(cl, SOURCE=2, BATCH=1, SEED=0.9, GLOBAL=8192, EMIT=emit, EMWEI=emission_weights(cl.CELLS, e), USE_EMWEIGHT=1 if e else 0)
    jb = mk(emw)
    g0, g1 = 4000, 4024 + (72 if grid == "odd" else 0)
    if emw == "zeros":                                   # (cells without weight are stepped over)
        assert_zero_weights_skipped(jb, mk(1), g0, g1, _oracle(oracle_soc, ("cl", grid, emw), jb, view(cl), 1, g0, g1)[1],
                                    _oracle(oracle_soc, ("cl", grid, 1), mk(1), view(cl), 1, g0, g1)[1])
    st = _parity(engine, oracle_soc, ("cl", grid, emw), jb, view(cl), 1, g0, g1)
    if emw == "zeros":                                   # a third fewer packets than with all weights positive: the exact number
        assert st["packets"] == cl_packets(jb, g0, g1) > 600
    else:
        assert st["packets"] > 800


@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("grid", GRIDS)
def test_healpix_sky_rays(grid, weighted, engine, oracle_soc):
    cl = cloud(grid)
    sky, P = cases.hp_sky(weighted=weighted)
    jb = job(cl, BATCH=4, SEED=0.37, GLOBAL=3000, HPBG=sky, HPBGP=P)
    st = _parity(engine, oracle_soc, ("hp", grid, weighted), jb, view(cl), 3, 0, 3000)
    assert st["packets"] == 4 * 3000 and st["scatterings"] > 500


@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("grid", GRIDS)
def test_healpix_image_rays(grid, where, engine, oracle_soc, parking):  # noqa: F811
    cl = cloud(grid)
    g0, g1 = 20000, 22000
    st = _parity(engine, oracle_soc, ("hpx", grid, where), job(cl, SOURCE=1, BATCH=3, SEED=0.51, BG=1.0), hview(cl, where), 0, g0, g1)
    assert st["packets"] == 3 * (g1 - g0) and st["scatterings"] > 500


@pytest.mark.parametrize("grid", GRIDS)
def test_healpix_sky_on_a_healpix_image(grid, engine, oracle_soc):
    cl = cloud(grid)
    sky, P = cases.hp_sky(weighted=True)
    jb = job(cl, BATCH=3, SEED=0.23, GLOBAL=2000, HPBG=sky, HPBGP=P)
    _parity(engine, oracle_soc, ("hphpx", grid), jb, hview(cl, "inside"), 3, 0, 2000)


@pytest.mark.parametrize("grid", GRIDS)
def test_reflecting_faces(grid, engine, oracle_soc, parking):  # noqa: F811
    """mask 21: one reflecting face per axis; against the oracle on a small range, and against the direct kernel on a launch larger
    than the oracle takes in seconds, with and without the faces"""
    cl = cloud(grid)
    vw = view(cl, angles=((60.0, 200.0), (10.0, 80.0)))
    try:
        _parity(engine, oracle_soc, ("mirror", grid), job(cl, SOURCE=1, BATCH=2, SEED=0.61, BG=1.0, MIRROR=21), vw, 0, 5000, 7000)
        for mirror in (0, 21):
            jb = job(cl, SOURCE=1, BATCH=2, SEED=0.61, BG=1.0, MIRROR=mirror)
            n = 40000 if grid == "odd" else 60000
            a, sa = _direct(engine, jb, vw, 0, 0, n)
            b, sb = _rays(engine, jb, vw, 0, 0, n)
            assert sa == sb and sb["packets"] == 2 * n
            assert_image_close(b, a)
    finally:
        engine.set_mirror(0)


def _defer(eng, jb, kind, g0, g1):
    """the calls of run_sca without the ones that would run what is pending (zero, stats, sync, read)"""
    eng.set_optical(jb.ABS, jb.SCA)
    eng.set_scatter_table(jb.DSC, jb.CSC)
    xps = (jb.XPS_NSIDE, jb.XPS_SIDE, jb.XPS_AREA)
    if kind == 2:
        eng.sca_sim_ps(jb.PACKETS, jb.BATCH, jb.SEED, jb.BG, jb.PSPOS[:, :3], jb.PS, XPS=xps, GLOBAL=jb.GLOBAL, gid_first=g0, gid_count=g1 - g0)
    elif kind == 0:
        eng.sca_sim_pb(jb.SOURCE, jb.PACKETS, jb.BATCH, jb.SEED, jb.BG, jb.PSPOS[:, :3], jb.PS, XPS=xps, GLOBAL=jb.GLOBAL, gid_first=g0, gid_count=g1 - g0)
    else:
        eng.set_emission(jb.EMIT, jb.EMWEI)
        eng.sca_sim_cl(jb.SOURCE, jb.PACKETS, jb.BATCH, jb.SEED, jb.GLOBAL, gid_first=g0, gid_count=g1 - g0)


@pytest.mark.parametrize("grid", GRIDS)
def test_rays_in_one_batch_equal_the_direct_kernel(grid, engine, parking):  # noqa: F811
    """three 'frequencies' (own opacities, scattering functions, emission, seeds), each with a point-source, a background and a
    cell-emission launch and an image of its own (soc_sca_batch_images), deferred into ONE sweep of rays: every image and the event
    counts equal those of the same launches through the direct kernel, one at a time"""
    cl = cloud(grid)
    k = kappa(cl)
    vw = view(cl, angles=((60.0, 200.0), (10.0, 80.0)))
    ps = np.array([[0.503 * cl.NX, 0.497 * cl.NY, 0.48 * cl.NZ]], np.float32)
    emit = (cl.DENS * 1e-3).astype(np.float32)
    tabs = [synth.hg_scattering_table(g) for g in (0.6, 0.2, 0.4)]                # (DSC, CSC)
    freqs = []
    for f in range(3):
        kw = dict(ABS=(0.2 + 0.1 * f) * k, SCA=(1.0 - 0.2 * f) * k, DSC=tabs[f][0], CSC=tabs[f][1])
        freqs.append([(2, job(cl, SOURCE=0, BATCH=6, SEED=0.2 + 0.1 * f, GLOBAL=4096, PSPOS=ps, PS=[1.0 + f], **kw), 0, 4096),
                      (0, job(cl, SOURCE=1, BATCH=2, SEED=0.3 + 0.1 * f, BG=1.0 + f, **kw), 1000, 21000),
                      (1, job(cl, SOURCE=2, BATCH=1, SEED=0.4 + 0.1 * f, GLOBAL=16384, EMIT=emit * (1 + f), **kw), 0, 16384)])
    single, total = [], dict(tally_events=0, packets=0, scatterings=0)
    for launches in freqs:
        img = None
        for kind, jb, g0, g1 in launches:
            a, st = _direct(engine, jb, vw, kind, g0, g1)
            img = a.astype(np.float64) if img is None else img + a
            for key in total:
                total[key] += st[key]
        single.append(img)
    engine.set_exec(1, 4)
    try:
        engine.stats(reset=True)
        engine.batch_begin(0)
        engine.sca_batch_images(3)
        for f, launches in enumerate(freqs):
            engine.sca_batch_select(f)
            for kind, jb, g0, g1 in launches:
                _defer(engine, jb, kind, g0, g1)
        assert engine.last_passes() == 0                          # nothing has run yet ...
        engine.batch_end()
        st = engine.stats()
        _check_variant(engine, 0, vw)                             # ... and all of it ran as one sweep of rays
        assert st == total and st["scatterings"] > 10000
        for f in range(3):
            assert_image_close(engine.sca_batch_read(f), single[f])
    finally:
        engine.sca_batch_images(0)
        engine.set_exec(-1, 4)


def test_scattering_run_end_to_end(engine, tmp_path):
    """python -m soc_amd.asocs on a small Cartesian model with soc_set_exec(1): the batch of every source block runs as one sweep of
    rays; each image equals the one of the same host loop on the oracle engine"""
    from oracle_engine import OracleEngine
    from soc_amd.asocs import ScatteringRun
    from soc_amd.ini import User
    from test_host import _write_model
    d = str(tmp_path)
    cl = synth.cartesian_cloud(20, NY=18, NZ=25, seed=3)
    f = np.float32(2.0 / (581.0 * 21 * float(cl.DENS.mean())))       # optical depth about 2 for the dust of _write_model (581 per unit density and cell)
    cl = synth.Cloud(cl.NX, cl.NY, cl.NZ, [cl.DENS * f])
    ini = _write_model(d, cl, nfreq=2, with_ps=True, extra="mapping 24 20 1.1\ndirection 30 40\ndirection 90 0\n")
    os.chdir(d)
    want = ScatteringRun(User(ini), OracleEngine("soc"), verbose=0).run()
    engine.set_exec(1, 4)
    try:
        got = ScatteringRun(User(ini), engine, verbose=0).run()
        assert engine.last_passes() > 0 and engine.last_form() != 0
        assert engine.last_variant()["rays"] == 1 and engine.last_variant()["octree"] == 0
    finally:
        engine.set_exec(-1, 4)
    assert got.shape == want.shape
    for i in range(want.shape[0]):
        assert (want[i] > 0).sum() > 400
        assert_image_close(got[i], want[i], rtol=2e-5)


def test_rays_refuse_per_cell_opacities_and_msf(engine):
    cl = cloud("odd")
    vw = view(cl)
    opt = np.tile(np.array([[0.3, 1.0]], np.float32) * kappa(cl), (cl.CELLS, 1))
    msf = Job(cl, None, SOURCE=1, BATCH=1, SEED=0.43, **cases.msf_inputs(cl, dsc=True))
    engine.set_exec(1, 4)
    try:
        with pytest.raises(SocError, match="not applicable: per-cell opacities"):
            run_sca(engine, job(cl, SOURCE=1, BATCH=1, SEED=0.3, BG=1.0, OPT=opt), vw, 0, 0, 1000)
        engine.set_opt(None)
        with pytest.raises(SocError, match=r"not applicable: several scattering functions \(WITH_MSF\)"):
            run_sca(engine, msf, vw, 0, 0, 1000)
    finally:
        engine.set_scatter_table(None, msf.MSF[2][0])          # (what run_sca undoes after a launch of WITH_MSF)
        engine.set_opt(None)
        engine.set_abundances(None)
        engine.set_exec(-1, 4)


def test_automatic_mode_keeps_small_grids_on_the_direct_kernel(engine, oracle_soc):
    """below the floor of 8 bricks (a 24 x 16 x 28 grid is 2 x 1 x 2 bricks of 16^3 cells) automatic mode runs the direct kernel, alone
    and in a batch; soc_set_exec(1) runs the sweep there too"""
    cl = synth.cartesian_cloud(24, NY=16, NZ=28, seed=11)
    vw = view(cl)
    jb = job(cl, SOURCE=1, BATCH=1, SEED=0.3, BG=1.0)
    want, n = oracle_sim_sca(oracle_soc, jb, vw, 0, gid0=0, gid1=3000, nthreads=8)
    got, st = run_sca(engine, jb, vw, 0, 0, 3000)
    assert engine.last_passes() == 0 and engine.last_form() == 0
    assert st["tally_events"] == n
    assert_image_close(got, want)
    engine.sca_zero()
    engine.stats(reset=True)
    engine.batch_begin(0)
    _defer(engine, jb, 0, 0, 3000)
    engine.batch_end()
    engine.sync()
    assert engine.last_passes() == 0 and engine.last_form() == 0
    assert engine.stats()["tally_events"] == n
    got, st = _rays(engine, jb, vw, 0, 0, 3000)
    assert st["tally_events"] == n
    assert_image_close(got, want)
