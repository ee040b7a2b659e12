"""Healpix images seen from a position (`perspective`, NDIR < 0) and the Healpix sky as the source (sca SimRAM_HP) through the sweep of
rays on brick-local hierarchies (soc_brick.hip: soc_lray_pass<true>, soc_sca_events) against the CPU oracle: identical trajectories
(image contributions, packets, scatterings equal) and images equal to fp32 summation order -- the bar of tests/test_gpu_sca_rays.py.
A peel-off ray of these images ends at the observer (observer inside the cloud) or leaves the model first (observer outside it)."""
import numpy as np
import pytest

import cases
from oracle.pyoracle import Job, oracle_sim_sca
from soc_amd.lib import SocError
from test_gpu_ltree import cloud104
from test_gpu_sca import assert_image_close, run_sca

pytestmark = pytest.mark.gpu

OBSERVERS = {"inside": (52.3, 51.7, 50.9), "outside": (150.0, 40.0, 60.0)}


def hview(where, FFS=1, nside=8):
    return cases.sca_view(healpix=(nside, OBSERVERS[where]), FFS=FFS)


@pytest.fixture(params=[0, 64, 1], ids=["park4096", "park64", "nopark"])
def parking(request, engine):
    engine.set_tuning(park_below=request.param)
    yield
    engine.set_tuning(park_below=0)


def _k(cl):
    return 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))


def _hpjob(weighted, **kw):
    cl = cloud104()
    bg, P = cases.hp_sky(weighted=weighted)
    return Job(cl, cases._CSC, ABS=0.3 * _k(cl), SCA=_k(cl), HPBG=bg, HPBGP=P, DSC=cases._DSC, **kw)


def _bgjob(**kw):
    cl = cloud104()
    kw.setdefault("SOURCE", 1)
    kw.setdefault("BG", 1.0)
    return Job(cl, cases._CSC, ABS=0.3 * _k(cl), SCA=_k(cl), DSC=cases._DSC, **kw)


def _check_variant(engine, kind, healpix=1):
    assert engine.last_passes() > 0 and engine.last_form() == 3
    v = engine.last_variant()
    assert v["rays"] == 1 and v["healpix"] == healpix and v["hpsky"] == (1 if kind == 3 else 0)


def _rays(engine, job, view, kind, g0, g1):
    engine.set_exec(1, 4)
    try:
        img, st = run_sca(engine, job, view, kind, g0, g1 - g0)
        _check_variant(engine, kind, healpix=1 if view.nside else 0)
        assert engine.sca_ray_steps() > st["packets"]
    finally:
        engine.set_exec(-1, 4)
    return img, st


def _direct(engine, job, view, kind, g0, g1):
    engine.set_exec(0, 4)
    try:
        img, st = run_sca(engine, job, view, kind, g0, g1 - g0)
        assert engine.last_passes() == 0
    finally:
        engine.set_exec(-1, 4)
    return img, st


def _parity(engine, oracle_soc, job, view, kind, g0, g1):
    want, n = oracle_sim_sca(oracle_soc, job, view, kind, gid0=g0, gid1=g1, nthreads=8)
    got, st = _rays(engine, job, view, kind, g0, g1)
    assert st["tally_events"] == n and n > 0
    assert_image_close(got, want, rtol=1e-5)
    return st


# ---- 1. oracle parity, observer inside and outside the cloud ----

@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("ffs", [1, 0])
def test_background_healpix(ffs, where, engine, oracle_soc):
    g0, g1 = 100000, 102000
    st = _parity(engine, oracle_soc, _bgjob(BATCH=3, SEED=0.377), hview(where, FFS=ffs), 0, g0, g1)
    assert st["packets"] == 3 * (g1 - g0) and st["scatterings"] > 500


@pytest.mark.parametrize("where", ["inside", "outside"])
def test_point_sources_healpix(where, engine, oracle_soc):
    ps = np.array([[52.3, 51.7, 50.2], [52.0, 52.0, 300.0]], np.float32)
    job = _bgjob(SOURCE=0, BG=0.0, BATCH=12, SEED=0.2, GLOBAL=512, PSPOS=ps, PS=[1.0, 2.5], PS_METHOD=0)
    for kind in (2, 0):                                   # SimRAM_PS, and the point sources of SimRAM_PB
        st = _parity(engine, oracle_soc, job, hview(where, nside=16), kind, 0, 512)
        assert st["packets"] == 12 * 512


@pytest.mark.parametrize("where", ["inside", "outside"])
def test_cell_emission_healpix(where, engine, oracle_soc):
    cl = cloud104()
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    job = _bgjob(SOURCE=2, BG=0.0, BATCH=1, SEED=0.9, GLOBAL=8192, EMIT=emit)
    st = _parity(engine, oracle_soc, job, hview(where), 1, 4000, 4024)
    assert st["packets"] > 1000


@pytest.mark.parametrize("where", ["inside", "outside"])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
def test_healpix_sky_healpix(weighted, where, engine, oracle_soc):
    job = _hpjob(weighted, BATCH=4, SEED=0.37, GLOBAL=3000)
    st = _parity(engine, oracle_soc, job, hview(where), 3, 0, 3000)
    assert st["packets"] == 4 * 3000 and st["scatterings"] > 500


# the background and the sky again: short brick queues parked or not, and slow steps on distance-limited rays

@pytest.mark.parametrize("tune", [dict(), dict(slow_every=3)], ids=["plain", "slow3"])
def test_background_healpix_parking(tune, engine, oracle_soc, tuned, parking):
    tuned(**tune)
    _parity(engine, oracle_soc, _bgjob(BATCH=2, SEED=0.51), hview("inside"), 0, 200000, 201500)


@pytest.mark.parametrize("tune", [dict(), dict(slow_every=3)], ids=["plain", "slow3"])
def test_healpix_sky_healpix_parking(tune, engine, oracle_soc, tuned, parking):
    tuned(**tune)
    _parity(engine, oracle_soc, _hpjob(True, BATCH=3, SEED=0.23, GLOBAL=2000), hview("inside"), 3, 0, 2000)


# ---- 2. the Healpix sky with flat images ----

def test_healpix_sky_flat_images(engine, oracle_soc):
    from test_gpu_sca_rays import view104
    job = _hpjob(False, BATCH=4, SEED=0.61, GLOBAL=3000)
    want, n = oracle_sim_sca(oracle_soc, job, view104(), 3, nthreads=8)
    got, st = _rays(engine, job, view104(), 3, 0, 3000)
    assert st["tally_events"] == n and st["packets"] == 4 * 3000
    assert_image_close(got, want, rtol=1e-5)


# ---- 3. the direct kernel as the second witness, on launches larger than the oracle takes in seconds ----

@pytest.mark.parametrize("mirror", [0, 21])
def test_direct_kernel_as_second_witness(mirror, engine):
    view = hview("inside", nside=16)
    launches = [(0, _bgjob(BATCH=2, SEED=0.61, MIRROR=mirror), 0, 60000),
                (3, _hpjob(False, BATCH=2, SEED=0.43, GLOBAL=60000, MIRROR=mirror), 0, 60000)]
    try:
        for kind, job, g0, g1 in launches:
            a, sa = _direct(engine, job, view, kind, g0, g1)
            b, sb = _rays(engine, job, view, kind, g0, g1)
            assert sa == sb and sb["packets"] >= 100000
            assert_image_close(b, a, rtol=2e-5)
    finally:
        engine.set_mirror(0)


# ---- 4. a batch of SimRAM_HP, SimRAM_PB and SimRAM_CL launches over three 'frequencies' ----

def _defer(eng, job, kind, g0, g1):
    """the calls of run_sca without the ones that would run what is pending (zero, stats, sync, read)"""
    eng.set_optical(job.ABS, job.SCA)
    eng.set_scatter_table(job.DSC, job.CSC)
    if kind == 3:
        eng.set_hpbg(job.HPBG, job.HPBGP)
        eng.sca_sim_hp(job.PACKETS, job.BATCH, job.SEED, job.GLOBAL, gid_first=g0, gid_count=g1 - g0)
    elif kind == 0:
        eng.sca_sim_pb(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.BG, job.PSPOS[:, :3], job.PS,
                       XPS=(job.XPS_NSIDE, job.XPS_SIDE, job.XPS_AREA), GLOBAL=job.GLOBAL, gid_first=g0, gid_count=g1 - g0)
    else:
        eng.set_emission(job.EMIT, job.EMWEI)
        eng.sca_sim_cl(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.GLOBAL, gid_first=g0, gid_count=g1 - g0)


def test_a_batch_of_sky_background_and_emission(engine, parking):
    from soc_amd import synth
    cl = cloud104()
    k = _k(cl)
    view = hview("inside")
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    tabs = [synth.hg_scattering_table(g) for g in (0.6, 0.2, 0.4)]                # (DSC, CSC)
    freqs = []
    for f in range(3):
        kw = dict(ABS=(0.2 + 0.1 * f) * k, SCA=(1.0 - 0.2 * f) * k, DSC=tabs[f][0])
        sky, P = cases.hp_sky(seed=8 + f, weighted=(f == 1))
        freqs.append([(3, Job(cl, tabs[f][1], BATCH=2, SEED=0.25 + 0.1 * f, GLOBAL=6000, HPBG=sky * (1 + f), HPBGP=P, **kw), 0, 6000),
                      (0, Job(cl, tabs[f][1], SOURCE=1, BATCH=2, SEED=0.3 + 0.1 * f, BG=1.0 + f, **kw), 1000, 11000),
                      (1, Job(cl, tabs[f][1], SOURCE=2, BATCH=1, SEED=0.4 + 0.1 * f, GLOBAL=16384, EMIT=emit * (1 + f), **kw), 0, 8192)])
    single, stats = [], []
    for launches in freqs:
        img = None
        tot = dict(tally_events=0, packets=0, scatterings=0)
        for kind, job, g0, g1 in launches:
            a, st = _rays(engine, job, view, kind, g0, g1)
            img = a.astype(np.float64) if img is None else img + a
            for key in tot:
                tot[key] += st[key]
        single.append(img)
        stats.append(tot)
    engine.set_exec(1, 4)
    try:
        engine.stats(reset=True)
        engine.batch_begin(0)
        engine.sca_batch_images(3)
        for f, launches in enumerate(freqs):
            engine.sca_batch_select(f)
            for kind, job, g0, g1 in launches:
                _defer(engine, job, kind, g0, g1)
        assert engine.last_passes() == 0                          # nothing has run yet ...
        engine.batch_end()
        st = engine.stats()
        _check_variant(engine, 3)                                 # ... and all of it ran as one sweep of rays, the sky among them
        for key in ("tally_events", "packets", "scatterings"):
            assert st[key] == sum(s[key] for s in stats)
        for f in range(3):
            assert_image_close(engine.sca_batch_read(f), single[f], rtol=2e-5)
    finally:
        engine.sca_batch_images(0)
        engine.set_exec(-1, 4)


# ---- 5. end to end: the scattering run (python -m soc_amd.asocs) with `perspective` + `outnside`, and with `hpbg` ----

_E2E = {}


def _thin_cloud104():
    """cloud104 with its densities scaled to an optical depth of about 2 across the root grid for the dust of test_host._write_model
    (kappa_abs + kappa_sca = 581 per unit density and cell at `gridlength 0.5`): peel-off rays to an observer in the cloud's centre
    carry light (at the file's own densities exp(-tau) is 0 for every one of them)"""
    if "c" not in _E2E:
        from soc_amd import synth
        cl = cloud104()
        root = cl.DENS[:104 ** 3]
        f = np.float32(2.0 / (581.0 * 104 * float(root[root > 0].mean())))
        _E2E["c"] = synth.Cloud(cl.NX, cl.NY, cl.NZ, [np.where(h > 0, h * f, h) for h in cl.H])      # (links <= 0 stay as they are)
    return _E2E["c"]


def _oracle_engine():
    """OracleEngine, its scattered-light launches on 8 threads (the background block is 8 * AREA = 519168 work items per frequency)"""
    from oracle.pyoracle import oracle_sim_sca as sim
    from oracle_engine import OracleEngine

    class Threaded(OracleEngine):
        def _sca(self, kind, job, GLOBAL, gid_first, gid_count):
            gid_count = GLOBAL - gid_first if gid_count is None else gid_count
            _, n = sim(self.orc, job, self.view, kind, gid_first, gid_first + gid_count, OUT=self.OUT, nthreads=8)
            self.events += n
    return Threaded("soc")


@pytest.mark.parametrize("hpbg", [None, 0, 1], ids=["background", "hpbg", "hpbg_weighted"])
def test_scattering_run_perspective_end_to_end(hpbg, engine, tmp_path):
    """the host loop of soc_amd.asocs unchanged: every launch of a source block is deferred into one batch (an image per frequency), which
    runs as one sweep of rays; each image equals the oracle engine's"""
    import os
    from soc_amd.asocs import ScatteringRun
    from soc_amd.ini import User
    from test_host import _write_model
    d = str(tmp_path)
    extra = "perspective 52.3 51.7 50.9\noutnside 8\nbgpackets 60000\n"
    if hpbg is not None:
        sky = np.random.default_rng(3).lognormal(0, 1, (2, 49152)).astype(np.float32) * 1e-13
        sky.tofile(os.path.join(d, "sky.bin"))
        extra += "hpbg %s/sky.bin 1.0 %d\n" % (d, hpbg)
    ini = _write_model(d, _thin_cloud104(), nfreq=2, extra=extra)
    os.chdir(d)
    want = ScatteringRun(User(ini), _oracle_engine(), verbose=0).run()
    engine.set_exec(1, 4)
    try:
        got = ScatteringRun(User(ini), engine, verbose=0).run()
        _check_variant(engine, 0 if hpbg is None else 3)              # the block's batch ran as one sweep of rays of a Healpix image
    finally:
        engine.set_exec(-1, 4)
    assert got.shape == want.shape == (2, 768)
    for i in range(want.shape[0]):
        assert (want[i] > 0).sum() > 700                            # (light in nearly every pixel)
        assert_image_close(got[i], want[i], rtol=2e-5)


# ---- 6. still refused ----

def test_healpix_rays_refuse_per_cell_opacities_and_msf(engine):
    cl = cloud104()
    view = hview("inside")
    opt = np.tile(np.array([[0.3, 1.0]], np.float32) * _k(cl), (cl.CELLS, 1))
    msf = Job(cl, None, SOURCE=1, BATCH=1, SEED=0.43, **cases.msf_inputs(cl, dsc=True))
    engine.set_exec(1, 4)
    try:
        # (each refusal names its own reason)
        with pytest.raises(SocError, match="not applicable: per-cell opacities"):
            run_sca(engine, _bgjob(BATCH=1, SEED=0.3, OPT=opt), view, 0, 0, 1000)
        engine.set_opt(None)
        with pytest.raises(SocError, match=r"not applicable: several scattering functions \(WITH_MSF\)"):
            run_sca(engine, msf, view, 0, 0, 1000)
    finally:
        engine.set_scatter_table(None, msf.MSF[2][0])          # (what run_sca undoes after a launch of WITH_MSF)
        engine.set_opt(None)
        engine.set_abundances(None)
        engine.set_exec(-1, 4)


def test_healpix_view_on_a_grid_that_is_not_brick_local_runs_the_direct_kernel(engine, oracle_soc):
    ref, kind, mk, vkw = cases.SCA_CASES["sca_hpx_bg_oct8_out"]
    job, view = mk(), cases.sca_view(**vkw)
    want, n = oracle_sim_sca(oracle_soc, job, view, kind)
    got, st = run_sca(engine, job, view, kind)
    assert engine.last_passes() == 0 and engine.last_form() == 0
    assert st["tally_events"] == n
    assert_image_close(got, want)
