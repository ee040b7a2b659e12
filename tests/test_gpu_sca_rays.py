"""Scattered-light images through the sweep of rays on brick-local hierarchies (soc_brick.hip: soc_lbrick_walk<., RAY> +
soc_sca_events) against the CPU oracle: identical trajectories (image contributions, packets, scatterings equal) and images
equal to fp32 summation order (1e-5 per pixel) -- the bar of tests/test_gpu_sca.py for the direct kernel, which is the second
witness here.  The hierarchy is one whose Index() the reference evaluates in double (104^3 roots, 4 levels)."""
import math

import numpy as np
import pytest

import cases
from oracle.pyoracle import Job, ScaView, oracle_sim_sca
from soc_amd import launch
from test_gpu_ltree import cloud104
from test_gpu_sca import assert_image_close, run_sca
from util import EMW, assert_zero_weights_skipped, cl_packets, emission_weights

pytestmark = pytest.mark.gpu


def view104(FFS=1, angles=((30.0, 40.0), (90.0, 0.0), (0.0, 0.0)), NPIX=(40, 36)):
    th = [math.radians(a[0]) for a in angles]
    ph = [math.radians(a[1]) for a in angles]
    _, OD, RA, DE = launch.set_observer_directions(th, ph)
    return ScaView(OD, RA, DE, NPIX=NPIX, MAP_DX=3.1, CENTRE=(52.0, 52.0, 52.0), FFS=FFS)


@pytest.fixture(params=[0, 64, 1], ids=["park4096", "park64", "nopark"])
def parking(request, engine):
    engine.set_tuning(park_below=request.param)
    yield
    engine.set_tuning(park_below=0)


def _rays(engine, job, view, kind, g0, g1):
    engine.set_exec(1, 4)
    try:
        img, st = run_sca(engine, job, view, kind, g0, g1 - g0)
        assert engine.last_passes() > 0 and engine.last_form() == 3 and engine.last_variant()["rays"] == 1
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


@pytest.mark.parametrize("tune", [dict(), dict(slow_every=3), dict(brick_cells=900, steps_per_visit=5), dict(chunk=64, threads=64)])
@pytest.mark.parametrize("ffs", [1, 0])
def test_background_rays(ffs, tune, engine, oracle_soc, tuned, parking):
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    job = Job(cl, cases._CSC, ABS=0.3 * k, SCA=k, SOURCE=1, BATCH=3, SEED=0.377, DSC=cases._DSC, BG=1.0)
    view = view104(FFS=ffs)
    g0, g1 = 100000, 103000
    want, n = oracle_sim_sca(oracle_soc, job, view, 0, gid0=g0, gid1=g1, nthreads=8)
    tuned(**tune)
    got, st = _rays(engine, job, view, 0, g0, g1)
    assert st["tally_events"] == n and st["packets"] == 3 * (g1 - g0) and st["scatterings"] > 1000
    assert_image_close(got, want)


def test_point_source_rays(engine, oracle_soc, parking):
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    ps = np.array([[52.3, 51.7, 50.2], [52.0, 52.0, 300.0]], np.float32)
    job = Job(cl, cases._CSC, ABS=0.3 * k, SCA=k, SOURCE=0, BATCH=12, SEED=0.2, GLOBAL=512, PSPOS=ps, PS=[1.0, 2.5], PS_METHOD=0, DSC=cases._DSC)
    view = view104()
    for kind in (2, 0):                                   # SimRAM_PS, and the point sources of SimRAM_PB
        want, n = oracle_sim_sca(oracle_soc, job, view, kind, nthreads=8)
        got, st = _rays(engine, job, view, kind, 0, 512)
        assert st["tally_events"] == n and st["packets"] == 12 * 512
        assert_image_close(got, want)


@pytest.mark.parametrize("emw", EMW)
def test_cell_emission_rays(emw, engine, oracle_soc, parking):
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)

    def mk(e):
        return Job(cl, cases._CSC, ABS=0.3 * k, SCA=k, SOURCE=2, BATCH=1, SEED=0.9, GLOBAL=8192, EMIT=emit,
                   EMWEI=emission_weights(cl.CELLS, e), USE_EMWEIGHT=1 if e else 0, DSC=cases._DSC)
    job = mk(emw)
    view = view104()
    g0, g1 = 4000, 4024
    want, n = oracle_sim_sca(oracle_soc, job, view, 1, gid0=g0, gid1=g1, nthreads=8)
    if emw == "zeros":                                   # (cells without weight are stepped over)
        assert_zero_weights_skipped(job, mk(1), g0, g1, n, oracle_sim_sca(oracle_soc, mk(1), view, 1, gid0=g0, gid1=g1, nthreads=8)[1])
    got, st = _rays(engine, job, view, 1, g0, g1)
    assert st["tally_events"] == n and st["packets"] > 1000
    if emw == "zeros":
        assert st["packets"] == cl_packets(job, g0, g1)
    assert_image_close(got, want)


def test_reflecting_faces_and_the_direct_kernel_as_second_witness(engine, parking):
    """a larger launch than the oracle takes in seconds: both execution modes of the library, event counts equal, images to summation order;
    with reflecting faces (mask 21: one face per axis, see test_gpu_ltree.test_reflecting_faces_in_the_sweep) and without"""
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    view = view104(angles=((60.0, 200.0), (10.0, 80.0)))
    for mirror in (0, 21):
        job = Job(cl, cases._CSC, ABS=0.3 * k, SCA=k, SOURCE=1, BATCH=2, SEED=0.61, DSC=cases._DSC, BG=1.0, MIRROR=mirror)
        a, sa = _direct(engine, job, view, 0, 0, 60000)
        b, sb = _rays(engine, job, view, 0, 0, 60000)
        assert sa == sb
        assert_image_close(b, a)
    engine.set_mirror(0)


def test_a_batch_of_launches_with_an_image_per_frequency(engine, parking):
    """soc_batch_begin ... soc_batch_end around scattered-light launches: point-source, background and cell-emission launches of several
    'frequencies' (own opacities, scattering functions, emission, seeds) deferred into ONE sweep of rays, each frequency adding to its own
    image (soc_sca_batch_images / _select / _read).  Every image equals the one the same launches give one at a time."""
    from soc_amd import synth
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    view = view104(angles=((60.0, 200.0), (10.0, 80.0)))
    ps = np.array([[52.3, 51.7, 50.2]], np.float32)
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    tabs = [synth.hg_scattering_table(g) for g in (0.6, 0.2, 0.4)]                # (DSC, CSC)
    freqs = []
    for f in range(3):
        kw = dict(ABS=(0.2 + 0.1 * f) * k, SCA=(1.0 - 0.2 * f) * k, DSC=tabs[f][0])
        freqs.append([(2, Job(cl, tabs[f][1], SOURCE=0, BATCH=6, SEED=0.2 + 0.1 * f, GLOBAL=4096, PSPOS=ps, PS=[1.0 + f], **kw), 0, 4096),
                      (0, Job(cl, tabs[f][1], SOURCE=1, BATCH=2, SEED=0.3 + 0.1 * f, BG=1.0 + f, **kw), 1000, 21000),
                      (1, Job(cl, tabs[f][1], SOURCE=2, BATCH=1, SEED=0.4 + 0.1 * f, GLOBAL=16384, EMIT=emit * (1 + f), **kw), 0, 16384)])
    # one at a time (rays too), one image
    single, stats = [], []
    for launches in freqs:
        img = None
        tot = dict(tally_events=0, packets=0, scatterings=0)
        for kind, job, g0, g1 in launches:
            engine.set_exec(1, 4)
            a, st = run_sca(engine, job, view, kind, g0, g1 - g0)
            img = a.astype(np.float64) if img is None else img + a
            for key in tot:
                tot[key] += st[key]
        single.append(img)
        stats.append(tot)
    # the same launches in one batch (soc_set_exec(1): in automatic mode a batch this small would go through the direct kernel)
    engine.set_exec(1, 4)
    engine.stats(reset=True)
    engine.batch_begin(0)
    engine.sca_batch_images(3)
    for f, launches in enumerate(freqs):
        engine.sca_batch_select(f)
        for kind, job, g0, g1 in launches:
            _defer(engine, job, view, kind, g0, g1 - g0)
    assert engine.last_passes() == 0                              # nothing has run yet (a launch run at once as rays would have left its passes) ...
    engine.batch_end()
    st = engine.stats()
    assert engine.last_form() == 3 and engine.last_passes() > 0   # ... and all of it ran as one sweep
    assert engine.last_variant()["rays"] == 1                     # (of rays)
    for key in ("tally_events", "packets", "scatterings"):
        assert st[key] == sum(s[key] for s in stats)
    for f in range(3):
        assert_image_close(engine.sca_batch_read(f), single[f], rtol=2e-5)
    engine.sca_batch_images(0)
    engine.set_exec(-1, 4)


def _defer(eng, job, view, kind, gid_first, gid_count):
    """the calls of run_sca without the ones that would run what is pending (zero, stats, sync, read)"""
    eng.set_optical(job.ABS, job.SCA)
    eng.set_scatter_table(job.DSC, job.CSC)
    xps = (job.XPS_NSIDE, job.XPS_SIDE, job.XPS_AREA)
    if kind == 2:
        eng.sca_sim_ps(job.PACKETS, job.BATCH, job.SEED, job.BG, job.PSPOS[:, :3], job.PS, XPS=xps, GLOBAL=job.GLOBAL, gid_first=gid_first, gid_count=gid_count)
    elif kind == 0:
        eng.sca_sim_pb(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.BG, job.PSPOS[:, :3], job.PS, XPS=xps, GLOBAL=job.GLOBAL, gid_first=gid_first, gid_count=gid_count)
    else:
        eng.set_emission(job.EMIT, job.EMWEI)
        eng.sca_sim_cl(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.GLOBAL, gid_first=gid_first, gid_count=gid_count)


def _run_batches(eng, cl, view, batches):
    """zeroed image and TABS, then every batch between its own batch_begin and batch_end (soc_set_exec(1): small batches still sweep);
    a launch is (kind, job, gid_first, gid_end) with kind None for an absorption launch (SimRAM_PB, or SimRAM_CL for SOURCE 2), or a
    function of the engine that makes calls of its own"""
    eng.set_cloud(cl)
    eng.set_features(0, 0, 0)
    eng.set_opt(None)
    eng.set_mirror(0)
    eng.set_exec(1, 4)
    try:
        eng.sca_set_view(view.ODIR, view.RA, view.DE, view.NPIX, view.MAP_DX, view.CENTRE, view.FFS)
        eng.sca_zero()
        eng.zero(0)
        eng.stats(reset=True)
        for launches in batches:
            eng.batch_begin(0)
            for launch in launches:
                if callable(launch):
                    launch(eng)
                    continue
                kind, job, g0, g1 = launch
                if kind is not None:
                    _defer(eng, job, view, kind, g0, g1 - g0)
                    continue
                eng.set_optical(job.ABS, job.SCA)
                eng.set_scatter_table(job.DSC, job.CSC)
                if job.SOURCE == 2:
                    eng.set_emission(job.EMIT, job.EMWEI)
                    eng.sim_cl(2, job.PACKETS, job.BATCH, job.SEED, job.TW, job.GLOBAL, gid_first=g0, gid_count=g1 - g0)
                else:
                    eng.sim_pb(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.BG, job.TW, GLOBAL=job.GLOBAL, gid_first=g0, gid_count=g1 - g0)
            eng.batch_end()
        eng.sync()
        return eng.sca_read_out(), eng.read_tally(0), eng.stats()
    finally:
        eng.set_exec(-1, 4)


def test_a_batch_of_both_families(engine):
    """scattered-light launches, then absorption launches, then scattered-light launches again in ONE batch: a sweep holds the launches of
    one family, so each change of family runs what is pending.  Event counts, image and TABS equal those of the same launches with the
    batch ended and begun again by hand at each change of family."""
    from soc_amd import synth
    from util import assert_tally_close
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    view = view104(angles=((60.0, 200.0), (10.0, 80.0)))
    ps = np.array([[52.3, 51.7, 50.2]], np.float32)
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    dsc2, csc2 = synth.hg_scattering_table(0.2)
    sca1 = dict(ABS=0.3 * k, SCA=k, DSC=cases._DSC)
    sca2 = dict(ABS=0.2 * k, SCA=0.8 * k, DSC=dsc2)
    families = [
        [(0, Job(cl, cases._CSC, SOURCE=1, BATCH=2, SEED=0.31, BG=1.0, **sca1), 1000, 21000),
         (2, Job(cl, cases._CSC, SOURCE=0, BATCH=6, SEED=0.22, GLOBAL=4096, PSPOS=ps, PS=[1.5], **sca1), 0, 4096),
         (1, Job(cl, cases._CSC, SOURCE=2, BATCH=1, SEED=0.43, GLOBAL=16384, EMIT=emit, **sca1), 0, 8192)],
        [(None, Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=4, SEED=0.377, BG=1.0), 100000, 106000),
         (None, Job(cl, csc2, ABS=2e-6, SCA=5e-5, SOURCE=2, BATCH=1, SEED=0.59, GLOBAL=16384, EMIT=emit, TW=0.5), 0, 8192)],
        [(1, Job(cl, csc2, SOURCE=2, BATCH=1, SEED=0.61, GLOBAL=16384, EMIT=emit * 2, **sca2), 4000, 12000),
         (0, Job(cl, csc2, SOURCE=1, BATCH=2, SEED=0.74, BG=2.0, **sca2), 30000, 45000)]]
    img_s, tabs_s, st_s = _run_batches(engine, cl, view, families)
    img, tabs, st = _run_batches(engine, cl, view, [sum(families, [])])
    assert engine.last_passes() > 0 and engine.last_form() == 3 and engine.last_variant()["rays"] == 1
    assert st == st_s and st["tally_events"] > 0 and st["scatterings"] > 0
    assert (img_s > 0).sum() > 100 and (tabs_s > 0).sum() > 1000
    assert_image_close(img, img_s)
    assert_tally_close(tabs, tabs_s, rtol=1e-5)


def test_a_refused_launch_in_a_batch_leaves_the_deferred_ones(engine):
    """a soc_sca_sim_* call refused inside a batch (its work items outside GLOBAL) raises; the launches deferred before and after it
    run at soc_batch_end as they would without it"""
    from soc_amd.lib import SocError
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    view = view104()
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    launches = [(0, Job(cl, cases._CSC, ABS=0.3 * k, SCA=k, SOURCE=1, BATCH=2, SEED=0.52, BG=1.0, DSC=cases._DSC), 2000, 14000),
                (1, Job(cl, cases._CSC, ABS=0.3 * k, SCA=k, SOURCE=2, BATCH=1, SEED=0.18, GLOBAL=8192, EMIT=emit, DSC=cases._DSC), 0, 8192)]
    want, _, st_want = _run_batches(engine, cl, view, [launches])

    def refused(eng):
        with pytest.raises(SocError, match="outside GLOBAL"):
            eng.sca_sim_pb(1, 0, 2, 0.5, 1.0, GLOBAL=1000, gid_first=900, gid_count=200)
    got, _, st = _run_batches(engine, cl, view, [[launches[0], refused, launches[1]]])
    assert st == st_want and st["tally_events"] > 0
    assert_image_close(got, want)
