"""Prologue and flush of the brick-local walk (soc_lbrick_walk): the brick's slots reach LDS in batches of loads, the tallies leave it in
batches of cell numbers with the tally pointers of the workgroup's launches in scalar registers; the ranks of the chunk's packets in the
arrivals table follow.  A slot not copied, copied to the wrong place or not flushed shows as another trajectory or a missing cell; a
pointer of the wrong launch as a tally in the wrong array.

Every case, on the 104^3-root, 4-level hierarchy of tests/test_gpu_ltree.py (the float form on its own 64^3-root one): tally events equal
to the oracle's, packets equal to the launch's count, tallies per cell to the 1e-5 of the walk tests (fp32 summation order), and packets,
tally events and scatterings equal to the same launch through the general kernel of the sweep (`general_kernel`) -- over a whole sweep
these counts are right only if every pass's queues were."""
import numpy as np
import pytest

import cases
from oracle.pyoracle import Job
from test_gpu_ltree import cloud104
from test_gpu_ltree_abu import opt104
from test_gpu_ltree_float import bg_job as float_bg_job
from test_gpu_tally_order import _check, _launch, _one, _oracle
from test_gpu_walk_outcomes import _bg, _ps, _thick
from util import assert_tally_close

pytestmark = pytest.mark.gpu


def _bgjob():
    return _bg(BATCH=3, SEED=0.43)


# ---- the copy and the flush at every remainder of a brick's slots modulo threads x batch ----

@pytest.mark.parametrize("brick_cells", [600, 4097, 8704])
def test_bricks_of_every_size(brick_cells, engine, oracle_soc, tuned):
    """thousands of bricks of up to 600 slots (fewer slots than threads, one batch), of up to 4097 (a batch and a slot), and the full
    8704 (17 slots per thread: two batches and one slot)"""
    job, g0, cnt = _bgjob(), 300000, 4000
    T, _, n, _ = _oracle(oracle_soc, "pf_bg", job, 0, g0, g0 + cnt)
    _check(engine, tuned, dict(brick_cells=brick_cells), _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)


# ---- a prologue whose copy is skipped, a flush that must not run, the keys handed back ----

@pytest.mark.parametrize("park", [0, 64], ids=["park4096", "park64"])
@pytest.mark.parametrize("case", ["ps1", "ps65", "bg"])
def test_short_and_parked_queues(case, park, engine, oracle_soc, tuned):
    """one brick queue of 1 and of 65 packets (parked pass after pass until nothing else is left), and the thousands of short queues of a
    background launch; short queues parked below 4096 packets (the default) and below 64"""
    if case == "bg":
        job, g0, cnt = _bgjob(), 300000, 4000
        T, _, n, _ = _oracle(oracle_soc, "pf_bg", job, 0, g0, g0 + cnt)
    else:
        job, g0, cnt = _ps(), 0, int(case[2:])
        T, _, n, _ = _oracle(oracle_soc, "pf_" + case, job, 0, g0, g0 + cnt)
    _check(engine, tuned, dict(park_below=park), _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)


# ---- every array of every instance, to the arrays of the workgroup's own launches ----

def test_flush_of_tabs_and_int_side_by_side(engine, oracle_soc, tuned):
    """WINT 1: two launches that share one INT array with different weights TW (batch_begin_shared_int, as
    tests/test_gpu_ltree_abu.py::test_point_sources_inside_and_outside builds it)"""
    cl = cloud104()
    jobs = [Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=2, SEED=0.377, WITH_INT=1, TW=1.5),
            Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=3, SEED=0.52, WITH_INT=1, TW=0.7)]
    g0, g1 = 200000, 202000
    T2, I2 = np.zeros(cl.CELLS, np.float32), np.zeros(cl.CELLS, np.float32)
    n2 = sum(oracle_soc.sim(j, 0, gid0=g0, gid1=g1, nthreads=8, TABS=T2, INT=I2)[2] for j in jobs)

    def run():
        e = engine
        e.set_cloud(cl)
        e.set_features(1, 0, 0)
        e.set_scatter_table(None, cases._CSC)
        e.set_optical(3e-6, 3e-5)
        e.set_opt(None)
        e.set_mirror(0)
        e.set_exec(1, 4)
        try:
            e.zero(0)
            e.zero(1)
            e.stats(reset=True)
            e.batch_begin_shared_int(0)
            for j in jobs:
                e.sim_pb(1, 0, j.BATCH, j.SEED, j.BG, j.TW, GLOBAL=j.GLOBAL, gid_first=g0, gid_count=g1 - g0)
            e.batch_end()
            assert e.last_passes() > 0 and e.last_form() == 3 and e.last_variant()["wint"] == 1
            assert_tally_close(e.read_tally(1), I2, rtol=1e-5)
            return e.read_tally(0), e.stats()
        finally:
            e.set_features(0, 0, 0)
            e.set_exec(-1, 4)

    _check(engine, tuned, dict(), run, T2, n2, (g1 - g0) * sum(j.BATCH for j in jobs))


def test_flush_of_int_alone(engine, oracle_soc, tuned):
    """WINT 3: INT alone in LDS, TABS = TW * INT with the weight the flush takes from the group's first launch"""
    job = Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=2, SEED=0.47, WITH_INT=1, TW=1.5)
    g0, g1 = 200000, 203000
    T, I, n, _ = _oracle(oracle_soc, "pf_int3", job, 0, g0, g1)

    def ran(Tg, Ig):
        assert engine.last_variant()["wint"] == 3
        assert_tally_close(Ig, I, rtol=1e-5)

    _check(engine, tuned, dict(), _launch(engine, job, 0, g0, g1, ran), T, n, (g1 - g0) * job.BATCH)


def test_flush_of_the_intensity_vectors(engine, oracle_soc, tuned):
    """WINT 2: TABS, INT and the three vector sums, whose stride the flush reads once (bounds of
    tests/test_gpu_ltree.py::test_intensity_vectors_in_the_sweep: signed sums, measured against INT)"""
    job = Job(cloud104(), cases._CSC, ABS=3e-5, SCA=6e-5, SOURCE=1, BATCH=2, SEED=0.377, WITH_INT=2, TW=1.7)
    g0, g1 = 100000, 103000
    T, I, n, extra = _oracle(oracle_soc, "pf_int2", job, 0, g0, g1)
    want = extra["INTV"]
    assert np.abs(want).sum() > 0

    def ran(Tg, Ig):
        assert engine.last_variant()["wint"] == 2
        assert_tally_close(Ig, I, rtol=1e-5)
        for k in range(3):
            got = job.INTV_gpu[k]
            assert np.abs(got - want[k]).max() <= 2e-6 * np.abs(I).max()
            assert np.all(np.abs(got - want[k]) <= 1e-5 * np.maximum(I, 1e-3 * I.max()))

    _check(engine, tuned, dict(), _launch(engine, job, 0, g0, g1, ran), T, n, (g1 - g0) * job.BATCH)


def test_copy_and_flush_of_the_ali_instance(engine, oracle_soc, tuned):
    """ALI: the cell numbers of the brick's slots are copied beside the cells, and XAB is flushed beside TABS"""
    cl = cloud104()
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    job = Job(cl, cases._CSC, ABS=3e-4, SCA=6e-4, SOURCE=2, BATCH=2, SEED=0.9, GLOBAL=8192, EMIT=emit, WITH_ALI=1, TW=1.3)
    g0, g1 = 4000, 4064
    T, _, n, extra = _oracle(oracle_soc, "pf_ali", job, 1, g0, g1)
    want = extra["XAB"]
    assert want.sum() > 0
    packets = job.BATCH * sum(len(range(i, cl.CELLS, job.GLOBAL)) for i in range(g0, g1))
    _check(engine, tuned, dict(), _launch(engine, job, 1, g0, g1, lambda Tg, Ig: assert_tally_close(job.XAB_gpu, want, rtol=1e-5)), T, n, packets)


# ---- the copy of the per-cell opacities ----

@pytest.mark.parametrize("tune", [dict(brick_cells=600), dict()], ids=["cells600", "default"])
def test_copy_of_per_cell_opacities(tune, engine, oracle_soc, tuned):
    job = Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=4, SEED=0.377, OPT=opt104())
    g0, g1 = 100000, 103000
    T, _, n, _ = _oracle(oracle_soc, "pf_abu", job, 0, g0, g1)

    def ran(Tg, Ig):
        assert engine.last_variant()["abu"] == 1

    try:
        _check(engine, tuned, dict(abu_local=1, **tune), _launch(engine, job, 0, g0, g1, ran), T, n, (g1 - g0) * job.BATCH)
    finally:
        engine.set_opt(None)


# ---- the launches' constants in LDS and the pointers of a workgroup belong to the right launch ----

def test_two_launches_of_different_kinds_and_weights(engine, oracle_soc, tuned):
    """a point-source launch (SimRAM_PB, TW 1) and a cell-emission launch (SimRAM_CL, TW 0.5) with optical constants of their own in
    one sweep"""
    cl = cloud104()
    ps = np.array([[52.3, 51.7, 50.2]], np.float32)
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    a = Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=0, BATCH=20, SEED=0.2, GLOBAL=512, PSPOS=ps, PS=[1.0], PS_METHOD=0, TW=1.0)
    b = Job(cl, cases._CSC, ABS=5e-6, SCA=2e-5, SOURCE=2, BATCH=1, SEED=0.6, GLOBAL=8192, EMIT=emit, TW=0.5)
    Ta, _, na, _ = _oracle(oracle_soc, "pf_two_ps", a, 0, 0, 512)
    Tb, _, nb, _ = _oracle(oracle_soc, "pf_two_cl", b, 1, 4000, 4048)
    packets = a.BATCH * 512 + b.BATCH * sum(len(range(i, cl.CELLS, b.GLOBAL)) for i in range(4000, 4048))

    def run():
        e = engine
        e.set_cloud(cl)
        e.set_features(0, 0, 0)
        e.set_opt(None)
        e.set_mirror(0)
        e.set_exec(1, 4)
        try:
            e.zero(0)
            e.stats(reset=True)
            e.batch_begin(4)
            e.set_optical(a.ABS, a.SCA)
            e.set_scatter_table(a.DSC, a.CSC)
            e.sim_pb(0, a.PACKETS, a.BATCH, a.SEED, a.BG, a.TW, PSPOS=a.PSPOS[:, :3], PS=a.PS, GLOBAL=a.GLOBAL, gid_first=0, gid_count=512)
            e.set_optical(b.ABS, b.SCA)
            e.set_scatter_table(b.DSC, b.CSC)
            e.set_emission(b.EMIT, None)
            e.sim_cl(2, b.PACKETS, b.BATCH, b.SEED, b.TW, b.GLOBAL, gid_first=4000, gid_count=48)
            e.batch_end()
            assert e.last_passes() > 0 and e.last_form() == 3
            return e.read_tally(0), e.stats()
        finally:
            e.set_exec(-1, 4)

    _check(engine, tuned, dict(), run, Ta.astype(np.float64) + Tb, na + nb, packets)


# ---- the copy without tallies ----

def test_one_launch_of_rays(engine, oracle_soc):
    """soc_lray_pass: the brick's cells alone in LDS, nothing to flush.  A sweep of rays has one kernel for every kind, so the second
    witness is the direct kernel, to the tolerance of tests/test_gpu_sca_rays_healpix.py::test_direct_kernel_as_second_witness."""
    from test_gpu_sca import assert_image_close
    from test_gpu_sca_rays_healpix import _bgjob as ray_job, _direct, _parity, _rays, hview
    g0, g1 = 300000, 301500
    job, view = ray_job(BATCH=2, SEED=0.71), hview("outside")
    st = _parity(engine, oracle_soc, job, view, 0, g0, g1)
    assert st["packets"] == 2 * (g1 - g0)
    b, sb = _rays(engine, job, view, 0, g0, g1)
    a, sa = _direct(engine, job, view, 0, g0, g1)
    for key in ("packets", "tally_events", "scatterings"):
        assert sa[key] == sb[key] == st[key], key
    assert_image_close(b, a, rtol=2e-5)


# ---- the float form ----

@pytest.mark.parametrize("tune", [dict(brick_cells=600), dict()], ids=["cells600", "default"])
def test_float_form(tune, engine, oracle_soc, tuned):
    job, g0, g1 = float_bg_job("oct64_l4")
    T, _, n, _ = _oracle(oracle_soc, "pf_flt", job, 0, g0, g1)

    def ran(Tg, Ig):
        v = engine.last_variant()                          # the brick-local kernel in its float form (_launch asserts the form of the sweep, 3)
        assert v["form"] == 3 and v["kind"] == 4 and v["dbl"] == 0 and v["octree"] == 1

    _check(engine, tuned, dict(float_local=1, **tune), _launch(engine, job, 0, g0, g1, ran), T, n, (g1 - g0) * job.BATCH)


# ---- the arrivals table: one entry per queue, the hash table, and a hash table so small that keys are counted in global memory ----

@pytest.mark.parametrize("tune", [dict(), dict(brick_cells=600), dict(brick_cells=600, hash_slots=64)], ids=["per_queue", "hash1024", "hash64"])
def test_forms_of_the_arrivals_table(tune, engine, oracle_soc, tuned):
    """the thick cloud (scatterings: event queues beside the brick queues).  The default bricks of this hierarchy make a few hundred
    queues, bricks of 600 cells more than 2048: the open-addressing table, and with 64 entries one that overflows"""
    job, g0, cnt = _thick(), 200000, 3000
    T, _, n, _ = _oracle(oracle_soc, "pf_thick", job, 0, g0, g0 + cnt)
    st = _check(engine, tuned, tune, _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)
    assert st["scatterings"] > st["packets"]
