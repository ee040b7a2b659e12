"""The tally of the brick-local walk (soc_lbrick_walk) is issued after the landing of the step, not ahead of it: the amounts are formed
where they were, the LDS atomics follow soc_lt_land.  Every case is the smallest shape at which a tally deferred like that can be lost or
added twice, on the smallest hierarchy that takes this walk (104^3 roots, 4 levels; the float form on its own 64^3-root hierarchy).

Every case: tally events equal to the oracle's (identical trajectories), packets equal to the launch's count, tallies to the 1e-5 of the
existing walk tests (fp32 summation order), and packets, tally events and scatterings equal to those of the `general_kernel` witness."""
import numpy as np
import pytest

import cases
from oracle.pyoracle import Job
from soc_amd import synth
from test_gpu_ltree import cloud104
from test_gpu_ltree_abu import opt104
from test_gpu_ltree_float import bg_job as float_bg_job
from test_gpu_walk_outcomes import _bg, _deferred, _ps, _thick
from util import assert_tally_close, run_engine

pytestmark = pytest.mark.gpu

_WANT = {}


def _oracle(oracle_soc, name, job, kind, g0, g1):
    """the oracle's (TABS, INT, events) of a launch and what it left in the job (XAB, vector sums): computed once, shared by the tests
    that run it, never written to"""
    if name not in _WANT:
        T, I, n = oracle_soc.sim(job, kind, gid0=g0, gid1=g1, nthreads=8)
        extra = {k: np.array(getattr(job, k), np.float32).copy() for k in ("XAB", "INTV") if getattr(job, k, None) is not None}
        for a in (T, I) + tuple(extra.values()):
            if a is not None:
                a.setflags(write=False)
        _WANT[name] = (T, I, n, extra)
    return _WANT[name]


def _check(engine, tuned, tune, run, T, n, packets):
    """`run()` with the tuning of the case against the oracle, then with the general kernel as the second witness"""
    tuned(**tune)
    Tg, st = run()
    print(tune, "oracle tally events", n, "engine", st)
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert st["packets"] == packets
    assert_tally_close(Tg, T, rtol=1e-5)
    tuned(general_kernel=1)
    Tw, sw = run()
    print(tune, "general kernel", sw)
    for key in ("packets", "tally_events", "scatterings"):
        assert st[key] == sw[key], key
    assert_tally_close(Tg, Tw, rtol=1e-5)
    return st


def _one(engine, job, g0, cnt):
    def run():
        T, _, st = _deferred(engine, job, g0, g0 + cnt)
        return T, st
    return run


def test_every_step_ends_a_visit(engine, oracle_soc, tuned):
    """steps_per_visit 1: the outcome of every step is leave, exit or own-queue, and the lane's packet is stored by the next entry of
    the swap arm -- the tally of such a step still lands"""
    job, g0, cnt = _bg(BATCH=3, SEED=0.29), 400000, 4000
    T, _, n, _ = _oracle(oracle_soc, "bg", job, 0, g0, g0 + cnt)
    _check(engine, tuned, dict(steps_per_visit=1), _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)


@pytest.mark.parametrize("cnt", [1, 63, 64, 65])
def test_the_last_iteration_of_a_wave(cnt, engine, oracle_soc, tuned):
    """one brick queue of 1, 63, 64 and 65 packets: the atomic of a wave's last iteration is in flight when the wave leaves the loop, ahead
    of the barrier and the flush of the tallies to global memory"""
    job = _ps()
    T, _, n, _ = _oracle(oracle_soc, "ps%d" % cnt, job, 0, 0, cnt)
    _check(engine, tuned, dict(), _one(engine, job, 0, cnt), T, n, cnt)


def test_scatterings_tally_nothing(engine, oracle_soc, tuned):
    """the thick cloud: a lane whose free path ends in the cell does not move, and nothing is tallied for it"""
    job = _thick()
    g0, cnt = 200000, 3000
    T, _, n, _ = _oracle(oracle_soc, "thick", job, 0, g0, g0 + cnt)
    st = _check(engine, tuned, dict(), _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)
    assert st["scatterings"] > st["packets"]


def test_slow_outcome_after_the_tally_was_formed(engine, oracle_soc, tuned):
    """slow_every 3: the step goes to the slow-step queue after its amounts were formed; it has crossed its cell and tallies"""
    job, g0, cnt = _bg(BATCH=3, SEED=0.61), 100000, 4000
    T, _, n, _ = _oracle(oracle_soc, "slow", job, 0, g0, g0 + cnt)
    _check(engine, tuned, dict(slow_every=3), _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)


def _deep_point(cl):
    """a point inside a cell of the deepest level (3): the root cell, then the octants of the chain of refined cells down to a level-2
    cell that is refined, then one of its children"""
    assert cl.LEVELS == 4
    idx = int(np.flatnonzero(cl.H[2] <= 0)[0])             # a refined cell of level 2: its children are leaves of level 3
    pos = np.array([0.37, 0.62, 0.55]) / 8.0 + np.array([1, 0, 1]) / 8.0      # inside child 5 (x + 2y + 4z) of it, in root-cell units
    for level in (2, 1):
        o = idx % 8
        pos += np.array([o & 1, (o >> 1) & 1, (o >> 2) & 1]) / float(1 << level)
        up = cl.H[level - 1]
        parents = np.flatnonzero((up <= 0) & (synth.F2I(-up) == 8 * (idx // 8)))
        assert len(parents) == 1
        idx = int(parents[0])
    root = np.array([idx % cl.NX, (idx // cl.NX) % cl.NY, idx // (cl.NX * cl.NY)])
    return (root + pos).astype(np.float32)


def test_descents_of_three_trips(engine, oracle_soc, tuned):
    """a point source inside the level-3 region: the packets are placed and make their first steps with descents through all levels --
    the landing whose waits the tally no longer stands ahead of"""
    cl = cloud104()
    ps = _deep_point(cl)[None, :]
    job = Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=0, BATCH=1, SEED=0.31, GLOBAL=8192, PSPOS=ps, PS=[1.0], PS_METHOD=0)
    cnt = 2000
    T, _, n, _ = _oracle(oracle_soc, "deep", job, 0, 0, cnt)
    _check(engine, tuned, dict(), _one(engine, job, 0, cnt), T, n, cnt)


def _launch(engine, job, kind, g0, g1, ran):
    def run():
        try:
            T, I, st = run_engine(engine, job, kind, exec_mode=1, gid_first=g0, gid_count=g1 - g0)
            assert engine.last_passes() > 0 and engine.last_form() == 3
            ran(T, I)
            return T, st
        finally:
            engine.set_features(0, 0, 0)
            engine.set_exec(-1, 4)
    return run


def test_every_atomic_of_the_int_instance(engine, oracle_soc, tuned):
    """WINT 1 at steps_per_visit 1: TABS and INT"""
    job = Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=2, SEED=0.47, WITH_INT=1, TW=1.5)
    g0, g1 = 200000, 203000
    T, I, n, _ = _oracle(oracle_soc, "int1", job, 0, g0, g1)
    _check(engine, tuned, dict(steps_per_visit=1), _launch(engine, job, 0, g0, g1, lambda Tg, Ig: assert_tally_close(Ig, I, rtol=1e-5)),
           T, n, (g1 - g0) * job.BATCH)


def test_every_atomic_of_the_intensity_vector_instance(engine, oracle_soc, tuned):
    """WINT 2 at steps_per_visit 1: TABS, INT and the three vector sums, to the bounds of
    tests/test_gpu_ltree.py::test_intensity_vectors_in_the_sweep (signed sums: measured against INT)"""
    job = Job(cloud104(), cases._CSC, ABS=3e-5, SCA=6e-5, SOURCE=1, BATCH=2, SEED=0.377, WITH_INT=2, TW=1.7)
    g0, g1 = 100000, 103000
    T, I, n, extra = _oracle(oracle_soc, "int2", job, 0, g0, g1)
    want = extra["INTV"]
    assert np.abs(want).sum() > 0

    def ran(Tg, Ig):
        assert_tally_close(Ig, I, rtol=1e-5)
        for k in range(3):
            got = job.INTV_gpu[k]
            assert np.abs(got - want[k]).max() <= 2e-6 * np.abs(I).max()
            assert np.all(np.abs(got - want[k]) <= 1e-5 * np.maximum(I, 1e-3 * I.max()))

    _check(engine, tuned, dict(steps_per_visit=1), _launch(engine, job, 0, g0, g1, ran), T, n, (g1 - g0) * job.BATCH)


def test_every_atomic_of_the_ali_instance(engine, oracle_soc, tuned):
    """ALI at steps_per_visit 1: the read of the slot's cell number and the atomic it sends to XAB or TABS"""
    cl = cloud104()
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    job = Job(cl, cases._CSC, ABS=3e-4, SCA=6e-4, SOURCE=2, BATCH=2, SEED=0.9, GLOBAL=8192, EMIT=emit, WITH_ALI=1, TW=1.3)
    g0, g1 = 4000, 4064
    T, _, n, extra = _oracle(oracle_soc, "ali", job, 1, g0, g1)
    want = extra["XAB"]
    assert want.sum() > 0
    # (SimRAM_CL: a work item walks the cells id, id + GLOBAL, ... and sends BATCH packets from each, kernel_ASOC.c:1318-1355)
    packets = job.BATCH * sum(len(range(i, cl.CELLS, job.GLOBAL)) for i in range(g0, g1))
    _check(engine, tuned, dict(steps_per_visit=1), _launch(engine, job, 1, g0, g1, lambda Tg, Ig: assert_tally_close(job.XAB_gpu, want, rtol=1e-5)),
           T, n, packets)


def test_float_form(engine, oracle_soc, tuned):
    """the float form of the walk (float_local), on the 64^3-root hierarchy of tests/test_gpu_ltree_float.py, at steps_per_visit 1"""
    job, g0, g1 = float_bg_job("oct64_l4")
    T, _, n, _ = _oracle(oracle_soc, "flt", job, 0, g0, g1)

    def ran(Tg, Ig):
        assert engine.last_variant()["dbl"] == 0

    _check(engine, tuned, dict(float_local=1, steps_per_visit=1), _launch(engine, job, 0, g0, g1, ran), T, n, (g1 - g0) * job.BATCH)


def test_per_cell_opacities(engine, oracle_soc, tuned):
    """the abundance instance (abu_local), as tests/test_gpu_ltree_abu.py::test_background_packets, at steps_per_visit 1"""
    job = Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=1, BATCH=4, SEED=0.377, OPT=opt104())
    g0, g1 = 100000, 103000
    T, _, n, _ = _oracle(oracle_soc, "abu", job, 0, g0, g1)

    def ran(Tg, Ig):
        assert engine.last_variant()["abu"] == 1

    try:
        _check(engine, tuned, dict(abu_local=1, steps_per_visit=1), _launch(engine, job, 0, g0, g1, ran), T, n, (g1 - g0) * job.BATCH)
    finally:
        engine.set_opt(None)
