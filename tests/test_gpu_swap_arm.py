"""The swap arm of the brick-local walk (soc_lbrick_walk): a lane stores its packet with the queue it goes to next, takes up the prefetched
one and asks for the record after it, which lands in the registers that carry it to the next entry of the arm.  Every case is the smallest
shape at which that exchange can go wrong, on the smallest hierarchy that takes this walk (104^3 roots, 4 levels), with the launches
deferred (batch_begin ... batch_end) as in tests/test_gpu_walk_outcomes.py.

Every case: tally events equal to the oracle's (identical trajectories), packets equal to the launches' count, tallies to the 1e-5 of the
existing walk tests (fp32 summation order), and packets, tally events and scatterings equal to those of the `general_kernel` witness."""
import numpy as np
import pytest

import cases
from oracle.pyoracle import Job
from test_gpu_ltree import cloud104
from test_gpu_walk_outcomes import _bg, _deferred, _ps, _thick
from util import assert_tally_close

pytestmark = pytest.mark.gpu

_WANT = {}


def _oracle(oracle_soc, name, job, kind, g0, g1):
    """the oracle's tallies of a launch: computed once, shared by the tests that run it, never written to"""
    if name not in _WANT:
        T, _, n = oracle_soc.sim(job, kind, gid0=g0, gid1=g1, nthreads=8)
        T.setflags(write=False)
        _WANT[name] = (T, n)
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


# 4000 background work items with BATCH 3: one oracle run serves the three shapes of the sweep
_BG = (lambda: _bg(BATCH=3, SEED=0.29), 400000, 4000)


@pytest.mark.parametrize("tune", [dict(steps_per_visit=1), dict(swap_lanes=1), dict(swap_lanes=64)], ids=lambda t: "%s%d" % next(iter(t.items())))
def test_every_field_round_trips(tune, engine, oracle_soc, tuned):
    """steps_per_visit 1: every step is followed by a store and a take-up, so every field of the record goes through memory every step.
    swap_lanes 1 and 64: the arm entered for a single lane, and only when all lanes wait for it or nobody can step."""
    mk, g0, cnt = _BG
    job = mk()
    T, n = _oracle(oracle_soc, "bg", job, 0, g0, g0 + cnt)
    _check(engine, tuned, tune, _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)


@pytest.mark.parametrize("cnt", [1, 63, 65, 511, 513])
def test_one_queue_of_few_packets(cnt, engine, oracle_soc, tuned):
    """a point source sends all its packets into one brick queue: lanes that never hold a packet, the two turns of a lane that only
    reserve, a chunk that ends inside a wave (1, 63, 65) and inside a workgroup (511, 513)"""
    job = _ps()
    T, n = _oracle(oracle_soc, "ps%d" % cnt, job, 0, 0, cnt)
    _check(engine, tuned, dict(), _one(engine, job, 0, cnt), T, n, cnt)


def test_two_launches_with_their_own_constants(engine, oracle_soc, tuned):
    """a point-source and a SimRAM_CL launch in one sweep, with different ABS, SCA and TW: the take-up reads the constants and the
    no-nudge flag of the packet's launch.  Against the sum of the oracle's two runs."""
    cl = cloud104()
    ps = np.array([[52.3, 51.7, 50.2]], np.float32)
    emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
    launches = [(0, Job(cl, cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=0, BATCH=20, SEED=0.2, GLOBAL=512, PSPOS=ps, PS=[1.0], PS_METHOD=0, TW=1.0), 0, 512),
                (1, Job(cl, cases._CSC, ABS=5e-6, SCA=2e-5, SOURCE=2, BATCH=1, SEED=0.7, GLOBAL=8192, EMIT=emit, TW=1.5), 4000, 4096)]
    want, n, packets = np.zeros(cl.CELLS, np.float64), 0, 0
    for k, (kind, job, g0, g1) in enumerate(launches):
        T, m = _oracle(oracle_soc, "two%d" % k, job, kind, g0, g1)
        want += T
        n += m
        # (SimRAM_CL: a work item walks the cells id, id + GLOBAL, ... and sends BATCH packets from each, kernel_ASOC.c:1318-1355)
        packets += job.BATCH * ((g1 - g0) if kind == 0 else sum(len(range(i, cl.CELLS, job.GLOBAL)) for i in range(g0, g1)))

    def run():
        e = engine
        e.set_cloud(cl)
        e.set_features(with_int=0, ps_method=0, use_emweight=0)
        e.set_opt(None)
        e.set_mirror(0)
        e.set_exec(1, 4)
        try:
            e.zero(0)
            e.stats(reset=True)
            e.batch_begin(2)
            for kind, job, g0, g1 in launches:
                e.set_optical(job.ABS, job.SCA)
                e.set_scatter_table(job.DSC, job.CSC)
                if kind == 0:
                    e.sim_pb(0, job.PACKETS, job.BATCH, job.SEED, job.BG, job.TW, PSPOS=job.PSPOS[:, :3], PS=job.PS, GLOBAL=job.GLOBAL,
                             gid_first=g0, gid_count=g1 - g0)
                else:
                    e.set_emission(job.EMIT, None)
                    e.sim_cl(2, job.PACKETS, job.BATCH, job.SEED, job.TW, job.GLOBAL, gid_first=g0, gid_count=g1 - g0)
            e.batch_end()
            st = e.stats()
            assert e.last_passes() > 0 and e.last_form() == 3
            return e.read_tally(0), st
        finally:
            e.set_features(0, 0, 0)
            e.set_exec(-1, 4)

    _check(engine, tuned, dict(), run, want, n, packets)


def test_arrivals_and_event_keys_in_a_thick_cloud(engine, oracle_soc, tuned):
    """more than one scattering per packet and two steps per visit: the ARRIVE bit and the keys of the event queues are formed in the arm"""
    job = _thick()
    g0, cnt = 200000, 3000
    T, n = _oracle(oracle_soc, "thick", job, 0, g0, g0 + cnt)
    st = _check(engine, tuned, dict(steps_per_visit=2), _one(engine, job, g0, cnt), T, n, cnt * job.BATCH)
    assert st["scatterings"] > st["packets"]
