"""The outcome codes of the brick-local walk (soc_lbrick_walk): the step arm leaves one code per lane, the swap arm makes the queue key of
it where it stores the packet.  One case per code, each on the smallest hierarchy that takes this walk (104^3 roots, 4 levels), with the
launch deferred (batch_begin ... batch_end) so that a small launch goes through the sweep.

Every case: tally events equal to the oracle's (identical trajectories), packets equal to the launch's count, tallies or images to the
tolerance of the feature's own tests (tests/test_gpu_ltree.py, tests/test_gpu_sca_rays_healpix.py: fp32 summation order, 1e-5).  The
oracle counts tally events only, so packets and scatterings are also compared with a second witness that forms its keys in other code:
the same launch through the older sweep (`global_tree`) and through the general kernel of this one (`general_kernel`)."""
import numpy as np
import pytest

import cases
from oracle.pyoracle import Job
from test_gpu_ltree import cloud104
from util import assert_tally_close, run_engine

pytestmark = pytest.mark.gpu

_WANT = {}


def _oracle(oracle_soc, name, job, g0, g1):
    """the oracle's tallies of a case: computed once, shared by the case's tests"""
    if name not in _WANT:
        T, I, n = oracle_soc.sim(job, 0, gid0=g0, gid1=g1, nthreads=8)
        T.setflags(write=False)
        _WANT[name] = (T, None if I is None else I, n)
    return _WANT[name]


def _deferred(e, job, g0, g1, form=3):
    """one sim_pb launch of `job`, deferred into a sweep"""
    e.set_cloud(job.cloud)
    e.set_features(with_int=job.WITH_INT, ps_method=job.PS_METHOD, use_emweight=0)
    e.set_opt(None)
    e.set_mirror(0)
    e.set_scatter_table(job.DSC, job.CSC)
    e.set_optical(job.ABS, job.SCA)
    e.set_exec(1, 4)
    try:
        e.zero(0)
        e.zero(1)
        e.stats(reset=True)
        e.batch_begin(2)                                  # (room for two: the sweep starts at batch_end)
        e.sim_pb(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.BG, job.TW, PSPOS=job.PSPOS[:, :3], PS=job.PS, GLOBAL=job.GLOBAL,
                 gid_first=g0, gid_count=g1 - g0)
        e.batch_end()
        st = e.stats()
        assert e.last_passes() > 0 and e.last_form() == form
        return e.read_tally(0), e.read_tally(1), st
    finally:
        e.set_features(0, 0, 0)
        e.set_exec(-1, 4)


def _bg(**kw):
    kw.setdefault("ABS", 3e-6)
    kw.setdefault("SCA", 3e-5)
    return Job(cloud104(), cases._CSC, SOURCE=1, **kw)


def _thick():
    cl = cloud104()
    k = 6.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))      # optical depth of scattering ~ 6 across the model
    return _bg(ABS=0.1 * k, SCA=k, BATCH=2, SEED=0.52)


def _ps():
    ps = np.array([[52.3, 51.7, 50.2]], np.float32)
    return Job(cloud104(), cases._CSC, ABS=3e-6, SCA=3e-5, SOURCE=0, BATCH=1, SEED=0.2, GLOBAL=8192, PSPOS=ps, PS=[1.0], PS_METHOD=0)


# name: (job, first work item, work items, tuning, what the case is about)
CASES = {
    "leave_exit": (lambda: _bg(BATCH=1, SEED=0.377), 100000, 1 << 16, dict()),
    "scatter":    (_thick, 200000, 3000, dict()),
    "slow":       (lambda: _bg(BATCH=3, SEED=0.61), 100000, 4000, dict(slow_every=3)),
    "budget":     (lambda: _bg(BATCH=3, SEED=0.43), 300000, 4000, dict(steps_per_visit=2)),
    "tail":       (_ps, 0, 8192, dict(tail_lanes=24)),                # one brick queue of 8192 packets: chunks of >= 8 per lane
}


@pytest.mark.parametrize("name", list(CASES))
def test_outcome_against_the_oracle(name, engine, oracle_soc, tuned):
    mk, g0, cnt, tune = CASES[name]
    job = mk()
    T, _, n = _oracle(oracle_soc, name, job, g0, g0 + cnt)
    tuned(**tune)
    Tg, _, st = _deferred(engine, job, g0, g0 + cnt)
    print(name, "oracle tally events", n, "engine", st)
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert st["packets"] == cnt * job.BATCH
    if name == "scatter":
        assert st["scatterings"] > st["packets"]                      # scatterings_per_packet > 1
    assert_tally_close(Tg, T, rtol=1e-5)


@pytest.mark.parametrize("witness", ["global_tree", "general_kernel"])
@pytest.mark.parametrize("name", list(CASES))
def test_outcome_against_a_second_witness(name, witness, engine, tuned):
    mk, g0, cnt, tune = CASES[name]
    job = mk()
    tuned(**tune)
    Ta, _, sa = _deferred(engine, job, g0, g0 + cnt)
    tuned(**{witness: 1})
    Tb, _, sb = _deferred(engine, job, g0, g0 + cnt, form=2 if witness == "global_tree" else 3)
    print(name, witness, sa, sb)
    for key in ("packets", "tally_events", "scatterings"):
        assert sa[key] == sb[key], key
    assert_tally_close(Ta, Tb, rtol=1e-5)


def test_roi_entry(engine, oracle_soc, tuned):
    """the record of packets entering a region of interest, as tests/test_gpu_ltree.py::test_record_of_packets_entering_roi_in_the_sweep.
    Only the brick-local sweep keeps the record (the `global_tree` sweep refuses it), so the second witness is `general_kernel`."""
    job = _bg(BATCH=3, SEED=0.377, ROI=[40, 63, 45, 70, 38, 60], ROI_STEP=2, ROI_NSIDE=2)
    g0, g1 = 100000, 104000
    T, _, n = oracle_soc.sim(job, 0, gid0=g0, gid1=g1, nthreads=8)
    want = np.array(job.ROI_SAVE, np.float32).copy()
    try:
        stats = []
        for tune in (dict(), dict(general_kernel=1)):
            tuned(**tune)
            Tg, _, st = run_engine(engine, job, 0, exec_mode=1, gid_first=g0, gid_count=g1 - g0)
            assert engine.last_passes() > 0 and engine.last_form() == 3
            print("roi", n, st)
            assert st["tally_events"] == n and st["packets"] == 3 * (g1 - g0)
            assert_tally_close(Tg, T, rtol=1e-5)
            assert want.sum() > 0 and np.array_equal(job.ROI_SAVE_gpu != 0, want != 0)
            assert_tally_close(job.ROI_SAVE_gpu, want, rtol=1e-5)
            stats.append(st)
        assert stats[0] == stats[1]
    finally:
        engine.set_roi_save(None)
        engine.set_exec(-1, 4)


def test_ray_done_at_the_observer(engine, oracle_soc):
    """peel-off rays towards an observer inside the cloud end at the observer (ray done) or are cut there (ray limited): the scattered-light
    sweep of rays, as tests/test_gpu_sca_rays_healpix.py.  Neither tuning knob gives a second sweep of rays: `general_kernel` chooses among
    the kernels of absorption sweeps only (rays have one kernel for every kind), and with `global_tree` the hierarchy is no longer one
    the sweep of rays takes, so the launch is refused.  The second witness is the direct kernel (no sweep, no outcome codes), with the
    tolerance of test_gpu_sca_rays_healpix.py::test_direct_kernel_as_second_witness."""
    from test_gpu_sca import assert_image_close
    from test_gpu_sca_rays_healpix import _bgjob, _direct, _parity, _rays, hview
    g0, g1 = 300000, 301500
    job, view = _bgjob(BATCH=2, SEED=0.83), hview("inside")
    st = _parity(engine, oracle_soc, job, view, 0, g0, g1)
    print("rays", st)
    assert st["packets"] == 2 * (g1 - g0) and st["scatterings"] > 500
    b, sb = _rays(engine, job, view, 0, g0, g1)
    a, sa = _direct(engine, job, view, 0, g0, g1)
    print("rays", sb, "direct", sa)
    for key in ("packets", "tally_events", "scatterings"):
        assert sa[key] == sb[key] == st[key], key
    assert_image_close(b, a, rtol=2e-5)
