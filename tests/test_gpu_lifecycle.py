"""Who owns the device memory of a handle, as assertions on soc_device_bytes: everything a handle allocated goes with it, paired
calls give back what they took, buffers grow once and stay, a caller's tensor is borrowed and never freed, and a handle that
changed its grid behaves like a new one.  Every count follows from the sizes the test passes (an owned buffer of n elements is
n * sizeof(element) bytes); nothing is measured.  The memory of the brick sweeps (packet records, queues, bricks) is the handle's
too: it is counted, it goes with the handle, and two handles on one GPU do not disturb each other -- its sizes belong to the plan
of a sweep, so the tests of it assert differences and no formulas."""
import math

import numpy as np
import pytest

from soc_amd import launch, synth
from soc_amd.lib import Engine, SocError, device_bytes
from test_gpu_noncubic import cloud as noncubic, oracle, report, sources
from util import assert_tally_close, run_engine

pytestmark = pytest.mark.gpu

DSC, CSC = synth.hg_scattering_table(0.6)
PSPOS, PS = np.asarray([[2.3, 2.1, 1.7]], np.float32), [1.0]         # inside both grids
ITEMS = 256
SOURCE_BYTES = 16 + 4 + 4 + 12 + 12                                  # a point source on the device: position, luminosity, XPS_NSIDE, _SIDE, _AREA
NPIX = (16, 16)
TTT = np.linspace(3.0, 1500.0, 64).astype(np.float32)                # a stand-in for the E -> T table: only its size matters here
FREQ = np.logspace(11.5, 15.0, 5).astype(np.float32)
FABS = (1.0e-22 * (FREQ / 1.0e13) ** 1.5).astype(np.float32)


def cart8():
    return synth.cartesian_cloud(8, seed=3)


def oct4():
    """a 4 x 4 x 4 root with one refined octet: two levels, 72 cells"""
    l0 = (1.0 + np.arange(64)).astype(np.float32)
    l1 = (70.0 + np.arange(8)).astype(np.float32)
    l0[21] = -synth.I2F(0)
    return synth.Cloud(4, 4, 4, [l0, l1])


GRIDS = {"cart8": cart8, "oct4": oct4}


def view():
    _, ODIR, RA, DE = launch.set_observer_directions([math.radians(50.0)], [math.radians(35.0)])
    return ODIR, RA, DE


def setup(eng, cloud):
    eng.set_cloud(cloud)
    eng.set_features(with_int=0, ps_method=0, use_emweight=0)
    eng.set_scatter_table(DSC, CSC)
    eng.set_optical(2.0e-3, 4.0e-3)


def launch_ps(eng, seed=0.37):
    eng.sim_pb(0, 0, 1, seed, 0.0, 1.0, PSPOS=PSPOS, PS=PS, GLOBAL=ITEMS)


def centre(cloud):
    return (0.5 * cloud.NX, 0.5 * cloud.NY, 0.5 * cloud.NZ)


def make_map(eng, cloud, npix=NPIX):
    ODIR, RA, DE = view()
    return eng.map(np.full(cloud.CELLS, 1.0e-3, np.float32), ODIR[0], RA[0], DE[0], npix, 0.6, centre(cloud), 4.0e-5, 6.0e-5)


def make_polmap(eng, cloud, polstat=0):
    ODIR, RA, DE = view()
    return eng.polmap(np.full(cloud.CELLS, 1.0e-3, np.float32), ODIR[0], RA[0], DE[0], NPIX, 0.6, centre(cloud), 4.0e-5, 6.0e-5, polstat=polstat)


def solve_temperature(eng, cloud):
    return eng.solve_temperature(1.0e-3, 1.2, 1.0e-12, TTT, 1.0e20, 1.0, np.full(cloud.CELLS, 1.0e-6, np.float32))


@pytest.fixture
def eng():
    """an engine of the test's own (the session's engine lives on beside it: the counts below are differences)"""
    e = Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_create_use_everything_close(grid):
    cloud = GRIDS[grid]()
    before = device_bytes()
    e = Engine(0)
    try:
        assert device_bytes() > before                                # (the seed table and the counters)
        setup(e, cloud)
        launch_ps(e)                                                  # one direct launch
        assert e.read_tally(0).any()
        e.set_features(with_int=1, ps_method=0, use_emweight=0)
        e.set_exec(1, 4)
        e.batch_begin_int(2)                                          # two deferred launches, an INT tally each
        launch_ps(e, 0.41)
        launch_ps(e, 0.43)
        e.batch_end()
        ints = [e.batch_read_int(k) for k in range(2)]
        assert ints[0].any() and ints[1].any() and not np.array_equal(ints[0], ints[1])
        e.set_exec(-1, 4)
        e.set_features(with_int=0, ps_method=0, use_emweight=0)
        ODIR, RA, DE = view()
        e.sca_set_view(ODIR, RA, DE, NPIX, 0.6, centre(cloud))
        e.sca_sim_pb(0, 0, 1, 0.47, 0.0, PSPOS=PSPOS, PS=PS, GLOBAL=ITEMS)
        assert e.sca_read_out().size == NPIX[0] * NPIX[1]
        solve_temperature(e, cloud)
        assert e.emission(FREQ[:2], FABS[:2], 1.0e20, 1.0).shape == (cloud.CELLS, 2)
        make_map(e, cloud)
        e.set_bfield(*synth.magnetic_field(cloud, seed=5))
        assert make_polmap(e, cloud).shape == (4, NPIX[1], NPIX[0])
        e.ps_tau(PSPOS, view()[0][0], 4.0e-5, 6.0e-5)
        sol = synth.synth_solver(NFREQ=12, NE=16, NSIZE=3, seed=2)
        e.a2e_set_size(16, 12, sol["sizes"][0], synth.a2e_absorption_fraction(sol, 0))
        assert np.isfinite(e.a2e_solve(np.full((8, 12), 1.0e-3, np.float32))).all()
        e.mabu_begin(cloud.CELLS, 12, 2)
        e.mabu_end()
        assert device_bytes() > before
    finally:
        e.close()
    assert device_bytes() == before


def test_paired_calls_return_what_they_took(eng):
    cloud = oct4()
    setup(eng, cloud)
    n0 = device_bytes()
    eng.mabu_begin(1000, 12, 2)
    # absorptions, the dust's share, its emission and the sum, the abundances, the temperatures, the relative cross sections
    assert device_bytes() == n0 + 4 * 1000 * 12 * 4 + 1000 * 2 * 4 + 1000 * 4 + 12 * 2 * 8
    with pytest.raises(SocError, match="soc_mabu_end first"):
        eng.a2e_resident_begin(500, 12)                               # refused: the count stays
    assert device_bytes() == n0 + 4 * 1000 * 12 * 4 + 1000 * 2 * 4 + 1000 * 4 + 12 * 2 * 8
    eng.mabu_end()
    assert device_bytes() == n0
    eng.a2e_resident_begin(500, 12)
    assert device_bytes() == n0 + 2 * 500 * 12 * 4
    eng.a2e_resident_end()
    assert device_bytes() == n0
    B = synth.magnetic_field(cloud, seed=5)
    eng.set_bfield(*B)
    assert device_bytes() == n0 + 16 * cloud.CELLS
    eng.set_bfield(*B)                                                # again: the same buffer
    assert device_bytes() == n0 + 16 * cloud.CELLS
    make_polmap(eng, cloud)
    n1 = device_bytes()
    assert n1 == n0 + 16 * cloud.CELLS + 4 * cloud.CELLS + 4 * 4 * NPIX[0] * NPIX[1]     # the field, EMIT, four planes
    with pytest.raises(SocError, match="polstat 2"):
        make_polmap(eng, cloud, polstat=2)
    assert device_bytes() == n1
    eng.set_bfield(None)
    assert device_bytes() == n1 - 16 * cloud.CELLS


def test_growth_is_monotone_and_idempotent(eng):
    cloud = cart8()
    cells = cloud.CELLS
    setup(eng, cloud)
    n0 = device_bytes()
    make_map(eng, cloud, (16, 16))
    assert device_bytes() == n0 + 4 * cells + 2 * 4 * 16 * 16           # EMIT, the map and its optical depths
    make_map(eng, cloud, (32, 32))
    assert device_bytes() == n0 + 4 * cells + 2 * 4 * 32 * 32
    make_map(eng, cloud, (16, 16))
    assert device_bytes() == n0 + 4 * cells + 2 * 4 * 32 * 32
    n1 = device_bytes()
    solve_temperature(eng, cloud)
    n2 = n1 + 4 * cells + 4 * TTT.size + 4 * cells                      # T, the table, the absorbed energies
    assert device_bytes() == n2
    for nfreq, held in ((2, 2), (5, 5), (2, 5)):                          # the frequencies and cross sections, CELLS x nfreq values
        eng.emission(FREQ[:nfreq], FABS[:nfreq], 1.0e20, 1.0)
        assert device_bytes() == n2 - 4 * cells + 4 * 2 * held + 4 * cells * held, nfreq


def test_borrowed_tallies(eng):
    import torch
    cloud = cart8()
    cells = cloud.CELLS
    setup(eng, cloud)
    n0 = device_bytes()
    tabs = torch.zeros(cells, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    eng.bind_tally(0, tabs.data_ptr(), cells)
    assert device_bytes() == n0 - 4 * cells                              # the handle's own TABS went; the tensor does not count
    assert eng.tally_ptr(0) == tabs.data_ptr()
    launch_ps(eng)
    eng.sync()
    got = eng.read_tally(0)
    assert np.array_equal(tabs.cpu().numpy(), got) and got.any()             # the tensor is the tally
    n0 += SOURCE_BYTES                                                   # (the launch's copy of its one point source stays)
    assert device_bytes() == n0 - 4 * cells
    other = Engine(0)                                                    # close() of a handle with a bound tally leaves the tensor alone
    try:
        setup(other, cloud)
        other.bind_tally(0, tabs.data_ptr(), cells)
    finally:
        other.close()
    assert device_bytes() == n0 - 4 * cells
    assert np.array_equal(tabs.cpu().numpy(), got)
    tabs.add_(1.0)                                                       # ... and usable
    assert np.array_equal(tabs.cpu().numpy(), got + np.float32(1.0))
    eng.bind_tally(0, None)
    assert device_bytes() == n0
    eng.set_cloud(cloud)
    assert device_bytes() == n0 and eng.tally_ptr(0) not in (None, 0, tabs.data_ptr())
    eng.zero(0)
    launch_ps(eng)
    assert eng.read_tally(0).any()


def test_regrid(eng):
    old, new = cart8(), oct4()
    setup(eng, old)
    solve_temperature(eng, old)
    eng.set_bfield(*synth.magnetic_field(old, seed=5))
    launch_ps(eng)
    eng.set_cloud(new)
    with pytest.raises(SocError, match="call soc_solve_temperature or soc_set_temperature first"):
        eng.emission(FREQ[:2], FABS[:2], 1.0e20, 1.0)
    with pytest.raises(SocError, match="call soc_set_bfield first"):
        make_polmap(eng, new)
    fresh = Engine(0)
    try:
        setup(fresh, new)
        res = []
        for e in (eng, fresh):
            e.zero(0)
            e.stats(reset=True)
            # the launch's 256 work items a wavefront at a time: float atomics add in the order they arrive, and only within one
            # wavefront is that order the program's -- so the tally is the same to the bit wherever the handle's state is
            for g in range(0, ITEMS, 64):
                e.sim_pb(0, 0, 1, 0.37, 0.0, 1.0, PSPOS=PSPOS, PS=PS, GLOBAL=ITEMS, gid_first=g, gid_count=64)
            res.append((e.read_tally(0), e.stats()))
    finally:
        fresh.close()
    assert res[0][1] == res[1][1] and res[0][1]["tally_events"] > 0
    assert np.array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32))
    n0 = device_bytes()
    eng.set_exec(1, 2)                                                   # ... and sweeps the new grid: bricks of the new hierarchy, its own
    eng.zero(0)
    eng.stats(reset=True)
    launch_ps(eng)
    assert eng.last_passes() > 0 and eng.last_form() == 2 and device_bytes() > n0
    assert eng.stats()["tally_events"] == res[0][1]["tally_events"]      # the packets of the direct launches, walked again
    assert_tally_close(eng.read_tally(0), res[0][0], rtol=1e-5)         # (to fp32 summation order, the bar of the sweeps everywhere)


# ---- the memory of the brick sweeps: the smallest grid the project has for each form (tests/test_gpu_noncubic.py) ----
def sweep_scalar(eng, cloud):
    return lambda: launch_ps(eng)


def sweep_rays(eng, cloud):
    """scattered light as a sweep of rays: the parked packets and the bricks of a single-level grid"""
    ODIR, RA, DE = view()
    eng.sca_set_view(ODIR, RA, DE, NPIX, 0.6, centre(cloud))
    eng.sca_zero()
    return lambda: eng.sca_sim_pb(0, 0, 1, 0.47, 0.0, PSPOS=PSPOS, PS=PS, GLOBAL=ITEMS)


def sweep_abu_local(eng, cloud):
    """per-cell opacities on the brick-local walk: the opacities in brick-slot order"""
    rr = np.random.default_rng(11)
    eng.set_tuning(abu_local=1)
    eng.set_opt(np.stack([2.0e-3 * rr.uniform(0.5, 2, cloud.CELLS), 4.0e-3 * rr.uniform(0.5, 2, cloud.CELLS)], axis=1).astype(np.float32))
    return lambda: launch_ps(eng)


SWEEPS = {                                                             # grid, the form of the sweep, its preparation
    "cartesian": (cart8, 1, sweep_scalar),
    "global_tree": (lambda: noncubic("oct759"), 2, sweep_scalar),
    "brick_local": (lambda: noncubic("oct104x6x5"), 3, sweep_scalar),
    "rays": (cart8, 3, sweep_rays),
    "abu_local": (lambda: noncubic("oct104x6x5"), 3, sweep_abu_local),
}


@pytest.mark.parametrize("case", sorted(SWEEPS))
def test_sweep_memory_goes_with_the_handle(case):
    grid, form, prepare = SWEEPS[case]
    cloud = grid()
    before = device_bytes()
    e = Engine(0)
    try:
        setup(e, cloud)
        e.set_exec(1, 2)
        run = prepare(e, cloud)
        n0 = device_bytes()
        run()
        assert e.last_passes() > 0 and e.last_form() == form, (e.last_passes(), e.last_form())
        n1 = device_bytes()
        assert n1 > n0                                                # the sweep's buffers and bricks are counted
        run()
        assert e.last_passes() > 0 and e.last_form() == form
        assert device_bytes() == n1                                   # ... and stay as they are for the same sweep again
    finally:
        e.close()
    assert device_bytes() == before


def oracle_sweep(eng, oracle_soc, name, src, form, first):
    """A forced sweep of a source of tests/test_gpu_noncubic.py, held to the oracle as `check` there holds it: the same event count,
    tallies to fp32 summation order.  first: the whole of run_engine, soc_set_grid included; else the launch alone, on the bricks
    the handle has."""
    kind, job, g0, g1 = sources(name)[src]
    assert kind == 0
    T, I, n = oracle(oracle_soc, (name, src), job, kind, gid0=g0, gid1=g1)
    assert n > 1000 and (T > 0).sum() > 900
    if first:
        Tg, Ig, st = run_engine(eng, job, kind, gid_first=g0, gid_count=g1 - g0, exec_mode=1, brick_log2=2)
    else:
        eng.zero(0)
        eng.zero(1)
        eng.stats(reset=True)
        eng.sim_pb(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.BG, job.TW, PSPOS=job.PSPOS[:, :3], PS=job.PS,
                   XPS=(job.XPS_NSIDE, job.XPS_SIDE, job.XPS_AREA), GLOBAL=job.GLOBAL, gid_first=g0, gid_count=g1 - g0)
        eng.sync()
        Tg, Ig, st = eng.read_tally(0), eng.read_tally(1), eng.stats()
    assert eng.last_passes() > 0 and eng.last_form() == form, (eng.last_passes(), eng.last_form())
    report("%s %s form %d" % (name, src, form), Tg, T, st["tally_events"])
    assert st["tally_events"] == n, "trajectories diverged from the oracle"
    assert_tally_close(Tg, T, rtol=1e-5)
    if job.WITH_INT:
        assert_tally_close(Ig, I, rtol=1e-5)


def test_handles_on_one_gpu_do_not_disturb_each_other(oracle_soc):
    A, B = Engine(0), None
    try:
        oracle_sweep(A, oracle_soc, "oct104x6x5", "ps", 3, True)
        held = device_bytes()                                         # (B opens after this: all it ever holds is in b_held)
        B = Engine(0)
        oracle_sweep(B, oracle_soc, "oct759", "ps", 2, True)
        b_held = device_bytes() - held
        assert b_held > 0
        oracle_sweep(A, oracle_soc, "oct104x6x5", "ps", 3, False)
        assert device_bytes() == held + b_held                        # A built and grew nothing: its bricks were still its own
        B.set_cloud(oct4())                                           # (marks B's bricks stale and frees none of them: B holds what it held,
        b_held = device_bytes() - held                                #  with the arrays of the new grid in place of the old)
        oracle_sweep(A, oracle_soc, "oct104x6x5", "ps", 3, False)
        assert device_bytes() == held + b_held
        B.close()
        B = None
        assert device_bytes() == held
        oracle_sweep(A, oracle_soc, "oct104x6x5", "ps", 3, False)
        assert device_bytes() == held
    finally:
        A.close()
        if B is not None:
            B.close()
