"""soc_emitted_change (soc_amd/csrc/soc_reemit.hip) -- the change of the resident emission between two re-emission iterations -- against
the restatement of converge_ref.py, its refusals and lifecycle, and soc_amd.driver with `convergence eps` on the HIP engine.

L and M are compared to the bit: the kernel's fp64 products, sums and its one division are IEEE operations (-ffp-contract=off,
-fno-fast-math; hipcc expands the fp64 division into its correctly rounded sequence), taken in the order of the restatement.  The three
sums are compared within CELLS * 2^-52 relative, the bound of any summation order of non-negative terms against the exact sum
(math.fsum); that they have ONE order is shown by running every call sequence twice and comparing the bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import converge_ref as ref                                   # noqa: E402
from soc_amd import synth                                    # noqa: E402

pytestmark = pytest.mark.gpu

NFREQ = 12                                                   # of test_driver.write_case
CHANGE_T = 256                                               # CHANGE_T: cells of a block of soc_emitted_change_kernel (soc_reemit.hip)
ERR_ARG, ERR_STATE = -1, -2
_F, _D = C.POINTER(C.c_float), C.POINTER(C.c_double)


def weights(nfreq):
    """integration weights of nfreq frequencies (one frequency has no trapezoid: any positive number)"""
    return ref.trapezoid(ref.frequencies(nfreq)) if nfreq > 1 else np.asarray([3.0e11])


class Grid:
    """what converge_ref.luminosity looks at, for a Cartesian grid"""
    def __init__(self, dims, seed):
        self.NX, self.NY, self.NZ = dims
        self.CELLS = dims[0] * dims[1] * dims[2]
        self.LEVELS, self.OFF, self.LCELLS = 1, [0], [self.CELLS]
        rng = np.random.default_rng(seed)
        self.DENS = rng.uniform(0.5, 2.0, self.CELLS).astype(np.float32)
        self.DENS[rng.choice(self.CELLS, max(1, self.CELLS // 50), replace=False)] = np.float32(1.0e-11)      # empty cells: below the 1e-10


def emissions(cloud, nfreq, seed):
    """two emissions of a model: the second a few per cent off the first, some cells switched off and some on"""
    rng = np.random.default_rng(seed)
    E1 = (10.0 ** rng.uniform(-30.0, -26.0, (cloud.CELLS, nfreq))).astype(np.float32)
    E1[rng.choice(cloud.CELLS, 3, replace=False)] = 0.0
    E2 = (E1 * rng.uniform(0.9, 1.1, E1.shape)).astype(np.float32)
    E2[rng.choice(cloud.CELLS, 3, replace=False)] = 0.0
    E2[rng.choice(cloud.CELLS, 2, replace=False)] = np.float32(1.0e-27)
    return E1, E2


def sequence(engine, cloud, nfreq, Es, W, COEFF):
    """emitted_begin, then for every emission upload + emitted_change -> [(stats, L read back)]"""
    engine.emitted_begin(nfreq)
    out = []
    assert not engine.emitted_read_luminosity(0, cloud.CELLS).any()          # zero before the first call
    for E in Es:
        engine.emitted_upload(0, E)
        st = engine.emitted_change(W, COEFF)
        out.append((st, engine.emitted_read_luminosity(0, cloud.CELLS)))
    return out


def check_parity(engine, cloud, nfreq, Es, nbad):
    W, COEFF = weights(nfreq), ref.coeff(cloud.LEVELS)
    try:
        got = sequence(engine, cloud, nfreq, Es, W, COEFF)
        again = sequence(engine, cloud, nfreq, Es, W, COEFF)                 # (emitted_begin zeroes the plane again)
    finally:
        engine.emitted_end()
    Lp = np.zeros(cloud.CELLS)
    for k, E in enumerate(Es):
        L, bad = ref.luminosity(E, W, cloud, COEFF)
        want = ref.change(L, Lp)
        st, Lgot = got[k]
        print("cells %d NFREQ %d call %d: got %r, want %r, bad %d" % (cloud.CELLS, nfreq, k, st, want, bad))
        assert bad == nbad and st["bad"] == nbad
        assert np.array_equal(ref.bits64(Lgot), ref.bits64(L)), np.flatnonzero(ref.bits64(Lgot) != ref.bits64(L))[:8]
        assert st["M"] == want["M"]
        assert ref.sums_close(st, want, cloud.CELLS)
        assert want["S_new"] > 0 and (k == 0 or 0 < want["S_abs"] < want["S_new"])
        assert again[k][0] == st and np.array_equal(ref.bits64(again[k][1]), ref.bits64(Lgot))       # one order of summation
        Lp = L
    assert got[0][0]["S_old"] == 0.0 and got[0][0]["M"] == 1.0


# 63, 64, 65 cells: a wave; 255, 256, 257: one under, at and one over a block's cells
SMALL = [(3, 3, 7), (4, 4, 4), (5, 13, 1), (5, 17, 3), (8, 8, 4), (257, 1, 1)]


@pytest.mark.parametrize("nfreq", [1, 3, 12, 50, 65])
@pytest.mark.parametrize("dims", SMALL)
def test_change_equals_the_restatement_at_the_edges_of_wave_and_block(engine, dims, nfreq):
    assert sorted(d[0] * d[1] * d[2] for d in SMALL) == [63, 64, 65, CHANGE_T - 1, CHANGE_T, CHANGE_T + 1]
    grid = Grid(dims, 100 * nfreq + dims[0])
    engine.set_grid(grid.NX, grid.NY, grid.NZ, 1, [grid.CELLS], grid.DENS)
    check_parity(engine, grid, nfreq, emissions(grid, nfreq, grid.CELLS + nfreq), 0)


@pytest.mark.parametrize("nfreq", [1, 3, 12, 50, 65])
def test_change_of_many_blocks_and_more_than_one_partial(engine, nfreq):
    grid = Grid((70, 70, 54), nfreq)                                         # 264600 cells: 1034 blocks, 5 partials per thread of the second kernel
    assert grid.CELLS > 4 * CHANGE_T * CHANGE_T
    engine.set_grid(grid.NX, grid.NY, grid.NZ, 1, [grid.CELLS], grid.DENS)
    check_parity(engine, grid, nfreq, emissions(grid, nfreq, 7 + nfreq), 0)


def test_change_on_a_hierarchy_with_dead_cells_and_specials(engine):
    nfreq = 7
    cloud, E, dead, nbad = ref.octree_with_specials(nfreq)
    rng = np.random.default_rng(21)
    E2 = (E * rng.uniform(0.9, 1.1, E.shape)).astype(np.float32)            # (NaN, inf and the negative row stay what they are)
    engine.set_cloud(cloud)
    check_parity(engine, cloud, nfreq, (E, E2), nbad)


# ---- refusals and lifecycle -------------------------------------------------------------------------------------------
def test_refused_calls_return_their_code_and_change_nothing(engine):
    from soc_amd.lib import SocError
    lib, h = engine.lib, engine.h
    grid = Grid((5, 13, 1), 3)
    engine.set_grid(grid.NX, grid.NY, grid.NZ, 1, [grid.CELLS], grid.DENS)
    nfreq = 5
    W, COEFF = weights(nfreq), ref.coeff(1)
    stats, bad, L = np.zeros(4), C.c_int64(0), np.zeros(grid.CELLS)
    pd, pf = (lambda a: a.ctypes.data_as(_D)), (lambda a: a.ctypes.data_as(_F))
    # before soc_emitted_begin
    assert lib.soc_emitted_change(h, pd(W), pf(COEFF), pd(stats), C.byref(bad)) == ERR_STATE and b"soc_emitted_begin first" in lib.soc_last_error(h)
    assert lib.soc_emitted_read_luminosity(h, 0, grid.CELLS, pd(L)) == ERR_STATE
    with pytest.raises(SocError, match="emitted_begin first"):
        engine.emitted_change(W, COEFF)
    with pytest.raises(SocError, match="emitted_begin first"):
        engine.emitted_read_luminosity(0, 1)
    E1, E2 = emissions(grid, nfreq, 5)
    engine.emitted_begin(nfreq)
    try:
        engine.emitted_upload(0, E1)
        first = engine.emitted_change(W, COEFF)
        L1 = engine.emitted_read_luminosity(0, grid.CELLS)
        engine.emitted_upload(0, E2)
        for rc in (lib.soc_emitted_change(h, None, pf(COEFF), pd(stats), C.byref(bad)), lib.soc_emitted_change(h, pd(W), None, pd(stats), C.byref(bad)),
                   lib.soc_emitted_change(h, pd(W), pf(COEFF), None, C.byref(bad)), lib.soc_emitted_change(h, pd(W), pf(COEFF), pd(stats), None),
                   lib.soc_emitted_read_luminosity(h, 0, grid.CELLS, None), lib.soc_emitted_read_luminosity(h, -1, 2, pd(L)),
                   lib.soc_emitted_read_luminosity(h, 0, 0, pd(L)), lib.soc_emitted_read_luminosity(h, 64, 2, pd(L))):
            assert rc == ERR_ARG, lib.soc_last_error(h)
        with pytest.raises(SocError, match="NFREQ = 5"):
            engine.emitted_change(W[:4], COEFF)                              # the library would read past the array
        with pytest.raises(SocError, match="NFREQ = 5"):
            engine.emitted_change(np.ones((5, 1)), COEFF)
        with pytest.raises(SocError, match="LEVELS = 1"):
            engine.emitted_change(W, np.ones(2, np.float32))
        assert not stats.any() and bad.value == 0
        assert np.array_equal(engine.emitted_download(0, grid.CELLS).view(np.uint32), E2.view(np.uint32))
        assert np.array_equal(ref.bits64(engine.emitted_read_luminosity(0, grid.CELLS)), ref.bits64(L1))
        second = engine.emitted_change(W, COEFF)
        assert second["S_old"] == first["S_new"] and 0 < second["S_abs"] < second["S_new"]
        # soc_emitted_begin zeroes the plane again
        engine.emitted_begin(nfreq)
        assert not engine.emitted_read_luminosity(0, grid.CELLS).any()
        engine.emitted_upload(0, E1)
        assert engine.emitted_change(W, COEFF) == first
        assert np.array_equal(ref.bits64(engine.emitted_read_luminosity(3, 60)), ref.bits64(L1[3:63]))
    finally:
        engine.emitted_end()


def test_the_plane_goes_with_end_with_the_model_and_with_the_handle(engine):
    from soc_amd import lib as soclib
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    engine.set_cloud(cloud)
    E1, _ = emissions(cloud, NFREQ, 5)
    W, COEFF = weights(NFREQ), ref.coeff(cloud.LEVELS)
    base = soclib.device_bytes()
    for _ in range(2):
        engine.emitted_begin(NFREQ)
        engine.emitted_upload(0, E1)
        held = soclib.device_bytes()
        assert held > base
        st = engine.emitted_change(W, COEFF)
        blocks = (cloud.CELLS + CHANGE_T - 1) // CHANGE_T
        plane = 8 * cloud.CELLS + 8 * (NFREQ + 4 + 4 * blocks) + 8           # L, the scratch (W, stats, the blocks' partials), the count of bad cells
        assert soclib.device_bytes() == held + plane
        assert engine.emitted_change(W, COEFF)["S_abs"] == 0.0 and soclib.device_bytes() == held + plane     # reserved once
        engine.emitted_end()
        assert soclib.device_bytes() == base
    engine.emitted_begin(NFREQ)
    engine.emitted_upload(0, E1)
    assert engine.emitted_change(W, COEFF) == st
    engine.set_cloud(cloud)                                                  # the plane goes with the model
    assert soclib.device_bytes() == base
    with pytest.raises(soclib.SocError, match="emitted_begin first"):
        engine.emitted_change(W, COEFF)
    other = soclib.Engine(0)                                                 # destroyed with the plane open
    other.set_cloud(cloud)
    other.emitted_begin(NFREQ)
    other.emitted_upload(0, E1)
    assert other.emitted_change(W, COEFF) == st
    assert soclib.device_bytes() > base
    other.close()
    assert soclib.device_bytes() == base


# ---- the pipeline on the HIP engine ---------------------------------------------------------------------------------
# Float atomics order the tallies differently from run to run, and the stochastic-heating solve amplifies the last digits of the
# absorptions (test_driver._emission_close: 1e-5 in, up to 2e-3 out for one pass).  The bound for two iterations is measured, not
# assumed: the chain of the EXISTING programs (AbsorptionRun.run + mabu.solve_emission per iteration) on the HIP engine against
# the same chain on the oracle engine, on the quantities of _emission_close -- the 0.98 quantile and the maximum of
# |a - b| / max(|b|, 1e-6 max|b|) over all cells that are no links.  Measured on an MI355X (3 runs of the HIP chain gave the same
# figures: at this size its tallies come out the same every time; after step 0, 1, 2 the quantile was 8.4e-11, 5.4e-11, 4.3e-11 -- 98 %
# of the values agree to the last bit or lie under the floor of the denominator -- and the maximum 3.7e-3, 3.6e-3, 3.0e-3):
CHAIN_Q98, CHAIN_MAX = 4.2538e-11, 3.0269e-3
# (copied from test_gpu_reemit.py.)  The pipeline may deviate by twice that from step 3 of the oracle chain.


def rel_deviation(a, b):
    rel = np.abs(np.asarray(a, np.float64) - b) / np.maximum(np.abs(b), 1e-6 * np.abs(b).max())
    return float(np.quantile(rel, 0.98)), float(rel.max())


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the 392-cell case of test_driver_iterations.py, three steps of the chain of the existing programs on the oracle engine, and eps
    placed half way between d_l1 of steps 2 and 3 as the restatement finds them: computed once"""
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import chain, iteration_case
    d = str(tmp_path_factory.mktemp("gpuconverge"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, ini0 = iteration_case(os.path.join(d, "oracle"), cloud, 3)
    cwd = os.getcwd()
    os.chdir(os.path.join(d, "oracle"))
    try:
        steps = chain(ini, ini0, lambda: OraclePipelineEngine("soc"), 3, cloud.CELLS, NFREQ)
    finally:
        os.chdir(cwd)
    FFREQ = np.loadtxt(os.path.join(d, "oracle", "sil.dust"), skiprows=4)[:, 0].astype(np.float32)
    W, COEFF = ref.trapezoid(FFREQ), ref.coeff(cloud.LEVELS)
    Lp, dl1 = np.zeros(cloud.CELLS), []
    for _, E in steps:
        L, bad = ref.luminosity(E, W, cloud, COEFF)
        assert bad == 0
        dl1.append(ref.d_l1(ref.change(L, Lp)))
        Lp = L
    assert dl1[0] == 1.0 and dl1[1] > dl1[2] > dl1[3] > 0
    eps = 0.5 * (dl1[2] + dl1[3])
    assert dl1[2] > 1.1 * eps and dl1[3] < 0.9 * eps                         # the gaps: over 10 %, the HIP chain differs by 3e-3
    return dict(d=d, cloud=cloud, oracle=steps, d_l1=dl1, eps=eps)


@pytest.fixture(scope="module")
def pipes(engine, case):
    """the pipeline with `iterations 5` and `convergence eps` on the HIP engine, once per emission source"""
    from reemit_chain import iteration_case
    from soc_amd import driver
    out = {}
    for source in ("resident", "host"):
        d = os.path.join(case["d"], "pipe_" + source)
        ini, _ = iteration_case(d, case["cloud"], 5, "convergence %.17g\n" % case["eps"])
        cwd = os.getcwd()
        os.chdir(d)
        try:
            P = driver.Pipeline(ini, engine, verbose=0, emission_source=None if source == "resident" else 'host')
            CTABS, FABS, EMITTED = P.run(keep_files=True)
        finally:
            os.chdir(cwd)
            engine.set_exec(-1, 4)
        out[source] = dict(P=P, FABS=FABS, EMITTED=EMITTED, d=d, emitted_after=engine._emitted)
    return out


@pytest.mark.parametrize("source", ["resident", "host"])
def test_pipeline_stops_at_the_step_of_the_criterion(engine, case, pipes, source):
    from soc_amd import files
    cloud, run = case["cloud"], pipes[source]
    P, EMITTED = run["P"], run["EMITTED"]
    conv, its = P.timers["convergence"], P.timers["iterations"]
    for c in conv:
        print("%s source, step %d: d_l1 %.6e (oracle chain %.6e)  d_total %.6e  d_max %.6e" % (source, c["k"], c["d_l1"], case["d_l1"][c["k"]], c["d_total"], c["d_max"]))
    assert P.converged == 3 and len(its) == 3 and [c["k"] for c in conv] == [0, 1, 2, 3]
    assert P.timers["emission_path"] == "device" and [it["source"] for it in its] == [source] * 3
    assert [c["source"] for c in conv] == [source] * 4 and all(c["bad"] == 0 for c in conv)
    assert conv[0]["d_l1"] == 1.0 and conv[3]["d_l1"] < case["eps"] <= conv[2]["d_l1"] < conv[1]["d_l1"]
    assert run["emitted_after"] is None                                      # closed again
    cells = cloud.DENS > 0
    assert np.isfinite(EMITTED[cells]).all() and EMITTED[cells].max() > 0
    assert np.array_equal(np.asarray(files.mmap_emitted(os.path.join(run["d"], "emitted.data"), cloud.CELLS, NFREQ)), EMITTED)
    assert np.array_equal(files.read_absorbed(os.path.join(run["d"], "abs.data")), run["FABS"])
    dat = np.loadtxt(os.path.join(run["d"], "convergence.dat"), ndmin=2)
    assert dat.shape == (4, 4) and [float(c["d_l1"]) for c in conv] == list(dat[:, 1])
    q98, worst = rel_deviation(EMITTED[cells], case["oracle"][3][1][cells])
    print("%s source against step 3 of the oracle chain: 0.98 quantile %.3e, maximum %.3e" % (source, q98, worst))
    assert q98 <= 2 * CHAIN_Q98 and worst <= 2 * CHAIN_MAX, (q98, worst)


def test_resident_and_host_figures_agree(pipes):
    a, b = pipes["resident"]["P"].timers["convergence"], pipes["host"]["P"].timers["convergence"]
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        for key in ("d_l1", "d_total", "d_max"):
            print("step %d %s: resident %.9e, host %.9e" % (x["k"], key, x[key], y[key]))
    for x, y in zip(a, b):
        for key in ("d_l1", "d_total", "d_max"):
            assert abs(x[key] - y[key]) <= 1e-6 * abs(y[key]), (x["k"], key, x[key], y[key])


class Without:
    """the HIP engine without emitted_change, or with one that finds no room for its plane: everything else is the engine's"""
    def __init__(self, engine, fits):
        self._engine, self._fits = engine, fits

    def __getattr__(self, name):
        if name == "emitted_change":
            if self._fits is None:
                raise AttributeError(name)
            return self._refuse
        return getattr(self._engine, name)

    def _refuse(self, W, COEFF):
        from soc_amd.lib import DoesNotFit
        raise DoesNotFit("emitted_change: no room (a test's stand-in)", 0)


@pytest.mark.parametrize("fits", [None, False])
def test_an_engine_that_cannot_give_the_figures_leaves_them_to_the_host_array(engine, case, pipes, fits):
    """the iterations keep the resident emission as their source, every step is read back, and the loop ends at the same step with the
    same figures as the host source gives them"""
    from reemit_chain import iteration_case
    from soc_amd import driver
    d = os.path.join(case["d"], "pipe_without_%s" % fits)
    ini, _ = iteration_case(d, case["cloud"], 5, "convergence %.17g\n" % case["eps"])
    cwd = os.getcwd()
    os.chdir(d)
    try:
        P = driver.Pipeline(ini, Without(engine, fits), verbose=0)
        CTABS, FABS, EMITTED = P.run()
    finally:
        os.chdir(cwd)
        engine.set_exec(-1, 4)
    conv, its = P.timers["convergence"], P.timers["iterations"]
    assert P.converged == 3 and [it["source"] for it in its] == ["resident"] * 3 and [c["source"] for c in conv] == ["host"] * 4
    assert engine._emitted is None
    host = pipes["host"]
    for x, y in zip(conv, host["P"].timers["convergence"]):
        assert abs(x["d_l1"] - y["d_l1"]) <= 1e-6 * y["d_l1"]
    cells = case["cloud"].DENS > 0
    q98, worst = rel_deviation(EMITTED[cells], case["oracle"][3][1][cells])
    assert q98 <= 2 * CHAIN_Q98 and worst <= 2 * CHAIN_MAX, (q98, worst)
