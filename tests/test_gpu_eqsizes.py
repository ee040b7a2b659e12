"""Equilibrium grain sizes on the device (soc_a2e_set_eq_sizes + soc_a2e_resident_solve_eq, soc_a2e_eqsizes_kernel of
soc_amd/csrc/soc_a2e.hip): soc_amd.a2e.run with the cells resident against the route through a2e_eqtemp size by size and batch by batch
(the route of an engine without the call) to the bit, against the oracle engine, polarised, at the edges of NFREQ; soc_amd.mabu and
soc_amd.driver with a gsetdust file that carries an `nstoch` line, device path against host path to the bit."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import aalg_cases as ac                               # noqa: E402
from soc_amd import a2e, synth                        # noqa: E402
from test_driver import NFREQ as CASE_NFREQ           # noqa: E402

pytestmark = pytest.mark.gpu

NSIZE, NFREQ = 5, 13                                  # NFREQ odd: no multiple of anything the tile uses
ALL_CELLS = [1, 63, 65, 1000]                         # 1000: no multiple of the tile of 64 cells, 16 workgroups
SKIPPED = 3                                           # the size whose S_FRAC is planted below 1e-30


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Counting:
    """the engine, counting the calls of a2e_eqtemp (the host route of an equilibrium size)"""

    def __init__(self, engine):
        self._e, self.eqtemp = engine, 0

    def __getattr__(self, name):
        return getattr(self._e, name)

    def a2e_eqtemp(self, *a):
        self.eqtemp += 1
        return self._e.a2e_eqtemp(*a)


_solvers = {}


def solver(n):
    """synth_solver with five sizes; where size 3 is an equilibrium size with equilibrium sizes on both sides (NSTOCH 0 and 2) its
    S_FRAC is below 1e-30, so that it is skipped in the middle of them.  (With NSTOCH 4 and 999 size 3 is solved stochastically: such
    a share would make its absorption fraction AF overflow, which is no case of this feature.)"""
    planted = n <= 2
    if planted not in _solvers:
        sol = synth.synth_solver(NFREQ=NFREQ, NE=16, NSIZE=NSIZE, seed=11)
        if planted:
            sol["S_FRAC"][SKIPPED] = np.float32(1.0e-31)
        _solvers[planted] = sol
    return _solvers[planted]


def absorptions(cells, nfreq=NFREQ, seed=3):
    """log-normal absorptions; a cell without any (the look-up clamped at 0) and one 1e12 times brighter (clamped at NIP - 2)"""
    ABS = (np.random.default_rng(seed + cells).lognormal(0, 1, (cells, nfreq)) * 1e-3).astype(np.float32)
    ABS[cells // 2] = 0.0
    ABS[(2 * cells) // 3] *= np.float32(1.0e12)
    if cells == 1:
        ABS[0] = (np.random.default_rng(seed).lognormal(0, 1, nfreq) * 1e-3).astype(np.float32)
    return ABS


# ---- 1. the kernel against the existing one ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 2, 4, 999])
@pytest.mark.parametrize("cells", ALL_CELLS)
def test_resident_route_equals_the_batched_route_to_the_bit(engine, cells, n):
    sol, ABS = solver(n), absorptions(cells)
    counted = Counting(engine)
    E1, _ = a2e.run(counted, sol, ABS, NSTOCH=n, batch=128, verbose=False)
    assert counted.eqtemp == 0                                   # no equilibrium size went through the host
    batched = Counting(ac.Batches(engine))
    E2, _ = a2e.run(batched, sol, ABS, NSTOCH=n, batch=128, verbose=False)
    assert batched.eqtemp == len(a2e.eq_sizes(sol, n)) * ((cells + 127) // 128)
    assert len(a2e.eq_sizes(sol, n)) == {0: 4, 2: 2, 4: 1, 999: 0}[n]
    assert np.isfinite(E2).all() and (E2 > 0).any()
    diff = np.argwhere(bits(E1) != bits(E2))
    assert same_bits(E1, E2), (cells, n, diff[:8])
    if cells == 65:
        from oracle_engine import OracleA2E
        E3, _ = a2e.run(OracleA2E("soc"), sol, ABS, NSTOCH=n, batch=128, verbose=False)
        assert same_bits(E1, E3), (n, np.argwhere(bits(E1) != bits(E3))[:8])


def test_planted_cells_reach_both_ends_of_the_table(engine):
    """what the planted cells are for: their temperatures are the table's first and last but one interval"""
    sol, ABS = solver(0), absorptions(65)
    Emin, kE, oplgkE, TTT, KABS = a2e.eq_table(sol, 4)
    T, _ = engine.a2e_eqtemp(0, 65, a2e.NIP, a2e.FACTOR, kE, oplgkE, Emin, sol["FREQ"], KABS, TTT,
                             np.asarray(ac.clipped(ABS) * synth.a2e_absorption_fraction(sol, 4), np.float32))
    assert T[32] <= TTT[1] and T[43] >= TTT[a2e.NIP - 2] and (T[:32] > TTT[1]).all() and (T[:32] < TTT[a2e.NIP - 2]).all()


# ---- 2. polarised -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("IFREQ, n", [(-1, 2), (2, 2), (-1, 0), (2, 0)])
@pytest.mark.parametrize("cells", ALL_CELLS)
def test_polarised_sum_equals_the_batched_route_and_the_restatement(engine, cells, IFREQ, n):
    sol, ABS = solver(n), absorptions(cells)
    aalg = ac.edge_aalg(sol["SIZE_A"], cells + 7)[7:]            # through every arm of every size (one cell: between sizes 1 and 2)
    counted = Counting(engine)
    E1, P1, _ = a2e.run(counted, sol, ABS, n, IFREQ, batch=128, verbose=False, aalg=aalg)
    assert counted.eqtemp == 0
    E2, P2, _ = a2e.run(ac.Batches(engine), sol, ABS, n, IFREQ, batch=128, verbose=False, aalg=aalg)
    assert P1.shape == (cells, 1 if IFREQ >= 0 else NFREQ)
    assert same_bits(E1, E2), np.argwhere(bits(E1) != bits(E2))[:8]
    assert same_bits(P1, P2), np.argwhere(bits(P1) != bits(P2))[:8]
    want = ac.restated_pemitted(sol, aalg, ac.per_size_emissions(engine, sol, ac.clipped(ABS), n), n, IFREQ, BATCH=100)
    assert same_bits(P1, want)
    if cells > 1:
        assert (P1 > 0).any() and (P1 < E1).any() and not P1[aalg > sol["SIZE_A"][-1]].any()


def test_sizes_set_with_aalg_need_polarised_arrays(engine):
    from soc_amd.lib import SocError
    sol = solver(0)
    with pytest.raises(SocError, match="resident_begin first"):
        engine.a2e_resident_solve_eq()
    engine.a2e_resident_begin(10, NFREQ)
    try:
        engine.a2e_set_eq_sizes(*a2e.eq_size_tables(sol, [0, 1], polarised=True))
        with pytest.raises(SocError, match="polarised output was not asked for"):
            engine.a2e_resident_solve_eq()
    finally:
        engine.a2e_resident_end()
    engine.a2e_resident_begin(10, NFREQ + 1)
    try:
        with pytest.raises(SocError, match="NFREQ = %d first" % (NFREQ + 1)):
            engine.a2e_resident_solve_eq()
    finally:
        engine.a2e_resident_end()
    with pytest.raises(SocError, match="array sizes do not match"):
        engine.a2e_set_eq_sizes(*(a2e.eq_size_tables(sol, [0, 1])[:-2] + (sol["S_FRAC"][:1], None)))


# ---- 3. the edges of NFREQ --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfreq, nsize, n", [(2, 3, 0), (50, 14, 2)])
def test_nfreq_edges_equal_the_batched_route(engine, nfreq, nsize, n):
    """NFREQ = 2, the smallest a2e_resident_begin takes (Ein is one term, the emission two values per cell), and NFREQ = 50 with
    twelve equilibrium sizes behind two stochastic ones"""
    sol = synth.synth_solver(NFREQ=nfreq, NE=16, NSIZE=nsize, seed=7)
    assert len(a2e.eq_sizes(sol, n)) == nsize - n
    ABS = absorptions(333, nfreq)
    counted = Counting(engine)
    E1, _ = a2e.run(counted, sol, ABS, NSTOCH=n, verbose=False)
    E2, _ = a2e.run(ac.Batches(engine), sol, ABS, NSTOCH=n, verbose=False)
    # (at NFREQ = 2 the brightest cell's emission at the lowest frequency is x / (exp(tiny) - 1) = +inf on both routes: no NaN, though)
    assert counted.eqtemp == 0 and not np.isnan(E2).any() and np.isfinite(E2[:100]).all() and (E2 > 0).any()
    assert same_bits(E1, E2), np.argwhere(bits(E1) != bits(E2))[:8]


# ---- 4. and 5. mabu and driver ----------------------------------------------------------------------------------------
def four_sizes(d, nstoch=2):
    """the case of test_driver.write_case (or reemit_chain.iteration_case) in d, its stochastically heated dust with four sizes: the
    solver file, the simple dust of the transfer run, the gsetdust file with an `nstoch` line, and in plain/ the same dust without
    the line"""
    sol = synth.synth_solver(NFREQ=CASE_NFREQ, NE=16, NSIZE=4, seed=5)
    synth.write_solver(os.path.join(d, "pah.solver"), sol)
    with open(os.path.join(d, "gs_pah.dust"), "w") as fp:
        fp.write("gsetdust\nnstoch %d\n" % nstoch)
    os.makedirs(os.path.join(d, "plain"), exist_ok=True)            # the same dust without the line
    synth.write_solver(os.path.join(d, "plain", "pah.solver"), sol)
    with open(os.path.join(d, "plain", "gs_pah.dust"), "w") as fp:
        fp.write("gsetdust\n")
    kabs = np.sum(np.asarray(sol["SK_ABS"], np.float64), axis=0)
    with open(os.path.join(d, "pah_simple.dust"), "w") as fp:
        fp.write("eqdust\n 1.0e-7\n 1.0e-4\n%d\n" % CASE_NFREQ)
        for f, k in zip(np.asarray(sol["FREQ"], np.float64), kabs):
            fp.write(" %.5e  0.3  %.5e  %.5e\n" % (f, k / (1.0e-7 * np.pi * 1.0e-8), 2.0 * k / (1.0e-7 * np.pi * 1.0e-8)))
    return sol


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """an equilibrium dust and a stochastically heated one with `nstoch 2` of four sizes; absorptions with parent-cell rows and rows
    of zeros, abundances, aalg arrays for both dusts (tests/aalg_cases.py)"""
    from test_driver import write_case
    d = str(tmp_path_factory.mktemp("gpueqsizes"))
    cells = 777
    write_case(d, synth.cartesian_cloud(3, seed=2))
    sol = four_sizes(d)
    rng = np.random.default_rng(31)
    FABS = (rng.uniform(0.0, 1.0, (cells, CASE_NFREQ)) * 10.0 ** rng.uniform(-9, -5, (cells, 1))).astype(np.float32)
    FABS[rng.uniform(size=cells) < 0.1] = np.float32(-1.0e20)
    FABS[3:cells:97] = 0.0
    ABU = rng.uniform(0.2, 1.5, (cells, 2)).astype(np.float32)
    apol = ac.synthetic_rpol(os.path.join(d, "sil.rpol"), sol["FREQ"], 2.0e-7, 6.0e-5)
    a_eq = (10.0 ** rng.uniform(np.log10(apol[0]) - 0.3, np.log10(apol[-1]) + 0.3, cells)).astype(np.float32)
    a_st = ac.edge_aalg(sol["SIZE_A"], cells)[rng.permutation(cells)]
    pol = [ac.write_aalg(os.path.join(d, "sil.aalg"), a_eq), ac.write_aalg(os.path.join(d, "pah.aalg"), a_st)]
    return dict(d=d, dusts=[os.path.join(d, "sil.dust"), os.path.join(d, "gs_pah.dust")], FABS=FABS, ABU=ABU, pol=pol, cells=cells,
                plain=os.path.join(d, "plain", "gs_pah.dust"))


@pytest.mark.parametrize("range_cells", [None, 400])
@pytest.mark.parametrize("polarised", [False, True])
def test_mabu_takes_the_device_path_and_gives_the_bits_of_the_host_path(engine, model, polarised, range_cells):
    from soc_amd import mabu
    dusts, FABS, ABU = model["dusts"], model["FABS"], model["ABU"]
    kinds = [mabu.dust_kind(x) for x in dusts]
    assert kinds == ['eqdust', 'gsetdust'] and mabu.read_nstoch(dusts[1]) == 2
    pol = model["pol"] if polarised else None
    counted = Counting(engine)
    with np.errstate(all='ignore'):
        dev, di = mabu.solve_emission(counted, dusts, kinds, FABS, ABU, pol=pol, range_cells=range_cells)
        assert (di["path"], di["ranges"], counted.eqtemp) == ("device", 1 if range_cells is None else 2, 0)
        host, hi = mabu.solve_emission(counted, dusts, kinds, FABS, ABU, pol=pol, path='host')
        # ... and the host path of an engine without the resident calls: every equilibrium size through a2e_eqtemp
        old, oi = mabu.solve_emission(Counting(ac.Batches(engine)), dusts, kinds, FABS, ABU, pol=pol, path='host')
    assert hi["path"] == oi["path"] == "host" and counted.eqtemp == 0
    live = FABS[:, 0] >= 0
    assert np.isfinite(old[live]).all() and (old[live] > 0).any()
    for name, ref, ri in (("host path", host, hi), ("batched host path", old, oi)):
        assert np.array_equal(bits(dev), bits(ref)), (name, np.argwhere(bits(dev) != bits(ref))[:8])
        if polarised:
            assert (ri["R"][live] > 0).any()
            assert np.array_equal(bits(di["R"]), bits(ri["R"])), (name, np.argwhere(bits(di["R"]) != bits(ri["R"]))[:8])
    if not polarised and range_cells is None:              # the line is honoured: without it (every size stochastic) other bits
        plain, pi = mabu.solve_emission(engine, [dusts[0], model["plain"]], kinds, FABS, ABU)
        assert pi["path"] == "device" and not np.array_equal(bits(plain[live]), bits(dev[live]))


INT = 1                                                      # SOC_TALLY_INT


class RecordingTallies:
    """The engine for the run with the resident sources.  Float atomics order the additions of a launch differently from run to run,
    so two runs of one pipeline do not tally the same bits on the GPU (measured with this model: 1504 of 4704 absorptions, 527 of 4704
    emission values and 97 of 770 map values differ between two identical runs, as many as between the two sources).  To compare the
    two sources bit for bit both must be handed the same tallies: this engine keeps, in order, every INT tally that the transfer
    stage adds to the resident absorptions -- read from the same device buffer just before the add, as MirrorEngine of
    tests/test_gpu_absorbed.py does."""

    def __init__(self, engine):
        self._e, self.tallies = engine, []

    def __getattr__(self, name):
        return getattr(self._e, name)

    def absorbed_add_tally(self, col):
        self.tallies.append(np.array(self._e.read_tally(INT), np.float32))
        self._e.absorbed_add_tally(col)

    def absorbed_add_slot(self, col, slot):
        self.tallies.append(np.array(self._e.batch_read_int(slot), np.float32))
        self._e.absorbed_add_slot(col, slot)


class ReplayingTallies:
    """The engine for the run with the host statements: every launch runs as always, but where the transfer stage reads an INT tally
    for FABSORBED[:, col] += tally (read_tally(INT), batch_read_int: the statements the resident adds stand for, in the same order)
    it is given the tally that the recorded run added at that point."""

    def __init__(self, engine, tallies):
        self._e, self.tallies, self.used = engine, tallies, 0

    def __getattr__(self, name):
        return getattr(self._e, name)

    def _next(self, own):
        assert self.used < len(self.tallies), "the host statements read more INT tallies than the resident run added"
        rec = self.tallies[self.used]
        self.used += 1
        assert rec.shape == own.shape
        return rec.copy()

    def read_tally(self, which=0):
        own = self._e.read_tally(which)
        return self._next(own) if which == INT else own

    def batch_read_int(self, k):
        return self._next(self._e.batch_read_int(k))


@pytest.fixture(scope="module")
def pipelines(engine, tmp_path_factory):
    """the iterating model of tests/test_gpu_reemit.py (reemit_chain.iteration_case: 392 cells, 12 frequencies, `iterations 2`,
    `cellpackets`) with `emweight 0` and the `nstoch 2` dust, run once with the resident sources and once with the host statements
    on the same INT tallies (RecordingTallies, ReplayingTallies)"""
    from reemit_chain import iteration_case
    from soc_amd import driver
    top = str(tmp_path_factory.mktemp("gpueqdriver"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    out = dict(cloud=cloud)
    recorder = RecordingTallies(engine)
    replayer = ReplayingTallies(engine, recorder.tallies)
    for tag, eng, kw in (("resident", recorder, {}), ("host", replayer, dict(emission_source='host', absorbed_source='host'))):
        d = os.path.join(top, tag)
        ini, _ = iteration_case(d, cloud, 2, extra="emweight 0\n")
        four_sizes(d)
        cwd = os.getcwd()
        os.chdir(d)
        try:
            P = driver.Pipeline(ini, eng, verbose=0, **kw)
            with np.errstate(all='ignore'):
                CTABS, FABS, EMITTED = P.run(keep_files=True)
        finally:
            os.chdir(cwd)
            engine.set_exec(-1, 4)
        out[tag] = dict(d=d, timers=dict(P.timers), FABS=FABS, EMITTED=EMITTED, open=(engine._absorbed, engine._emitted),
                        maps=np.fromfile(os.path.join(d, "map_dir_00.bin"), np.float32))
    out["tallies"] = (len(recorder.tallies), replayer.used)
    return out


def test_driver_keeps_the_chain_resident_with_an_nstoch_dust(engine, pipelines):
    """stage 2 on the device, emission and absorptions resident in both iterations -- and the emission is what the host path of
    stage 2 makes of the pipeline's own last absorptions with `nstoch 2`, to the bit (stage 2 has no atomics: this part of the
    comparison with the host statements does not depend on the order of the tallies)"""
    from soc_amd import mabu
    cloud = pipelines["cloud"]
    for tag in ("resident", "host"):
        r = pipelines[tag]
        its = r["timers"]["iterations"]
        assert r["timers"]["emission_path"] == "device" and len(its) == 2
        assert r["timers"]["absorbed_source"] == tag and [it["absorbed"] for it in its] == [tag, tag]
        assert [it["source"] for it in its] == [tag, tag]
        assert r["open"] == (None, None)                                         # closed again
    r = pipelines["resident"]
    leaf = cloud.DENS > 0
    assert np.isfinite(r["EMITTED"][leaf]).all() and (r["EMITTED"][leaf] > 0).any() and r["maps"][2:].max() > 0
    dusts = [os.path.join(r["d"], "sil.dust"), os.path.join(r["d"], "gs_pah.dust")]
    kinds = [mabu.dust_kind(x) for x in dusts]
    assert mabu.read_nstoch(dusts[1]) == 2
    ABU = np.stack([np.fromfile(os.path.join(r["d"], "sil.abu"), np.float32), np.ones(cloud.CELLS, np.float32)], axis=1)
    with np.errstate(all='ignore'):
        want, info = mabu.solve_emission(Counting(ac.Batches(engine)), dusts, kinds, r["FABS"], ABU, path='host')
        every, _ = mabu.solve_emission(engine, dusts[:1] + [os.path.join(r["d"], "plain", "gs_pah.dust")], kinds, r["FABS"], ABU)
    assert info["path"] == "host"
    assert np.array_equal(bits(r["EMITTED"]), bits(want)), np.argwhere(bits(r["EMITTED"]) != bits(want))[:8]
    assert not np.array_equal(bits(r["EMITTED"][leaf]), bits(every[leaf]))       # (with every size stochastic: another emission)


def test_driver_resident_chain_equals_the_host_statements_to_the_bit(pipelines):
    """The emitted array and the maps of the resident chain against Pipeline(..., emission_source='host', absorbed_source='host'),
    bit for bit, both on the same INT tallies (see RecordingTallies: two runs of the SAME pipeline do not tally the same bits on the
    GPU, whichever the sources; left to their own tallies the two differed in 483 to 546 of the 4704 emission values and 84 to 108
    of the 770 map values, as two identical runs do).  Everything behind the tallies -- the constant sources' share kept and
    restored, the scaled hand-over to stage 2, stage 2 with the equilibrium sizes, the emission's way back into the cell-emission
    launches of the next iteration, the maps -- must then give the same bits."""
    res, host = pipelines["resident"], pipelines["host"]
    added, read = pipelines["tallies"]
    assert added == read and added > 2 * 12                     # every tally added was read: 12 frequencies in 2 iterations, and the constant sources
    assert np.array_equal(bits(res["FABS"]), bits(host["FABS"])), np.argwhere(bits(res["FABS"]) != bits(host["FABS"]))[:8]
    for name in ("EMITTED", "maps"):
        a, b = res[name], host[name]
        n = int((bits(a) != bits(b)).sum())
        ok = np.isfinite(a) & np.isfinite(b)                    # (the rows of the links are not: their absorptions are -1e20)
        rel = np.abs(a[ok].astype(np.float64) - b[ok]) / np.maximum(np.abs(b[ok]), 1e-6 * np.abs(b[ok]).max())
        print("%s: %d of %d values differ in their bits, largest relative difference %.3e" % (name, n, a.size, float(rel.max())))
    assert np.array_equal(bits(res["EMITTED"]), bits(host["EMITTED"])), np.argwhere(bits(res["EMITTED"]) != bits(host["EMITTED"]))[:8]
    assert np.array_equal(bits(res["maps"]), bits(host["maps"]))
