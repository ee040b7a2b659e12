"""The absorptions of the transfer stage resident on the device (soc_absorbed_*: soc_amd/csrc/soc_capi_absorbed.hip, kernels in
soc_reemit.hip) and the pipeline that keeps them there: the per-frequency add to the bit at every row alignment, the scaled rows
against files.scale_absorbed to the bit, the device-to-device hand-over to the multi-dust stage, keep / restore, the plumbing of
AbsorptionRun in its three INT policies, refusals, lifecycle, and soc_amd.driver with either source."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import files, synth                              # noqa: E402

pytestmark = pytest.mark.gpu

NFREQ = 12                                                   # of test_driver.write_case
ERR_ARG, ERR_STATE = -1, -2
_F = C.POINTER(C.c_float)
INT = 1                                                      # SOC_TALLY_INT


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def values(n, seed, sign=False):
    """n floats for arithmetic: finite values of wide range, +infinity, denormals and both zeros; no NaN and, with sign=False, nothing
    negative but -0 (so that no sum is inf - inf: a NaN's sign differs between the host and the device)"""
    rng = np.random.default_rng(seed)
    v = (10.0 ** rng.uniform(-44.0, 38.0, n)).astype(np.float32)
    if sign:
        v *= rng.choice(np.array([-1.0, 1.0], np.float32), n)
    special = np.array([np.inf, 1.0e-45, 3.0e-39, 0.0, -0.0, 3.4e38, 1.0, 1.1754944e-38], np.float32)
    where = rng.choice(n, min(n, special.size), replace=False)
    v[where] = special[:where.size]
    return v


def cartesian(engine, NX, NY, NZ):
    cells = NX * NY * NZ
    engine.set_grid(NX, NY, NZ, 1, [cells], np.ones(cells, np.float32))
    return cells


# ---- 1. the add -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfreq", [1, 3])
@pytest.mark.parametrize("dims", [(3, 3, 7), (4, 4, 4), (5, 13, 1), (2, 3, 11),      # 63, 64, 65, 66 cells: rows at every alignment mod 4
                                  (70, 70, 54)])                                     # 264600 cells: more than one staged piece (2^18)
def test_add_equals_the_host_sum_to_the_bit(engine, dims, nfreq):
    cells = cartesian(engine, *dims)
    engine.absorbed_begin(nfreq)
    try:
        assert not bits(engine.absorbed_download(0, cells)).any()                    # zeroed
        want = np.zeros((cells, nfreq), np.float32)
        for col in range(min(1, nfreq - 1), nfreq):
            T1, T2 = values(cells, 100 * cells + col), values(cells, 100 * cells + col + 50)
            engine.write_tally(INT, T1)
            engine.absorbed_add_tally(col)
            assert np.array_equal(bits(engine.read_tally(INT)), bits(T1))            # the tally is left as it is
            engine.write_tally(INT, T2)
            engine.absorbed_add_tally(col)
            assert np.array_equal(bits(engine.read_tally(INT)), bits(T2))
            with np.errstate(over='ignore'):
                want[:, col] = (np.zeros(cells, np.float32) + T1) + T2
        got = engine.absorbed_download(0, cells)
        assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))[:8]
        if nfreq > 1:
            assert not bits(got[:, 0]).any()                                         # every other column is still zero
    finally:
        engine.absorbed_end()


# ---- 2. the scaled rows -----------------------------------------------------------------------------------------------
def fill(engine, A):
    """A[cells, nfreq] into the zeroed resident array, column by column through the INT tally (0 + a = a, but -0: those become +0)"""
    for f in range(A.shape[1]):
        engine.write_tally(INT, A[:, f])
        engine.absorbed_add_tally(f)


@pytest.fixture(scope="module")
def octree3():
    cloud = synth.octree_cloud(6, levels=3, frac=0.15, seed=4)
    assert cloud.LEVELS == 3 and all(int(n) > 0 for n in cloud.LCELLS)
    leaves = np.flatnonzero(cloud.DENS > 0)
    cloud.thin_cell = int(leaves[len(leaves) // 2])
    cloud.DENS[cloud.thin_cell] = np.float32(1.0e-11)                                # live with nnnlimit 0, empty with 1e-10
    assert (cloud.DENS <= 0).sum() > 8                                               # links
    return cloud


# grid lengths that give the physical factors K (8^level FACTOR / (GL PARSEC) ~ 1e3), factors of ~1e36 that overflow the products, and
# factors of ~1e-39 that are denormal themselves and make denormal products (no factor / density underflows to 0: inf x 0 would be a NaN)
GRID_LENGTHS = [0.05, 3.0e-35, 1.0e40]


@pytest.mark.parametrize("nfreq", [1, 3, 12, 50, 65])
def test_scaled_rows_equal_scale_absorbed_to_the_bit(engine, octree3, nfreq):
    cloud = octree3
    CELLS = cloud.CELLS
    engine.set_cloud(cloud)
    engine.absorbed_begin(nfreq)
    try:
        A = values(CELLS * nfreq, 7 + nfreq, sign=True).reshape(CELLS, nfreq)
        A[cloud.thin_cell] = np.float32(-2.5)                    # (its factor overflows to inf with the second grid length: no 0 x inf)
        fill(engine, A)
        raw = engine.absorbed_download(0, CELLS)
        assert np.array_equal(bits(raw), bits(np.zeros_like(A) + A))                 # K None: what was accumulated
        levels = np.searchsorted(np.asarray(cloud.OFF[:3]), np.arange(CELLS), side='right') - 1
        for GL in GRID_LENGTHS:
            K = files.absorbed_scale_factors(cloud, GL)
            assert K.dtype == np.float32 and K.shape == (3,)
            for nnnlimit in (0.0, 1.0e-10):
                want = files.scale_absorbed(raw.copy(), cloud, GL, nnnlimit)
                live = ~(cloud.DENS <= np.float32(nnnlimit))
                assert set(levels[live]) == {0, 1, 2}                                # a live cell of every level was present
                assert (want[~live] == np.float32(-1.0e20)).all() and not np.isnan(want).any()
                for c0, n in [(0, CELLS), (1, 62), (63, 2)]:                         # chunks that start and end off the 64-cell tile
                    got = engine.absorbed_download(c0, n, K, nnnlimit)
                    assert np.array_equal(bits(got), bits(want[c0:c0 + n])), (GL, nnnlimit, c0, np.argwhere(bits(got) != bits(want[c0:c0 + n]))[:8])
        K = files.absorbed_scale_factors(cloud, GRID_LENGTHS[1])
        with np.errstate(over='ignore'):
            assert np.isinf(files.scale_absorbed(raw.copy(), cloud, GRID_LENGTHS[1])[np.isfinite(raw)]).any()       # products overflowed
        tiny = np.abs(files.scale_absorbed(raw.copy(), cloud, GRID_LENGTHS[2]))
        assert ((tiny > 0) & (tiny < np.float32(1.1754944e-38))).any() and (K > 0).all()                                # denormal products
        assert np.array_equal(bits(engine.absorbed_download(0, CELLS)), bits(raw))   # a scaled read leaves the array as it was
    finally:
        engine.absorbed_end()


# ---- 3. the hand-over to the multi-dust stage -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the dust files and the ini of test_driver.write_case with `iterations 2` and `cellpackets` (392 cells, 12 frequencies), and the
    chain of the existing programs on the oracle engine: the reference of the pipeline tests, computed once"""
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import chain, iteration_case
    d = str(tmp_path_factory.mktemp("gpuabsorbed"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, ini0 = iteration_case(os.path.join(d, "oracle"), cloud, 2)
    cwd = os.getcwd()
    os.chdir(os.path.join(d, "oracle"))
    try:
        steps = chain(ini, ini0, lambda: OraclePipelineEngine("soc"), 2, cloud.CELLS, NFREQ)
    finally:
        os.chdir(cwd)
    return dict(d=d, cloud=cloud, oracle=steps, ini=ini, ini0=ini0)


def test_to_mabu_hands_over_the_bits_of_the_host_array(engine, case):
    """the multi-dust stage in ranges of 37 cells (11 ranges, the last of 22), once from the resident absorptions and once from the
    host array of the same scaled bits"""
    from soc_amd import mabu
    cloud, d = case["cloud"], os.path.join(case["d"], "oracle")
    dusts = [os.path.join(d, "sil.dust"), os.path.join(d, "gs_pah.dust")]
    kinds = [mabu.dust_kind(x) for x in dusts]
    ABU = np.stack([np.fromfile(os.path.join(d, "sil.abu"), np.float32), np.ones(cloud.CELLS, np.float32)], axis=1)
    GL, nnnlimit = 0.05, 0.0
    scaled = case["oracle"][0][0]                                # absorptions of the right size for these dusts, as the file holds them
    K = files.absorbed_scale_factors(cloud, GL)
    live = cloud.DENS > 0
    levels = np.searchsorted(np.asarray(cloud.OFF[:cloud.LEVELS]), np.arange(cloud.CELLS), side='right') - 1
    raw = np.zeros_like(scaled)
    raw[live] = scaled[live] / (K[levels[live]] / cloud.DENS[live])[:, None]         # any unscaled values of that size will do
    from soc_amd.asoc import ResidentAbsorptions
    engine.set_cloud(cloud)
    engine.absorbed_begin(NFREQ)
    try:
        fill(engine, raw)
        host = engine.absorbed_download(0, cloud.CELLS, K, nnnlimit)
        assert np.array_equal(bits(host), bits(files.scale_absorbed(engine.absorbed_download(0, cloud.CELLS), cloud, GL, nnnlimit)))
        sink = ResidentAbsorptions(engine, cloud.CELLS, NFREQ)
        EM, info = mabu.solve_emission(engine, dusts, kinds, sink, ABU, range_cells=37, absorbed_scale=(K, nnnlimit))
        assert (info["path"], info["ranges"]) == ("device", 11)
        EMH, infoh = mabu.solve_emission(engine, dusts, kinds, host, ABU, range_cells=37)
        assert (infoh["path"], infoh["ranges"]) == ("device", 11)
        assert (EM[live] > 0).any()
        assert np.array_equal(bits(EM), bits(EMH))
        with pytest.raises(ValueError, match="absorbed_scale"):
            mabu.solve_emission(engine, dusts, kinds, sink, ABU)
        with pytest.raises(ValueError, match="device path"):
            mabu.solve_emission(engine, dusts, kinds, sink, ABU, path='host', absorbed_scale=(K, nnnlimit))
    finally:
        engine.absorbed_end()


# ---- 4. keep and restore ----------------------------------------------------------------------------------------------
def payload(n, nfreq, seed):
    """arbitrary bit patterns, NaNs with payloads among them: for what is only copied"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 32, (n, nfreq), dtype=np.uint64).astype(np.uint32).view(np.float32)


def test_keep_and_restore(engine):
    lib, h = engine.lib, engine.h
    cells = cartesian(engine, 5, 13, 1)
    engine.absorbed_begin(3)                                                         # no second plane
    try:
        assert lib.soc_absorbed_keep(h) == ERR_STATE and b"second plane" in lib.soc_last_error(h)
        assert lib.soc_absorbed_restore(h) == ERR_STATE
    finally:
        engine.absorbed_end()
    engine.absorbed_begin(3, keep_constant=True)
    try:
        assert lib.soc_absorbed_restore(h) == ERR_STATE and b"soc_absorbed_keep first" in lib.soc_last_error(h)
        # the array holds arbitrary bits: accumulated as 0 + a, which keeps every pattern but -0 and the quiet bit of a NaN; so compare
        # with what the array really holds
        fill(engine, payload(cells, 3, 5))
        constant = engine.absorbed_download(0, cells)
        engine.absorbed_keep()
        assert np.array_equal(bits(engine.absorbed_download(0, cells)), bits(constant))
        T = values(cells, 11)
        engine.write_tally(INT, T)
        engine.absorbed_add_tally(1)
        summed = engine.absorbed_download(0, cells)
        assert not np.array_equal(bits(summed), bits(constant))
        assert np.array_equal(bits(summed[:, 0::2]), bits(constant[:, 0::2]))
        engine.absorbed_restore()
        assert np.array_equal(bits(engine.absorbed_download(0, cells)), bits(constant))
        engine.absorbed_add_tally(2)                                                 # adds after a restore leave the kept plane alone
        engine.absorbed_restore()
        assert np.array_equal(bits(engine.absorbed_download(0, cells)), bits(constant))
    finally:
        engine.absorbed_end()


# ---- 5. the plumbing of AbsorptionRun ---------------------------------------------------------------------------------
class MirrorEngine:
    """the engine, with absorbed_add_tally / absorbed_add_slot that also read the same buffer to the host and apply the host statement
    FABSORBED[:, col] += tally to self.host"""

    def __init__(self, engine):
        self._e = engine
        self.host = None
        self.calls = []
        self.largest = 0.0

    def __getattr__(self, name):
        return getattr(self._e, name)

    def absorbed_add_tally(self, col):
        tally = self._e.read_tally(INT)
        self.largest = max(self.largest, float(tally.max()))
        self.host[:, col] += tally
        self.calls.append("tally")
        self._e.absorbed_add_tally(col)

    def absorbed_add_slot(self, col, slot):
        self.host[:, col] += self._e.batch_read_int(slot)
        self.calls.append("slot")
        self._e.absorbed_add_slot(col, slot)


@pytest.mark.parametrize("policy, grid, extra", [("INT groups per frequency", "octree", ""),
                                                 ("INT groups per launch", "cartesian", ""),
                                                 ("sequential", "octree", "hpbg {d}/sky.bin 2.0 1\n")])
def test_transfer_stage_adds_what_the_host_statements_add(engine, tmp_path, policy, grid, extra):
    """the three INT policies, forced as test_launch_plan's configurations force them; within one run, because float atomics may
    order the tallies differently from run to run"""
    from test_host import _write_model
    from soc_amd.asoc import AbsorptionRun, ResidentAbsorptions
    from soc_amd.ini import User
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9) if grid == "octree" else synth.cartesian_cloud(6, seed=9)
    sky = np.random.default_rng(3).lognormal(0, 1, (3, 49152)).astype(np.float32) * 1e-13
    sky.tofile(os.path.join(d, "sky.bin"))
    ini = _write_model(d, cloud, with_ps=True, with_diffuse=True, extra=extra.format(d=d) + "cellpackets %d\n" % (2 * cloud.CELLS))
    proxy = MirrorEngine(engine)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        rt = AbsorptionRun(User(ini), proxy, verbose=0)
        assert rt.resident_absorptions_refused() is None
        rt.write_packet_info()
        rt.setup_engine()
        proxy.host = np.zeros((cloud.CELLS, rt.NFREQ), np.float32)
        engine.absorbed_begin(rt.NFREQ)
        try:
            sink = ResidentAbsorptions(proxy, cloud.CELLS, rt.NFREQ)
            CTABS, F = rt.simulate_constant_sources(absorbed=sink)
            assert F is sink and CTABS.any()
            assert {p for p, _, _ in rt._plan(True, 1)[0]} == {policy}
            assert set(proxy.calls) == ({"tally"} if policy == "sequential" else {"slot"}) and len(proxy.calls) >= rt.NFREQ
            got = engine.absorbed_download(0, cloud.CELLS)
            assert got[cloud.DENS > 0].any() and np.array_equal(bits(got), bits(proxy.host))
            del proxy.calls[:]
            proxy.largest = 0.0
            EMITTED = np.where(cloud.DENS > 0, 1.0e-2, 0.0).astype(np.float32)[:, None] * np.ones((1, rt.NFREQ), np.float32)
            rt.simulate_cell_emission(EMITTED, sink)
            assert proxy.calls == ["tally"] * rt.NFREQ
            after = engine.absorbed_download(0, cloud.CELLS)
            print("%s: largest tally of the cell emission %.3e, largest absorption before it %.3e" % (policy, proxy.largest, float(got.max())))
            assert not np.array_equal(bits(after), bits(got)) and np.array_equal(bits(after), bits(proxy.host))
        finally:
            engine.absorbed_end()
    finally:
        os.chdir(cwd)
        engine.set_exec(-1, 4)


# ---- 6. refusals and lifecycle ----------------------------------------------------------------------------------------
def test_refused_calls_return_their_code_and_change_nothing(engine):
    lib, h = engine.lib, engine.h
    cells = cartesian(engine, 5, 13, 1)
    out = np.zeros((cells, 5), np.float32)
    one = np.ones(1, np.float32)
    p = lambda a: a.ctypes.data_as(_F)                                       # noqa: E731
    nn = C.c_float(0.0)
    # before soc_absorbed_begin
    assert lib.soc_absorbed_add_tally(h, 0) == ERR_STATE and b"soc_absorbed_begin first" in lib.soc_last_error(h)
    assert lib.soc_absorbed_add_slot(h, 0, 0) == ERR_STATE
    assert lib.soc_absorbed_keep(h) == ERR_STATE and lib.soc_absorbed_restore(h) == ERR_STATE
    assert lib.soc_absorbed_to_mabu(h, 0, p(one), nn) == ERR_STATE
    assert lib.soc_absorbed_download(h, 0, cells, p(out), None, nn) == ERR_STATE
    assert lib.soc_absorbed_begin(h, 0, 0) == ERR_ARG
    from soc_amd import lib as soclib
    base = soclib.device_bytes()
    for keep in (0, 1):                                                      # 65 cells x 2^31 floats: 558 GB, twice that with the second plane
        assert lib.soc_absorbed_begin(h, 2 ** 31 - 1, keep) == ERR_STATE and b"GB" in lib.soc_last_error(h)
    assert soclib.device_bytes() == base                                     # ... and nothing was reserved
    assert lib.soc_absorbed_download(h, 0, cells, p(out), None, nn) == ERR_STATE
    engine.absorbed_begin(5, keep_constant=True)
    try:
        rows = values(cells * 5, 3).reshape(cells, 5)
        fill(engine, rows)
        rows = engine.absorbed_download(0, cells)
        engine.absorbed_keep()
        T = np.arange(cells, dtype=np.float32)
        engine.write_tally(INT, T)
        engine.batch_begin_int_groups(4)                                     # an open batch: as soc_batch_read_int
        try:
            assert lib.soc_absorbed_add_slot(h, 0, 0) == ERR_STATE and b"soc_batch_end first" in lib.soc_last_error(h)
        finally:
            engine.batch_end()
        assert lib.soc_absorbed_add_slot(h, 0, 0) == ERR_ARG                 # the batch deferred no launch with the INT tally
        for rc, want in [(lib.soc_absorbed_begin(h, 0, 1), ERR_ARG), (lib.soc_absorbed_begin(h, 2 ** 31 - 1, 1), ERR_STATE),
                         (lib.soc_absorbed_add_tally(h, -1), ERR_ARG), (lib.soc_absorbed_add_tally(h, 5), ERR_ARG),
                         (lib.soc_absorbed_add_slot(h, -1, 0), ERR_ARG), (lib.soc_absorbed_add_slot(h, 5, 0), ERR_ARG),
                         (lib.soc_absorbed_add_slot(h, 0, -1), ERR_ARG), (lib.soc_absorbed_add_slot(h, 0, 127), ERR_ARG),
                         (lib.soc_absorbed_download(h, -1, 2, p(out), None, nn), ERR_ARG), (lib.soc_absorbed_download(h, 0, 0, p(out), None, nn), ERR_ARG),
                         (lib.soc_absorbed_download(h, 64, 2, p(out), None, nn), ERR_ARG), (lib.soc_absorbed_download(h, cells + 1, 1, p(out), None, nn), ERR_ARG),
                         (lib.soc_absorbed_download(h, 2 ** 62, 2 ** 62, p(out), None, nn), ERR_ARG), (lib.soc_absorbed_download(h, 1, cells, p(out), None, nn), ERR_ARG),
                         (lib.soc_absorbed_download(h, 0, cells, None, None, nn), ERR_ARG), (lib.soc_absorbed_to_mabu(h, 0, p(one), nn), ERR_STATE)]:
            assert rc == want, lib.soc_last_error(h)
        engine.mabu_begin(10, 4, 1)                                          # another NFREQ
        try:
            assert lib.soc_absorbed_to_mabu(h, 0, p(one), nn) == ERR_ARG and b"4 frequencies" in lib.soc_last_error(h)
        finally:
            engine.mabu_end()
        engine.mabu_begin(10, 5, 1)                                          # its 10 cells run past the 65
        try:
            assert lib.soc_absorbed_to_mabu(h, 56, p(one), nn) == ERR_ARG and lib.soc_absorbed_to_mabu(h, -1, p(one), nn) == ERR_ARG
            assert lib.soc_absorbed_to_mabu(h, 0, None, nn) == ERR_ARG
        finally:
            engine.mabu_end()
        assert np.array_equal(bits(engine.absorbed_download(0, cells)), bits(rows))
        engine.absorbed_restore()
        assert np.array_equal(bits(engine.absorbed_download(0, cells)), bits(rows))
        assert np.array_equal(engine.read_tally(INT), T)
    finally:
        engine.absorbed_end()


def test_binding_refuses_what_the_library_cannot_check(engine):
    from soc_amd.lib import DoesNotFit, SocError
    cells = cartesian(engine, 4, 4, 4)
    for call in (lambda: engine.absorbed_add_tally(0), lambda: engine.absorbed_add_slot(0, 0), engine.absorbed_keep, engine.absorbed_restore,
                 lambda: engine.absorbed_to_mabu(0, np.ones(1, np.float32)), lambda: engine.absorbed_download(0, cells)):
        with pytest.raises(SocError, match="absorbed_begin first"):
            call()
    with pytest.raises(DoesNotFit) as err:
        engine.absorbed_begin(2 ** 31 - 1)
    assert err.value.cells_fit == 0 and "GB" in str(err.value) and engine._absorbed is None
    engine.absorbed_begin(3)
    try:
        with pytest.raises(SocError, match=r"shape \(5, 3\)"):
            engine.absorbed_download(0, 5, out=np.zeros((5, 2), np.float32))  # narrower rows: the library would write past the array
        with pytest.raises(SocError, match="C-contiguous float32"):
            engine.absorbed_download(0, 5, out=np.zeros((5, 3), np.float64))
        with pytest.raises(SocError, match="LEVELS = 1"):
            engine.absorbed_download(0, 5, K=np.ones(2, np.float32))
        with pytest.raises(SocError, match="LEVELS = 1"):
            engine.absorbed_to_mabu(0, np.ones(2, np.float32))
        with pytest.raises(SocError, match="LEVELS = 1"):
            engine.absorbed_to_mabu(0, None)
    finally:
        engine.absorbed_end()


def test_begin_and_end_twice_set_grid_and_destroy_release_it(engine):
    from soc_amd import lib as soclib
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    engine.set_cloud(cloud)
    plane = 4 * cloud.CELLS * NFREQ
    base = soclib.device_bytes()
    for keep in (False, True):
        engine.absorbed_begin(NFREQ, keep_constant=keep)
        assert soclib.device_bytes() == base + plane * (2 if keep else 1)
        assert not bits(engine.absorbed_download(0, cloud.CELLS)).any()
        engine.absorbed_end()
        assert soclib.device_bytes() == base
    engine.absorbed_begin(NFREQ, keep_constant=True)
    engine.absorbed_download(0, cloud.CELLS)                                 # (the stage of a download goes with the arrays)
    engine.absorbed_begin(3)                                                 # a second begin replaces the first, its second plane too
    assert soclib.device_bytes() == base + 4 * cloud.CELLS * 3
    assert engine.lib.soc_absorbed_keep(engine.h) == ERR_STATE
    engine.set_cloud(cloud)                                                  # the resident absorptions go with the model
    assert soclib.device_bytes() == base
    with pytest.raises(soclib.SocError, match="absorbed_begin first"):
        engine.absorbed_download(0, 1)
    assert engine.lib.soc_absorbed_add_tally(engine.h, 0) == ERR_STATE
    engine.absorbed_end()                                                    # (nothing open: fine)
    other = soclib.Engine(0)                                                 # destroyed with the arrays open
    other.set_cloud(cloud)
    other.absorbed_begin(NFREQ, keep_constant=True)
    assert soclib.device_bytes() > base
    other.close()
    assert soclib.device_bytes() == base


# ---- 7. the pipeline on the HIP engine --------------------------------------------------------------------------------
# The bounds are those of test_gpu_reemit.py, measured there on an MI355X for the chain of the existing programs on the HIP engine
# against the same chain on the oracle engine -- the 0.98 quantile and the maximum of |a - b| / max(|b|, 1e-6 max|b|) over all cells
# that are no links (float atomics order the tallies differently, and the stochastic-heating solve amplifies the last digits of the
# absorptions): the pipeline may deviate by twice that from the oracle chain.
CHAIN_Q98, CHAIN_MAX = 4.2538e-11, 3.0269e-3


def rel_deviation(a, b):
    rel = np.abs(np.asarray(a, np.float64) - b) / np.maximum(np.abs(b), 1e-6 * np.abs(b).max())
    return float(np.quantile(rel, 0.98)), float(rel.max())


@pytest.mark.parametrize("source", ["resident", "host"])
@pytest.mark.parametrize("iterations", [2, 0])
def test_pipeline_with_either_source_on_the_gpu(engine, case, iterations, source):
    """iterations 0: the ini without `cellpackets` -- no re-emission iteration, the single hand-over from stage 1 to stage 2 (step 0 of
    the oracle chain)"""
    from reemit_chain import iteration_case
    from soc_amd import driver
    cloud = case["cloud"]
    d = os.path.join(case["d"], "pipe_%d_%s" % (iterations, source))
    ini, ini0 = iteration_case(d, cloud, 2)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        P = driver.Pipeline(ini if iterations else ini0, engine, verbose=0, absorbed_source=None if source == "resident" else 'host')
        CTABS, FABS, EMITTED = P.run(keep_files=True)
    finally:
        os.chdir(cwd)
        engine.set_exec(-1, 4)
    its = P.timers["iterations"]
    assert P.timers["emission_path"] == "device" and P.timers["absorbed_source"] == source
    assert len(its) == iterations and [it["absorbed"] for it in its] == [source] * iterations
    assert engine._absorbed is None and engine._emitted is None              # closed again
    assert engine.lib.soc_absorbed_add_tally(engine.h, 0) == ERR_STATE
    cells = cloud.DENS > 0                                                   # every cell but the links
    assert FABS.shape == (cloud.CELLS, NFREQ) and (FABS[~cells] == np.float32(-1.0e20)).all() and (FABS[cells] > 0).any()
    assert np.isfinite(EMITTED[cells]).all()
    assert np.array_equal(bits(files.read_absorbed(os.path.join(d, "abs.data"))), bits(FABS))
    F_N, E_N = case["oracle"][iterations]
    print("%s source, %d iterations: absorptions against the oracle chain: 0.98 quantile %.3e, maximum %.3e"
          % ((source, iterations) + rel_deviation(FABS[cells], F_N[cells])))
    q98, worst = rel_deviation(EMITTED[cells], E_N[cells])
    print("%s source, %d iterations: emission against the oracle chain: 0.98 quantile %.3e, maximum %.3e" % (source, iterations, q98, worst))
    assert q98 <= 2 * CHAIN_Q98 and worst <= 2 * CHAIN_MAX, (q98, worst)


def test_pipeline_reads_the_absorptions_back_only_where_they_are_wanted(engine, case):
    from reemit_chain import iteration_case
    from soc_amd import driver
    d = os.path.join(case["d"], "pipe_unwanted")
    _, ini0 = iteration_case(d, case["cloud"], 2)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        P = driver.Pipeline(ini0, engine, verbose=0)
        CTABS, FABS, EMITTED = P.run(want_absorbed=False)
    finally:
        os.chdir(cwd)
        engine.set_exec(-1, 4)
    assert P.timers["absorbed_source"] == "resident" and FABS is None and not os.path.exists(os.path.join(d, "abs.data"))
    assert EMITTED[case["cloud"].DENS > 0].any() and engine._absorbed is None
