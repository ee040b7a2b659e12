"""The streaming per-cell kernels of soc_emit.hip (soc_eqtemp_kernel, soc_emission_kernel, soc_opt_kernel,
soc_opt_half_kernel) against the oracle, bit for bit: the edges of the table lookup, of the Planck exponent and of the
fp16 rounding on small clouds, and one production-size cloud on which every grid-stride loop takes a second cell and
soc_emission a second, ragged batch.

Every comparison is made on uint32 views.  A mismatch is reported with the first differing flat indices, their
index modulo the launch's lane count and their hierarchy level, so that it points at the loop that broke."""
import functools
import gc

import numpy as np
import pytest

from oracle.pyoracle import Job
from soc_amd import launch, synth

pytestmark = pytest.mark.gpu

FF = np.logspace(np.log10(3e11), np.log10(3e15), 40)            # the dust of tests/test_temperature.py
FABS = 1e-5 * (FF / 1e13) ** 1.6
GL = 0.01
FACTOR, LENGTH = launch.kernel_literals(GL)
CSC = np.linspace(1, -1, 8)
F32 = np.float32

LANES_EQTEMP = 65536 * 256                                      # soc_launch_eqtemp, soc_launch_emission: blocks x lanes
LANES_OPT = 16384 * 256                                         # soc_launch_opt, soc_launch_opt_half
EMISSION_BATCH_FLOATS = 64 << 20                                # soc_emission: floats per batch


@functools.lru_cache(maxsize=None)
def table(NE):
    return launch.temperature_table(FF, FABS, GL, NE=NE)


def assert_bits(got, want, cloud, lanes, what, per_cell=1, skip=None):
    got, want = np.ascontiguousarray(got, F32).ravel(), np.ascontiguousarray(want, F32).ravel()
    assert got.shape == want.shape
    diff = got.view(np.uint32) != want.view(np.uint32)
    if skip is not None:
        diff &= ~np.repeat(skip, per_cell) if per_cell > 1 else ~skip
    bad = np.flatnonzero(diff)
    if bad.size:
        off = np.asarray(cloud.OFF, np.int64)
        lines = ["flat %d (cell %d, mod lanes %d, level %d): device %r, oracle %r"
                 % (k, k // per_cell, k % lanes, int(np.searchsorted(off, k // per_cell, side="right")) - 1, got[k], want[k]) for k in bad[:8]]
        raise AssertionError("%s: %d of %d values differ\n  " % (what, bad.size, got.size) + "\n  ".join(lines))


# ------------------------------------------------------------------------------------------------
# clouds
# ------------------------------------------------------------------------------------------------

def _with_threshold_densities(cloud, seed):
    """some leaves get the densities around the kernel's test `DENS > 1.0e-7f`: the threshold and its two neighbours"""
    thr = F32(1.0e-7)
    leaf = np.flatnonzero(cloud.DENS > 0)
    pick = np.random.default_rng(seed).choice(leaf, 30, replace=False)
    for k, v in enumerate((thr, np.nextafter(thr, F32(0)), np.nextafter(thr, F32(1)))):
        cloud.DENS[pick[k::3]] = v
    return cloud


@functools.lru_cache(maxsize=None)
def small_cloud(name):
    if name == "cart":
        return _with_threshold_densities(synth.cartesian_cloud(12, seed=3, NY=11, NZ=13), 1)
    if name == "oct5":                                          # 5 levels, 3800 cells
        return _with_threshold_densities(synth.octree_cloud(8, levels=5, frac=0.15, seed=7), 2)
    cl = synth.octree_cloud(3, levels=16, frac=0.16, seed=3)    # SOC_MAXL = 16 levels in 4435 cells: 8^15 on the last one
    assert cl.LEVELS == 16 and cl.CELLS < 5000
    return _with_threshold_densities(cl, 3)


SMALL = ["cart", "oct5", "deep"]


def kernel_Ein(cloud, lev, adhoc, EABS):
    """Ein of the kernel in its own fp32 operation order (without the cosmic-ray term)"""
    scale = (F32(6.62607e-27) * FACTOR) / LENGTH
    with np.errstate(all="ignore"):
        return (scale / F32(adhoc)) * EABS * (F32(8.0) ** lev).astype(F32) / cloud.DENS


def invert(cloud, lev, adhoc, Ein):
    """absorbed energy that gives the kernel Ein (tests/test_temperature.py::_absorbed)"""
    scale = 6.62607e-27 * float(FACTOR) / float(LENGTH)
    with np.errstate(all="ignore"):
        return np.minimum(Ein * np.abs(cloud.DENS.astype(np.float64)) * float(F32(adhoc)) / (scale * 8.0 ** lev), 3.0e38).astype(F32)


def edge_energies(cloud, NE, adhoc, oracle):
    """EABS[CELLS] that takes the lookup through its branches; returns (EABS, dict of index sets)"""
    Emin, kE, TTT = table(NE)
    rng = np.random.default_rng(100 + NE)
    lev = cloud.level_of_cells().astype(np.int64)
    cells = cloud.CELLS
    idx = rng.permutation(cells)
    part = {}
    names = ["below", "edge", "above", "inside", "special"]
    share = [0.1, 0.45, 0.1, 0.25, 0.1]
    cut = np.concatenate([[0], np.cumsum(np.asarray(share) * cells).astype(int)])
    for k, nm in enumerate(names):
        part[nm] = np.sort(idx[cut[k]:cut[k + 1]])
    Ein = np.zeros(cells, np.float64)
    Ein[part["below"]] = Emin * 10.0 ** -rng.uniform(0.001, 6, part["below"].size)          # iE clamped to 0, 3 K clamp
    top = Emin * kE ** (NE - 1)
    Ein[part["above"]] = top * 10.0 ** rng.uniform(0.5, 1, part["above"].size)              # iE = NE-2, 1600 K clamp
    Ein[part["inside"]] = Emin * kE ** rng.uniform(0, NE - 1, part["inside"].size)
    # the bins next to the table, floor(...) = -1 and NE-1: the values the two clamps of iE are there for
    Ein[part["inside"][:20]] = Emin * kE ** rng.uniform(-0.95, -0.05, 20)
    Ein[part["inside"][20:40]] = Emin * kE ** (NE - 1 + rng.uniform(0.05, 0.95, 20))
    # the bin edges as the kernel computes them, Emin * pown(kE, i), and a few floats either side
    ne = part["edge"].size
    i_edge = rng.integers(0, NE, ne).astype(np.int32) if NE > 2 else (np.arange(ne) % 2).astype(np.int32)
    if NE > 2:
        i_edge[:30] = np.repeat([0, 1, NE // 2, NE - 2, NE - 1], 6)            # the first and the last bins for certain
    edge = F32(Emin) * oracle.math("pown", np.full(ne, kE, F32), i_edge)
    Ein[part["edge"]] = edge.astype(np.float64) * (1.0 + rng.integers(-2, 3, ne) * 2.0 ** -23)
    EABS = invert(cloud, lev, adhoc, Ein)
    # the inversion goes through four roundings: nudge EABS float by float until the kernel's Ein is the target
    tgt = np.zeros(cells, F32)
    tgt[part["edge"]] = edge
    third = part["edge"][0::3], part["edge"][1::3], part["edge"][2::3]
    tgt[third[1]] = np.nextafter(tgt[third[1]], F32(0))
    tgt[third[2]] = np.nextafter(tgt[third[2]], F32(np.inf))
    e = part["edge"]
    for _ in range(6):
        have = kernel_Ein(cloud, lev, adhoc, EABS)[e]
        up = (have < tgt[e]) == (cloud.DENS[e] > 0)
        step = np.where(up, np.nextafter(EABS[e], F32(np.inf)), np.nextafter(EABS[e], F32(-np.inf)))
        EABS[e] = np.where(have == tgt[e], EABS[e], step)
    have = kernel_Ein(cloud, lev, adhoc, EABS)
    hit = {"at": third[0][have[third[0]] == tgt[third[0]]], "under": third[1][have[third[1]] == tgt[third[1]]],
           "over": third[2][have[third[2]] == tgt[third[2]]]}
    # absorbed energies that are no energies
    sp = part["special"]
    vals = F32([0.0, -0.0, -1.0e-3, -3.0e38, 1.0e-45, 1.1e-39, 3.0e38, np.inf, -np.inf, np.nan])
    EABS[sp] = vals[np.arange(sp.size) % vals.size]
    part.update(hit)
    part["zero"] = sp[EABS[sp] == 0]
    part["lev"] = lev
    return EABS, part


def cr_rate_inside(NE):
    """a cosmic-ray heating rate whose term alone, 1e-27 * FACTOR * rate, heats a cell to about 400 K"""
    Emin, kE, TTT = table(NE)
    E = 0.5 * Emin * kE if NE == 2 else Emin * kE ** int(np.abs(TTT - 400.0).argmin())
    return float(E / (1.0e-27 * float(FACTOR)))


@pytest.mark.parametrize("cr", [False, True], ids=["nocr", "cr"])
@pytest.mark.parametrize("adhoc", [1.0, 0.37])
@pytest.mark.parametrize("NE", [2, 3000, 6000])
@pytest.mark.parametrize("name", SMALL)
def test_temperature_edges(name, NE, adhoc, cr, engine, oracle_soc):
    """soc_eqtemp_kernel at the edges of its lookup: energies below the table, beyond its top, on the bin edges
    Emin * kE^i as the kernel computes them and one float either side, EABS of 0, -0, negative, subnormal and 3e38,
    densities at the 1e-7 threshold, link cells (density -0 and negative), 8^level up to level 15, tables of 2, 3000
    and 6000 entries, adhoc 1 and 0.37, cosmic-ray heating on cells with and without absorbed energy.

    EABS of +inf, -inf and NaN are in the input and are left out of the comparison: the kernel converts
    floor(...) of a non-finite value to int, which C leaves undefined, so the x86 build of the oracle and the
    conversion instruction of the GPU need not agree on them and nothing is claimed for them here."""
    cloud = small_cloud(name)
    Emin, kE, TTT = table(NE)
    EABS, part = edge_energies(cloud, NE, adhoc, oracle_soc)
    job = Job(cloud, CSC)
    rate = cr_rate_inside(NE) if cr else 0.0
    job.CR_HEATING_RATE = rate
    want = oracle_soc.eqtemp(job, adhoc, kE, Emin, TTT, FACTOR, LENGTH, EABS)
    job.CR_HEATING_RATE = 0.0
    plain = want if not cr else oracle_soc.eqtemp(job, adhoc, kE, Emin, TTT, FACTOR, LENGTH, EABS)
    finite = np.isfinite(EABS)
    # the oracle's own output says that every branch was taken
    leaf = cloud.DENS > F32(1.0e-7)
    w = want[finite]
    assert (w == 3.0).any() and (w == 1600.0).any() and (w == 10.0).any() and ((w > 3.0) & (w < 1600.0) & (w != 10.0)).any()
    assert (plain[part["below"]][leaf[part["below"]]] == 3.0).all()
    assert (plain[part["above"]][leaf[part["above"]]] == 1600.0).all()
    assert (want[~leaf] == 10.0).all() and (~leaf & (cloud.DENS > 0)).sum() >= 20 and (cloud.DENS[leaf] > F32(1.0e-7)).all()
    assert (cloud.DENS == np.nextafter(F32(1.0e-7), F32(1))).any() and (want[cloud.DENS == np.nextafter(F32(1.0e-7), F32(1))] != 10.0).any()
    if cloud.LEVELS > 1:
        assert (cloud.DENS < 0).any() and ((cloud.DENS == 0) & np.signbit(cloud.DENS)).any()      # link cells, the first one is -0
    for k in ("at", "under", "over"):                           # the bin edges were really hit
        assert part[k].size >= (20 if NE > 2 else 5), (k, part[k].size)
    zl = part["zero"][leaf[part["zero"]]]
    assert zl.size and (plain[zl] == 3.0).all()                 # log10(0) = -inf: iE = 0
    if cr:
        assert ((want[zl] > 3.0) & (want[zl] < 1600.0)).all()   # heated by cosmic rays alone
        assert not np.array_equal(want[finite], plain[finite])
    engine.set_cloud(cloud)
    engine.set_temperature(np.zeros(cloud.CELLS, F32))          # no temperature: a cell the kernel skips shows
    engine.set_cr_heating(rate)
    try:
        got = engine.solve_temperature(adhoc, kE, Emin, TTT, FACTOR, LENGTH, EABS)
    finally:
        engine.set_cr_heating(0.0)
    assert_bits(got, want, cloud, LANES_EQTEMP, "TNEW %s NE=%d adhoc=%g cr=%g" % (name, NE, adhoc, rate), skip=~finite)


# ------------------------------------------------------------------------------------------------
# emission
# ------------------------------------------------------------------------------------------------

def emission_temperatures(cells, seed):
    rng = np.random.default_rng(seed)
    T = np.exp(rng.uniform(np.log(3.0), np.log(1600.0), cells)).astype(F32)
    T[0::7] = 3.0
    T[1::7] = 10.0
    T[2::7] = 1600.0
    return T


def emission_frequencies(nfreq, k=0):
    if nfreq == 1:
        return F32([[1.0e8], [3.0e16], [2.0e12]][k])
    return np.logspace(8, np.log10(3e16), nfreq).astype(F32)


@pytest.mark.parametrize("nfreq", [1, 7, 50])
@pytest.mark.parametrize("name", SMALL)
def test_emission_edges(name, nfreq, engine, oracle_soc):
    """soc_emission_kernel from 1e8 to 3e16 Hz at 3 K to 1600 K: the Planck exponent h nu / k T runs from 3e-6, where
    exp(x) - 1 cancels, to 4.8e5, where soc_expf returns +inf and the emission is exactly 0; nfreq 1 (three separate
    frequencies), 7 and 50"""
    cloud = small_cloud(name)
    T = emission_temperatures(cloud.CELLS, 5)
    engine.set_cloud(cloud)
    engine.set_temperature(T)
    xs, zeros = [], 0
    for k in range(3 if nfreq == 1 else 1):
        FREQ = emission_frequencies(nfreq, k)
        FA = (1e-5 * (FREQ.astype(np.float64) / 1e13) ** 1.6).astype(F32)
        want = oracle_soc.emission(FREQ, FA, FACTOR, LENGTH, T)
        x = F32(4.7995074e-11) * FREQ[None, :] / T[:, None]
        zeros += int(((want == 0) & (x > F32(88.72))).sum())
        assert ((want == 0) == (x > F32(88.72))).all() and np.isfinite(want).all()
        xs.append(x.min())
        got = engine.emission(FREQ, FA, FACTOR, LENGTH)
        assert got.shape == (cloud.CELLS, nfreq)
        assert_bits(got, want, cloud, LANES_EQTEMP, "EMITTED %s nfreq=%d" % (name, nfreq), per_cell=nfreq)
    assert zeros > 0 and min(xs) < 1e-5                         # overflow and cancellation both occurred


# ------------------------------------------------------------------------------------------------
# opacities
# ------------------------------------------------------------------------------------------------

def abundances(cells, ndust, single, seed):
    """uniform and logarithmic spreads, exact 0 and 1"""
    rng = np.random.default_rng(seed)
    shape = cells if single else (cells, ndust)
    ABU = rng.uniform(0.0, 1.0, shape)
    sel = rng.uniform(0, 1, shape)
    ABU = np.where(sel < 0.3, 10.0 ** rng.uniform(-14, 0, shape), ABU)
    ABU = np.where(sel > 0.9, 0.0, ABU)
    ABU = np.where((sel > 0.8) & (sel <= 0.9), 1.0, ABU)
    return np.ascontiguousarray(ABU, F32)


def cross_sections(ndust):
    """from 7e4 (fp16 overflows above 65520) down to 1e-9 (fp16 holds nothing below 3e-8)"""
    a = F32([7.0e4, 3.0e-7, 1.0e-4, 2.0e-8, 1.0e-9])[:ndust]
    s = F32([9.0e4, 2.0e-8, 3.0e-4, 5.0e-6, 3.0e-9])[:ndust]
    return a, s


def numpy_opt(ABU, AFABS, AFSCA, single, half):
    """the expressions of test_gpu_parity.py::test_opt_from_abundances_on_device (ASOC.py:1146-1160)"""
    cells = ABU.shape[0]
    OPT = np.zeros((cells, 2), F32)
    if single:
        OPT[:, 0] += ABU * AFABS[0] + (1.0 - ABU) * AFABS[1]
        OPT[:, 1] += ABU * AFSCA[0] + (1.0 - ABU) * AFSCA[1]
    else:
        for d in range(len(AFABS)):
            OPT[:, 0] += ABU[:, d] * AFABS[d]
            OPT[:, 1] += ABU[:, d] * AFSCA[d]
    if half:
        with np.errstate(over="ignore"):
            OPT = np.asarray(np.asarray(OPT, np.float16), F32)
    return OPT


def run_opt(engine, cloud, ABU, AFABS, AFSCA, single, half):
    engine.set_opt_half(half)
    try:
        engine.set_abundances(ABU, single=single)
        engine.set_optical_abu(AFABS, AFSCA)
        return engine.read_opt()
    finally:
        engine.set_opt_half(False)
        engine.set_abundances(None)
        engine.set_opt(None)


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["ndust1", "ndust3", "ndust5", "single"])
def test_opacity_edges(kind, half, engine):
    """soc_opt_kernel (1, 3 and 5 species, the one-abundance form) and soc_opt_half_kernel against the numpy
    expressions: abundances of exactly 0 and 1, and sums that fp16 holds as subnormals, as zero and as inf"""
    single = kind == "single"
    ndust = 2 if single else int(kind[5:])
    AFABS, AFSCA = cross_sections(ndust)
    for name in ("cart", "oct5"):
        cloud = small_cloud(name)
        ABU = abundances(cloud.CELLS, ndust, single, 17)
        want = numpy_opt(ABU, AFABS, AFSCA, single, half)
        assert (ABU == 0).any() and (ABU == 1).any()
        if half:
            plain = numpy_opt(ABU, AFABS, AFSCA, single, False)
            assert np.isinf(want).any() and ((want == 0) & (plain > 0)).any()
            assert ((want > 0) & (want < F32(6.1035156e-5))).any() and not np.array_equal(want, plain)
        engine.set_cloud(cloud)
        got = run_opt(engine, cloud, ABU, AFABS, AFSCA, single, half)
        assert_bits(got, want, cloud, LANES_OPT, "OPT %s %s half=%d" % (name, kind, half), per_cell=2)


# ------------------------------------------------------------------------------------------------
# production size: every lane of every launch takes a second cell
# ------------------------------------------------------------------------------------------------

class Big:
    pass


@pytest.fixture(scope="module")
def big_cart():
    b = Big()
    b.cloud = synth.cartesian_cloud(259, NY=257, NZ=253)
    b.job = Job(b.cloud, CSC)
    yield b
    b.__dict__.clear()
    gc.collect()


@pytest.fixture(scope="module")
def big_oct():
    b = Big()
    b.cloud = synth.octree_cloud(256, levels=4, frac=0.001, seed=5)
    b.job = Job(b.cloud, CSC)
    yield b
    b.__dict__.clear()
    gc.collect()


def spread_energies(cloud, NE, seed):
    """energies over the whole table and 5 % of its length (in bins) beyond either end"""
    Emin, kE, TTT = table(NE)
    rng = np.random.default_rng(seed)
    Ein = Emin * kE ** (rng.random(cloud.CELLS, F32).astype(np.float64) * (1.1 * NE) - 0.05 * NE)
    lev = cloud.level_of_cells().astype(np.int64)
    scale = 6.62607e-27 * float(FACTOR) / float(LENGTH)
    return np.minimum(Ein * np.abs(cloud.DENS.astype(np.float64)) / (scale * 8.0 ** lev), 3.0e38).astype(F32)      # finite


def check_big_temperature(engine, oracle, b, NE=6000):
    Emin, kE, TTT = table(NE)
    EABS = spread_energies(b.cloud, NE, 21)
    want = oracle.eqtemp(b.job, 1.0, kE, Emin, TTT, FACTOR, LENGTH, EABS)
    n3, n1600 = int((want == 3.0).sum()), int((want == 1600.0).sum())
    inside = int(((want > 3.0) & (want < 1600.0) & (want != 10.0)).sum())
    assert n3 > 1000 and n1600 > 1000 and inside > 0.5 * b.cloud.CELLS
    assert np.unique(want).size > 100000                        # all over the table
    engine.set_temperature(np.zeros(b.cloud.CELLS, F32))        # no temperature: a cell the kernel skips shows
    got = engine.solve_temperature(1.0, kE, Emin, TTT, FACTOR, LENGTH, EABS)
    assert_bits(got, want, b.cloud, LANES_EQTEMP, "TNEW")
    return want


def test_big_cartesian_temperature_and_emission(engine, oracle_soc, big_cart):
    """259 x 257 x 253 = 16 840 439 cells, an odd number above the 65536 x 256 lanes of soc_launch_eqtemp: a lane takes
    a second cell and the last tile is ragged.  Emission at 5 frequencies is 84 202 195 values: soc_emission takes them
    as two batches, the second one starting at cell c0 > 0 and ragged, each a grid-stride launch.  Then the shared
    buffer dEbuf in either order: a small emission after the large solve, a solve after the large emission."""
    cloud = big_cart.cloud
    assert cloud.CELLS == 16840439 and cloud.CELLS > LANES_EQTEMP and cloud.CELLS % 256 != 0
    engine.set_cloud(cloud)
    T = check_big_temperature(engine, oracle_soc, big_cart)
    # a small emission after the large solve
    FREQ = F32([2.0e12])
    got = engine.emission(FREQ, F32([1e-5]), FACTOR, LENGTH)
    assert_bits(got, oracle_soc.emission(FREQ, F32([1e-5]), FACTOR, LENGTH, T), cloud, LANES_EQTEMP, "EMITTED nfreq=1 after the solve")
    del got
    # the large emission: two strided batches
    nfreq = 5
    batch = EMISSION_BATCH_FLOATS // nfreq
    assert batch < cloud.CELLS <= 2 * batch                     # two batches ...
    assert batch * nfreq > LANES_EQTEMP and (cloud.CELLS - batch) * nfreq > LANES_EQTEMP and ((cloud.CELLS - batch) * nfreq) % 256 != 0
    FREQ = emission_frequencies(nfreq)
    FA = (1e-5 * (FREQ.astype(np.float64) / 1e13) ** 1.6).astype(F32)
    want = oracle_soc.emission(FREQ, FA, FACTOR, LENGTH, T)
    assert (want == 0).any() and (want > 0).sum() > 0.5 * want.size
    got = engine.emission(FREQ, FA, FACTOR, LENGTH)
    diff = np.flatnonzero(got.ravel().view(np.uint32) != want.ravel().view(np.uint32))
    if diff.size:
        k = diff[:8]
        raise AssertionError("EMITTED nfreq=5: %d values differ; flat, cell, batch, (flat in batch) mod lanes: %s" % (
            diff.size, [(int(i), int(i // nfreq), int(i // nfreq // batch), int((i - (i // nfreq // batch) * batch * nfreq) % LANES_EQTEMP)) for i in k]))
    del got, want
    # a solve after the large emission (dEbuf has grown to a batch of emission by now)
    check_big_temperature(engine, oracle_soc, big_cart, NE=3000)


def test_big_octree_temperature(engine, oracle_soc, big_oct):
    """a 256^3-root octree with 4 levels: the level lookup (sOFF) and 8^level for cells that only a second
    iteration of the grid-stride loop reaches"""
    cloud = big_oct.cloud
    assert cloud.CELLS > LANES_EQTEMP
    assert cloud.CELLS % 256 != 0
    assert cloud.LEVELS == 4 and cloud.OFF[cloud.LEVELS - 1] > LANES_EQTEMP
    engine.set_cloud(cloud)
    want = check_big_temperature(engine, oracle_soc, big_oct)
    assert (want[cloud.DENS <= 0] == 10.0).all() and (cloud.DENS <= 0).sum() > 10000
    deep = want[cloud.OFF[1]:]
    assert ((deep > 3.0) & (deep < 1600.0) & (deep != 10.0)).sum() > 0.4 * deep.size


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("kind", ["ndust3", "single"])
def test_big_cartesian_opacities(kind, half, engine, big_cart):
    """16 840 439 cells against the 16384 x 256 lanes of soc_launch_opt and soc_launch_opt_half: five cells per lane"""
    cloud = big_cart.cloud
    assert cloud.CELLS > 4 * LANES_OPT
    single = kind == "single"
    ndust = 2 if single else 3
    AFABS, AFSCA = cross_sections(ndust)
    ABU = abundances(cloud.CELLS, ndust, single, 23)
    want = numpy_opt(ABU, AFABS, AFSCA, single, half)
    engine.set_cloud(cloud)
    got = run_opt(engine, cloud, ABU, AFABS, AFSCA, single, half)
    assert_bits(got, want, cloud, LANES_OPT, "OPT %s half=%d" % (kind, half), per_cell=2)
