"""The library method for several dust components on the device (soc_mabu_library_*, soc_mabu_gather_rows;
soc_amd/csrc/soc_mabu_library.hip): the fused look-up against the composition of the pinned pieces on the host -- per dust
mabu.split_absorbed, the soc-mode restatement of the look-up (tests/csrc/library_host.c) with missed rows zeroed, SUM += EMI *
ABU[:, d] in float32 -- to the bit, the sum and the miss masks of every cell; the refusals; the ranges after a refusal for lack
of memory; the libraries --makelib writes on the device path against those of the host path; the row gather.  (The look-up of one
library, whose index arithmetic the fused kernel shares, stays pinned by tests/test_gpu_library.py.)"""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import library_cases as lc                             # noqa: E402
from mabu_library_engine import composition            # noqa: E402

pytestmark = pytest.mark.gpu

LIB_KINDS = ("mixed", "empty", "tight")                # per dust in turn: a tenth of the bins empty; four in ten; none, representatives near the centres

# name: (n, NDUST, N, NFREQ, ocol, abundances).  Every value of every axis at least once -- n at the wave (64) and tile (256) edges,
# NDUST 1, 2, 3 and the 32 of the mask, N 2, 3, 30, nout 1, 7, 65, with and without ocol -- and the extremes together
CASES = {
    "n1": (1, 1, 2, 1, None, "ones"),
    "n63": (63, 2, 3, 7, None, "single"),
    "n64": (64, 3, 30, 65, None, "random"),
    "n65_ocol": (65, 3, 3, 9, [5, 0, 6, 2, 8, 8, 1], "zero"),
    "n255_ocol": (255, 2, 2, 5, [3], "single"),
    "n256": (256, 32, 3, 7, None, "random"),
    "n257": (257, 1, 30, 7, None, "ones"),
    "n1000": (1000, 32, 30, 65, None, "zero"),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_case(name):
    """dict(libs, ABS3, ABU, RABS3, ocol, shifted): a library per dust (tests/library_cases.py::_library, its kinds in turn; one
    positive emission table scaled per dust, so that a dust taken for another shows), with NDUST >= 2 the library of dust 1 shifted
    on axis 1 as `all_miss` is (by 1000 bins, not two: the cells here also lie beyond the edges, further than a bin from a representative); cell c aims at the grid of dust c % NDUST: most anywhere from two bins below the first to one
    above the last (`mixed`), some near a bin centre, some beyond an edge on one axis or on all (`clamped`), four with values the
    clamp of the look-up catches; the abundances ones, random in (0, 1], (a, 1 - a), or random with zeros for dust 0 in every
    fifth cell (with NDUST 1 none: a row keeps a positive entry)"""
    n, NDUST, N, NFREQ, ocol, abu = CASES[name]
    rng = lc._rng("mabu_library_" + name)
    RABS3 = rng.random((3, NDUST)) + 0.05
    RABS3 /= RABS3.sum(axis=1)[:, None]
    if abu == "ones":
        ABU = np.ones((n, NDUST), np.float32)
    elif abu == "single":
        a = (0.02 + 0.96 * rng.random(n)).astype(np.float32)
        ABU = np.stack([a, np.float32(1.0) - a], axis=1)
    else:
        ABU = (1.0 - rng.random((n, NDUST))).astype(np.float32)
        if abu == "zero" and NDUST > 1:
            ABU[::5, 0] = 0.0
    assert (ABU.max(axis=1) > 0).all()
    base = (10.0 ** (-20.0 + 10.0 * rng.random((N ** 3, NFREQ)))).astype(np.float32)
    libs = []
    for d in range(NDUST):
        kind = LIB_KINDS[d % 3]
        lib = lc._library(rng, N, 1, empty=dict(mixed=0.1, empty=0.4, tight=0.0)[kind], spread=0.5 if kind == "mixed" else 0.3)
        lib["E"] = np.where(lib["E"][:, :1] > 1.0e31, np.float32(1.0e32), base * np.float32(1.0 + 0.125 * d)).astype(np.float32)
        libs.append(lib)
    shifted = 1 if NDUST >= 2 else None
    if shifted is not None:
        libs[1]["Y"] = (libs[1]["Y"] + np.float32(1000.0)).astype(np.float32)
    # the shares the cells aim at, then the absorptions that give them: share = a * R[f, d] / den[f]
    den = np.zeros((n, 3), np.float32)
    for j in range(NDUST):
        den = (den.astype(np.float64) + ABU[:, j:j + 1].astype(np.float64) * RABS3[None, :, j]).astype(np.float32)
    ABS3 = np.zeros((n, 3), np.float32)
    for d in range(NDUST):
        cells = np.arange(d, n, NDUST)
        m = len(cells)
        if m < 1:
            continue
        x, y, z = (lc._uniform(rng, m, -2.0, N + 1.0) for _ in range(3))
        how = rng.random(m) if n > 1 else np.zeros(m)              # (the one cell of n = 1 gets an answer)
        near = how < 0.2
        x, y, z = (np.where(near, rng.integers(0, N, m) + lc._uniform(rng, m, -0.3, 0.3), v) for v in (x, y, z))
        out = np.where(rng.random(m) < 0.5, lc._uniform(rng, m, -1.6, -0.6), lc._uniform(rng, m, N - 0.4, N + 0.6))
        axis = rng.integers(0, 4, m)
        for k, v in enumerate((x, y, z)):
            v[:] = np.where((how > 0.8) & ((axis == k) | (axis == 3)), out, v)
        share = lc._cells(libs[d], x, y, z).astype(np.float64)
        ABS3[cells] = (share * den[cells] / RABS3[None, :, d]).astype(np.float32)
    if n >= 63:
        ABS3[5, 0], ABS3[6, 1], ABS3[7, 2], ABS3[8, :] = 0.0, 1.0e20, 0.0, 1.0e-35
    return dict(libs=libs, ABS3=ABS3, ABU=ABU, RABS3=RABS3, ocol=None if ocol is None else np.asarray(ocol, np.int32), shifted=shifted)


def device_lookup(engine, c, chunks=2):
    n, NDUST = c["ABU"].shape
    nout = c["libs"][0]["E"].shape[1] if c["ocol"] is None else len(c["ocol"])
    engine.mabu_library_begin(n, NDUST, nout)
    try:
        for d, lib in enumerate(c["libs"]):
            engine.mabu_library_set(d, lib, c["ocol"])
        step = max(1, (n + chunks - 1) // chunks)
        for a in range(0, n, step):
            engine.mabu_library_upload(a, c["ABS3"][a:a + step])
        engine.mabu_library_set_tables(c["ABU"], c["RABS3"])
        engine.mabu_library_solve()
        SUM = np.concatenate([engine.mabu_library_download(a, min(step, n - a)) for a in range(0, n, step)])
        MISS = np.concatenate([engine.mabu_library_misses(a, min(step, n - a)) for a in range(0, n, step)])
    finally:
        engine.mabu_library_end()
    return SUM, MISS


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_lookup_equals_the_host_composition_to_the_bit(engine, name):
    c = make_case(name)
    n, NDUST = c["ABU"].shape
    want, wmiss = composition("soc", c["libs"], c["ABS3"], c["ABU"], c["RABS3"], c["ocol"])
    got, miss = device_lookup(engine, c)
    assert got.shape == want.shape and miss.shape == (n,) and miss.dtype == np.uint32
    assert np.array_equal(miss, wmiss)                               # every cell, every dust
    assert np.array_equal(bits(got), bits(want))
    if c["shifted"] is not None:                                     # `all_miss` for exactly that dust
        assert (wmiss & np.uint32(2)).astype(bool).all()
    if n >= 63:                                                      # the case means something: answers and misses, sums of several dusts
        hits = np.asarray([np.count_nonzero(~(wmiss >> np.uint32(d)) & np.uint32(1)) for d in range(NDUST) if d != c["shifted"]])
        assert hits.sum() > 0 and (hits < n).all() and (want > 0).any()
        assert np.count_nonzero(want.sum(axis=1) == 0) < n


def test_halves_round_away_from_zero_in_the_fused_kernel(engine):
    """one dust with the cross section 1 and the abundance 1: the share is the absorption, and the planted case of
    tests/library_cases.py (coordinates of 0.5 exactly) takes the bins the look-up of one library takes"""
    case = lc.solve_case("halves")
    n = len(case["ABS3"])
    c = dict(libs=[case["lib"]], ABS3=case["ABS3"], ABU=np.ones((n, 1), np.float32), RABS3=np.ones((3, 1), np.float64), ocol=None)
    want, wmiss = composition("soc", c["libs"], c["ABS3"], c["ABU"], c["RABS3"])
    got, miss = device_lookup(engine, c, chunks=1)
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(miss, wmiss)
    engine.library_set(case["lib"])
    try:
        one, _ = engine.library_solve(case["ABS3"])
    finally:
        engine.library_set(None)
    assert np.array_equal(bits(got), bits(one)) and not wmiss.any()


def test_refusals(engine):
    from soc_amd.lib import SocError
    with pytest.raises(SocError, match="1 <= NDUST <= 32, the width of the miss mask"):
        engine.mabu_library_begin(10, 33, 5)
    with pytest.raises(SocError, match="call soc_mabu_library_begin first"):
        engine.mabu_library_solve()
    c = make_case("n63")
    engine.mabu_library_begin(63, 2, 7)
    try:
        engine.mabu_library_set(0, c["libs"][0])
        engine.mabu_library_upload(0, c["ABS3"])
        with pytest.raises(SocError, match="call soc_mabu_library_set_tables first"):
            engine.mabu_library_solve()
        engine.mabu_library_set_tables(c["ABU"], c["RABS3"])
        with pytest.raises(SocError, match="dust 1 of 2 has no library"):
            engine.mabu_library_solve()
        with pytest.raises(SocError, match="gives 4 columns, soc_mabu_library_begin reserved 7"):
            engine.mabu_library_set(1, c["libs"][1], [0, 1, 2, 3])
        with pytest.raises(SocError, match=r"cells \[60, 70\) of 63"):
            engine.mabu_library_download(60, 10)
        with pytest.raises(SocError, match=r"cells \[63, 64\) of 63"):
            engine.mabu_library_upload(63, c["ABS3"][:1])
    finally:
        engine.mabu_library_end()
    with pytest.raises(SocError, match="call mabu_begin first"):
        engine.mabu_gather_rows([0])


def write_eq_dusts(d, NDUST, NFREQ):
    """NDUST equilibrium dust files on one frequency table, with cross sections of different slopes"""
    FREQ = np.logspace(11.2, 15.3, NFREQ)
    names = []
    for i in range(NDUST):
        names.append(os.path.join(d, "eq%d.dust" % i))
        with open(names[-1], "w") as fp:
            fp.write("eqdust\n %.3e\n 5.0e-5\n%d\n" % (1.0e-7 * (1 + i), NFREQ))
            for f in FREQ:
                fp.write(" %.5e  0.4  %.5e  %.5e\n" % (f, 3.0e-2 * (f / 1e14) ** (0.8 + 0.3 * i), 3.0e-2 * (f / 1e14) ** 1.1))
    return names


class ShortOfMemory:
    """the engine with a device that takes at most `capacity` cells per look-up: mabu_library_begin refuses more as the library does"""

    def __init__(self, engine, capacity):
        self.eng, self.capacity, self.begun = engine, capacity, []

    def __getattr__(self, name):
        return getattr(self.eng, name)

    def mabu_library_begin(self, cells, NDUST, nout):
        from soc_amd.lib import DoesNotFit
        if cells > self.capacity:
            raise DoesNotFit("%d cells need more device memory than is free (%d cells fit)" % (cells, self.capacity), self.capacity)
        self.begun.append(cells)
        return self.eng.mabu_library_begin(cells, NDUST, nout)


def test_cells_are_looked_up_in_ranges_after_a_refusal_and_both_paths_agree(engine, tmp_path):
    from soc_amd import mabu
    c = make_case("n1000")
    NDUST, NFREQ = 32, 65
    dusts = write_eq_dusts(str(tmp_path), NDUST, NFREQ)
    cols = [3, 20, 40]
    RABS, _ = mabu.relative_cross_sections(dusts, ['eqdust'] * NDUST)
    want, wmiss = composition("soc", c["libs"], c["ABS3"], c["ABU"], RABS[cols])
    one, i1 = mabu.solve_emission_library(engine, dusts, ['eqdust'] * NDUST, c["ABS3"], c["ABU"], c["libs"], cols)
    assert (i1["path"], i1["ranges"]) == ("device", 1)
    tight = ShortOfMemory(engine, 300)
    many, im = mabu.solve_emission_library(tight, dusts, ['eqdust'] * NDUST, c["ABS3"], c["ABU"], c["libs"], cols)
    assert (im["path"], im["ranges"], tight.begun) == ("device", 4, [300, 300, 300, 100])
    host, ih = mabu.solve_emission_library(engine, dusts, ['eqdust'] * NDUST, c["ABS3"], c["ABU"], c["libs"], cols, path='host')
    assert ih["path"] == "host"
    for em, info in ((one, i1), (many, im), (host, ih)):
        assert np.array_equal(bits(em), bits(want)) and np.array_equal(info["miss"], wmiss)
        assert info["missed"] == [int(np.count_nonzero(wmiss & np.uint32(1 << d))) for d in range(NDUST)]
    assert i1["missed"][1] == 1000


def test_gather_rows(engine, tmp_path):
    """1, 64 and 65 indices, repeats and both ends of the resident cells included, against the rows of the emission read back"""
    from soc_amd import mabu
    from soc_amd.launch import FACTOR
    from soc_amd.lib import SocError
    NFREQ, n = 7, 300
    dust = write_eq_dusts(str(tmp_path), 1, NFREQ)[0]
    Fq, KABS, Emin, kE, oplgkE, TTT = mabu.eq_dust_table(dust)
    rng = lc._rng("mabu_gather_rows")
    ABS = (10.0 ** lc._uniform(rng, (n, NFREQ), -9.0, -5.0)).astype(np.float32)
    engine.mabu_begin(n, NFREQ, 1)
    try:
        engine.mabu_upload(0, ABS)
        engine.mabu_set_tables(np.ones((n, 1), np.float32), np.ones((NFREQ, 1), np.float64))
        engine.mabu_split(0)
        engine.mabu_solve_eq(mabu.NE_EQ, FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT)
        EM = engine.a2e_resident_download(0, n)
        assert (EM > 0).any() and len(np.unique(EM[:, 0])) > n // 2
        for m in (1, 64, 65):
            idx = rng.integers(0, n, m).astype(np.int32)
            idx[0] = n - 1
            if m > 1:
                idx[1], idx[2], idx[-1] = 0, n - 1, idx[3]           # repeats
            got = engine.mabu_gather_rows(idx)
            assert got.shape == (m, NFREQ) and np.array_equal(bits(got), bits(EM[idx]))
        for bad in ([n], [-1], [0, n + 5]):
            with pytest.raises(SocError, match="of %d resident cells" % n):
                engine.mabu_gather_rows(bad)
    finally:
        engine.mabu_end()


def test_makelib_on_the_device_path_writes_the_bytes_of_the_host_path(engine, tmp_path):
    """the three-dust model of tests/test_mabu_library.py: the emitted file and every <dust>.mlib, device path against host path; the
    look-up from those libraries on the device against the host composition, and --uselib's direct rows"""
    from oracle_engine import OraclePipelineEngine
    from soc_amd import driver, files, library, mabu, synth
    from test_driver import NFREQ, write_case
    from test_mabu import write_ini, write_third_dust
    from test_mabu_library import NBINS, REF, SCALE, three_optical
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, sol, abu = write_case(d, cloud)
    os.chdir(d)
    driver.Pipeline(ini, OraclePipelineEngine("soc"), verbose=0).run(keep_files=True)
    carb = write_third_dust(d, cloud.CELLS)
    A = files.read_absorbed(os.path.join(d, "abs.data"))
    FABS = np.where(A > -1.0e19, A * SCALE, A).astype(np.float32)
    absorbed, abs3, lfreq = (os.path.join(d, x) for x in ("abs_scaled.data", "abs3.data", "lfreq.dat"))
    files.write_absorbed(absorbed, FABS)
    files.write_absorbed(abs3, np.ascontiguousarray(FABS[:, REF]))
    np.savetxt(lfreq, np.asarray(sol["FREQ"], np.float64)[REF])
    ini3 = write_ini(d, "three.ini", three_optical(d))
    inilib = write_ini(d, "three_lib.ini", three_optical(d), "libabs %s\n" % lfreq)
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    products = {}
    for path in ("host", "device"):
        out = os.path.join(d, "emitted_%s.data" % path)
        info = mabu.run(ini3, absorbed, out, engine, makelib=(lfreq, NBINS), path=path)
        assert info["path"] == path
        products[path] = [open(out, "rb").read()] + [open(mabu.library_name(x), "rb").read() for x in dusts]
    assert products["host"] == products["device"]
    plain = os.path.join(d, "emitted_plain.data")
    mabu.run(ini3, absorbed, plain, engine)
    assert open(plain, "rb").read() == products["device"][0]       # the option changes no product
    libs = [library.read_library(mabu.library_name(x)) for x in dusts]
    assert all(50 < np.count_nonzero(lib["E"][:, 0] < 1e31) < cloud.CELLS for lib in libs)
    # the look-up of a `libabs` run and --uselib, device against host
    ABU = np.stack([abu, np.ones(cloud.CELLS, np.float32), carb], axis=1)
    RABS, _ = mabu.relative_cross_sections(dusts, [mabu.dust_kind(x) for x in dusts])
    want, wmiss = composition("soc", libs, FABS[:, REF], ABU, RABS[REF])
    out = os.path.join(d, "emitted_look.data")
    info = mabu.run(inilib, abs3, out, engine)
    got = np.asarray(files.mmap_emitted(out, cloud.CELLS, NFREQ))
    assert info["path"] == "device" and np.array_equal(bits(got), bits(want)) and np.array_equal(info["miss"], wmiss)
    assert 0 < np.count_nonzero(wmiss) < cloud.CELLS
    info = mabu.run(ini3, absorbed, out, engine, uselib=lfreq)
    got = np.asarray(files.mmap_emitted(out, cloud.CELLS, NFREQ))
    direct = np.asarray(files.mmap_emitted(plain, cloud.CELLS, NFREQ))
    missed = wmiss != 0
    assert np.array_equal(bits(got[~missed]), bits(want[~missed]))
    leaf = cloud.DENS > 0
    assert np.array_equal(info["solved"], np.flatnonzero(missed))
    assert np.array_equal(bits(got[missed & leaf]), bits(direct[missed & leaf]))   # (cells are independent: the direct solve of the same run)
