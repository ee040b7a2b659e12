"""The library method for dust emission on the CPU: the restatement of the look-up against what the reference's kernel gives
(tests/golden/library.npz), its two math modes against each other, the restatement of the build against a numpy statement of
soc_library.py:127-217, and the round trip of the program soc_amd.library on a synthetic solver."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import library_cases as lc                             # noqa: E402
import library_host                                    # noqa: E402
from library_numpy import GRID, bits, numpy_build, same_build   # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "library.npz")
f32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_is_for_these_cases(golden):
    assert str(golden["meta"]) == lc.meta()


@pytest.mark.parametrize("name", sorted(lc.SOLVE))
def test_lookup_restatement_equals_the_reference(golden, name):
    """libm mode, bit for bit: column 0 of every cell, the whole row of every cell the library answers; and a missed row is
    1e32 followed by zeros, the missed cells listed in ascending order"""
    case = lc.solve_case(name)
    EMI, ijkm, miss = library_host.solve("libm", case["lib"], case["ABS3"])
    hit = ~(golden["EMI0_" + name] > 1.0e31)
    assert np.array_equal(bits(EMI[:, 0]), bits(golden["EMI0_" + name]))
    assert np.array_equal(bits(EMI[hit]), bits(golden["ROWS_" + name]))
    assert np.array_equal(miss, np.nonzero(~hit)[0]) and np.array_equal(ijkm[:, 3] != 0, ~hit)
    assert (EMI[~hit, 0] == f32(1.0e32)).all() and (EMI[~hit, 1:] == 0.0).all()
    if case["ocol"] is not None:                       # the selection of output columns is the same rows, those columns
        sel, _, miss2 = library_host.solve("libm", case["lib"], case["ABS3"], ocol=case["ocol"])
        assert np.array_equal(bits(sel[hit]), bits(EMI[hit][:, case["ocol"]])) and np.array_equal(miss2, miss)
        assert (sel[~hit, 0] == f32(1.0e32)).all() and (sel[~hit, 1:] == 0.0).all()


def test_lookup_cases_cover_what_they_are_there_for(golden):
    miss = {k: int((golden["EMI0_" + k] > 1.0e31).sum()) for k in lc.SOLVE}
    n = {k: lc.SOLVE[k][2] for k in lc.SOLVE}
    assert miss["all_miss"] == n["all_miss"] and miss["no_miss"] == 0 and miss["halves"] == 0
    assert 0 < miss["clamped"] < n["clamped"] and 0 < miss["empty_bins"] < n["empty_bins"]
    # "halves": coordinates of exactly 0.5 go to bin 1 (away from zero), not to bin 0 (to even)
    case = lc.solve_case("halves")
    _, ijkm, _ = library_host.solve("libm", case["lib"], case["ABS3"])
    assert (ijkm[0::2, :3] == 1).all() and (ijkm[:, 0] == 1).all() and (ijkm[:, 2] == 1).all()
    # "clamped": cells beyond the first and beyond the last bin on every axis, answered and missed
    case = lc.solve_case("clamped")
    _, ijkm, _ = library_host.solve("libm", case["lib"], case["ABS3"])
    N = case["lib"]["N"]
    for axis in range(3):
        for edge in (0, N - 1):
            at = ijkm[:, axis] == edge
            assert (ijkm[at, 3] == 0).any() and (ijkm[at, 3] == 1).any()
    # "empty_bins": misses that come from the 1e32 row alone
    case = lc.solve_case("empty_bins")
    L = case["lib"]
    _, ijkm, _ = library_host.solve("libm", L, case["ABS3"])
    b = ijkm[:, 2] + N * (ijkm[:, 1] + N * ijkm[:, 0])
    assert ((L["E"][b, 0] > 1.0e31) & (ijkm[:, 3] == 1)).any()


@pytest.mark.parametrize("name", sorted(lc.SOLVE))
def test_lookup_math_modes_differ_only_where_a_rounding_moves_a_cell(name):
    """soc_log10f against libm's log10f: a last-bit difference may move a cell across a half-integer or across the 1.1
    threshold; at most 0.5 % of a case's cells may land elsewhere, all others are the same bits.  (Counted on these fixtures
    when they were made: no cell of any case differs.)"""
    case = lc.solve_case(name)
    A, ia, _ = library_host.solve("libm", case["lib"], case["ABS3"])
    B, ib, _ = library_host.solve("soc", case["lib"], case["ABS3"])
    moved = (ia != ib).any(axis=1)
    print("%s: %d of %d cells differ in (i, j, k, miss)" % (name, int(moved.sum()), len(moved)))
    assert moved.sum() <= 0.005 * len(moved)
    assert np.array_equal(bits(A[~moved]), bits(B[~moved]))


# ---- the build against a numpy statement of soc_library.py:127-217 (tests/library_numpy.py) ----

@pytest.mark.parametrize("name", [k for k in sorted(lc.BUILD) if lc.BUILD[k][1] <= 5000])
def test_build_restatement_equals_numpy(name):
    case = lc.build_case(name)
    N, ABS3 = case["N"], case["ABS3"]
    got = library_host.build("libm", N, ABS3)
    assert same_build(got, numpy_build(N, ABS3, lambda x: library_host.log10("libm", x))) == []


def test_build_restatement_equals_numpy_with_numpys_own_log10():
    """numpy's float32 log10 is not libm's log10f (it differs in the last bit on about a third of all inputs), so the cases above
    hand numpy_build the restatement's logarithm.  Here the premise is made to hold instead: of a pool of candidate values those
    on which the two logarithms agree are kept, and a case is drawn from them alone."""
    pool = np.asarray([10.0 ** -k for k in range(25)] + [2.0 ** -k for k in range(1, 80)] + [3.0 * 10.0 ** -k for k in range(1, 20)], f32)
    keep = pool[bits(np.log10(pool)) == bits(library_host.log10("libm", pool))]
    assert len(keep) >= 20, "numpy.log10 and log10f agree on %d of %d candidate values only" % (len(keep), len(pool))
    rng = np.random.Generator(np.random.PCG64(5))
    ABS3 = np.ascontiguousarray(keep[rng.integers(0, len(keep), (400, 3))])
    assert np.array_equal(bits(np.log10(ABS3)), bits(library_host.log10("libm", ABS3)))
    for N in (3, 6):
        assert same_build(library_host.build("libm", N, ABS3), numpy_build(N, ABS3)) == []


def test_build_edge_cases_are_what_they_claim():
    b = {k: library_host.build("libm", lc.BUILD[k][0], lc.build_case(k)["ABS3"]) for k in ("one_cell", "two_cells", "two_clumps", "clipped", "twins", "c5000")}
    # one cell: its own bin on axes 0 and 1; one cell is no grid on axis 2 (`< 2`), so no bin represents it
    assert (b["one_cell"]["I1"] < 99.0).sum() == 1 and (b["one_cell"]["I2"] == f32(100.0)).all() and (b["one_cell"]["IND"] == -1).all()
    # two cells far apart: windows of axis 1 with exactly one cell are defined, those of axis 2 are not; everything is filled in
    t = b["two_cells"]
    assert (t["I1"] < 99.0).sum() == 2 and (t["I2"] == f32(100.0)).all() and (t["dI2"] == f32(0.001)).all()
    # two clumps: empty windows of axis 0 in between, and the raster fill gives their (i, j) the grid of the last defined one
    c = b["two_clumps"]
    empty = np.nonzero(c["I1"] == f32(100.0))[0]
    flat = c["I2"].ravel()
    assert len(empty) >= 2 and (flat[np.argmax(flat < 99.0):] < 99.0).all()       # (only what precedes the first defined one stays undefined)
    i = empty[0]
    assert i > 0 and (bits(c["I2"][i]) == bits(c["I2"][i - 1, -1])).all()
    # absorptions of 0 and above 1 are clipped to 1e-25 and 1: the grid of axis 0 spans exactly those
    case = lc.build_case("clipped")
    assert (case["ABS3"] == 0.0).any() and (case["ABS3"] > 1.0).any()
    lo, hi = f32(-25.0), f32(0.0)
    d = (hi - lo) / f32(5) + f32(0.1)
    assert b["clipped"]["dI0"] == np.clip(f32(1.001) * ((hi + d) - (lo - d)) / f32(5), f32(1e-30), f32(1e30))
    # identical cells: the lower index represents the bin
    ind = b["twins"]["IND"]
    assert (ind >= 0).any() and not ((ind >= 100) & (ind < 200)).any()
    # a populated case: windows with no cell, with one and with many, and most bins of the cube empty
    assert (b["c5000"]["IND"] >= 0).sum() > 20 and (b["c5000"]["IND"] < 0).any()


@pytest.mark.parametrize("mode", ["libm", "soc"])
def test_build_rounds_halves_to_even_and_the_lookup_away_from_zero(mode):
    """The build case "halves" plants a cell whose coordinates on axes 0 and 1 are 2.5 exactly, in either math mode (the grid is
    spanned by cells whose logarithms agree in both).  The build puts it into bin (2, 2, .) -- numpy's round, halves to even --
    and it represents that bin; the look-up on the library of that very grid rounds away from zero, to (3, 3, .).  (The numpy
    statement and the device kernels are held to the case through lc.BUILD.)"""
    case = lc.build_case("halves")
    N, ABS3, P = case["N"], case["ABS3"], lc.HALF_CELL
    g = library_host.build(mode, N, ABS3)
    IREF = library_host.log10(mode, np.clip(ABS3[P], f32(1.0e-25), f32(1.0)))
    x = (IREF[0] - g["I0"]) / g["dI0"]
    y = (IREF[1] - g["I1"][2]) / g["dI1"][2]
    assert x == f32(2.5) and y == f32(2.5)                            # the premise, in float32 as the build computes it
    bins = np.nonzero(g["IND"] == P)[0]
    assert len(bins) == 1
    i, j, k = bins[0] // (N * N), (bins[0] // N) % N, bins[0] % N
    assert (i, j) == (2, 2)
    assert g["X"][i, j, k] == f32(2.5) and g["Y"][i, j, k] == f32(2.5) and abs(g["Z"][i, j, k] - k) < 0.5
    assert (g["IND"].reshape(N, N, N)[3] != P).all()                  # not where rounding away from zero would put it
    L = dict(g, E=np.ones((N ** 3, 1), f32))
    _, ijkm, _ = library_host.solve(mode, L, ABS3[P:P + 1])
    assert tuple(ijkm[0, :2]) == (3, 3)
    # the look-up's own case of halves: coordinates of 0.5 exactly go to bin 1
    case = lc.solve_case("halves")
    _, ijkm, _ = library_host.solve(mode, case["lib"], case["ABS3"][:1])
    assert tuple(ijkm[0, :3]) == (1, 1, 1)


# ---- the round trip of the program ----

@pytest.fixture(scope="module")
def roundtrip(tmp_path_factory):
    import library_roundtrip as rt
    from library_engine import LibraryEngine
    return rt, rt.run_program(tmp_path_factory.mktemp("library"), lambda: LibraryEngine("soc"))


def test_roundtrip_library_file_and_build_set(roundtrip):
    from soc_amd import a2e
    from library_engine import LibraryEngine
    rt, out = roundtrip
    sol = rt.solver()
    first, _ = rt.sets(sol)
    L = out["lib"]
    eng = LibraryEngine("soc")
    grid = library_host.build("soc", rt.N, first[:, list(rt.REF)])
    # the file read back with the layout of soc_library.py:246-266 reproduces the arrays
    assert L["N"] == rt.N and L["NFREQ"] == rt.NFREQ and np.array_equal(L["FREQ"], sol["FREQ"])
    assert [k for k in GRID + ("X", "Y", "Z") if not np.array_equal(bits(L[k]), bits(grid[k]))] == []
    rep = grid["IND"]
    has = rep >= 0
    assert has.sum() > 20 and (L["E"][~has] == f32(1.0e32)).all()
    direct, _ = a2e.run(eng, sol, first[rep[has]], verbose=False)
    direct = np.clip(direct, f32(1.0e-30), f32(1.0e30))
    assert np.array_equal(bits(L["E"][has]), bits(direct))
    # solving the build set with its own library: no miss; a representative gets its own row, every other cell its bin's row
    E1 = out["first"]
    assert E1.shape == (rt.CELLS, rt.NFREQ) and not (E1[:, 0] > 1.0e31).any()
    assert np.array_equal(bits(E1[rep[has]]), bits(direct))
    _, ijkm, miss = library_host.solve("soc", L, first[:, list(rt.REF)])
    assert len(miss) == 0
    b = ijkm[:, 2] + rt.N * (ijkm[:, 1] + rt.N * ijkm[:, 0])
    assert np.array_equal(bits(E1), bits(L["E"][b]))
    # ofreq selects those columns, in its order
    assert np.array_equal(bits(out["ofreq"]), bits(E1[:, list(rt.OFREQ)]))


def test_roundtrip_cells_outside_the_library(roundtrip):
    from soc_amd import a2e
    from library_engine import LibraryEngine
    rt, out = roundtrip
    sol = rt.solver()
    _, second = rt.sets(sol)
    L, new = out["lib"], out["new"]
    looked, ijkm, miss = library_host.solve("soc", L, second[:, list(rt.REF)])
    assert 0 < len(miss) < len(second)
    hit = ijkm[:, 3] == 0
    direct, _ = a2e.run(LibraryEngine("soc"), sol, second[miss], verbose=False)
    # all frequencies: the missed cells are solved directly, the others looked up
    assert np.array_equal(bits(out["second"][hit]), bits(looked[hit]))
    assert np.array_equal(bits(out["second"][miss]), bits(direct))
    # ... and their rows are in the new library, whose grid is the old one
    assert [k for k in GRID if not np.array_equal(bits(new[k]), bits(L[k]))] == []
    changed = np.nonzero((bits(new["E"]) != bits(L["E"])).any(axis=1))[0]
    assert 0 < len(changed) <= len(miss)
    rows = {bits(r).tobytes() for r in direct}
    assert all(bits(new["E"][c]).tobytes() in rows for c in changed)
    # three columns: the same misses, their rows zero, the others as before
    assert np.array_equal(bits(out["three"][hit]), bits(looked[hit])) and (out["three"][miss] == 0.0).all()


def test_a_library_misses_only_cells_that_are_alone_in_their_window():
    """The set of the round trip without the twins: a cell that is alone in its (i, j) window gets no grid of its own on axis 2
    (`< 2`, soc_library.py:162) but the one the raster fill hands it.  Where that grid does not reach the cell no bin represents
    it, and the library built from the set misses it; a lone cell the borrowed grid does reach is answered.  So the library
    misses some cells of its own set, every one of them alone in its window, and no cell that has company."""
    import library_roundtrip as rt
    N = rt.N
    A = rt.absorptions(rt.solver(), 11, -9.0, -6.0)[:, list(rt.REF)]
    g = library_host.build("soc", N, A)
    L = dict(g, E=np.where((g["IND"] >= 0)[:, None], f32(1.0), f32(1.0e32)).astype(f32))
    _, _, miss = library_host.solve("soc", L, A)
    R = library_host.log10("soc", np.clip(A, f32(1.0e-25), f32(1.0)))
    alone = []
    for c in range(len(A)):                                           # the windows of the reference, as it writes them (:148, :161)
        i = int(np.clip(np.round((R[c, 0] - g["I0"]) / g["dI0"]), 0, N - 1))
        in0 = np.abs(R[:, 0] - (g["I0"] + f32(i) * g["dI0"])) < f32(0.5) * g["dI0"]
        j = int(np.clip(np.round((R[c, 1] - g["I1"][i]) / g["dI1"][i]), 0, N - 1))
        both = in0 & (np.abs(R[:, 1] - (g["I1"][i] + f32(j) * g["dI1"][i])) < f32(0.5) * g["dI1"][i])
        if both.sum() < 2:
            alone.append(c)
    assert 0 < len(miss) <= len(alone) < 20 and set(miss.tolist()) <= set(alone)


def test_program_refuses_a_dust_file(tmp_path, capsys):
    from soc_amd import library
    p = tmp_path / "dust.dust"
    p.write_text("eqdust\n1.0e-7\n")
    assert library.main(["library", "1", str(p), str(p)], lambda: None) == 1
    assert "eqdust" in capsys.readouterr().out


# ---- `libabs` and `libmaps` of python -m soc_amd.asoc ----

def _absorption_run(ini, **kw):
    from oracle_engine import OracleEngine
    from soc_amd.asoc import AbsorptionRun
    from soc_amd.ini import User
    run = AbsorptionRun(User(ini), OracleEngine("soc"), verbose=0, **kw)
    run.run()
    return run


@pytest.fixture(scope="module")
def libabs_runs(tmp_path_factory):
    """One model (an octree with a point source and the background: the frequencies of a launch group share a sweep) run with
    all three frequencies, with `libabs` on the first and the last, and both again under a `simum` that leaves the first out."""
    from soc_amd import files, synth
    from test_host import _write_model
    d = str(tmp_path_factory.mktemp("libabs"))
    cloud = synth.octree_cloud(5, levels=2, frac=0.1, seed=4)
    np.savetxt(os.path.join(d, "sel.txt"), [5.4e14 * 1.0005, 4.0e14 * 0.9995])          # any order, within 0.1 %
    cwd = os.getcwd()
    os.chdir(d)
    try:
        out = {}
        for name, extra in (("full", ""), ("libabs", "libabs %s/sel.txt\n" % d), ("full_simum", "simum 0.5 0.7\n"),
                            ("libabs_simum", "libabs %s/sel.txt\nsimum 0.5 0.7\n" % d)):
            ini = _write_model(d, cloud, with_ps=True, extra=extra + "absorbed %s/%s.abs\n" % (d, name))
            _absorption_run(ini)
            out[name] = files.read_absorbed(os.path.join(d, name + ".abs"))
    finally:
        os.chdir(cwd)
    return cloud, out


def test_libabs_columns_are_those_of_the_full_run(libabs_runs):
    cloud, out = libabs_runs
    leaf = cloud.DENS > 0
    assert out["full"].shape == (cloud.CELLS, 3) and out["libabs"].shape == (cloud.CELLS, 2)
    assert (out["full"][leaf] > 0).any(axis=0).all()
    # the columns count the selected frequencies in table order, whatever the order of the file
    assert np.array_equal(bits(out["libabs"][:, 0]), bits(out["full"][:, 0]))
    assert np.array_equal(bits(out["libabs"][:, 1]), bits(out["full"][:, 2]))
    # `simum 0.5 0.7` leaves the first frequency (0.75 um) out: its column keeps its place and stays empty
    assert (out["full_simum"][leaf, 0] == 0.0).all() and (out["full_simum"][leaf, 1:] > 0).any(axis=0).all()
    assert out["libabs_simum"].shape == (cloud.CELLS, 2) and (out["libabs_simum"][leaf, 0] == 0.0).all()
    assert np.array_equal(bits(out["libabs_simum"][:, 1]), bits(out["full"][:, 2]))
    assert np.array_equal(bits(out["full_simum"][:, 2]), bits(out["full"][:, 2]))


def test_libabs_on_a_cartesian_grid_and_a_single_frequency(tmp_path):
    """a file with one value is a list of one (every launch an INT group of its own on this grid)"""
    from soc_amd import files, synth
    from test_host import _write_model
    d = str(tmp_path)
    cloud = synth.cartesian_cloud(4, seed=1)
    np.savetxt(os.path.join(d, "one.txt"), [4.677e14])
    os.chdir(d)
    _absorption_run(_write_model(d, cloud, extra="absorbed %s/full.abs\n" % d))
    run = _absorption_run(_write_model(d, cloud, extra="libabs %s/one.txt\nabsorbed %s/one.abs\n" % (d, d)))
    assert run.U.LIB_ABS and not run.U.LIB_MAPS and run.U.FSELECT.shape == (1,)
    one, full = files.read_absorbed(os.path.join(d, "one.abs")), files.read_absorbed(os.path.join(d, "full.abs"))
    assert one.shape == (cloud.CELLS, 1) and np.array_equal(bits(one[:, 0]), bits(full[:, 1]))


def test_libabs_reaches_the_plan_of_both_shard_modes(tmp_path):
    """only the selected frequencies are launched; shard "launches" deals those out, the k-th to rank k % world"""
    import types
    from soc_amd import synth
    from soc_amd.asoc import AbsorptionRun
    from soc_amd.ini import User
    from test_host import _write_model
    d = str(tmp_path)
    np.savetxt(os.path.join(d, "sel.txt"), [4.0e14, 5.4e14])
    ini = _write_model(d, synth.octree_cloud(5, levels=2, frac=0.1, seed=4), with_ps=True, extra="libabs %s/sel.txt\n" % d)
    for shard in ("items", "launches"):
        owners = []
        for rank in (0, 1):
            run = AbsorptionRun(User(ini), None, types.SimpleNamespace(rank=rank, world=2), verbose=0, shard=shard)
            run.ROI_LOAD = None
            segments, owner = run._plan(True, 1)
            assert sorted({f for _, _, steps in segments for f, _, _ in steps}) == [0, 2]
            assert [run._abs_col(f) for f in (0, 2)] == [0, 1]
            owners.append(owner)
        assert owners == ([None, None] if shard == "items" else [{0: 0, 2: 1}] * 2)


def test_library_keys_are_refused_with_their_reason(tmp_path):
    from soc_amd import synth
    from soc_amd.asoc import AbsorptionRun, UnsupportedOption
    from soc_amd.ini import User
    from test_host import _write_model
    d = str(tmp_path)
    cloud = synth.cartesian_cloud(4, seed=1)
    np.savetxt(os.path.join(d, "sel.txt"), [4.0e14, 5.4e14])
    key = "libabs %s/sel.txt\n" % d
    for extra, reason in ((key + "libmaps %s/sel.txt\n" % d, "libabs together with libmaps"),
                          (key + "saveint 1 %s/int.bin\n" % d, "libabs with saveint"),
                          (key + "cellpackets 1000\n", "libabs with iterations > 0 and cellpackets"),
                          (key + "absthin 4\n", "libabs with absthin or nnmake"),
                          (key + "nnmake 1\n", "libabs with absthin or nnmake"),
                          ("libmaps %s/sel.txt\nmaplevels 1\n" % d, "libmaps with maplevels"),
                          ("libmaps %s/sel.txt\nmapping 12 10 0.8 999\n" % d, "libmaps with a fourth mapping argument"),
                          ("libmaps %s/sel.txt\npolmap bx by bz\n" % d, "polmap together with libmaps")):
        with pytest.raises(UnsupportedOption, match=reason):
            AbsorptionRun(User(_write_model(d, cloud, extra=extra)), None)
    # a file that cannot be read is reported by the run with its name -- after the refusals, which need no file
    with pytest.raises(UnsupportedOption, match="polmap together with libmaps"):
        AbsorptionRun(User(_write_model(d, cloud, extra="libmaps %s/none.txt\npolmap bx by bz\n" % d)), None)
    with pytest.raises(ValueError, match="libabs .*none.txt"):
        AbsorptionRun(User(_write_model(d, cloud, extra="libabs %s/none.txt\n" % d)), None)


def test_libmaps_images_are_those_of_the_run_with_the_full_emission(tmp_path):
    """maps of the selected frequencies from an emitted file that holds only their columns: the same bytes as those images of a
    run that has the emission of all frequencies; the other frequencies are absent.  Flat maps and a Healpix map."""
    from soc_amd import files, synth
    from test_host import _write_model
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    for sub in ("full", "lib", "hfull", "hlib"):
        os.mkdir(os.path.join(d, sub))
    np.savetxt(os.path.join(d, "sel.txt"), [5.4e14, 4.0e14])

    def ini_for(extra):
        ini = _write_model(d, cloud, extra=extra)
        txt = open(ini).read().replace("nosolve\n", "").replace("nomap\n", "").replace("absorbed %s/abs.data\n" % d, "")
        open(ini, "w").write(txt)
        return ini

    flat = "mapping 12 10 0.8\ndirection 30 40\ndirection 90 0\n"
    os.chdir(os.path.join(d, "full"))
    run = _absorption_run(ini_for("noabsorbed\niterations 1\ntemperature %s/T.bin\nemitted %s/em.bin\n%s" % (d, d, flat)))
    assert run.EMITTED.shape == (cloud.CELLS, 3)
    files.write_emitted(os.path.join(d, "em_sel.bin"), np.ascontiguousarray(np.asarray(run.EMITTED)[:, [0, 2]]))
    os.chdir(os.path.join(d, "lib"))
    lib = _absorption_run(ini_for("libmaps %s/sel.txt\nemitted %s/em_sel.bin\nremit 0.6 0.7\nwavelength 0.6 0.7\niterations 3\n%s" % (d, d, flat)))
    assert lib.U.ITERATIONS == 0 and lib.U.NOSOLVE == 1 and lib.U.FAST_MAP == 0 and lib.U.MAP_FREQ == [1.0e-10, 1.0e30]     # ASOC.py:124-129
    for idir in (0, 1):
        name = "map_dir_%02d.bin" % idir
        full = np.fromfile(os.path.join(d, "full", name), np.float32, offset=8).reshape(3, 10, 12)
        got = np.fromfile(os.path.join(d, "lib", name), np.float32, offset=8)
        assert list(np.fromfile(os.path.join(d, "lib", name), np.int32, 2)) == [12, 10]
        assert got.size == 2 * 120 and full[[0, 2]].tobytes() == got.tobytes() and full.sum() > 0
    # a Healpix map
    heal = "mapping 4 -1 0.8\nperspective 3.0 3.0 3.0\n"
    os.chdir(os.path.join(d, "hfull"))
    _absorption_run(ini_for("noabsorbed\niterations 1\ntemperature %s/T.bin\nemitted %s/em2.bin\n%s" % (d, d, heal)))
    os.chdir(os.path.join(d, "hlib"))
    _absorption_run(ini_for("libmaps %s/sel.txt\nemitted %s/em_sel.bin\n%s" % (d, d, heal)))
    full = np.fromfile(os.path.join(d, "hfull", "map_dir_00_H.bin"), np.float32, offset=16).reshape(3, 192)
    got = np.fromfile(os.path.join(d, "hlib", "map_dir_00_H.bin"), np.float32, offset=16)
    assert list(np.fromfile(os.path.join(d, "hlib", "map_dir_00_H.bin"), np.int32, 4)) == [4, -1, 2, cloud.LEVELS]
    assert full[[0, 2]].tobytes() == got.tobytes() and full.sum() > 0


def test_without_the_keys_nothing_changes(tmp_path):
    """the parser's defaults, and the maps of the run of tests/test_maps.py re-derived from the oracle's map kernel"""
    import math
    from oracle.pyoracle import Job, Oracle, oracle_mapping
    from soc_amd import files, launch, synth
    from soc_amd.ini import User
    from test_host import _write_model
    U = User(text="cloud a.cloud\n")
    assert U.LIB_ABS is False and U.LIB_MAPS is False and len(U.FSELECT) == 0
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini = _write_model(d, cloud, extra="noabsorbed\niterations 1\ntemperature %s/T.bin\nemitted %s/em.bin\nmapping 12 10 0.8\ndirection 30 40\n" % (d, d))
    txt = open(ini).read().replace("nosolve\n", "").replace("nomap\n", "").replace("absorbed %s/abs.data\n" % d, "")
    open(ini, "w").write(txt)
    os.chdir(d)
    run = _absorption_run(ini)
    assert run.lib_col is None
    FFREQ, _, AFABS, AFSCA = files.read_dust([os.path.join(d, "m.dust")], 0.5)
    KK = (1.0e23 / launch.FACTOR) * launch.PLANCK / (4.0 * np.pi) * 0.5 * launch.PARSEC
    _, OD, RA, DE = launch.set_observer_directions([math.radians(30)], [math.radians(40)])
    _, csc = synth.hg_scattering_table(0.6, 500)
    maps = np.fromfile("map_dir_00.bin", np.float32, offset=8).reshape(3, 10, 12)
    for i in range(3):
        emit = np.asarray(KK * float(FFREQ[i]) * run.EMITTED[:, i], np.float32)
        want, _ = oracle_mapping(Oracle("soc"), Job(cloud, csc, ABS=AFABS[0][i], SCA=AFSCA[0][i]), emit, OD[0], RA[0], DE[0], (12, 10), 0.8, (3.0, 3.0, 3.0))
        assert np.array_equal(bits(maps[i].ravel()), bits(want))
