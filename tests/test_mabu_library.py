"""The library method for a model with several dust components (soc_amd.mabu --makelib / libabs / --uselib, soc_amd.driver) on the
CPU: the oracle-backed engine with the restated library calls (tests/mabu_library_engine.py), i.e. the host paths, and the device
branches on a numpy stand-in for the resident calls.

The model is the three-dust case of tests/test_mabu.py with its absorptions scaled by 1e-6: the library's grid clips the
absorptions to [1e-25, 1] as the reference does (soc_library.py:127-131), and the synthetic sources of tests/test_driver.py leave
absorptions of up to 5e4, which all fall on the upper clip."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import a2e, files, library, synth       # noqa: E402
from test_driver import NFREQ, write_case            # noqa: E402
from test_mabu import write_ini, write_third_dust    # noqa: E402

REF = [2, 6, 10]                                      # the reference columns
NBINS = 30                                            # 27000 bins for 392 cells
SCALE = np.float32(1.0e-6)


def three_optical(d, simple=False):
    return ["%s/sil.dust %s/sil.abu" % (d, d), "%s/%s.dust" % (d, "pah_simple" if simple else "gs_pah"), "%s/carb.dust %s/carb.abu" % (d, d)]


def direct_per_dust(engine, dusts, kinds, FABS, ABU):
    """the emission of every dust from its share, as mabu._solve_host solves it: [NDUST][CELLS, NFREQ]"""
    from soc_amd import mabu
    from soc_amd.launch import FACTOR
    RABS, _ = mabu.relative_cross_sections(dusts, kinds)
    tables = mabu._tables(dusts, kinds, FABS.shape[1])
    out = []
    for i, k in enumerate(kinds):
        part = mabu.split_absorbed(FABS, RABS, ABU, i)
        if k == 'eqdust':
            Fq, KABS, Emin, kE, oplgkE, TTT = tables[i]
            _, em = engine.eqsolver(0, len(part), mabu.NE_EQ, FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT, part)
        else:
            em, _ = a2e.run(engine, tables[i], part, NSTOCH=mabu.NSTOCH_ALL, verbose=False)
        out.append(np.asarray(em, np.float32))
    return out, RABS


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the pipeline of tests/test_driver.py run once for its absorbed file; the third dust; the absorptions scaled; the libraries built
    by the program on its host path, beside a run without the option"""
    from mabu_library_engine import MabuLibraryEngine
    from soc_amd import driver, mabu
    d = str(tmp_path_factory.mktemp("mabulib"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, sol, abu = write_case(d, cloud)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        driver.Pipeline(ini, MabuLibraryEngine("soc"), verbose=0).run(keep_files=True)
    finally:
        os.chdir(cwd)
    carb = write_third_dust(d, cloud.CELLS)
    A = files.read_absorbed(os.path.join(d, "abs.data"))
    FABS = np.where(A > -1.0e19, A * SCALE, A).astype(np.float32)
    absorbed = os.path.join(d, "abs_scaled.data")
    files.write_absorbed(absorbed, FABS)
    abs3 = os.path.join(d, "abs3.data")
    files.write_absorbed(abs3, np.ascontiguousarray(FABS[:, REF]))
    FREQ = np.asarray(sol["FREQ"], np.float64)
    lfreq = os.path.join(d, "lfreq.dat")
    np.savetxt(lfreq, FREQ[REF])
    ini3 = write_ini(d, "three.ini", three_optical(d))
    inilib = write_ini(d, "three_lib.ini", three_optical(d), "libabs %s\n" % lfreq)
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    kinds = [mabu.dust_kind(x) for x in dusts]
    eng = MabuLibraryEngine("soc")
    plain, made = os.path.join(d, "emitted_plain.data"), os.path.join(d, "emitted_makelib.data")
    mabu.run(ini3, absorbed, plain, eng)
    mabu.run(ini3, absorbed, made, eng, makelib=(lfreq, NBINS))
    ABU = np.stack([abu, np.ones(cloud.CELLS, np.float32), carb], axis=1)
    EMD, RABS = direct_per_dust(eng, dusts, kinds, FABS, ABU)
    return dict(d=d, cloud=cloud, CELLS=cloud.CELLS, FREQ=FREQ, FABS=FABS, ABU=ABU, RABS=RABS, EMD=EMD, dusts=dusts, kinds=kinds, eng=eng,
                absorbed=absorbed, abs3=abs3, lfreq=lfreq, ini3=ini3, inilib=inilib, plain=plain, made=made,
                direct=np.asarray(files.mmap_emitted(plain, cloud.CELLS, NFREQ)),
                libs=[library.read_library(mabu.library_name(x)) for x in dusts],
                mlib={x: open(mabu.library_name(x), "rb").read() for x in dusts})


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_makelib_changes_no_product_and_writes_the_library_of_every_dust(case, tmp_path):
    import library_host
    from soc_amd import mabu
    with open(case["plain"], "rb") as a, open(case["made"], "rb") as b:
        assert a.read() == b.read()                                # the emitted file, bit for bit
    assert [os.path.basename(mabu.library_name(x)) for x in case["dusts"]] == ["sil.mlib", "gs_pah.mlib", "carb.mlib"]
    for i, (dust, lib) in enumerate(zip(case["dusts"], case["libs"])):
        again = str(tmp_path / ("again%d.mlib" % i))
        library.write_library(again, lib)                          # round trip
        with open(again, "rb") as fp:
            assert fp.read() == case["mlib"][dust]
        assert lib["N"] == NBINS and lib["E"].shape == (NBINS ** 3, NFREQ)
        assert np.allclose(lib["FREQ"], case["FREQ"], rtol=1e-5)    # (the table as the last dust file prints it: five decimals)
        part = mabu.split_absorbed(case["FABS"], case["RABS"], case["ABU"], i)     # the plain split, no clip of the last channel
        want = library_host.build("soc", NBINS, part[:, REF])
        for k in ("I0", "dI0", "I1", "dI1", "I2", "dI2", "X", "Y", "Z"):
            assert np.array_equal(bits(lib[k]), bits(want[k])), (dust, k)
        m = want["IND"] >= 0
        assert 50 < m.sum() < case["CELLS"]
        rows = np.clip(case["EMD"][i][want["IND"][m]], np.float32(1e-30), np.float32(1e30))
        assert np.array_equal(bits(lib["E"][m]), bits(rows)), dust                 # that dust's direct emission of the cell IND names
        assert (lib["E"][~m] == np.float32(1e32)).all()


def test_device_branch_writes_the_same_libraries_from_one_cell_range_only(case, tmp_path):
    from mabu_library_engine import ResidentLibraryStandIn
    from soc_amd import mabu
    from soc_amd.asoc import UnsupportedOption
    st = ResidentLibraryStandIn(10 ** 9)
    out = str(tmp_path / "emitted.data")
    try:
        info = mabu.run(case["ini3"], case["absorbed"], out, st, makelib=(case["lfreq"], NBINS))
        assert info["path"] == "device" and st.begun == [case["CELLS"]] and not st.open
        for dust in case["dusts"]:
            with open(mabu.library_name(dust), "rb") as fp:
                assert fp.read() == case["mlib"][dust], dust
        with open(out, "rb") as a, open(case["plain"], "rb") as b:
            assert a.read() == b.read()
        # a reference column that is the last channel: the grid comes from the share before the solver route clips it
        lf = str(tmp_path / "lfreq_last.dat")
        np.savetxt(lf, case["FREQ"][[2, 6, NFREQ - 1]])
        libs = []
        for eng in (case["eng"], ResidentLibraryStandIn(10 ** 9)):
            mabu.run(case["ini3"], case["absorbed"], out, eng, makelib=(lf, 8))
            libs.append([open(mabu.library_name(x), "rb").read() for x in case["dusts"]])
        assert libs[0] == libs[1]
        # the cells need several ranges: refused, no library from part of the model
        with pytest.raises(UnsupportedOption, match="from one cell range.*%d fit the free device memory" % 100):
            mabu.run(case["ini3"], case["absorbed"], out, ResidentLibraryStandIn(100), makelib=(case["lfreq"], NBINS))
        with pytest.raises(UnsupportedOption, match="from one cell range.*the caller limits a range to 50"):
            mabu.run(case["ini3"], case["absorbed"], out, ResidentLibraryStandIn(10 ** 9), makelib=(case["lfreq"], NBINS), range_cells=50)
    finally:
        for dust in case["dusts"]:                                 # the libraries of the fixture, for the tests after this one
            with open(mabu.library_name(dust), "wb") as fp:
                fp.write(case["mlib"][dust])


def test_lookup_equals_the_composition_on_both_paths(case, tmp_path):
    from mabu_library_engine import ResidentLibraryStandIn, composition
    from soc_amd import mabu
    want, MISS = composition("soc", case["libs"], case["FABS"][:, REF], case["ABU"], case["RABS"][REF])
    out = str(tmp_path / "emitted.data")
    info = mabu.run(case["inilib"], case["abs3"], out, case["eng"])
    assert info["path"] == "host"
    assert list(np.fromfile(out, np.int32, 2)) == [case["CELLS"], NFREQ]
    got = np.asarray(files.mmap_emitted(out, case["CELLS"], NFREQ))
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(info["miss"], MISS)
    assert info["missed"] == [int(np.count_nonzero(MISS & (1 << i))) for i in range(3)]
    assert 0 < min(info["missed"]) and max(info["missed"]) < case["CELLS"]
    # the device branch, all cells at once and in ranges after a refusal
    for capacity, begun in ((10 ** 9, [case["CELLS"]]), (150, [150, 150, case["CELLS"] - 300])):
        st = ResidentLibraryStandIn(capacity)
        info = mabu.run(case["inilib"], case["abs3"], out, st)
        assert (info["path"], info["ranges"], st.lib_begun, st.lib_open) == ("device", len(begun), begun, False)
        assert np.array_equal(bits(np.asarray(files.mmap_emitted(out, case["CELLS"], NFREQ))), bits(want))
        assert np.array_equal(info["miss"], MISS)


def test_cells_that_represent_their_bin_in_every_dust_reproduce_their_direct_emission(case, tmp_path):
    """With 27000 bins for 392 cells many cells are the representative of their bin in all three libraries.  Where such a cell is
    found again by the look-up in every dust its row is, bit for bit, the sum of the rows the libraries stored for it: that dust's
    direct emission clipped to [1e-30, 1e30] as the library file holds it.  On every element where no dust's emission was clipped
    -- the emission of the cold dusts underflows 1e-30 towards the high frequencies; 10 of the 12 columns still come out equal,
    a clipped term vanishing in the sum -- that is the direct emission of the emitted file itself.  A representative the look-up does not find again has a share below the
    look-up's lower clamp region (the build clips at 1e-25, the look-up at 1e-29, as the reference does).  The deviation of the
    other cells is printed, not bounded."""
    import library_host
    from soc_amd import mabu
    out = str(tmp_path / "emitted.data")
    info = mabu.run(case["inilib"], case["abs3"], out, case["eng"])
    look = np.asarray(files.mmap_emitted(out, case["CELLS"], NFREQ))
    reps, low = None, np.zeros(case["CELLS"], bool)
    for i in range(3):
        part = mabu.split_absorbed(case["FABS"], case["RABS"], case["ABU"], i)[:, REF]
        IND = library_host.build("soc", NBINS, part)["IND"]
        own = np.zeros(case["CELLS"], bool)
        own[IND[IND >= 0]] = True
        reps = own if reps is None else reps & own
        low |= (part < np.float32(1e-25)).any(axis=1) | (part > np.float32(1.0)).any(axis=1)
    found = reps & (info["miss"] == 0)
    assert found.sum() >= 1 and (~reps).sum() >= 1
    assert low[reps & ~found].all()                                # only cells beyond the build's clip are not found again
    stored = np.zeros((case["CELLS"], NFREQ), np.float32)
    unclipped = np.ones((case["CELLS"], NFREQ), bool)
    for i in range(3):
        stored += np.clip(case["EMD"][i], np.float32(1e-30), np.float32(1e30)) * case["ABU"][:, i:i + 1]
        unclipped &= (case["EMD"][i] >= np.float32(1e-30)) & (case["EMD"][i] <= np.float32(1e30))
    assert np.array_equal(bits(look[found]), bits(stored[found]))
    same = bits(look) == bits(case["direct"])
    assert same[found][unclipped[found]].all() and unclipped[found].any(axis=1).all()
    print("%d of the %d elements of those rows equal the emitted file of the direct run bit for bit (%d had no dust clipped)"
          % (same[found].sum(), same[found].size, unclipped[found].sum()))
    others = np.flatnonzero(~reps & (case["cloud"].DENS > 0) & (info["miss"] == 0))
    rel = np.abs(look[others][:, :10] - case["direct"][others][:, :10]) / np.abs(case["direct"][others][:, :10])
    print("%d cells represent their bin in all dusts, %d of them are found again; %d other cells with an answer from every library: "
          "relative deviation from the direct solve median %.3e, maximum %.3e" % (reps.sum(), found.sum(), len(others), np.median(rel), rel.max()))


def test_ofreq_selects_and_orders_the_columns(case, tmp_path):
    from soc_amd import mabu
    full, sub = str(tmp_path / "full.data"), str(tmp_path / "sub.data")
    mabu.run(case["inilib"], case["abs3"], full, case["eng"])
    ofreq = str(tmp_path / "ofreq.dat")
    np.savetxt(ofreq, case["FREQ"][[7, 1, 4]] * 1.01)              # (the nearest library frequency per line)
    mabu.run(case["inilib"], case["abs3"], sub, case["eng"], ofreq=ofreq)
    assert list(np.fromfile(sub, np.int32, 2)) == [case["CELLS"], 3]
    a = np.asarray(files.mmap_emitted(full, case["CELLS"], NFREQ))
    b = np.asarray(files.mmap_emitted(sub, case["CELLS"], 3))
    assert np.array_equal(bits(b), bits(a[:, [7, 1, 4]])) and (b > 0).any()


def test_misses_are_counted_per_dust(case, capsys):
    """coarse libraries (3 bins per axis: every window of the grid holds cells) built from the cells themselves answer for every
    cell; the library of one dust shifted by two bins on axis 1, as the case all_miss of tests/library_cases.py, for none"""
    import library_cases
    from soc_amd import mabu
    n = 200
    rng = library_cases._rng("mabu_library_misses")
    ABS3 = library_cases._cloud(rng, n)
    ABU = (0.2 + rng.random((n, 3))).astype(np.float32)
    libs = []
    for i in range(3):
        part = mabu.split_absorbed(ABS3, case["RABS"][REF], ABU, i)
        lib = case["eng"].library_build(3, ABS3=part)
        lib["E"] = np.where((lib["IND"] >= 0)[:, None], np.float32(1e-10 * (i + 1)), np.float32(1e32)) * np.ones((1, NFREQ), np.float32)
        libs.append(lib)
    EM, info = mabu.solve_emission_library(case["eng"], case["dusts"], case["kinds"], ABS3, ABU, libs, REF)
    assert info["missed"] == [0, 0, 0] and (EM > 0).all()
    libs[1] = dict(libs[1], Y=(libs[1]["Y"] + np.float32(2.0)).astype(np.float32))
    EM2, info = mabu.solve_emission_library(case["eng"], case["dusts"], case["kinds"], ABS3, ABU, libs, REF)
    assert info["missed"] == [0, n, 0]
    assert np.array_equal(info["miss"], np.full(n, 2, np.uint32))
    want = np.float32(1e-10) * ABU[:, 0:1] + np.float32(3e-10) * ABU[:, 2:3]       # the missed dust adds zero
    assert np.array_equal(bits(EM2), bits(want * np.ones((1, NFREQ), np.float32)))
    mabu.print_misses(case["dusts"], info, n, False)
    text = capsys.readouterr().out
    assert "gs_pah.dust: %d cells without answer in the library" % n in text and "sil.dust: all cells matched" in text


def test_uselib_solves_the_cells_with_a_miss_directly(case, tmp_path):
    from mabu_library_engine import composition
    from soc_amd import mabu
    out = str(tmp_path / "emitted.data")
    info = mabu.run(case["ini3"], case["absorbed"], out, case["eng"], uselib=case["lfreq"])
    got = np.asarray(files.mmap_emitted(out, case["CELLS"], NFREQ))
    want, MISS = composition("soc", case["libs"], case["FABS"][:, REF], case["ABU"], case["RABS"][REF])
    missed = MISS != 0
    assert np.array_equal(info["solved"], np.flatnonzero(missed)) and 0 < missed.sum() < case["CELLS"]
    assert np.array_equal(bits(got[missed]), bits(case["direct"][missed]))         # the direct solve of the same run
    assert np.array_equal(bits(got[~missed]), bits(want[~missed]))


class TwoRanks:
    rank, world = 0, 2


def test_refusals_name_their_reason(case, tmp_path):
    from soc_amd import driver, mabu
    from soc_amd.asoc import UnsupportedOption
    d, eng = case["d"], case["eng"]
    out = str(tmp_path / "refused.data")
    lib = "libabs %s\n" % case["lfreq"]
    np.zeros(case["CELLS"], np.float32).tofile(str(tmp_path / "a.aalg"))
    for extra, reason in (("iterations 2\ncellpackets 1000\n", "iterations > 0 with cellpackets"),
                          ("polarisation %s/sil.dust %s/a.aalg\n" % (d, tmp_path), "polarisation lines"),
                          ("saveint 1\n", "saveint"), ("nnmake x 10\n", "nnmake"), ("absthin 4\n", "absthin")):
        ini = write_ini(d, "refused.ini", three_optical(d), lib + extra)
        with pytest.raises(UnsupportedOption, match="libabs .a library run. together with.*" + reason):
            mabu.run(ini, case["abs3"], out, eng)
        with pytest.raises(UnsupportedOption, match="libabs .a library run. together with.*" + reason):
            driver.Pipeline(ini, eng, verbose=0)
    with pytest.raises(UnsupportedOption, match="more than one rank"):
        mabu.run(case["inilib"], case["abs3"], out, eng, TwoRanks())
    with pytest.raises(UnsupportedOption, match="more than one rank"):
        driver.Pipeline(case["inilib"], eng, TwoRanks(), verbose=0)
    ini = write_ini(d, "mapsonly.ini", three_optical(d), "libmaps %s\n" % case["lfreq"])
    for call in (lambda: mabu.run(ini, case["absorbed"], out, eng), lambda: driver.Pipeline(ini, eng, verbose=0)):
        with pytest.raises(UnsupportedOption, match="libmaps without libabs"):
            call()
    with pytest.raises(UnsupportedOption, match="fourth argument .*not supported for a direct run"):
        mabu.run(case["ini3"], case["absorbed"], out, eng, ofreq=case["lfreq"])
    with pytest.raises(UnsupportedOption, match="makelib with 2 ranks"):
        mabu.run(case["ini3"], case["absorbed"], out, eng, TwoRanks(), makelib=(case["lfreq"], NBINS))
    with pytest.raises(UnsupportedOption, match="makelib in a library run"):
        driver.Pipeline(case["inilib"], eng, verbose=0, makelib=(case["lfreq"], NBINS))
    ini = write_ini(d, "reemit.ini", three_optical(d), "iterations 2\ncellpackets 1000\n")
    with pytest.raises(UnsupportedOption, match="makelib with dust re-emission iterations"):
        driver.Pipeline(ini, eng, verbose=0, makelib=(case["lfreq"], NBINS))
    many = [case["dusts"][0]] * 33                                 # the miss mask has 32 bits
    with pytest.raises(UnsupportedOption, match="33 dusts: a library run takes at most 32"):
        mabu.solve_emission_library(eng, many, ['eqdust'] * 33, np.ones((4, 3), np.float32), np.ones((4, 33), np.float32), case["libs"][:1] * 33, REF)
    # a missing library names the file and the command that writes it
    hidden = mabu.library_name(case["dusts"][2]) + ".hidden"
    os.replace(mabu.library_name(case["dusts"][2]), hidden)
    try:
        for call in (lambda: mabu.run(case["inilib"], case["abs3"], out, eng), lambda: driver.Pipeline(case["inilib"], eng, verbose=0)):
            with pytest.raises(FileNotFoundError, match=r"carb\.mlib: the library of .*carb\.dust is missing.*python -m soc_amd\.mabu .* --makelib"):
                call()
    finally:
        os.replace(hidden, mabu.library_name(case["dusts"][2]))
    assert not os.path.exists(out)
    assert mabu.main(["mabu", "a.ini", "b", "c", "--makelib", "lfreq.dat", "--bins", "1"]) == 1      # 2 <= N <= 64
    assert mabu.main(["mabu", "a.ini", "b", "c", "--bins"]) == 1


def run_asoc(ini, engine):
    from soc_amd.asoc import AbsorptionRun
    from soc_amd.ini import User
    AbsorptionRun(User(ini), engine, verbose=0).run()


def test_driver_library_run_equals_the_three_programs_chained_through_files(tmp_path):
    """`libabs` + `libmaps` in the ini of soc_amd.driver against soc_amd.asoc (libabs) -> soc_amd.mabu (ofreq) -> soc_amd.asoc (libmaps)"""
    from mabu_library_engine import MabuLibraryEngine
    from soc_amd import driver, mabu
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, sol, abu = write_case(d, cloud)
    write_third_dust(d, cloud.CELLS)
    for name in ("bg.bin", "ps.bin"):                              # (absorptions below 1: see the module's docstring)
        (np.fromfile(os.path.join(d, name), np.float32) * SCALE).tofile(os.path.join(d, name))
    FREQ = np.asarray(sol["FREQ"], np.float64)
    lfreq, mfreq = os.path.join(d, "lfreq.dat"), os.path.join(d, "mfreq.dat")
    np.savetxt(lfreq, FREQ[REF])
    np.savetxt(mfreq, FREQ[[3, 5, 8]])
    with open(ini) as fp:
        tail = "".join(line for line in fp if line.split()[0] not in ("optical", "absorbed", "emitted"))

    def write(name, simple, extra, absorbed="abs.data", emitted="emitted.data"):
        path = os.path.join(d, name)
        with open(path, "w") as fp:
            fp.write("".join("optical %s\n" % o for o in three_optical(d, simple)) + tail + extra
                     + "absorbed %s/%s\nemitted %s/%s\n" % (d, absorbed, d, emitted))
        return path
    for sub in ("full", "drv", "chain"):
        os.makedirs(os.path.join(d, sub))
    eng = MabuLibraryEngine("soc")
    # the libraries: a by-product of the full run, whose emitted file does not change
    os.chdir(os.path.join(d, "full"))
    full = write("full.ini", False, "nomap\n", emitted="emitted_full.data")
    driver.Pipeline(full, eng, verbose=0).run()
    first = open(os.path.join(d, "emitted_full.data"), "rb").read()
    P = driver.Pipeline(full, eng, verbose=0, makelib=(lfreq, NBINS))
    P.run()
    assert open(os.path.join(d, "emitted_full.data"), "rb").read() == first
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    assert all(os.path.exists(mabu.library_name(x)) for x in dusts)
    # the driver
    os.chdir(os.path.join(d, "drv"))
    P = driver.Pipeline(write("lib.ini", False, "libabs %s\nlibmaps %s\n" % (lfreq, mfreq), "abs_drv.data", "emitted_drv.data"), eng, verbose=0)
    CTABS, ABS3, EM = P.run(keep_files=True)
    assert ABS3.shape == (cloud.CELLS, 3) and EM.shape == (cloud.CELLS, 3) and P.timers["emission_path"] == "host"
    assert (EM > 0).any() and max(P.timers["missed"]) < cloud.CELLS
    drv_map = open("map_dir_00.bin", "rb").read()
    assert len(drv_map) == 8 + 4 * 64 * 3
    # the chain through files
    os.chdir(os.path.join(d, "chain"))
    run_asoc(write("rt.ini", True, "libabs %s\nnomap\nnosolve\n" % lfreq, "abs_chain.data", "unused.data"), eng)
    with open(os.path.join(d, "abs_chain.data"), "rb") as a, open(os.path.join(d, "abs_drv.data"), "rb") as b:
        assert a.read() == b.read()
    mabu.run(write("mabu.ini", False, "libabs %s\n" % lfreq), os.path.join(d, "abs_chain.data"), os.path.join(d, "emitted_chain.data"), eng, ofreq=mfreq)
    with open(os.path.join(d, "emitted_chain.data"), "rb") as a, open(os.path.join(d, "emitted_drv.data"), "rb") as b:
        assert a.read() == b.read()
    run_asoc(write("maps.ini", True, "libmaps %s\n" % mfreq, "unused.data", "emitted_drv.data"), eng)      # from the file the driver wrote
    assert open("map_dir_00.bin", "rb").read() == drv_map
    assert np.fromfile("map_dir_00.bin", np.float32)[2:].max() > 0
    # without libmaps the library run maps every frequency
    os.chdir(os.path.join(d, "drv"))
    P = driver.Pipeline(write("liball.ini", False, "libabs %s\n" % lfreq, "abs_drv2.data", "emitted_drv2.data"), eng, verbose=0)
    _, _, EM = P.run()
    assert EM.shape == (cloud.CELLS, NFREQ) and os.path.getsize("map_dir_00.bin") == 8 + 4 * 64 * NFREQ
