"""The library method for dust emission on the device (soc_library_*, soc_amd/csrc/soc_library.hip): the look-up and the build
against the soc-mode restatement (tests/csrc/library_host.c) to the bit, the resident variants against the host-array ones, and
the program soc_amd.library against its run on the CPU stand-in engine."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import library_cases as lc                             # noqa: E402
import library_host                                    # noqa: E402

pytestmark = pytest.mark.gpu

GRID = ("I0", "dI0", "I1", "dI1", "I2", "dI2")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(lc.SOLVE))
def test_lookup_equals_the_restatement_to_the_bit(engine, name):
    """N in {2, 3, 30}, NFREQ in {1, 7, 65}, n in {1, 63, 64, 65, 1000} (one workgroup is 256 cells: 1000 is four, the last
    partly filled), a permuted selection of columns, all misses, no miss, clamped indices on every axis, empty bins; the miss
    list included"""
    case = lc.solve_case(name)
    want, _, wmiss = library_host.solve("soc", case["lib"], case["ABS3"], ocol=case["ocol"])
    engine.library_set(case["lib"], case["ocol"])
    try:
        got, miss = engine.library_solve(case["ABS3"])
    finally:
        engine.library_set(None)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert np.array_equal(miss, wmiss)


def test_lookup_resident_equals_the_host_arrays(engine):
    """the reference columns read out of rows of 7 frequencies (columns 5, 0, 3), the emission left in the resident sum"""
    case = lc.solve_case("n30_f7_c1000")
    cols = np.asarray([5, 0, 3], np.int32)
    n = len(case["ABS3"])
    rows = np.random.Generator(np.random.PCG64(3)).random((n, 7)).astype(np.float32)
    rows[:, cols] = case["ABS3"]
    engine.library_set(case["lib"])
    try:
        want, wmiss = engine.library_solve(case["ABS3"])
        engine.a2e_resident_begin(n, 7)
        try:
            engine.a2e_resident_upload(0, rows[:300])
            engine.a2e_resident_upload(300, rows[300:])
            miss = engine.library_solve_resident(cols)
            got = engine.a2e_resident_download(0, n)
        finally:
            engine.a2e_resident_end()
    finally:
        engine.library_set(None)
    assert 0 < len(wmiss) < n
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(miss, wmiss)


def test_lookup_refusals(engine):
    from soc_amd.lib import SocError
    with pytest.raises(SocError, match="soc_library_set first"):
        engine.library_solve(np.ones((4, 3), np.float32))
    case = lc.solve_case("n3_f7_c63")
    with pytest.raises(SocError, match="ocol"):
        engine.library_set(case["lib"], [0, 7])
    engine.library_set(case["lib"])
    try:
        engine.a2e_resident_begin(10, 5)
        try:
            with pytest.raises(SocError, match="7 columns, a resident row holds 5"):
                engine.library_solve_resident([0, 1, 2])
        finally:
            engine.a2e_resident_end()
    finally:
        engine.library_set(None)


@pytest.mark.parametrize("name", sorted(lc.BUILD))
def test_build_equals_the_restatement(engine, name):
    """cells in {1, 2, 70, 5000} and 300 000 (1172 workgroups flush into the same table entries), the edge cases of
    tests/test_library.py: the tables bit for bit, IND exactly"""
    case = lc.build_case(name)
    want = library_host.build("soc", case["N"], case["ABS3"])
    got = engine.library_build(case["N"], ABS3=case["ABS3"])
    assert [k for k in GRID + ("X", "Y", "Z") if not np.array_equal(bits(got[k]), bits(want[k]))] == []
    assert np.array_equal(got["IND"], want["IND"])


def test_build_resident_equals_the_host_arrays(engine):
    case = lc.build_case("c5000")
    cols = np.asarray([4, 1, 2], np.int32)
    n = len(case["ABS3"])
    rows = np.random.Generator(np.random.PCG64(4)).random((n, 6)).astype(np.float32)
    rows[:, cols] = case["ABS3"]
    want = engine.library_build(case["N"], ABS3=case["ABS3"])
    engine.a2e_resident_begin(n, 6)
    try:
        engine.a2e_resident_upload(0, rows)
        got = engine.library_build(case["N"], cols=cols)
    finally:
        engine.a2e_resident_end()
    assert [k for k in GRID + ("X", "Y", "Z") if not np.array_equal(bits(got[k]), bits(want[k]))] == []
    assert np.array_equal(got["IND"], want["IND"]) and (got["IND"] >= 0).sum() > 20


def test_program_equals_its_run_on_the_cpu(tmp_path):
    """python -m soc_amd.library, build and solve, on the synthetic solver of the CPU round trip: the library files and the
    emitted files of the device run equal those of the stand-in engine (oracle A2E, restatement) bit for bit"""
    import library_roundtrip as rt
    from library_engine import LibraryEngine
    (tmp_path / "cpu").mkdir()
    (tmp_path / "gpu").mkdir()
    want = rt.run_program(tmp_path / "cpu", lambda: LibraryEngine("soc"))
    got = rt.run_program(tmp_path / "gpu")
    for k in ("first", "ofreq", "second", "three"):
        assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), k
    for k in ("lib", "new"):
        assert [t for t in GRID + ("X", "Y", "Z", "E", "FREQ") if not np.array_equal(bits(got[k][t]), bits(want[k][t]))] == [], k


def test_asoc_libabs_columns_are_those_of_the_full_run(engine, tmp_path):
    """python -m soc_amd.asoc's run with `libabs` on the smallest octree of the GPU ini tests, fixed seed: the absorbed file has a
    column per listed frequency, each that column of the run with all frequencies.  The same packets are simulated (the seed of
    a launch is a function of the frequency's index in the table), but a cell's tally is a sum of float atomics in the order the
    hardware takes them, so two runs agree to the rounding of that sum and not to the bit (on the CPU engine, which adds in
    work-item order, tests/test_library.py asks for the bits): the bound is the one tests/test_gpu_brick.py holds an absorbed
    file of this engine to against the oracle's."""
    from test_host import _write_model
    from soc_amd import files, synth
    from soc_amd.asoc import AbsorptionRun
    from soc_amd.ini import User
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    np.savetxt(os.path.join(d, "sel.txt"), [5.4e14, 4.0e14])
    os.chdir(d)
    try:
        AbsorptionRun(User(_write_model(d, cloud, with_ps=True, extra="absorbed %s/full.abs\n" % d)), engine, verbose=0).run()
        AbsorptionRun(User(_write_model(d, cloud, with_ps=True, extra="libabs %s/sel.txt\nabsorbed %s/lib.abs\n" % (d, d))), engine, verbose=0).run()
    finally:
        engine.set_features(0, 0, 0)
    full, lib = files.read_absorbed(os.path.join(d, "full.abs")), files.read_absorbed(os.path.join(d, "lib.abs"))
    assert full.shape == (cloud.CELLS, 3) and lib.shape == (cloud.CELLS, 2) and (full[cloud.DENS > 0] > 0).any(axis=0).all()
    leaf = cloud.DENS > 0                                             # (the other rows hold the marker -1e20 in every column)
    assert (lib[~leaf] == np.float32(-1.0e20)).all() and (full[~leaf] == np.float32(-1.0e20)).all()

    def close(a, b):
        return np.allclose(a[leaf], b[leaf], rtol=2e-5, atol=1e-6 * np.abs(b[leaf]).max())
    for col, f in ((0, 0), (1, 2)):
        print("column %d: largest relative difference %.3e, same bits: %s" % (
            col, float(np.max(np.abs(lib[leaf, col] - full[leaf, f]) / np.maximum(np.abs(full[leaf, f]), 1e-30))), np.array_equal(bits(lib[:, col]), bits(full[:, f]))))
        assert close(lib[:, col], full[:, f])
    assert not close(lib[:, 1], full[:, 1])                           # (and not the column of the frequency left out)
