"""Dust temperatures and enthalpy-level populations out of the emission stage, without a GPU: soc_amd.a2e.run(dump=...) (the files of
the reference's DUMP_TDUST=1: A2E.py:378-400, 506-522), soc_amd.mabu.solve_emission(temperatures=True) host path against device path,
the files of soc_amd.mabu and soc_amd.driver with `--temperatures` (A2E_MABU.py:551), the refusals, and that nothing is written
without the options.  The engines are those of tests/temperature_engine.py; every comparison is on bits."""
import glob
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import temperature_engine as te                       # noqa: E402
from soc_amd import a2e, driver, files, mabu, synth   # noqa: E402
from soc_amd.asoc import UnsupportedOption            # noqa: E402
from test_driver import NFREQ as CASE_NFREQ, write_case   # noqa: E402

NSIZE, NFREQ, NE, SKIPPED, CELLS = 5, 13, 16, 3, 37   # the five-size solver of tests/test_gpu_eqsizes.py


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def solver(n):
    """size 3 planted below 1e-30 where it is an equilibrium size (NSTOCH 0 and 2), as tests/test_gpu_eqsizes.py::solver"""
    sol = synth.synth_solver(NFREQ=NFREQ, NE=NE, NSIZE=NSIZE, seed=11)
    if n <= 2:
        sol["S_FRAC"][SKIPPED] = np.float32(1.0e-31)
    return sol


def absorptions(cells=CELLS):
    ABS = (np.random.default_rng(3 + cells).lognormal(0, 1, (cells, NFREQ)) * 1e-3).astype(np.float32)
    ABS[cells // 2] = 0.0
    ABS[(2 * cells) // 3] *= np.float32(1.0e12)
    return ABS


def read_dump(name):
    """(header, values) of a dump file, the size checked against the header"""
    hdr = np.fromfile(name, np.int32, 2)
    assert os.path.getsize(name) == 8 + 4 * int(hdr[0]) * int(hdr[1]), name
    return [int(hdr[0]), int(hdr[1])], np.fromfile(name, np.float32, offset=8).reshape(int(hdr[0]), int(hdr[1]))


def clipped(ABS):
    ABS = np.array(ABS, np.float32)
    ABS[:, -1] = np.clip(ABS[:, -1], 0.0, 0.2 * ABS[:, -2])
    return ABS


# ---- a2e.run(dump=...) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 2, 4, 999])
def test_a2e_dump_files_on_both_routes(tmp_path, n):
    sol, ABS = solver(n), absorptions()
    routes = {"resident": te.ResidentStandIn(), "batched": te.TemperatureEngine("soc"),
              "no_eq_call": te.Hide(te.ResidentStandIn(), "a2e_resident_solve_eq", "a2e_set_eq_sizes")}
    plain, _ = a2e.run(te.TemperatureEngine("soc"), sol, ABS, NSTOCH=n, batch=16, verbose=False)
    got = {}
    for tag, eng in routes.items():
        prefix = os.path.join(str(tmp_path), tag, "pah")
        os.makedirs(os.path.dirname(prefix))
        E0, _ = a2e.run(eng, sol, ABS, NSTOCH=n, batch=16, verbose=False)
        E1, _ = a2e.run(eng, sol, ABS, NSTOCH=n, batch=16, verbose=False, dump=prefix)
        assert same_bits(E0, E1), tag                                    # the emission does not notice the dump
        got[tag] = {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(prefix + "*"))}
    nst = min(n, NSIZE)
    want = ["pah_size%03d.dump" % i for i in range(NSIZE) if i < nst or i != SKIPPED or n > 2]
    if n <= 2:
        assert "pah_size%03d.dump" % SKIPPED not in got["resident"]      # A2E.py:465: `continue` before the file is opened
    for tag in routes:
        assert sorted(got[tag]) == want, (tag, sorted(got[tag]))
        assert got[tag] == got["resident"], tag                          # identical bytes on every route
    # contents: populations from the restatement, temperatures from the engine's own a2e_eqtemp
    eng = te.TemperatureEngine("soc")
    A = clipped(ABS)
    for isize in range(NSIZE):
        name = os.path.join(str(tmp_path), "resident", "pah_size%03d.dump" % isize)
        if os.path.basename(name) not in want:
            continue
        hdr, val = read_dump(name)
        AF = synth.a2e_absorption_fraction(sol, isize)
        if isize < nst:
            assert hdr == [CELLS, NE]
            X = te.populations(NE, NFREQ, sol["sizes"][isize], AF, A)
            assert same_bits(val, X) and val.min() >= np.float32(1.0e-35) and val.max() <= 10.0
            assert (np.abs(val[0].sum() - 1.0) < 1e-3)                   # (normalised populations)
        else:
            assert hdr == [CELLS, 1]
            Emin, kE, oplgkE, TTT, KABS = a2e.eq_table(sol, isize)
            T, _ = eng.a2e_eqtemp(0, CELLS, a2e.NIP, a2e.FACTOR, kE, oplgkE, Emin, sol["FREQ"], KABS, TTT, np.asarray(A * AF, np.float32))
            assert same_bits(val[:, 0], T) and (T > 0).all()
    assert same_bits(plain, E1)


def test_a2e_dump_with_aalg_leaves_both_emissions_alone(tmp_path):
    sol, ABS = solver(2), absorptions()
    aalg = np.asarray(sol["SIZE_A"][1] * np.random.default_rng(5).uniform(0.3, 3.0, CELLS), np.float32)
    for tag, eng in (("resident", te.ResidentStandIn()), ("batched", te.TemperatureEngine("soc"))):
        prefix = os.path.join(str(tmp_path), tag)
        E0, P0, _ = a2e.run(eng, sol, ABS, NSTOCH=2, batch=16, verbose=False, aalg=aalg)
        E1, P1, _ = a2e.run(eng, sol, ABS, NSTOCH=2, batch=16, verbose=False, aalg=aalg, dump=prefix)
        assert same_bits(E0, E1) and same_bits(P0, P1) and (P0 > 0).any()
        assert len(glob.glob(prefix + "_size*.dump")) == 4
    a, b = (open(os.path.join(str(tmp_path), t + "_size001.dump"), "rb").read() for t in ("resident", "batched"))
    assert a == b


def test_a2e_without_dump_writes_nothing(tmp_path):
    os.chdir(str(tmp_path))
    a2e.run(te.ResidentStandIn(), solver(2), absorptions(), NSTOCH=2, verbose=False)
    assert os.listdir(str(tmp_path)) == []


def test_a2e_program_switch_and_its_refusal(tmp_path):
    assert a2e.dump_prefix("dir/pah.solver", {"DUMP_TDUST": "1"}) == "dir/pah"       # A2E.py:108-117
    assert a2e.dump_prefix("dir/pah.solver", {"DUMP_TDUST": "0"}) is None
    assert a2e.dump_prefix("dir/pah.solver", {}) is None

    class TwoRanks:
        rank, world = 0, 2

    emitted = os.path.join(str(tmp_path), "emitted.data")
    with pytest.raises(a2e.DumpNeedsOneRank, match="DUMP_TDUST=1 with 2 ranks"):
        a2e.run_sharded(None, "pah.solver", "absorbed.data", emitted, comm=TwoRanks(), dump="pah")
    assert not os.path.exists(emitted)


# ---- mabu.solve_emission(temperatures=True) ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the case of tests/test_mabu.py: the two-dust pipeline of tests/test_driver.py on 392 cells, run once with keep_files and
    --temperatures; in nstoch/ the same dusts with `nstoch 1` in the gsetdust file (its second size an equilibrium size)"""
    d = str(tmp_path_factory.mktemp("temperatures"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, sol, abu = write_case(d, cloud)
    sub = os.path.join(d, "nstoch")
    os.makedirs(sub)
    synth.write_solver(os.path.join(sub, "pah.solver"), sol)
    with open(os.path.join(sub, "gs_pah.dust"), "w") as fp:
        fp.write("gsetdust\nnstoch 1\n")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        P = driver.Pipeline(ini, te.TemperatureEngine("soc"), verbose=0, temperatures=True)
        CTABS, FABS, EMITTED = P.run(keep_files=True)
    finally:
        os.chdir(cwd)
    ABU = np.stack([abu, np.ones(cloud.CELLS, np.float32)], axis=1)
    return dict(d=d, ini=ini, sol=sol, ABU=ABU, cloud=cloud, FABS=FABS, EMITTED=EMITTED, T=P.T,
                dusts=[os.path.join(d, "sil.dust"), os.path.join(d, "gs_pah.dust")],
                dusts_nstoch=[os.path.join(d, "sil.dust"), os.path.join(sub, "gs_pah.dust")])


def same_temperatures(A, B):
    assert len(A) == len(B)
    for a, b in zip(A, B):
        if isinstance(a, dict):
            assert isinstance(b, dict) and sorted(a) == sorted(b)
            assert all(same_bits(a[k], b[k]) for k in a)
        else:
            assert same_bits(a, b)
    return True


@pytest.mark.parametrize("which", ["dusts", "dusts_nstoch"])
def test_stage_temperatures_host_against_device(case, which):
    dusts, CELLS_ = case[which], case["cloud"].CELLS
    kinds = [mabu.dust_kind(x) for x in dusts]
    assert CELLS_ == 392 and kinds == ['eqdust', 'gsetdust']
    plain, _ = mabu.solve_emission(te.TemperatureEngine("soc"), dusts, kinds, case["FABS"], case["ABU"])
    host, hi = mabu.solve_emission(te.TemperatureEngine("soc"), dusts, kinds, case["FABS"], case["ABU"], temperatures=True)
    assert hi["path"] == "host" and same_bits(host, plain)
    T = hi["T"]
    assert isinstance(T[0], np.ndarray) and T[0].shape == (CELLS_,) and T[0].dtype == np.float32
    assert sorted(T[1]) == ([] if which == "dusts" else [1])                     # the equilibrium sizes only; none: an empty dict
    leaf = case["cloud"].DENS > 0
    assert np.isfinite(T[0]).all() and (T[0][leaf] > 0).all() and len(np.unique(T[0][leaf])) > 100
    assert (T[0][~leaf] == np.float32(2.7)).all() and (~leaf).any()              # (parent cells: Ein <= 0, kernel_eqsolver.c's 2.7 K)
    for rc, ranges in ((None, 1), (50, 8)):
        eng = te.ResidentStandIn()
        dev, di = mabu.solve_emission(eng, dusts, kinds, case["FABS"], case["ABU"], temperatures=True, range_cells=rc)
        assert (di["path"], di["ranges"]) == ("device", ranges) and not eng.open
        assert same_bits(dev, host)
        assert same_temperatures(di["T"], T)
        again, ai = mabu.solve_emission(te.ResidentStandIn(), dusts, kinds, case["FABS"], case["ABU"], range_cells=rc)
        assert "T" not in ai and same_bits(again, dev)                            # EM unchanged against a run without the option
    # the temperature of the equilibrium dust is the engine's own
    RABS, _ = mabu.relative_cross_sections(dusts, kinds)
    Fq, KABS, Emin, kE, oplgkE, TTT = mabu.eq_dust_table(dusts[0])
    want, _ = te.TemperatureEngine("soc").eqsolver(0, CELLS_, mabu.NE_EQ, mabu.FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT,
                                                   mabu.split_absorbed(case["FABS"], RABS, case["ABU"], 0))
    assert same_bits(T[0], want)


def test_device_path_without_the_calls_is_refused_by_name(case):
    from test_mabu import ResidentStandIn as Old
    kinds = ['eqdust', 'gsetdust']
    with pytest.raises(UnsupportedOption, match="mabu_download_t"):
        mabu.solve_emission(Old(10 ** 9), case["dusts"], kinds, case["FABS"], case["ABU"], temperatures=True)


# ---- the programs -----------------------------------------------------------------------------------------------------
def temperature_files(d):
    return sorted(f for f in os.listdir(d) if f.endswith(".T") or f.endswith(".dump"))


def program_files(d, ini, absorbed, sub):
    """the temperature files soc_amd.mabu --temperatures writes from an absorbed file, read and moved out of the way"""
    before = {f: open(os.path.join(d, f), "rb").read() for f in temperature_files(d)}
    for f in before:
        os.remove(os.path.join(d, f))
    out = os.path.join(d, "emitted_%s.data" % sub)
    mabu.run(ini, absorbed, out, te.TemperatureEngine("soc"), temperatures=True)
    after = {f: open(os.path.join(d, f), "rb").read() for f in temperature_files(d)}
    return before, after, out


def test_driver_files_equal_the_programs_on_the_kept_absorbed_file(case):
    d, CELLS_ = case["d"], case["cloud"].CELLS
    assert temperature_files(d) == ["sil.dust.T"]                                # (every size of the gsetdust is stochastically heated)
    raw = np.fromfile(os.path.join(d, "sil.dust.T"), np.float32)                 # A2E_MABU.py:551: no header
    assert raw.shape == (CELLS_,) and same_bits(raw, case["T"][0])
    before, after, out = program_files(d, case["ini"], os.path.join(d, "abs.data"), "program")
    assert before == after
    em = np.asarray(files.mmap_emitted(out, CELLS_, CASE_NFREQ))
    assert same_bits(em, case["EMITTED"])


def iteration_run(d, N, extra):
    from reemit_chain import iteration_case
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, _ = iteration_case(d, cloud, N, extra)
    with open(os.path.join(d, "gs_pah.dust"), "w") as fp:                        # the second size an equilibrium size: a .dump file too
        fp.write("gsetdust\nnstoch 1\n")
    os.chdir(d)
    P = driver.Pipeline(ini, te.TemperatureEngine("soc"), verbose=0, temperatures=True)
    P.run(keep_files=True)
    return P, ini, cloud


def test_driver_iterations_write_the_last_steps_temperatures(tmp_path):
    d = os.path.join(str(tmp_path), "it")
    P, ini, cloud = iteration_run(d, 2, "")
    assert len(P.timers["iterations"]) == 2 and temperature_files(d) == ["pah_size001.dump", "sil.dust.T"]
    hdr, T1 = read_dump(os.path.join(d, "pah_size001.dump"))
    assert hdr == [cloud.CELLS, 1] and same_bits(T1[:, 0], P.T[1][1])
    before, after, _ = program_files(d, ini, os.path.join(d, "abs.data"), "last")   # abs.data: the last step's absorbed file
    assert before == after


def test_driver_convergence_writes_the_stopping_steps_temperatures(tmp_path):
    d = os.path.join(str(tmp_path), "conv")
    P, ini, cloud = iteration_run(d, 4, "convergence 0.9\n")
    assert P.converged is not None and P.converged < 4 and len(P.timers["iterations"]) == P.converged
    before, after, _ = program_files(d, ini, os.path.join(d, "abs.data"), "stop")   # abs.data: the stopping step's absorbed file
    assert sorted(before) == ["pah_size001.dump", "sil.dust.T"] and before == after
    # ... and not those of a later step: one more iteration gives other temperatures
    d2 = os.path.join(str(tmp_path), "more")
    P2, _, _ = iteration_run(d2, P.converged + 1, "")
    assert not same_bits(P2.T[0], P.T[0])


def test_refusals_name_their_reason(case, tmp_path):
    d = case["d"]
    absorbed, out = os.path.join(d, "abs.data"), os.path.join(str(tmp_path), "emitted_refused.data")

    class TwoRanks:
        rank, world = 0, 2

    eng = te.TemperatureEngine("soc")
    with pytest.raises(UnsupportedOption, match="temperatures with 2 ranks"):
        mabu.run(case["ini"], absorbed, out, eng, TwoRanks(), temperatures=True)
    with pytest.raises(UnsupportedOption, match="temperatures with 2 ranks"):
        driver.Pipeline(case["ini"], eng, TwoRanks(), temperatures=True)
    with pytest.raises(UnsupportedOption, match=r"temperatures together with a library look-up \(uselib\)"):
        mabu.run(case["ini"], absorbed, out, eng, uselib=os.path.join(d, "lfreq.dat"), temperatures=True)
    sol = case["sol"]
    np.savetxt(os.path.join(d, "lfreq.dat"), np.asarray(sol["FREQ"], np.float64)[[2, 5, 9]])
    with open(case["ini"]) as fp:
        text = fp.read()
    libini = os.path.join(d, "lib.ini")
    with open(libini, "w") as fp:
        fp.write(text + "libabs %s/lfreq.dat\n" % d)
    with pytest.raises(UnsupportedOption, match=r"temperatures together with a library look-up \(libabs\)"):
        driver.Pipeline(libini, eng, temperatures=True)
    abs3 = os.path.join(str(tmp_path), "abs3.data")
    files.write_absorbed(abs3, np.zeros((case["cloud"].CELLS, 3), np.float32))
    with pytest.raises(UnsupportedOption, match=r"temperatures together with a library look-up \(libabs\)"):
        mabu.run(libini, abs3, out, eng, temperatures=True)
    assert not os.path.exists(out)


def test_without_the_option_no_temperature_file_appears(tmp_path):
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, _, _ = write_case(d, cloud)
    with open(os.path.join(d, "gs_pah.dust"), "w") as fp:
        fp.write("gsetdust\nnstoch 1\n")
    os.chdir(d)
    P = driver.Pipeline(ini, te.TemperatureEngine("soc"), verbose=0)
    P.run(keep_files=True)
    assert P.T is None
    info = mabu.run(ini, os.path.join(d, "abs.data"), os.path.join(d, "emitted_program.data"), te.TemperatureEngine("soc"))
    assert "T" not in info and temperature_files(d) == []
