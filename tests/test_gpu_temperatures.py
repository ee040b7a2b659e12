"""Dust temperatures and enthalpy-level populations from the device (soc_a2e_dosolve_kernel<C, POL, DUMP>, soc_a2e_eqsizes_kernel<POL,
KEEP>, soc_a2e_solve_dump, soc_a2e_resident_solve_dump, soc_a2e_resident_keep_teq / _download_teq, soc_mabu_download_t): the
populations against the fp32 restatement tests/a2e_rows.py::find_rows at every launch shape, the temperatures against the kernels that
already return them (a2e_eqtemp, eqsolver), the emission against the calls without the new outputs -- all on bits --, the pipeline
with `temperatures` end to end, and the handle after the new buffers are released."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import a2e_rows as R                                  # noqa: E402
import aalg_cases as ac                               # noqa: E402
import temperature_engine as te                       # noqa: E402
from soc_amd import a2e, mabu, synth                  # noqa: E402
from soc_amd.lib import SocError                      # noqa: E402

pytestmark = pytest.mark.gpu

NFREQ_EQ, NSIZE, SKIPPED = 13, 5, 3


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def set_size(engine, NE, isize, NFREQ=50):
    sol, AF = R.solver(NE, NFREQ)
    engine.a2e_set_size(NE, NFREQ, sol["sizes"][isize], AF[isize])
    return sol["sizes"][isize], AF[isize]


# ---- DoSolve populations ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NE", [3, 70, 143, 202])
def test_populations_at_every_launch_shape(engine, NE):
    """C = 4 without a suffix-sum column, C = 4 with 256 threads and two row blocks, the first C = 2, the first C = 1; 4*C + 3 cells:
    the last workgroup partly filled, a zero row, the k grid up to K_TOP"""
    C = R.TABLE[NE][0]
    ABS, _ = R.absorptions(NE, 50, C)
    for isize in range(2):
        set_size(engine, NE, isize)
        assert engine.a2e_launch_shape()[:2] == R.TABLE[NE]
        plain = engine.a2e_solve(ABS)
        emit, X = engine.a2e_solve_dump(ABS)
        want = te.clamp(R.case_rows(NE, 50, C, isize)[2])
        assert X.shape == (4 * C + 3, NE) and np.isfinite(want).all()
        assert same_bits(X, want), (NE, isize, np.argwhere(bits(X) != bits(want))[:8])
        assert same_bits(emit, plain)
        assert (X >= np.float32(1.0e-35)).all() and (X <= 10.0).all() and (X > np.float32(1.0e-35)).any()


@pytest.mark.parametrize("NE", sorted(R.RESIDENT))
def test_populations_on_the_resident_route(engine, NE):
    """8*C + 5 cells, two sizes added to the sum: X of either size, and the sum with the bits of the plain resident solve"""
    C = R.RESIDENT[NE]
    ABS = R.resident_absorptions(NE)
    sums = {}
    for dump in (False, True):
        engine.a2e_resident_begin(ABS.shape[0], 50)
        try:
            engine.a2e_resident_upload(0, ABS[:5])
            engine.a2e_resident_upload(5, ABS[5:])
            for isize in range(2):
                size, AF = set_size(engine, NE, isize)
                assert engine.a2e_launch_shape()[0] == C
                if dump:
                    X = engine.a2e_resident_solve_dump()
                    want = te.populations(NE, 50, size, AF, ABS)
                    assert same_bits(X, want), (NE, isize, np.argwhere(bits(X) != bits(want))[:8])
                else:
                    engine.a2e_resident_solve()
            sums[dump] = engine.a2e_resident_download(0, ABS.shape[0])
        finally:
            engine.a2e_resident_end()
    assert np.isfinite(sums[False]).all() and (sums[False] > 0).any() and same_bits(sums[True], sums[False])


def test_populations_of_more_than_one_chunk(engine):
    """65536 + 77 cells at NE = 3: the populations come back in two chunks through one device plane"""
    NE, n = 3, 65536 + 77
    base = R.absorptions(NE, 50, 4)[0]
    ABS = np.ascontiguousarray(base[np.arange(n) % 17] * np.linspace(0.5, 2.0, n, dtype=np.float32)[:, None], np.float32)
    sums = {}
    for dump in (False, True):
        engine.a2e_resident_begin(n, 50)
        try:
            engine.a2e_resident_upload(0, ABS)
            size, AF = set_size(engine, NE, 1)
            if dump:
                X = engine.a2e_resident_solve_dump(out=np.full((n, NE), np.nan, np.float32))
                assert same_bits(X, te.populations(NE, 50, size, AF, ABS))
            else:
                engine.a2e_resident_solve()
            sums[dump] = engine.a2e_resident_download(0, n)
        finally:
            engine.a2e_resident_end()
    assert same_bits(sums[True], sums[False]) and (sums[False] > 0).any()


def eq_solver(n):
    sol = synth.synth_solver(NFREQ=NFREQ_EQ, NE=16, NSIZE=NSIZE, seed=11)
    if n <= 2:
        sol["S_FRAC"][SKIPPED] = np.float32(1.0e-31)
    return sol


def eq_absorptions(cells):
    ABS = (np.random.default_rng(3 + cells).lognormal(0, 1, (cells, NFREQ_EQ)) * 1e-3).astype(np.float32)
    ABS[cells // 2] = 0.0
    ABS[(2 * cells) // 3] *= np.float32(1.0e12)
    return ABS


def test_polarised_run_with_the_dump(engine, tmp_path):
    """POL + DUMP: NE 16, 65 cells, aalg through every arm of every size; X, the emission and the polarised emission as without"""
    sol, ABS = eq_solver(999), eq_absorptions(65)
    aalg = ac.edge_aalg(sol["SIZE_A"], 65)
    E0, P0, _ = a2e.run(engine, sol, ABS, aalg=aalg, verbose=False)
    prefix = os.path.join(str(tmp_path), "pah")
    E1, P1, _ = a2e.run(engine, sol, ABS, aalg=aalg, verbose=False, dump=prefix)
    assert same_bits(E0, E1) and same_bits(P0, P1) and (P0 > 0).any() and (P0 < E0).any()
    batched = os.path.join(str(tmp_path), "batched")
    E2, _ = a2e.run(ac.Batches(engine), sol, ABS, verbose=False, dump=batched)
    assert same_bits(E2, E0)
    for isize in range(NSIZE):
        hdr = np.fromfile(a2e.dump_name(prefix, isize), np.int32, 2)
        X = np.fromfile(a2e.dump_name(prefix, isize), np.float32, offset=8).reshape(65, 16)
        assert list(hdr) == [65, 16]
        assert same_bits(X, te.populations(16, NFREQ_EQ, sol["sizes"][isize], synth.a2e_absorption_fraction(sol, isize), ac.clipped(ABS)))
        with open(a2e.dump_name(prefix, isize), "rb") as a, open(a2e.dump_name(batched, isize), "rb") as b:
            assert a.read() == b.read()                                  # the resident and the batched route: the same file


# ---- equilibrium sizes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 2])
@pytest.mark.parametrize("cells", [1, 63, 65, 1000])
def test_temperatures_of_the_equilibrium_sizes(engine, cells, n):
    sol, ABS = eq_solver(n), ac.clipped(eq_absorptions(cells))
    sizes = a2e.eq_sizes(sol, n)
    assert sizes == ([0, 1, 2, 4] if n == 0 else [2, 4])
    sums = {}
    for keep in (False, True):
        engine.a2e_resident_begin(cells, NFREQ_EQ)
        try:
            engine.a2e_resident_upload(0, ABS)
            engine.a2e_set_eq_sizes(*a2e.eq_size_tables(sol, sizes))
            if keep:
                engine.a2e_resident_keep_teq(True)
            engine.a2e_resident_solve_eq()
            sums[keep] = engine.a2e_resident_download(0, cells)
            if not keep:
                with pytest.raises(SocError, match="no temperatures are kept"):
                    engine.a2e_resident_download_teq(0, 0, cells)
                continue
            for slot, isize in enumerate(sizes):
                Emin, kE, oplgkE, TTT, KABS = a2e.eq_table(sol, isize)
                want, _ = engine.a2e_eqtemp(0, cells, a2e.NIP, a2e.FACTOR, kE, oplgkE, Emin, sol["FREQ"], KABS, TTT,
                                            np.asarray(ABS * synth.a2e_absorption_fraction(sol, isize), np.float32))
                T = engine.a2e_resident_download_teq(slot, 0, cells)
                assert T.shape == (cells,) and (want > 0).all()
                assert same_bits(T, want), (cells, n, isize, np.flatnonzero(bits(T) != bits(want))[:8])
                if cells > 2:
                    assert same_bits(engine.a2e_resident_download_teq(slot, 1, cells - 2, out=np.zeros(cells - 2, np.float32)), want[1:-1])
            with pytest.raises(SocError, match="size %d of %d" % (len(sizes), len(sizes))):
                engine.a2e_resident_download_teq(len(sizes), 0, cells)
            with pytest.raises(SocError, match=r"cells \[1, %d\) of %d" % (cells + 1, cells)):
                engine.a2e_resident_download_teq(0, 1, cells)
        finally:
            engine.a2e_resident_end()
    assert same_bits(sums[True], sums[False]) and np.isfinite(sums[False]).all() and (sums[False] > 0).any()


# ---- the multi-dust stage and the pipeline --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory, engine):
    """the case of tests/test_driver.py (392 cells, an equilibrium dust with abundances and a stochastically heated one, here with
    `nstoch 1`: its second size an equilibrium size) through the pipeline on the GPU with `temperatures`, and once more without on
    the same INT tallies (tests/test_gpu_eqsizes.py: two runs do not tally the same bits on the GPU)"""
    from soc_amd import driver
    from test_driver import write_case
    from test_gpu_eqsizes import RecordingTallies, ReplayingTallies
    top = str(tmp_path_factory.mktemp("gputemperatures"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    recorder = RecordingTallies(engine)
    replayer = ReplayingTallies(engine, recorder.tallies)
    out = dict(cloud=cloud)
    for tag, eng, kw in (("with", recorder, dict(temperatures=True)), ("without", replayer, dict(absorbed_source='host'))):
        d = os.path.join(top, tag)
        os.makedirs(d)
        ini, sol, abu = write_case(d, cloud)
        with open(os.path.join(d, "gs_pah.dust"), "w") as fp:
            fp.write("gsetdust\nnstoch 1\n")
        cwd = os.getcwd()
        os.chdir(d)
        try:
            P = driver.Pipeline(ini, eng, verbose=0, **kw)
            CTABS, FABS, EMITTED = P.run(keep_files=True)
        finally:
            os.chdir(cwd)
            engine.set_exec(-1, 4)
        out[tag] = dict(d=d, ini=ini, timers=dict(P.timers), FABS=FABS, EMITTED=EMITTED, T=P.T,
                        files={f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))
                               if f.endswith((".T", ".dump", ".bin")) or f == "emitted.data"})
    out["ABU"] = np.stack([abu, np.ones(cloud.CELLS, np.float32)], axis=1)
    out["tallies"] = (len(recorder.tallies), replayer.used)
    return out


def test_pipeline_with_temperatures_end_to_end(engine, model):
    w, wo, CELLS = model["with"], model["without"], model["cloud"].CELLS
    assert w["timers"]["emission_path"] == "device" and w["timers"]["absorbed_source"] == "resident"     # the option takes nothing off the device
    assert wo["timers"]["emission_path"] == "device" and wo["T"] is None
    assert model["tallies"][0] == model["tallies"][1] > 0
    names = ["pah_size001.dump", "sil.dust.T"]
    assert [f for f in w["files"] if f.endswith((".T", ".dump"))] == names
    assert not [f for f in wo["files"] if f.endswith((".T", ".dump"))]
    # emitted file and maps: unchanged against the run without the option
    for f in ("emitted.data", "map_dir_00.bin"):
        assert w["files"][f] == wo["files"][f], f
    assert np.fromfile(os.path.join(w["d"], "map_dir_00.bin"), np.float32)[2:].max() > 0
    # the files against the host path of the program on the absorbed file the pipeline kept
    d = w["d"]
    assert list(np.frombuffer(w["files"]["pah_size001.dump"][:8], np.int32)) == [CELLS, 1] and len(w["files"]["sil.dust.T"]) == 4 * CELLS
    for f in names:
        os.remove(os.path.join(d, f))
    info = mabu.run(w["ini"], os.path.join(d, "abs.data"), os.path.join(d, "emitted_host.data"), engine, temperatures=True, path='host')
    assert info["path"] == "host"
    for f in names:
        with open(os.path.join(d, f), "rb") as fp:
            assert fp.read() == w["files"][f], f
    with open(os.path.join(d, "emitted_host.data"), "rb") as fp:
        assert fp.read() == w["files"]["emitted.data"]


def test_mabu_download_t_equals_eqsolver_in_two_ranges(engine, model):
    w, CELLS = model["with"], model["cloud"].CELLS
    dusts = [os.path.join(w["d"], "sil.dust"), os.path.join(w["d"], "gs_pah.dust")]
    kinds = [mabu.dust_kind(x) for x in dusts]
    plain, _ = mabu.solve_emission(engine, dusts, kinds, w["FABS"], model["ABU"])
    dev, di = mabu.solve_emission(engine, dusts, kinds, w["FABS"], model["ABU"], temperatures=True, range_cells=200)
    assert (di["path"], di["ranges"]) == ("device", 2) and same_bits(dev, plain)
    RABS, _ = mabu.relative_cross_sections(dusts, kinds)
    Fq, KABS, Emin, kE, oplgkE, TTT = mabu.eq_dust_table(dusts[0])
    want, _ = engine.eqsolver(0, CELLS, mabu.NE_EQ, mabu.FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT, mabu.split_absorbed(w["FABS"], RABS, model["ABU"], 0))
    T = di["T"]
    assert same_bits(T[0], want) and len(np.unique(T[0])) > 100
    assert same_bits(T[0], w["T"][0]) and sorted(T[1]) == [1] and same_bits(T[1][1], w["T"][1][1])      # what the pipeline kept
    host, hi = mabu.solve_emission(engine, dusts, kinds, w["FABS"], model["ABU"], temperatures=True, path='host')
    assert hi["path"] == "host" and same_bits(host, dev) and same_bits(hi["T"][0], T[0]) and same_bits(hi["T"][1][1], T[1][1])


# ---- lifecycle --------------------------------------------------------------------------------------------------------
def test_a_plain_solve_after_the_new_buffers_are_released(engine):
    NE, C = 70, 4
    ABS, _ = R.absorptions(NE, 50, C)
    set_size(engine, NE, 0)
    plain = engine.a2e_solve(ABS)
    n = ABS.shape[0]

    def resident(dump):
        engine.a2e_resident_begin(n, 50)
        try:
            engine.a2e_resident_upload(0, ABS)
            engine.a2e_resident_solve_dump() if dump else engine.a2e_resident_solve()
            return engine.a2e_resident_download(0, n)
        finally:
            engine.a2e_resident_end()

    first = resident(True)
    assert same_bits(first, plain) and same_bits(resident(False), plain)           # no stale pointer to the freed plane
    assert same_bits(engine.a2e_solve_dump(ABS)[0], plain) and same_bits(engine.a2e_solve(ABS), plain)
    with pytest.raises(SocError, match="resident_begin"):
        engine.a2e_resident_keep_teq(True)
    with pytest.raises(SocError, match="no temperatures are kept"):
        engine.a2e_resident_download_teq(0, 0, 1)
    with pytest.raises(SocError, match="mabu_begin first"):
        engine.mabu_download_t(0, 1)
    engine.mabu_begin(10, 50, 1)
    try:
        with pytest.raises(SocError, match="no soc_mabu_solve_eq since soc_mabu_begin"):
            engine.mabu_download_t(0, 10)
        with pytest.raises(SocError, match=r"shape \(10,\)"):
            engine.mabu_download_t(0, 10, out=np.zeros(9, np.float32))
    finally:
        engine.mabu_end()
    # the switch goes with the block: a solve in the next block keeps nothing
    sol = eq_solver(0)
    EQ = ac.clipped(eq_absorptions(65))
    for keep in (True, False):
        engine.a2e_resident_begin(65, NFREQ_EQ)
        try:
            engine.a2e_resident_upload(0, EQ)
            engine.a2e_set_eq_sizes(*a2e.eq_size_tables(sol, [0, 4]))
            if keep:
                engine.a2e_resident_keep_teq()
            engine.a2e_resident_solve_eq()
            if keep:
                assert (engine.a2e_resident_download_teq(1, 0, 65) > 0).all()
                kept = engine.a2e_resident_download(0, 65)
            else:
                with pytest.raises(SocError, match="no temperatures are kept"):
                    engine.a2e_resident_download_teq(1, 0, 65)
                assert same_bits(engine.a2e_resident_download(0, 65), kept)
        finally:
            engine.a2e_resident_end()
