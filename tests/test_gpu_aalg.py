"""Polarised emission of aligned grains on the device: the second, weighted accumulator in the epilogue of soc_a2e_dosolve_kernel at
every launch shape of the resident path, soc_amd.a2e.run resident against batches, the multi-dust stage with `polarisation` lines
device against host (one range and offset ranges), the two new streaming kernels on strided grids, the a2e program in a child
process, the pipeline end to end, and the refusals of the binding.  Every comparison is util.same_bits against the restatement of
tests/aalg_cases.py or against the other path: equal bits where finite, the same finite / non-finite pattern; no tolerance."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import a2e_rows as R                                 # noqa: E402
import aalg_cases as ac                              # noqa: E402
from soc_amd import a2e, files, mabu, synth          # noqa: E402
from soc_amd.lib import SocError                     # noqa: E402
from test_driver import NFREQ, write_case            # noqa: E402
from test_mabu import write_third_dust               # noqa: E402
from util import same_bits                           # noqa: E402

pytestmark = pytest.mark.gpu

CELLS = 3 * 256 + 77


@pytest.mark.parametrize("NE", sorted(R.RESIDENT))
def test_fused_epilogue_adds_the_weighted_emission_at_every_launch_shape(NE, engine):
    """4*C + 3 cells (the last workgroup is ragged), aalg through every arm of both sizes with neighbouring cells in different arms
    (weight 0, 1 and w inside a workgroup, the equalities with a size, a = 0), uploaded in two pieces that meet inside a workgroup"""
    sol, AF = R.solver(NE)
    ASIZE = np.asarray(sol["SIZE_A"], np.float32)
    engine.a2e_set_size(NE, 50, sol["sizes"][0], AF[0])
    C = engine.a2e_launch_shape()[0]
    assert C == R.RESIDENT[NE]
    ABS = R.absorptions(NE, 50, C)[0]
    n = 4 * C + 3
    assert ABS.shape[0] == n
    S0, S1 = ASIZE[:2]
    seven = np.asarray([0.0, S0, np.sqrt(np.float64(S0) * np.float64(S1)), S1, 2.0 * S1, np.nextafter(S0, np.float32(np.inf)),
                        0.75 * S0 + 0.25 * S1], np.float32)              # size 0: 1, 1 (=), w, 0 (= the next size), 0, w, w; size 1: 0 at 2 * S1
    aalg = seven[np.arange(n) % 7]
    W = [a2e.aalg_weight(ASIZE, isize, aalg) for isize in range(2)]
    assert ((W[0] > 0) & (W[0] < 1)).any() and (W[0] == 1).any() and (W[0] == 0).any() and set(np.unique(W[1])) == {0.0, 1.0}
    emits = []
    for isize in range(2):
        engine.a2e_set_size(NE, 50, sol["sizes"][isize], AF[isize])
        emits.append(engine.a2e_solve(ABS))
    want_p = ac.restated_pemitted(sol, aalg, emits, BATCH=5)
    assert np.isfinite(want_p).all() and (want_p > 0).any()

    def resident(polarised):
        engine.a2e_resident_begin(n, 50, polarised=polarised)
        try:
            engine.a2e_resident_upload(0, ABS)
            if polarised:
                engine.a2e_resident_upload_aalg(0, aalg[:C + 1])
                engine.a2e_resident_upload_aalg(C + 1, aalg[C + 1:])
            for isize in range(2):
                engine.a2e_set_size(NE, 50, sol["sizes"][isize], AF[isize])
                if polarised:
                    engine.a2e_set_size_aalg(ASIZE, isize)
                engine.a2e_resident_solve()
            s = engine.a2e_resident_download(0, n)
            if not polarised:
                return s, None, None, None
            p = engine.a2e_resident_download_p(0, n)
            engine.a2e_set_size(NE, 50, sol["sizes"][0], AF[0])              # a size without weights: the polarised sum stays
            engine.a2e_resident_solve()
            return s, p, engine.a2e_resident_download(0, n), engine.a2e_resident_download_p(0, n)
        finally:
            engine.a2e_resident_end()
    plain = resident(False)[0]
    s, p, s3, p3 = resident(True)
    assert same_bits(p, want_p), np.flatnonzero((p.view(np.uint32) != want_p.view(np.uint32)).any(axis=1))
    assert same_bits(s, plain) and same_bits(plain, emits[0] + emits[1])     # the plain sum is not disturbed
    assert np.array_equal(p3.view(np.uint32), p.view(np.uint32))
    assert same_bits(s3, s + emits[0]) and not np.array_equal(s3, s)


@pytest.mark.parametrize("IFREQ, NSTOCH", [(-1, 999), (2, 999), (-1, 2), (2, 2)])
def test_resident_path_equals_the_batches(engine, IFREQ, NSTOCH):
    """soc_amd.a2e.run with aalg: the cells resident (the kernel's accumulator) against batches (numpy on the per-size emission),
    all frequencies and one, and with the last size an equilibrium size (NSTOCH = NSIZE - 1)"""
    sol = synth.synth_solver(NFREQ=12, NE=16, NSIZE=3, seed=2)
    ABS = (np.random.default_rng(3).lognormal(0, 1, (301, 12)) * 1e-3).astype(np.float32)
    aalg = ac.edge_aalg(sol["SIZE_A"], 301)
    E1, P1, _ = a2e.run(engine, sol, ABS, NSTOCH, IFREQ, batch=128, verbose=False, aalg=aalg)
    E2, P2, _ = a2e.run(ac.Batches(engine), sol, ABS, NSTOCH, IFREQ, batch=128, verbose=False, aalg=aalg)
    assert P1.shape == (301, 1 if IFREQ >= 0 else 12)
    assert same_bits(E1, E2) and same_bits(P1, P2)
    want = ac.restated_pemitted(sol, aalg, ac.per_size_emissions(engine, sol, ac.clipped(ABS), NSTOCH), NSTOCH, IFREQ, BATCH=100)
    assert same_bits(P1, want) and (P1 > 0).any() and (P1 < E1).any()


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("gpuaalg"))
    write_case(d, synth.octree_cloud(6, levels=2, frac=0.1, seed=9))
    write_third_dust(d, CELLS)
    FABS, ABU, a_eq, a_st, sol = ac.stage_inputs(d, CELLS, NFREQ)
    pol = [ac.write_aalg(os.path.join(d, "sil.aalg"), a_eq), ac.write_aalg(os.path.join(d, "pah.aalg"), a_st), None]
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    return dict(d=d, FABS=FABS, ABU=ABU, a_eq=a_eq, a_st=a_st, sol=sol, pol=pol, dusts=dusts, kinds=[mabu.dust_kind(x) for x in dusts])


def test_stage_on_the_device_equals_the_host_path(engine, stage):
    """three dusts -- equilibrium with .rpol, stochastic with aalg, one without polarisation -- at 3*256+77 cells: one range, and
    three ranges of at most 300 cells (the rows of aalg offset); frequencies outside the .rpol columns on both sides, aalg outside the nodes on
    both sides and on nodes, rows whose total emission is 0"""
    s = stage
    raw = np.loadtxt(os.path.join(s["d"], "sil.rpol"))
    Fq = mabu.eq_dust_table(s["dusts"][0])[0]
    assert (Fq < raw[0, 1]).any() and (Fq > raw[0, -1]).any()
    assert (s["a_eq"] < raw[1, 0]).any() and (s["a_eq"] > raw[-1, 0]).any() and np.isin(raw[1:, 0], s["a_eq"].astype(np.float64)).all()
    with np.errstate(all="ignore"):
        host, hi = mabu.solve_emission(engine, s["dusts"], s["kinds"], s["FABS"], s["ABU"], path='host', pol=s["pol"])
    dev, di = mabu.solve_emission(engine, s["dusts"], s["kinds"], s["FABS"], s["ABU"], pol=s["pol"])
    many, mi = mabu.solve_emission(engine, s["dusts"], s["kinds"], s["FABS"], s["ABU"], range_cells=300, pol=s["pol"])
    assert (hi["path"], di["path"], di["ranges"], mi["ranges"]) == ("host", "device", 1, 3)
    assert (host == 0).any() and (hi["R"][host == 0] == 0).all()                    # 0 / (0 + 1e-32)
    ok = np.isfinite(hi["R"])
    assert ok.any() and (hi["R"][ok] > 0).any() and (hi["R"][ok] < 1).any()
    for got, info in ((dev, di), (many, mi)):
        assert same_bits(got, host) and same_bits(info["R"], hi["R"]), np.flatnonzero((info["R"].view(np.uint32) != hi["R"].view(np.uint32)).any(axis=1))[:8]
    plain, pi = mabu.solve_emission(engine, s["dusts"], s["kinds"], s["FABS"], s["ABU"])
    assert "R" not in pi and same_bits(plain, dev)


def test_streaming_kernels_on_strided_grids_equal_numpy_to_the_bit(engine, tmp_path):
    """45001 x 50: 2198 tiles of 1024 elements on 2048 workgroups, the array ends inside a float4 -- the equilibrium multiply and
    the final ratio against numpy"""
    cells, nfreq = 45001, 50
    rng = np.random.default_rng(cells)
    ABS = (rng.uniform(0.0, 1.0, (cells, nfreq)) * 10.0 ** rng.uniform(-12, 3, (cells, 1))).astype(np.float32)
    ABS[rng.uniform(size=cells) < 0.1] = np.float32(-1.0e20)
    ABU = rng.uniform(1.0e-3, 2.0, (cells, 1)).astype(np.float32)
    FREQ = np.logspace(11.5, 15.0, nfreq).astype(np.float32)
    KABS = (1.0e-22 * (FREQ / 1.0e13) ** 1.5).astype(np.float32)
    TTT = np.linspace(3.0, 1500.0, 200).astype(np.float32)
    apol = ac.synthetic_rpol(os.path.join(str(tmp_path), "x.rpol"), FREQ, 2.0e-7, 6.0e-5, NA=17)
    ap, tab = mabu.rpol_table(os.path.join(str(tmp_path), "x.dust"), FREQ)
    aalg = (10.0 ** rng.uniform(np.log10(apol[0]) - 0.3, np.log10(apol[-1]) + 0.3, cells)).astype(np.float32)
    aalg[::1000][:len(apol)] = apol
    engine.mabu_begin(cells, nfreq, 1, polarised=True)
    try:
        engine.mabu_upload(0, ABS)
        engine.mabu_set_tables(ABU, np.ones((nfreq, 1)))
        engine.mabu_split(0)
        engine.mabu_solve_eq(TTT.size, 1.0e20, 1.05, 1.0 / np.log10(1.05), 1.0e-12, FREQ, KABS, TTT)
        em = engine.a2e_resident_download(0, cells, out=np.zeros((cells, nfreq), np.float32))
        assert np.isfinite(em).all() and (em > 0).any() and (em == 0).any()
        engine.a2e_resident_upload_aalg(0, aalg[:20001])
        engine.a2e_resident_upload_aalg(20001, aalg[20001:])
        engine.mabu_pol_eq(ap, tab)
        pem = engine.a2e_resident_download_p(0, cells, out=np.zeros((cells, nfreq), np.float32))
        want = mabu.polarised_eq(em, aalg, ap, tab)
        assert same_bits(pem, want), np.flatnonzero((pem.view(np.uint32) != want.view(np.uint32)).any(axis=1))[:8]
        assert (pem > 0).any() and (pem[aalg > ap[-1]] == 0).all()
        engine.mabu_accumulate(0)
        engine.mabu_accumulate_p(0)
        total, psum = engine.mabu_download(0, cells), engine.mabu_download_p(0, cells)
        zero = np.zeros((cells, nfreq), np.float32)                              # the sums start from +0: -0 * ABU adds up to +0 (A2E_MABU.py:1137, :1145)
        assert same_bits(total, zero + em * ABU) and same_bits(psum, zero + want * ABU)
        engine.mabu_ratio()
        got = engine.mabu_download_p(0, cells)
        assert same_bits(got, mabu.reduction_factor(psum, total)) and (got[total == 0] == 0).all()
    finally:
        engine.mabu_end()


def test_a2e_program_in_a_child_process_writes_the_polarised_emission(engine, tmp_path):
    d = str(tmp_path)
    sol = synth.synth_solver(NFREQ=12, NE=16, NSIZE=3, seed=2)
    synth.write_solver(os.path.join(d, "x.solver"), sol)
    ABS = (np.random.default_rng(3).lognormal(0, 1, (301, 12)) * 1e-3).astype(np.float32)
    files.write_absorbed(os.path.join(d, "abs.bin"), ABS)
    aalg = ac.edge_aalg(sol["SIZE_A"], 301)
    ac.write_aalg(os.path.join(d, "x.aalg"), aalg)
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "soc_amd.a2e", "x.solver", "abs.bin", "em.bin", "0", "999", "-1", "x.aalg"],
                       env=env, cwd=d, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert list(np.fromfile(os.path.join(d, "em.bin.P"), np.int32, 2)) == [301, 12]
    P = np.fromfile(os.path.join(d, "em.bin.P"), np.float32)[2:].reshape(301, 12)
    want = ac.restated_pemitted(sol, aalg, ac.per_size_emissions(engine, sol, ac.clipped(ABS)))
    assert same_bits(P, want) and (P > 0).any()
    E, _ = a2e.run(engine, sol, ABS, verbose=False)
    assert same_bits(files.read_absorbed(os.path.join(d, "em.bin")), E)


def test_pipeline_makes_polarisation_maps_from_the_factor_in_memory(engine, tmp_path):
    """soc_amd.driver with `polarisation` lines and `polmap`, no `polred`: the maps are byte for byte those made with a `polred` file
    that holds {CELLS} and the column of R of the map's frequency.  (The transfer run sums Monte Carlo packets with atomic float
    additions, so two runs differ in their last bits: the maps of the file are made from the emission of the same run.)"""
    from soc_amd import driver
    from soc_amd.asoc import AbsorptionRun
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    IF = 5
    inis, sol = ac.driver_case(d, cloud, IF)
    try:
        os.chdir(os.path.join(d, "mem"))
        P = driver.Pipeline(inis["mem"], engine, verbose=0)
        CTABS, FABS, EMITTED = P.run(keep_files=True)
        assert P.timers["emission_path"] == "device" and P.R.shape == (cloud.CELLS, NFREQ)
        Rfile = np.fromfile(os.path.join(d, "emitted.data.R"), np.float32)
        assert int(Rfile[:1].view(np.int32)[0]) == cloud.CELLS and same_bits(Rfile[1:].reshape(cloud.CELLS, NFREQ), P.R)
        ac.write_aalg(os.path.join(d, "R.bin"), P.R[:, IF])                        # ({CELLS}, then the column)
        made = sorted(glob.glob("polmap_*.fits"))
        assert len(made) == 1
        os.chdir(os.path.join(d, "file"))
        P2 = driver.Pipeline(inis["file"], engine, verbose=0)
        rt = AbsorptionRun(P2.U, engine, verbose=0)
        rt.write_packet_info()
        rt.setup_engine()
        assert rt.write_polmaps(EMITTED, R=P.R * 0.5) == made                      # (with `polred` in the ini the file wins)
        for name in made:
            with open(os.path.join(d, "mem", name), "rb") as a, open(os.path.join(d, "file", name), "rb") as b:
                assert a.read() == b.read(), name
        leaf = cloud.DENS > 0
        assert np.isfinite(P.R[leaf]).all() and (P.R[leaf, IF] > 0).any() and (P.R[leaf, IF] < 1).any()
    finally:
        engine.set_exec(-1, 4)


def test_binding_refuses_what_was_not_asked_for_and_rows_outside(engine):
    engine.a2e_resident_begin(10, 4)
    try:
        with pytest.raises(SocError, match="polarised output was not asked for"):
            engine.a2e_resident_download_p(0, 5)
        with pytest.raises(SocError, match="polarised output was not asked for"):
            engine.a2e_resident_upload_aalg(0, np.ones(5, np.float32))
    finally:
        engine.a2e_resident_end()
    engine.a2e_resident_begin(10, 4, polarised=True)
    try:
        with pytest.raises(SocError, match=r"cells \[8, 12\) of 10"):
            engine.a2e_resident_upload_aalg(8, np.ones(4, np.float32))
        with pytest.raises(SocError, match=r"cells \[8, 12\) of 10"):
            engine.a2e_resident_download_p(8, 4)
        with pytest.raises(SocError, match="one value per cell"):
            engine.a2e_resident_upload_aalg(0, np.ones((2, 2), np.float32))
        assert (engine.a2e_resident_download_p(0, 10) == 0).all()
    finally:
        engine.a2e_resident_end()
    engine.mabu_begin(10, 4, 2)
    try:
        with pytest.raises(SocError, match="polarised output was not asked for"):
            engine.mabu_ratio()
        with pytest.raises(SocError, match="polarised output was not asked for"):
            engine.mabu_download_p(0, 5)
    finally:
        engine.mabu_end()
    engine.mabu_begin(10, 4, 2, polarised=True)
    try:
        with pytest.raises(SocError, match=r"apol\(3,\), tab\(3, 3\) for 4 frequencies"):
            engine.mabu_pol_eq(np.arange(3.0), np.zeros((3, 3)))
        with pytest.raises(SocError, match="must not decrease"):
            engine.mabu_pol_eq(np.asarray([1.0, 3.0, 2.0]), np.zeros((4, 3)))
    finally:
        engine.mabu_end()
