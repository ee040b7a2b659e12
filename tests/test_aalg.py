"""Polarised emission of aligned grains without a GPU (the oracle-backed engine of the mabu and driver tests): the vectorised weight
of soc_amd.a2e against a literal loop, the size interpolation of an equilibrium dust against scipy, soc_amd.mabu with two
`polarisation` lines against the restatement of tests/aalg_cases.py (<emitted>.R: its header, its body, and no file without the
lines), the refusals, and two gloo ranks against one."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import aalg_cases as ac                              # noqa: E402
from soc_amd import a2e, files, mabu, synth          # noqa: E402
from test_driver import NFREQ                        # noqa: E402
from test_mabu import case, write_ini                # noqa: E402,F401  (the module's fixture: the pipeline's absorbed file)
from util import same_bits                           # noqa: E402


def test_vectorised_weight_equals_the_literal_loop():
    """A2E.py:413-429, 533-539: a equal to a size (>=: aligned), equal to the next size (0 for this one), above the largest size, 0
    (log10 = -inf, which must not be used), and the last size, which has no partial arm"""
    ASIZE = np.asarray(synth.synth_solver(NFREQ=12, NE=16, NSIZE=4, seed=2)["SIZE_A"], np.float32)
    assert (np.diff(ASIZE) > 0).all()
    aalg = np.concatenate([ac.edge_aalg(ASIZE, 40), (10.0 ** np.random.default_rng(5).uniform(np.log10(ASIZE[0]) - 0.5, np.log10(ASIZE[-1]) + 0.5, 200)).astype(np.float32)])
    assert aalg[0] == 0 and (aalg > ASIZE[-1]).any() and all((aalg == s).any() for s in ASIZE)
    seen = set()
    for isize in range(len(ASIZE)):
        with np.errstate(divide="ignore"):
            want = ac.literal_weight(ASIZE, isize, aalg)
            got = a2e.aalg_weight(ASIZE, isize, aalg)
        assert np.isfinite(got).all() and same_bits(got, want), isize
        assert got[aalg == ASIZE[isize]].min() == 1.0                                  # falls in >=
        if isize + 1 < len(ASIZE):
            assert (got[aalg == ASIZE[isize + 1]] == 0.0).all()                        # the next size: strictly between fails
            assert ((got > 0) & (got < 1)).any()
        else:
            assert set(np.unique(got)) == {0.0, 1.0}                                   # the last size has no partial arm
        hard = a2e.aalg_weight(ASIZE, isize, aalg, stochastic=False)                   # an equilibrium size: the mask alone
        assert np.array_equal(hard, (ASIZE[isize] >= aalg).astype(np.float32))
        seen |= set(np.unique(got > 0))
    assert seen == {True, False}


def test_size_interpolation_equals_scipy_interp1d(tmp_path):
    """A2E_MABU.py:635-637: the formula of soc_amd.mabu.interp_rpol against interp1d(apol, tmp, bounds_error=False, fill_value=0.0)
    after the cast of EMITTED * ipR(aalg) to float32 -- equal bits; below, on and above the nodes"""
    from scipy.interpolate import interp1d
    d = str(tmp_path)
    FREQ = np.asarray(synth.synth_solver(NFREQ=NFREQ, NE=16, NSIZE=2, seed=5)["FREQ"], np.float32)
    apol = ac.synthetic_rpol(os.path.join(d, "x.rpol"), FREQ, 2.0e-7, 6.0e-5)
    rng = np.random.default_rng(9)
    aalg = (10.0 ** rng.uniform(np.log10(apol[0]) - 0.3, np.log10(apol[-1]) + 0.3, 4000)).astype(np.float32)
    aalg[:len(apol)] = apol
    EM = (rng.lognormal(0, 3, (aalg.size, NFREQ)) * 1e-20).astype(np.float32)
    ap, tab = mabu.rpol_table(os.path.join(d, "x.dust"), FREQ)
    assert np.array_equal(ap, apol) and (aalg < ap[0]).any() and (aalg > ap[-1]).any()
    raw = np.loadtxt(os.path.join(d, "x.rpol"))
    worst = 0
    for f in range(NFREQ):
        a2, tmp = ac.literal_rpol_column(raw, FREQ[f])
        assert np.array_equal(tab[f], tmp)
        want = np.asarray(EM[:, f] * interp1d(a2, tmp, bounds_error=False, fill_value=0.0)(aalg), np.float32)
        got = np.asarray(EM[:, f] * mabu.interp_rpol(ap, tab[f], aalg), np.float32)
        lit = np.asarray(EM[:, f] * ac.literal_ipR(a2, tmp, aalg), np.float32)
        assert same_bits(got, lit)
        worst = max(worst, int(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32)).max()))
    print("largest difference to scipy: %d float32 ulp" % worst)
    assert worst == 0
    assert (FREQ < raw[0, 1]).any() and (FREQ > raw[0, -1]).any()                      # frequencies outside the columns, both sides


@pytest.fixture(scope="module")
def polcase(case):
    """the case of tests/test_mabu.py with sil.rpol and two aalg files"""
    d, CELLS = case["d"], case["cloud"].CELLS
    sol = case["sol"]
    apol = ac.synthetic_rpol(os.path.join(d, "sil.rpol"), sol["FREQ"], 2.0e-7, 6.0e-5)
    rng = np.random.default_rng(13)
    a_eq = (10.0 ** rng.uniform(np.log10(apol[0]) - 0.3, np.log10(apol[-1]) + 0.3, CELLS)).astype(np.float32)
    a_eq[1:1 + 5 * len(apol):5] = apol
    a_st = ac.edge_aalg(sol["SIZE_A"], CELLS)[rng.permutation(CELLS)]
    ac.write_aalg(os.path.join(d, "sil.aalg"), a_eq)
    ac.write_aalg(os.path.join(d, "pah.aalg"), a_st)
    optical = ["%s/sil.dust %s/sil.abu" % (d, d), "%s/gs_pah.dust" % d, "%s/carb.dust %s/carb.abu" % (d, d)]
    ini = write_ini(d, "pol.ini", optical, ac.pol_ini_lines(d, os.path.join(d, "sil.aalg"), os.path.join(d, "pah.aalg")))
    return dict(d=d, CELLS=CELLS, ini=ini, optical=optical, a_eq=a_eq, a_st=a_st,
                ABU=np.stack([case["abu"], np.ones(CELLS, np.float32), case["carb"]], axis=1))


def test_program_writes_the_reduction_factor_the_restatement_gives(case, polcase):
    from oracle_engine import OraclePipelineEngine
    d, CELLS = polcase["d"], polcase["CELLS"]
    out = os.path.join(d, "emitted_pol.data")
    info = mabu.run(polcase["ini"], os.path.join(d, "abs.data"), out, OraclePipelineEngine("soc"))
    assert info["path"] == "host" and "R" not in info
    assert os.path.getsize(out + ".R") == 4 + 4 * CELLS * NFREQ                        # the header is one int32: {CELLS}
    assert int(np.fromfile(out + ".R", np.int32, 1)[0]) == CELLS
    R = np.fromfile(out + ".R", np.float32)[1:].reshape(CELLS, NFREQ)
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    want, FPE = ac.restated_R(OraclePipelineEngine("soc"), dusts, [mabu.dust_kind(x) for x in dusts], case["FABS"], polcase["ABU"],
                              [polcase["a_eq"], polcase["a_st"], None])
    em = np.asarray(files.mmap_emitted(out, CELLS, NFREQ))
    assert same_bits(em, FPE)                                                          # the emission is what it is without the lines
    leaf = case["cloud"].DENS > 0
    assert same_bits(R, want)
    assert np.isfinite(R[leaf]).all() and (R[leaf] > 0).any() and (R[leaf] < 1).any() and R[leaf].max() <= 1.0
    # without the lines: the same emission, no .R
    plain = os.path.join(d, "emitted_nopol.data")
    mabu.run(write_ini(d, "nopol.ini", polcase["optical"]), os.path.join(d, "abs.data"), plain, OraclePipelineEngine("soc"))
    assert not os.path.exists(plain + ".R")
    with open(plain, "rb") as a, open(out, "rb") as b:
        assert a.read() == b.read()


def test_a2e_batches_equal_the_restatement():
    """soc_amd.a2e.run with aalg on an engine without the resident calls: all frequencies, one frequency, one equilibrium size"""
    from oracle_engine import OracleA2E
    sol = synth.synth_solver(NFREQ=12, NE=16, NSIZE=3, seed=2)
    ABS = (np.random.default_rng(3).lognormal(0, 1, (301, 12)) * 1e-3).astype(np.float32)
    aalg = ac.edge_aalg(sol["SIZE_A"], 301)
    for IFREQ, NSTOCH in ((-1, 999), (2, 999), (-1, 2), (2, 2)):
        eng = OracleA2E()
        E, P, _ = a2e.run(eng, sol, ABS, NSTOCH, IFREQ, batch=128, verbose=False, aalg=aalg)
        E0, _ = a2e.run(eng, sol, ABS, NSTOCH, IFREQ, batch=128, verbose=False)
        want = ac.restated_pemitted(sol, aalg, ac.per_size_emissions(eng, sol, ac.clipped(ABS), NSTOCH), NSTOCH, IFREQ, BATCH=100)
        assert P.shape == E.shape == (301, 1 if IFREQ >= 0 else 12)
        assert same_bits(E, E0) and same_bits(P, want), (IFREQ, NSTOCH)
        assert (P > 0).any() and (P < E).any() and (P[aalg > sol["SIZE_A"][-1]] == 0).all()


def test_files_that_do_not_fit_are_refused(case, polcase, tmp_path):
    from oracle_engine import OracleA2E, OraclePipelineEngine
    d, CELLS = polcase["d"], polcase["CELLS"]
    absorbed, out = os.path.join(d, "abs.data"), os.path.join(d, "emitted_refused_pol.data")
    short = ac.write_aalg(os.path.join(d, "short.aalg"), polcase["a_eq"][:-1])
    with pytest.raises(files.FileError, match="aalg file for %d cells, the run has %d" % (CELLS - 1, CELLS)):
        mabu.run(write_ini(d, "short.ini", polcase["optical"], "polarisation %s/sil.dust %s\n" % (d, short)), absorbed, out, OraclePipelineEngine("soc"))
    with pytest.raises(ValueError, match=r"`polarisation .*/olivine.dust .*` names a dust that is not in the ini"):
        mabu.run(write_ini(d, "unknown.ini", polcase["optical"], "polarisation %s/olivine.dust %s\n" % (d, short)), absorbed, out, OraclePipelineEngine("soc"))
    with pytest.raises(ValueError, match="polarisation dust_name aalg_file_name"):
        mabu.run(write_ini(d, "few.ini", polcase["optical"], "polarisation %s/sil.dust\n" % d), absorbed, out, OraclePipelineEngine("soc"))
    assert not os.path.exists(out) and not os.path.exists(out + ".R")
    # the a2e program (A2E.py:382-386)
    t = str(tmp_path)
    sol = synth.synth_solver(NFREQ=12, NE=16, NSIZE=2, seed=2)
    synth.write_solver(os.path.join(t, "x.solver"), sol)
    files.write_absorbed(os.path.join(t, "abs.bin"), np.full((9, 12), 1e-3, np.float32))
    ac.write_aalg(os.path.join(t, "bad.aalg"), np.ones(9, np.float32), cells=8)
    with pytest.raises(files.FileError, match="aalg file for 8 cells, the run has 9"):
        a2e.run_sharded(OracleA2E, os.path.join(t, "x.solver"), os.path.join(t, "abs.bin"), os.path.join(t, "em.bin"), verbose=False,
                        aalg=os.path.join(t, "bad.aalg"))
    ac.write_aalg(os.path.join(t, "ok.aalg"), ac.edge_aalg(sol["SIZE_A"], 9))
    a2e.run_sharded(OracleA2E, os.path.join(t, "x.solver"), os.path.join(t, "abs.bin"), os.path.join(t, "em.bin"), IFREQ=3, verbose=False,
                    aalg=os.path.join(t, "ok.aalg"))
    assert list(np.fromfile(os.path.join(t, "em.bin.P"), np.int32, 2)) == [9, 1] and os.path.getsize(os.path.join(t, "em.bin.P")) == 8 + 4 * 9


WORKER = r"""
import os, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests"))
from soc_amd.dist import Comm
from soc_amd import mabu
from oracle_engine import OraclePipelineEngine
comm = Comm(backend="gloo")
info = mabu.run(sys.argv[1], sys.argv[2], sys.argv[3], OraclePipelineEngine("soc"), comm)
assert info["path"] == "host"
comm.close()
"""


def test_two_ranks_write_the_reduction_factor_one_rank_writes(case, polcase):
    from oracle_engine import OraclePipelineEngine
    d = polcase["d"]
    one = os.path.join(d, "emitted_pol_w1.data")
    mabu.run(polcase["ini"], os.path.join(d, "abs.data"), one, OraclePipelineEngine("soc"))
    script = os.path.join(d, "worker_pol.py")
    with open(script, "w") as fp:
        fp.write(WORKER.format(repo=REPO))
    out = os.path.join(d, "emitted_pol_w2.data")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                           "--master-addr", "127.0.0.1", "--master-port", "29549", script, polcase["ini"], os.path.join(d, "abs.data"), out],
                          env=env, timeout=900)
    for suffix in ("", ".R"):
        with open(out + suffix, "rb") as a, open(one + suffix, "rb") as b:
            assert a.read() == b.read(), suffix


def test_pipeline_makes_polarisation_maps_from_the_factor_in_memory(tmp_path):
    """soc_amd.driver with `polarisation` lines and `polmap`, no `polred`: the maps are byte for byte those of a second run whose
    ini names, through `polred`, a file with {CELLS} and the column of the first run's R at the map's frequency; with --keep-files
    the first run also writes <emitted>.R"""
    import glob
    from oracle_engine import _A2EMethods
    from polmap_engine import PolOracleEngine
    from soc_amd import driver

    class PolPipelineEngine(PolOracleEngine, _A2EMethods):
        pass
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    IF = 5
    inis, sol = ac.driver_case(d, cloud, IF)
    os.chdir(os.path.join(d, "mem"))
    eng = PolPipelineEngine("soc")
    P = driver.Pipeline(inis["mem"], eng, verbose=0)
    CTABS, FABS, EMITTED = P.run(keep_files=True)
    assert P.R.shape == (cloud.CELLS, NFREQ) and len(eng.polmap_calls) == 1 and eng.polmap_calls[0]["polred"] == 1
    Rfile = np.fromfile(os.path.join(d, "emitted.data.R"), np.float32)
    assert int(Rfile[:1].view(np.int32)[0]) == cloud.CELLS and same_bits(Rfile[1:].reshape(cloud.CELLS, NFREQ), P.R)
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust")]
    ABU = np.stack([np.fromfile(os.path.join(d, "sil.abu"), np.float32), np.ones(cloud.CELLS, np.float32)], axis=1)
    want, _ = ac.restated_R(eng, dusts, P.kinds, FABS, ABU, [np.fromfile(os.path.join(d, x), np.float32)[1:] for x in ("sil.aalg", "pah.aalg")])
    assert same_bits(P.R, want)
    made = sorted(glob.glob("polmap_*.fits"))
    assert len(made) == 1
    ac.write_aalg(os.path.join(d, "R.bin"), P.R[:, IF])
    os.chdir(os.path.join(d, "file"))
    eng2 = PolPipelineEngine("soc")
    P2 = driver.Pipeline(inis["file"], eng2, verbose=0)
    P2.run()
    assert sorted(glob.glob("polmap_*.fits")) == made
    for k in range(3):
        assert np.array_equal(eng2.polmap_calls[0]["B"][k], eng.polmap_calls[0]["B"][k])
    with open(os.path.join(d, "mem", made[0]), "rb") as a, open(os.path.join(d, "file", made[0]), "rb") as b:
        assert a.read() == b.read()
    leaf = cloud.DENS > 0
    assert np.isfinite(P.R[leaf]).all() and (P.R[leaf, IF] > 0).any() and (P.R[leaf, IF] < 1).any()


def test_device_branch_of_the_stage_follows_the_cell_ranges(case, polcase):
    """the device branch of mabu.solve_emission with `polarisation` lines on a numpy stand-in for the resident calls (the one of
    tests/test_mabu.py plus the polarised ones): one range, and three ranges after a refusal -- the rows of each dust's aalg follow
    the range -- give the host path's emission and R"""
    from test_mabu import ResidentStandIn

    class PolarisedStandIn(ResidentStandIn):
        def mabu_begin(self, cells, NFREQ, NDUST, polarised=False):
            ResidentStandIn.mabu_begin(self, cells, NFREQ, NDUST)
            self.polarised = polarised
            self.PSUM, self.aalg, self.PEM, self.w = np.zeros((cells, NFREQ), np.float32), np.full(cells, np.nan, np.float32), None, None

        def mabu_split(self, idust, clip_last=False):
            ResidentStandIn.mabu_split(self, idust, clip_last)
            self.PEM, self.w = np.zeros_like(self.PART), None

        def a2e_resident_upload_aalg(self, c0, aalg):
            assert self.polarised
            self.aalg[c0:c0 + len(aalg)] = aalg

        def a2e_set_size(self, *a):
            self.eng.a2e_set_size(*a)
            self.w = None

        def a2e_set_size_aalg(self, ASIZE, isize):
            self.w = (ASIZE, isize)

        def a2e_resident_solve(self):
            emit = self.eng.a2e_solve(self.PART)
            self.EM += emit
            if self.w is not None:
                a2e._add_polarised(self.PEM, emit, *a2e.aalg_weights(self.w[0], self.w[1], self.aalg))

        def mabu_pol_eq(self, apol, tab):
            self.PEM = mabu.polarised_eq(self.EM, self.aalg, apol, tab)

        def mabu_accumulate_p(self, idust):
            self.PSUM += self.PEM * self.ABU[:, idust:idust + 1]

        def mabu_ratio(self):
            self.PSUM = mabu.reduction_factor(self.PSUM, self.SUM)

        def mabu_download_p(self, c0, n, out=None):
            out[:] = self.PSUM[c0:c0 + n]
            return out
    d, CELLS = polcase["d"], polcase["CELLS"]
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    kinds = [mabu.dust_kind(x) for x in dusts]
    pol = mabu.polarisation_lines(polcase["ini"], dusts)
    assert pol == [os.path.join(d, "sil.aalg"), os.path.join(d, "pah.aalg"), None]
    roomy = PolarisedStandIn(10 ** 9)
    host, hi = mabu.solve_emission(roomy, dusts, kinds, case["FABS"], polcase["ABU"], path='host', pol=pol)
    one, i1 = mabu.solve_emission(roomy, dusts, kinds, case["FABS"], polcase["ABU"], pol=pol)
    assert (hi["path"], i1["path"], i1["ranges"]) == ("host", "device", 1) and roomy.polarised
    assert same_bits(one, host) and same_bits(i1["R"], hi["R"])
    fit = CELLS // 3 + 1
    tight = PolarisedStandIn(fit)
    many, im = mabu.solve_emission(tight, dusts, kinds, case["FABS"], polcase["ABU"], pol=pol)
    assert im["ranges"] == 3 and tight.begun == [fit, fit, CELLS - 2 * fit]
    assert same_bits(many, host) and same_bits(im["R"], hi["R"])
    parts = [mabu.solve_emission(roomy, dusts, kinds, case["FABS"], polcase["ABU"], r, 2, pol=pol)[1]["R"] for r in (0, 1)]
    assert same_bits(np.concatenate(parts), hi["R"])
    # an engine with the resident calls of the emission alone takes the host path when the ini has `polarisation` lines
    assert mabu.solve_emission(ResidentStandIn(10 ** 9), dusts, kinds, case["FABS"], polcase["ABU"], pol=pol)[1]["path"] == "host"
