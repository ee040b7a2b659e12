"""soc_amd.mabu: the multi-dust emission program (reference A2E_MABU.py) on the oracle-backed engine, i.e. the host
path of the stage -- against the pipeline that produced the absorbed file, against a cell-by-cell restatement of the
reference formulas (singleabu, three dusts), two gloo ranks against one process, the refusals, and the device branch of the stage on a numpy
stand-in for the resident calls whose memory is too small (ranges sized from what the refusal reports)."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import files, synth                     # noqa: E402
from test_driver import NFREQ, write_case            # noqa: E402


def write_third_dust(d, cells):
    """a second equilibrium dust with its own abundance file, on the frequencies of tests/test_driver.py::write_case"""
    FREQ = np.asarray(synth.synth_solver(NFREQ=NFREQ, NE=16, NSIZE=2, seed=5)["FREQ"], np.float64)
    with open(os.path.join(d, "carb.dust"), "w") as fp:
        fp.write("eqdust\n 2.0e-7\n 5.0e-5\n%d\n" % NFREQ)
        for f in FREQ:
            fp.write(" %.5e  0.4  %.5e  %.5e\n" % (f, 5.0e-2 * (f / 1e14) ** 0.9, 3.0e-2 * (f / 1e14) ** 1.1))
    abu = np.random.default_rng(11).uniform(0.2, 1.2, cells).astype(np.float32)
    abu.tofile(os.path.join(d, "carb.abu"))
    return abu


def write_ini(d, name, optical, extra=""):
    """an ini for the program: the dust list (and what `extra` adds); the other keys of a run are not read"""
    path = os.path.join(d, name)
    with open(path, "w") as fp:
        fp.write("gridlength 0.05\ncloud %s/m.cloud\n%s%s" % (d, "".join("optical %s\n" % o for o in optical), extra))
    return path


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the two-dust pipeline of tests/test_driver.py run once with keep_files: its absorbed file feeds every test here"""
    from oracle_engine import OraclePipelineEngine
    from soc_amd import driver
    d = str(tmp_path_factory.mktemp("mabu"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, sol, abu = write_case(d, cloud)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        P = driver.Pipeline(ini, OraclePipelineEngine("soc"), verbose=0)
        CTABS, FABS, EMITTED = P.run(keep_files=True)
    finally:
        os.chdir(cwd)
    return dict(d=d, ini=ini, sol=sol, abu=abu, cloud=cloud, FABS=FABS, EMITTED=EMITTED, timers=P.timers,
                carb=write_third_dust(d, cloud.CELLS))


def test_program_reproduces_the_pipelines_emission_from_its_absorbed_file(case):
    from oracle_engine import OraclePipelineEngine
    from soc_amd import mabu
    d = case["d"]
    assert case["timers"]["emission_path"] == "host"               # (the oracle-backed engine has no soc_mabu_* calls)
    out = os.path.join(d, "emitted_program.data")
    info = mabu.run(case["ini"], os.path.join(d, "abs.data"), out, OraclePipelineEngine("soc"))
    assert info["path"] == "host"
    assert list(np.fromfile(out, np.int32, 2)) == [case["cloud"].CELLS, NFREQ]
    em = np.asarray(files.mmap_emitted(out, case["cloud"].CELLS, NFREQ))
    assert np.array_equal(em.view(np.uint32), case["EMITTED"].view(np.uint32))
    assert (em[case["cloud"].DENS > 0] > 0).any()


def eq_cross_section(path):
    with open(path) as fp:
        lines = fp.readlines()
    gd, radius = float(lines[1].split()[0]), float(lines[2].split()[0])
    return np.pi * radius ** 2.0 * gd * np.loadtxt(path, skiprows=4)[:, 2]


def restated_emission(case, dusts, ABU, cells):
    """stage 2 cell by cell from the reference formulas, as tests/test_driver.py restates it: RABS (A2E_MABU.py:245-342), the split
    (kernel_A2E_MABU_aux.c:3-23), the solvers on the oracle, the abundance-weighted sum (A2E_MABU.py:1128-1140).
    dusts: 'pah' (the stochastically heated dust of the case) or the path of an equilibrium dust file"""
    from oracle.pyoracle import Oracle, a2e_oracle_dosolve, oracle_eqsolver
    from soc_amd import driver
    from soc_amd.launch import FACTOR
    orc = Oracle("soc")
    sol, FABS = case["sol"], case["FABS"]
    cols = [np.sum(np.asarray(sol["SK_ABS"], np.float64), axis=0) if x == 'pah' else eq_cross_section(x) for x in dusts]
    R = np.clip(np.stack(cols, axis=1), 1e-40, 1e30)
    R /= (1e-40 + R.sum(axis=1))[:, None]
    R = np.clip(R, 1e-30, 1.0)
    want = np.zeros((len(cells), NFREQ), np.float32)
    for idust, x in enumerate(dusts):
        part = np.zeros((len(cells), NFREQ), np.float32)
        for n, c in enumerate(cells):
            for f in range(NFREQ):
                den = np.float32(0.0)
                for j in range(len(dusts)):
                    den = np.float32(np.float64(den) + np.float64(ABU[c, j]) * R[f, j])
                part[n, f] = np.float32(np.float64(FABS[c, f]) * R[f, idust] / np.float64(den))
        if x == 'pah':
            p = part.copy()
            p[:, NFREQ - 1] = np.clip(p[:, NFREQ - 1], 0.0, 0.2 * p[:, NFREQ - 2])                   # A2E.py:184-185
            em = np.zeros_like(p)
            for isize in range(sol["NSIZE"]):
                em += a2e_oracle_dosolve(orc, sol["NE"], NFREQ, sol["sizes"][isize], synth.a2e_absorption_fraction(sol, isize), p)
        else:
            Fq, KABS, Emin, kE, oplgkE, TTT = driver.eq_dust_table(x)
            _, em = oracle_eqsolver(orc, 0, len(cells), driver.NE_EQ, FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT, part)
        want += em * ABU[cells, idust:idust + 1]
    return want


def run_program(case, ini, name):
    from oracle_engine import OraclePipelineEngine
    from soc_amd import mabu
    out = os.path.join(case["d"], name)
    mabu.run(ini, os.path.join(case["d"], "abs.data"), out, OraclePipelineEngine("soc"))
    return np.asarray(files.mmap_emitted(out, case["cloud"].CELLS, NFREQ))


def test_singleabu_matches_a_cell_by_cell_restatement(case):
    d, CELLS = case["d"], case["cloud"].CELLS
    x = (case["abu"] / 2.0).astype(np.float32)                     # abundances x and 1 - x, both in (0, 1)
    x.tofile(os.path.join(d, "half.abu"))
    ini = write_ini(d, "single.ini", ["%s/sil.dust %s/half.abu" % (d, d), "%s/gs_pah.dust" % d], "singleabu\n")
    em = run_program(case, ini, "emitted_single.data")
    ABU = np.stack([x, np.float32(1.0) - x], axis=1)
    cells = np.flatnonzero(case["cloud"].DENS > 0)[::7]
    want = restated_emission(case, [os.path.join(d, "sil.dust"), 'pah'], ABU, cells)
    assert np.allclose(em[cells], want, rtol=2e-6, atol=1e-30)
    assert (em[cells] > 0).any()
    assert not np.array_equal(em, case["EMITTED"])                 # (the abundances took effect)


def test_three_dusts_match_a_cell_by_cell_restatement(case):
    d, CELLS = case["d"], case["cloud"].CELLS
    ini = write_ini(d, "three.ini", ["%s/sil.dust %s/sil.abu" % (d, d), "%s/gs_pah.dust" % d, "%s/carb.dust %s/carb.abu" % (d, d)])
    em = run_program(case, ini, "emitted_three.data")
    ABU = np.stack([case["abu"], np.ones(CELLS, np.float32), case["carb"]], axis=1)
    cells = np.flatnonzero(case["cloud"].DENS > 0)[::7]
    want = restated_emission(case, [os.path.join(d, "sil.dust"), 'pah', os.path.join(d, "carb.dust")], ABU, cells)
    assert np.allclose(em[cells], want, rtol=2e-6, atol=1e-30)
    assert (em[cells] > 0).any()


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


def test_two_ranks_write_the_file_one_rank_writes(case):
    d = case["d"]
    ini = write_ini(d, "three_w2.ini", ["%s/sil.dust %s/sil.abu" % (d, d), "%s/gs_pah.dust" % d, "%s/carb.dust %s/carb.abu" % (d, d)])
    one = run_program(case, ini, "emitted_w1.data")
    script = os.path.join(d, "worker.py")
    with open(script, "w") as fp:
        fp.write(WORKER.format(repo=REPO))
    out = os.path.join(d, "emitted_w2.data")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                           "--master-addr", "127.0.0.1", "--master-port", "29547", script, ini, os.path.join(d, "abs.data"), out],
                          env=env, timeout=900)
    with open(out, "rb") as a, open(os.path.join(d, "emitted_w1.data"), "rb") as b:
        assert a.read() == b.read()
    assert (one[case["cloud"].DENS > 0] > 0).any()


def test_refusals_name_their_reason(case):
    from oracle_engine import OraclePipelineEngine
    from soc_amd import mabu
    from soc_amd.asoc import UnsupportedOption
    d = case["d"]
    eng = OraclePipelineEngine("soc")
    absorbed, out = os.path.join(d, "abs.data"), os.path.join(d, "emitted_refused.data")
    with pytest.raises(UnsupportedOption, match="subset of the frequencies"):
        mabu.run(case["ini"], absorbed, out, eng, ofreq=os.path.join(d, "ofreq.dat"))
    with pytest.raises(UnsupportedOption, match="nnsolve"):
        mabu.run(write_ini(d, "nn.ini", ["%s/sil.dust" % d, "%s/gs_pah.dust" % d], "nnsolve lib\n"), absorbed, out, eng)
    with open(os.path.join(d, "gs_other.dust"), "w") as fp:
        fp.write("gsetdust\n")
    with pytest.raises(FileNotFoundError, match="the solver file of .*gs_other.dust is missing; write it with python -m soc_amd.a2e_pre"):
        mabu.run(write_ini(d, "nosolver.ini", ["%s/sil.dust" % d, "%s/gs_other.dust" % d]), absorbed, out, eng)
    assert not os.path.exists(out)
    assert mabu.main(["mabu", "soc.ini"]) == 1                    # usage


class ResidentStandIn:
    """The soc_mabu_* methods of soc_amd.lib.Engine restated in numpy on the oracle-backed engine, with a device that holds
    at most `capacity` cells: mabu_begin refuses more with lib.DoesNotFit, as the library does when memory is short.  Lets the
    device branch of mabu.solve_emission -- its call order, the resize after a refusal, the end of its loop -- run without a GPU."""

    def __init__(self, capacity):
        from oracle_engine import OraclePipelineEngine
        self.eng, self.capacity, self.begun, self.open = OraclePipelineEngine("soc"), capacity, [], False

    def __getattr__(self, name):                                   # eqsolver, a2e_solve ...: the host path's calls
        if name.startswith("a2e_resident"):
            raise AttributeError(name)
        return getattr(self.eng, name)

    def mabu_begin(self, cells, NFREQ, NDUST):
        from soc_amd.lib import DoesNotFit
        assert not self.open
        if cells > self.capacity:
            raise DoesNotFit("%d cells need more device memory than is free (%d cells fit)" % (cells, self.capacity), self.capacity)
        self.begun.append(cells)
        self.open = True
        self.ABS, self.SUM = np.zeros((cells, NFREQ), np.float32), np.zeros((cells, NFREQ), np.float32)
        self.PART = self.EM = None

    def mabu_upload(self, c0, ABS):
        self.ABS[c0:c0 + len(ABS)] = ABS

    def mabu_set_tables(self, ABU, RABS):
        assert ABU.shape == (len(self.ABS), RABS.shape[1])
        self.ABU, self.RABS = np.array(ABU, np.float32), np.array(RABS, np.float64)

    def mabu_split(self, idust, clip_last=False):
        from soc_amd import mabu
        self.PART = mabu.split_absorbed(self.ABS, self.RABS, self.ABU, idust)
        if clip_last:
            self.PART[:, -1] = np.clip(self.PART[:, -1], 0.0, 0.2 * self.PART[:, -2])
        self.EM = np.zeros_like(self.PART)

    def mabu_solve_eq(self, NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT):
        _, self.EM = self.eng.eqsolver(0, len(self.PART), NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, self.PART)

    def a2e_set_size(self, *a):
        self.eng.a2e_set_size(*a)

    def a2e_resident_solve(self):
        self.EM += self.eng.a2e_solve(self.PART)

    def mabu_accumulate(self, idust):
        self.SUM += self.EM * self.ABU[:, idust:idust + 1]

    def mabu_download(self, c0, n, out=None):
        out[:] = self.SUM[c0:c0 + n]
        return out

    def mabu_end(self):
        self.open = False


def test_refused_cells_are_solved_in_ranges_of_the_size_the_refusal_reports(case):
    from soc_amd import mabu
    d, CELLS = case["d"], case["cloud"].CELLS
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    kinds = [mabu.dust_kind(x) for x in dusts]
    ABU = np.stack([case["abu"], np.ones(CELLS, np.float32), case["carb"]], axis=1)
    roomy = ResidentStandIn(10 ** 9)
    host, hi = mabu.solve_emission(roomy, dusts, kinds, case["FABS"], ABU, path='host')
    one, i1 = mabu.solve_emission(roomy, dusts, kinds, case["FABS"], ABU)
    assert (hi["path"], i1["path"], i1["ranges"], roomy.begun) == ("host", "device", 1, [CELLS])
    assert np.array_equal(one.view(np.uint32), host.view(np.uint32))
    fit = CELLS // 3 + 1                                            # the whole is refused once, then three ranges
    tight = ResidentStandIn(fit)
    many, im = mabu.solve_emission(tight, dusts, kinds, case["FABS"], ABU)
    assert (im["path"], im["ranges"]) == ("device", 3)
    assert tight.begun == [fit, fit, CELLS - 2 * fit] and not tight.open
    assert np.array_equal(many.view(np.uint32), host.view(np.uint32))
    # a limit the caller gives that is larger than what fits is cut down the same way
    tight = ResidentStandIn(fit)
    again, ia = mabu.solve_emission(tight, dusts, kinds, case["FABS"], ABU, range_cells=CELLS - 1)
    assert ia["ranges"] == 3 and np.array_equal(again.view(np.uint32), host.view(np.uint32))
