"""`convergence eps [kmin]`: the host statements of soc_amd.converge against a restatement (converge_ref.py), the ini key, and
soc_amd.driver's loop on the oracle-backed engine -- it stops at the step the criterion names and leaves, bit for bit, the products of
`iterations k` without the key.

The 392-cell case of test_driver_iterations.py does not converge (its synthetic dusts answer a 0.3 % rise of the absorptions with a
doubled emission): d_l1 of steps 1..5, with W = launch.trapezoid_weight, is 0.4968, 0.3300, 0.2470, 0.1972, 0.1641 on the oracle
engine, falling monotonically (d_total equals it to 15 digits: every cell brightens).  So the tests do not wait for
convergence; they place eps between the figures of two steps, computed by the restatement from the chain of the existing programs
(reemit_chain.chain)."""
import math
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import converge_ref as ref                           # noqa: E402
from soc_amd import converge, files, synth           # noqa: E402
from soc_amd.asoc import UnsupportedOption           # noqa: E402
from soc_amd.ini import IniError, User               # noqa: E402

NFREQ = 12                                           # of test_driver.write_case


# ---- the host statements ------------------------------------------------------------------------------------------------
def test_luminosity_and_change_equal_the_restatement():
    nfreq = 7
    cloud, E, dead, nbad = ref.octree_with_specials(nfreq)
    W = ref.trapezoid(ref.frequencies(nfreq))
    COEFF = ref.coeff(cloud.LEVELS)
    L, bad = converge.luminosity(E, W, cloud.DENS, cloud.OFF, cloud.LCELLS, COEFF)
    Lw, badw = ref.luminosity(E, W, cloud, COEFF)
    assert bad == badw == nbad == 2
    assert np.array_equal(ref.bits64(L), ref.bits64(Lw))
    assert (L[dead] == 0).all() and np.isfinite(L).all() and (L >= 0).all() and (L[~dead] > 0).sum() == (~dead).sum() - 2
    levels = np.searchsorted(np.asarray(cloud.OFF[:3]), np.flatnonzero(L > 0), side='right') - 1
    assert set(levels) == {0, 1, 2}                                          # every level's coefficient was used by a live cell
    # a second emission: most cells a few per cent off, some switched off, some switched on
    rng = np.random.default_rng(11)
    E2 = (E * rng.uniform(0.9, 1.1, E.shape)).astype(np.float32)
    live = np.flatnonzero(~dead)
    E2[live[5:9]] = 0.0
    L2, bad2 = converge.luminosity(E2, W, cloud.DENS, cloud.OFF, cloud.LCELLS, COEFF)
    L2w, _ = ref.luminosity(E2, W, cloud, COEFF)
    assert bad2 == 2 and np.array_equal(ref.bits64(L2), ref.bits64(L2w))
    for a, b in ((L, np.zeros_like(L)), (L2, L), (L, L2), (L, L)):
        got, want = converge.change(a, b), ref.change(a, b)
        assert ref.sums_close(got, want, cloud.CELLS), (got, want)
        assert got["M"] == want["M"]
    assert converge.change(L, np.zeros_like(L))["M"] == 1.0 and converge.change(L2, L)["M"] == 1.0       # (cells switched off)
    assert converge.change(L, L) == dict(S_abs=0.0, S_new=converge.change(L, L)["S_new"], S_old=converge.change(L, L)["S_old"], M=0.0)
    first = converge.figures(converge.change(L, np.zeros_like(L)))
    assert first["d_l1"] == 1.0 and first["d_total"] == 1.0 and first["d_max"] == 1.0                     # step 0 primes the plane
    fig = converge.figures(converge.change(L2, L))
    assert 0.0 < fig["d_l1"] < math.inf and fig["d_total"] <= fig["d_l1"] * (1 + 1e-12)


def test_figures_of_an_emission_that_is_zero():
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    W = ref.trapezoid(ref.frequencies(5))
    L, bad = converge.luminosity(np.zeros((cloud.CELLS, 5), np.float32), W, cloud.DENS, cloud.OFF, cloud.LCELLS, ref.coeff(2))
    assert bad == 0 and not L.any()
    st = converge.change(L, L)
    assert st == dict(S_abs=0.0, S_new=0.0, S_old=0.0, M=0.0)
    assert converge.figures(st) == dict(d_l1=0.0, d_total=0.0, d_max=0.0)
    gone = converge.figures(converge.change(L, np.ones_like(L)))             # everything switched off: only S_new is 0
    assert gone["d_l1"] == math.inf and gone["d_total"] == math.inf and gone["d_max"] == 1.0


# ---- the ini key ------------------------------------------------------------------------------------------------------
def test_ini_key():
    U = User(text="iterations 3\n")
    assert U.CONVERGENCE < 0 and U.CONVERGENCE_MIN == 1
    U = User(text="convergence 0.3\n")
    assert (U.CONVERGENCE, U.CONVERGENCE_MIN) == (0.3, 1)
    U = User(text="convergence 0.3 2   # comment\n")
    assert (U.CONVERGENCE, U.CONVERGENCE_MIN) == (0.3, 2)
    U = User(text="convergence 0\n")
    assert (U.CONVERGENCE, U.CONVERGENCE_MIN) == (0.0, 1)
    for line in ("convergence -1", "convergence 0.1 0", "convergence nan", "convergence 0.1 x"):
        with pytest.raises(IniError, match=line):
            User(text="iterations 3\n%s\n" % line)
    # no other key fires on it, and it fires on no other key
    U = User(text="convergence 0.25 3\ncellpackets 10\ncloud a.cloud\n")
    V = User(text="cellpackets 10\ncloud a.cloud\n")
    differ = {k for k in vars(V) if k != "KEYS" and repr(getattr(U, k)) != repr(getattr(V, k))}
    assert differ == {"CONVERGENCE", "CONVERGENCE_MIN"}


# ---- the loop on the oracle engine ----------------------------------------------------------------------------------------
def cloud_():
    return synth.octree_cloud(6, levels=2, frac=0.1, seed=9)                # 392 cells


class Recording:
    """mixed into the oracle engine: an emitted_change that records its calls (the oracle engine has no resident emission, so the
    loop must not call it with or without the key)"""
    def emitted_change(self, W, COEFF):
        self.change_calls = getattr(self, "change_calls", 0) + 1
        raise AssertionError("emitted_change on an engine without emitted_begin")


def recording_engine():
    from oracle_engine import OraclePipelineEngine

    class Engine(Recording, OraclePipelineEngine):
        pass
    return Engine("soc")


def run_pipeline(d, cloud, iterations, extra):
    """the pipeline in directory d -> dict of what the tests compare"""
    from reemit_chain import iteration_case
    from soc_amd import driver
    ini, _ = iteration_case(d, cloud, iterations, extra)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        eng = recording_engine()
        P = driver.Pipeline(ini, eng, verbose=0)
        CTABS, FABS, EMITTED = P.run(keep_files=True)
    finally:
        os.chdir(cwd)
    dat = os.path.join(d, "convergence.dat")
    return dict(P=P, FABS=FABS, EMITTED=EMITTED, d=d, calls=getattr(eng, "change_calls", 0),
                emitted_file=np.asarray(files.mmap_emitted(os.path.join(d, "emitted.data"), cloud.CELLS, NFREQ)),
                absorbed_file=files.read_absorbed(os.path.join(d, "abs.data")),
                map=np.fromfile(os.path.join(d, "map_dir_00.bin"), np.float32),
                dat=np.loadtxt(dat, ndmin=2) if os.path.exists(dat) else None)


@pytest.fixture(scope="module")
def chain3(tmp_path_factory):
    """the chain of the existing programs for three steps, and d_l1 of steps 0..3 by the restatement"""
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import chain, iteration_case
    root = str(tmp_path_factory.mktemp("converge"))
    cloud = cloud_()
    d = os.path.join(root, "chain")
    ini, ini0 = iteration_case(d, cloud, 3)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        steps = chain(ini, ini0, lambda: OraclePipelineEngine("soc"), 3, cloud.CELLS, NFREQ)
    finally:
        os.chdir(cwd)
    FFREQ = np.loadtxt(os.path.join(d, "sil.dust"), skiprows=4)[:, 0].astype(np.float32)
    W, COEFF = ref.trapezoid(FFREQ), ref.coeff(cloud.LEVELS)
    Lp, stats = np.zeros(cloud.CELLS), []
    for FABS, E in steps:
        L, bad = ref.luminosity(E, W, cloud, COEFF)
        assert bad == 0
        stats.append(ref.change(L, Lp))
        Lp = L
    d_ = [ref.d_l1(st) for st in stats]
    print("d_l1 of steps 0..3 by the restatement:", d_)
    assert d_[0] == 1.0 and d_[1] > d_[2] > d_[3] > 0.0                      # they fall
    return dict(root=root, cloud=cloud, steps=steps, d=d_, eps=0.5 * (d_[2] + d_[3]), W=W, COEFF=COEFF)


@pytest.fixture(scope="module")
def plain3(chain3):
    return run_pipeline(os.path.join(chain3["root"], "plain3"), chain3["cloud"], 3, "")


def same_figures(run, chain3, upto):
    cells = chain3["cloud"].CELLS
    tol = cells * 2.0 ** -52                                                 # the bound of the sums (converge_ref.sums_close)
    conv = run["P"].timers["convergence"]
    assert [c["k"] for c in conv] == list(range(upto + 1)) and all(c["source"] == 'host' and c["bad"] == 0 and c["seconds"] >= 0 for c in conv)
    assert run["dat"].shape == (upto + 1, 4) and list(run["dat"][:, 0]) == list(range(upto + 1))
    for k in range(min(upto, 3) + 1):
        want = chain3["d"][k]
        assert abs(conv[k]["d_l1"] - want) <= tol * want and abs(run["dat"][k, 1] - want) <= tol * want
        assert run["dat"][k, 2] == conv[k]["d_total"] and run["dat"][k, 3] == conv[k]["d_max"]


def test_the_loop_stops_where_the_criterion_says_and_leaves_the_products_of_that_step(chain3, plain3):
    cloud, eps = chain3["cloud"], chain3["eps"]
    run = run_pipeline(os.path.join(chain3["root"], "eps"), cloud, 5, "convergence %.17g\n" % eps)
    P = run["P"]
    assert P.converged == 3 and len(P.timers["iterations"]) == 3
    FABS3, E3 = chain3["steps"][3]
    assert np.array_equal(run["EMITTED"], E3) and np.array_equal(run["FABS"], FABS3)
    assert np.array_equal(run["emitted_file"], E3) and np.array_equal(run["absorbed_file"], FABS3)
    same_figures(run, chain3, 3)
    assert P.timers["convergence"][3]["d_l1"] < eps <= P.timers["convergence"][2]["d_l1"]
    assert np.array_equal(run["map"], plain3["map"]) and np.array_equal(run["EMITTED"], plain3["EMITTED"])
    assert run["calls"] == 0


def test_kmin_holds_the_loop(chain3):
    run = run_pipeline(os.path.join(chain3["root"], "kmin"), chain3["cloud"], 5, "convergence %.17g 4\n" % chain3["eps"])
    P = run["P"]
    assert P.converged == 4 and len(P.timers["iterations"]) == 4
    same_figures(run, chain3, 4)
    assert P.timers["convergence"][4]["d_l1"] < P.timers["convergence"][3]["d_l1"] < chain3["eps"]


def test_eps_zero_reports_and_never_stops(chain3):
    cloud = chain3["cloud"]
    run = run_pipeline(os.path.join(chain3["root"], "zero"), cloud, 5, "convergence 0\n")
    plain = run_pipeline(os.path.join(chain3["root"], "plain5"), cloud, 5, "")
    P = run["P"]
    assert P.converged is None and len(P.timers["iterations"]) == 5
    same_figures(run, chain3, 5)
    d = [c["d_l1"] for c in P.timers["convergence"]]
    assert all(a > b for a, b in zip(d[1:], d[2:]))
    for key in ("EMITTED", "FABS", "emitted_file", "absorbed_file", "map"):
        assert np.array_equal(run[key], plain[key]), key
    assert plain["P"].converged is None and "convergence" not in plain["P"].timers and plain["dat"] is None


def test_without_the_key_nothing_is_measured(chain3, plain3):
    P = plain3["P"]
    assert "convergence" not in P.timers and P.converged is None and len(P.timers["iterations"]) == 3
    assert not os.path.exists(os.path.join(plain3["d"], "convergence.dat")) and plain3["calls"] == 0
    assert np.array_equal(plain3["EMITTED"], chain3["steps"][3][1]) and np.array_equal(plain3["FABS"], chain3["steps"][3][0])


def test_without_cellpackets_the_key_has_no_effect(tmp_path):
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import iteration_case
    from soc_amd import driver
    _, ini0 = iteration_case(str(tmp_path), cloud_(), 2, "convergence 0.1\n")
    cwd = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        P = driver.Pipeline(ini0, OraclePipelineEngine("soc"), verbose=0)
        P.run()
    finally:
        os.chdir(cwd)
    assert "convergence" not in P.timers and P.converged is None and P.timers["iterations"] == []
    assert not os.path.exists(os.path.join(str(tmp_path), "convergence.dat"))


def test_asoc_alone_refuses_the_key(tmp_path):
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import iteration_case
    from soc_amd.asoc import AbsorptionRun
    ini, ini0 = iteration_case(str(tmp_path), cloud_(), 2, "convergence 0.1\n")
    for name, refused in ((ini, True), (ini0, False)):                       # (without cellpackets the key is without effect, not refused)
        U = User(name)
        U.file_optical = [os.path.join(str(tmp_path), "sil.dust"), os.path.join(str(tmp_path), "pah_simple.dust")]
        if refused:
            with pytest.raises(UnsupportedOption, match="convergence"):
                AbsorptionRun(U, OraclePipelineEngine("soc"), verbose=0)
        else:
            AbsorptionRun(U, OraclePipelineEngine("soc"), verbose=0)


WORKER = r"""
import json, os, sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, os.path.join({repo!r}, "tests"))
import numpy as np
from soc_amd import driver
from soc_amd.dist import Comm
from oracle_engine import OraclePipelineEngine
comm = Comm(backend="gloo")
os.chdir(os.path.join(sys.argv[2], "r%d" % comm.rank))
P = driver.Pipeline(sys.argv[1], OraclePipelineEngine("soc"), comm, verbose=0)
CTABS, FABS, EMITTED = P.run()
np.save("emitted_rank%d.npy" % comm.rank, EMITTED)
with open("convergence_rank%d.json" % comm.rank, "w") as fp:
    json.dump(dict(converged=P.converged, iterations=len(P.timers["iterations"]), steps=P.timers["convergence"]), fp)
comm.close()
"""


def test_two_ranks_stop_at_the_same_step(chain3):
    """every rank holds the whole emission and takes the figures on the host; both act on rank 0's decision, rank 0 writes the file"""
    import json
    import subprocess
    from reemit_chain import iteration_case
    cloud = chain3["cloud"]
    d = os.path.join(chain3["root"], "ranks")
    ini, _ = iteration_case(d, cloud, 5, "convergence %.17g\n" % chain3["eps"])
    for r in (0, 1):
        os.makedirs(os.path.join(d, "r%d" % r))
    script = os.path.join(d, "worker.py")
    with open(script, "w") as fp:
        fp.write(WORKER.format(repo=REPO))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                           "--master-addr", "127.0.0.1", "--master-port", "29553", script, ini, d], env=env, timeout=600)
    E3 = chain3["steps"][3][1]
    leaf = cloud.DENS > 0
    for r in (0, 1):
        with open(os.path.join(d, "r%d" % r, "convergence_rank%d.json" % r)) as fp:
            got = json.load(fp)
        assert got["converged"] == 3 and got["iterations"] == 3 and [s["source"] for s in got["steps"]] == ['host'] * 4
        for k in range(4):                                                   # (the tallies of two ranks are summed in another order)
            assert abs(got["steps"][k]["d_l1"] - chain3["d"][k]) <= 1e-4 * chain3["d"][k]
        E = np.load(os.path.join(d, "r%d" % r, "emitted_rank%d.npy" % r))
        assert np.allclose(E[leaf], E3[leaf], rtol=1e-2, atol=1e-6 * np.abs(E3[leaf]).max())
    assert os.path.exists(os.path.join(d, "r0", "convergence.dat")) and not os.path.exists(os.path.join(d, "r1", "convergence.dat"))
