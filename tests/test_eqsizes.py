"""Equilibrium grain sizes of a stochastically heated dust (`nstoch N` in its gsetdust file, A2E_MABU.py:124-143) without a GPU: the
parser, the host path of soc_amd.mabu on the oracle-backed engine against soc_amd.a2e.run with that NSTOCH, the kept E -> T tables,
and which path the stage takes with an engine that has the soc_mabu_* calls but no a2e_resident_solve_eq."""
import os
import shutil
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import a2e, mabu, synth                  # noqa: E402
from soc_amd.launch import FACTOR                     # noqa: E402
from test_driver import NFREQ, write_case             # noqa: E402

CELLS = 37


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def nstoch_copy(d, tag, lines):
    """a directory <d>/<tag> with a copy of the solver file and a gs_pah.dust that holds `lines` after its first line"""
    sub = os.path.join(d, tag)
    os.makedirs(sub)
    shutil.copy(os.path.join(d, "pah.solver"), os.path.join(sub, "pah.solver"))
    with open(os.path.join(sub, "gs_pah.dust"), "w") as fp:
        fp.write("gsetdust\n" + lines)
    return os.path.join(sub, "gs_pah.dust")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the dust files of test_driver.write_case, the stochastically heated dust with four sizes, and absorptions of their size"""
    d = str(tmp_path_factory.mktemp("eqsizes"))
    write_case(d, synth.cartesian_cloud(3, seed=2))
    sol = synth.synth_solver(NFREQ=NFREQ, NE=16, NSIZE=4, seed=5)
    synth.write_solver(os.path.join(d, "pah.solver"), sol)
    rng = np.random.default_rng(8)
    FABS = (rng.uniform(0.0, 1.0, (CELLS, NFREQ)) * 10.0 ** rng.uniform(-9, -5, (CELLS, 1))).astype(np.float32)
    FABS[5] = 0.0
    ABU = rng.uniform(0.2, 1.5, (CELLS, 2)).astype(np.float32)
    return dict(d=d, sol=sol, FABS=FABS, ABU=ABU)


def test_parser_reads_the_line_as_the_reference_does(case):
    d = case["d"]
    assert mabu.read_nstoch(os.path.join(d, "gs_pah.dust")) == 9999 == mabu.NSTOCH_ALL                  # no line
    assert mabu.read_nstoch(nstoch_copy(d, "p3", "nstoch 3\n")) == 3
    assert mabu.read_nstoch(nstoch_copy(d, "pm", "nstoch -1\n")) == 9999
    assert mabu.read_nstoch(nstoch_copy(d, "p0", "# sizes\n  nstoch   0   # all at their equilibrium temperature\n1.0 2.0\n")) == 0
    assert mabu.read_nstoch(nstoch_copy(d, "pl", "nstoch 1\nnstoch 2\n")) == 2                          # the last line holds
    assert mabu.read_nstoch(nstoch_copy(d, "pn", "nstoch\nnstochastic 1\nxnstoch 1\n")) == 9999         # the first token, and a value
    eq = os.path.join(d, "sil_nstoch.dust")
    with open(os.path.join(d, "sil.dust")) as fp, open(eq, "w") as out:
        out.write(fp.read() + "nstoch 1\n")
    assert mabu.dust_kind(eq) == 'eqdust' and mabu.read_nstoch(eq) == 9999                              # ignored in an eqdust file
    tables = mabu._tables([os.path.join(d, "sil.dust"), os.path.join(d, "p3", "gs_pah.dust")], ['eqdust', 'gsetdust'], NFREQ)
    assert tables[1]["nstoch"] == 3 and mabu.stochastic_sizes(tables[1]) == 3
    tables = mabu._tables([os.path.join(d, "gs_pah.dust")], ['gsetdust'], NFREQ)
    assert tables[0]["nstoch"] == 9999 and mabu.stochastic_sizes(tables[0]) == 4


@pytest.mark.parametrize("n", [0, 2, 3, 9])
def test_host_path_gives_a2e_run_with_that_nstoch_per_dust(case, n):
    from oracle_engine import OraclePipelineEngine
    d, sol, FABS, ABU = case["d"], case["sol"], case["FABS"], case["ABU"]
    eng = OraclePipelineEngine("soc")
    dusts = [os.path.join(d, "sil.dust"), nstoch_copy(d, "h%d" % n, "nstoch %d\n" % n)]
    kinds = [mabu.dust_kind(x) for x in dusts]
    EM, info = mabu.solve_emission(eng, dusts, kinds, FABS, ABU)
    assert info["path"] == "host"
    RABS, _ = mabu.relative_cross_sections(dusts, kinds)
    Fq, KABS, Emin, kE, oplgkE, TTT = mabu.eq_dust_table(dusts[0])
    _, em0 = eng.eqsolver(0, CELLS, mabu.NE_EQ, FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT, mabu.split_absorbed(FABS, RABS, ABU, 0))
    em1, _ = a2e.run(eng, sol, mabu.split_absorbed(FABS, RABS, ABU, 1), NSTOCH=n, verbose=False)
    want = np.zeros((CELLS, NFREQ), np.float32)
    want += em0 * ABU[:, 0:1]
    want += em1 * ABU[:, 1:2]
    assert np.isfinite(want).all() and (want > 0).any()
    assert np.array_equal(bits(EM), bits(want))
    if n < 4:                                                   # ... and the line changes the result: all sizes stochastic gives other bits
        plain, _ = a2e.run(eng, sol, mabu.split_absorbed(FABS, RABS, ABU, 1), verbose=False)
        assert not np.array_equal(bits(plain), bits(em1))


def test_eq_table_is_built_once_per_solver_and_size(case, monkeypatch):
    sol = synth.synth_solver(NFREQ=7, NE=16, NSIZE=2, seed=41)
    calls = []
    real = a2e._eq_table
    monkeypatch.setattr(a2e, "_eq_table", lambda s, i: calls.append(i) or real(s, i))
    first = a2e.eq_table(sol, 1)
    again = a2e.eq_table(sol, 1)
    assert calls == [1]
    assert all(x is y for x, y in zip(first, again))                                    # the kept arrays
    fresh = real(sol, 1)
    for x, y in zip(again, fresh):                                                      # ... with the bits of a fresh table
        assert np.asarray(x).dtype == np.asarray(y).dtype and np.asarray(x).tobytes() == np.asarray(y).tobytes()
    reread = dict(sol, FREQ=np.array(sol["FREQ"]), SK_ABS=np.array(sol["SK_ABS"]))      # another dict of the same solver: the same table
    assert a2e.eq_table(reread, 1)[3] is first[3] and calls == [1]
    other = a2e.eq_table(sol, 0)
    assert calls == [1, 0] and not np.array_equal(other[3], first[3])
    changed = dict(sol, GD=np.float32(2.0) * sol["GD"])                                 # another solver: its own table
    a2e.eq_table(changed, 1)
    assert calls == [1, 0, 1]


def test_engine_without_the_eq_call_keeps_the_device_path_for_stochastic_sizes_only(case):
    """the numpy stand-in of tests/test_mabu.py has mabu_begin and no a2e_resident_solve_eq"""
    from test_mabu import ResidentStandIn
    d, FABS, ABU = case["d"], case["FABS"], case["ABU"]
    eng = ResidentStandIn(10 ** 9)
    assert hasattr(eng, "mabu_begin") and not hasattr(eng, "a2e_resident_solve_eq")
    for k, (lines, path) in enumerate((("", "device"), ("nstoch 9\n", "device"), ("nstoch 4\n", "device"), ("nstoch 3\n", "host"))):
        dusts = [os.path.join(d, "sil.dust"), nstoch_copy(d, "f%d" % k, lines)]
        kinds = [mabu.dust_kind(x) for x in dusts]
        assert mabu.device_path_offered(eng, dusts, kinds, NFREQ) == (path == "device")
        EM, info = mabu.solve_emission(eng, dusts, kinds, FABS, ABU)
        assert info["path"] == path, lines
        host, _ = mabu.solve_emission(eng, dusts, kinds, FABS, ABU, path='host')
        assert np.array_equal(bits(EM), bits(host))
    with pytest.raises(ValueError, match="not available"):
        mabu.solve_emission(eng, dusts, kinds, FABS, ABU, path='device')                # (the last case: one equilibrium size)


def test_engine_with_the_eq_call_is_offered_the_device_path(case):
    class WithEq:
        def mabu_begin(self, *a):
            pass

        def a2e_resident_solve_eq(self):
            pass

    d = case["d"]
    dusts = [os.path.join(d, "sil.dust"), nstoch_copy(d, "w", "nstoch 1\n")]
    assert mabu.device_path_offered(WithEq(), dusts, ['eqdust', 'gsetdust'], NFREQ)
