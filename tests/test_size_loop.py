"""The calls that solve one solver file's grain sizes on resident cells, as soc_amd.a2e.run and the device branch of
soc_amd.mabu.solve_emission issue them, without a GPU: a wrapper records every a2e_* / mabu_* call of the two programs on engines
that only stand in for the device, the sequences are compared with the literal ones, and the per-size part of the two with each
other.  Only the public entry points are used: a2e.run and mabu.solve_emission."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import a2e, mabu, synth                  # noqa: E402
from test_mabu import ResidentStandIn                 # noqa: E402

CELLS, NFREQ, NSIZE = 5, 7, 3
PER_SIZE = ("a2e_set_size", "a2e_set_size_aalg", "a2e_resident_solve", "a2e_set_eq_sizes", "a2e_resident_solve_eq")


class Recorder:
    """an engine that hands every attribute of `engine` through (so a probe with hasattr sees what the engine has) and logs the calls
    named a2e_* or mabu_* as (name, what): the size of a2e_set_size and a2e_set_size_aalg, the tuple of the sizes of
    a2e_set_eq_sizes -- both read back from the tables handed over --, None for every other call"""

    def __init__(self, engine, sol):
        self.engine, self.sol, self.log = engine, sol, []
        self.AF = [synth.a2e_absorption_fraction(sol, i) for i in range(sol["NSIZE"])]
        assert all(not np.array_equal(self.AF[i], self.AF[j]) for i in range(NSIZE) for j in range(i))

    def what(self, name, args):
        if name == "a2e_set_size":                    # (NE, NFREQ, the size's tables, AF)
            return [i for i, s in enumerate(self.sol["sizes"]) if np.array_equal(s["Tdown"], args[2]["Tdown"])
                    and np.array_equal(self.AF[i], args[3])][0]
        if name == "a2e_set_size_aalg":               # (ASIZE, isize)
            assert np.array_equal(args[0], self.sol["SIZE_A"])
            return int(args[1])
        if name == "a2e_set_eq_sizes":                # (NIP, FACTOR, FREQ, AF[nsizes, NFREQ], ...)
            return tuple([i for i, af in enumerate(self.AF) if np.array_equal(af, row)][0] for row in args[3])
        return None

    def __getattr__(self, name):
        f = getattr(self.engine, name)
        if not (name.startswith("a2e_") or name.startswith("mabu_")):
            return f

        def call(*args, **kw):
            self.log.append((name, self.what(name, args)))
            return f(*args, **kw)
        return call


class ResidentA2E:
    """what a2e.run needs of an engine to keep the cells resident, the equilibrium sizes included; nothing is computed"""

    def a2e_resident_begin(self, cells, NFREQ, polarised=False):
        self.NFREQ = NFREQ

    def a2e_resident_download(self, c0, n, out=None):
        return np.zeros((n, self.NFREQ), np.float32)

    a2e_resident_download_p = a2e_resident_download

    def _nothing(self, *a):
        pass

    a2e_resident_upload = a2e_resident_upload_aalg = a2e_set_size = a2e_set_size_aalg = a2e_resident_solve = _nothing
    a2e_set_eq_sizes = a2e_resident_solve_eq = a2e_resident_end = _nothing


class ResidentMabu(ResidentStandIn):
    """the stand-in of tests/test_mabu.py with the calls of the polarised sum and of the equilibrium sizes, which compute nothing"""

    def mabu_begin(self, cells, NFREQ, NDUST, polarised=False):
        ResidentStandIn.mabu_begin(self, cells, NFREQ, NDUST)

    def mabu_download_p(self, c0, n, out=None):
        out[:] = 0.0
        return out

    def _nothing(self, *a):
        pass

    a2e_set_size_aalg = a2e_set_eq_sizes = a2e_resident_solve_eq = a2e_resident_upload_aalg = _nothing
    mabu_pol_eq = mabu_accumulate_p = mabu_ratio = _nothing


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a synthetic solver with three sizes, as a dict and as the file of a stochastically heated dust, with and without `nstoch 2`"""
    d = str(tmp_path_factory.mktemp("size_loop"))
    sol = synth.synth_solver(NFREQ=NFREQ, NE=16, NSIZE=NSIZE, seed=5)
    rng = np.random.default_rng(3)
    FABS = (rng.uniform(0.1, 1.0, (CELLS, NFREQ)) * 1.0e-6).astype(np.float32)
    aalg = np.asarray(sol["SIZE_A"][1] * rng.uniform(0.5, 2.0, CELLS), np.float32)
    with open(os.path.join(d, "pah.aalg"), "wb") as fp:
        np.asarray([CELLS], np.int32).tofile(fp)
        aalg.tofile(fp)
    dusts = {}
    for tag, lines in (("all", ""), ("two", "nstoch 2\n")):
        os.makedirs(os.path.join(d, tag))
        synth.write_solver(os.path.join(d, tag, "pah.solver"), sol)
        dusts[tag] = os.path.join(d, tag, "gs_pah.dust")
        with open(dusts[tag], "w") as fp:
            fp.write("gsetdust\n" + lines)
    return dict(sol=sol, FABS=FABS, aalg=aalg, aalg_file=os.path.join(d, "pah.aalg"), dusts=dusts)


def traces(case, tag, NSTOCH, polarised):
    """the calls of a2e.run and of mabu.solve_emission (one dust, one cell range) for the same solver"""
    one = Recorder(ResidentA2E(), case["sol"])
    a2e.run(one, case["sol"], case["FABS"], NSTOCH=NSTOCH, verbose=False, aalg=case["aalg"] if polarised else None)
    two = Recorder(ResidentMabu(10 ** 9), case["sol"])
    _, info = mabu.solve_emission(two, [case["dusts"][tag]], ['gsetdust'], case["FABS"], np.ones((CELLS, 1), np.float32),
                                  pol=[case["aalg_file"]] if polarised else None)
    assert info["path"] == "device" and info["ranges"] == 1
    return one.log, two.log


def stochastic(isize, polarised=False):
    return [("a2e_set_size", isize)] + ([("a2e_set_size_aalg", isize)] if polarised else []) + [("a2e_resident_solve", None)]


def plain(*names):
    return [(n, None) for n in names]


def test_all_sizes_stochastic(case):
    run, stage = traces(case, "all", 999, False)
    sizes = stochastic(0) + stochastic(1) + stochastic(2)
    assert run == plain("a2e_resident_begin", "a2e_resident_upload") + sizes + plain("a2e_resident_download", "a2e_resident_end")
    assert stage == plain("mabu_begin", "mabu_upload", "mabu_set_tables", "mabu_split") + sizes + \
        plain("mabu_accumulate", "mabu_download", "mabu_end")


def test_the_last_size_an_equilibrium_size(case):
    run, stage = traces(case, "two", 2, False)
    sizes = stochastic(0) + stochastic(1) + [("a2e_set_eq_sizes", (2,)), ("a2e_resident_solve_eq", None)]
    assert run == plain("a2e_resident_begin", "a2e_resident_upload") + sizes + plain("a2e_resident_download", "a2e_resident_end")
    assert stage == plain("mabu_begin", "mabu_upload", "mabu_set_tables", "mabu_split") + sizes + \
        plain("mabu_accumulate", "mabu_download", "mabu_end")


def test_the_last_size_an_equilibrium_size_polarised(case):
    run, stage = traces(case, "two", 2, True)
    sizes = stochastic(0, True) + stochastic(1, True) + [("a2e_set_eq_sizes", (2,)), ("a2e_resident_solve_eq", None)]
    assert run == plain("a2e_resident_begin", "a2e_resident_upload", "a2e_resident_upload_aalg") + sizes + \
        plain("a2e_resident_download", "a2e_resident_download_p", "a2e_resident_end")
    assert stage == plain("mabu_begin", "mabu_upload", "mabu_set_tables", "mabu_split", "a2e_resident_upload_aalg") + sizes + \
        plain("mabu_accumulate", "mabu_accumulate_p", "mabu_ratio", "mabu_download", "mabu_download_p", "mabu_end")


@pytest.mark.parametrize("tag, NSTOCH, polarised", [("all", 999, False), ("all", 999, True), ("two", 2, False), ("two", 2, True)])
def test_the_two_programs_issue_the_same_calls_per_size(case, tag, NSTOCH, polarised):
    run, stage = traces(case, tag, NSTOCH, polarised)
    per_size = [x for x in run if x[0] in PER_SIZE]
    assert per_size == [x for x in stage if x[0] in PER_SIZE]
    assert len(per_size) == (2 + polarised) * min(NSTOCH, NSIZE) + 2 * (NSTOCH < NSIZE)
