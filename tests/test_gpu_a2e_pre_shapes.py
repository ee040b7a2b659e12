"""soc_pre_weights_kernel and soc_pre_cooling_kernel against the oracle at the sizes the solver runs at and at the edges of their
loops and of their launcher: second and later passes of upper bins (NE 66 .. 280; the carried count `filled`, the LDS columns and
the scan used again), second and later passes of frequency intervals (NFREQ 130 .. 639), the LDS attribute (NFREQ >= 256) and
the LDS limit (NFREQ 639), the smallest sizes, grids with uneven frequencies, a narrow bin, pairs no frequency feeds and no window
at all; then the tables the device built through the device solver.

Windows, counts and weights are the oracle's to the bit; the cooling rates go through the device's double exp() and another
order of summation and are held to rtol 1e-6 (the bound of tests/test_a2e_pre.py).  tests/test_a2e_pre_shapes.py asserts on the
CPU that the cases reach what they are meant to reach and that the oracle equals the reference there; the cases are those of
tests/a2e_pre_shapes.py."""
import numpy as np
import pytest

import a2e_pre_shapes as S
from soc_amd import a2e_pre, synth
from soc_amd.lib import SocError
from util import same_bits

pytestmark = pytest.mark.gpu

TDOWN_RTOL = 1e-6
_single = {}                       # name -> the result of the first call for this case in this process


def _pre(engine, name):
    return engine.a2e_pre(*S.inputs(name), S.FACTOR)


def _first(engine, name):
    if name not in _single:
        _single[name] = _pre(engine, name)
    return _single[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(got, want, name):
    """windows, counts and weights to the bit, cooling rates within the bound; returns the largest relative difference of Tdown"""
    NFREQ, NE = S.shape(name)
    for key in ("L1", "L2", "noIw"):
        bad = np.nonzero(got[key] != want[key])[0]
        assert bad.size == 0, "%s: %s differs first at (l, u) = %s: %d, oracle %d" % (
            name, key, divmod(int(bad[0]), NE) if key != "noIw" else int(bad[0]), got[key][bad[0]], want[key][bad[0]])
    assert S.first_difference(got, want, NE) is None, "%s: Iw differs first in the window of (l, u) = %s" % (name, S.first_difference(got, want, NE))
    assert got["Iw"].dtype == np.float32 and np.array_equal(_bits(got["Iw"]), _bits(want["Iw"]))
    a, b = got["Tdown"].astype(np.float64), want["Tdown"].astype(np.float64)
    assert np.isfinite(a).all() and a[0] == 0.0
    rel = float(np.max(np.abs(a - b) / np.where(b != 0.0, np.abs(b), 1.0)))      # (where the oracle has 0 the difference itself)
    print("a2e_pre %-7s NFREQ %3d NE %3d  max |Tdown - oracle| / oracle = %.3e" % (name, NFREQ, NE, rel))
    assert np.allclose(got["Tdown"], want["Tdown"], rtol=TDOWN_RTOL, atol=0.0), "%s: Tdown differs by %.3e (bin %d)" % (
        name, rel, int(np.argmax(np.abs(a - b) / np.where(b != 0.0, np.abs(b), 1.0))))
    return rel


def _same_call(got, want, name):
    """two calls of the library on the same input: every array to the bit, the cooling rates too"""
    for key in ("L1", "L2", "noIw", "Iw", "Tdown"):
        assert np.array_equal(_bits(got[key]), _bits(want[key])), (name, key)


@pytest.mark.parametrize("name", S.NAMES)
def test_pre_equals_the_oracle(name, engine, oracle_soc):
    _check(_first(engine, name), S.oracle(oracle_soc, name), name)


def test_sizes_in_turn_on_one_handle(engine, oracle_soc):
    """the LDS attribute is set on the kernel for one call (160 KB, then 64.25 KB, and the other way round) with a call below
    64 KB between them: every result is that of the case called alone, and the oracle's"""
    order = ("nf639", "small", "nf256")
    alone = {name: _first(engine, name) for name in order}
    for name in order + order[::-1]:
        got = _pre(engine, name)
        _same_call(got, alone[name], name)
        _check(got, S.oracle(oracle_soc, name), name)


def test_one_frequency_too_many_is_refused_by_name(engine, oracle_soc):
    assert S.shape("nf640") == (S.NFREQ_MAX + 1, 8)
    with pytest.raises(SocError, match=r"NFREQ = 640, the limit is 639.*LDS"):
        _pre(engine, "nf640")
    got = _pre(engine, "small")                                 # the handle is as good as before
    _check(got, S.oracle(oracle_soc, "small"), "small")
    _same_call(got, _first(engine, "small"), "small")


@pytest.mark.parametrize("NE", S.SOLVER_NE)
def test_device_built_tables_through_the_device_solver(NE, engine, oracle_soc):
    """make_solver with the engine against make_solver with the oracle, then the engine's own tables through soc_a2e_set_size
    (its host validation of windows against weights takes real preprocessing output) and DoSolve, against the oracle's
    DoSolve on the same tables: real windows reach over the whole frequency axis and about half of the pairs are empty"""
    from oracle.pyoracle import a2e_oracle_dosolve
    want, _ = S.oracle_solver(oracle_soc, NE)
    got = a2e_pre.make_solver(a2e_pre.AnalyticDust(NSIZE=3), S.standard_freq(50), NE, engine)
    ABS = S.solver_absorptions()
    assert got["NE"] == NE and got["NFREQ"] == 50 and got["NSIZE"] == 3
    for isize in range(3):
        a, b = got["sizes"][isize], want["sizes"][isize]
        for key in ("Iw", "L1", "L2", "EA", "Ibeg"):
            assert a[key].size == b[key].size and np.array_equal(_bits(a[key]), _bits(b[key])), (isize, key)
        assert np.allclose(a["Tdown"], b["Tdown"], rtol=TDOWN_RTOL, atol=0.0), isize
        AF = synth.a2e_absorption_fraction(got, isize)
        engine.a2e_set_size(NE, 50, a, AF)
        assert engine.a2e_launch_shape()[0] == {128: 4, 256: 1}[NE]
        em = engine.a2e_solve(ABS)
        ref = a2e_oracle_dosolve(oracle_soc, NE, 50, a, AF, ABS)
        assert np.isfinite(ref).all() and np.isfinite(em).all() and (em >= 0).all()
        assert not em[-1].any() and em[:-1].any(axis=1).all()   # the zero row gives zero, every other row emits
        assert same_bits(em, ref), "NE %d size %d: cells %s differ" % (NE, isize, [c for c in range(len(ref)) if not same_bits(em[c], ref[c])])
