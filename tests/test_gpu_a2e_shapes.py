"""soc_a2e_dosolve_kernel against the oracle at every launch shape the launcher can choose: the <4>, <2> and <1> instances (cells
per workgroup), 256 and 1024 threads, one to five row blocks with a last block that is partly filled, the rescaling branch in
every block, ragged batches, the accumulate path of the resident calls, the edges of NFREQ and of the LDS.

Every comparison is the standard of this kernel: the oracle's bits wherever the oracle is finite and its finite / non-finite
pattern (util.same_bits); no tolerance.  tests/test_a2e_shapes.py asserts on the CPU that the inputs used here reach the branches
they are meant to reach; the cases and inputs are those of tests/a2e_rows.py."""
import numpy as np
import pytest

import a2e_rows as R
from soc_amd.lib import SocError
from util import same_bits

pytestmark = pytest.mark.gpu

TABLE_CASES = [(NE, 50, C) for NE, (C, _) in R.TABLE.items()]
EDGE_CASES = [(NE, NF, C) for (NE, NF), C in R.NFREQ_EDGES.items()]


def _set_size(engine, NE, NFREQ, isize):
    sol, AF = R.solver(NE, NFREQ)
    engine.a2e_set_size(NE, NFREQ, sol["sizes"][isize], AF[isize])


def _check_case(engine, orc, NE, NFREQ, C, cuts=True):
    """both sizes of the solver in turn: the full batch of 4*C + 3 cells, then batches of 1, C-1, C and C+1 cells cut from it"""
    ABS, _ = R.absorptions(NE, NFREQ, C)
    for isize in range(2):
        want = R.oracle_emission(orc, NE, NFREQ, C, isize)
        _set_size(engine, NE, NFREQ, isize)
        assert engine.a2e_launch_shape()[0] == C
        got = engine.a2e_solve(ABS)
        assert np.isfinite(got).all()
        assert same_bits(got, want), "NE %d NFREQ %d size %d: cells %s differ" % (
            NE, NFREQ, isize, [c for c in range(len(want)) if not same_bits(got[c], want[c])])
        if cuts:
            for n in sorted({1, C - 1, C, C + 1} - {0}):
                for c0 in (1, ABS.shape[0] - n):                # (not at a multiple of C: other waves than in the full batch)
                    assert same_bits(engine.a2e_solve(ABS[c0:c0 + n]), want[c0:c0 + n]), (NE, isize, n, c0)


@pytest.mark.parametrize("NE,NFREQ,C", TABLE_CASES)
def test_dosolve_equals_the_oracle_at_every_launch_shape(NE, NFREQ, C, engine, oracle_soc):
    _check_case(engine, oracle_soc, NE, NFREQ, C)
    assert engine.a2e_launch_shape()[:2] == R.TABLE[NE]


def _empty_size(engine, NE, NFREQ):
    """set_size with tables whose windows are all empty: valid, and nothing is launched"""
    size = dict(Iw=np.zeros(0, np.float32), L1=np.ones(NE * NE, np.int32), L2=np.zeros(NE * NE, np.int32),
                Tdown=np.ones(NE, np.float32), EA=np.zeros(NE * NFREQ, np.float32), Ibeg=np.zeros(NFREQ, np.int32))
    engine.a2e_set_size(NE, NFREQ, size, np.ones(NFREQ, np.float32))


def test_every_reachable_variant_has_a_case(engine):
    """The (C, T) pairs are read from the launcher for every accepted NE at NFREQ 50, not computed from a copy of its rule; the
    table must reach every one of them, with the C and T it states."""
    def shape(NE):
        _empty_size(engine, NE, 50)
        return engine.a2e_launch_shape()
    seen = {}
    for NE in range(3, 281):
        C, T, lds = shape(NE)
        assert C in (4, 2, 1) and T in (256, 1024) and 0 < lds <= 160 * 1024
        seen.setdefault((C, T), []).append(NE)
    for NE, want in R.TABLE.items():
        assert shape(NE)[:2] == want, "NE %d is launched as %s now, the table says %s: move the case" % (NE, shape(NE)[:2], want)
    assert set(seen) == set(R.TABLE.values()), "a (C, T) pair without a case: %s" % {k: (v[0], v[-1]) for k, v in seen.items()}
    for (C, T), nes in seen.items():                            # the first and the last size of every pair are cases
        assert nes[0] in R.TABLE and nes[-1] in R.TABLE and nes == list(range(nes[0], nes[-1] + 1)), (C, T, nes[0], nes[-1])


def test_dosolve_where_values_leave_fp32(engine, oracle_soc):
    """rows base * 10**k, k = 11 .. 16: the oracle's finite values to the bit, its infinities and NaNs where it has them"""
    ABS = R.overflow_absorptions()
    for isize in range(2):
        want = R.oracle_emission(oracle_soc, R.OVERFLOW_NE, 50, 1, isize, True)
        _set_size(engine, R.OVERFLOW_NE, 50, isize)
        assert same_bits(engine.a2e_solve(ABS), want)


def test_set_size_replaces_the_tables_of_another_shape(engine, oracle_soc):
    """from a C = 1 size to a C = 4 size and back, then C = 2: every table, the LDS attribute and the launch shape are the new size's"""
    for NE in (280, 3, 280, 100, 202, 143, 65):
        _check_case(engine, oracle_soc, NE, 50, R.TABLE[NE][0], cuts=False)
        assert engine.a2e_launch_shape()[:2] == R.TABLE[NE]


@pytest.mark.parametrize("NE,NFREQ,C", EDGE_CASES)
def test_dosolve_at_the_edges_of_nfreq(NE, NFREQ, C, engine, oracle_soc):
    _check_case(engine, oracle_soc, NE, NFREQ, C)


def _largest_nfreq(engine, NE):
    """the largest NFREQ soc_a2e_set_size accepts at this NE, asked of the library (bisection over its refusals)"""
    lo, hi = 2, 1 << 14                                         # accepted, refused
    with pytest.raises(SocError, match="bytes of LDS"):
        _empty_size(engine, NE, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        try:
            _empty_size(engine, NE, mid)
            lo = mid
        except SocError:
            hi = mid
    return lo


def test_the_lds_boundary(engine, oracle_soc):
    NE = 280
    NFREQ = _largest_nfreq(engine, NE)
    assert NFREQ == 810                                         # 4*((NE^2-NE)/2 + NE + NFREQ) + 4*NFREQ <= 160 KB
    _check_case(engine, oracle_soc, NE, NFREQ, 1)
    assert engine.a2e_launch_shape() == (1, 1024, 160 * 1024)   # the whole LDS of the CU
    # one frequency more: refused by set_size, nothing launched; the size before stays and still solves
    ABS, _ = R.absorptions(NE, NFREQ, 1)
    with pytest.raises(SocError, match=r"NE = 280 with NFREQ = 811 needs 163848 bytes of LDS for one cell, the limit is 163840"):
        _empty_size(engine, NE, NFREQ + 1)
    assert engine.a2e_launch_shape() == (1, 1024, 160 * 1024)
    assert same_bits(engine.a2e_solve(ABS), R.oracle_emission(oracle_soc, NE, NFREQ, 1, 1))
    _check_case(engine, oracle_soc, 100, 50, 4, cuts=False)


def test_launch_shape_before_any_size():
    from soc_amd.lib import Engine
    eng = Engine(0)
    try:
        with pytest.raises(SocError, match="soc_a2e_set_size first"):
            eng.a2e_launch_shape()
    finally:
        eng.close()


@pytest.mark.parametrize("NE", sorted(R.RESIDENT))
def test_resident_cells_accumulate_the_sizes_to_the_bit(NE, engine, oracle_soc):
    """begin / upload in two chunks at an odd offset / set_size + resident_solve for two sizes / download against
    a2e_solve(size 0) + a2e_solve(size 1) added in fp32 on the host, in that order -- and both against the oracle"""
    from oracle.pyoracle import a2e_oracle_dosolve
    C = R.RESIDENT[NE]
    sol, AF = R.solver(NE)
    ABS = R.resident_absorptions(NE)                            # 8*C + 5 cells
    parts = []
    for isize in range(2):
        _set_size(engine, NE, 50, isize)
        assert engine.a2e_launch_shape()[0] == C
        parts.append(engine.a2e_solve(ABS))
        assert same_bits(parts[-1], a2e_oracle_dosolve(oracle_soc, NE, 50, sol["sizes"][isize], AF[isize], ABS))
    want = parts[0] + parts[1]
    assert want.dtype == np.float32 and np.isfinite(want).all() and (parts[1] > 0).any()
    engine.a2e_resident_begin(ABS.shape[0], 50)
    try:
        engine.a2e_resident_upload(0, ABS[:5])
        engine.a2e_resident_upload(5, ABS[5:])
        for isize in range(2):
            _set_size(engine, NE, 50, isize)
            engine.a2e_resident_solve()
        got = engine.a2e_resident_download(0, ABS.shape[0])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(engine.a2e_resident_download(3, 2 * C + 1).view(np.uint32), want[3:2 * C + 4].view(np.uint32))
    finally:
        engine.a2e_resident_end()
