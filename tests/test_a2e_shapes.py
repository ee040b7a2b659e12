"""What the inputs of tests/test_gpu_a2e_shapes.py must be for those tests to mean something, asserted on the CPU with the oracle
and the row finder of tests/a2e_rows.py only: the rescaling branch of DoSolve's forward substitution is taken in every row block,
at the first and the last row of a block, at the last row of the matrix and in consecutive rows; the expected values are finite
where the case says so; faint rows run through fp32 denormals.  A kernel that is wrong in one of these places then differs from
the oracle in a GPU test; without them it could be wrong there and equal everywhere it is looked at."""
import numpy as np
import pytest

import a2e_rows as R
from util import same_bits

TABLE_CASES = [(NE, 50, C) for NE, (C, _) in R.TABLE.items()]
EDGE_CASES = [(NE, NF, C) for (NE, NF), C in R.NFREQ_EDGES.items()]
FLT_MIN = np.float32(1.1754944e-38)


def _rows(NE, NFREQ=50, C=None):
    """the rescale rows of every cell of a case, both sizes of the solver"""
    C = R.TABLE[NE][0] if C is None else C
    return [r for isize in range(2) for r in R.case_rows(NE, NFREQ, C, isize)[0]]


@pytest.mark.parametrize("NE", [16, 100])
def test_the_finder_reaches_the_oracles_bits(NE, oracle_soc):
    """its XL pushed through the emission sum: only then are its row lists those of the oracle's own loop"""
    C = 4                                                    # 19 cells (NE 16 is no case of the table)
    for isize in range(2):
        sol, _ = R.solver(NE)
        rows, _, XL = R.case_rows(NE, 50, C, isize)
        want = R.oracle_emission(oracle_soc, NE, 50, C, isize)
        assert np.isfinite(want).all() and any(rows)
        assert same_bits(R.emission(NE, 50, sol["sizes"][isize], XL), want)


def test_the_finder_reaches_the_oracles_bits_where_values_overflow(oracle_soc):
    sol, _ = R.solver(R.OVERFLOW_NE)
    for isize in range(2):
        _, _, XL = R.case_rows(R.OVERFLOW_NE, 50, 1, isize, True)
        assert same_bits(R.emission(R.OVERFLOW_NE, 50, sol["sizes"][isize], XL),
                         R.oracle_emission(oracle_soc, R.OVERFLOW_NE, 50, 1, isize, True))


def test_the_cases_are_the_stated_ones():
    assert sorted(R.TABLE) == [3, 65, 70, 71, 100, 129, 142, 143, 193, 201, 202, 256, 280]
    for NE, NFREQ, C in TABLE_CASES + EDGE_CASES:
        ABS, ks = R.absorptions(NE, NFREQ, C)
        assert ABS.shape == (4 * C + 3, NFREQ) and (C == 1 or ABS.shape[0] % C != 0)       # a last workgroup that is not full
        grid = [k for k in ks if k is not None]
        assert grid[0] == -14 and grid[-1] == R.K_TOP_AT.get((NE, NFREQ), R.K_TOP) and sorted(set(grid)) == grid
        assert not ABS[len(grid)].any() and len(ks) - len(grid) - 1 >= 1       # the zero row, at least one lognormal row
        assert np.isfinite(ABS).all() and (ABS >= 0).all()


@pytest.mark.parametrize("NE,NFREQ,C", TABLE_CASES + EDGE_CASES + [(280, 810, 1)])
def test_the_oracle_is_finite_and_non_negative_up_to_the_top_of_the_grid(NE, NFREQ, C, oracle_soc):
    """k <= K_TOP = 10 everywhere but at NE 143 / NFREQ 130 and NE 280 / NFREQ 810, where base * 1e10 is non-finite in the
    oracle at size 1: the grid ends at k = 9 there (K_TOP_AT), and only there"""
    from oracle.pyoracle import a2e_oracle_dosolve
    for isize in range(2):
        e = R.oracle_emission(oracle_soc, NE, NFREQ, C, isize)
        assert np.isfinite(e).all() and (e >= 0).all()
        assert e[:-1].max() > 0
    if (NE, NFREQ) in R.K_TOP_AT:
        sol, AF = R.solver(NE, NFREQ)
        ten = (R.base_row(NFREQ) * 10.0 ** R.K_TOP).astype(np.float32)[None]
        assert not np.isfinite(a2e_oracle_dosolve(oracle_soc, NE, NFREQ, sol["sizes"][1], AF[1], ten)).all()


@pytest.mark.parametrize("NE", sorted(R.RESIDENT))
def test_the_resident_cases_are_finite_and_rescale_in_every_block(NE, oracle_soc):
    """the inputs of the accumulate path: both sizes and their fp32 sum finite in the oracle, rescales in every row block"""
    from oracle.pyoracle import a2e_oracle_dosolve
    sol, AF = R.solver(NE)
    ABS = R.resident_absorptions(NE)
    assert ABS.shape[0] == 8 * R.RESIDENT[NE] + 5
    e = [a2e_oracle_dosolve(oracle_soc, NE, 50, sol["sizes"][isize], AF[isize], ABS) for isize in range(2)]
    assert np.isfinite(e[0] + e[1]).all() and (e[0] >= 0).all() and (e[1] >= 0).all() and (e[0] > 0).any() and (e[1] > 0).any()
    for isize in range(2):
        rows = R.find_rows(NE, 50, sol["sizes"][isize], AF[isize], ABS)[0]
        assert {j // 64 for r in rows for j in r} == set(range((NE + 63) // 64))


@pytest.mark.parametrize("NE", [NE for NE in R.TABLE if NE > 64])
def test_some_cell_rescales_in_every_row_block(NE):
    C = R.TABLE[NE][0]
    for isize in range(2):
        hit = {j // 64 for r in R.case_rows(NE, 50, C, isize)[0] for j in r}
        assert hit == set(range((NE + 63) // 64))
    if NE == 280:
        assert any(j >= 256 for r in _rows(280) for j in r)                    # the fifth block, of 24 rows


def test_rescales_at_the_edges_of_blocks_and_of_the_matrix():
    rows = {NE: _rows(NE) for NE in R.TABLE}
    every = {j for rs in rows.values() for r in rs for j in r}
    assert every & {64, 128, 192, 256} == {64, 128, 192, 256}                  # k = 0 of a block that is not the first
    assert every & {127, 191} == {127, 191}                                    # k = 63 of such a block
    for NE in (65, 129, 193):                                                  # the block of one row: that row rescales
        assert any(NE - 1 in r for r in rows[NE])
    assert any(279 in r for r in rows[280])                                    # the last row of the matrix, in a short last block
    for NE in R.TABLE:
        if NE > 64:
            assert any(a + 1 == b for r in rows[NE] for a, b in zip(r, r[1:]))  # two in consecutive rows
            assert any(not r for r in rows[NE])                                # a cell that never rescales
    assert any(a + 1 == b and a >= 64 for r in rows[280] for a, b in zip(r, r[1:]))    # consecutive rows below the first block
    assert not any(rows[3])                                                    # (NE 3: XL[1], XL[2] stay far below 1e20)


def test_a_faint_row_runs_through_denormals():
    """a denormal XL entry before normalisation, in a cell of the k grid with k < 0, at every size of the table but NE 3"""
    for NE, (C, _) in R.TABLE.items():
        if NE == 3:
            continue
        ks = R.absorptions(NE, 50, C)[1]
        for isize in range(2):
            raw = R.case_rows(NE, 50, C, isize)[1]
            den = (raw != 0) & (np.abs(raw) < FLT_MIN)
            assert any(den[c].any() for c, k in enumerate(ks) if k is not None and k < 0)


def test_the_overflow_case_overflows_and_not_everywhere(oracle_soc):
    """k = 11 .. 16 at NE 280: at size 0 the cells k = 11, 12, 13 are finite at every frequency, the others at none; at size 1
    none is.  The rescales go on into the fifth block before the values leave fp32's range."""
    e = np.stack([R.oracle_emission(oracle_soc, R.OVERFLOW_NE, 50, 1, isize, True) for isize in range(2)])
    assert e.shape == (2, len(R.OVERFLOW_K), 50)
    fin = np.isfinite(e)
    assert fin.all(axis=2).any() and not fin.all()
    assert (e[fin] >= 0).all()
    assert all(r and r[-1] >= 256 for isize in range(2) for r in R.case_rows(R.OVERFLOW_NE, 50, 1, isize, True)[0])
