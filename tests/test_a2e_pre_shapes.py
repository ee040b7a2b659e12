"""What the cases of tests/test_gpu_a2e_pre_shapes.py must be for those tests to mean something, asserted on the CPU from the
oracle's output and the cases of tests/a2e_pre_shapes.py only: the later passes of the weights kernel's loop over upper bins hold
non-empty windows, and lower bins have windows both in the first and in a later pass (the carried count `filled` places the
later ones); the LDS of the weights kernel is below, at and above the sizes the launcher treats differently; the later passes of
the cooling kernel's loop over frequency intervals carry weight in the cooling rates; the grids that are meant to have empty
pairs, a narrow bin or no window at all have them.  A kernel that is wrong in one of these places then differs from the oracle in
a GPU test; without them it could be wrong there and equal everywhere it is looked at."""
import numpy as np
import pytest

import a2e_pre_shapes as S
from oracle.pyoracle import RefA2EPre, a2e_oracle_pre

KEYS = ("L1", "L2", "noIw", "Iw", "Tdown")


def _ref_available():
    try:
        RefA2EPre()
        return True
    except (FileNotFoundError, OSError):
        return False


def test_the_cases_are_the_stated_ones():
    assert [S.STANDARD[n] for n in S.STANDARD] == [(50, 65, 1), (50, 66, 1), (50, 128, 1), (50, 256, 0), (70, 130, 1), (50, 280, 1),
                                                   (130, 24, 0), (255, 12, 0), (256, 12, 0), (639, 8, 0), (2, 3, 1), (3, 2, 1)]
    assert [S.RANDOM[n] for n in S.RANDOM] == [(90, 150), (140, 70), (300, 30)]
    for name in S.STANDARD:
        assert S.shape(name) == S.STANDARD[name][:2]
    for name in S.RANDOM:
        assert S.shape(name) == S.RANDOM[name]                # (np.unique dropped no frequency)
    assert S.shape(S.EMPTY) == (8, 10)
    for name in S.NAMES:
        FREQ, Ef, SK, E, T = S.inputs(name)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in (FREQ, Ef, SK, E, T))
        assert (np.diff(FREQ) > 0).all() and (np.diff(Ef) > 0).all() and (np.diff(E) > 0).all()      # what soc_a2e_pre asks for
        assert Ef.size == FREQ.size == SK.size and T.size == E.size
        assert 2 <= FREQ.size <= S.NFREQ_MAX and 2 <= E.size - 1 <= 280


@pytest.mark.parametrize("name", S.NAMES)
def test_the_oracle_output_is_a_valid_size(name, oracle_soc):
    """the layout the comparisons of the GPU test rely on: noIw[l] is the sum of l's window lengths, every weight is positive at
    the ends of its window, the cooling rates are finite (not positive: where every frequency lies above the bin centres the
    reference integrates the first interval backwards, and the oracle follows it)"""
    NFREQ, NE = S.shape(name)
    k = S.oracle(oracle_soc, name)
    l, u, n = S.windows(k, NE)
    assert (n >= 0).all() and (n <= NFREQ).all() and n.sum() == k["Iw"].size
    assert np.array_equal(np.bincount(l, weights=n, minlength=NE - 1).astype(np.int64), k["noIw"])
    off = np.cumsum(n) - n
    on = n > 0
    assert (k["Iw"][off[on]] > 0).all() and (k["Iw"][off[on] + n[on] - 1] > 0).all()
    assert np.isfinite(k["Iw"]).all() and np.isfinite(k["Tdown"]).all() and k["Tdown"][0] == 0.0
    assert name == S.EMPTY or (k["Tdown"][1:] > 0).all()


def test_the_passes_of_the_weights_kernel(oracle_soc):
    """non-empty windows per pass (u - l - 1) // 64 and lower bins whose non-empty windows span passes"""
    def passes(name):
        return S.passes(S.oracle(oracle_soc, name), S.shape(name)[1])
    assert passes("ne65") == ([1087], 0)                        # one pass
    counts, _ = passes("ne66")                                  # a second pass of one lane: the pair (0, 65)
    assert len(counts) == 2 and counts[0] > 0
    assert passes("ne130") == ([3879, 406, 0], 28)
    assert passes("ne280") == ([10569, 6655, 2528, 28, 0], 137)
    for name in ("ne128", "ne256", "ne130", "ne280"):
        counts, spans = passes(name)
        assert counts[0] > 0 and counts[1] > 0 and spans >= 1, name
    assert len(passes("ne128")[0]) == 2 and len(passes("ne256")[0]) == 4
    # windows of the full length NFREQ (the whole LDS column of a lane is copied out) at three passes
    NFREQ, NE = S.shape("ne130")
    assert int((S.windows(S.oracle(oracle_soc, "ne130"), NE)[2] == NFREQ).sum()) == 6
    # a second pass of a lower bin l starts behind l's first pass: its place is the carried count, not 0
    k = S.oracle(oracle_soc, "ne130")
    l, u, n = S.windows(k, NE)
    first = np.bincount(l[(u - l - 1) < S.PRE_T], weights=n[(u - l - 1) < S.PRE_T], minlength=NE - 1)
    later = np.bincount(l[(u - l - 1) >= S.PRE_T], weights=n[(u - l - 1) >= S.PRE_T], minlength=NE - 1)
    assert ((first > 0) & (later > 0)).sum() == 28 and np.array_equal((first + later).astype(np.int64), k["noIw"])


def test_the_lds_of_the_weights_kernel():
    """(NFREQ * 64 + 64) * 4 bytes as soc_launch_a2e_pre computes them: the attribute above 64 KB, the limit at 160 KB"""
    assert S.lds_bytes(255) == S.LDS_DEFAULT                    # the last size without the attribute: exactly 64 KB
    assert S.lds_bytes(256) == S.LDS_DEFAULT + 256              # the first with it
    assert S.lds_bytes(S.NFREQ_MAX) == S.LDS_LIMIT == 163840    # exactly the LDS of a workgroup
    assert S.lds_bytes(S.NFREQ_MAX + 1) > S.LDS_LIMIT
    for name in S.NAMES:
        assert S.lds_bytes(S.shape(name)[0]) <= S.LDS_LIMIT
    with_attribute = sorted(n for n in S.NAMES if S.lds_bytes(S.shape(n)[0]) > S.LDS_DEFAULT)
    assert with_attribute == ["nf256", "nf639", "rnd30"]


def test_the_later_intervals_carry_weight_in_the_cooling_rates(oracle_soc):
    """Tdown is compared with a tolerance (1e-6), so an error in a later pass of the cooling kernel's interval loop
    (i = lane + 64, lane + 128) shows only where those intervals carry weight.  At (130, 24, 0) they do: with SKABS[64:] = 0
    more than half of the bins change by more than 10 % (16 of 23).  (Its bins take one or two passes; a third and later pass
    is taken at NFREQ 255, 256, 639 and on the random grids, and is held to the same condition there with SKABS[128:] = 0.)  At NFREQ = 66 or 70 the intervals from 64 on lie so far in
    the Wien tail of every bin of the standard grids that the same change moves no rate by more than 2e-4 (most by nothing):
    a second pass wrong by a percent would stay below the bound, which is why those sizes are not the cooling cases."""
    def changed(name, first_zero):
        FREQ, Ef, SK, E, T = S.inputs(name)
        want = S.oracle(oracle_soc, name)["Tdown"]
        cut = SK.copy()
        cut[first_zero:] = 0.0
        got = a2e_oracle_pre(oracle_soc, FREQ, Ef, cut, E, T, S.FACTOR)["Tdown"]
        assert (want[1:] > 0).all()
        change = np.abs(got[1:] - want[1:]) / want[1:]
        return int((change > 0.10).sum()), change.size
    assert S.shape("nf130")[0] - 1 > 2 * S.PRE_T                # room for three passes of the interval loop ...
    assert np.bincount(S.interval_passes("nf130")).tolist() == [0, 7, 16]     # ... of which the bins of this grid take one or two:
    more, bins = changed("nf130", S.PRE_T)                      # their centres end below Ef[120]
    assert (more, bins) == (16, 23) and more >= (bins + 1) // 2
    # the third and later passes run, with weight, at the cases of the LDS attribute and of the LDS limit and on the random grids
    assert np.bincount(S.interval_passes("nf255")).tolist() == [0, 2, 1, 2, 6]
    assert np.bincount(S.interval_passes("nf256")).tolist() == [0, 2, 1, 2, 6]
    assert S.interval_passes("nf639").max() == 10 and S.interval_passes("rnd30").max() == 5 and S.interval_passes("rnd70").max() == 3
    for name in ("nf255", "nf256", "nf639", "rnd30"):
        more, bins = changed(name, 2 * S.PRE_T)
        assert more >= (bins + 1) // 2, name
    assert changed("nf255", 2 * S.PRE_T) == (8, 11) and changed("nf639", 3 * S.PRE_T) == (6, 7)
    # and one pass is all there is at NFREQ = 50
    for name in ("ne65", "ne66", "ne128", "ne256", "ne280"):
        assert S.interval_passes(name).max() == 1


def test_the_grids_that_are_meant_to_be_awkward_are(oracle_soc):
    for name in S.RANDOM:
        FREQ, _, _, E, _ = S.inputs(name)
        NFREQ, NE = S.shape(name)
        k = S.oracle(oracle_soc, name)
        _, _, n = S.windows(k, NE)
        step = np.diff(np.log(FREQ.astype(np.float64)))
        assert step.max() > 10.0 * step.min()                   # uneven frequencies
        width = np.diff(E.astype(np.float64))
        assert width.min() < 1e-3 * np.median(width)            # one very narrow bin
        assert (n == 0).sum() > n.size // 2 and (n > 0).sum() > 0      # mostly empty pairs (L1 = -1, L2 = -2)
    L1 = S.oracle(oracle_soc, "rnd150")["L1"].reshape(150, 150)
    assert (L1[np.triu_indices(150, 1)] == -1).any()
    # no window at all
    k = S.oracle(oracle_soc, S.EMPTY)
    up = np.triu_indices(10, 1)
    assert (k["L1"].reshape(10, 10)[up] == -1).all() and (k["L2"].reshape(10, 10)[up] == -2).all()
    assert k["Iw"].size == 0 and not k["noIw"].any() and np.isfinite(k["Tdown"]).all()
    # the smallest sizes: one pair; three pairs on one frequency interval
    assert S.windows(S.oracle(oracle_soc, "ne2"), 2)[2].tolist() == [3]
    assert S.windows(S.oracle(oracle_soc, "nf2"), 3)[2].tolist() == [2, 2, 2]


@pytest.mark.parametrize("NE", S.SOLVER_NE)
def test_real_tables_through_the_solver_are_finite(NE, oracle_soc):
    """what the GPU test asserts of the device's emission holds of the oracle's: all 7 rows finite and non-negative at the three
    grain sizes, the zero row zero, every other row emitting -- and the tables are unlike the synthetic ones of synth.synth_solver:
    windows that reach over the whole frequency axis (synthetic: 11 frequencies at most) and, at the middle size, about half of
    the pairs empty"""
    from oracle.pyoracle import a2e_oracle_dosolve
    sol, AF = S.oracle_solver(oracle_soc, NE)
    ABS = S.solver_absorptions()
    assert ABS.shape == (7, 50) and np.isfinite(ABS).all() and not ABS[-1].any() and (ABS[:-1] > 0).all()
    longest = 0
    for isize in range(3):
        size = sol["sizes"][isize]
        _, _, n = S.windows(size, NE)
        longest = max(longest, int(n.max()))
        assert (n == 0).any() and ((0.4 < (n == 0).mean() < 0.6) == (isize == 1))
        em = a2e_oracle_dosolve(oracle_soc, NE, 50, size, AF[isize], ABS)
        assert np.isfinite(em).all() and (em >= 0).all() and not em[-1].any() and em[:-1].any(axis=1).all()
    assert longest >= 40                                        # of 50 frequencies


def test_first_difference_names_the_pair(oracle_soc):
    """the failure message of the GPU test: a changed weight is traced to its (l, u), a missing tail to the pair it belongs to"""
    NE = S.shape("ne130")[1]
    want = S.oracle(oracle_soc, "ne130")
    l, u, n = S.windows(want, NE)
    off = np.cumsum(n) - n
    assert S.first_difference(want, want, NE) is None
    for i in (int(np.nonzero(n > 0)[0][0]), int(np.nonzero((u - l - 1 >= S.PRE_T) & (n > 0))[0][0]), int(np.nonzero(n > 0)[0][-1])):
        bad = dict(want, Iw=want["Iw"].copy())
        bad["Iw"][off[i] + n[i] - 1] *= np.float32(1.5)
        assert S.first_difference(bad, want, NE) == (l[i], u[i])
    i = int(np.nonzero(n > 0)[0][-1])
    assert S.first_difference(dict(want, Iw=want["Iw"][:off[i]]), want, NE) == (l[i], u[i])


@pytest.mark.skipif(not _ref_available(), reason="reference build not available (GPU box)")
@pytest.mark.parametrize("name", S.NAMES)
def test_oracle_bit_exact_vs_reference(name, oracle_libm, oracle_soc):
    """the oracle is the reference of the GPU test: at every case it equals the x86 build of kernel_A2E_pre.c bit for bit"""
    want = RefA2EPre().pre(*S.inputs(name))
    got = a2e_oracle_pre(oracle_libm, *S.inputs(name), S.FACTOR)
    for key in KEYS:
        assert np.array_equal(np.asarray(got[key]).view(np.uint32), np.asarray(want[key]).view(np.uint32)), key
    soc = S.oracle(oracle_soc, name)                            # (double arithmetic and libm exp in both modes)
    for key in KEYS:
        assert np.array_equal(np.asarray(soc[key]).view(np.uint32), np.asarray(want[key]).view(np.uint32)), key
