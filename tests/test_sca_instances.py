"""The cases of tests/sca_instance_cases.py on the CPU: the oracle's scattered-light walk pinned bit for bit to the reference's kernel on
their grids (tests/golden/sca_instances.npz: the images of the x86 builds of kernel_ASOC_sca.c, made by tests/golden/make_golden.py
--sca-instances), and the conditions the table must keep (sca_instance_cases.problems).  The GPU side is tests/test_gpu_sca_instances.py."""
import os

import numpy as np
import pytest

import sca_instance_cases as si
from oracle import build as ob
from oracle.pyoracle import Job, RefSca, oracle_sca_counts, oracle_sim_sca
from soc_amd import synth

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "sca_instances.npz"))
IDS = [si.case_id(k) for k in si.CASES]


def test_the_table_and_the_reference_builds_agree():
    assert set(GOLD.files) == set(IDS) and len(IDS) == 44
    assert {si.ref_tag(k) for k in si.CASES} == {t for t in ob.sca_ref_models() if t.startswith("si_")}
    assert si.cloud(si.DEEP).CELLS == synth.SCA_INSTANCE_CELLS[si.DEEP] == 23224 and si.cloud(si.DEEP).LEVELS == 5
    for key in si.CASES:
        m, c, j = ob.sca_ref_models()[si.ref_tag(key)], si.cloud(si.CASES[key]["grid"]), si.job(key)
        assert (m["NX"], m["NY"], m["NZ"], m["LEVELS"], m["CELLS"]) == (c.NX, c.NY, c.NZ, c.LEVELS, c.CELLS)
        assert (m["WITH_ABU"], m["HPBG_WEIGHTED"], m["MIRROR"], m["NO_PS"]) == (int(j.OPT is not None), int(j.HPBGP is not None and
                                                                               si.CASES[key]["kind"] == si.HP), j.MIRROR, j.NO_PS)
    # the boundary of soc_grid_variant's rule, as the extra cases are meant to sit on it
    assert [si.instance(k)[1:3] for k in ("l2float-bg", "l2double-bg", "nyfloat-bg")] == [(1, 0), (1, 1), (1, 0)]


@pytest.mark.parametrize("key", list(si.CASES), ids=IDS)
def test_oracle_bit_exact_vs_reference_golden(key, oracle_libm):
    g0, n = si.items(key)
    OUT, nadd = oracle_sim_sca(oracle_libm, si.job(key), si.view(key), si.CASES[key]["kind"], g0, g0 + n)
    assert nadd >= si.MIN_CONTRIBUTIONS
    assert np.array_equal(OUT.view(np.uint32), GOLD[si.case_id(key)].view(np.uint32))


def test_the_table_keeps_its_conditions():
    assert si.problems(verbose=True) == []                     # (prints each case's counts and its float-walk figure)


def test_counters_of_the_oracle(oracle_soc):
    """packets as the kernels count them: BATCH per work item of a background launch, every sky packet whether it hits or not"""
    for key, per_item in (((si.BG, 1, 1, 0), 2), ((si.HP, 1, 1, 0), 16), ((si.PS, 0, 0, 0), 12)):
        g0, n = si.items(key)
        _, nadd = oracle_sim_sca(oracle_soc, si.job(key), si.view(key), key[0], g0, g0 + n, nthreads=4)
        npkt, nscat = oracle_sca_counts(oracle_soc)
        assert npkt == per_item * n and 0 < nscat <= nadd
    key = "hpx-bg"                                             # a Healpix image takes one contribution per scattering
    assert si.expected(key)[1] == si.expected(key)[3]


def test_the_old_witness_could_not_tell_a_float_walk(oracle_soc):
    # oct104x6x5 (3 levels) was the only DBL case of the direct kernel: a walk in float moves none of its pixels, so deep104x6x5 replaced it
    import cases
    import oracle.pyoracle
    from test_gpu_noncubic import _view, opacities
    cl = synth.noncubic_cloud("oct104x6x5")
    a, s = opacities(cl)
    job = Job(cl, cases._CSC, ABS=3.0 * a, SCA=s, SOURCE=1, BATCH=3, SEED=0.377, DSC=cases._DSC, BG=1.0)
    view = _view(cl, (14, 11), 0.8)
    want, n = oracle_sim_sca(oracle_soc, job, view, 0, 0, 3000)
    keep = oracle.pyoracle.double_index
    oracle.pyoracle.double_index = lambda NX, LEVELS: 0
    try:
        got, m = oracle_sim_sca(oracle_soc, job, view, 0, 0, 3000)
    finally:
        oracle.pyoracle.double_index = keep
    assert keep(cl.NX, cl.LEVELS) == 1 and (want > 0).sum() > 30
    assert m == n and si.outside_the_bar(got, want) == 0


@pytest.mark.skipif(not RefSca.available("si_deep104x6x5"), reason="reference builds (oracle/_ref) not present")
@pytest.mark.parametrize("key", [(si.BG, 1, 1, 0), (si.CL, 0, 1, 1), "mirror-cl"], ids=["bg-1-1-0", "cl-0-1-1", "mirror-cl"])
def test_live_reference(key, oracle_libm):
    job, view, kind = si.job(key), si.view(key), si.CASES[key]["kind"]
    OUT, _ = oracle_sim_sca(oracle_libm, job, view, kind, 0, 64)
    want = RefSca(si.ref_tag(key)).sim(job, view, kind, 0, 64)
    assert OUT.any() and np.array_equal(OUT.view(np.uint32), want.view(np.uint32))
