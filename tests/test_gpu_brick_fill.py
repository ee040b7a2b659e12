"""The brick-local sweep on the bricks of either partition of soc_amd/csrc/soc_lbricks.h -- Engine.set_tuning(brick_partition=1): the
tiles of 16^3 root cells, halved; 2 (and 0, the built-in choice): of the tiles and the slabs the partition with the smaller total face
area, whose boxes have edges of any length and lie on no tile's grid.  A batch of a background, a point-source and a cell-emission launch
(the mixed-source kernel of the bench) on a hierarchy whose Index() runs in double and on one where it runs in float, at bricks of 600
cells -- thousands of ragged boxes -- and at the built-in size; the INT tally kept; a sweep of rays.  The bar of tests/test_gpu_ltree.py:
tally events equal to the oracle's (the count the oracle reports), tallies to fp32 summation order (rtol 1e-5) -- and packets, tally
events and scatterings equal between the two partitions."""
import numpy as np
import pytest

import cases
from oracle.pyoracle import Job, oracle_sim_sca
from soc_amd import synth
from test_gpu_ltree import cloud104
from test_gpu_sca import assert_image_close
from test_gpu_sca_rays import _rays, view104
from util import assert_tally_close

pytestmark = pytest.mark.gpu

TILES, BEST = 1, 2
_MEMO = {}


def cloud(name):
    if name == "oct104_l4":
        return cloud104()
    if name not in _MEMO:
        _MEMO[name] = synth.octree_cloud(64, levels=4)
    return _MEMO[name]


def launches(name):
    """[(kind, Job, gid0, gid1)]: background, point sources inside and outside the model, cell emission; with the oracle's TABS, INT and
    events of each, computed once per session and left unchanged"""
    key = "launches " + name
    if key not in _MEMO:
        cl = cloud(name)
        N = cl.NX
        if name == "oct104_l4":
            a, s = 3e-6, 3e-5                                 # the opacities of tests/test_gpu_ltree.py
        else:
            root = cl.DENS[:N ** 3]
            s = 1.0 / (N * float(root[root > 0].mean()))      # of tests/test_gpu_ltree_float.py: about one optical depth of scattering
            a = 0.1 * s
        G = 8 * cl.AREA
        g0 = 100000 if G > 106000 else 0
        ps = np.array([[0.5 * N + 0.3, 0.5 * N - 0.3, 0.5 * N - 1.8], [0.5 * N, 0.5 * N, 3.0 * N]], np.float32)
        emit = np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)
        L = [(0, Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=1, BATCH=4, SEED=0.377, WITH_INT=1), g0, min(G, g0 + 6000)),
             (0, Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=0, BATCH=30, SEED=0.2, GLOBAL=512, PSPOS=ps, PS=[1.0, 2.5], PS_METHOD=0, WITH_INT=1, TW=1.5), 0, 512),
             (1, Job(cl, cases._CSC, ABS=a, SCA=s, SOURCE=2, BATCH=1, SEED=0.9, GLOBAL=8192, EMIT=emit, WITH_INT=1, TW=0.7), 4000, 4096)]
        _MEMO[key] = L
    return _MEMO[key]


def oracle(orc, name):
    key = "oracle " + name
    if key not in _MEMO:
        out = []
        for kind, job, g0, g1 in launches(name):
            T, I, n = orc.sim(job, kind, gid0=g0, gid1=g1, nthreads=8)
            T.setflags(write=False)
            I.setflags(write=False)
            out.append((T, I, n))
        _MEMO[key] = out
    return _MEMO[key]


def run_batch(e, name, keep_int):
    """the launches deferred into one sweep; (TABS, [INT of each launch], stats)"""
    cl = cloud(name)
    e.set_cloud(cl)
    e.set_features(with_int=keep_int, ps_method=0, use_emweight=0)
    e.set_opt(None)
    e.set_mirror(0)
    e.set_exec(1, 4)
    e.zero(0)
    e.stats(reset=True)
    (e.batch_begin_int if keep_int else e.batch_begin)(4)
    for kind, job, g0, g1 in launches(name):
        e.set_scatter_table(job.DSC, job.CSC)
        e.set_optical(job.ABS, job.SCA)
        if kind == 0:
            e.sim_pb(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.BG, job.TW, PSPOS=job.PSPOS[:, :3], PS=job.PS, GLOBAL=job.GLOBAL,
                     gid_first=g0, gid_count=g1 - g0)
        else:
            e.set_emission(job.EMIT, None)
            e.sim_cl(job.SOURCE, job.PACKETS, job.BATCH, job.SEED, job.TW, job.GLOBAL, gid_first=g0, gid_count=g1 - g0)
    assert e.last_passes() == 0
    e.batch_end()
    st = e.stats()
    assert e.last_passes() > 0 and e.last_form() == 3
    assert e.last_variant()["dbl"] == (1 if name == "oct104_l4" else 0)
    ints = [e.batch_read_int(k) for k in range(3)] if keep_int else []
    return e.read_tally(0), ints, st


@pytest.fixture
def partitioned(engine):
    """the float form where the hierarchy needs it; everything back to the built-in choices afterwards"""
    engine.set_tuning(float_local=1)
    yield engine
    engine.set_tuning(float_local=0, brick_partition=0, brick_cells=0, steps_per_visit=0)
    engine.set_features(0, 0, 0)
    engine.set_exec(-1, 4)


@pytest.mark.parametrize("name,cells,keep_int", [("oct104_l4", 600, 0), ("oct104_l4", 0, 0), ("oct64_l4", 600, 0), ("oct64_l4", 0, 0),
                                                 ("oct104_l4", 600, 1)],
                         ids=["dbl_cells600", "dbl_default", "flt_cells600", "flt_default", "dbl_cells600_int"])
def test_a_batch_of_three_sources_on_either_partition(name, cells, keep_int, partitioned, oracle_soc):
    e = partitioned
    want = oracle(oracle_soc, name)
    tabs = sum(T.astype(np.float64) for T, _, _ in want)
    n = sum(k for _, _, k in want)
    e.set_tuning(brick_cells=cells)
    stats, passes = [], []
    for part in (TILES, BEST):
        e.set_tuning(brick_partition=part)
        T, ints, st = run_batch(e, name, keep_int)
        passes.append(e.last_passes())
        print("%s cells %d partition %d: passes %d, %s" % (name, cells, part, e.last_passes(), st))
        assert st["tally_events"] == n, "trajectories diverged from the oracle"
        assert st["packets"] > 30000 and st["scatterings"] > 1000
        assert_tally_close(T, tabs, rtol=1e-5)
        for I, (_, Iw, _) in zip(ints, want):
            assert_tally_close(I, Iw, rtol=1e-5)
        stats.append(st)
    assert stats[0] == stats[1]
    # the key reaches the builder: a sweep needs as many passes as its longest chain of brick visits, and on these hierarchies the
    # bricks of the smaller face area make that chain shorter (tests/test_lbricks_fill.py: 0.82 ... 0.90 of the tiles' area)
    assert passes[1] < passes[0], passes


def test_a_sweep_of_rays_on_either_partition(partitioned, oracle_soc):
    """soc_lray_pass: the background rays of tests/test_gpu_sca_rays.py at its small bricks (900 cells, 5 steps per visit)"""
    e = partitioned
    cl = cloud104()
    k = 2.0 / (104 * float(cl.DENS[:104 ** 3][cl.DENS[:104 ** 3] > 0].mean()))
    job = Job(cl, cases._CSC, ABS=0.3 * k, SCA=k, SOURCE=1, BATCH=3, SEED=0.377, DSC=cases._DSC, BG=1.0)
    view = view104(FFS=1)
    g0, g1 = 100000, 103000
    want, n = oracle_sim_sca(oracle_soc, job, view, 0, gid0=g0, gid1=g1, nthreads=8)
    e.set_tuning(brick_cells=900, steps_per_visit=5)
    stats = []
    for part in (TILES, BEST):
        e.set_tuning(brick_partition=part)
        got, st = _rays(e, job, view, 0, g0, g1)
        assert st["tally_events"] == n and st["packets"] == 3 * (g1 - g0) and st["scatterings"] > 1000
        assert_image_close(got, want)
        stats.append(st)
    assert stats[0] == stats[1]


def test_the_key_takes_three_values(engine):
    from soc_amd.lib import SocError
    with pytest.raises(SocError, match="brick_partition"):
        engine.set_tuning(brick_partition=3)
    engine.set_tuning(brick_partition=0)
