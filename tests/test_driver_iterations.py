"""soc_amd.driver with dust re-emission iterations (`iterations N` + `cellpackets`), on the oracle-backed engine: the in-memory loop
equals, bit for bit, the chain of the existing programs -- the pipeline without `cellpackets`, then per iteration soc_amd.asoc
(`iterations 1`, `nosolve`, reading the emitted file of the iteration before) and soc_amd.mabu.solve_emission on the absorbed file it
wrote (reemit_chain.chain).  The oracle engine is deterministic, so equal means np.array_equal."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import files, synth                     # noqa: E402
from soc_amd.asoc import UnsupportedOption           # noqa: E402

NFREQ = 12
N = 2


def cloud_():
    return synth.octree_cloud(6, levels=2, frac=0.1, seed=9)            # 392 cells


@pytest.mark.parametrize("emweight", [0, 1])
def test_pipeline_iterations_equal_the_chain_of_programs(tmp_path, emweight):
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import chain, iteration_case
    from soc_amd import driver
    cloud = cloud_()
    extra = "emweight %d\n" % emweight if emweight else ""
    dc, dp = os.path.join(str(tmp_path), "chain"), os.path.join(str(tmp_path), "pipe")
    ini, ini0 = iteration_case(dc, cloud, N, extra)
    os.chdir(dc)
    steps = chain(ini, ini0, lambda: OraclePipelineEngine("soc"), N, cloud.CELLS, NFREQ)
    ini, _ = iteration_case(dp, cloud, N, extra)
    os.chdir(dp)
    P = driver.Pipeline(ini, OraclePipelineEngine("soc"), verbose=0)
    CTABS, FABS, EMITTED = P.run(keep_files=True)
    FABS_N, E_N = steps[N]
    assert np.array_equal(EMITTED, E_N) and np.array_equal(FABS, FABS_N)
    assert np.array_equal(np.asarray(files.mmap_emitted(os.path.join(dp, "emitted.data"), cloud.CELLS, NFREQ)), E_N)
    assert np.array_equal(files.read_absorbed(os.path.join(dp, "abs.data")), FABS_N)
    # the loop did something, in every iteration
    leaf = cloud.DENS > 0
    for k in range(N):
        assert not np.array_equal(steps[k + 1][1], steps[k][1])
        # (the dust's own emission adds to the absorptions of the constant sources)
        assert (steps[k + 1][0][leaf] >= steps[0][0][leaf]).all() and (steps[k + 1][0][leaf] > steps[0][0][leaf]).any()
    assert np.isfinite(EMITTED[leaf]).all() and (EMITTED[leaf] >= 0).all()
    its = P.timers["iterations"]
    assert len(its) == N and all(it["source"] == 'host' for it in its)
    assert all(it["transfer"] > 0 and it["emission"] > 0 for it in its)
    maps = np.fromfile("map_dir_00.bin", np.float32)[2:].reshape(NFREQ, 8, 8)
    assert np.isfinite(maps).all() and maps.max() > 0


def test_without_cellpackets_nothing_changes(tmp_path):
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import iteration_case
    from soc_amd import driver
    cloud = cloud_()
    d1, d2 = os.path.join(str(tmp_path), "one"), os.path.join(str(tmp_path), "two")
    _, ini0 = iteration_case(d1, cloud, 1)                               # write_case's own ini: `iterations 1`, no cellpackets
    os.chdir(d1)
    P1 = driver.Pipeline(ini0, OraclePipelineEngine("soc"), verbose=0)
    C1, F1, E1 = P1.run()
    assert P1.timers["iterations"] == []
    _, ini0 = iteration_case(d2, cloud, N)                               # `iterations 2` alone is no iteration either
    os.chdir(d2)
    P2 = driver.Pipeline(ini0, OraclePipelineEngine("soc"), verbose=0)
    C2, F2, E2 = P2.run()
    assert P2.timers["iterations"] == []
    assert np.array_equal(C1, C2) and np.array_equal(F1, F2) and np.array_equal(E1, E2)


@pytest.mark.parametrize("line, key", [("ali 1\n", "ali"), ("reference 1\n", "reference"), ("remit 10.0 3000.0\n", "remit")])
def test_what_the_loop_does_not_carry_is_refused_by_name(tmp_path, line, key):
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import iteration_case
    from soc_amd import driver
    cloud = cloud_()
    ini, ini0 = iteration_case(str(tmp_path), cloud, N, line)
    os.chdir(str(tmp_path))
    with pytest.raises((UnsupportedOption, ValueError), match=key):
        driver.Pipeline(ini, OraclePipelineEngine("soc"), verbose=0).run()
    assert not os.path.exists(os.path.join(str(tmp_path), "emitted.data"))
    driver.Pipeline(ini0, OraclePipelineEngine("soc"), verbose=0)        # without cellpackets the key stays accepted
