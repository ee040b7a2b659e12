"""The resident absorptions (soc_absorbed_*) as far as they can be checked without a GPU: the factors K that the device scales with
against files.scale_absorbed in numpy, the pipeline's choice of the host source on an engine without the calls, and the C ABI's
symbols in the header, the built library and the binding."""
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import files, synth                              # noqa: E402

CALLS = ["begin", "add_tally", "add_slot", "keep", "restore", "to_mabu", "download", "end"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_statement(A, cloud, K, nnnlimit):
    """what soc_absorbed_to_mabu computes, in numpy: one float32 division per cell, one float32 product per value, -1e20 by selection"""
    levels = np.searchsorted(np.asarray(cloud.OFF[:cloud.LEVELS]), np.arange(cloud.CELLS), side='right') - 1
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        w = K[levels] / cloud.DENS
        out = A * w[:, None]
    assert w.dtype == np.float32 and out.dtype == np.float32
    out[cloud.DENS <= np.float32(nnnlimit)] = np.float32(-1.0e20)
    return out


@pytest.mark.parametrize("seed, levels, GL", [(1, 1, 0.05), (2, 2, 0.5), (3, 3, 0.013), (4, 3, 7.7), (5, 4, 1.0e-3)])
def test_scale_factors_reproduce_scale_absorbed_to_the_bit(seed, levels, GL):
    rng = np.random.default_rng(seed)
    cloud = synth.octree_cloud(6, levels=levels, frac=0.15, seed=seed) if levels > 1 else synth.cartesian_cloud(6, seed=seed)
    leaves = np.flatnonzero(cloud.DENS > 0)
    cloud.DENS[leaves[:3]] = np.asarray([1.0e-11, 0.0, 3.0e-10], np.float32)
    cloud.DENS[leaves[3:]] = (10.0 ** rng.uniform(-6.0, 6.0, leaves.size - 3)).astype(np.float32)
    K = files.absorbed_scale_factors(cloud, GL)
    assert K.dtype == np.float32 and K.shape == (cloud.LEVELS,)
    A = (10.0 ** rng.uniform(-40.0, 30.0, (cloud.CELLS, 7))).astype(np.float32)
    for nnnlimit in (0.0, 1.0e-10, 1.0e-3):
        want = files.scale_absorbed(A.copy(), cloud, GL, nnnlimit)
        assert np.array_equal(bits(device_statement(A, cloud, K, nnnlimit)), bits(want))
        assert (want[cloud.DENS <= nnnlimit] == np.float32(-1.0e20)).all()


def test_pipeline_on_an_engine_without_the_calls_takes_the_host_source_and_says_so(tmp_path, capsys):
    """the oracle engine has none of the absorbed_* calls: the run is the restatement of what the pipeline did before them, to the bit"""
    from oracle_engine import OraclePipelineEngine
    from reemit_chain import iteration_case
    from soc_amd import driver, mabu
    from soc_amd.asoc import AbsorptionRun
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    d = str(tmp_path)
    ini, ini0 = iteration_case(d, cloud, 1)
    os.chdir(d)
    eng = OraclePipelineEngine("soc")
    assert not any(hasattr(eng, "absorbed_" + c) for c in CALLS)
    P = driver.Pipeline(ini0, eng, verbose=1)
    CTABS, FABS, EMITTED = P.run()
    assert "the absorptions go through the host: the engine has no absorbed_* calls" in capsys.readouterr().out
    assert P.timers["absorbed_source"] == "host" and P.timers["iterations"] == []
    # the statements of the pipeline before the resident absorptions
    Q = driver.Pipeline(ini0, eng, verbose=0)
    rt = AbsorptionRun(Q.U, eng, verbose=0)
    rt.write_packet_info()
    rt.setup_engine()
    C0, F0 = rt.simulate_constant_sources()
    files.scale_absorbed(F0, rt.cloud, Q.U.GL, Q.U.NNNLIMIT)
    E0, _ = mabu.solve_emission(eng, Q.dusts, Q.kinds, F0, mabu.abundance_table(rt.ABU, Q.U.SINGLE_ABU, cloud.CELLS, 2))
    assert np.array_equal(bits(CTABS), bits(C0)) and np.array_equal(bits(FABS), bits(F0)) and np.array_equal(bits(EMITTED), bits(E0))
    # with an iteration: the same source per iteration, asked for or not
    runs = []
    for source in (None, 'host'):
        P = driver.Pipeline(ini, eng, verbose=0, absorbed_source=source)
        runs.append(P.run(want_absorbed=source is None))
        assert P.timers["absorbed_source"] == "host" and [it["absorbed"] for it in P.timers["iterations"]] == ["host"]
    for a, b in zip(*runs):                                      # (the host source returns its array whatever want_absorbed says)
        assert np.array_equal(bits(a), bits(b))
    eng.close()


def test_absorbed_source_is_none_or_host(tmp_path):
    from reemit_chain import iteration_case
    from soc_amd import driver
    ini, _ = iteration_case(str(tmp_path), synth.octree_cloud(6, levels=2, frac=0.1, seed=9), 1)
    with pytest.raises(ValueError, match="absorbed_source"):
        driver.Pipeline(ini, None, verbose=0, absorbed_source='bogus')


def test_transfer_stage_refuses_a_sink_it_cannot_fill(tmp_path):
    from test_host import _write_model
    from soc_amd.asoc import AbsorptionRun, ResidentAbsorptions
    from soc_amd.ini import User
    import types
    d = str(tmp_path)
    cloud = synth.cartesian_cloud(6, seed=9)
    calls = types.SimpleNamespace(absorbed_begin=None, absorbed_add_tally=None, absorbed_add_slot=None)
    rt = AbsorptionRun(User(_write_model(d, cloud)), calls, verbose=0)
    assert rt.resident_absorptions_refused() is None
    assert "no absorbed_* calls" in AbsorptionRun(User(_write_model(d, cloud)), None, verbose=0).resident_absorptions_refused()
    rt = AbsorptionRun(User(_write_model(d, cloud, extra="saveint 1 %s/int.bin\n" % d)), calls, verbose=0)
    assert rt.resident_absorptions_refused() == "saveint"
    with pytest.raises(ValueError, match="saveint"):
        rt.simulate_constant_sources(absorbed=ResidentAbsorptions(calls, cloud.CELLS, rt.NFREQ))
    rt = AbsorptionRun(User(_write_model(d, cloud)), calls, types.SimpleNamespace(rank=0, world=2), verbose=0)
    assert rt.resident_absorptions_refused() == "several ranks"


def test_every_symbol_of_the_header_is_exported_and_bound():
    from soc_amd import lib as soclib
    with open(os.path.join(REPO, "include", "soc_hip.h")) as fp:
        declared = re.findall(r"^int (soc_absorbed_\w+)\(", fp.read(), re.M)
    assert declared == ["soc_absorbed_" + c for c in CALLS]
    lib = soclib.load_library()
    for name in declared:
        assert name in soclib.API and getattr(lib, name).argtypes == soclib.API[name][1]
        assert callable(getattr(soclib.Engine, name[4:]))
    assert callable(files.absorbed_scale_factors)
