"""AbsorptionRun asks the engine for the float form of the brick-local walk (Engine.set_tuning(float_local=1)) exactly on a hierarchy
whose Index() the reference evaluates in float (LEVELS > 1 and NX <= 399 with two levels, <= 100 with three or more), only while its
transfer stages run and only with the class switch FLOAT_LOCAL on; a Cartesian model and a hierarchy with Index() in double issue no
tuning call at all."""
import os

import pytest

from oracle_engine import OracleEngine
from soc_amd import synth
from soc_amd.asoc import AbsorptionRun, float_index
from soc_amd.ini import User
from test_abu_local_host import Recording
from test_host import _write_model


def _run(d, cloud, switch, monkeypatch):
    monkeypatch.setattr(AbsorptionRun, "FLOAT_LOCAL", switch)
    os.chdir(d)
    eng = Recording("soc")
    run = AbsorptionRun(User(_write_model(d, cloud, nfreq=2, extra="gridlength 5e-7\n")), eng)
    CT, _ = run.run()
    assert CT.sum() > 0 and eng.launches == 2
    return eng


def test_float_index_hierarchy_asks_for_float_local(tmp_path, monkeypatch):
    cloud = synth.octree_cloud(8, levels=3, frac=0.15, seed=7)
    assert float_index(cloud)
    eng = _run(str(tmp_path), cloud, True, monkeypatch)
    assert eng.tuning == [("float_local", 1, 0), ("float_local", 0, 2)]      # on before the first launch, off again after the last


def test_class_switch_off_does_not_ask(tmp_path, monkeypatch):
    eng = _run(str(tmp_path), synth.octree_cloud(8, levels=3, frac=0.15, seed=7), False, monkeypatch)
    assert eng.tuning == []


def test_cartesian_model_does_not_ask(tmp_path, monkeypatch):
    cloud = synth.cartesian_cloud(6, seed=2)
    assert not float_index(cloud)
    eng = _run(str(tmp_path), cloud, True, monkeypatch)
    assert eng.tuning == []


class _Shape:
    def __init__(self, NX, LEVELS):
        self.NX, self.LEVELS = NX, LEVELS


@pytest.mark.parametrize("NX,LEVELS,want", [(64, 4, True), (100, 3, True), (101, 3, False), (104, 3, False), (104, 2, True), (256, 2, True),
                                            (399, 2, True), (400, 2, False), (64, 1, False), (512, 1, False)])
def test_float_index_is_the_reference_rule(NX, LEVELS, want):
    """kernel_ASOC_aux.c:25-37: DIMLIM is 100, or 399 with fewer than three levels; a single-level grid has no Index() climb at all"""
    assert float_index(_Shape(NX, LEVELS)) == want


def test_double_index_hierarchy_does_not_ask(monkeypatch):
    """a 104^3-root hierarchy of three levels: the stage wrapper issues no tuning call (the run itself is not made: its cloud is large)"""
    cloud = synth.octree_cloud(104, levels=3, frac=0.02, seed=3)
    assert not float_index(cloud)
    calls = []

    class Stub:
        WITH_ABU, ABU_LOCAL, FLOAT_LOCAL = False, True, True

        def _tune(self, **kw):
            calls.append(kw)

        @staticmethod
        def body():
            return 7
    stub = Stub()
    stub.cloud = cloud
    from soc_amd.asoc import _local_routing
    assert _local_routing()(lambda self: self.body())(stub) == 7 and _local_routing(abu=False)(lambda self: self.body())(stub) == 7
    assert calls == []
    stub.cloud = synth.octree_cloud(8, levels=3, frac=0.15, seed=7)
    assert _local_routing()(lambda self: self.body())(stub) == 7
    assert calls == [dict(float_local=1), dict(float_local=0)]


class RecordingSca(Recording):
    """... and the scattered-light launches counted with the absorption ones"""

    def _sca(self, *a, **kw):
        self.launches += 1
        return super()._sca(*a, **kw)


@pytest.mark.parametrize("switch", [True, False])
def test_scattered_light_driver_asks_for_float_local(switch, tmp_path, monkeypatch):
    """soc_amd.asocs on a float-Index hierarchy (6^3 roots, two levels): the key is set before the first scattered-light launch and
    taken back after the last; with the class switch off, and on a Cartesian grid, the engine is not asked"""
    from soc_amd.asocs import ScatteringRun
    from test_host_sca import _ini
    monkeypatch.setattr(AbsorptionRun, "FLOAT_LOCAL", switch)
    for k, cloud in enumerate((synth.octree_cloud(6, levels=2, frac=0.1, seed=9), synth.cartesian_cloud(6, seed=2))):
        d = str(tmp_path / ("m%d" % k))
        os.makedirs(d)
        os.chdir(d)
        eng = RecordingSca("soc")
        out = ScatteringRun(User(_ini(d, cloud, with_ps=True)), eng, verbose=0).run()
        assert out.sum() > 0 and eng.launches > 0
        if switch and float_index(cloud):
            assert eng.tuning == [("float_local", 1, 0), ("float_local", 0, eng.launches)]
        else:
            assert eng.tuning == []
