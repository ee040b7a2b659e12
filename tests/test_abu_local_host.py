"""AbsorptionRun asks the engine for the brick-local walk of launches with per-cell opacities (Engine.set_tuning(abu_local=1)) exactly
when the run has an abundance file, only while its transfer stages run, and the engine has its built-in routing back afterwards."""
import os

import numpy as np

from oracle_engine import OracleEngine
from soc_amd import synth
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User
from test_host import _write_model


class Recording(OracleEngine):
    """the oracle behind the Engine calls, with the tuning calls kept: [(key, value, launches issued so far)]"""

    def __init__(self, *a):
        super().__init__(*a)
        self.tuning, self.launches = [], 0

    def set_tuning(self, **kw):
        self.tuning += [(k, v, self.launches) for k, v in kw.items()]

    def sim_pb(self, *a, **kw):
        self.launches += 1
        return super().sim_pb(*a, **kw)


def _model(d, with_abundances):
    cloud = synth.cartesian_cloud(6, seed=2)
    ini = _write_model(d, cloud, nfreq=2, extra="gridlength 5e-7\n")
    if with_abundances:
        np.random.default_rng(4).uniform(0.2, 1.0, cloud.CELLS).astype(np.float32).tofile(os.path.join(d, "a.abu"))
        with open(os.path.join(d, "m2.dust"), "w") as fp:
            fp.write("eqdust\n 1.0e-7\n 0.7e-4\n2\n 4.00000e+14  0.6  2.0e-2  1.2e-1\n 4.67700e+14  0.6  2.5e-2  1.0e-1\n")
        txt = open(ini).read().replace("optical %s/m.dust\n" % d, "optical %s/m.dust %s/a.abu\noptical %s/m2.dust\n" % (d, d, d))
        open(ini, "w").write(txt)
    return ini


def test_run_with_an_abundance_file_asks_for_abu_local(tmp_path):
    d = str(tmp_path)
    os.chdir(d)
    eng = Recording("soc")
    run = AbsorptionRun(User(_model(d, True)), eng)
    assert run.WITH_ABU
    CT, _ = run.run()
    assert CT.sum() > 0 and eng.launches == 2
    if AbsorptionRun.ABU_LOCAL:
        # on before the first launch, off again after the last
        assert eng.tuning == [("abu_local", 1, 0), ("abu_local", 0, 2)]
    else:
        assert eng.tuning == []
    # the class switch (what the measurement decides) off: the engine is not asked
    eng = Recording("soc")
    run = AbsorptionRun(User(_model(d, True)), eng)
    run.ABU_LOCAL = False
    run.run()
    assert eng.tuning == []


def test_run_without_an_abundance_file_does_not(tmp_path):
    d = str(tmp_path)
    os.chdir(d)
    eng = Recording("soc")
    run = AbsorptionRun(User(_model(d, False)), eng)
    assert not run.WITH_ABU
    run.run()
    assert eng.launches == 2 and eng.tuning == []


def test_an_engine_without_tuning_runs_as_before(tmp_path):
    d = str(tmp_path)
    os.chdir(d)
    assert not hasattr(OracleEngine, "set_tuning")
    CT, _ = AbsorptionRun(User(_model(d, True)), OracleEngine("soc")).run()
    assert CT.sum() > 0
