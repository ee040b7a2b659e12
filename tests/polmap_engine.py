"""OracleEngine plus the two polarisation-map methods of soc_amd.lib.Engine, backed by the CPU restatement of PolMapping
(tests/csrc/polmap_host.c).  Lets AbsorptionRun.write_polmaps run without a GPU."""
import numpy as np

import polmap_host
from oracle_engine import OracleEngine


class PolOracleEngine(OracleEngine):
    def __init__(self, mode="soc"):
        OracleEngine.__init__(self, mode)
        self.pol_mode = mode
        self.B = None
        self.polmap_calls = []                                 # keyword arguments of every polmap call

    def set_bfield(self, Bx, By=None, Bz=None):
        if Bx is None:
            self.B = None
            return
        self.B = [np.asarray(b, np.float32).copy() for b in (Bx, By, Bz)]
        assert all(b.size == self.cloud.CELLS for b in self.B)

    def polmap(self, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, polstat=0, polred=0, rho_weight=0, p0=0.2, LENGTH=1.0):
        if self.B is None:
            raise RuntimeError("polmap: no field set")
        self.polmap_calls.append(dict(polstat=polstat, polred=polred, rho_weight=rho_weight, p0=p0, LENGTH=LENGTH, ABS=ABS, SCA=SCA,
                                      EMIT=np.asarray(EMIT, np.float32).copy(), B=[b.copy() for b in self.B],
                                      OPT=None if self.OPT is None else np.asarray(self.OPT, np.float32).copy()))
        return polmap_host.polmap(self.pol_mode, self.cloud, self.B, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, OPT=self.OPT,
                                  polstat=polstat, polred=polred, rho_weight=rho_weight, threshold=getattr(self, "map_threshold", 0),
                                  p0=p0, LENGTH=LENGTH)


def write_model(d, cloud, B, extra="", T=None, abundance=False):
    """cloud, dust (three far-infrared frequencies), scattering function, background, the three B files and -- with T -- a
    temperature file; returns the ini file of a run that takes its emission from the temperatures (`loadtemp`, `iterations 0`)"""
    import os
    from soc_amd import files, synth
    cloud.write(os.path.join(d, "m.cloud"))
    freq = [1.0e12, 1.5e12, 3.0e12]
    with open(os.path.join(d, "m.dust"), "w") as fp:
        fp.write("eqdust\n 1.0e-7\n 1.0e-4\n%d\n" % len(freq))
        for f in freq:
            fp.write(" %.5e  0.6  %.5e  %.5e\n" % (f, 3.0e-2 * f / 3.0e12, 9.0e-3))
    dsc, csc = synth.hg_scattering_table(0.6, 500)
    files.write_scattering_functions(os.path.join(d, "m.dsc"), np.tile(dsc, (len(freq), 1)), np.tile(csc, (len(freq), 1)))
    np.asarray([1e-13, 2e-13, 1.5e-13], np.float32).tofile(os.path.join(d, "bg.bin"))
    for name, b in zip("xyz", B):
        files.write_temperature(os.path.join(d, "b%s.bin" % name), cloud, b)
    if T is None:
        T = np.random.default_rng(8).uniform(10.0, 18.0, cloud.CELLS)
    files.write_temperature(os.path.join(d, "m.T"), cloud, np.asarray(T, np.float32))
    ini = ("gridlength 0.5\ncloud %s/m.cloud\noptical %s/m.dust\ndsc %s/m.dsc 500\nbackground %s/bg.bin\n"
           "bgpackets 2000\nseed 0.7853981634\niterations 0\nloadtemp\ntemperature %s/m.T\nemitted %s/m.emit\n"
           "device g\nverbose 0\nmapping 14 11 0.9\ndirection 50 35\ndirection 90 0\n"
           "polmap %s/bx.bin %s/by.bin %s/bz.bin\n" % (d, d, d, d, d, d, d, d, d))
    ini += extra
    with open(os.path.join(d, "m.ini"), "w") as fp:
        fp.write(ini)
    return os.path.join(d, "m.ini")
