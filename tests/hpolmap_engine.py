"""PolOracleEngine plus polmap_healpix of soc_amd.lib.Engine, backed by the CPU restatement of PolHealpixMapping
(tests/csrc/hpolmap_host.c).  Lets AbsorptionRun.write_healpix_polmaps run without a GPU."""
import numpy as np

import hpolmap_host
from polmap_engine import PolOracleEngine


class HPolOracleEngine(PolOracleEngine):
    def __init__(self, mode="soc"):
        PolOracleEngine.__init__(self, mode)
        self.hpolmap_calls = []                                # keyword arguments of every polmap_healpix call

    def polmap_healpix(self, EMIT, NSIDE, INTOBS, ABS, SCA, polred=0, p0=0.2, interpolate=0, minlos=-1.0, maxlos=1e10, y_shear=0.0,
                       LENGTH=1.0):
        if self.B is None:
            raise RuntimeError("polmap_healpix: no field set")
        self.hpolmap_calls.append(dict(NSIDE=NSIDE, INTOBS=tuple(INTOBS), polred=polred, p0=p0, interpolate=interpolate, minlos=minlos,
                                       maxlos=maxlos, y_shear=y_shear, LENGTH=LENGTH, ABS=ABS, SCA=SCA,
                                       EMIT=np.asarray(EMIT, np.float32).copy(), B=[b.copy() for b in self.B],
                                       OPT=None if self.OPT is None else np.asarray(self.OPT, np.float32).copy()))
        return hpolmap_host.polmap(self.pol_mode, self.cloud, self.B, EMIT, NSIDE, INTOBS, ABS, SCA, OPT=self.OPT, polred=polred,
                                   threshold=getattr(self, "map_threshold", 0), p0=p0, interpolate=interpolate, minlos=minlos,
                                   maxlos=maxlos, y_shear=y_shear, LENGTH=LENGTH)
