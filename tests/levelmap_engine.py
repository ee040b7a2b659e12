"""OracleEngine plus the per-level map method of soc_amd.lib.Engine, backed by the CPU restatement of the Mapping kernel of
kernel_ASOC_map_H.c (tests/csrc/levelmap_host.c).  Lets AbsorptionRun.write_level_maps run without a GPU."""
import numpy as np

import levelmap_host
from oracle_engine import OracleEngine, OraclePipelineEngine


class _LevelMaps:
    def map_levels(self, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, INTOBS=None):
        if not hasattr(self, "level_calls"):
            self.level_calls = []                              # keyword arguments of every map_levels call
        self.level_calls.append(dict(EMIT=np.asarray(EMIT, np.float32).copy(), DIR=np.asarray(DIR, np.float32).copy(), ABS=ABS, SCA=SCA,
                                     INTOBS=None if INTOBS is None else tuple(INTOBS), NPIX=tuple(NPIX), MAP_DX=MAP_DX, CENTRE=tuple(CENTRE),
                                     OPT=None if self.OPT is None else np.asarray(self.OPT, np.float32).copy()))
        return levelmap_host.levelmap(self.level_mode, self.cloud, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, INTOBS=INTOBS,
                                      OPT=self.OPT)


class LevelOracleEngine(_LevelMaps, OracleEngine):
    def __init__(self, mode="soc"):
        OracleEngine.__init__(self, mode)
        self.level_mode = mode


class LevelPipelineEngine(_LevelMaps, OraclePipelineEngine):
    """everything soc_amd.driver.Pipeline calls, and map_levels"""
    def __init__(self, mode="soc"):
        OraclePipelineEngine.__init__(self, mode)
        self.level_mode = mode
