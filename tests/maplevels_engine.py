"""The CPU stand-in of Engine.map_block_levels (`maplevels 1`), built from the definition of the product: plane (f, l) is
OracleEngine.map of frequency f with the emission of every cell that is not on hierarchy level l set to zero.  Nothing here
knows how the HIP kernel gets its planes.  Never imported by the product."""
import numpy as np

from oracle_engine import OracleEngine
from test_fastmap import BlockOracleEngine


def cell_levels(cloud):
    """the hierarchy level of every cell, in the order of the per-cell arrays"""
    return np.repeat(np.arange(cloud.LEVELS, dtype=np.int32), np.asarray(cloud.LCELLS[:cloud.LEVELS], np.int64))


def masked_emission(cloud, EMIT, level):
    """EMIT with 0.0f in every cell that is not on `level`"""
    return np.where(cell_levels(cloud) == level, np.asarray(EMIT, np.float32), np.float32(0.0)).astype(np.float32)


class LevelsOracleEngine(BlockOracleEngine):
    """BlockOracleEngine (OracleEngine + set_map_block / map_block) with map_block_levels by the definition"""

    def __init__(self, mode="soc"):
        BlockOracleEngine.__init__(self, mode)
        self.level_calls = 0

    def map_block_levels(self, DIR, RA, DE, NPIX, MAP_DX, CENTRE, INTOBS=None, healpix=0):
        assert self.block is not None, "map_block_levels without a batch"
        EMITX, ABS, SCA, OPT = self.block
        keep, out = self.OPT, []
        for k in range(EMITX.shape[1]):
            self.OPT = None if OPT is None else OPT[:, k, :]
            out.append(np.stack([OracleEngine.map(self, masked_emission(self.cloud, EMITX[:, k], l), DIR, RA, DE, NPIX, MAP_DX, CENTRE,
                                                  ABS[k], SCA[k], INTOBS=INTOBS, save_colden=0, LENGTH=1.0, healpix=healpix)[0]
                                 for l in range(self.cloud.LEVELS)]))
        self.OPT = keep
        self.level_calls += 1
        return np.stack(out)
