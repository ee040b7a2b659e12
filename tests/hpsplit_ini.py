"""`split 1` + `hpbg` ini runs for the tests: split_ini's model files plus a sky file of hpsplit_cases.sky, one row per frequency."""
import os

import numpy as np

import hpsplit_cases as hc
from split_ini import FREQ, run_ini

SKY_SCALE = 1.0e-13
SKIES = (1, 2, 3)


def sky_rows():
    """[NFREQ, 49152] float32 as written to the sky file"""
    return np.stack([np.float32(SKY_SCALE) * hc.sky(s) for s in SKIES[:len(FREQ)]]).astype(np.float32)


def run_hp_ini(engine, d, weighted, split=1, cloud=None, extra="", bgpackets=300, seed=None):
    """split_ini.run_ini with `hpbg <sky file> 1.0 <weighted>`; the result also carries hp_launches of an HpSplitOracleEngine"""
    os.makedirs(str(d), exist_ok=True)
    path = os.path.join(str(d), "sky.bin")
    sky_rows().tofile(path)
    r = run_ini(engine, d, split=split, cloud=cloud, extra="hpbg %s 1.0 %d\n" % (path, weighted) + extra, bgpackets=bgpackets, seed=seed)
    r["hp_launches"] = getattr(engine, "hp_split_launches", None)
    return r
