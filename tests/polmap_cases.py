"""The polarisation-map cases of tests/golden/polmaps.npz: models, switches and views.  Shared by the tests and by
tools/make_polmap_golden.py, which records what the reference's PolMapping gives for them."""
import math

import numpy as np

from soc_amd import launch, synth

GL = 0.01
P0 = 0.15                                  # ini key p0; the kernel sees -D p00=%.4ff (ASOC.py:349,359)
VIEWS = [(50.0, 35.0), (90.0, 0.0)]        # (theta, phi) in degrees: one oblique direction, one along the x axis

# name: (model, POLSTAT, POLRED, POL_RHO_WEIGHT, LEVEL_THRESHOLD)
CASES = {
    "c8_s0":          ("c8", 0, 0, 0, 0),
    "oct8_s0":        ("oct8", 0, 0, 0, 0),
    "oct8_s0_polred": ("oct8", 0, 1, 0, 0),
    "oct8_s0_rhow":   ("oct8", 0, 0, 1, 0),
    "oct8_s0_thr1":   ("oct8", 0, 0, 0, 1),
    "c8abu_s0":       ("c8abu", 0, 0, 0, 0),
    "c8abuh_s0":      ("c8abuh", 0, 0, 0, 0),     # OPT rounded through fp16 and widened again, as the engine keeps it
    "oct104_s0":      ("oct104", 0, 0, 0, 0),     # NX > 100: Index() in double
    "oct8_s1":        ("oct8", 1, 0, 0, 0),
    "oct8_s1_polred": ("oct8", 1, 1, 0, 0),
    "oct8_s1_thr2":   ("oct8", 1, 0, 0, 2),
    "oct8_s3":        ("oct8", 3, 0, 0, 0),
    "oct8_s3_thr1":   ("oct8", 3, 0, 0, 1),
    # grids whose three sides differ (synth.NONCUBIC)
    "r759_s0":        ("r759", 0, 0, 0, 0),
    "oct759_s0":      ("oct759", 0, 0, 0, 0),
    "oct759_s1":      ("oct759", 1, 0, 0, 0),
    "oct759_s3":      ("oct759", 3, 0, 0, 0),
    "oct759_s0_thr1": ("oct759", 0, 1, 1, 1),
    "oct104x6x5_s0":  ("oct104x6x5", 0, 0, 0, 0),     # NX > 100: Index() in double
    "oct6x104x5_s0":  ("oct6x104x5", 0, 0, 0, 0),     # NY > 100 but NX is not: Index() in float
}

NPIX = (24, 20)                            # 480 pixels: not a multiple of 256

_models = {}


def p0_literal(p0):
    """the value of -D p00=%.4ff"""
    return float("%.4f" % p0)


def model(name):
    """dict(cloud, B, EMIT, OPT, ABS, SCA, MAP_DX): MAP_DX makes the map wider than the cloud, so some rays miss"""
    if name in _models:
        return _models[name]
    if name.startswith("c8"):
        cloud = synth.cartesian_cloud(8, seed=3)
    elif name == "oct8":
        cloud = synth.octree_cloud(8, levels=3, frac=0.15, seed=7)
    elif name == "oct104":
        cloud = synth.octree_cloud(104, levels=3, frac=0.002, seed=11)
    elif name in synth.NONCUBIC:
        cloud = synth.noncubic_cloud(name)
    else:
        raise KeyError(name)
    rng = np.random.default_rng(2024)
    m = dict(cloud=cloud, B=synth.magnetic_field(cloud, seed=5), OPT=None)
    m["EMIT"] = np.asarray(rng.uniform(0.5e-3, 1.5e-3, cloud.CELLS), np.float32)
    big = cloud.NX > 100
    long_side = max(cloud.NX, cloud.NY, cloud.NZ) > 100        # the thin slabs: the opacities of the large models, the pixels of the small ones
    m["ABS"], m["SCA"] = (np.float32(4.0e-6), np.float32(6.0e-6)) if long_side else (np.float32(4.0e-5), np.float32(6.0e-5))
    m["MAP_DX"] = 7.0 if (big and name not in synth.NONCUBIC) else 0.6
    if "abu" in name:
        OPT = np.asarray(rng.uniform(2.0e-5, 8.0e-5, (cloud.CELLS, 2)), np.float32)
        if name.endswith("h"):
            OPT = np.asarray(np.asarray(OPT, np.float16), np.float32)
        m["OPT"] = OPT
    _models[name] = m
    return m


def views():
    """ODIR, RA, DE as the reference host forms them (ASOC_aux.py:1129-1183)"""
    _, ODIR, RA, DE = launch.set_observer_directions([math.radians(t) for t, _ in VIEWS], [math.radians(p) for _, p in VIEWS])
    return ODIR, RA, DE


def length_literal():
    return launch.kernel_literals(GL)[1]


def centre(cloud):
    return (0.5 * cloud.NX, 0.5 * cloud.NY, 0.5 * cloud.NZ)


def fingerprint(m):
    """float64 sums of the inputs: the golden file records them, so a drifting generator shows up as such"""
    c = m["cloud"]
    v = [np.abs(c.DENS.astype(np.float64)).sum(), m["EMIT"].astype(np.float64).sum()] + [np.abs(b.astype(np.float64)).sum() for b in m["B"]]
    v.append(0.0 if m["OPT"] is None else m["OPT"].astype(np.float64).sum())
    return np.asarray(v, np.float64)
