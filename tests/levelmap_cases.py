"""The per-level map cases of tests/golden/levelmaps.npz (`mapping nx ny dx 999`): models and views.  Shared by the tests and
by tools/make_levelmap_golden.py, which records what the Mapping kernel of the reference's kernel_ASOC_map_H.c gives for
them.  The models and the two external views are those of polmap_cases.py."""
import polmap_cases as pc

NPIX = pc.NPIX                             # 24 x 20 = 480 pixels: not a multiple of 256
GL = pc.GL


def case(model, view, dx=None):
    return dict(model=model, view=view, dx=dx)


# view: an index into polmap_cases.VIEWS (external), or the observer of a perspective image.  dx: MAP_DX where it is not the
# model's (which already makes the map a little wider than the cloud).
# oct8_face: the observer's y sits on a cell face, so the fmod nudge of kernel_ASOC_map_H.c:433 runs.
# c8_wide, oct8_wide: pixels so large that the whole outer ring of the map misses the model.
CASES = {
    "c8_v0":      case("c8", 0),                           # LEVELS = 1: one image
    "c8_v1":      case("c8", 1),
    "c8_wide":    case("c8", 0, dx=1.2),
    "oct8_v0":    case("oct8", 0),
    "oct8_v1":    case("oct8", 1),
    "oct8_wide":  case("oct8", 1, dx=1.2),
    "oct8_face":  case("oct8", (0.5, 3.0, 2.9)),
    "oct8_in":    case("oct8", (4.3, 3.6, 4.2)),
    "c8abu_v0":   case("c8abu", 0),
    "c8abuh_v1":  case("c8abuh", 1),                       # OPT rounded through fp16 and widened again, as the engine keeps it
    "oct104_v0":  case("oct104", 0),                       # NX > 100: Index() in double
    "oct104_v1":  case("oct104", 1),
    # grids whose three sides differ (synth.NONCUBIC)
    "r759_v0":    case("r759", 0),
    "r759_v1":    case("r759", 1),
    "oct759_v0":  case("oct759", 0),
    "oct759_v1":  case("oct759", 1),
    "oct759_in":  case("oct759", (4.3, 3.6, 4.2)),
    "oct104x6x5_v0": case("oct104x6x5", 0),                # NX > 100: Index() in double
    "oct104x6x5_v1": case("oct104x6x5", 1),
    "oct6x104x5_v0": case("oct6x104x5", 0),                # NY > 100 but NX is not: Index() in float
    "oct6x104x5_v1": case("oct6x104x5", 1),
}

model = pc.model
views = pc.views
centre = pc.centre
fingerprint = pc.fingerprint


def case_args(name, ODIR, RA, DE):
    """(m, keyword arguments of levelmap_host.levelmap / Engine.map_levels) of one case, without the opacities"""
    k = CASES[name]
    m = pc.model(k["model"])
    c = m["cloud"]
    kw = dict(NPIX=NPIX, MAP_DX=m["MAP_DX"] if k["dx"] is None else k["dx"], CENTRE=pc.centre(c), ABS=m["ABS"], SCA=m["SCA"])
    if isinstance(k["view"], tuple):
        kw.update(DIR=ODIR[0], RA=RA[0], DE=DE[0], INTOBS=k["view"])
    else:
        kw.update(DIR=ODIR[k["view"]], RA=RA[k["view"]], DE=DE[k["view"]], INTOBS=None)
    return m, kw


# How a result in soc_math.h arithmetic (the CPU restatement in "soc" mode, the HIP kernel) must agree with the recorded
# reference, whose transcendentals are libm's.  External views: only exp differs, in its last bits, and the walk is the same
# -- the tolerance of the polarisation maps' intensity plane, rtol 1e-5 (tests/test_polmap.py).  Perspective views on the octree:
# sin and cos of the pixel's angles differ in their last bits as well, and that file's walk is discontinuous there (a ray that
# climbs into a root leaf goes on from the corner of the grid, tests/test_hpolmap.py), so a handful of rays take another way.
# Measured between the two math modes of the restatement: the rays that take the same number of steps (474 and 471 of 480)
# differ by at most 8.6e-6 of the pixel's sum over the levels, the others by at most 5.06e-5 of it (two pixels per case beyond
# 1e-5).  The bound is twice that, as in tests/test_hpolmap.py.
PERSPECTIVE_BOUND = 2 * 5.06e-5


def close_to_reference(name, got, ref):
    import numpy as np
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return False
    if isinstance(CASES[name]["view"], tuple) and pc.model(CASES[name]["model"])["cloud"].LEVELS > 1:
        total = ref.sum(axis=0)
        return bool((total > 0.0).all() and (np.abs(got - ref).max(axis=0) <= PERSPECTIVE_BOUND * total).all())
    return bool(np.array_equal(got != 0.0, ref != 0.0) and np.allclose(got, ref, rtol=1e-5, atol=0.0))
