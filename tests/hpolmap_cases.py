"""The all-sky polarisation-map cases of tests/golden/hpolmaps.npz: models, switches and observer positions.  Shared by the
tests and by tools/make_hpolmap_golden.py, which records what the reference's PolHealpixMapping gives for them.  The models
are those of polmap_cases.py."""
import numpy as np

import polmap_cases as pc
import polmap_host

NSIDE = 6                                  # 432 pixels: not a multiple of 64 or 256
P0 = pc.P0                                 # ini key p0; the kernel sees -D p00=%.4ff (ASOC.py:349,359)
GL = pc.GL


def los_literal(x):
    """the value of -D MINLOS=%.3ef / -D MAXLOS=%.3ef (ASOC.py:349)"""
    return float("%.3e" % x)


def case(model, obs, polred=0, thr=0, interp=0, minlos=-1.0, maxlos=1e10, yshear=0.0):
    return dict(model=model, obs=obs, polred=polred, thr=thr, interp=interp, minlos=minlos, maxlos=maxlos, yshear=yshear)


# observers: "centre"; "face" 0.3 root cells from the faces x = 0 and y = NY, so also from their edge; "integral" on cell
# corners (every coordinate gets the 2e-5 nudge); "outside" the cloud: four planes of zeros; "deep<L>" in the middle of a
# leaf of level L, so that with LEVEL_THRESHOLD <= L every ray registers the cell it starts in.
# On a hierarchy the reference's walk can cycle without end (its Index() keeps octet coordinates when it climbs into a root
# leaf, see soc_map.hip): from the centre of oct8 three rays never leave.  The observers of the octree cases are ones from
# which every ray ends -- "near" the centre instead of on it, and the leaves DEEP_LEAF; make_hpolmap_golden.py checks that
# with the restatement's step counter before it calls the reference.
CASES = {
    "c8_centre":      case("c8", "centre"),
    "c8_face":        case("c8", "face"),
    "c8_integral":    case("c8", "integral"),
    "c8_outside":     case("c8", "outside"),
    "c8_polred":      case("c8", "face", polred=1),
    "c8_i1":          case("c8", "face", interp=1),
    "c8_i2":          case("c8", "face", interp=2),
    "c8_i3":          case("c8", "centre", interp=3),
    "c8_maxlos":      case("c8", "centre", maxlos=3.0),          # shorter than the cloud
    "c8_minlos":      case("c8", "centre", minlos=1.5),
    "c8_minmax":      case("c8", "face", minlos=1.0, maxlos=5.0),
    "c8_shear":       case("c8", "centre", yshear=2.5, maxlos=20.0),
    "c8_shear_i2":    case("c8", "face", yshear=2.5, maxlos=20.0, interp=2, polred=1),
    "c8abu_centre":   case("c8abu", "centre"),
    "c8abuh_face":    case("c8abuh", "face"),
    "oct8_near":      case("oct8", "near"),
    "oct8_face":      case("oct8", "face"),
    "oct8_integral":  case("oct8", "integral"),
    "oct8_outside":   case("oct8", "outside"),
    "oct8_polred":    case("oct8", "deep2", polred=1),
    "oct8_thr1":      case("oct8", "deep2", thr=1),
    "oct8_thr2":      case("oct8", "deep2", thr=2),
    "oct8_i3":        case("oct8", "near", interp=3),
    "oct8_i3_thr1":   case("oct8", "deep2", interp=3, thr=1, maxlos=6.0),
    "oct8_shear":     case("oct8", "near", yshear=2.5, maxlos=20.0),
    "oct104_centre":  case("oct104", "centre"),                  # NX > 100: Index() in double
    "oct104_deep":    case("oct104", "deep2", thr=1, interp=3),
    # grids whose three sides differ (synth.NONCUBIC): the 3 x 3 x 3 neighbour sums of INTERPOLATE and the periodic wrap of
    # Y_SHEAR read NX, NY and NZ apart
    "r759_centre":    case("r759", "centre"),
    "r759_face":      case("r759", "face"),
    "r759_integral":  case("r759", "integral"),
    "r759_i1":        case("r759", "face", interp=1),
    "r759_i2":        case("r759", "face", interp=2),
    "r759_i3":        case("r759", "centre", interp=3),
    "r759_shear":     case("r759", "centre", yshear=2.5, maxlos=20.0),
    "r759_shear_i2":  case("r759", "face", yshear=2.5, maxlos=20.0, interp=2),
    "oct759_near":    case("oct759", "near"),
    "oct759_face":    case("oct759", "face"),
    "oct759_integral": case("oct759", "integral"),
    "oct759_i3":      case("oct759", "near", interp=3),
    "oct759_shear":   case("oct759", "near", yshear=2.5, maxlos=20.0),
    "oct104x6x5_near": case("oct104x6x5", "near"),               # NX > 100: Index() in double
    "oct6x104x5_near": case("oct6x104x5", "near"),               # NY > 100 but NX is not: Index() in float
}


def model(name):
    return pc.model(name)


DEEP_LEAF = {"oct8": 182, "oct104": 0}     # which leaf of the level "deep<L>" takes


def leaf_position(cloud, level, n=0):
    """root-grid coordinates of the middle of the n-th leaf of `level`"""
    c = cloud
    PAR = polmap_host.parents(c)
    d = c.DENS[c.OFF[level]:c.OFF[level] + c.LCELLS[level]]
    ind = int(np.nonzero(d > 0.0)[0][n])
    x = np.asarray([0.5, 0.5, 0.5])
    for l in range(level, 0, -1):
        sid = ind % 8
        x = 0.5 * (x + np.asarray([sid % 2, (sid // 2) % 2, sid // 4]))
        ind = int(PAR[c.OFF[l] + ind - c.NX * c.NY * c.NZ])
    return tuple(float(v) for v in x + np.asarray([ind % c.NX, (ind // c.NX) % c.NY, ind // (c.NX * c.NY)]))


def observer(cloud, key, model=None):
    c = cloud
    if key == "centre":
        return (0.5 * c.NX, 0.5 * c.NY, 0.5 * c.NZ)
    if key == "face":
        return (0.3, c.NY - 0.3, 0.55 * c.NZ)
    if key == "integral":
        return (3.0, 4.0, 5.0)
    if key == "outside":
        return (-2.0, 0.5 * c.NY, 0.5 * c.NZ)
    if key == "near":
        return (0.5 * c.NX + 0.3, 0.5 * c.NY - 0.4, 0.5 * c.NZ + 0.2)
    if key.startswith("deep"):
        return leaf_position(c, int(key[4:]), DEEP_LEAF[model])
    raise KeyError(key)


def switches(name):
    """keyword arguments of one case as the kernel sees them: the -D literals rounded as ASOC.py:349 prints them"""
    k = CASES[name]
    return dict(polred=k["polred"], threshold=k["thr"], interpolate=k["interp"], minlos=los_literal(k["minlos"]),
                maxlos=los_literal(k["maxlos"]), y_shear=k["yshear"], p0=pc.p0_literal(P0), LENGTH=pc.length_literal())


def case_observer(name):
    k = CASES[name]
    return observer(pc.model(k["model"])["cloud"], k["obs"], k["model"])


fingerprint = pc.fingerprint
