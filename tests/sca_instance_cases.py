"""One launch per compiled instance of the direct scattered-light kernel, soc_sca_kernel<OCT, DBL, ABU, KIND> (soc_amd/csrc/soc_sca.hip),
and twelve more on the paths its small-grid tests never took.  Shared by tests/test_sca_instances.py (CPU: the oracle pinned to the
reference on these grids, the conditions below), tests/test_gpu_sca_instances.py (the instances against the oracle) and
tests/golden/make_golden.py --sca-instances (the images of the reference's own kernel, tests/golden/sca_instances.npz).

REACHABLE = {(kind, octree, dbl, abu)}: 32 keys, kind the SOC_SCA_* value (0 SimRAM_PB, 1 _CL, 2 _PS, 3 _HP).  sca_dispatch takes dbl
from soc_grid_variant as it comes -- NX > 100 with three levels or more, NX > 399 below that -- and, unlike the absorption launchers,
does not clear it on a single-level grid, so all 32 can run.  GRIDS gives the grid of each (octree, dbl):
  (0, 0) r759: 7 x 5 x 9 cells;                    (0, 1) c400: 400 x 3 x 2 cells, NX > 399;
  (1, 0) oct759: 7 x 5 x 9 roots, three levels;    (1, 1) deep104x6x5: 104 x 6 x 5 roots, five levels, 23224 cells.
EXTRA holds the cases outside the matrix: a Healpix image seen from inside the deep hierarchy for every kind (the HPX branch of the
kernel, SimRAM_PB's fp64 `+ 1.0e-6` in it), reflecting faces on a hierarchy (MIRROR 21: the lower x, y and z faces), and the boundary
of soc_grid_variant's rule -- 104 x 6 x 5 roots with two levels (float), 400 x 3 x 2 roots with two levels (double), 6 x 104 x 5 roots
with three (float: the switch is on NX alone).

What the table must keep true is problems(), a list of complaints that tests/test_sca_instances.py asserts empty:
  * every case gives at least 1000 image contributions and 100 scatterings, a finite image, lit and dark pixels;
  * every case on a hierarchy with Index() in double tells a walk in float from one in double: with oracle.pyoracle.double_index
    forced to 0 the oracle (soc mode) changes an event count or moves at least 3 pixels outside the bar of
    test_gpu_sca.assert_image_close (rtol 1e-5) -- float_walk_differs, after split_cases.float_walk_differs.  So every group
    (a grid and a kind) that has such cases has one that does, which is what the condition is for: a DBL instance that walked
    in float would fail its test.
The condition does not apply to c400: Index() has no double arithmetic at level 0, a walk in float is bit-identical there on the CPU
(problems() checks that too), and those eight instances are checked for dispatch and parity with the oracle only.  Nor can the two
cases on 400 x 3 x 2 roots with two levels meet it (double_index_matters): there the two walks differ in last bits only.

Figures of the float walk on the CPU (pixels outside the bar of 1296 flat or 768 Healpix ones; * an event count changes too), as
problems() prints them:
  flat images, scalar opacities    PB 5    CL 13*   PS 11    HP 5          per-cell opacities   PB 4*   CL 21*   PS 17*   HP 14*
  Healpix image from inside        PB 10   CL 16*   PS 21    HP 10         MIRROR 21            PB 77*  CL 71*
  400 x 3 x 2 roots, two levels    PB 0    CL 0     (last bits only)       c400                 bit-identical, all eight
The old witness, oct104x6x5 (three levels), moves 0 pixels: tests/test_sca_instances.py keeps that on record.
"""
import math

import numpy as np

import cases
import split_cases as sc
from oracle.pyoracle import Job, ScaView
from soc_amd import files, launch, synth

BG, CL, PS, HP = 0, 1, 2, 3                                  # SOC_SCA_*: the kind of run_sca and oracle_sim_sca
KIND_NAME = {BG: "bg", CL: "cl", PS: "ps", HP: "hp"}
GRIDS = {(0, 0): "r759", (0, 1): "c400", (1, 0): "oct759", (1, 1): "deep104x6x5"}
DEEP = GRIDS[(1, 1)]

REACHABLE = {(k, o, d, a) for k in (BG, CL, PS, HP) for (o, d) in GRIDS for a in (0, 1)}

ANGLES = ((30.0, 40.0), (90.0, 0.0), (0.0, 0.0))
HPX_NSIDE = 8
MIN_CONTRIBUTIONS, MIN_SCATTERINGS, MIN_FLOAT_PIXELS = 1000, 100, 3

_MEMO = {}


def cloud(grid):
    if ("cloud", grid) not in _MEMO:
        _MEMO[("cloud", grid)] = synth.sca_instance_cloud(grid)
    return _MEMO[("cloud", grid)]


def _case(grid, kind, abu, weighted=0, mirror=0, hpx=None, items=3000, **launch_kw):
    """items: the launch runs its first `items` work items (all of them where it has fewer); hpx: the observer's position"""
    return dict(grid=grid, kind=kind, abu=abu, weighted=weighted, mirror=mirror, hpx=hpx, items=items, launch=launch_kw)


# the Healpix sky is weighted and plain in turn
CASES = {(k, o, d, a): _case(GRIDS[(o, d)], k, a, weighted=(o + d + a) % 2 if k == HP else 0) for (k, o, d, a) in REACHABLE}
# (with 2048 work items a walk in float moved 2 pixels of this one; the first 3000 of 4096 move 14 and change the counts)
CASES[(HP, 1, 1, 1)]["launch"] = dict(GLOBAL=4096)
# SimRAM_CL on the deep hierarchy sends a packet from every cell: all 1024 work items gave 2e5 to 4e5 contributions, thousands per lit
# pixel, and the order of the fp32 sums alone then moved a pixel by 7e-6 between two runs of the oracle and by 1e-5 to 2e-5 on the GPU
# (identical event counts).  The first 256 work items (64 with mirrors, 128 for the Healpix image) keep the sums short.
for _a in (0, 1):
    CASES[(CL, 1, 1, _a)]["items"] = 256
# The observer of the Healpix images, inside the hierarchy.  Of 40 random positions inside it 23 gave SimRAM_PB an infinite pixel (the
# reference's kernel gives the same: problems() refuses such a table); of the 17 others this one and (22.43, 4.53, 3.2) also let all
# four kinds tell a walk in float (10 / 45 / 21 / 10 pixels for PB / CL / PS / HP)
_INSIDE = (52.99, 5.16, 1.15)
EXTRA = {
    "hpx-bg": _case(DEEP, BG, 0, hpx=_INSIDE),
    "hpx-cl": _case(DEEP, CL, 1, hpx=_INSIDE, items=128),
    "hpx-ps": _case(DEEP, PS, 0, hpx=_INSIDE),
    "hpx-hp": _case(DEEP, HP, 1, weighted=1, hpx=_INSIDE),
    "mirror-bg": _case(DEEP, BG, 0, mirror=21),
    "mirror-cl": _case(DEEP, CL, 1, mirror=21, items=64),
    "l2float-bg": _case("oct104x6x5l2", BG, 0),
    "l2float-cl": _case("oct104x6x5l2", CL, 0),
    "l2double-bg": _case("oct400x3x2l2", BG, 0),
    "l2double-cl": _case("oct400x3x2l2", CL, 0),
    "nyfloat-bg": _case("oct6x104x5", BG, 0),
    "nyfloat-cl": _case("oct6x104x5", CL, 0),
}
CASES.update(EXTRA)


def case_id(key):
    return key if isinstance(key, str) else "%s-%d-%d-%d" % (KIND_NAME[key[0]], key[1], key[2], key[3])


def instance(key):
    """(kind, octree, dbl, abu): the instance a case runs, by soc_grid_variant's rule as sca_dispatch takes it"""
    k = CASES[key]
    c = cloud(k["grid"])
    return (k["kind"], int(c.LEVELS > 1), int(c.NX > (399 if c.LEVELS < 3 else 100)), k["abu"])


def group(key):
    """a grid and a kind"""
    return (CASES[key]["grid"], KIND_NAME[CASES[key]["kind"]])


def ref_tag(key):
    """the reference build of a case (oracle/build.py: sca_ref_models)"""
    k = CASES[key]
    return "si_" + k["grid"] + ("abu" if k["abu"] else "") + ("hpw" if k["weighted"] else "") + ("mir" if k["mirror"] else "")


def opacities(c):
    """(ABS, SCA): an optical depth of scattering of about 2 across the shortest side of the grid, ABS = 0.3 SCA"""
    root = c.DENS[:c.NX * c.NY * c.NZ]
    s = 2.0 / (min(c.NX, c.NY, c.NZ) * float(root[root > 0].mean()))
    return np.float32(0.3 * s), np.float32(s)


def point_sources(c):
    """one source inside the grid and one outside, above its upper z face"""
    return np.asarray([[0.5 * c.NX + 0.3, 0.5 * c.NY + 0.2, 0.5 * c.NZ + 0.1], [0.4 * c.NX, 0.5 * c.NY + 0.2, c.NZ + 6.0]], np.float32)


def job(key):
    k = CASES[key]
    c = cloud(k["grid"])
    a, s = opacities(c)
    ps = point_sources(c)
    # (the reference builds of these grids are made for two point sources, -D NO_PS=2: every job carries them, SimRAM_PS sends from them)
    kw = dict(ABS=a, SCA=s, DSC=cases._DSC, MIRROR=k["mirror"], PSPOS=ps, PS=[1.0, 2.0],
              XPS=files.analyse_external_point_sources(c.NX, c.NY, c.NZ, ps, len(ps), 0))
    if k["abu"]:
        kw["OPT"] = sc.per_cell_opt(c, a, s)
    if k["kind"] == BG:
        kw.update(SOURCE=1, BATCH=2, SEED=0.377)
    elif k["kind"] == PS:
        kw.update(SOURCE=0, GLOBAL=512, BATCH=12, SEED=0.2)
    elif k["kind"] == CL:
        kw.update(SOURCE=2, GLOBAL=1024, BATCH=1, SEED=0.9, EMIT=cases._emit(c))
    else:
        sky, P = cases.hp_sky(weighted=bool(k["weighted"]))
        kw.update(GLOBAL=2048, BATCH=16, SEED=0.11, HPBG=sky, HPBGP=P)
    kw.update(k["launch"])
    return Job(c, cases._CSC, **kw)


def view(key):
    """Healpix image seen from inside, or three flat images centred on the grid: 54 x 8 pixels of 1/52 of the longest side on the
    long grids, 14 x 11 pixels of one cell on the 7 x 5 x 9 ones"""
    k = CASES[key]
    c = cloud(k["grid"])
    if k["hpx"] is not None:
        return cases.sca_view(healpix=(HPX_NSIDE, k["hpx"]))
    n = max(c.NX, c.NY, c.NZ)
    NPIX, MAP_DX = ((14, 11), 1.0) if n < 52 else ((54, 8), n / 52.0)
    _, OD, RA, DE = launch.set_observer_directions([math.radians(t) for t, _ in ANGLES], [math.radians(p) for _, p in ANGLES])
    return ScaView(OD, RA, DE, NPIX=NPIX, MAP_DX=MAP_DX, CENTRE=(0.5 * c.NX, 0.5 * c.NY, 0.5 * c.NZ), FFS=1)


def items(key):
    """(gid_first, gid_count) of the case's launch"""
    return 0, min(job(key).GLOBAL, CASES[key]["items"])


def expected(key, orc=None, nthreads=8):
    """The oracle's result of a case in soc mode, computed once: (image, contributions, packets, scatterings)"""
    from oracle.pyoracle import Oracle, oracle_sca_counts, oracle_sim_sca
    memo = orc is None
    if memo and ("want", key) in _MEMO:
        return _MEMO[("want", key)]
    if orc is None:
        if "soc" not in _MEMO:
            _MEMO["soc"] = Oracle("soc")
        orc = _MEMO["soc"]
    g0, n = items(key)
    img, nadd = oracle_sim_sca(orc, job(key), view(key), CASES[key]["kind"], gid0=g0, gid1=g0 + n, nthreads=nthreads)
    out = (img, nadd) + oracle_sca_counts(orc)
    if memo:
        _MEMO[("want", key)] = out
    return out


def outside_the_bar(got, want, rtol=1e-5):
    """pixels of `got` that test_gpu_sca.assert_image_close would refuse against `want`"""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return int((np.abs(got - want) > rtol * np.abs(want) + 1e-6 * rtol * np.abs(want).max()).sum())


def float_walk_differs(key):
    """(pixels outside the bar, event counts changed, image bit-identical) when Index() is made to run in float:
    oracle.pyoracle.double_index forced to 0, as split_cases.float_walk_differs does for the tallies of the split kernels"""
    import oracle.pyoracle
    from oracle.pyoracle import Oracle
    if ("float", key) not in _MEMO:
        orc = Oracle("soc")
        want = expected(key, orc=orc, nthreads=1)           # (one thread: the same order of the sums in both, so the figure is reproducible)
        keep = oracle.pyoracle.double_index
        oracle.pyoracle.double_index = lambda NX, LEVELS: 0
        try:
            got = expected(key, orc=orc, nthreads=1)
        finally:
            oracle.pyoracle.double_index = keep
        _MEMO[("float", key)] = (outside_the_bar(got[0], want[0]), got[1:] != want[1:],
                                 np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)))
    return _MEMO[("float", key)]


def double_index_matters(key):
    """Whether a case on a grid with Index() in double is held to the float-walk condition: from three levels on.  At level 0 Index()
    has no double arithmetic, and problems() checks that a walk in float is bit-identical there (c400).  With two levels the double
    walk differs from the float one only in the last bits -- a position carried from a refined root cell into a refined neighbour
    keeps its fraction where float rounds it to an ulp of a number below 512, 3e-5 -- and on 400 x 3 x 2 roots that moved no event
    count and no pixel past the bar (measured: 0 of 1296, for both kinds), so those two cases check dispatch and parity only."""
    return cloud(CASES[key]["grid"]).LEVELS >= 3


def tells_a_float_walk(key):
    pixels, counts, _ = float_walk_differs(key)
    return bool(counts or pixels >= MIN_FLOAT_PIXELS)


def problems(verbose=False):
    bad = []
    if set(k for k in CASES if not isinstance(k, str)) != REACHABLE or len(REACHABLE) != 32 or len(EXTRA) != 12:
        bad.append("the cases are not the 32 instances and 12 more")
    told = {}
    for key in CASES:
        name = case_id(key)
        k = CASES[key]
        if not isinstance(key, str) and instance(key) != key:
            bad.append("%s: the grid gives instance %s" % (name, instance(key)))
        img, nadd, npkt, nscat = expected(key)
        if nadd < MIN_CONTRIBUTIONS or nscat < MIN_SCATTERINGS:
            bad.append("%s: %d image contributions, %d scatterings" % (name, nadd, nscat))
        if not np.isfinite(img).all():
            bad.append("%s: the expected image is not finite" % name)
        if not ((img > 0).any() and (img == 0).any()):
            bad.append("%s: %d lit and %d dark pixels" % (name, (img > 0).sum(), (img == 0).sum()))
        _, octree, dbl, _ = instance(key)
        if dbl:
            pixels, counts, identical = float_walk_differs(key)
            if verbose:
                print("%-14s float walk: %3d pixels outside the bar, event counts %s%s" % (
                    name, pixels, "differ" if counts else "equal", ", image bit-identical" if identical else ""))
            if octree and double_index_matters(key):
                told.setdefault(group(key), []).append(tells_a_float_walk(key))
                if not tells_a_float_walk(key):
                    bad.append("%s: a walk in float moves %d pixels and no event count" % (name, pixels))
            elif not octree and (counts or not identical):
                bad.append("%s: a walk in float is not bit-identical on a single-level grid (%d pixels)" % (name, pixels))
        if verbose:
            print("%-14s %-13s contributions %6d packets %6d scatterings %6d lit %4d / %d" % (
                name, k["grid"], nadd, npkt, nscat, (img > 0).sum(), img.size))
    for g, t in told.items():
        if not any(t):
            bad.append("group %s-%s: no case tells a walk in float from one in double" % g)
    if set(told) != {(DEEP, n) for n in KIND_NAME.values()}:
        bad.append("the groups that tell a walk in float are %s" % sorted(told))
    return bad
