"""The two partitions of soc_amd/csrc/soc_lbricks.h on the CPU: the tiles of 16^3 root cells, halved (SOC_LB_TILES), and the one the
builder makes by default -- of the tiles and the slabs the partition with the smaller total face area (SOC_LB_BEST).  Both must be
partitions of the root grid into boxes of at most `cap` cells with every cell in exactly one slot; the default's face area is never
the larger one, and on the hierarchies of the bench's kind it is smaller by the factors below.  Then rays through the bricks of the
default, every step the oracle's.  The builder runs in tests/csrc/lbricks_fill_host.cpp, a program of its own built with
-fsanitize=address,undefined (tests/lbricks_fill.py)."""
import numpy as np
import pytest

from lbricks_fill import BEST, TILES, run
from oracle.pyoracle import Job
from soc_amd import synth
from test_ltree import RAGGED, _rays

_MEMO = {}


def ball_cloud(N=40, r=7.0, depth=3):
    """a clustered model: every root cell within r of (0.4, 0.55, 0.5) N is refined, and so is everything below it, `depth` levels
    deep; nothing outside the ball is"""
    rng = np.random.default_rng(17)
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    inside = ((x + 0.5 - 0.4 * N) ** 2 + (y + 0.5 - 0.55 * N) ** 2 + (z + 0.5 - 0.5 * N) ** 2 <= r * r).ravel()
    H = [rng.uniform(1.0, 2.0, N ** 3).astype(np.float32)]
    parents = np.flatnonzero(inside)
    for l in range(depth):
        H[l][parents] = -synth.I2F((8 * np.arange(len(parents))).astype(np.int32)).astype(np.float32)
        H.append(rng.uniform(1.0, 2.0, 8 * len(parents)).astype(np.float32))
        parents = np.arange(8 * len(parents))
    return synth.Cloud(N, N, N, H)


CLOUDS = {
    "oct64_l4": lambda: synth.octree_cloud(64, levels=4),
    "oct64_l3": lambda: synth.octree_cloud(64, levels=3),
    "oct128_l3": lambda: synth.octree_cloud(128, levels=3),
    "oct104_l4": lambda: synth.octree_cloud(104, levels=4, frac=0.08, seed=3),
    "ball40": ball_cloud,
}


def cloud(name):
    if name not in _MEMO:
        _MEMO[name] = CLOUDS[name]() if name in CLOUDS else synth.noncubic_cloud(name)
    return _MEMO[name]


def check(cl, cap, B):
    """what the device relies on: a partition of the root grid, rbrick the brick of every root cell, no brick above cap, every cell in
    exactly one slot with its density or the link to its children (lt_check)"""
    assert B.ok and B.check == 0 and B.slots == cl.CELLS
    assert 0 < B.max_slots <= cap and B.boxes[:, 6].max() == B.max_slots and int(B.boxes[:, 6].sum()) == cl.CELLS
    count = np.zeros((cl.NZ, cl.NY, cl.NX), np.int32)
    for b, (x0, y0, z0, bx, by, bz, n) in enumerate(B.boxes):
        assert bx >= 1 and by >= 1 and bz >= 1 and x0 >= 0 and y0 >= 0 and z0 >= 0 and x0 + bx <= cl.NX and y0 + by <= cl.NY and z0 + bz <= cl.NZ
        count[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] += 1
        assert (B.rbrick[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] == b).all()
    assert (count == 1).all()


CASES = ([(n, c) for n in ("oct64_l4", "oct64_l3", "oct128_l3") for c in (8704, 5888, 600)] + [("oct104_l4", 8704), ("oct104_l4", 600)]
         + RAGGED + [("oct759", 1139), ("oct104x6x5", 12288)] + [("ball40", 8704), ("ball40", 600)])
# the default's face area against the tiles': measured by a count-balanced prototype 0.81 on these two
SMALLER = {("oct64_l3", 8704): 0.85, ("oct128_l3", 8704): 0.85}


@pytest.mark.parametrize("name,cap", CASES)
def test_both_partitions_are_partitions_and_the_default_has_no_more_area(name, cap):
    cl = cloud(name)
    old = run(cl, cap, TILES)
    new = run(cl, cap, BEST)
    check(cl, cap, old)
    check(cl, cap, new)
    assert not old.slabs and old.n_slabs == 0 and old.area() == old.area_tiles
    assert new.area_tiles == old.area_tiles and new.n_tiles == len(old.boxes)
    assert new.area() == (new.area_slabs if new.slabs else new.area_tiles)
    print("%s cap %d: tiles %d bricks, area %d; default %d bricks, area %d (%.3f), %s" % (
        name, cap, len(old.boxes), old.area(), len(new.boxes), new.area(), new.area() / old.area(), "slabs" if new.slabs else "tiles"))
    assert new.area() <= old.area()
    if not new.slabs:
        assert np.array_equal(new.boxes, old.boxes)              # a tie, or the tiles smaller: the tiles themselves
    assert new.area() <= SMALLER.get((name, cap), 1.0) * old.area()
    again = run(cl, cap, BEST, boxes_only=True)
    assert np.array_equal(again.boxes, new.boxes)                # the same grid and cap: the same bricks


def test_a_root_cell_above_the_cap_is_refused_by_both():
    deep = synth.octree_cloud(4, levels=4, frac=0.5, seed=1)
    assert not run(deep, 64, TILES).ok and not run(deep, 64, BEST).ok
    assert not run(cloud("ball40"), 584, BEST).ok and run(cloud("ball40"), 585, BEST).ok      # 1 + 8 + 64 + 512 cells below a root cell


def test_face_area_on_the_geometry_of_the_bench():
    """256^3 roots, 4 levels, 49 526 352 cells at 8704 cells per brick: the boxes of both partitions without the bricks themselves.
    The tiles: 8194 boxes with a face area of 8.389e6; the prototype reached 0.863 of that."""
    cl = synth.octree_cloud(256, levels=4, frac=0.10, seed=1234)
    B = run(cl, 8704, BEST, boxes_only=True)
    assert B.ok and B.slabs and B.n_tiles == 8194 and B.area_tiles == 8389120.0
    n = B.boxes[:, 6]
    print("C3 at 8704: %d boxes, fill %.3f, face area %.4g = %.4f of the tiles'" % (len(n), n.mean() / 8704, B.area(), B.area() / B.area_tiles))
    assert n.max() <= 8704 and int(n.sum()) == cl.CELLS
    vol = B.boxes[:, 3].astype(np.int64) * B.boxes[:, 4] * B.boxes[:, 5]
    assert int(vol.sum()) == 256 ** 3
    assert B.area() <= 0.88 * B.area_tiles


@pytest.mark.parametrize("cap", [600, 8704])
def test_steps_through_the_default_bricks_are_the_oracles_steps(cap, oracle_soc):
    """tests/test_ltree.py::test_local_tree_steps_are_the_oracles_steps on bricks whose boxes lie on no tile's grid: level, cell, step length
    and end position of every ray, bit for bit"""
    cl = cloud("oct104_l4")
    pos, u = _rays(cl, 3000, np.random.default_rng(11))
    B = run(cl, cap, BEST, pos, u)
    assert B.ok and B.slabs and B.check == 0
    edges = B.boxes[:, 3:6]
    assert ((B.boxes[:, :3] % 16 != 0).any(axis=1)).mean() > 0.5 and len(np.unique(edges)) > 4      # not the tiles
    if cap == 8704:
        assert edges.max() > 16
    job = Job(cl, np.linspace(1, -1, 16).astype(np.float32))
    steps = slow = 0
    deeper = set()
    for i, (lev, cel, ds, end, st) in enumerate(B.rays):
        assert st in (0, 2), "ray %d: status %d" % (i, st)
        olev, oind, ods, oend = oracle_soc.trace(job, pos[i], u[i], maxsteps=20000)
        n = len(lev)
        if st == 2:                      # stopped where the generic Index() has to decide: compare what was walked
            slow += 1
            assert n <= len(olev)
        else:
            assert n == len(olev), "ray %d: %d steps, oracle %d" % (i, n, len(olev))
            assert np.array_equal(end.view(np.uint32), oend.view(np.uint32)), "ray %d: end position" % i
        assert np.array_equal(lev, olev[:n]) and np.array_equal(cel, cl.OFF[olev[:n]] + oind[:n]), "ray %d: cells differ" % i
        assert np.array_equal(ds.view(np.uint32), ods[:n].view(np.uint32)), "ray %d: step lengths differ" % i
        steps += n
        deeper.update(lev.tolist())
    assert steps > 120000 and deeper == set(range(cl.LEVELS))
    assert slow < 0.02 * len(pos)
