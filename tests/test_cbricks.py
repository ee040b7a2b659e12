"""The brick cutter of single-level grids (soc_amd/csrc/soc_lbricks.h: soc_cbricks_build), whose bricks the sweep of rays on Cartesian
grids walks: every root cell in exactly one brick and one slot, boxes that tile the grid, the brick numbers of face neighbours
consistent with the boxes, edges that are no multiple of the brick edge or shorter than it.  The harness tests/cbricks_host.cpp
compiles the product header with g++."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
_I = np.ctypeslib.ndpointer(np.int32, flags="C")
_F = np.ctypeslib.ndpointer(np.float32, flags="C")


def _harness():
    out = os.path.join(REPO, "oracle", "_build", "libcbricks_host.so")
    src = os.path.join(HERE, "cbricks_host.cpp")
    deps = [src] + [os.path.join(REPO, "soc_amd", "csrc", f) for f in ("soc_ltree.h", "soc_lbricks.h", "soc_math.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", out, src])
    return out


@pytest.fixture(scope="module")
def lib():
    L = C.CDLL(_harness())
    L.cb_build.restype = C.c_void_p
    L.cb_build.argtypes = [C.c_int] * 3 + [_F, C.c_int]
    L.cb_nslots.restype = C.c_long
    for f in (L.cb_free, L.cb_ok, L.cb_nbricks, L.cb_max_slots, L.cb_nslots):
        f.argtypes = [C.c_void_p]
    L.cb_read.argtypes = [C.c_void_p, _I, _I, _I, _F]
    return L


def cut(L, NX, NY, NZ, edge, dens=None):
    cells = NX * NY * NZ
    dens = np.random.default_rng(NX + 7 * NY + 31 * NZ).uniform(0.5, 2.0, cells).astype(np.float32) if dens is None else dens
    h = L.cb_build(NX, NY, NZ, dens, edge)
    try:
        if not L.cb_ok(h):
            return None
        nb, ns = L.cb_nbricks(h), L.cb_nslots(h)
        boxes, rbrick = np.zeros((nb, 8), np.int32), np.zeros(cells, np.int32)
        bcell, btree = np.zeros(ns, np.int32), np.zeros(ns, np.float32)
        L.cb_read(h, boxes, rbrick, bcell, btree)
        return dens, boxes, rbrick.reshape(NZ, NY, NX), bcell, btree, L.cb_max_slots(h)
    finally:
        L.cb_free(h)


@pytest.mark.parametrize("shape,edge", [((40, 36, 50), 16), ((40, 36, 50), 9), ((104, 104, 104), 16), ((5, 3, 70), 16), ((1, 1, 1), 4),
                                        ((16, 32, 48), 16), ((17, 16, 15), 16), ((7, 7, 7), 1), ((33, 2, 9), 8)])
def test_every_root_cell_in_exactly_one_brick(shape, edge, lib):
    NX, NY, NZ = shape
    dens, boxes, rbrick, bcell, btree, max_slots = cut(lib, NX, NY, NZ, edge)
    cells = NX * NY * NZ
    # the slots are a permutation of the cells and hold their densities
    assert bcell.size == cells and np.array_equal(np.sort(bcell), np.arange(cells))
    assert np.array_equal(btree, dens[bcell])
    # boxes: inside the grid, at most edge cells per axis, the short ones at the far faces only; they tile the grid
    nbx, nby, nbz = -(-NX // edge), -(-NY // edge), -(-NZ // edge)
    assert boxes.shape[0] == nbx * nby * nbz
    count = np.zeros((NZ, NY, NX), np.int32)
    for b, (x0, y0, z0, bx, by, bz, base, nslot) in enumerate(boxes):
        assert 1 <= bx <= edge and 1 <= by <= edge and 1 <= bz <= edge and nslot == bx * by * bz
        assert x0 % edge == 0 and y0 % edge == 0 and z0 % edge == 0
        assert bx == min(edge, NX - x0) and by == min(edge, NY - y0) and bz == min(edge, NZ - z0)
        count[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] += 1
        assert (rbrick[z0:z0 + bz, y0:y0 + by, x0:x0 + bx] == b).all()
        # slot of cell (x, y, z) of the box: ((z - z0) * by + (y - y0)) * bx + (x - x0) -- what the walk computes
        z, y, x = np.meshgrid(np.arange(z0, z0 + bz), np.arange(y0, y0 + by), np.arange(x0, x0 + bx), indexing="ij")
        assert np.array_equal(bcell[base:base + nslot], ((z * NY + y) * NX + x).ravel())
    assert (count == 1).all()
    assert max_slots == boxes[:, 7].max() and boxes[:, 7].sum() == cells
    assert np.array_equal(np.sort(boxes[:, 6]), np.concatenate([[0], np.cumsum(boxes[:, 7])[:-1]]))


@pytest.mark.parametrize("shape,edge", [((40, 36, 50), 16), ((5, 3, 70), 16), ((33, 2, 9), 8)])
def test_face_neighbours_brick_numbers(shape, edge, lib):
    """a step across a cell face stays in the brick or enters the brick whose box holds the neighbour: the neighbour's brick
    differs exactly where the face is a face of the box, and the two boxes touch there"""
    NX, NY, NZ = shape
    _, boxes, rbrick, _, _, _ = cut(lib, NX, NY, NZ, edge)
    for axis, n in ((2, NX), (1, NY), (0, NZ)):
        a = np.take(rbrick, np.arange(n - 1), axis=axis)
        b = np.take(rbrick, np.arange(1, n), axis=axis)
        coord = np.arange(1, n).reshape([-1 if i == axis else 1 for i in range(3)])      # coordinate of the second cell
        on_face = np.broadcast_to(coord % edge == 0, a.shape)
        assert np.array_equal(a != b, on_face)
        k = {2: 0, 1: 1, 0: 2}[axis]
        lo, hi = boxes[a[a != b]], boxes[b[a != b]]
        assert (lo[:, k] + lo[:, 3 + k] == hi[:, k]).all()                 # the boxes touch along the axis ...
        for o in range(3):
            if o != k:
                assert (lo[:, o] == hi[:, o]).all() and (lo[:, 3 + o] == hi[:, 3 + o]).all()      # ... and agree across it


def test_a_cell_without_density_is_refused(lib):
    dens = np.ones(4 * 5 * 6, np.float32)
    assert cut(lib, 4, 5, 6, 4, dens) is not None
    for bad in (0.0, -1.0, np.nan):
        d = dens.copy()
        d[37] = bad
        assert cut(lib, 4, 5, 6, 4, d) is None
    assert cut(lib, 4, 5, 6, 0, dens) is None
