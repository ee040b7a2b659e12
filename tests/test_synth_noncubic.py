"""synth.octree_cloud with a root grid whose sides differ (NY, NZ), and the named models of synth.NONCUBIC.

With NY and NZ left out the generator must return what it returned before it had them, bit for bit: every golden file of the
hierarchies was recorded on those arrays."""
import os

import numpy as np
import pytest

from soc_amd import synth


def _octree_cloud_cubic(N, levels, frac, seed, sigma=0.3):
    """the generator as it was when it could build cubes only (lognormal densities), kept here as the yardstick"""
    rng = np.random.default_rng(seed)
    d0 = np.clip(np.exp(rng.standard_normal(N * N * N)) * 1.0e3, 1.0, 1.0e5)
    H = [d0]
    for l in range(levels - 1):
        cur = H[l]
        n_ref = int(round(frac * len(cur)))
        if n_ref < 1:
            break
        parents = np.sort(np.argpartition(cur, len(cur) - n_ref)[len(cur) - n_ref:])
        w = np.exp(sigma * rng.standard_normal((n_ref, 8)))
        w *= 8.0 / w.sum(axis=1, keepdims=True)
        H.append((cur[parents][:, None] * w).reshape(-1))
        cur = cur.astype(np.float32)
        cur[parents] = -synth.I2F((8 * np.arange(n_ref)).astype(np.int32)).astype(np.float32)
        H[l] = cur
    H = [np.asarray(h, np.float32) for h in H]
    for h in H:
        h[h > 0] = np.maximum(h[h > 0], 1.0e-6)
    return H


@pytest.mark.parametrize("N,levels,frac,seed", [(8, 3, 0.15, 7), (104, 3, 0.002, 11), (104, 4, 0.08, 3)])
def test_cubic_clouds_of_the_goldens_are_unchanged(N, levels, frac, seed):
    c = synth.octree_cloud(N, levels=levels, frac=frac, seed=seed)
    H = _octree_cloud_cubic(N, levels, frac, seed)
    assert (c.NX, c.NY, c.NZ) == (N, N, N) and c.LEVELS == len(H)
    want = np.concatenate(H)
    assert c.DENS.dtype == np.float32 and np.array_equal(c.DENS.view(np.uint32), want.view(np.uint32))
    assert list(c.LCELLS) == [len(h) for h in H]
    # the same with the sides spelled out
    c2 = synth.octree_cloud(N, levels=levels, frac=frac, seed=seed, NY=N, NZ=N)
    assert np.array_equal(c2.DENS.view(np.uint32), want.view(np.uint32))
    if N == 8:                                                 # ... and the array a golden file recorded
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sims.npz"))
        assert np.array_equal(c.DENS.view(np.uint32), g["bg_oct8_DENS"].view(np.uint32))


def test_uniform_cubic_cloud_is_unchanged():
    a = synth.octree_cloud(4, levels=2, frac=1.0, uniform=1.0e3)
    assert list(a.LCELLS) == [64, 512] and (a.DENS[64:] == np.float32(1.0e3)).all() and (a.DENS[:64] <= 0).all()


def test_named_models_and_their_cell_counts():
    assert set(synth.NONCUBIC) == {"r759", "oct759", "oct104x6x5", "oct6x104x5", "oct5x6x104", "r208x6x5", "r6x208x5"}
    levels = {"r759": [315], "oct759": [315, 376, 448], "oct104x6x5": [3120, 1248, 496], "oct6x104x5": [3120, 1248, 496],
              "oct5x6x104": [3120, 1248, 496, 200], "r208x6x5": [6240], "r6x208x5": [6240]}
    for name, k in synth.NONCUBIC.items():
        c = synth.noncubic_cloud(name)
        assert (c.NX, c.NY, c.NZ) == tuple(k[:3]) and len({c.NX, c.NY, c.NZ}) == 3
        assert c.CELLS == synth.NONCUBIC_CELLS[name] and list(c.LCELLS) == levels[name]
        assert c.AREA == 2 * (c.NX * c.NY + c.NY * c.NZ + c.NZ * c.NX)
        # a well-formed hierarchy: every link names an octet of the next level, every octet has one parent
        for l in range(c.LEVELS - 1):
            d = c.DENS[c.OFF[l]:c.OFF[l] + c.LCELLS[l]]
            first = np.sort(synth.F2I(-d[d <= 0]))
            assert np.array_equal(first, 8 * np.arange(c.LCELLS[l + 1] // 8))
        assert (c.DENS[c.OFF[-1]:] > 0).all()
    # Index() runs in double iff NX > 100 with three levels or more: the three slabs differ in exactly that
    from oracle.pyoracle import double_index
    assert [double_index(synth.NONCUBIC[n][0], 3) for n in ("oct104x6x5", "oct6x104x5", "oct5x6x104")] == [1, 0, 0]
    # the same root densities in the same order whatever the sides: the generator draws NX * NY * NZ values first
    a, b = synth.noncubic_cloud("oct104x6x5"), synth.noncubic_cloud("oct6x104x5")
    assert np.array_equal(a.DENS, b.DENS)
