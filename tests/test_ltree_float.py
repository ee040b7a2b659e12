"""The FLOAT form of the brick-local Index() (soc_amd/csrc/soc_ltree.h: soc_lt_aim_flt / soc_lt_land_flt) on the CPU, for
hierarchies on which the reference evaluates Index() with float3 POS (NX <= 100, or <= 399 with two levels): the climb fma by fma,
then the integer descent, against the oracle's restatement of kernel_ASOC_aux.c:198-278 (float POS), ray by ray and bit for bit.
The harness tests/ltree_float_host.cpp compiles the product headers with g++; a stand-alone build of it runs under sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import Job
from soc_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
_F, _I = C.POINTER(C.c_float), C.POINTER(C.c_int)
INSIDE, LEAVE, EXIT, SLOW = 0, 1, 2, 3                         # soc_ltree.h: SOC_LT_*

SRC = os.path.join(HERE, "ltree_float_host.cpp")
DEPS = [SRC] + [os.path.join(REPO, "soc_amd", "csrc", f) for f in ("soc_ltree.h", "soc_lbricks.h", "soc_math.h")]


def _build(out, flags):
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++"] + flags + ["-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-Wall", "-o", out, SRC])
    return out


def _harness():
    return _build(os.path.join(REPO, "oracle", "_build", "libltree_float_host.so"), ["-O2", "-fPIC", "-shared"])


class LTreeF:
    def __init__(self, cloud, cap):
        self.lib = L = C.CDLL(_harness())
        L.ltf_build.restype = C.c_void_p
        L.ltf_build.argtypes = [C.c_int] * 4 + [_I, _I, _F, C.c_int]
        L.ltf_free.argtypes = [C.c_void_p]
        L.ltf_info.argtypes = [C.c_void_p, _I, _I, C.POINTER(C.c_long)]
        L.ltf_locate.argtypes = [C.c_void_p, _F, _I, _I, _F]
        L.ltf_step.argtypes = [C.c_void_p, _I, _I, _F]
        L.ltf_trace_move.restype = C.c_int
        L.ltf_trace_move.argtypes = [C.c_void_p, _F, _F, C.c_int, _I, _I, _F, _F, _I]
        self.cloud = cloud
        self.LCELLS = np.ascontiguousarray(cloud.LCELLS, np.int32)
        self.OFF = np.ascontiguousarray(cloud.OFF, np.int32)
        self.DENS = np.ascontiguousarray(cloud.DENS, np.float32)
        self.h = L.ltf_build(cloud.NX, cloud.NY, cloud.NZ, cloud.LEVELS, self.LCELLS.ctypes.data_as(_I), self.OFF.ctypes.data_as(_I),
                             self.DENS.ctypes.data_as(_F), cap)
        self._lev = np.zeros(20000, np.int32)
        self._cel = np.zeros(20000, np.int32)
        self._ds = np.zeros(20000, np.float32)

    def info(self):
        nb, ms, ns = C.c_int(), C.c_int(), C.c_long()
        self.lib.ltf_info(self.h, C.byref(nb), C.byref(ms), C.byref(ns))
        return nb.value, ms.value, ns.value

    def trace(self, pos, d):
        pos = np.ascontiguousarray(pos, np.float32)
        d = np.ascontiguousarray(d, np.float32)
        end = np.zeros(3, np.float32)
        st = C.c_int()
        n = self.lib.ltf_trace_move(self.h, pos.ctypes.data_as(_F), d.ctypes.data_as(_F), len(self._lev), self._lev.ctypes.data_as(_I),
                                    self._cel.ctypes.data_as(_I), self._ds.ctypes.data_as(_F), end.ctypes.data_as(_F), C.byref(st))
        return self._lev[:n].copy(), self._cel[:n].copy(), self._ds[:n].copy(), end, st.value

    def locate(self, pos):
        pos = np.ascontiguousarray(pos, np.float32)
        lev, c, loc = C.c_int(), np.zeros(3, np.int32), np.zeros(3, np.float32)
        r = self.lib.ltf_locate(self.h, pos.ctypes.data_as(_F), C.byref(lev), c.ctypes.data_as(_I), loc.ctypes.data_as(_F))
        return r, lev.value, c, loc

    def step(self, level, c, pos):
        lev, c, pos = C.c_int(level), np.ascontiguousarray(c, np.int32).copy(), np.ascontiguousarray(pos, np.float32).copy()
        r = self.lib.ltf_step(self.h, C.byref(lev), c.ctypes.data_as(_I), pos.ctypes.data_as(_F))
        return r, lev.value, c, pos

    def close(self):
        if self.h:
            self.lib.ltf_free(self.h)
            self.h = None


def _rays(cloud, n, rng):
    """the ray generator of tests/test_ltree.py: starting points on the faces and inside, directions with the reference's clamp
    (|u| >= DEPS) and normalisation, one in ten grazing"""
    N = np.asarray([cloud.NX, cloud.NY, cloud.NZ], np.float32)
    pos = (rng.random((n, 3)) * (N - 2e-4) + 1e-4).astype(np.float32)
    face = rng.integers(0, 7, n)
    for i in range(n):
        if face[i] < 6:
            a = face[i] // 2
            pos[i, a] = np.float32(1e-4) if face[i] % 2 == 0 else np.float32(N[a] - 1e-4)
    u = rng.standard_normal((n, 3)).astype(np.float32)
    grazing = rng.random(n) < 0.1
    u[grazing, rng.integers(0, 3)] *= np.float32(1e-5)
    u = np.where(np.abs(u) < 5e-5, np.float32(5e-5), u)
    u /= np.sqrt((u.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32))[:, None]
    return pos, u.astype(np.float32)


# hierarchies with Index() in float: NX <= 100 with three or more levels, NX <= 399 with two (kernel_ASOC_aux.c:25-37)
CLOUDS = {
    "oct64_l4": lambda: synth.octree_cloud(64, levels=4, frac=0.08, seed=3),
    "oct104_l2": lambda: synth.octree_cloud(104, levels=2, frac=0.08, seed=3),      # one level of climb onto a 104-cell root grid
    "oct8_l3": lambda: synth.octree_cloud(8, levels=3, frac=0.15, seed=7),          # the oct8 of tests/cases.py
    "oct759": lambda: synth.noncubic_cloud("oct759"),
}
# (cloud, cells per brick, rays, steps expected at least)
CASES = [("oct64_l4", 6144, 3000, 100000), ("oct64_l4", 700, 3000, 100000), ("oct104_l2", 6144, 2000, 80000),
         ("oct8_l3", 6144, 3000, 12000), ("oct759", 200, 3000, 12000)]      # (the small grids: four steps a ray and more)


@pytest.mark.parametrize("name,cap,nrays,minsteps", CASES)
def test_float_form_steps_are_the_oracles_steps(name, cap, nrays, minsteps, oracle_soc):
    cloud = CLOUDS[name]()
    lt = LTreeF(cloud, cap)
    assert lt.h, "bricks could not be built"
    nb, ms, ns = lt.info()
    assert ms <= cap and ns == cloud.CELLS
    job = Job(cloud, np.linspace(1, -1, 16).astype(np.float32))
    pos, u = _rays(cloud, nrays, np.random.default_rng(11))
    steps = slow = 0
    deeper = set()
    for i in range(len(pos)):
        lev, cel, ds, end, st = lt.trace(pos[i], u[i])
        assert st in (0, 2), "ray %d: status %d" % (i, st)
        olev, oind, ods, oend = oracle_soc.trace(job, pos[i], u[i], maxsteps=20000)
        n = len(lev)
        if st == 2:                      # stopped where the generic Index() has to decide: compare what was walked
            slow += 1
            assert n <= len(olev)
        else:
            assert n == len(olev), "ray %d: %d steps, oracle %d" % (i, n, len(olev))
            assert np.array_equal(end.view(np.uint32), oend.view(np.uint32)), "ray %d: end position %r, oracle %r" % (i, end, oend)
        ocell = cloud.OFF[olev[:n]] + oind[:n]
        assert np.array_equal(lev, olev[:n]) and np.array_equal(cel, ocell), "ray %d: cells differ" % i
        assert np.array_equal(ds.view(np.uint32), ods[:n].view(np.uint32)), "ray %d: step lengths differ" % i
        steps += n
        deeper.update(lev.tolist())
    print("%s cap %d: %d bricks, %d rays, %d steps, %d rays stopped at a slow step" % (name, cap, nb, len(pos), steps, slow))
    assert steps > minsteps and deeper == set(range(cloud.LEVELS))
    assert slow <= 0.02 * len(pos)
    lt.close()


def test_a_stop_at_exactly_two_goes_to_the_slow_queue():
    """pos = 2.0f on an axis, in a cell whose parent's octant bit on that axis is 1: the climb gives P = 2.0f * 0.5f + 1 = 2.0f, the
    inclusive test of kernel_ASOC_aux.c:254 accepts it and floor() indexes past the octet -- SOC_LT_SLOW.  The same position in a
    cell whose parent's bit is 0 gives P = 1.0f: an ordinary step."""
    cloud = CLOUDS["oct64_l4"]()
    lt = LTreeF(cloud, 6144)
    rng = np.random.default_rng(2)
    seen = {0: 0, 1: 0}
    for _ in range(20000):
        p = (rng.random(3) * 63.9 + 0.05).astype(np.float32)
        r, level, c, loc = lt.locate(p)
        if r != INSIDE or level < 2:
            continue
        for axis in range(3):
            bit = int((c[axis] >> 1) & 1)
            q = loc.copy()
            q[axis] = np.float32(2.0)
            r2, l2, c2, p2 = lt.step(level, c, q)
            if bit == 1:
                assert r2 == SLOW, (level, c, axis, r2)
            else:
                assert r2 == INSIDE and (c2[axis] >> l2) == (c[axis] >> level), (level, c, axis, r2, c2)
            seen[bit] += 1
        if min(seen.values()) > 50:
            break
    assert min(seen.values()) > 50
    lt.close()


def _write_case(path, cloud, cap, pos, u):
    with open(path, "wb") as f:
        np.asarray([cloud.NX, cloud.NY, cloud.NZ, cloud.LEVELS, cap, len(pos)], np.int32).tofile(f)
        np.ascontiguousarray(cloud.LCELLS, np.int32).tofile(f)
        np.ascontiguousarray(cloud.OFF, np.int32).tofile(f)
        np.ascontiguousarray(cloud.DENS, np.float32).tofile(f)
        np.concatenate([pos, u], axis=1).astype(np.float32).tofile(f)


def test_float_form_under_sanitizers(tmp_path):
    """the harness as a stand-alone program built with -fsanitize=address,undefined, on a hierarchy that is no multiple of the
    16-cell tile with small bricks, on oct759, and on one whose bricks cannot be built"""
    exe = _build(os.path.join(REPO, "oracle", "_build", "ltree_float_host_san"),
                 ["-O1", "-DLTF_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    jobs = [(synth.octree_cloud(19, levels=4, frac=0.2, seed=2), 600, 300), (synth.noncubic_cloud("oct759"), 200, 300),
            (synth.octree_cloud(4, levels=4, frac=0.5, seed=1), 64, 10)]
    for k, (cloud, cap, n) in enumerate(jobs):
        pos, u = _rays(cloud, n, np.random.default_rng(5))
        path = str(tmp_path / ("case%d.bin" % k))
        _write_case(path, cloud, cap, pos, u)
        out = subprocess.run([exe, path], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr[-3000:]
        if k < 2:
            assert "bad 0" in out.stdout and ("rays %d" % n) in out.stdout, out.stdout
        else:
            assert "bricks refused" in out.stdout, out.stdout
