"""Runs tests/csrc/lbricks_fill_host.cpp, the stand-alone program around soc_amd/csrc/soc_lbricks.h (tests/test_lbricks_fill.py):
writes a hierarchy and rays to a file, starts the program, reads back the bricks and the steps of every ray."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BEST, TILES = 0, 1                      # soc_lbricks.h: SOC_LB_BEST, SOC_LB_TILES


def program(sanitize=True):
    out = os.path.join(REPO, "oracle", "_build", "lbricks_fill_host%s" % ("_san" if sanitize else ""))
    src = os.path.join(HERE, "csrc", "lbricks_fill_host.cpp")
    deps = [src, os.path.join(HERE, "ltree_host.cpp")] + [os.path.join(REPO, "soc_amd", "csrc", f)
                                                          for f in ("soc_ltree.h", "soc_lbricks.h", "soc_octbricks.h", "soc_math.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        cmd = ["g++", "-O1" if sanitize else "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-mfma", "-w", "-o", out + ".tmp%d" % os.getpid(), src]
        if sanitize:
            cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        subprocess.check_call(cmd)
        os.replace(cmd[cmd.index("-o") + 1], out)
    return out


class Bricks:
    """ok; boxes [bricks, 7] (x0, y0, z0, bx, by, bz, cells); rbrick [NZ, NY, NX]; max_slots, slots, check (lt_check's result);
    area_tiles, area_slabs, n_tiles, n_slabs, slabs (the bricks are the slab partition's); rays: list of (level, cell, ds, end, status)"""

    def area(self):
        b = self.boxes.astype(np.int64)
        return int(2 * (b[:, 3] * b[:, 4] + b[:, 4] * b[:, 5] + b[:, 5] * b[:, 3]).sum())


def run(cloud, cap, partition, pos=None, u=None, maxsteps=20000, boxes_only=False, sanitize=True):
    pos = np.zeros((0, 3), np.float32) if pos is None else np.ascontiguousarray(pos, np.float32)
    u = np.zeros((0, 3), np.float32) if u is None else np.ascontiguousarray(u, np.float32)
    head = np.asarray([cloud.NX, cloud.NY, cloud.NZ, cloud.LEVELS, cap, partition, len(pos), maxsteps, int(boxes_only), cloud.CELLS], np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        with open(fin, "wb") as f:
            for a in (head, np.asarray(cloud.LCELLS, np.int32), np.asarray(cloud.OFF, np.int32), np.asarray(cloud.DENS, np.float32), pos, u):
                np.ascontiguousarray(a).tofile(f)
        r = subprocess.run([program(sanitize), fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, "lbricks_fill_host: exit %d\n%s" % (r.returncode, r.stderr[-3000:])
        raw = np.fromfile(fout, np.uint8)
    B = Bricks()
    at = [0]

    def take(dtype, n):
        nb = np.dtype(dtype).itemsize * n
        a = raw[at[0]:at[0] + nb].view(dtype)
        assert len(a) == n, "output file too short"
        at[0] += nb
        return a
    ok, nb, B.max_slots, B.check, slabs, B.n_tiles, B.n_slabs, _ = (int(v) for v in take(np.int32, 8))
    B.ok, B.slabs = bool(ok), bool(slabs)
    B.slots = int(take(np.int64, 1)[0])
    B.area_tiles, B.area_slabs = (float(v) for v in take(np.float64, 2))
    B.boxes = take(np.int32, 7 * nb).reshape(nb, 7).copy()
    B.rbrick, B.rays = None, []
    if B.ok and not boxes_only:
        B.rbrick = take(np.int32, cloud.NX * cloud.NY * cloud.NZ).reshape(cloud.NZ, cloud.NY, cloud.NX).copy()
        for _ in range(len(pos)):
            n, st = (int(v) for v in take(np.int32, 2))
            end = take(np.float32, 3).copy()
            B.rays.append((take(np.int32, n).copy(), take(np.int32, n).copy(), take(np.float32, n).copy(), end, st))
    assert at[0] == len(raw), "output file too long"
    return B
