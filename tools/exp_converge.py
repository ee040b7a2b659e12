#!/usr/bin/env python3
"""The convergence check of one dust re-emission iteration on one GPU: emitted_change (soc_emitted_change: one pass over the resident
emission ET[NFREQ][CELLS], the luminosities of the iteration before kept as one plane of doubles), timed at the sizes of
profiles/reemit_lines.json.

    python tools/exp_converge.py [--roots 16 64 256] [--nfreq 50] [--reps 3] [--out profiles/converge_lines.json]

The geometry is that of config 3, synth.octree_cloud(root, levels=4, frac=0.10, seed=1234): root 256 is config 3 itself (4.95e7
cells).  The emission is synthetic (its values do not change the work) and uploaded once; a second one, a few per cent off, alternates
with it so that every timed call finds a plane that differs from its result.

Every call is timed twice: with the host clock around the whole call (it uploads W, launches the two kernels, reads 40 bytes back and
synchronises: what an iteration of soc_amd.driver pays), and between device events around the same call (soc_timer_*).  Medians of
--reps with their spread, after a warm-up call at the timed shape.  Reported against two yardsticks: the hand-over of one iteration at
the same size as profiles/reemit_lines.json and profiles/absorbed_lines.json have it (10.7 ms + 14.2 ms at config 3), passed in with
--handover-ms where known, and the bytes the pass moves, (4 NFREQ + 16) CELLS, over the copy ceiling of VERDICT.md (6.29 TB/s).  One
JSON line per size is appended to --out, with the commit (`git rev-parse`, else the environment variable SOC_COMMIT)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soc_amd import converge, launch, synth         # noqa: E402
from soc_amd.launch import FACTOR, PARSEC           # noqa: E402
from soc_amd.lib import Engine                      # noqa: E402

GL = 0.05
COPY_CEILING_TBPS = 6.29                            # the device-to-device copy ceiling of an MI355X


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


def upload(eng, cells, block, scale):
    for i in range(0, cells, block.shape[0]):
        part = block[:min(block.shape[0], cells - i)]
        eng.emitted_upload(i, part if scale is None else (part * scale[:part.shape[0]]).astype(np.float32))


def one_size(eng, root, nfreq, reps, out, handover_ms):
    cloud = synth.octree_cloud(root, levels=4, frac=0.10, seed=1234)
    cells = cloud.CELLS
    COEFF = np.asarray([GL * PARSEC / (8.0 ** level) / FACTOR for level in range(cloud.LEVELS)], np.float32)
    FFREQ = np.logspace(11.5, 15.0, nfreq).astype(np.float32)
    W = np.asarray([launch.trapezoid_weight(FFREQ, f) for f in range(nfreq)], np.float64)
    rng = np.random.default_rng(2)
    block = (rng.lognormal(0, 1, (min(cells, 1 << 16), nfreq)) * 1e-28).astype(np.float32)
    off = rng.uniform(0.95, 1.05, (block.shape[0], 1)).astype(np.float32)
    eng.set_cloud(cloud)
    eng.emitted_begin(nfreq)
    try:
        upload(eng, cells, block, None)
        eng.emitted_change(W, COEFF)                                           # reserves the plane; warm-up at the timed shape
        # parity at this size on a sample: cells of the root grid (links among them) against the host statement
        n = min(block.shape[0], int(cloud.LCELLS[0]))
        want, _ = converge.luminosity(block[:n], W, cloud.DENS[:n], [0], [n], COEFF[:1])
        same = bool(np.array_equal(eng.emitted_read_luminosity(0, n).view(np.uint64), want.view(np.uint64)))
        host_s, dev_ms, figs = [], [], []
        for r in range(reps):
            upload(eng, cells, block, off if r % 2 == 0 else None)             # (the plane now differs from what the call will find)
            eng.sync()
            t0 = time.time()
            eng.timer_start()
            st = eng.emitted_change(W, COEFF)
            dev_ms.append(eng.timer_stop())
            host_s.append(time.time() - t0)
            figs.append(converge.figures(st)["d_l1"])
    finally:
        eng.emitted_end()
    moved = (4.0 * nfreq + 16.0) * cells
    dev = float(np.median(dev_ms)) * 1e-3
    line = {"what": "convergence check of one iteration: one pass over ET[NFREQ][CELLS] on the device -> 4 statistics",
            "commit": commit(), "root": root, "levels": 4, "cells": cells, "NFREQ": nfreq,
            "host_s": host_s, "host_median_s": float(np.median(host_s)), "host_spread_s": float(max(host_s) - min(host_s)),
            "device_ms": dev_ms, "device_median_ms": dev * 1e3, "device_spread_ms": float(max(dev_ms) - min(dev_ms)),
            "bytes_moved": moved, "moved_TBps": moved / dev * 1e-12, "fraction_of_copy_ceiling": moved / dev * 1e-12 / COPY_CEILING_TBPS,
            "ceiling_ms": moved / (COPY_CEILING_TBPS * 1e12) * 1e3,
            "handover_ms_of_the_parent": handover_ms, "share_of_the_handover": None if handover_ms is None else dev * 1e3 / handover_ms,
            "d_l1": figs, "luminosity_bit_identical_sample": same}
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as fp:
            fp.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--roots", type=int, nargs="+", default=[256])
    ap.add_argument("--nfreq", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--handover-ms", type=float, nargs="+", default=None, help="per root: emission + absorption hand-over of the parent commit [ms]")
    a = ap.parse_args()
    eng = Engine(0)
    try:
        for i, root in enumerate(a.roots):
            one_size(eng, root, a.nfreq, a.reps, a.out, a.handover_ms[i] if a.handover_ms and i < len(a.handover_ms) else None)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
