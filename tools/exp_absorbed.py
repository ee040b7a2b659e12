#!/usr/bin/env python3
"""The absorption hand-over of one dust re-emission iteration on one GPU: from the INT tallies the launches leave on the device, one
per frequency, to the rows ABS[cells][NFREQ] of the multi-dust stage, scaled as the absorbed file holds them -- the host source
against the resident one (soc_amd.driver takes the second where it can).

    python tools/exp_absorbed.py [--roots 16 64 256] [--nfreq 50] [--reps 3] [--out profiles/absorbed_lines.json]

The geometry is that of config 3, synth.octree_cloud(root, levels=4, frac=0.10, seed=1234): root 256 is config 3 itself (4.95e7
cells), the smaller roots show where the hand-over is all overhead.  The tally is synthetic (its values do not change the work).

    host      the statements of soc_amd.driver's host source: CONSTANT.copy(), per frequency read_tally (CELLS floats down,
              synchronised) and the strided add FABSORBED[:, f] += TMP, files.scale_absorbed over the whole array, then the
              mabu_upload loop into the open mabu_begin
    resident  absorbed_restore (device to device), per frequency absorbed_add_tally (one kernel over a contiguous row), then
              absorbed_to_mabu (one tiled transpose that scales on the way); a synchronise at the end

Both are timed with the host clock around work that ends in a device synchronise, alternating, after a warm-up of every call at the
timed shape; the resident source's three pieces also between device events (soc_timer_*).  The scaled rows of the last 2^18 cells are
compared bit for bit.  One JSON line per size is appended to --out, with the commit (`git rev-parse`, else the environment variable
SOC_COMMIT)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soc_amd import files, synth                    # noqa: E402
from soc_amd.lib import Engine                      # noqa: E402
from soc_amd.mabu import CHUNK                      # noqa: E402

GL, NNNLIMIT, INT = 0.05, 0.0, 1


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


def host_source(eng, cloud, CONSTANT, freqs):
    """the hand-over through the host: every tally comes down, the scaled array goes up"""
    cells = cloud.CELLS
    FABSORBED = CONSTANT.copy()
    for f in freqs:
        TMP = eng.read_tally(INT)                   # (synchronises)
        FABSORBED[:, f] += TMP
    files.scale_absorbed(FABSORBED, cloud, GL, NNNLIMIT)
    for i in range(0, cells, CHUNK):
        eng.mabu_upload(i, FABSORBED[i:min(i + CHUNK, cells)])
    eng.sync()
    return FABSORBED


def resident_source(eng, K, freqs, events=None):
    def timed(name, call):
        if events is None:
            return call()
        eng.timer_start()
        call()
        events[name].append(eng.timer_stop())
    timed("restore_ms", eng.absorbed_restore)
    timed("adds_ms", lambda: [eng.absorbed_add_tally(f) for f in freqs])
    timed("to_mabu_ms", lambda: eng.absorbed_to_mabu(0, K, NNNLIMIT))
    eng.sync()


def one_size(eng, root, nfreq, reps, out):
    cloud = synth.octree_cloud(root, levels=4, frac=0.10, seed=1234)
    cells = cloud.CELLS
    K = files.absorbed_scale_factors(cloud, GL)
    freqs = list(range(nfreq))
    eng.set_cloud(cloud)
    eng.set_features(1, 0, 0)
    rng = np.random.default_rng(2)
    eng.write_tally(INT, np.resize((rng.lognormal(0, 1, 1 << 16) * 1e-3).astype(np.float32), cells))
    CONSTANT = np.resize((rng.lognormal(0, 1, (1 << 16, nfreq)) * 1e-2).astype(np.float32), (cells, nfreq))
    eng.absorbed_begin(nfreq, keep_constant=True)
    eng.mabu_begin(cells, nfreq, 1)
    try:
        # the constant sources' share on the device: the same values, through the tally, column by column
        TALLY = eng.read_tally(INT)
        for f in freqs:
            eng.write_tally(INT, CONSTANT[:, f])
            eng.absorbed_add_tally(f)
        eng.absorbed_keep()
        eng.write_tally(INT, TALLY)
        host_source(eng, cloud, CONSTANT, freqs[-2:])                          # warm-up of every call at the timed shape
        resident_source(eng, K, freqs[-2:])
        host_s, res_s, events = [], [], dict(restore_ms=[], adds_ms=[], to_mabu_ms=[])
        for _ in range(reps):                                                  # alternating
            t0 = time.time()
            want = host_source(eng, cloud, CONSTANT, freqs)
            host_s.append(time.time() - t0)
            t0 = time.time()
            resident_source(eng, K, freqs, events)
            res_s.append(time.time() - t0)
        tail = min(cells, 1 << 18)
        got = eng.absorbed_download(cells - tail, tail, K, NNNLIMIT)
    finally:
        eng.mabu_end()
        eng.absorbed_end()
    n = cells * nfreq
    med = {k: float(np.median(v)) * 1e-3 for k, v in events.items()}
    line = {"what": "absorption hand-over of one iteration: NFREQ INT tallies on the device -> scaled ABS[cells][NFREQ] of the multi-dust stage",
            "commit": commit(), "root": root, "levels": 4, "cells": cells, "NFREQ": nfreq,
            "host_s": host_s, "resident_s": res_s, "host_median_s": float(np.median(host_s)), "resident_median_s": float(np.median(res_s)),
            "host_spread_s": float(max(host_s) - min(host_s)), "resident_spread_s": float(max(res_s) - min(res_s)),
            "ratio": float(np.median(host_s) / np.median(res_s)),
            "resident_restore_ms": events["restore_ms"], "resident_adds_ms": events["adds_ms"], "resident_to_mabu_ms": events["to_mabu_ms"],
            "restore_moved_TBps": 8.0 * n / med["restore_ms"] * 1e-12, "adds_moved_TBps": 12.0 * n / med["adds_ms"] * 1e-12,
            "to_mabu_moved_TBps": 8.0 * n / med["to_mabu_ms"] * 1e-12,
            "bit_identical_last_rows": bool(np.array_equal(got.view(np.uint32), want[cells - tail:].view(np.uint32)))}
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
    a = ap.parse_args()
    eng = Engine(0)
    try:
        for root in a.roots:
            one_size(eng, root, a.nfreq, a.reps, a.out)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
