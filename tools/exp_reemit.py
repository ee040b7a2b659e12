#!/usr/bin/env python3
"""The emission hand-over of one dust re-emission iteration on one GPU: from the sum the multi-dust stage leaves on the device
(SUM[cells][NFREQ]) to the NFREQ arrays EMIT[CELLS] that the cell-emission launches of the next iteration read -- the host source
against the resident one (soc_amd.driver takes the second where it can).

    python tools/exp_reemit.py [--roots 16 64 256] [--nfreq 50] [--reps 3] [--out profiles/reemit_lines.json]

The geometry is that of config 3, synth.octree_cloud(root, levels=4, frac=0.10, seed=1234): root 256 is config 3 itself (4.95e7
cells), the smaller roots show where the hand-over is all overhead.  The emission is synthetic (its values do not change the work).

    host      mabu_download of SUM (device to host), then per frequency the statements of AbsorptionRun -- the strided gather
              EMITTED[:, f], the scaling pass per level, the mask of empty cells -- and set_emission (CELLS floats up, synchronised)
    resident  emitted_from_mabu (one tiled transpose, device to device), then per frequency set_emission_column (one kernel over a
              contiguous row); a synchronise at the end

Both are timed with the host clock around work that ends in a device synchronise, alternating, after a warm-up of every call at the
timed shape; the resident source's two pieces also between device events (soc_timer_*).  The EMIT of the last frequency is compared
bit for bit.  One JSON line per size is appended to --out, with the commit (`git rev-parse`, else the environment variable SOC_COMMIT)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soc_amd import synth                           # noqa: E402
from soc_amd.launch import FACTOR, PARSEC           # noqa: E402
from soc_amd.lib import Engine                      # noqa: E402
from soc_amd.mabu import CHUNK                      # noqa: E402

GL = 0.05


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


def host_source(eng, cloud, EM, COEFF, freqs):
    """today's hand-over: SUM comes down, every frequency goes up"""
    cells = cloud.CELLS
    for i in range(0, cells, CHUNK):
        m = min(i + CHUNK, cells) - i
        eng.mabu_download(i, m, out=EM[i:i + m])
    EMIT = np.zeros(cells, np.float32)
    for f in freqs:
        EMIT[:] = EM[:, f]
        for level in range(cloud.LEVELS):
            a, b = int(cloud.OFF[level]), int(cloud.OFF[level] + cloud.LCELLS[level])
            EMIT[a:b] *= COEFF[level] * cloud.DENS[a:b]
        EMIT[cloud.DENS < 1.0e-10] = 0.0
        eng.set_emission(EMIT)                      # (synchronises)
    return EMIT


def resident_source(eng, COEFF32, freqs, events=None):
    if events is not None:
        eng.timer_start()
    eng.emitted_from_mabu(0)
    if events is not None:
        events["transpose_ms"].append(eng.timer_stop())
        eng.timer_start()
    for f in freqs:
        eng.set_emission_column(f, COEFF32)
    if events is not None:
        events["columns_ms"].append(eng.timer_stop())
    eng.sync()


def one_size(eng, root, nfreq, reps, out):
    cloud = synth.octree_cloud(root, levels=4, frac=0.10, seed=1234)
    cells = cloud.CELLS
    COEFF = [GL * PARSEC / (8.0 ** level) / FACTOR for level in range(cloud.LEVELS)]
    COEFF32 = np.asarray(COEFF, np.float32)
    freqs = list(range(nfreq))
    eng.set_cloud(cloud)
    # SUM on the device: an equilibrium dust's emission of synthetic absorptions, abundance 1 (the work does not depend on the values)
    rng = np.random.default_rng(2)
    block = (rng.lognormal(0, 1, (min(cells, 1 << 16), nfreq)) * 1e-3).astype(np.float32)
    FREQ = np.logspace(11.5, 15.0, nfreq).astype(np.float32)
    KABS = (1.0e-22 * (FREQ / 1.0e13) ** 1.5).astype(np.float32)
    TTT = np.linspace(3.0, 1500.0, 200).astype(np.float32)
    eng.emitted_begin(nfreq)
    eng.mabu_begin(cells, nfreq, 1)
    try:
        for i in range(0, cells, block.shape[0]):
            eng.mabu_upload(i, block[:min(block.shape[0], cells - i)])
        eng.mabu_set_tables(np.ones((cells, 1), np.float32), np.ones((nfreq, 1)))
        eng.mabu_split(0)
        eng.mabu_solve_eq(TTT.size, 1.0e20, 1.05, 1.0 / np.log10(1.05), 1.0e-12, FREQ, KABS, TTT)
        eng.mabu_accumulate(0)
        EM = np.zeros((cells, nfreq), np.float32)
        host_source(eng, cloud, EM, COEFF, freqs[-2:])                         # warm-up of every call at the timed shape
        resident_source(eng, COEFF32, freqs[-2:])
        host_s, res_s, events = [], [], dict(transpose_ms=[], columns_ms=[])
        for _ in range(reps):                                                  # alternating
            t0 = time.time()
            want = host_source(eng, cloud, EM, COEFF, freqs)
            host_s.append(time.time() - t0)
            t0 = time.time()
            resident_source(eng, COEFF32, freqs, events)
            res_s.append(time.time() - t0)
        got = eng.read_emission()
    finally:
        eng.mabu_end()
        eng.emitted_end()
    n = cells * nfreq
    tr, co = float(np.median(events["transpose_ms"])) * 1e-3, float(np.median(events["columns_ms"])) * 1e-3
    line = {"what": "emission hand-over of one iteration: SUM[cells][NFREQ] on the device -> NFREQ EMIT[CELLS] arrays on the device",
            "commit": commit(), "root": root, "levels": 4, "cells": cells, "NFREQ": nfreq,
            "host_s": host_s, "resident_s": res_s, "host_median_s": float(np.median(host_s)), "resident_median_s": float(np.median(res_s)),
            "host_spread_s": float(max(host_s) - min(host_s)), "resident_spread_s": float(max(res_s) - min(res_s)),
            "ratio": float(np.median(host_s) / np.median(res_s)),
            "resident_transpose_ms": events["transpose_ms"], "resident_columns_ms": events["columns_ms"],
            "transpose_moved_TBps": 8.0 * n / tr * 1e-12, "columns_moved_TBps": 12.0 * n / co * 1e-12,
            "bit_identical_last_frequency": bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))}
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
