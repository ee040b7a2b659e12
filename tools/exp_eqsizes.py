#!/usr/bin/env python3
"""The equilibrium grain sizes of one dust on one GPU: the resident solve (soc_a2e_set_eq_sizes + soc_a2e_resident_solve_eq: all sizes
in one sweep over the resident cells) against the route of an engine without it -- soc_amd.a2e.run with a host multiply, an upload,
soc_a2e_eqtemp, a download and a host += per size and batch of 65536 cells.

    python tools/exp_eqsizes.py [--cells 12000 770000 49500000] [--sizes 4 12] [--nfreq 50] [--reps 3] [--host-cells 4194304]
                                [--out profiles/eqsizes_lines.json]

The solver is synthetic (synth.synth_solver, every size an equilibrium size: NSTOCH 0), the absorptions a log-normal block repeated
(their values do not change the work).  Per cell count and number of sizes:

    fused     one a2e_resident_solve_eq over all cells with all sizes set, between device events (soc_timer_*), after a warm-up
    per size  the same kernel with one size set at a time, one launch per size; the launches alone between device events, summed
    host      a2e.run on an engine wrapper without the resident calls, host clock, the E -> T tables already built (the build is
              timed apart: before the tables were kept, every call paid it).  It needs three host arrays of cells x NFREQ floats and
              9e3 round trips at 4.95e7 cells, so above --host-cells cells it is timed on that many cells -- its batches are
              independent, its time is linear in the cells -- and the line says so (host_cells) and scales the figure

Medians of --reps with the spread (max - min); the fused kernel's share of the copy ceiling from 12 * NFREQ bytes per cell (the
absorptions in, the sum in and out) at 6.29 TB/s.  At the smallest cell count the fused result is compared with the host route's bit
for bit.  One JSON line per case is appended to --out, with the commit (`git rev-parse`, else the environment variable SOC_COMMIT)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soc_amd import a2e, synth                      # noqa: E402
from soc_amd.lib import Engine                      # noqa: E402

COPY_CEILING = 6.29e12                              # bytes per second: the project's measured copy figure of the MI355X
BLOCK = 1 << 16


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


class Batches:
    """an engine without the resident calls: a2e.run then takes every equilibrium size through a2e_eqtemp in batches"""

    def __init__(self, engine):
        self.engine = engine

    def __getattr__(self, name):
        if name.startswith("a2e_resident"):
            raise AttributeError(name)
        return getattr(self.engine, name)


def spread(v):
    return float(max(v) - min(v))


def one_case(eng, cells, ns, nfreq, reps, host_cells, check, out):
    sol = synth.synth_solver(NFREQ=nfreq, NE=16, NSIZE=ns, seed=5)
    sizes = a2e.eq_sizes(sol, 0)
    t0 = time.time()
    tables = a2e.eq_size_tables(sol, sizes)
    table_s = time.time() - t0                                                 # (the first call for this solver builds them)
    block = (np.random.default_rng(2).lognormal(0, 1, (min(cells, BLOCK), nfreq)) * 1e-3).astype(np.float32)
    block[:, -1] = np.clip(block[:, -1], 0.0, 0.2 * block[:, -2])              # as a2e.run clips
    fused_ms, each_ms = [], []
    eng.a2e_resident_begin(cells, nfreq)
    try:
        for i in range(0, cells, BLOCK):
            eng.a2e_resident_upload(i, block[:min(BLOCK, cells - i)])
        eng.a2e_set_eq_sizes(*tables)
        eng.a2e_resident_solve_eq()                                            # warm-up at the timed shape
        eng.sync()
        for _ in range(reps):
            eng.timer_start()
            eng.a2e_resident_solve_eq()
            fused_ms.append(eng.timer_stop())
        for rep in range(reps + 1):                                            # (the first turn warms the one-size shape up)
            total = 0.0
            for s in sizes:
                eng.a2e_set_eq_sizes(*a2e.eq_size_tables(sol, [s]))
                eng.timer_start()
                eng.a2e_resident_solve_eq()
                total += eng.timer_stop()
            if rep:
                each_ms.append(total)
    finally:
        eng.a2e_resident_end()
    nh = min(cells, host_cells)
    ABS = np.tile(block, ((nh + BLOCK - 1) // BLOCK, 1))[:nh]
    host_s, same = [], None
    a2e.run(Batches(eng), sol, ABS[:min(nh, BLOCK)], NSTOCH=0, verbose=False)  # warm-up
    for _ in range(reps):
        t0 = time.time()
        EH, _ = a2e.run(Batches(eng), sol, ABS, NSTOCH=0, verbose=False)
        host_s.append(time.time() - t0)
    if check:
        ER, _ = a2e.run(eng, sol, ABS, NSTOCH=0, verbose=False)
        same = bool(np.array_equal(ER.view(np.uint32), EH.view(np.uint32)))
    del ABS, EH
    fused = float(np.median(fused_ms)) * 1e-3
    scale = cells / float(nh)
    line = {"what": "equilibrium sizes of one dust: resident solve (all sizes in one sweep) against a2e.run with a2e_eqtemp per size and batch",
            "commit": commit(), "cells": cells, "NFREQ": nfreq, "eq_sizes": len(sizes),
            "fused_ms": fused_ms, "fused_median_ms": float(np.median(fused_ms)), "fused_spread_ms": spread(fused_ms),
            "per_size_launches_ms": each_ms, "per_size_launches_median_ms": float(np.median(each_ms)), "per_size_launches_spread_ms": spread(each_ms),
            "fused_bytes_per_cell": 12 * nfreq, "fused_TBps": 12.0 * nfreq * cells / fused * 1e-12,
            "fused_share_of_copy_ceiling": 12.0 * nfreq * cells / fused / COPY_CEILING,
            "fused_cell_sizes_per_s": cells * len(sizes) / fused,
            "host_cells": nh, "host_s": host_s, "host_median_s": float(np.median(host_s)), "host_spread_s": spread(host_s),
            "host_scaled_to_cells_s": float(np.median(host_s)) * scale, "host_over_fused": float(np.median(host_s)) * scale / fused,
            "eq_tables_build_s": table_s, "bit_identical_to_host_route": same}
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as fp:
            fp.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[12000, 770000, 49500000])
    ap.add_argument("--sizes", type=int, nargs="+", default=[4, 12])
    ap.add_argument("--nfreq", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-cells", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = Engine(0)
    try:
        for cells in a.cells:
            for ns in a.sizes:
                one_case(eng, cells, ns, a.nfreq, a.reps, a.host_cells, cells == min(a.cells), a.out)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
