#!/usr/bin/env python3
"""What the dust temperatures and the populations cost on one GPU.

    python tools/exp_temperatures.py [--cells 12000 770000 49500000] [--reps 3] [--out profiles/temperatures_lines.json]
    rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python tools/exp_temperatures.py --kernel-only [--reps 5]
    python tools/exp_temperatures.py --cells --trace <dir>/.../t_kernel_trace.csv --out profiles/temperatures_lines.json

pipeline  Stage 2 of the three-dust model of tools/exp_mabu_library.py (two equilibrium dusts with abundances, a stochastically heated
          one of one size, 50 frequencies) on its device path, host arrays in and out, wall clock, with and without `temperatures`,
          the two alternating after a warm-up of either.  The option adds the read-back of 4 bytes per cell and equilibrium dust (here
          two) after each dust's solve; the line gives the added time beside the time those bytes take at the nominal rate of the
          host link (PCIe 5.0 x16, 64 GB/s) -- a floor, not a measurement of the link.  At the smallest cell count the temperatures of
          the device path are compared with the host path's bit for bit.
kernel    soc_a2e_dosolve_kernel<4, false, true> (the populations written, 4*NE bytes per cell) against <4, false, false> at NE 128,
          NFREQ 50, 65536 cells: --kernel-only launches the two alternating (a2e_solve, a2e_solve_dump) after a warm-up of either, and
          is meant to run under rocprofv3 --kernel-trace; --trace FILE then reads the dispatches of the two instances from the trace
          and writes the line (medians and spread over the dispatches, the warm-up pair left out).  Without a trace no kernel time is
          reported: the calls' wall clock holds the copies.

Medians of --reps with the spread (max - min).  JSON lines are appended to --out, with the commit (`git rev-parse`, else SOC_COMMIT)."""
import argparse
import csv
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from exp_mabu_library import BLOCK, NDUST, NFREQ, Tiled, commit, dusts_of, spread   # noqa: E402
from soc_amd import mabu, synth           # noqa: E402
from soc_amd.lib import Engine            # noqa: E402

LINK = 64.0e9                             # B/s, PCIe 5.0 x16 in one direction, nominal
K_NE, K_CELLS = 128, 65536


def emit(line, out):
    line["commit"] = commit()
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as fp:
            fp.write(json.dumps(line) + "\n")


def pipeline(eng, d, cells, reps, check, out):
    dusts, kinds, FREQ = dusts_of(d)
    rng = np.random.default_rng(7)
    ABU = np.ones((cells, NDUST), np.float32)
    ABU[:, 0], ABU[:, 2] = rng.uniform(0.5, 1.5, cells), rng.uniform(0.2, 1.2, cells)
    block = rng.lognormal(0, 1, (min(cells, BLOCK), NFREQ)).astype(np.float32)
    block *= (1e-3 * (FREQ[None, :] / 1e13) ** -1.0).astype(np.float32)
    FABS = Tiled(block, 0, cells) if cells > BLOCK else block
    for t in (False, True):                                            # warm-up of either
        mabu.solve_emission(eng, dusts, kinds, block[:4096], ABU[:4096], temperatures=t)
    secs = {False: [], True: []}
    ranges = planes = None
    for _ in range(reps):
        for t in (False, True):                                        # alternating
            t0 = time.time()
            EM, info = mabu.solve_emission(eng, dusts, kinds, FABS, ABU, path='device', temperatures=t)
            secs[t].append(time.time() - t0)
            ranges = info["ranges"]
            if t:
                planes = sum(1 if isinstance(T, np.ndarray) else len(T) for T in info["T"])
            del EM, info
    same = None
    if check:
        n = min(cells, 4096)
        _, hi = mabu.solve_emission(eng, dusts, kinds, block[:n], ABU[:n], path='host', temperatures=True)
        _, di = mabu.solve_emission(eng, dusts, kinds, block[:n], ABU[:n], path='device', temperatures=True)
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(hi["T"], di["T"]) if isinstance(a, np.ndarray))
    plain, temp = float(np.median(secs[False])), float(np.median(secs[True]))
    emit({"what": "stage 2 on the device path with and without temperatures (host arrays in and out, wall clock)",
          "cells": cells, "NDUST": NDUST, "NFREQ": NFREQ, "ranges": ranges, "temperature_planes": planes,
          "plain_s": secs[False], "plain_median_s": plain, "plain_spread_s": spread(secs[False]),
          "temperatures_s": secs[True], "temperatures_median_s": temp, "temperatures_spread_s": spread(secs[True]),
          "added_s": temp - plain, "added_share": (temp - plain) / plain,
          "read_back_bytes": 4 * planes * cells, "read_back_at_nominal_link_s": 4.0 * planes * cells / LINK,
          "device_temperatures_bit_identical_to_host_path": same}, out)


def kernel_only(eng, reps):
    sol = synth.synth_solver(NFREQ=NFREQ, NE=K_NE, NSIZE=1, seed=5)
    ABS = (np.random.default_rng(1).lognormal(0, 1, (K_CELLS, NFREQ)) * 1e-3 * (np.asarray(sol["FREQ"])[None, :] / 1e13) ** -1.0).astype(np.float32)
    eng.a2e_set_size(K_NE, NFREQ, sol["sizes"][0], synth.a2e_absorption_fraction(sol, 0))
    assert eng.a2e_launch_shape()[0] == 4
    same = True
    for _ in range(reps + 1):                                          # the first pair is the warm-up
        plain = eng.a2e_solve(ABS)
        em, X = eng.a2e_solve_dump(ABS)
        same = same and bool(np.array_equal(plain.view(np.uint32), em.view(np.uint32)))
    print(json.dumps({"kernel_only": True, "pairs": reps + 1, "emission_bit_identical": same,
                      "populations_min": float(X.min()), "populations_max": float(X.max())}), flush=True)


def kernel_line(trace, out):
    """the dispatches of the two C = 4 instances in a rocprofv3 kernel trace (csv): durations in microseconds, in order"""
    dur = {False: [], True: []}
    with open(trace, newline="") as fp:
        for row in csv.DictReader(fp):
            name = row.get("Kernel_Name", "")
            m = re.search(r"soc_a2e_dosolve_kernel<4, ?false, ?(true|false)>", name) or re.search(r"soc_a2e_dosolve_kernelILi4ELb0ELb([01])E", name)
            if m:
                dur[m.group(1) in ("true", "1")].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
    if len(dur[False]) < 2 or len(dur[True]) < 2:
        raise SystemExit("%s: %d and %d dispatches of the two instances; at least two of each" % (trace, len(dur[False]), len(dur[True])))
    p, x = dur[False][1:], dur[True][1:]                               # (without the warm-up pair)
    mp, mx = float(np.median(p)), float(np.median(x))
    lds_bytes = 4 * ((K_NE * K_NE - K_NE) // 2 + K_NE + NFREQ)
    emit({"what": "soc_a2e_dosolve_kernel<4, false, true> (populations written) against <4, false, false>, rocprofv3 kernel trace",
          "NE": K_NE, "NFREQ": NFREQ, "cells": K_CELLS, "plain_us": p, "plain_median_us": mp, "plain_spread_us": spread(p),
          "dump_us": x, "dump_median_us": mx, "dump_spread_us": spread(x), "dump_over_plain": mx / mp,
          "added_us": mx - mp, "extra_bytes_written_per_cell": 4 * K_NE, "lds_bytes_per_cell": lds_bytes,
          "extra_write_rate_GBps_if_all_added_time": 4.0 * K_NE * K_CELLS / max(mx - mp, 1e-9) * 1e-3}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="*", default=[12000, 770000, 49500000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        kernel_line(a.trace, a.out)
    if a.kernel_only or a.cells:
        eng = Engine(0)
        try:
            if a.kernel_only:
                kernel_only(eng, a.reps)
            else:
                with tempfile.TemporaryDirectory() as d:
                    for cells in a.cells:
                        pipeline(eng, d, cells, a.reps, cells == min(a.cells), a.out)
        finally:
            eng.close()


if __name__ == "__main__":
    main()
