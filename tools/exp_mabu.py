#!/usr/bin/env python3
"""Stage 2 of a multi-dust run (soc_amd.mabu.solve_emission) on one GPU: the device path against the host path.

    python tools/exp_mabu.py [--log2cells 20 22 24] [--reps 3] [--out profiles/mabu_lines.json]
    python tools/exp_mabu.py --kernels 22          (the split and sum kernels alone: run this one under
                                                    rocprofv3 --kernel-trace --stats for the kernel times)

The model is synthetic: 2^k cells x 50 frequencies, an equilibrium dust with an abundance file and a stochastically
heated dust (synth.synth_solver, NE 128, one size).  The host path of this build is the stage as it was before the
device path existed (numpy split and sum around the engine's solvers), so the two times come from the same session.
One JSON line per size is appended to --out, with the commit it was taken at (`git rev-parse`; where the tree is not a
git checkout, what the environment variable SOC_COMMIT says); --kernels prints, and appends to --out, one line with the
streaming rates: the issue's figure (8 B per element + 4 B x NDUST per cell) and the bytes each kernel really moves."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soc_amd import mabu, synth           # noqa: E402
from soc_amd.lib import Engine            # noqa: E402

NFREQ, NE = 50, 128
COPY_CEILING = 6.29e12                    # B/s, float4 copy


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


def model(d, cells):
    sol = synth.synth_solver(NFREQ=NFREQ, NE=NE, NSIZE=1, seed=5)
    FREQ = np.asarray(sol["FREQ"], np.float64)
    synth.write_solver(os.path.join(d, "pah.solver"), sol)
    with open(os.path.join(d, "gs_pah.dust"), "w") as fp:
        fp.write("gsetdust\n")
    with open(os.path.join(d, "sil.dust"), "w") as fp:
        fp.write("eqdust\n 1.0e-7\n 1.0e-4\n%d\n" % NFREQ)
        for f in FREQ:
            fp.write(" %.5e  0.5  %.5e  %.5e\n" % (f, 2.0e-2 * (f / 1e14) ** 1.2, 5.0e-2 * (f / 1e14) ** 1.5))
    rng = np.random.default_rng(1)
    ABS = rng.lognormal(0, 1, (cells, NFREQ)).astype(np.float32)
    ABS *= (1e-3 * (FREQ[None, :] / 1e13) ** -1.0).astype(np.float32)
    ABU = np.ones((cells, 2), np.float32)
    ABU[:, 0] = rng.uniform(0.5, 1.5, cells)
    dusts = [os.path.join(d, "sil.dust"), os.path.join(d, "gs_pah.dust")]
    return dusts, [mabu.dust_kind(x) for x in dusts], ABS, ABU


def stage(eng, d, k, reps, out):
    cells = 1 << k
    dusts, kinds, ABS, ABU = model(d, cells)
    mabu.solve_emission(eng, dusts, kinds, ABS[:4096], ABU[:4096])             # (first-use costs of the kernels)
    dev, host, E = [], [], {}
    for it in range(reps):
        for tag, ts in (("device", dev), ("host", host)):
            t0 = time.time()
            E[tag], info = mabu.solve_emission(eng, dusts, kinds, ABS, ABU, path=tag)
            ts.append(time.time() - t0)
            assert info["path"] == tag
    line = {"what": "mabu.solve_emission, host arrays in and out", "commit": commit(), "cells": cells, "NFREQ": NFREQ, "NE": NE,
            "dusts": "eqdust with abundances + gsetdust (1 size)", "ranges": info["ranges"],
            "device_s": dev, "host_s": host, "device_median_s": float(np.median(dev)), "host_median_s": float(np.median(host)),
            "host_spread_s": float(max(host) - min(host)), "speedup": float(np.median(host) / np.median(dev)),
            "bit_identical": bool(np.array_equal(E["device"].view(np.uint32), E["host"].view(np.uint32)))}
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as fp:
            fp.write(json.dumps(line) + "\n")


def kernels(eng, d, k, reps, out):
    cells = 1 << k
    dusts, kinds, ABS, ABU = model(d, cells)
    RABS, _ = mabu.relative_cross_sections(dusts, kinds)
    eng.mabu_begin(cells, NFREQ, 2)
    try:
        eng.mabu_upload(0, ABS)
        eng.mabu_set_tables(ABU, RABS)
        ms = {"split": [], "sum": []}
        for it in range(reps + 1):
            for tag, call in (("split", lambda: eng.mabu_split(it % 2)), ("sum", lambda: eng.mabu_accumulate(it % 2))):
                eng.timer_start()
                call()
                ms[tag].append(eng.timer_stop())
    finally:
        eng.mabu_end()
    n = cells * NFREQ
    line = {"what": "soc_mabu_split (+ the zeroing of EM) and soc_mabu_accumulate between events", "commit": commit(), "cells": cells,
            "NFREQ": NFREQ, "NDUST": 2, "copy_ceiling_TBps": COPY_CEILING * 1e-12}
    for tag, moved in (("split", 8 * n + 8 * cells + 4 * n), ("sum", 12 * n + 8 * cells)):
        t = float(np.median(ms[tag][1:])) * 1e-3
        line[tag] = {"ms": ms[tag][1:], "issue_formula_TBps": (8 * n + 8 * cells) / t * 1e-12, "moved_TBps": moved / t * 1e-12}
    print(json.dumps(line), flush=True)
    if out:
        with open(out, "a") as fp:
            fp.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2cells", type=int, nargs="+", default=[20, 22, 24])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", type=int, default=None, metavar="LOG2CELLS")
    a = ap.parse_args()
    eng = Engine(0)
    try:
        with tempfile.TemporaryDirectory() as d:
            if a.kernels is not None:
                kernels(eng, d, a.kernels, a.reps, a.out)
            else:
                for k in a.log2cells:
                    stage(eng, d, k, a.reps, a.out)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
