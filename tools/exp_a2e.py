#!/usr/bin/env python3
"""Throughput of the A2E DoSolve kernel (config 5): batch resident on the device, kernel alone and with PCIe copies.

    python tools/exp_a2e.py [--ne 128] [--nfreq 50] [--batch 8192] [--reps 5] [--aalg FRACTION | --aalg-partial]

Prints one JSON line: cell-sizes/s, and the roofline numbers of SURVEY.md 8(d): algorithmic HBM bytes = 8*NFREQ per
cell and size (absorptions in, emission out; weights and tables are shared by all cells and stay in cache).

--aalg FRACTION adds the polarised output (the second, weighted accumulator of the kernel's epilogue): that fraction of the cells
aligned for every size, the rest for none; --aalg-partial puts every cell into the partial-weight arm.  The kernel is then timed
on the resident path (soc_a2e_resident_solve, which is where the accumulator lives: it reads and adds to the sums, 16*NFREQ bytes per
cell and size without and at most 24*NFREQ with the polarised sum); "resident_kernel_ms" is printed without the option as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soc_amd import synth                 # noqa: E402
from soc_amd.lib import Engine            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ne", type=int, default=128)
    ap.add_argument("--nfreq", type=int, default=50)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--program", type=int, nargs=2, metavar=("CELLS", "NSIZE"), default=None,
                    help="also time soc_amd.a2e.run end to end (host arrays in, host array out) for CELLS cells and NSIZE sizes: with the cells resident on the device, and in batches as the reference does")
    ap.add_argument("--aalg", type=float, default=None, metavar="FRACTION", help="polarised output: this fraction of the cells aligned for every size, the rest for none")
    ap.add_argument("--aalg-partial", action="store_true", help="polarised output with every cell in the partial-weight arm")
    a = ap.parse_args()
    pol = a.aalg is not None or a.aalg_partial
    prof = None
    if os.environ.get("SOC_HIP_LIB"):                     # a -DSOC_A2E_PROF build (tools/build_prof.sh): cycles per phase
        import ctypes as C
        from soc_amd import lib as soclib
        L = soclib.load_library(os.environ["SOC_HIP_LIB"])
        if hasattr(L, "soc_a2e_prof_read"):
            prof = L.soc_a2e_prof_read
    eng = Engine(0)
    sol = synth.synth_solver(NFREQ=a.nfreq, NE=a.ne, NSIZE=1, seed=5)
    rng = np.random.default_rng(1)

    def aalg_for(ASIZE, cells):
        """the minimum aligned sizes of the mode: 0 (aligned for every size) or above the largest size (for none); or, for
        --aalg-partial, between the first two sizes"""
        if a.aalg_partial:
            return np.full(cells, np.sqrt(float(ASIZE[0]) * float(ASIZE[1])), np.float32)
        x = np.full(cells, 2.0 * float(np.max(ASIZE)), np.float32)
        x[rng.permutation(cells)[:int(round(a.aalg * cells))]] = 0.0
        return x

    ABS = (rng.lognormal(0, 1, (a.batch, a.nfreq)) * 1e-3 * (sol['FREQ'][None, :] / 1e13) ** -1.0).astype(np.float32)
    AF = synth.a2e_absorption_fraction(sol, 0)
    eng.a2e_set_size(a.ne, a.nfreq, sol['sizes'][0], AF)
    eng.a2e_upload(ABS)
    ms = []
    for it in range(a.reps):
        eng.timer_start()
        eng.a2e_run(a.batch)
        ms.append(eng.timer_stop())
    if prof:
        buf = (C.c_ulonglong * 8)()
        prof(buf, 1)
        eng.a2e_run(a.batch)
        eng.sync()
        prof(buf, 0)
        p = list(buf)
        tot = max(sum(p[:5]), 1)
        print("cycles of wave 0 per workgroup phase: heating %.1f %%, suffix sums %.1f %%, substitution %.1f %%, normalisation %.1f %%, emission %.1f %%"
              % tuple(100.0 * x / tot for x in p[:5]), file=sys.stderr)
    # the resident path (the sums stay on the device; with --aalg / --aalg-partial the polarised sum as well)
    two = synth.synth_solver(NFREQ=a.nfreq, NE=a.ne, NSIZE=2, seed=5)["SIZE_A"]        # (a second size for the partial arm's upper end)
    eng.a2e_resident_begin(a.batch, a.nfreq, polarised=pol)
    eng.a2e_resident_upload(0, ABS)
    if pol:
        eng.a2e_resident_upload_aalg(0, aalg_for(two, a.batch))
        eng.a2e_set_size_aalg(two, 0)
    rms = []
    for it in range(a.reps + 1):
        eng.timer_start()
        eng.a2e_resident_solve()
        rms.append(eng.timer_stop())
    eng.a2e_resident_end()
    eng.a2e_set_size(a.ne, a.nfreq, sol['sizes'][0], AF)
    t0 = time.time()
    out = eng.a2e_solve(ABS)
    t1 = time.time()
    k = float(np.median(ms))
    alg = 8.0 * a.nfreq * a.batch
    print(json.dumps({"kernel": "soc_a2e_dosolve_kernel", "NE": a.ne, "NFREQ": a.nfreq, "batch": a.batch, "kernel_ms": k,
                      "aalg": "partial" if a.aalg_partial else a.aalg, "resident_kernel_ms": float(np.median(rms[1:])),
                      "resident_cell_sizes_per_s": a.batch / float(np.median(rms[1:])) * 1e3,
                      "cell_sizes_per_s": a.batch / k * 1e3, "with_pcie_cell_sizes_per_s": a.batch / (t1 - t0),
                      "roofline": {"bound": "hbm", "algorithmic_bytes_per_launch": alg, "achieved": alg / k * 1e-6, "peak": 8000.0,
                                   "unit": "GB/s", "frac": alg / k * 1e-6 / 8000.0},
                      "note": "LDS/latency-bound: the transition matrix (NE^2/2 floats per cell) never leaves LDS",
                      "finite": bool(np.isfinite(out).all())}))
    if a.program:
        from soc_amd import a2e
        cells, nsize = a.program
        sol = synth.synth_solver(NFREQ=a.nfreq, NE=a.ne, NSIZE=nsize, seed=5)
        ABS = (rng.lognormal(0, 1, (cells, a.nfreq)) * 1e-3 * (sol['FREQ'][None, :] / 1e13) ** -1.0).astype(np.float32)
        kw = dict(aalg=aalg_for(sol["SIZE_A"], cells)) if pol else {}

        class Batches:
            def __getattr__(self, name):
                if name.startswith("a2e_resident"):
                    raise AttributeError(name)
                return getattr(eng, name)
        res = {}
        for tag, e in (("resident", eng), ("batches", Batches())):
            t0 = time.time()
            E = a2e.run(e, sol, ABS, verbose=False, **kw)[:-1]
            res[tag] = (time.time() - t0, E)
        same = all(bool(np.array_equal(x.view(np.uint32), y.view(np.uint32))) for x, y in zip(res["resident"][1], res["batches"][1]))
        print(json.dumps({"program": "soc_amd.a2e.run, host arrays in and out", "NE": a.ne, "NFREQ": a.nfreq, "cells": cells, "sizes": nsize,
                          "aalg": "partial" if a.aalg_partial else a.aalg,
                          "resident_s": res["resident"][0], "resident_cell_sizes_per_s": cells * nsize / res["resident"][0],
                          "batches_s": res["batches"][0], "batches_cell_sizes_per_s": cells * nsize / res["batches"][0],
                          "bit_identical": same}))
    eng.close()


if __name__ == "__main__":
    main()
