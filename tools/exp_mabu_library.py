#!/usr/bin/env python3
"""The library method for several dust components on one GPU: the fused look-up (soc_mabu_library_kernel) against the direct
device stage 2 and against the host composition.

    python tools/exp_mabu_library.py [--cells 12000 770000 49500000] [--nout 50 5] [--bins 30] [--reps 3] [--host-cells 4194304]
                                     [--out profiles/mabu_library_lines.json]

The model is synthetic: three dusts on 50 frequencies (two equilibrium dusts with abundances, a stochastically heated one:
synth.synth_solver, NE 128, one size, as tools/exp_mabu.py), a library of N^3 bins per dust with its own grid and a tenth of the
bins empty, and cells whose shares fall anywhere on the grid of one of the dusts in turn, independently from cell to cell: the
gathers of neighbouring cells go to unrelated rows of the tables (a model's neighbouring cells share bins; this is the worse case).
Per cell count:

    fused    soc_mabu_library_solve between device events (soc_timer_*), after a warm-up, at every --nout (nout < 50: the first
             columns, selected at upload as `libmaps` / ofreq.dat do).  Bytes: 4 nout written, 12 + 4 NDUST read per cell; their rate
             as a share of the copy ceiling (6.29 TB/s)
    lookup   mabu.solve_emission_library on its device path, host arrays in and out, wall clock: the uploads and the read-back of
             [cells, nout] floats included
    direct   mabu.solve_emission on its device path on the same number of cells with all 50 frequencies, host arrays in and out, wall
             clock: what a run without libraries pays for stage 2
    host     mabu.solve_emission_library with path='host': per dust a numpy split, engine.library_solve and a numpy multiply-add.
             Above --host-cells cells it is timed on that many (its chunks are independent, its time linear in the cells); the
             line says so and scales the figure

Medians of --reps with the spread (max - min).  At the smallest cell count the device and the host path are compared bit for bit.  One
JSON line per cell count and nout is appended to --out, with the commit (`git rev-parse`, else the environment variable SOC_COMMIT)."""
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

NFREQ, NE, NDUST = 50, 128, 3
REF = (10, 25, 40)                        # the reference columns
COPY_CEILING = 6.29e12                    # B/s, float4 copy
BLOCK = 1 << 16


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


def spread(v):
    return float(max(v) - min(v))


class Tiled:
    """[cells, NFREQ] absorptions that repeat a block: rows on demand, so that 4.95e7 x 50 floats need not exist on the host"""

    def __init__(self, block, start, stop):
        self.block, self.start, self.stop = block, start, stop
        self.shape = (stop - start, block.shape[1])

    def __getitem__(self, key):
        a, b, _ = key.indices(self.shape[0])
        if b - a > mabu.CHUNK:
            return Tiled(self.block, self.start + a, self.start + b)
        return np.take(self.block, (self.start + np.arange(a, b)) % len(self.block), axis=0)


def dusts_of(d):
    sol = synth.synth_solver(NFREQ=NFREQ, NE=NE, NSIZE=1, seed=5)
    FREQ = np.asarray(sol["FREQ"], np.float64)
    synth.write_solver(os.path.join(d, "pah.solver"), sol)
    with open(os.path.join(d, "gs_pah.dust"), "w") as fp:
        fp.write("gsetdust\n")
    for name, slope in (("sil", 1.2), ("carb", 0.9)):
        with open(os.path.join(d, name + ".dust"), "w") as fp:
            fp.write("eqdust\n 1.0e-7\n 1.0e-4\n%d\n" % NFREQ)
            for f in FREQ:
                fp.write(" %.5e  0.5  %.5e  %.5e\n" % (f, 2.0e-2 * (f / 1e14) ** slope, 5.0e-2 * (f / 1e14) ** 1.5))
    dusts = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    return dusts, [mabu.dust_kind(x) for x in dusts], FREQ


def library(rng, N):
    """a grid with its own origin and width per i and per (i, j), representatives within half a bin of the centres, positive rows, a
    tenth of the bins empty"""
    idx = np.indices((N, N, N)).astype(np.float64)
    X, Y, Z = ((idx[a] + 0.5 * (2.0 * rng.random((N, N, N)) - 1.0)).astype(np.float32) for a in range(3))
    E = (10.0 ** (-20.0 + 10.0 * rng.random((N ** 3, NFREQ)))).astype(np.float32)
    E[rng.random(N ** 3) < 0.1, :] = 1.0e32
    return dict(N=N, I0=np.float32(-13.0 + rng.random()), dI0=np.float32(0.15 + 0.2 * rng.random()),
                I1=(-12.0 + rng.random(N)).astype(np.float32), dI1=(0.1 + 0.2 * rng.random(N)).astype(np.float32),
                I2=(-11.0 + rng.random((N, N))).astype(np.float32), dI2=(0.1 + 0.2 * rng.random((N, N))).astype(np.float32),
                X=X, Y=Y, Z=Z, E=E, FREQ=np.zeros(NFREQ, np.float32))


def cells_of(rng, libs, RABS3, ABU):
    """ABS3[n, 3]: cell c's share of dust c % NDUST lies at uniform coordinates on that dust's grid"""
    n, N = len(ABU), libs[0]["N"]
    den = np.zeros((n, 3), np.float32)
    for j in range(NDUST):
        den = (den.astype(np.float64) + ABU[:, j:j + 1].astype(np.float64) * RABS3[None, :, j]).astype(np.float32)
    ABS3 = np.zeros((n, 3), np.float32)
    for d, lib in enumerate(libs):
        c = np.arange(d, n, NDUST)
        x, y, z = (-0.4 + N * rng.random(len(c)) for _ in range(3))
        i, j = np.clip(np.rint(x).astype(int), 0, N - 1), np.clip(np.rint(y).astype(int), 0, N - 1)
        lg = np.stack([float(lib["I0"]) + x * float(lib["dI0"]), lib["I1"][i] + y * lib["dI1"][i], lib["I2"][i, j] + z * lib["dI2"][i, j]], axis=1)
        ABS3[c] = (10.0 ** lg * den[c] / RABS3[None, :, d]).astype(np.float32)
    return ABS3


def one_count(eng, d, cells, nouts, N, reps, host_cells, check, out):
    dusts, kinds, FREQ = dusts_of(d)
    rng = np.random.default_rng(7)
    RABS, _ = mabu.relative_cross_sections(dusts, kinds)
    RABS3 = np.ascontiguousarray(RABS[list(REF)])
    libs = [library(rng, N) for _ in range(NDUST)]
    ABU = np.ones((cells, NDUST), np.float32)
    ABU[:, 0], ABU[:, 2] = rng.uniform(0.5, 1.5, cells), rng.uniform(0.2, 1.2, cells)
    ABS3 = cells_of(rng, libs, RABS3, ABU)
    # the direct device stage 2 on the same number of cells (its absorptions: a block repeated, their values do not change the work)
    block = rng.lognormal(0, 1, (min(cells, BLOCK), NFREQ)).astype(np.float32)
    block *= (1e-3 * (FREQ[None, :] / 1e13) ** -1.0).astype(np.float32)
    FABS = Tiled(block, 0, cells) if cells > BLOCK else block
    mabu.solve_emission(eng, dusts, kinds, block[:4096], ABU[:4096])
    direct_s = []
    for _ in range(reps):
        t0 = time.time()
        EM, info = mabu.solve_emission(eng, dusts, kinds, FABS, ABU, path='device')
        direct_s.append(time.time() - t0)
        direct_ranges = info["ranges"]
        del EM
    for nout in nouts:
        ocol = None if nout == NFREQ else np.arange(nout, dtype=np.int32)
        fused_ms = []
        eng.mabu_library_begin(cells, NDUST, nout)
        try:
            for i, lib in enumerate(libs):
                eng.mabu_library_set(i, lib, ocol)
            for a in range(0, cells, mabu.CHUNK):
                eng.mabu_library_upload(a, ABS3[a:a + mabu.CHUNK])
            eng.mabu_library_set_tables(ABU, RABS3)
            eng.mabu_library_solve()                                           # warm-up at the timed shape
            for _ in range(reps):
                eng.timer_start()
                eng.mabu_library_solve()
                fused_ms.append(eng.timer_stop())
            MISS = eng.mabu_library_misses(0, cells)
        finally:
            eng.mabu_library_end()
        lookup_s, host_s, same = [], [], None
        for _ in range(reps):
            t0 = time.time()
            ED, idev = mabu.solve_emission_library(eng, dusts, kinds, ABS3, ABU, libs, REF, ocol, path='device')
            lookup_s.append(time.time() - t0)
        nh = min(cells, host_cells)
        for _ in range(reps):
            t0 = time.time()
            EH, _ = mabu.solve_emission_library(eng, dusts, kinds, ABS3[:nh], ABU[:nh], libs, REF, ocol, path='host')
            host_s.append(time.time() - t0)
        if check:
            same = bool(np.array_equal(ED[:nh].view(np.uint32), EH.view(np.uint32)))
        del ED, EH
        fused = float(np.median(fused_ms)) * 1e-3
        moved = (4.0 * nout + 12.0 + 4.0 * NDUST) * cells
        line = {"what": "library method for several dusts: fused look-up against the direct device stage 2 and the host composition",
                "commit": commit(), "cells": cells, "NDUST": NDUST, "NFREQ": NFREQ, "N": N, "nout": nout,
                "tables_MB": NDUST * N ** 3 * nout * 4 / 1e6,
                "answered_share_per_dust": [float(np.mean((MISS >> np.uint32(i)) & np.uint32(1) == 0)) for i in range(NDUST)],
                "fused_ms": fused_ms, "fused_median_ms": float(np.median(fused_ms)), "fused_spread_ms": spread(fused_ms),
                "fused_bytes_per_cell": 4 * nout + 12 + 4 * NDUST, "fused_TBps": moved / fused * 1e-12,
                "fused_share_of_copy_ceiling": moved / fused / COPY_CEILING,
                "lookup_host_arrays_s": lookup_s, "lookup_host_arrays_median_s": float(np.median(lookup_s)), "lookup_host_arrays_spread_s": spread(lookup_s),
                "lookup_ranges": idev["ranges"],
                "direct_device_stage2_s": direct_s, "direct_device_stage2_median_s": float(np.median(direct_s)),
                "direct_device_stage2_spread_s": spread(direct_s), "direct_ranges": direct_ranges,
                "host_cells": nh, "host_composition_s": host_s, "host_composition_median_s": float(np.median(host_s)),
                "host_composition_spread_s": spread(host_s), "host_composition_scaled_to_cells_s": float(np.median(host_s)) * cells / nh,
                "direct_over_lookup": float(np.median(direct_s) / np.median(lookup_s)),
                "host_composition_over_lookup": float(np.median(host_s)) * cells / nh / float(np.median(lookup_s)),
                "bit_identical_to_host_composition": same}
        print(json.dumps(line), flush=True)
        if out:
            with open(out, "a") as fp:
                fp.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="+", default=[12000, 770000, 49500000])
    ap.add_argument("--nout", type=int, nargs="+", default=[50, 5])
    ap.add_argument("--bins", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-cells", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = Engine(0)
    try:
        with tempfile.TemporaryDirectory() as d:
            for cells in a.cells:
                one_count(eng, d, cells, a.nout, a.bins, a.reps, a.host_cells, cells == min(a.cells), a.out)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
