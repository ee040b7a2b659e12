#!/usr/bin/env python3
"""The library method on one GPU: what the look-up writes per second, the build against its numpy statement, and the look-up
against the direct solve of the same cells.

    python tools/exp_library.py [--cells 10000000] [--solve-cells 1048576] [--reps 5] [--out profiles/library_lines.json]

Three JSON lines are appended to --out, each with the commit it was taken at (`git rev-parse`; where the tree is not a git
checkout, what the environment variable SOC_COMMIT says):
  1. the look-up with the cells resident (soc_library_solve_resident), N = 30, NFREQ = 50: the kernel with its miss count read
     back, host clock around a call that ends in a device synchronise, warmed up; bytes written (cells x NFREQ x 4) per second
     and that as a fraction of the float4 copy this project measured (6.29 TB/s);
  2. the build (soc_library_build on the resident columns: four sweeps and the table arithmetic on the host in between) against
     the numpy statement of tests/library_numpy.py (soc_library.py's N + N^2 masked passes) on the host;
  3. soc_amd.library.solve against soc_amd.a2e.run on the same cells, host arrays in and out, with the synthetic 128-bin solver
     (3 sizes): the factor a user gets.
The absorptions are synthetic: a power law in frequency with a level spread over six decades and lognormal scatter."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from soc_amd import a2e, library, synth   # noqa: E402
from soc_amd.lib import Engine            # noqa: E402

N, NFREQ, NE = 30, 50, 128
COPY_CEILING = 6.29e12                    # B/s, float4 copy
REF = np.asarray([10, 25, 40], np.int32)  # the reference columns


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


def absorptions(sol, cells, seed=1):
    """distinct rows for up to 2^20 cells, repeated beyond that (the kernels do not care, the host generator does)"""
    rng = np.random.default_rng(seed)
    n = min(cells, 1 << 20)
    u = rng.uniform(-9.0, -3.0, n)
    A = (10.0 ** u[:, None] * (np.asarray(sol["FREQ"], np.float64)[None, :] / 1e13) ** -1.0 * rng.lognormal(0, 0.5, (n, NFREQ))).astype(np.float32)
    return np.ascontiguousarray(np.tile(A, ((cells + n - 1) // n, 1))[:cells])


def synthetic_library(grid, seed=2):
    """the grid of a build with an emission row for every represented bin (the look-up copies rows, whatever they hold)"""
    lib = dict(grid)
    E = np.full((N ** 3, NFREQ), 1.0e32, np.float32)
    has = grid["IND"] >= 0
    E[has] = np.random.default_rng(seed).lognormal(0, 1, (int(has.sum()), NFREQ)).astype(np.float32)
    lib["E"] = E
    return lib


def timed(fn, reps):
    fn()                                                             # warm-up: code objects, allocations
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=10_000_000)
    ap.add_argument("--numpy-cells", type=int, default=10_000_000, help="cells of the numpy statement of the build (its passes are linear in them)")
    ap.add_argument("--solve-cells", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "library_lines.json"))
    a = ap.parse_args()
    sol = synth.synth_solver(NFREQ=NFREQ, NE=NE, NSIZE=3, seed=5)
    eng = Engine(0)
    lines = []
    ABS = absorptions(sol, a.cells)
    eng.a2e_resident_begin(a.cells, NFREQ)
    try:
        for c0 in range(0, a.cells, 1 << 20):
            eng.a2e_resident_upload(c0, ABS[c0:c0 + (1 << 20)])
        tb = timed(lambda: eng.library_build(N, cols=REF), a.reps)
        grid = eng.library_build(N, cols=REF)
        lib = synthetic_library(grid)
        eng.library_set(lib)
        miss = eng.library_solve_resident(REF)
        ts = timed(lambda: eng.library_solve_resident(REF), a.reps)
        eng.library_set(None)
    finally:
        eng.a2e_resident_end()
    written = a.cells * NFREQ * 4
    best = min(ts)
    lines.append(dict(what="library look-up, cells resident (soc_library_solve_resident): kernel + miss count read back, host clock to the synchronise",
                      commit=commit(), cells=a.cells, N=N, NFREQ=NFREQ, misses=int(len(miss)), bins_filled=int((grid["IND"] >= 0).sum()),
                      s=ts, bytes_written=written, written_TBps=written / best / 1e12, read_TBps=a.cells * 12 / best / 1e12,
                      copy_ceiling_TBps=COPY_CEILING / 1e12, fraction_of_copy_ceiling=written / best / COPY_CEILING))
    # 2. the build against numpy
    from library_numpy import numpy_build, same_build
    import library_host
    sub = np.ascontiguousarray(ABS[:a.numpy_cells, REF])
    t0 = time.perf_counter()
    want = numpy_build(N, sub, lambda x: library_host.log10("soc", x))
    tn = time.perf_counter() - t0
    td = timed(lambda: eng.library_build(N, ABS3=sub), 2)
    got = eng.library_build(N, ABS3=sub)
    lines.append(dict(what="library build: device (resident columns; host arrays) against the numpy statement of tests/library_numpy.py on the host",
                      commit=commit(), cells=a.cells, N=N, device_resident_s=tb, numpy_cells=a.numpy_cells, numpy_s=tn,
                      device_host_arrays_s_at_numpy_cells=td, same_result=same_build(got, want) == [],
                      speedup_resident=tn * (a.cells / a.numpy_cells) / min(tb), host_threads=int(os.environ.get("OMP_NUM_THREADS", os.cpu_count()))))
    # 3. the look-up against the direct solve, host arrays in and out
    n = a.solve_cells
    small = np.ascontiguousarray(ABS[:n])
    t0 = time.perf_counter()
    full = library.build(eng, sol, small, sol["FREQ"], REF, N, verbose=False)
    tlib = time.perf_counter() - t0
    EM = np.zeros((n, NFREQ), np.float32)
    library.solve(eng, sol, full, small, REF, EM, verbose=False)     # warm-up
    tl = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        mis, _ = library.solve(eng, sol, full, small, REF, EM, verbose=False)
        tl.append(time.perf_counter() - t0)
    a2e.run(eng, sol, small[:4096], verbose=False)
    ta = []
    for _ in range(2):
        t0 = time.perf_counter()
        direct, _ = a2e.run(eng, sol, small, verbose=False)
        ta.append(time.perf_counter() - t0)
    hit = EM[:, 0] < 1.0e31
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(EM[hit] - direct[hit]) / np.maximum(np.abs(direct[hit]), 1e-30)
    lines.append(dict(what="soc_amd.library.solve (missed cells solved directly) against soc_amd.a2e.run on the same cells, host arrays in and out",
                      commit=commit(), cells=n, N=N, NFREQ=NFREQ, NE=NE, NSIZE=3, library_build_s=tlib, library_solve_s=tl, missed=int(mis),
                      a2e_run_s=ta, speedup=min(ta) / min(tl), median_relative_difference_to_direct=float(np.median(rel))))
    eng.close()
    with open(a.out, "a") as fp:
        for ln in lines:
            fp.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))
    return 0


if __name__ == "__main__":
    sys.exit(main())
