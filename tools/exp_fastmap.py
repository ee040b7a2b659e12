#!/usr/bin/env python3
"""Time the maps of --nfreq frequencies of a synthetic cloud on one GPU, one direction: frequency by frequency (Engine.map), or
in batches of NF frequencies per walk along the lines of sight (Engine.set_map_block + Engine.map_block; `mapping nx ny dx NF`).

    python tools/exp_fastmap.py --case oct256 --per-frequency [--nfreq 32] [--reps 5] [--out profiles/fastmap_lines.json]
    python tools/exp_fastmap.py --case oct256 --block 2 4 8 16 32
    python tools/exp_fastmap.py --case c128 --per-frequency --tree <checkout of another commit, built>
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/exp_fastmap.py --case oct256 --per-frequency --block 16 --reps 1 --out /dev/null

Cases: oct256 = 1024 x 1024 pixels of the config-3 octree (synth.octree_cloud(256, levels=4, frac=0.10, seed=1234)); c128 = 512 x
512 pixels of a 128^3 Cartesian cloud.  --per-frequency uses Engine.set_cloud and Engine.map only, so with --tree it runs on a
build of a commit that has no batch calls: that is the yardstick.  A time is the wall clock around all --nfreq frequencies, end
to end -- uploads of the emission, kernels, downloads of the planes -- with the host arrays laid out before the clock starts (one
contiguous array per frequency, or one cell-major array per batch); after one warm-up pass, --reps passes: min, median, max.
The kernels alone are in the rocprofv3 summary.  One JSON line per run is printed and appended to --out."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = {
    "oct256": dict(cloud=lambda synth: synth.octree_cloud(256, levels=4, frac=0.10, seed=1234), NPIX=(1024, 1024), MAP_DX=0.4, opt=2.0e-6),
    "c128": dict(cloud=lambda synth: synth.cartesian_cloud(128, seed=21), NPIX=(512, 512), MAP_DX=0.4, opt=8.0e-6),
}


def commit(tree):
    try:
        return subprocess.check_output(["git", "-C", tree, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


def passes(fn, reps):
    fn()                                   # warm-up: buffers allocated, code objects loaded
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1.0e3 * (time.perf_counter() - t0))
    t = np.asarray(t)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), all_ms=[float(x) for x in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="oct256", choices=sorted(CASES))
    ap.add_argument("--nfreq", type=int, default=32)
    ap.add_argument("--per-frequency", action="store_true")
    ap.add_argument("--block", type=int, nargs="*", default=[], help="batch sizes NF to time")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose soc_amd (and built library) is used")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastmap_lines.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from soc_amd import launch, synth
    from soc_amd.lib import Engine

    k = CASES[a.case]
    c = k["cloud"](synth)
    _, ODIR, RA, DE = launch.set_observer_directions([math.radians(50.0)], [math.radians(35.0)])
    centre = (0.5 * c.NX, 0.5 * c.NY, 0.5 * c.NZ)
    base = np.asarray(np.random.default_rng(3).uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
    scale = np.linspace(0.5, 2.0, a.nfreq, dtype=np.float32)
    ABS = np.asarray(0.4 * k["opt"] * np.geomspace(0.1, 10.0, a.nfreq), np.float32)
    SCA = np.asarray(0.6 * k["opt"] * np.geomspace(0.1, 10.0, a.nfreq), np.float32)
    eng = Engine(0)
    head = dict(case=a.case, cells=int(c.CELLS), levels=int(c.LEVELS), npix=list(k["NPIX"]), nfreq=a.nfreq, reps=a.reps,
                commit=commit(os.path.abspath(a.tree)), label=a.label)

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as fp:
            fp.write(json.dumps(line) + "\n")

    try:
        eng.set_cloud(c)
        check = None
        if a.per_frequency:
            cols = [base * scale[f] for f in range(a.nfreq)]
            last = {}

            def run():
                for f in range(a.nfreq):
                    last["m"], last["t"] = eng.map(cols[f], ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre, ABS[f], SCA[f])
            emit(dict(head, mode="per-frequency", NF=1, **passes(run, a.reps)))
            check = (last["m"].copy(), last["t"].copy())
            del cols
        for NF in a.block:
            nb = min(NF, eng.map_block_max)
            batches = [(np.ascontiguousarray(np.multiply.outer(base, scale[b:b + nb]), np.float32), ABS[b:b + nb], SCA[b:b + nb])
                       for b in range(0, a.nfreq, nb)]
            last = {}

            def run():
                for E, A, S in batches:
                    eng.set_map_block(E, A, S)
                    last["m"], last["t"], _ = eng.map_block(ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre)
            line = dict(head, mode="block", NF=nb, **passes(run, a.reps))
            if check is not None:                              # the last frequency's planes against the per-frequency pass of this process
                line["same_bits"] = bool(np.array_equal(last["m"][-1].view(np.uint32), check[0].view(np.uint32))
                                         and np.array_equal(last["t"][-1].view(np.uint32), check[1].view(np.uint32)))
            emit(line)
            eng.set_map_block(None)
            del batches
    finally:
        eng.close()


if __name__ == "__main__":
    main()
