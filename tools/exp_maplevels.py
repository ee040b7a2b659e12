#!/usr/bin/env python3
"""Time the levels of the plain map (Engine.map_block_levels; `maplevels 1`) of a synthetic cloud on one GPU, one direction, next
to the plain maps of the same resident batch (Engine.map_block) in the same process.

    python tools/exp_maplevels.py [--case oct256] [--nfreq 8] [--reps 5] [--out profiles/maplevels_lines.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/exp_maplevels.py --reps 1 --out /dev/null

Cases: those of tools/exp_fastmap.py (oct256 = 1024 x 1024 pixels of the config-3 octree).  The batch of --nfreq frequencies is
uploaded once, before the clock starts.  A time is the wall clock around one call, end to end -- kernel launches and the download
of the planes (2 * nfreq + 1 for map_block, nfreq * LEVELS for map_block_levels) -- after one warm-up call, --reps calls: min,
median, max.  The kernels alone are in the rocprofv3 summary.  Without this call the same planes cost LEVELS masked uploads and
LEVELS map_block calls, so the line of map_block_levels also gives its time over LEVELS times that of map_block (the uploads
left out, which favours the old way).  The sum of the planes is compared with the plain map (printed, not a check).  One JSON
line per mode is printed and appended to --out."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from exp_fastmap import CASES, commit, passes          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="oct256", choices=sorted(CASES))
    ap.add_argument("--nfreq", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maplevels_lines.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
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
    EMITX = np.ascontiguousarray(np.multiply.outer(base, scale), np.float32)
    eng = Engine(0)
    head = dict(case=a.case, cells=int(c.CELLS), levels=int(c.LEVELS), npix=list(k["NPIX"]), nfreq=a.nfreq, reps=a.reps,
                commit=commit(ROOT), label=a.label)
    last = {}

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as fp:
            fp.write(json.dumps(line) + "\n")

    def plain():
        last["plain"] = eng.map_block(ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre)[0]

    def levels():
        last["levels"] = eng.map_block_levels(ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre)

    try:
        eng.set_cloud(c)
        eng.set_map_block(EMITX, ABS, SCA)
        p = passes(plain, a.reps)
        emit(dict(head, mode="map_block", **p))
        q = passes(levels, a.reps)
        total = last["levels"].astype(np.float64).sum(axis=1)
        ref = last["plain"].astype(np.float64)
        lit = ref > 0.0
        emit(dict(head, mode="map_block_levels", columns_per_launch=int(eng.map_block_levels_width),
                  ratio_to_map_block=q["median_ms"] / p["median_ms"], ratio_to_levels_times_map_block=q["median_ms"] / (c.LEVELS * p["median_ms"]),
                  pixels_lit_per_level=[int((last["levels"][0, l] != 0.0).sum()) for l in range(c.LEVELS)],
                  sum_of_levels_vs_plain_max_rel=float(np.max(np.abs(total[lit] / ref[lit] - 1.0))), **q))
        eng.set_map_block(None)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
