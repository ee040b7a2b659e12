#!/usr/bin/env python3
"""Time the per-level maps (Engine.map_levels; `mapping nx ny dx 999`) of a synthetic cloud on one GPU, one direction, next to
the plain map (Engine.map) of the same size in the same process: one frequency, and --nfreq frequencies one after the other.

    python tools/exp_levelmap.py [--case oct256] [--nfreq 8] [--reps 5] [--out profiles/levelmap_lines.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/exp_levelmap.py --reps 1 --nfreq 1 --out /dev/null

Cases: those of tools/exp_fastmap.py (oct256 = 1024 x 1024 pixels of the config-3 octree).  A time is the wall clock around the
calls, end to end -- upload of the emission, kernel, download of the planes (LEVELS planes for the per-level maps, two for the
plain one) -- after one warm-up pass, --reps passes: min, median, max.  The kernels alone are in the rocprofv3 summary.  The
sum of the levels is compared with the plain map (the two kernel files enter the cloud an EPS apart and walk differently
after a climb into a root leaf, so this is a loose figure, printed, not a check).  One JSON line per mode is printed and
appended to --out."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levelmap_lines.json"))
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
    cols = [base * scale[f] for f in range(a.nfreq)]
    eng = Engine(0)
    head = dict(case=a.case, cells=int(c.CELLS), levels=int(c.LEVELS), npix=list(k["NPIX"]), reps=a.reps, commit=commit(ROOT), label=a.label)
    last = {}

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as fp:
            fp.write(json.dumps(line) + "\n")

    def plain(n):
        for f in range(n):
            last["plain"], _ = eng.map(cols[f], ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre, ABS[f], SCA[f])

    def levels(n):
        for f in range(n):
            last["levels"] = eng.map_levels(cols[f], ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre, ABS[f], SCA[f])

    try:
        eng.set_cloud(c)
        for n in sorted({1, a.nfreq}):
            p = passes(lambda: plain(n), a.reps)
            emit(dict(head, mode="plain", nfreq=n, **p))
            q = passes(lambda: levels(n), a.reps)
            total = last["levels"].astype(np.float64).sum(axis=0)
            ref = last["plain"].astype(np.float64)
            lit = ref > 0.0
            emit(dict(head, mode="levels", nfreq=n, ratio_to_plain=q["median_ms"] / p["median_ms"],
                      pixels_lit_per_level=[int((last["levels"][l] != 0.0).sum()) for l in range(c.LEVELS)],
                      sum_of_levels_vs_plain_median_rel=float(np.median(np.abs(total[lit] / ref[lit] - 1.0))), **q))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
