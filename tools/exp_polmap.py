#!/usr/bin/env python3
"""Time soc_polmap (POLSTAT 0, 1, 3) against soc_map of the same size on one GPU -- and, with --healpix NSIDE,
soc_polmap_healpix (interpolate 0 and 3) against soc_map(healpix=1) of the same NSIDE, seen from near the cloud's centre.

    python tools/exp_polmap.py [--cases c128 oct104abu oct256] [--reps 7] [--out profiles/polmap_lines.json]
    python tools/exp_polmap.py --healpix 256 [--cases ...] [--out profiles/hpolmap_lines.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/exp_polmap.py --cases c128 oct104abu --reps 3 --out /dev/null

Cases: c128 = 500 x 333 pixels of a 128^3 Cartesian cloud; oct104abu = 300 x 300 pixels of the 104^3-root octree with per-cell
opacities; oct256 = 1024 x 1024 pixels of the config-3 octree (synth.octree_cloud(256, levels=4, frac=0.10, seed=1234)).
Every time is taken with the handle's HIP events (soc_timer_start / soc_timer_stop) around one call -- the upload of EMIT, the
kernel and the download of the planes, for soc_map and soc_polmap alike -- after one warm-up call; median and spread
(min, max) of --reps repetitions.  The kernels alone are in the rocprofv3 summary.  One JSON line per case is appended to --out."""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from soc_amd import launch, synth         # noqa: E402
from soc_amd.lib import Engine            # noqa: E402


def commit():
    try:
        return subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL, text=True).strip()
    except Exception:
        return os.environ.get("SOC_COMMIT", "unknown")


CASES = {
    "c128": dict(cloud=lambda: synth.cartesian_cloud(128, seed=21), NPIX=(500, 333), MAP_DX=0.45, abu=False, opt=8.0e-6),
    "oct104abu": dict(cloud=lambda: synth.octree_cloud(104, levels=3, frac=0.002, seed=11), NPIX=(300, 300), MAP_DX=0.6, abu=True, opt=8.0e-6),
    "oct256": dict(cloud=lambda: synth.octree_cloud(256, levels=4, frac=0.10, seed=1234), NPIX=(1024, 1024), MAP_DX=0.4, abu=False, opt=2.0e-6),
}


def timed(eng, fn, reps):
    fn()                                   # warm-up
    t = []
    for _ in range(reps):
        eng.timer_start()
        fn()
        t.append(eng.timer_stop())
    t = np.asarray(t)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["c128", "oct104abu", "oct256"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polmap_lines.json"))
    ap.add_argument("--healpix", type=int, default=0, help="NSIDE: time the all-sky maps instead of the flat ones")
    a = ap.parse_args()
    if a.healpix and a.out.endswith("polmap_lines.json") and not a.out.endswith("hpolmap_lines.json"):
        a.out = os.path.join(ROOT, "profiles", "hpolmap_lines.json")
    _, ODIR, RA, DE = launch.set_observer_directions([math.radians(50.0)], [math.radians(35.0)])
    eng = Engine(0)
    try:
        for name in a.cases:
            k = CASES[name]
            c = k["cloud"]()
            rng = np.random.default_rng(3)
            EMIT = np.asarray(rng.uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
            centre = (0.5 * c.NX, 0.5 * c.NY, 0.5 * c.NZ)
            eng.set_cloud(c)
            eng.set_opt(np.asarray(rng.uniform(0.25, 1.0, (c.CELLS, 2)) * k["opt"], np.float32) if k["abu"] else None)
            eng.set_bfield(*synth.magnetic_field(c, seed=6))
            ABS, SCA = 0.4 * k["opt"], 0.6 * k["opt"]
            if a.healpix:
                obs = (0.5 * c.NX + 0.3, 0.5 * c.NY - 0.4, 0.5 * c.NZ + 0.2)
                line = dict(case=name, cells=c.CELLS, levels=c.LEVELS, nside=a.healpix, observer=list(obs), reps=a.reps, commit=commit())
                line["soc_map_healpix"] = timed(eng, lambda: eng.map(EMIT, ODIR[0], RA[0], DE[0], (a.healpix, -1), 1.0, centre, ABS, SCA, INTOBS=obs,
                                                                     healpix=a.healpix), a.reps)
                for mode in (0, 3):
                    line["soc_polmap_healpix_i%d" % mode] = timed(eng, lambda: eng.polmap_healpix(EMIT, a.healpix, obs, ABS, SCA, interpolate=mode), a.reps)
                    line["ratio_i%d" % mode] = line["soc_polmap_healpix_i%d" % mode]["median_ms"] / line["soc_map_healpix"]["median_ms"]
                eng.set_bfield(None)
                print(json.dumps(line))
                with open(a.out, "a") as fp:
                    fp.write(json.dumps(line) + "\n")
                continue
            line = dict(case=name, cells=c.CELLS, levels=c.LEVELS, npix=list(k["NPIX"]), reps=a.reps, commit=commit())
            line["soc_map"] = timed(eng, lambda: eng.map(EMIT, ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre, ABS, SCA, save_colden=1), a.reps)
            for polstat in (0, 1, 3):
                line["soc_polmap_%d" % polstat] = timed(eng, lambda: eng.polmap(EMIT, ODIR[0], RA[0], DE[0], k["NPIX"], k["MAP_DX"], centre, ABS, SCA,
                                                                                polstat=polstat), a.reps)
                line["ratio_%d" % polstat] = line["soc_polmap_%d" % polstat]["median_ms"] / line["soc_map"]["median_ms"]
            eng.set_bfield(None)
            print(json.dumps(line))
            with open(a.out, "a") as fp:
                fp.write(json.dumps(line) + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
