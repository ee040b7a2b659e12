#!/usr/bin/env python3
"""Throughput of the scattered-light kernel (config 4) on its geometry: 256^3-root octree with 3 refinement levels,
3 observers, 256^2 pixels, forced first scattering; background, point-source and cell-emission launches, and launches of the
Healpix sky as the source (SimRAM_HP, --kinds hp).  --healpix NSIDE X Y Z: one Healpix map seen from (X, Y, Z) [root cells] instead.

    python tools/exp_sca.py [--n 256] [--batch 1] [--ndir 3] [--healpix 64 128.3 127.7 126.9] [--kinds bg,ps,cl,hp]

Cartesian geometries: --levels 1 (synth.cartesian_cloud of N^3 cells; --n 128 | 256 | 512 are the grids behind the automatic-mode rule of
the sweep of rays on single-level grids).  --compare times the direct kernel (soc_set_exec(0)) and the sweep of rays
(soc_set_exec(1)) on the same launches in one process: one warm-up of each, then --reps alternated pairs; the line holds the best and the
median of either path and their ratio.

    python tools/exp_sca.py --levels 1 --n 256 --kinds bg --compare [--launches 8] [--batch 1] [--tune '{"brick_cells": 4096}']

Prints one JSON line per launch kind: packets/s and the read-only roofline of SURVEY.md 8(d): 4 B (density) per cell
step of a packet, of a look-ahead and of a peel-off ray (the kernel counts them)."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soc_amd import launch, synth         # noqa: E402
from soc_amd.lib import Engine            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--ndir", type=int, default=3)
    ap.add_argument("--exec", dest="exec_mode", type=int, default=-1, help="-1 automatic, 0 the direct kernel (soc_sca_kernel), 1 the sweep of rays (brick-local hierarchies, single-level grids)")
    ap.add_argument("--cl-global", type=int, default=1048576, help="work items of the cell-emission launch")
    ap.add_argument("--ps-global", type=int, default=1048576)
    ap.add_argument("--tune", default="{}", help="soc_set_tuning settings as JSON")
    ap.add_argument("--launches", type=int, default=1, help="launches (seeds) per measurement, deferred into one batch: soc_batch_begin ... soc_batch_end, as soc_amd.asocs runs the frequencies of a source block")
    ap.add_argument("--healpix", nargs=4, type=float, metavar=("NSIDE", "X", "Y", "Z"), help="a Healpix map of NSIDE seen from (X, Y, Z) in root-grid units instead of --ndir flat images")
    ap.add_argument("--kinds", default="bg,ps,cl", help="launch kinds to time, of bg (SimRAM_PB background), ps (SimRAM_PS), cl (SimRAM_CL), hp (SimRAM_HP: the Healpix sky)")
    ap.add_argument("--compare", action="store_true", help="time the direct kernel and the sweep of rays on the same launches, alternated, after a warm-up of each")
    ap.add_argument("--reps", type=int, default=3, help="--compare: timed pairs")
    a = ap.parse_args()
    N = a.n
    cloud = synth.octree_cloud(N, levels=a.levels, frac=0.10, seed=1234) if a.levels > 1 else synth.cartesian_cloud(N, seed=1234)
    dsc, csc = synth.hg_scattering_table(0.6)
    eng = Engine(0)
    eng.set_cloud(cloud)
    eng.set_features(0, 0, 0)
    eng.set_exec(a.exec_mode, 4)
    eng.set_tuning(**json.loads(a.tune))
    eng.set_scatter_table(dsc, csc)
    k = 2.0 / (N * float(cloud.DENS[cloud.DENS > 0][:N ** 3].mean()))          # optical depth ~2 across the cloud
    eng.set_optical(0.5 * k, k)
    eng.set_opt(None)
    th = [math.radians(30 + 25 * i) for i in range(a.ndir)]
    ph = [math.radians(40 * i) for i in range(a.ndir)]
    _, OD, RA, DE = launch.set_observer_directions(th, ph)
    if a.healpix:
        eng.sca_set_healpix(int(a.healpix[0]), a.healpix[1:], 1)
    else:
        eng.sca_set_view(OD, RA, DE, (256, 256), N / 256.0 * 1.5, (N / 2, N / 2, N / 2), 1)
    AREA = 6 * N * N
    GLOBAL = launch.Fix(8 * AREA, 64)
    ps = np.array([[N / 2 + 0.3, N / 2 + 0.2, N / 2 + 0.1]], np.float32)
    emit = np.where(cloud.DENS > 0, cloud.DENS * 1e-3, 0).astype(np.float32)
    eng.set_emission(emit)
    kinds = a.kinds.split(",")
    if "hp" in kinds:
        eng.set_hpbg(np.random.default_rng(8).lognormal(0, 1, 49152).astype(np.float32))   # a synthetic sky, uniform pixel choice
    runs = (("bg", "SimRAM_PB background", lambda s: eng.sca_sim_pb(1, 8 * AREA * a.batch, a.batch, s, 1.0, GLOBAL=GLOBAL)),
            ("ps", "SimRAM_PS point source", lambda s: eng.sca_sim_ps(a.ps_global * 8, 8, s, 0.0, ps, [1.0], GLOBAL=a.ps_global)),
            ("cl", "SimRAM_CL cell emission", lambda s: eng.sca_sim_cl(2, cloud.CELLS, 1, s, a.cl_global)),
            ("hp", "SimRAM_HP Healpix sky", lambda s: eng.sca_sim_hp(GLOBAL * a.batch, a.batch, s, GLOBAL)))
    def timed(fn, seed):
        eng.sca_zero()
        eng.stats(reset=True)
        eng.timer_start()
        if a.launches > 1:
            eng.batch_begin(0)
            for k in range(a.launches):
                fn(seed + 0.01 * k)
            eng.batch_end()
        else:
            fn(seed)
        ms = eng.timer_stop()
        st = eng.stats()
        st["ray_steps"] = eng.sca_ray_steps()
        st["passes"], st["form"], st["variant"] = eng.last_passes(), eng.last_form(), eng.last_variant()
        return ms, st

    for key, name, fn in runs:
        if key not in kinds or not a.compare:
            continue
        ms = {0: [], 1: []}
        forms = {}
        for rep in range(-1, a.reps):                      # rep -1: the warm-up of either path (bricks built, buffers grown), not counted
            for mode in (0, 1):
                eng.set_exec(mode, 4)
                t, st = timed(fn, 0.3)                     # the same launches for both paths: same packets, same image
                forms[mode] = (st["form"], st["packets"], st["ray_steps"], st["passes"])
                if rep >= 0:
                    ms[mode].append(t)
        assert forms[0][0] == 0 and forms[1][0] != 0 and forms[0][1] == forms[1][1], forms
        pk = forms[0][1]
        line = {"launch": name, "grid": "%d^3 Cartesian" % N, "cells": cloud.CELLS, "launches_in_the_batch": a.launches, "batch": a.batch,
                "work_items": (GLOBAL if key in ("bg", "hp") else a.ps_global if key == "ps" else a.cl_global) * a.launches,
                "ndir": a.ndir, "npix": 256, "packets": pk, "tune": json.loads(a.tune), "reps": a.reps,
                "ray_steps": forms[1][2], "passes": forms[1][3]}
        for mode, tag in ((0, "direct"), (1, "rays")):
            line[tag + "_ms"] = [round(x, 3) for x in ms[mode]]
            line[tag + "_packets_per_s_best"] = pk / min(ms[mode]) * 1e3
            line[tag + "_packets_per_s_median"] = pk / float(np.median(ms[mode])) * 1e3
        line["rays_over_direct_best"] = min(ms[0]) / min(ms[1])
        line["rays_over_direct_median"] = float(np.median(ms[0])) / float(np.median(ms[1]))
        print(json.dumps(line), flush=True)
    for key, name, fn in runs:
        if key not in kinds or a.compare:
            continue
        best = None
        for rep in range(2):
            eng.sca_zero()
            eng.stats(reset=True)
            eng.timer_start()
            if a.launches > 1:
                eng.batch_begin(0)
                for k in range(a.launches):
                    fn(0.3 + 0.1 * rep + 0.01 * k)
                eng.batch_end()
            else:
                fn(0.3 + 0.1 * rep)
            ms = eng.timer_stop()
            st = eng.stats()
            st["ray_steps"] = eng.sca_ray_steps()
            st["passes"], st["form"], st["variant"] = eng.last_passes(), eng.last_form(), eng.last_variant()
            if best is None or ms < best[0]:
                best = (ms, st)
        ms, st = best
        rays = st["form"] == 3
        roof = {}
        if rays:                  # read-only roofline of SURVEY 8(d): 4 B (density) per cell step of a ray
            roof = {"ray_steps": st["ray_steps"], "steps_per_s": st["ray_steps"] / ms * 1e3, "passes": st["passes"],
                    "roofline": {"bound": "hbm", "achieved": 4.0 * st["ray_steps"] / ms * 1e-6, "peak": 8000.0, "unit": "GB/s",
                                 "frac": 4.0 * st["ray_steps"] / ms * 1e-6 / 8000.0}}
        view = ("healpix NSIDE %d from (%g, %g, %g)" % (int(a.healpix[0]), *a.healpix[1:])) if a.healpix else "%d flat images" % a.ndir
        ndir = -int(a.healpix[0]) if a.healpix else a.ndir                       # (NDIR as the kernels see it: -NSIDE for a Healpix map)
        print(json.dumps({"kernel": ("soc_lray_pass (rays on brick-local hierarchies)" if a.levels > 1 else "soc_lray_pass (rays on a single-level grid)") if rays else "soc_sca_kernel", **roof, "launch": name, "launches_in_the_batch": a.launches, "cells": cloud.CELLS, "ndir": ndir, "view": view, "kernel_ms": ms,
                          "variant": st["variant"],
                          "packets": st["packets"], "packets_per_s": st["packets"] / ms * 1e3,
                          "image_contributions": st["tally_events"], "scatterings": st["scatterings"]}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
