#!/usr/bin/env python3
"""Time a `split 1` background launch (soc_sim_bg_split) next to the plain background launch (soc_sim_pb, direct kernel) with the
same number of root rays, on the config-3 geometry (256^3 roots, 4 levels) and on octree_cloud(64, levels=4).

    python tools/exp_split.py [--small] [--hpbg] [--out profiles/split_lines.json]

--hpbg: the same with a Healpix sky -- a `split 1` + `hpbg` launch (soc_sim_hp_split) next to the plain Healpix launch (soc_sim_hp) with
the same number of root rays, 100 per work item (profiles/hpsplit_lines.json).

Prints one JSON line per model: launch shapes, milliseconds (median of 3 after a warm-up), root rays and rays per second of both
launches, their ratio, the split counters and the memory the ray stacks take.  Needs a GPU.
"""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from soc_amd import launch, synth                      # noqa: E402
from soc_amd.lib import Engine, device_bytes           # noqa: E402


def timed(eng, fn, n=3):
    fn()
    eng.sync()
    ts = []
    for _ in range(n):
        eng.timer_start()
        fn()
        ts.append(eng.timer_stop())
    return float(np.median(ts))


def one(eng, name, cloud, BGPAC, ABS, SCA, max_split=0):
    _, csc = synth.hg_scattering_table(0.6)
    eng.set_cloud(cloud)
    eng.set_features(0, 0, 0)
    eng.set_scatter_table(None, csc)
    eng.set_optical(ABS, SCA)
    eng.set_exec(0, 4)
    S = launch.bg_split_launch(BGPAC, cloud.AREA)
    P = launch.bg_launch(S["PACKETS"], cloud.AREA)
    before = device_bytes()
    eng.zero(0)
    eng.split_stats(reset=True)
    t_split = timed(eng, lambda: eng.sim_bg_split(S["PACKETS"], S["BATCH"], 0.377, 1.0, 1.0, S["SELEM"], max_split, GLOBAL=S["GLOBAL"]))
    st = eng.split_stats(reset=True)
    stack = device_bytes() - before
    e_split = float(eng.read_tally(0).astype(np.float64).sum()) / 4.0 / S["BATCH"]
    eng.zero(0)
    t_plain = timed(eng, lambda: eng.sim_pb(1, P["PACKETS"], P["BATCH"], 0.377, 1.0, 1.0, GLOBAL=P["GLOBAL"]))
    e_plain = float(eng.read_tally(0).astype(np.float64).sum()) / 4.0 / (8 * P["BATCH"])
    line = dict(model=name, cells=int(cloud.CELLS), levels=int(cloud.LEVELS), split=dict(S, WBG=None, ms=t_split, roots_per_s=S["PACKETS"] / (1e-3 * t_split)),
                plain=dict(P, WBG=None, ms=t_plain, roots_per_s=P["PACKETS"] / (1e-3 * t_plain)), ms_ratio_split_over_plain=t_split / t_plain,
                absorbed_per_ray_per_element=dict(split=e_split, plain=e_plain), counters_of_4_launches=st, stack_bytes=int(stack))
    print(json.dumps(line))
    return line


def one_hp(eng, name, cloud, ABS, SCA, max_split=0, n=5):
    """sim_hp_split on GLOBAL_SPLIT work items x 100 rays next to sim_hp on the same number of work items (all below 8*AREA, so none
    returns early): the same number of root rays from the same sky"""
    _, csc = synth.hg_scattering_table(0.6)
    eng.set_cloud(cloud)
    eng.set_features(0, 0, 0)
    eng.set_scatter_table(None, csc)
    eng.set_optical(ABS, SCA)
    eng.set_exec(0, 4)
    rr = np.random.default_rng(5)
    sky = ((1.0 + 0.6 * np.cos(np.pi * (np.arange(49152) + 0.5) / 49152.0)) * np.exp(0.5 * np.log(10.0) * rr.standard_normal(49152))).astype(np.float32)
    eng.set_hpbg(sky, None)
    S = launch.hp_split_launch(1, cloud.NX, cloud.NY, cloud.NZ, cloud.AREA)
    G = launch.Fix(S["GLOBAL"], 64)
    assert G <= 8 * cloud.AREA
    roots = G * S["BATCH"]
    before = device_bytes()
    eng.zero(0)
    eng.split_stats(reset=True)
    t_split = timed(eng, lambda: eng.sim_hp_split(roots, S["BATCH"], 0.377, 1.0, max_split, GLOBAL=G), n)
    st = eng.split_stats(reset=True)
    stack = device_bytes() - before
    e_split = float(eng.read_tally(0).astype(np.float64).sum()) / (n + 1) / roots
    eng.zero(0)
    t_plain = timed(eng, lambda: eng.sim_hp(roots, S["BATCH"], 0.377, 1.0, G), n)
    e_plain = float(eng.read_tally(0).astype(np.float64).sum()) / (n + 1) / roots
    line = dict(model=name, cells=int(cloud.CELLS), levels=int(cloud.LEVELS), GLOBAL=G, BATCH=S["BATCH"], root_rays=roots, launches_timed=n,
                split=dict(ms=t_split, roots_per_s=roots / (1e-3 * t_split)), plain=dict(ms=t_plain, roots_per_s=roots / (1e-3 * t_plain)),
                ms_ratio_split_over_plain=t_split / t_plain, absorbed_per_root_ray=dict(split=e_split, plain=e_plain),
                counters_of_all_launches=st, stack_bytes=int(stack))
    print(json.dumps(line))
    return line


def main(argv):
    small = "--small" in argv
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    eng = Engine(0)
    lines = []
    try:
        if "--hpbg" in argv:
            if small:
                lines.append(one_hp(eng, "octree_cloud(16, levels=3)", synth.octree_cloud(16, levels=3, frac=0.1, seed=3), 3e-6 * 16, 3e-5 * 16, 64))
            else:
                lines.append(one_hp(eng, "config 3: octree_cloud(256, levels=4)", synth.octree_cloud(256, levels=4, frac=0.08, seed=3), 3e-6, 3e-5))
        elif small:
            lines.append(one(eng, "octree_cloud(16, levels=3)", synth.octree_cloud(16, levels=3, frac=0.1, seed=3), 20000, 3e-6 * 16, 3e-5 * 16, 64))
        else:
            lines.append(one(eng, "octree_cloud(64, levels=4)", synth.octree_cloud(64, levels=4, frac=0.1, seed=3), 400000, 1.2e-5, 1.2e-4))
            lines.append(one(eng, "config 3: octree_cloud(256, levels=4)", synth.octree_cloud(256, levels=4, frac=0.08, seed=3), 2000000, 3e-6, 3e-5))
    finally:
        eng.close()
    if out:
        with open(out, "w") as fp:
            json.dump(lines, fp, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
