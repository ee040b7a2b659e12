#!/usr/bin/env python3
"""Time the brick-local walk in its float form (soc_set_tuning float_local=1: soc_lbrick_pass_flt, form 3) next to the sweep that
hierarchies with Index() in float took before it (float_local=0: the hierarchy read from global memory, form 2), on two geometries:

    oct64_l4     synth.octree_cloud(64, levels=4, frac=0.10, seed=1234)      a 64^3-root octree of four levels
    oct256_l2    synth.octree_cloud(256, levels=2, frac=0.10, seed=1234)     a 256^3 root grid with one level of refinement

    python tools/exp_float_local.py [--small] [--models oct64_l4,oct256_l2] [--freqs 3] [--repeats 3] [--out profiles/float_local_lines.json]

One set of launches per geometry -- a point source, the isotropic background and cell emission at each of --freqs frequencies, scalar
opacities -- is handed to the engine as one batch (soc_batch_begin / soc_batch_end, TABS only).  After a warm-up round the two routings
are timed in turn, --repeats times round (a, b, a, b, ...), in one process, with HIP events.  Prints one JSON line per geometry and
routing: packets/s and cell steps/s (median, and the spread (max - min) / median over the repeats), the form and kernel that ran, the
event counts -- and per geometry a verdict line: (b) faster than (a) by more than the larger of the two spreads, event counts equal.
The last line says what the drivers' switch AbsorptionRun.FLOAT_LOCAL should be: on only if (b) wins on every geometry.
--small: octree_cloud(32, levels=4) and octree_cloud(64, levels=2) with short launches, to try the tool.  Needs a GPU.
"""
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from soc_amd import synth                              # noqa: E402
from soc_amd.lib import Engine                         # noqa: E402

MODELS = {
    "oct64_l4": (lambda: synth.octree_cloud(64, levels=4, frac=0.10, seed=1234), "octree_cloud(64, levels=4, frac=0.10, seed=1234)"),
    "oct256_l2": (lambda: synth.octree_cloud(256, levels=2, frac=0.10, seed=1234), "octree_cloud(256, levels=2, frac=0.10, seed=1234)"),
}
SMALL = {
    "oct64_l4": (lambda: synth.octree_cloud(32, levels=4, frac=0.10, seed=1234), "small: octree_cloud(32, levels=4, frac=0.10, seed=1234)"),
    "oct256_l2": (lambda: synth.octree_cloud(64, levels=2, frac=0.10, seed=1234), "small: octree_cloud(64, levels=2, frac=0.10, seed=1234)"),
}


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def opacities(cloud):
    """about one optical depth of scattering across the model: packets scatter a few times before they leave"""
    root = cloud.DENS[:cloud.NX * cloud.NY * cloud.NZ]
    k = 1.0 / (cloud.NX * float(root[root > 0].mean()))
    return 0.1 * k, k


def launches(eng, cloud, freqs, small, target):
    """the batch: per frequency a point-source, a background and a cell-emission launch, about `target` packets each"""
    n = cloud.NX
    ps = np.array([[0.501 * n, 0.501 * n, 0.501 * n]], np.float32)
    bg_items = 8 * cloud.AREA
    G0 = 65536 if small else 1048576
    a, s = opacities(cloud)
    eng.batch_begin(0)
    for f in range(freqs):
        eng.set_optical(a * (1 + 0.3 * f), s * (1 + 0.1 * f))
        seed = 0.2 + 0.013 * f
        eng.sim_pb(0, 0, max(1, target // G0), seed, 0.0, 1.0, PSPOS=ps, PS=[1.0 + f], GLOBAL=G0)
        eng.sim_pb(1, 0, max(1, target // bg_items), seed + 0.1, 1.0 + f, 1.0, GLOBAL=bg_items)
        eng.sim_cl(2, 0, 1, seed + 0.2, 1.0, min(target, 4 * G0))
    eng.batch_end()
    eng.sync()


def measure(eng, name, make, model, freqs, repeats, small):
    cloud = make()
    _, csc = synth.hg_scattering_table(0.6)
    emit = np.where(cloud.DENS > 0, cloud.DENS * 1e-3, 0).astype(np.float32)
    variants = (("a", "float_local=0: the hierarchy in global memory (the path of these grids before the float form)", 0),
                ("b", "float_local=1: brick-local walk, float form", 1))
    res = {k: dict(ms=[], stats=None, form=None, variant=None) for k, _, _ in variants}
    target = 400000 if small else 16000000
    eng.set_cloud(cloud)
    eng.set_features(0, 0, 0)
    eng.set_scatter_table(None, csc)
    eng.set_opt(None)
    eng.set_exec(1, 4)
    eng.set_emission(emit, None)                                   # (once: the cell-emission launches share the copy)
    a, s = opacities(cloud)
    for rnd in range(repeats + 1):                                 # round 0 warms up: brick tables, buffers, clocks
        for key, _, local in variants:
            eng.set_tuning(float_local=local)
            # (a small launch of the routing builds its brick tables before the clock starts)
            eng.set_optical(a, s)
            eng.sim_pb(1, 0, 1, 0.5, 1.0, 1.0, GLOBAL=8 * cloud.AREA, gid_first=0, gid_count=4096)
            eng.sync()
            eng.zero(0)
            eng.stats(reset=True)
            eng.timer_start()
            launches(eng, cloud, freqs, small, target)
            ms = eng.timer_stop()
            st = eng.stats()
            r = res[key]
            r["form"], r["variant"] = eng.last_form(), eng.last_variant()
            if rnd > 0:
                r["ms"].append(ms)
                assert r["stats"] is None or r["stats"] == st, "the event counts of a routing changed between repeats"
                r["stats"] = st
    eng.set_tuning(float_local=0)
    lines = []
    for key, text, local in variants:
        r = res[key]
        ms = np.asarray(r["ms"])
        med = float(np.median(ms))
        lines.append(dict(geometry=name, variant=key, what=text, model=model, cells=int(cloud.CELLS), launches=3 * freqs, frequencies=freqs,
                          form=r["form"], kernel=r["variant"], ms=[float(x) for x in ms], ms_median=med, spread=float((ms.max() - ms.min()) / med),
                          packets=r["stats"]["packets"], tally_events=r["stats"]["tally_events"], scatterings=r["stats"]["scatterings"],
                          packets_per_s=r["stats"]["packets"] / (1e-3 * med), cell_steps_per_s=r["stats"]["tally_events"] / (1e-3 * med),
                          commit=commit()))
        print(json.dumps(lines[-1]), flush=True)
    a_, b_ = lines
    spread = max(a_["spread"], b_["spread"])
    gain = a_["ms_median"] / b_["ms_median"] - 1.0
    verdict = dict(verdict=True, geometry=name, b_over_a_speedup=a_["ms_median"] / b_["ms_median"], gain=gain, spread_of_the_call=spread,
                   b_faster_than_a_beyond_spread=bool(gain > spread), forms=[a_["form"], b_["form"]],
                   events_equal_a_b=bool(all(a_[k] == b_[k] for k in ("packets", "tally_events", "scatterings"))), commit=commit())
    print(json.dumps(verdict), flush=True)
    return lines + [verdict]


def main(argv):
    def arg(name, default):
        return type(default)(argv[argv.index(name) + 1]) if name in argv else default
    small = "--small" in argv
    freqs, repeats, out = arg("--freqs", 3), arg("--repeats", 3), arg("--out", "")
    names = arg("--models", "oct64_l4,oct256_l2").split(",")
    table = SMALL if small else MODELS
    eng = Engine(0)
    lines = []
    try:
        for name in names:
            make, model = table[name]
            lines += measure(eng, name, make, model, freqs, repeats, small)
    finally:
        eng.set_tuning(float_local=0)
        eng.close()
    verdicts = [x for x in lines if x.get("verdict")]
    switch = dict(switch="AbsorptionRun.FLOAT_LOCAL", geometries=[v["geometry"] for v in verdicts],
                  on=bool(len(verdicts) == len(MODELS) and all(v["b_faster_than_a_beyond_spread"] and v["events_equal_a_b"] and v["forms"] == [2, 3] for v in verdicts)),
                  rule="on only if form 3 is faster than form 2 on both geometries by more than the spread of the repeats, with equal event counts")
    print(json.dumps(switch), flush=True)
    lines.append(switch)
    if out:
        with open(out, "w") as fp:
            json.dump(lines, fp, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
