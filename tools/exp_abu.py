#!/usr/bin/env python3
"""Time the brick-local walk with per-cell opacities (soc_set_tuning abu_local=1, soc_lbrick_pass_abu) next to the sweep such launches
took before it (abu_local=0: the hierarchy and OPT read from global memory, form 2) and next to the same launches with scalar opacities
on the brick-local walk (form 3), on the config-3 geometry: synth.octree_cloud(256, levels=4, frac=0.10, seed=1234) with two dust
species of variable abundance.

    python tools/exp_abu.py [--small] [--freqs 3] [--repeats 3] [--global0 1048576] [--out profiles/abu_local_lines.json]

One set of launches -- a point source, the isotropic background and cell emission at each of --freqs frequencies, every frequency with
opacities of its own -- is handed to the engine as one batch (soc_batch_begin / soc_batch_end, TABS only).  After a warm-up of every
variant the three are timed in turn, --repeats times round (a, b, c, a, b, c, ...), in one process.  Prints one JSON line per variant:
packets/s and cell steps/s (median, and the spread (max - min) / median over the repeats), the form that ran, the event counts -- and
a last line with the verdict: (b) faster than (a) by more than the larger of the two spreads, the event counts of (a) and (b) equal.
--small: octree_cloud(104, levels=4) and short launches, to try the tool.  Needs a GPU.
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


def commit():
    try:
        return subprocess.run(["git", "-C", REPO, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def launches(eng, cloud, freqs, small, G0, ABU, scalar):
    """the batch: per frequency (own opacities) a point-source, a background and a cell-emission launch"""
    n = cloud.NX
    ps = np.array([[0.501 * n, 0.501 * n, 0.501 * n]], np.float32)
    emit = np.where(cloud.DENS > 0, cloud.DENS * 1e-3, 0).astype(np.float32)
    bg_items = 8 * cloud.AREA
    eng.set_emission(emit, None)                                  # (once: the cell-emission launches share the copy)
    eng.batch_begin(0)
    for f in range(freqs):
        a = (2e-6 * (1 + 0.3 * f), 1e-6 * (1 + 0.2 * f))          # cross sections of the two species
        s = (2e-5 * (1 + 0.1 * f), 1e-5 * (1 + 0.4 * f))
        if scalar:
            eng.set_optical(0.6 * a[0] + 0.6 * a[1], 0.6 * s[0] + 0.6 * s[1])      # (the mean abundance of both species is 0.6)
        else:
            eng.set_optical_abu(a, s)
        seed = 0.2 + 0.013 * f
        eng.sim_pb(0, 0, 2 if small else 64, seed, 0.0, 1.0, PSPOS=ps, PS=[1.0 + f], GLOBAL=G0)
        eng.sim_pb(1, 0, 1 if small else 8, seed + 0.1, 1.0 + f, 1.0, GLOBAL=bg_items)
        eng.sim_cl(2, 0, 1, seed + 0.2, 1.0, G0 if small else 4 * G0)
    eng.batch_end()
    eng.sync()


def main(argv):
    def arg(name, default):
        return type(default)(argv[argv.index(name) + 1]) if name in argv else default
    small = "--small" in argv
    freqs, repeats, G0 = arg("--freqs", 3), arg("--repeats", 3), arg("--global0", 65536 if small else 1048576)
    out = arg("--out", "")
    cloud = synth.octree_cloud(104, levels=4, frac=0.08, seed=3) if small else synth.octree_cloud(256, levels=4, frac=0.10, seed=1234)
    model = "octree_cloud(104, levels=4)" if small else "config 3: octree_cloud(256, levels=4, frac=0.10, seed=1234)"
    ABU = np.random.default_rng(7).uniform(0.2, 1.0, (cloud.CELLS, 2)).astype(np.float32)
    _, csc = synth.hg_scattering_table(0.6)
    eng = Engine(0)
    variants = (("a", "abu_local=0: per-cell opacities, hierarchy and OPT in global memory", 0, False),
                ("b", "abu_local=1: per-cell opacities, brick-local walk", 1, False),
                ("c", "scalar opacities, brick-local walk (context)", 0, True))
    res = {k: dict(ms=[], stats=None, form=None, variant=None) for k, _, _, _ in variants}
    try:
        eng.set_cloud(cloud)
        eng.set_features(0, 0, 0)
        eng.set_scatter_table(None, csc)
        eng.set_optical(2e-6, 2e-5)
        eng.set_exec(1, 4)
        eng.set_abundances(ABU)
        for rnd in range(repeats + 1):                             # round 0 warms up: brick tables, buffers, clocks
            for key, _, local, scalar in variants:
                eng.set_tuning(abu_local=local)
                if scalar:
                    eng.set_opt(None)
                # (bricks are kept for one size: 4352 cells with per-cell opacities, 8704 with scalars -- a small launch of the variant's
                # kind rebuilds the tables before the clock starts)
                if scalar:
                    eng.set_optical(2e-6, 2e-5)
                else:
                    eng.set_optical_abu((2e-6, 1e-6), (2e-5, 1e-5))
                eng.sim_pb(1, 0, 1, 0.5, 1.0, 1.0, GLOBAL=8 * cloud.AREA, gid_first=0, gid_count=4096)
                eng.sync()
                eng.zero(0)
                eng.stats(reset=True)
                eng.timer_start()
                launches(eng, cloud, freqs, small, G0, ABU, scalar)
                ms = eng.timer_stop()
                st = eng.stats()
                r = res[key]
                r["form"], r["variant"] = eng.last_form(), eng.last_variant()
                if rnd > 0:
                    r["ms"].append(ms)
                    assert r["stats"] is None or r["stats"] == st, "the event counts of a variant changed between repeats"
                    r["stats"] = st
    finally:
        eng.set_tuning(abu_local=0)
        eng.close()
    lines = []
    for key, text, local, scalar in variants:
        r = res[key]
        ms = np.asarray(r["ms"])
        med = float(np.median(ms))
        lines.append(dict(variant=key, what=text, model=model, cells=int(cloud.CELLS), launches=3 * freqs, frequencies=freqs, form=r["form"],
                          kernel=r["variant"], ms=[float(x) for x in ms], ms_median=med, spread=float((ms.max() - ms.min()) / med),
                          packets=r["stats"]["packets"], tally_events=r["stats"]["tally_events"], scatterings=r["stats"]["scatterings"],
                          packets_per_s=r["stats"]["packets"] / (1e-3 * med), cell_steps_per_s=r["stats"]["tally_events"] / (1e-3 * med),
                          commit=commit()))
        print(json.dumps(lines[-1]))
    a, b = lines[0], lines[1]
    spread = max(a["spread"], b["spread"])
    gain = a["ms_median"] / b["ms_median"] - 1.0
    verdict = dict(verdict=True, b_over_a_speedup=a["ms_median"] / b["ms_median"], gain=gain, spread_of_the_call=spread,
                   b_faster_than_a_beyond_spread=bool(gain > spread),
                   events_equal_a_b=bool(all(a[k] == b[k] for k in ("packets", "tally_events", "scatterings"))), commit=commit())
    print(json.dumps(verdict))
    lines.append(verdict)
    if out:
        with open(out, "w") as fp:
            json.dump(lines, fp, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
