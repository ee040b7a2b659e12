"""The cases of packet splitting with a Healpix sky (`split 1` + `hpbg`, SimHpSplit) of tests/golden/hpsplit.npz: skies, models
and launches.  Shared by the tests and by tools/make_hpsplit_golden.py, which records what the reference's kernel gives for
them, work item by work item in id order.  The models are those of split_cases.py; a launch has GLOBAL 96 work items (one
and a half waves) of BATCH 2-6 root rays, the x104 cases -- the hierarchy whose Index() runs in double -- 1024 work items.

The skies are generated here from a seed and not stored: a smooth dipole times log-normal noise, strictly positive; the
weighted inputs (sky x pixel weight, cumulative probability) come through files.hpbg_for_frequency as in a run.

Together the cases reach (coverage() is asserted over the restatement's counters before anything is recorded):
  an initial split (oct4b), a jump over two or more levels (kat), the stop after more than 20 scatterings (oct4b_opaque),
  rays ending below their RL, rays dropped with their stack (nest5_ms16), splits skipped on a nearly full stack and drops
  (jump3_ms17, see jump3_cloud), replicas of a two-level jump that do not fit (kat_ms14), an unweighted and a weighted sky, the variants abu, abuh, msf, int2; no 30000-step
  return; and no root ray born too deep for its stack (guard == 0: the reference would write past its slab).
"""
import json

import numpy as np

from soc_amd import files, synth
from oracle.pyoracle import Job

import split_cases as sc

GLOBAL = 96
COUNTERS = sc.COUNTERS


def case(model, BATCH, max_split=64, SEED=0.5, ABS=1e-4, SCA=3e-4, variant="scalar", TW=1.0, weighted=0, sky=1, scale=1.0, GLOBAL=GLOBAL):
    return dict(model=model, BATCH=BATCH, max_split=max_split, SEED=SEED, ABS=ABS, SCA=SCA, variant=variant, TW=TW,
                weighted=weighted, sky=sky, scale=scale, GLOBAL=GLOBAL)


CASES = {
    "kat":          case("kat", 4, SEED=0.4137, ABS=1e-3, SCA=3e-3),
    "kat_w_int2":   case("kat", 3, SEED=0.77, ABS=1e-3, SCA=3e-3, variant="int2", TW=2.5, weighted=1, sky=2),
    "kat_ms14":     case("kat", 6, max_split=14, SEED=0.2718, ABS=1e-3, SCA=3e-3),
    "oct4b":        case("oct4b", 3, SEED=0.2891),
    "oct4b_w":      case("oct4b", 3, SEED=0.5772, weighted=1, sky=3),
    "oct4b_opaque": case("oct4b", 2, SEED=0.611, ABS=1e-5, SCA=3e-2),
    "oct4b_abu":    case("oct4b", 2, SEED=0.35, variant="abu", scale=3.0),
    "oct4b_abuh":   case("oct4b", 2, SEED=0.35, variant="abuh", weighted=1, sky=2),
    "oct4b_msf":    case("oct4b", 3, SEED=0.93, variant="msf"),
    "nest5_ms16":   case("nest5", 6, max_split=16, SEED=0.1234),
    "jump3_ms17":   case("jump3", 6, max_split=17, SEED=0.3183),
    "oct6_w":       case("oct6", 2, SEED=0.8080, weighted=1, sky=3),
    "x104":         case("x104", 3, SEED=0.2891, GLOBAL=1024),
    "x104_w_int2":  case("x104", 3, SEED=0.2891, variant="int2", weighted=1, sky=2, GLOBAL=1024),
    "x104_abu":     case("x104", 3, SEED=0.2891, variant="abu", GLOBAL=1024),
}

_skies = {}
_jump3 = []


def jump3_cloud(seed=7):
    """4^3 root cells, four levels, refined in the interior only: root cell 21 -> all eight level-1 cells -> 64 level-2 cells, of
    which three in ten -> level 3.  With single-level jumps a stack never comes near full without dropping first (a split adds
    three entries net and NBUF > MAX_SPLIT-10 drops); a ray that steps from a root cell into this block jumps two levels or
    three and holds 15 entries, and a later step from level 2 to level 3 finds a stack too full to split (MAX_SPLIT 17: no split
    from NBUF 12 on, a drop at NBUF 8 to 11).  No boundary cell is refined, so no ray is born deep."""
    if not _jump3:
        rr = np.random.default_rng(seed)
        fine = np.sort(rr.choice(64, 19, replace=False))
        H = [np.clip(np.exp(0.3 * rr.standard_normal(n)) * 1.0e3, 1.0, 1.0e5).astype(np.float32) for n in (64, 8, 64, 8 * len(fine))]
        H[0][21] = -synth.I2F(0)
        for j in range(8):
            H[1][j] = -synth.I2F(8 * j)
        for k, cell in enumerate(fine):
            H[2][cell] = -synth.I2F(8 * k)
        _jump3.append(synth.Cloud(4, 4, 4, H))
    return _jump3[0]


def model(name):
    return jump3_cloud() if name == "jump3" else sc.model(name)


def sky(seed):
    """[49152] float32, strictly positive: (1 + 0.6 cos(angle to an axis drawn from the seed)) x log-normal noise of 0.5 dex.  The
    pixel order does not matter to the kernel, so the dipole is laid over the pixel index as over a latitude."""
    if seed not in _skies:
        rr = np.random.default_rng(1000 + seed)
        mu = np.cos(np.pi * (np.arange(49152) + 0.5) / 49152.0 + rr.uniform(0.0, np.pi))
        _skies[seed] = ((1.0 + 0.6 * mu) * np.exp(0.5 * np.log(10.0) * rr.standard_normal(49152))).astype(np.float32)
    return _skies[seed]


def sky_inputs(name):
    """(HPBG, HPBGP or None) of a case, as a run uploads them"""
    k = CASES[name]
    return files.hpbg_for_frequency(sky(k["sky"]), k["scale"], k["weighted"])


def job(name):
    """(Job, max_split) of a case; Job.GLOBAL is the number of work items launched"""
    k = CASES[name]
    c = model(k["model"])
    HPBG, HPBGP = sky_inputs(name)
    kw = dict(ABS=k["ABS"], SCA=k["SCA"], SOURCE=1, BATCH=k["BATCH"], SEED=k["SEED"], BG=0.0, TW=k["TW"], GLOBAL=k["GLOBAL"], WITH_INT=1,
              HPBG=HPBG, HPBGP=HPBGP)
    v = k["variant"]
    if v == "abu":
        kw["OPT"] = sc.per_cell_opt(c, k["ABS"], k["SCA"])
    elif v == "abuh":
        kw["OPT"] = sc.per_cell_opt(c, k["ABS"], k["SCA"]).astype(np.float16).astype(np.float32)
    elif v == "msf":
        kw.update(sc.msf_inputs(c, k["ABS"], k["SCA"]))
    elif v == "int2":
        kw["WITH_INT"] = 2
    return Job(c, sc._CSC, **kw), k["max_split"]


WANT = {"kat": "deep_splits", "oct4b": "initial", "oct4b_opaque": "stop20", "nest5_ms16": "overflow_drops",
        "jump3_ms17": ("skipped_splits", "overflow_drops"), "kat_ms14": "skipped_replicas"}


def coverage(stats_by_case):
    """What the cases must reach.  stats_by_case: {name: the restatement's stats}.  Returns a list of failures."""
    bad = []
    total = {k: sum(int(s[k]) for s in stats_by_case.values()) for k in COUNTERS + ("skipped_splits", "skipped_replicas", "initial", "stop20")}
    for k in total:
        if k != "long_returns" and total[k] < 1:
            bad.append("no case reaches '%s'" % k)
    if total["long_returns"] != 0:
        bad.append("%d work items returned at 30000 steps" % total["long_returns"])
    for name, s in stats_by_case.items():
        if int(s["guard"]) != 0:
            bad.append("%s: %d root rays born too deep for the stack (the reference writes past its slab)" % (name, int(s["guard"])))
        if int(s["roots"]) != CASES[name]["GLOBAL"] * CASES[name]["BATCH"]:
            bad.append("%s: %d root rays for %d work items x %d" % (name, int(s["roots"]), CASES[name]["GLOBAL"], CASES[name]["BATCH"]))
    for name, keys in WANT.items():
        for key in ((keys,) if isinstance(keys, str) else keys):
            if name in stats_by_case and int(stats_by_case[name][key]) < 1:
                bad.append("%s does not reach '%s'" % (name, key))
    if "x104" in stats_by_case and int(stats_by_case["x104"]["splits"]) < 500:     # the double-Index() case: see split_cases.coverage
        bad.append("x104 reaches 'splits' %d times, not 500" % int(stats_by_case["x104"]["splits"]))
    if {CASES[n]["weighted"] for n in stats_by_case} != {0, 1}:
        bad.append("an unweighted and a weighted sky")
    if not {"abu", "abuh", "msf", "int2"} <= {CASES[n]["variant"] for n in stats_by_case}:
        bad.append("the variants abu, abuh, msf, int2")
    return bad


def meta():
    return json.dumps(dict(cases=CASES, GLOBAL=GLOBAL))
