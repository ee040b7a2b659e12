"""Every compiled absorption kernel variant the dispatch rules can reach, run once against the oracle.

The host picks one of about a hundred kernels per launch or sweep: the direct kernels (SOC_DISPATCH, soc_kernels.hip), the sweeps of
Cartesian grids and of hierarchies in global memory (soc_brick_pass_fns) and the brick-local sweep (soc_lbrick_pass_fns, _ali_fns).
soc_last_variant names the one that ran.  REACHABLE lists what the rules can produce, CASES holds one small run per entry; each
asserts the variant, tally events equal to the oracle's (packets and scatterings equal to the direct kernels' for the sweeps: the
oracle counts only tally events) and every tally the variant writes equal to the oracle's to fp32 summation order.  The scenarios
at the end are where the variants meet: INT tallies shared by launches of one frequency, groups with differing TW, the brick
tables rebuilt between sweeps of the two brick sizes."""
import numpy as np
import pytest

import cases
from oracle_engine import OracleEngine
from soc_amd import synth
from soc_amd.lib import SocError
from util import assert_tally_close

pytestmark = pytest.mark.gpu

FIELDS = ("form", "kind", "wint", "octree", "dbl", "abu", "ali")       # the fields of Engine.last_variant() a key lists
PB, HP, CL = 0, 1, 2                                                    # the kernels: SimRAM_PB, _HP, _CL (a sweep's KIND 0-2 too)

# ---- what the dispatch rules can produce (soc_capi.hip route_sim / flush_pending, soc_brick.hip plan_sweep / plan_kernel) ----
CLOUDS = ((0, 0), (1, 0), (1, 1))                                       # (octree, dbl): Cartesian, hierarchy with float / double Index()
REACHABLE = set()
# direct kernels: every kernel x grid x opacities x INT tally (exec mode 0 takes any launch there).
#   excluded: dbl without octree -- a Cartesian grid's Index() has no double arithmetic, the wrappers take the float kernels
REACHABLE |= {(0, k, w, o, d, a, 0) for k in (PB, HP, CL) for (o, d) in CLOUDS for a in (0, 1) for w in (0, 1)}
# sweeps of Cartesian grids (form 1) and of hierarchies read from global memory (form 2): KIND 0-3 x opacities x INT tally.
#   excluded: KIND 4 -- launches of several kinds share a sweep on brick-local hierarchies only (same_sweep);
#             WINT 2 -- with_int 2 needs the brick-local sweep (route_sim), elsewhere it runs direct; WINT 3 -- the INT-only form is brick-local;
#             ALI -- a cell-emission launch with XAB is swept on brick-local hierarchies only; dbl on Cartesian grids -- as above
REACHABLE |= {(f, k, w, o, d, a, 0) for (f, o, d) in ((1, 0, 0), (2, 1, 0), (2, 1, 1)) for k in range(4) for a in (0, 1) for w in (0, 1)}
# brick-local sweep (form 3): WINT 0-3 x KIND 0-4, and the ALI kernels with and without the INT tally.
#   excluded: per-cell opacities -- they keep the global-tree form (soc_brick_local); ALI with another KIND -- ALI needs every launch to be
#             CL with one XAB; ALI with WINT 2 -- route_sim keeps with_int 2 from it; ALI with WINT 3 -- ALI turns the INT-only form off
REACHABLE |= {(3, k, w, 1, 1, 0, 0) for w in range(4) for k in range(5)} | {(3, CL, w, 1, 1, 0, 1) for w in (0, 1)}

# ---- clouds, inputs ----
_CLOUD = {}


def _cloud(name):
    if name not in _CLOUD:
        _CLOUD[name] = {"cart": lambda: synth.cartesian_cloud(40, seed=21),
                        "oct": lambda: synth.octree_cloud(40, levels=3, frac=0.1, seed=3),
                        "c104": lambda: synth.octree_cloud(104, levels=4, frac=0.08, seed=3)}[name]()
    return _CLOUD[name]


def _opt(cl):
    if ("opt", cl.CELLS) not in _CLOUD:
        rr = np.random.default_rng(11)
        opt = np.zeros((cl.CELLS, 2), np.float32)
        opt[:, 0] = 3e-6 * rr.uniform(0.5, 2, cl.CELLS)
        opt[:, 1] = 3e-5 * rr.uniform(0.5, 2, cl.CELLS)
        _CLOUD[("opt", cl.CELLS)] = opt
    return _CLOUD[("opt", cl.CELLS)]


def _emit(cl):
    return np.where(cl.DENS > 0, cl.DENS * 1e-3, 1e-4).astype(np.float32)


_SKY = cases.hp_sky(weighted=True)


def L(kind, seed, tw=1.0, f=1.0):
    """one launch: kind ps / bg / hp / cl, its seed, TW, and a factor on the opacities (another 'frequency')"""
    return dict(kind=kind, seed=seed, tw=tw, f=f)


def _launch(e, cl, spec, la):
    f = la["f"]
    if spec.get("abu"):
        e.set_opt(_opt(cl) * np.float32(f))
    else:
        e.set_optical(3e-6 * f, 3e-5 * f)
    small = cl.NX < 100
    k = la["kind"]
    if k == "ps":
        ps = np.array([[0.51 * cl.NX + 0.3, 0.49 * cl.NY + 0.2, 0.5 * cl.NZ + 0.1]], np.float32)
        e.sim_pb(0, 0, 8, la["seed"], 1.0, la["tw"], PSPOS=ps, PS=[1.0 + f], GLOBAL=256)
    elif k == "bg":
        g0 = 1000 if small else 100000
        e.sim_pb(1, 0, 2, la["seed"], 1.5, la["tw"], GLOBAL=8 * cl.AREA, gid_first=g0, gid_count=2000)
    elif k == "hp":
        e.set_hpbg(*_SKY)
        e.sim_hp(0, 2, la["seed"], la["tw"], 2048)
    else:
        e.set_emission(_emit(cl) * np.float32(f), None)
        g0, n = (1000, 256) if small else (4000, 32)
        e.sim_cl(2, 0, 1, la["seed"], la["tw"], 8192, gid_first=g0, gid_count=n)


_BEGIN = {"plain": "batch_begin", "int": "batch_begin_int", "shared": "batch_begin_shared_int", "groups": "batch_begin_int_groups"}


def _drive(e, spec):
    """Run one case on an engine (the HIP one, the oracle, or the HIP one forced to the direct kernels); returns (stats, tallies)."""
    cl = _cloud(spec["cloud"])
    e.set_cloud(cl)
    e.set_features(spec.get("with_int", 0), 0, 0)
    e.set_scatter_table(None, cases._CSC)
    e.set_opt(None)
    e.set_optical(3e-6, 3e-5)
    e.set_exec(spec["exec"], 4)
    e.set_tuning(**spec.get("tune", {}))
    e.set_ali(spec.get("ali", 0))
    e.zero(0)
    e.zero(1)
    e.stats(reset=True)
    batch = spec.get("batch")
    groups = spec["launches"] if batch == "groups" else [spec["launches"]]
    if batch:
        getattr(e, _BEGIN[batch])(0)
    for g in groups:
        if batch == "groups":
            e.batch_next_int()
        for la in g:
            _launch(e, cl, spec, la)
    if batch:
        e.batch_end()
    st = e.stats()
    out = {"tabs": e.read_tally(0)}
    if spec.get("with_int"):
        if batch in ("int", "groups"):                    # an INT array per launch, or per group
            for k in range(len(spec["launches"])):
                out["int%d" % k] = e.batch_read_int(k)
        else:
            out["int"] = e.read_tally(1)
    if spec.get("with_int") == 2:
        out["intv"] = np.stack([e.read_tally(3 + k) for k in range(3)])
    if spec.get("ali"):
        out["xab"] = e.read_tally(2)
    return st, out


class _Oracle(OracleEngine):
    """the oracle behind the Engine calls a case makes: execution knobs do nothing, a shared-INT batch runs its launches at once"""
    threads = 8

    def set_exec(self, mode=-1, brick_log2=4):
        pass

    def set_tuning(self, **kw):
        pass

    def batch_begin_shared_int(self, max_launches=0):
        self.batch_begin(max_launches)

    def stats(self, reset=False):
        if reset:
            self.events = 0
        return dict(tally_events=self.events)


class _Direct:
    """the HIP engine with every launch on the direct kernels: the witness of packet and scattering counts"""

    def __init__(self, e):
        self._e = e

    def __getattr__(self, name):
        return getattr(self._e, name)

    def set_exec(self, mode=-1, brick_log2=4):
        self._e.set_exec(0, brick_log2)


def _reset(e):
    e.set_features(0, 0, 0)
    e.set_ali(0)
    e.set_opt(None)
    e.set_exec(-1, 4)
    e.set_tuning(general_kernel=0, global_tree=0)


def _key(v):
    assert v is not None and v["rays"] == 0
    return tuple(v[f] for f in FIELDS)


def _compare(got, want):
    """every tally to fp32 summation order, cell by cell and as a float64 total; the signed vector sums INTX/Y/Z against INT"""
    assert set(got) == set(want)
    for name, w in want.items():
        g = got[name]
        if name == "intv":
            I = want["int"]
            assert np.abs(w).sum() > 0
            for k in range(3):
                assert np.all(np.abs(g[k] - w[k]) <= 1e-5 * np.maximum(I, 1e-3 * I.max())), "INTV[%d]" % k
                assert abs(g[k].sum(dtype=np.float64) - w[k].sum(dtype=np.float64)) <= 1e-5 * I.sum(dtype=np.float64)
            continue
        assert w.sum() > 0, "%s: the oracle tallied nothing" % name
        assert_tally_close(g, w, rtol=1e-5)
        tg, tw = g.sum(dtype=np.float64), w.sum(dtype=np.float64)
        assert abs(tg - tw) <= 1e-5 * abs(tw), "%s total %.9e vs %.9e" % (name, tg, tw)


def _check(engine, spec, key=None):
    """run `spec` on the GPU and on the oracle; the variant is `key` (if given).  Returns the variant that ran."""
    want_st, want = _drive(_Oracle(), spec)
    try:
        st, got = _drive(engine, spec)
        v = engine.last_variant()
        if key is not None:
            assert _key(v) == key, "ran %s, expected %s" % (_key(v), key)
        assert st["tally_events"] == want_st["tally_events"], "trajectories diverged from the oracle"
        _compare(got, want)
        if not spec.get("with_int"):
            assert not engine.read_tally(1).any(), "a TABS-only kernel wrote INT"
        if v["form"] != 0:
            wst, _ = _drive(_Direct(engine), spec)
            assert engine.last_variant()["form"] == 0
            assert st == wst, "the sweep and the direct kernels ran different packets: %s vs %s" % (st, wst)
    finally:
        _reset(engine)
    return v


# ---- one case per reachable variant ----
_LONE = {"ps": [L("ps", 0.21)], "bg": [L("bg", 0.377, 1.2)], "hp": [L("hp", 0.11, 0.8)], "cl": [L("cl", 0.9, 1.3)]}
_KIND_OF = {0: "ps", 1: "hp", 2: "cl", 3: "bg"}
CASES = {}

for o, d in CLOUDS:                                       # direct kernels: one lone launch each
    for k in (PB, HP, CL):
        for a in (0, 1):
            for w in (0, 1):
                cloud = "cart" if not o else ("c104" if d else "oct")
                kn = ("ps" if (a + w) % 2 else "bg") if k == PB else ("hp" if k == HP else "cl")   # (point sources on half the PB cases)
                CASES[(0, k, w, o, d, a, 0)] = dict(cloud=cloud, exec=0, with_int=w, abu=a, launches=_LONE[kn])

for f, o, d, cloud in ((1, 0, 0, "cart"), (2, 1, 0, "oct"), (2, 1, 1, "c104")):     # the two older sweeps: one lone launch each
    for k in range(4):
        for a in (0, 1):
            for w in (0, 1):
                tune = {}
                kn = _KIND_OF[k]
                if k == 0 and f == 2:
                    kn, tune = "bg", dict(general_kernel=1)       # background packets on the general kernel
                if d and not a:
                    tune = dict(tune, global_tree=1)              # a brick-local hierarchy walked in global memory
                CASES[(f, k, w, o, d, a, 0)] = dict(cloud=cloud, exec=1, with_int=w, abu=a, tune=tune, launches=_LONE[kn])

_TWO = {k: [L(_KIND_OF[k], 0.31, 1.0, 1.0), L(_KIND_OF[k], 0.57, 0.6, 1.7)] for k in range(4)}
_MIX = [L("ps", 0.31, 1.0, 1.0), L("bg", 0.57, 0.6, 1.7), L("cl", 0.73, 1.4, 0.8)]     # (point sources and background alone: both KIND 0)
for k in range(5):                                        # brick-local sweep
    mixed = k == 4
    # WINT 0: TABS only (several kinds: one soc_batch_begin sweep)
    CASES[(3, k, 0, 1, 1, 0, 0)] = dict(cloud="c104", exec=1, launches=_MIX, batch="plain") if mixed else \
        dict(cloud="c104", exec=1, launches=_LONE[_KIND_OF[k]])
    # WINT 1: one INT array shared by launches with different TW (soc_batch_begin_shared_int)
    CASES[(3, k, 1, 1, 1, 0, 0)] = dict(cloud="c104", exec=1, with_int=1, batch="shared",
                                        launches=[L("hp", 0.31, 1.0, 1.0), L("bg", 0.57, 0.6, 1.7)] if mixed else _TWO[k])
    # WINT 2: INT and INTX/Y/Z (several kinds: deferred together, only soc_batch_begin_shared_int allows it)
    CASES[(3, k, 2, 1, 1, 0, 0)] = dict(cloud="c104", exec=1, with_int=2, batch="shared", launches=_MIX) if mixed else \
        dict(cloud="c104", exec=1, with_int=2, launches=_LONE[_KIND_OF[k]])
    # WINT 3: the INT-only form, an INT array per launch, two launches with different TW (TABS = TW x INT at the flush)
    CASES[(3, k, 3, 1, 1, 0, 0)] = dict(cloud="c104", exec=1, with_int=1, batch="int",
                                        launches=[L("hp", 0.31, 1.0, 1.0), L("cl", 0.57, 0.6, 1.7)] if mixed else _TWO[k])
for w in (0, 1):                                          # ALI: a cell-emission launch with the XAB tally
    CASES[(3, CL, w, 1, 1, 0, 1)] = dict(cloud="c104", exec=1, with_int=w, ali=1, launches=_LONE["cl"])


def _id(key):
    return "form%d-kind%d-wint%d-oct%d-dbl%d-abu%d-ali%d" % key


def test_every_reachable_variant_has_a_case():
    assert set(CASES) == REACHABLE
    assert len(REACHABLE) == 36 + 48 + 22


@pytest.mark.parametrize("key", sorted(CASES), ids=_id)
def test_variant_against_the_oracle(key, engine):
    _check(engine, CASES[key], key)


# ---- where the variants meet ----

def test_shared_int_alternating_brick_sizes(engine):
    """a. point-source, background and cell-emission launches of one frequency in one soc_batch_begin_shared_int sweep, three times:
    equal TW (the INT-only form, 8704-cell bricks), one TW changed (INT beside TABS, 5888-cell bricks), equal TW again -- the brick
    tables are rebuilt in both directions.  The INT of all three launches is read with read_tally(1); there is no per-launch INT."""
    for tws, wint in (((1.0, 1.0, 1.0), 3), ((1.0, 1.0, 1.6), 1), ((0.7, 0.7, 0.7), 3)):
        spec = dict(cloud="c104", exec=1, with_int=1, batch="shared",
                    launches=[L("ps", 0.31, tws[0], 1.0), L("bg", 0.57, tws[1], 1.0), L("cl", 0.73, tws[2], 1.0)])
        _check(engine, spec, (3, 4, wint, 1, 1, 0, 0))
    with pytest.raises(SocError):
        engine.batch_read_int(0)
    _reset(engine)


def test_int_groups_with_differing_tw_in_a_later_group(engine):
    """b. soc_batch_begin_int_groups on a brick-local hierarchy: the second group's two launches differ in TW, so the whole sweep keeps
    INT beside TABS (WINT 1), brick queues per group; every group's INT and the shared TABS equal the oracle's"""
    spec = dict(cloud="c104", exec=1, with_int=1, batch="groups",
                launches=[[L("ps", 0.31, 1.0, 1.0), L("bg", 0.57, 1.0, 1.0)],
                          [L("bg", 0.43, 0.7, 1.5), L("cl", 0.61, 1.3, 1.5)],
                          [L("hp", 0.29, 1.1, 0.7)]])
    _check(engine, spec, (3, 4, 1, 1, 1, 0, 0))


def test_shared_int_across_kind_changes_on_a_global_tree(engine):
    """c. soc_batch_begin_shared_int on a hierarchy of the global-tree form: background launches, then a cell-emission launch -- the change
    of kind runs what is pending first, both sweeps tally into the one INT array, the tally events add up"""
    spec = dict(cloud="oct", exec=1, with_int=1, batch="shared",
                launches=[L("bg", 0.31, 1.0, 1.0), L("bg", 0.57, 0.6, 1.7), L("cl", 0.73, 1.4, 0.8)])
    _check(engine, spec, (2, CL, 1, 1, 0, 0, 0))


def test_shared_int_with_intensity_vectors(engine):
    """d. with_int 2 deferred into one sweep (only soc_batch_begin_shared_int allows it): launches of three kinds, INT and INTX/Y/Z"""
    spec = dict(cloud="c104", exec=1, with_int=2, batch="shared",
                launches=[L("hp", 0.31, 1.0, 1.0), L("cl", 0.57, 0.6, 1.7), L("bg", 0.73, 1.4, 0.8)])
    _check(engine, spec, (3, 4, 2, 1, 1, 0, 0))
