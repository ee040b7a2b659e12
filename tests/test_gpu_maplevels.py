"""soc_map_block_levels on the device (`maplevels 1`): the planes MAPL[f][l] of the resident batch are, bit for bit, what the
per-frequency kernel (Engine.map) gives for frequency f when the emission of every cell not on hierarchy level l is set to zero --
the definition of the product, computed once per case by the kernels of the plain map, never by the code under test.  Every
bitwise comparison is of uint32 views over all pixels."""
import os

import numpy as np
import pytest

from maplevels_engine import LevelsOracleEngine, masked_emission
from oracle.pyoracle import NO_INTOBS
from soc_amd import files, launch, lib as soclib, synth
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User
from test_gpu_fastmap import ABS0, SCA0, Case, _factors, _reset, _same
from test_host import _write_model
from test_maps import DE, LENGTH, MAP_CASES, N, OD, RA, _opt

pytestmark = pytest.mark.gpu

CASES = ["map_oct8", "map_oct8_inside", "map_oct8_healpix", "map_oct8_roimap", "map_oct8_threshold", "map_oct8_mapint1", "map_oct8_mapint2",
         "map_oct8_mapint1_inside", "map_oct104_double", "map_oct104_mapint2_double", "map_c8_abu", "map_oct8_mapint2+abu",
         # grids whose three sides differ (synth.NONCUBIC)
         "map_r759", "map_oct759", "map_oct759_inside", "map_oct759_mapint2", "map_oct759_mapint2+abu", "map_oct759_threshold",
         "map_oct759_healpix5", "map_oct104x6x5", "map_oct104x6x5_mapint1", "map_oct104x6x5_abu", "map_oct6x104x5", "map_oct6x104x5_mapint2",
         "map_oct6x104x5_inside", "map_oct5x6x104_mapint1", "map_r208x6x5", "map_r6x208x5"]
# (not map_oct104x6x5_mapint2 and map_oct5x6x104_mapint2: with `mapint 2` along 104 cells the CPU oracle's own fp32 sum along the ray and
# the sum of its per-level sums are 2.09e-6 and 1.88e-6 apart, at the 2e-6 of LCase.check, which was sized on rays of 8 root cells;
# tests/test_gpu_fastmap.py and tests/test_maps.py have those two cases against the per-frequency kernel and the oracle)
# which planes the definition lights in view 0 (found with the CPU oracle in soc mode); the others are dark
LIT = {"map_oct8": [0, 1, 2], "map_oct8_mapint2": [0, 1, 2], "map_oct8_roimap": [0, 1, 2], "map_oct8_healpix": [0, 1, 2],
       "map_oct8_inside": [0, 1, 2], "map_oct8_threshold": [1, 2], "map_oct104_double": [0, 1],
       "map_oct759": [0, 1, 2], "map_oct759_threshold": [1, 2], "map_oct759_healpix5": [0, 1, 2], "map_oct104x6x5": [0, 1],
       "map_oct6x104x5": [0, 1, 2], "map_oct5x6x104_mapint1": [0, 1, 2]}
DEEP = {6: 8648, 9: 120184}                                   # levels -> cells of synth.octree_cloud(4, levels, frac=0.3, seed=3)


class LCase(Case):
    """Case of tests/test_gpu_fastmap.py (the same inputs: opacity factors whose first two span both branches of the DTAU < 1e-3
    test, column 1 without emission) with the planes of the definition, made on demand, once, and kept unchanged.  `name+abu` is
    the case `name` with per-cell opacities; cloud / kw: a case that is not in MAP_CASES."""

    def __init__(self, name, engine, nmax, cloud=None, kw=None, views=None):
        if kw is None:
            _, mk, kw = MAP_CASES[name.split("+")[0]]
            kw = dict(kw, abu=True) if name.endswith("+abu") else kw
            cloud = mk()
        self.name, self.kw, self.cloud = name, kw, cloud
        c = self.cloud
        if nmax is None:                                       # one more than the widest kernel instance takes for this model
            engine.set_cloud(c)
            nmax = engine.map_block_levels_width + 1
        self.centre = (c.NX / 2, c.NY / 2, c.NZ / 2)
        self.views = views if views else (1 if kw.get("healpix") else N)
        fac = _factors(nmax)
        emit = np.where(c.DENS > 0, np.abs(c.DENS) * 1e-3 * np.random.default_rng(1).uniform(0.5, 2, c.CELLS), 0).astype(np.float32)
        self.EMITX = np.ascontiguousarray(emit[:, None] * np.linspace(0.5, 2.0, nmax, dtype=np.float32)[None, :], np.float32)
        if nmax > 1:
            self.EMITX[:, 1] = 0.0
        self.ABS, self.SCA = ABS0 * fac, SCA0 * fac
        self.OPTX = np.ascontiguousarray(_opt(c.CELLS)[:, None, :] * fac[None, :, None], np.float32) if kw.get("abu") else None
        self.nmax = nmax
        self._want = {}
        self.switch(engine)

    def want(self, engine, f, v):
        """[LEVELS, ...]: Engine.map of frequency f and view v on the emission masked per level"""
        if (f, v) not in self._want:
            engine.set_opt(None if self.OPTX is None else self.OPTX[:, f, :])
            planes = [engine.map(masked_emission(self.cloud, self.EMITX[:, f], l), *self.args(v), self.ABS[f], self.SCA[f],
                                 INTOBS=self.kw.get("intobs", NO_INTOBS), save_colden=0, LENGTH=LENGTH, healpix=self.kw.get("healpix", 0))[0]
                      for l in range(self.cloud.LEVELS)]
            engine.set_opt(None)
            self._want[(f, v)] = np.stack(planes)
            self._want[(f, v)].setflags(write=False)
        return self._want[(f, v)]

    def levels(self, engine, v):
        return engine.map_block_levels(*self.args(v), INTOBS=self.kw.get("intobs", NO_INTOBS), healpix=self.kw.get("healpix", 0))

    def check(self, engine, nf, views=None):
        """the planes of the resident batch of nf frequencies, every view: equal to the definition bit for bit; a pixel the plain
        map leaves at zero is zero on every plane; on every lit pixel the planes add up to the plain map within 2e-6 of it (four
        times the largest distance the CPU oracle shows between the fp32 sum along the ray and the float64 sum of the per-level
        fp32 sums: 5.2e-7).  Returns the lit pixels per plane of view 0, frequency 0."""
        lit0 = None
        for v in (range(self.views) if views is None else views):
            MAPL = self.levels(engine, v)
            MAPX = self.block(engine, v)[0]
            assert MAPL.shape == (nf, self.cloud.LEVELS) + MAPX.shape[1:] and MAPX.shape[0] == nf
            for f in range(nf):
                assert _same(MAPL[f], self.want(engine, f, v)), (self.name, nf, f, v)
                dark = MAPX[f] == 0
                assert not MAPL[f][:, dark].any(), (self.name, nf, f, v)
                total = MAPL[f].astype(np.float64).sum(axis=0)
                assert (np.abs(total - MAPX[f])[~dark] <= 2e-6 * MAPX[f][~dark]).all(), (self.name, nf, f, v)
            assert np.isfinite(MAPL).all()
            if nf > 1:
                assert not MAPL[1].any()                       # the frequency without emission
            if lit0 is None:
                lit0 = [int((MAPL[0, l] > 0).sum()) for l in range(self.cloud.LEVELS)]
        return lit0


@pytest.fixture(scope="module")
def cases(engine):
    made = {}

    def get(name):
        if name not in made:
            made[name] = LCase(name, engine, 32 if name == "map_oct8" else None)
        made[name].switch(engine)
        return made[name]
    yield get
    _reset(engine)


@pytest.mark.parametrize("name", CASES)
def test_planes_equal_the_masked_per_frequency_kernel(name, engine, cases):
    """widths 1 and 2; 3 after a full-width batch of NaN; one more than the widest kernel instance (two launches, the second a
    single column); for map_oct8 the widest batch (four launches).  With the conditions that keep this from passing on dark
    planes: every plane the definition lights has at least 5 lit pixels, and the planes it leaves dark are all zero bits."""
    case = cases(name)
    width = engine.map_block_levels_width
    assert width == 8 and engine.map_block_max == 32           # all these models have at most 8 levels
    for nf in [1, 2, 3, width + 1] + ([32] if name == "map_oct8" else []):
        if nf == 3:
            case.poison(engine)                                # nothing behind the third column may reach a plane
        case.upload(engine, nf)
        lit = case.check(engine, nf)
        for l, n in enumerate(lit):
            assert n == 0 or n >= 5, (name, nf, lit)
        if name in LIT:
            assert [l for l, n in enumerate(lit) if n] == LIT[name], (name, lit)
        else:
            assert lit[0] >= 5, (name, lit)
    if name == "map_oct8_threshold":                           # `threshold 1`: level 0 does not emit
        assert not case.want(engine, 0, 0)[0].view(np.uint32).any() and not case.levels(engine, 0)[:, 0].view(np.uint32).any()
    if name == "map_oct104_double":
        assert not case.levels(engine, 0)[:, 2].view(np.uint32).any()
    _reset(engine)


@pytest.mark.parametrize("name", ["map_c8_abu", "map_c8_mapint1"])
def test_cartesian_grid_has_one_plane_the_plain_map(name, engine, cases):
    case = cases(name)
    assert case.cloud.LEVELS == 1
    for nf in (1, 3):
        case.upload(engine, nf)
        for v in range(case.views):
            MAPL, MAPX = case.levels(engine, v), case.block(engine, v)[0]
            assert MAPL.shape[1] == 1 and _same(MAPL[:, 0], MAPX), (name, nf, v)
        assert (MAPL[0, 0] > 0).sum() > 30
        case.check(engine, nf)
    _reset(engine)


@pytest.mark.parametrize("levels", sorted(DEEP))
@pytest.mark.parametrize("mapint", [0, 2])
def test_deep_hierarchies(levels, mapint, engine):
    """more levels than a 4- or an 8-wide scheme holds, and the LDS sizing: 6 levels run 8 frequencies per launch, 9 levels 4"""
    cloud = synth.octree_cloud(4, levels=levels, frac=0.3, seed=3)
    assert cloud.LEVELS == levels and cloud.CELLS == DEEP[levels]
    case = LCase("deep%d" % levels, engine, 2, cloud=cloud, kw=dict(npix=(32, 24), dx=0.15, mapint=mapint), views=1)
    assert case.centre == (2, 2, 2) and engine.map_block_levels_width == (8 if levels <= 8 else 4)
    case.upload(engine, 2)
    lit = case.check(engine, 2)
    assert all(n >= 5 for n in lit), lit                       # every level is lit
    _reset(engine)


def test_wide_batch_on_nine_levels(engine):
    """9 levels: 4 frequencies per launch; 5 frequencies are two launches, the second a single column"""
    cloud = synth.octree_cloud(4, levels=9, frac=0.3, seed=3)
    case = LCase("deep9w", engine, 5, cloud=cloud, kw=dict(npix=(32, 24), dx=0.15), views=1)
    assert engine.map_block_levels_width == 4
    case.poison(engine)
    case.upload(engine, 5)
    case.check(engine, 5)
    _reset(engine)


@pytest.mark.parametrize("npix", [(96, 80), (97, 81)])
def test_more_than_one_workgroup_and_a_ragged_last_one(npix, engine):
    """96 x 80 pixels are 30 full workgroups; 97 x 81 are 30 and a last one of 177 lanes"""
    _, mk, kw = MAP_CASES["map_oct8"]
    case = LCase("map_oct8_%dx%d" % npix, engine, 2, cloud=mk(), kw=dict(kw, npix=npix, dx=0.12))
    assert npix[0] * npix[1] > 256 and ((npix[0] * npix[1]) % 256 != 0) == (npix == (97, 81))
    case.upload(engine, 2)
    lit = case.check(engine, 2)
    assert all(n >= 5 for n in lit), lit
    _reset(engine)


def test_a_batch_stays_resident_and_unchanged(engine, cases):
    case = cases("map_oct8")
    case.upload(engine, 3)                                     # once
    before = [case.block(engine, v) for v in range(case.views)]
    planes = [case.levels(engine, v) for v in range(case.views)]
    after = [case.block(engine, v) for v in range(case.views)]
    for v in range(case.views):
        assert all(_same(a, b) for a, b in zip(before[v], after[v])), v
        for f in range(3):
            assert _same(planes[v][f], case.want(engine, f, v)), (f, v)
    assert not _same(planes[0], planes[1])
    _reset(engine)


def test_argument_errors_leave_the_engine_usable(engine, cases):
    case = cases("map_oct8")
    engine.set_map_block(None)
    with pytest.raises(soclib.SocError, match="no batch is resident"):
        case.levels(engine, 0)
    case.upload(engine, 2)
    d, ra, de, npix, dx, centre = case.args(0)
    with pytest.raises(soclib.SocError, match="NPIX 0 x 10"):
        engine.map_block_levels(d, ra, de, (0, 10), dx, centre)
    with pytest.raises(soclib.SocError, match="observer position"):
        engine.map_block_levels(d, ra, de, npix, dx, centre, INTOBS=None, healpix=8)
    with pytest.raises(soclib.SocError, match="DIR, RA, DE, CENTRE and MAP_DX > 0 are needed"):
        engine.map_block_levels(None, ra, de, npix, dx, centre)
    case.check(engine, 2, views=[0])
    _reset(engine)


def test_ini_run_writes_the_level_file(tmp_path):
    """a map-only run with `maplevels 1` on the HIP engine: map_dir_00.bin and map_dir_00_L.bin against the helper engine of
    tests/test_maplevels.py (the soc-mode oracle on masked emission) fed with the emission and opacities of the run -- bit for bit,
    as tests/test_gpu_fastmap.py has the map kernels against that oracle.  The cloud is opaque, so a level is seen only where
    its cells lie at the surface: with a refined fraction of 0.3 the oracle lights 52 pixels of plane 0 and 28 of plane 1 at each
    of the three frequencies, 80 of the plain map (at 0.1 plane 1 has 6 pixels, too few for the check on dark planes below)"""
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.3, seed=9)
    files.write_temperature(os.path.join(d, "m.T"), cloud, np.asarray(np.random.default_rng(8).uniform(2500.0, 6000.0, cloud.CELLS), np.float32))
    extra = "iterations 0\nloadtemp\ntemperature %s/m.T\nemitted %s/m.emit\nmapping 12 10 0.8 2\ndirection 30 40\nmaplevels 1\n" % (d, d)
    ini = _write_model(d, cloud, extra=extra)
    txt = open(ini).read().replace("nosolve\n", "").replace("nomap\n", "").replace("absorbed %s/abs.data\n" % d, "")
    open(ini, "w").write(txt)
    os.chdir(d)
    hip = soclib.Engine(0)
    try:
        run = AbsorptionRun(User(ini), hip, verbose=0)
        run.run()
        opa = [run._optical_for(i) for i in range(3)]
    finally:
        hip.close()
    U = run.U
    KK = (1.0e23 / launch.FACTOR) * launch.PLANCK / (4.0 * np.pi) * (U.GL * launch.PARSEC)
    EMITTED = run.EMITTED
    helper = LevelsOracleEngine("soc")
    helper.set_cloud(cloud)
    EMITX = np.stack([np.asarray(KK * float(run.FFREQ[i]) * EMITTED[:, i], np.float32) for i in range(3)], axis=1)
    _, ODIR, RA_, DE_ = launch.set_observer_directions(U.OBS_THETA, U.OBS_PHI)
    view = (ODIR[0], RA_[0], DE_[0], U.NPIX, U.MAP_DX, (3.0, 3.0, 3.0))
    helper.set_map_block(EMITX, [a for a, _ in opa], [s for _, s in opa])
    MAPX = helper.map_block(*view, INTOBS=U.INTOBS)[0]
    MAPL = helper.map_block_levels(*view, INTOBS=U.INTOBS)
    assert list(np.fromfile("map_dir_00.bin", np.int32, 2)) == [12, 10]
    assert list(np.fromfile("map_dir_00_L.bin", np.int32, 4)) == [12, 10, 3, 2]
    got = np.fromfile("map_dir_00.bin", np.float32, offset=8).reshape(3, 10, 12)
    gotl = np.fromfile("map_dir_00_L.bin", np.float32, offset=16).reshape(3, 2, 10, 12)
    assert _same(got, MAPX) and _same(gotl, MAPL)
    assert ((gotl > 0).sum(axis=(0, 2, 3)) > 20).all() and (got > 0).sum() > 100
