"""soc_map_block on the device: the maps of a batch of frequencies from one walk per pixel are, plane by plane and bit by bit,
those of the per-frequency kernel (Engine.map) -- and, for two cases, of its CPU restatement (oracle_mapping, soc mode).
Every comparison is of uint32 views over all pixels."""
import os

import numpy as np
import pytest

from oracle.pyoracle import Job, NO_INTOBS, oracle_mapping
from soc_amd import files, lib as soclib
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User
from test_host import _write_model
from test_maps import CSC, DE, LENGTH, MAP_CASES, N, OD, RA, _opt

pytestmark = pytest.mark.gpu

CASES = ["map_oct8", "map_c8_abu", "map_oct8_inside", "map_oct8_healpix", "map_oct8_colden", "map_oct8_roimap", "map_oct8_threshold",
         "map_oct8_mapint1", "map_oct8_mapint2", "map_oct104_mapint2_double", "map_c208_entry",
         # grids whose three sides differ (synth.NONCUBIC)
         "map_r759", "map_oct759", "map_oct759_inside", "map_oct759_mapint1", "map_oct759_mapint2", "map_oct759_roimap", "map_oct759_threshold",
         "map_oct104x6x5", "map_oct104x6x5_inside", "map_oct104x6x5_mapint2", "map_oct104x6x5_abu", "map_oct6x104x5", "map_oct6x104x5_inside",
         "map_oct6x104x5_mapint2", "map_oct5x6x104", "map_oct5x6x104_mapint1", "map_r208x6x5", "map_r208x6x5_inside", "map_r6x208x5",
         "map_r6x208x5_inside"]
ABS0, SCA0 = np.float32(1e-3), np.float32(3e-3)               # the opacities of tests/test_maps.py::run_case


def _factors(nmax):
    """opacity factors of the frequencies of a batch: 1e-2 and 1e2 first, so that every batch of two or more spans both
    branches of the DTAU < 1e-3 test along the rays, the others spread between them"""
    rest = np.geomspace(1e-2, 1e2, nmax)[1:-1]
    return np.concatenate([[1e-2, 1e2], rest[np.random.default_rng(2).permutation(rest.size)]])[:nmax].astype(np.float32)


class Case:
    """one case of MAP_CASES with nmax frequencies: inputs, switches and -- computed once, never changed -- the planes of the
    per-frequency kernel for every view"""

    def __init__(self, name, engine, nmax):
        _, mk, kw = MAP_CASES[name]
        self.name, self.kw, self.cloud = name, kw, mk()
        c = self.cloud
        self.centre = (c.NX / 2, c.NY / 2, c.NZ / 2)
        self.views = 1 if kw.get("healpix") else N
        fac = _factors(nmax)
        emit = np.where(c.DENS > 0, np.abs(c.DENS) * 1e-3 * np.random.default_rng(1).uniform(0.5, 2, c.CELLS), 0).astype(np.float32)
        self.EMITX = np.ascontiguousarray(emit[:, None] * np.linspace(0.5, 2.0, nmax, dtype=np.float32)[None, :], np.float32)
        if nmax > 1:
            self.EMITX[:, 1] = 0.0                             # one frequency without emission
        self.ABS, self.SCA = ABS0 * fac, SCA0 * fac
        self.OPTX = np.ascontiguousarray(_opt(c.CELLS)[:, None, :] * fac[None, :, None], np.float32) if kw.get("abu") else None
        self.switch(engine)
        self.ref = [[self.per_frequency(engine, f, v) for v in range(self.views)] for f in range(nmax)]
        self.colden = [self.per_frequency(engine, 0, v, colden=1)[1] for v in range(self.views)]

    def switch(self, engine):
        engine.set_cloud(self.cloud)
        engine.set_opt(None)
        engine.set_map_threshold(self.kw.get("threshold", 0))
        engine.set_map_interpolation(self.kw.get("mapint", 0))
        engine.set_map_roi(self.kw.get("roi"))

    def args(self, v):
        kw = self.kw
        return (OD[v], RA[v], DE[v], kw.get("npix", (12, 10)), kw.get("dx", 0.9), self.centre)

    def per_frequency(self, engine, f, v, colden=0):
        engine.set_opt(None if self.OPTX is None else self.OPTX[:, f, :])
        m, t = engine.map(self.EMITX[:, f], *self.args(v), self.ABS[f], self.SCA[f], INTOBS=self.kw.get("intobs", NO_INTOBS), save_colden=colden,
                          LENGTH=LENGTH, healpix=self.kw.get("healpix", 0))
        engine.set_opt(None)
        return m, t

    def upload(self, engine, nf):
        engine.set_map_block(self.EMITX[:, :nf], self.ABS[:nf], self.SCA[:nf], None if self.OPTX is None else self.OPTX[:, :nf, :])

    def block(self, engine, v):
        return engine.map_block(*self.args(v), INTOBS=self.kw.get("intobs", NO_INTOBS), LENGTH=LENGTH, healpix=self.kw.get("healpix", 0))

    def poison(self, engine):
        """a full-width batch of NaN: what a narrower batch after it leaves unwritten in the device buffers stays NaN"""
        n = engine.map_block_max
        nan = np.full((self.cloud.CELLS, n), np.nan, np.float32)
        engine.set_map_block(nan, np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32),
                             None if self.OPTX is None else np.full((self.cloud.CELLS, n, 2), np.nan, np.float32))


def _reset(engine):
    engine.set_map_block(None)
    engine.set_map_threshold(0)
    engine.set_map_interpolation(0)
    engine.set_map_roi(None)
    engine.set_opt(None)


def _same(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def cases(engine):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, engine, 2 if name == "map_c208_entry" else engine.map_block_max)   # 208^3 cells: 2 x 36 MB
        made[name].switch(engine)
        return made[name]
    yield get
    _reset(engine)


@pytest.mark.parametrize("name", CASES)
def test_block_planes_equal_the_per_frequency_kernel(name, engine, cases):
    case = cases(name)
    assert engine.map_block_max == 32
    widths = [2] if name == "map_c208_entry" else [1, 2, 3, engine.map_block_max]
    lit = 0
    for nf in widths:
        if nf == 3:
            case.poison(engine)                                # nothing behind the third column may reach the planes
        case.upload(engine, nf)
        for v in range(case.views):
            MAPX, TAUX, COLDEN = case.block(engine, v)
            assert MAPX.shape[0] == nf and TAUX.shape[0] == nf
            for f in range(nf):
                m, t = case.ref[f][v]
                assert _same(MAPX[f], m), (name, nf, f, v)
                assert _same(TAUX[f], t), (name, nf, f, v)
                lit += int((m > 0).sum())
            assert _same(COLDEN, case.colden[v]), (name, nf, v)
            assert np.isfinite(MAPX).all() and np.isfinite(TAUX).all() and (COLDEN > 0).any()
            if nf > 1:
                assert not MAPX[1].any() and TAUX[1].any()     # the frequency without emission still has its optical depth
    assert lit > 30
    _reset(engine)


def test_both_branches_of_the_step_integral_are_taken(engine, cases):
    """the opacity factors put single steps on both sides of DTAU = 1e-3: at the thinnest frequency a pixel's whole optical depth
    is below it (map_c8_abu: 2.0e-4), so each of its steps is; at the thickest a pixel's depth passes 1, over the fewer than a
    thousand cells (8 root cells, at most three levels) that a ray can cross"""
    for name in ("map_c8_abu", "map_oct8"):
        case = cases(name)
        taus = [np.concatenate([case.ref[f][v][1].ravel() for v in range(case.views)]) for f in (0, 1)]
        assert taus[1].max() > 1.0
        if name == "map_c8_abu":
            assert 0 < taus[0][taus[0] > 0].min() < 1e-3


@pytest.mark.parametrize("name", ["map_oct8", "map_oct8_healpix"])
def test_block_planes_equal_the_oracle(name, engine, cases, oracle_soc):
    case = cases(name)
    nf = 3
    case.upload(engine, nf)
    kw = case.kw
    for v in range(case.views):
        MAPX, TAUX, COLDEN = case.block(engine, v)
        for f in range(nf):
            job = Job(case.cloud, CSC, ABS=case.ABS[f], SCA=case.SCA[f])
            m, t = oracle_mapping(oracle_soc, job, case.EMITX[:, f].copy(), *case.args(v), kw.get("intobs", NO_INTOBS), 0, LENGTH, kw.get("healpix", 0))
            assert _same(MAPX[f].ravel(), m.ravel()) and _same(TAUX[f].ravel(), t.ravel()), (name, f, v)
        _, col = oracle_mapping(oracle_soc, Job(case.cloud, CSC, ABS=case.ABS[0], SCA=case.SCA[0]), case.EMITX[:, 0].copy(), *case.args(v),
                                kw.get("intobs", NO_INTOBS), 1, LENGTH, kw.get("healpix", 0))
        assert _same(COLDEN.ravel(), col.ravel())
    _reset(engine)


@pytest.mark.parametrize("name", ["map_oct759_1080", "map_oct759_healpix5"])
def test_more_than_one_workgroup_and_a_ragged_last_one(name, engine, cases, oracle_soc):
    """1080 pixels are four workgroups of 256 and one of 56 lanes, 300 are one and 44 lanes: blockIdx.x * blockDim.x and the plane
    stride f * npix + id matter.  Widths 1, 3 (after a full-width batch of NaN) and 32: every plane equals the per-frequency
    kernel's, and three of them the oracle's."""
    case = cases(name)
    kw = case.kw
    npix = 12 * kw["healpix"] ** 2 if kw.get("healpix") else kw["npix"][0] * kw["npix"][1]
    assert npix > 256 and npix % 256 != 0
    for nf in (1, 3, engine.map_block_max):
        if nf == 3:
            case.poison(engine)
        case.upload(engine, nf)
        for v in range(case.views):
            MAPX, TAUX, COLDEN = case.block(engine, v)
            assert MAPX.shape[0] == nf and TAUX.shape[0] == nf and MAPX[0].size == npix
            for f in range(nf):
                m, t = case.ref[f][v]
                assert _same(MAPX[f], m) and _same(TAUX[f], t), (name, nf, f, v)
            assert _same(COLDEN, case.colden[v]) and np.isfinite(MAPX).all() and np.isfinite(TAUX).all()
            assert (MAPX[0] > 0).sum() > 30
            if nf == 3:
                for f in range(3):
                    job = Job(case.cloud, CSC, ABS=case.ABS[f], SCA=case.SCA[f])
                    m, t = oracle_mapping(oracle_soc, job, case.EMITX[:, f].copy(), *case.args(v), kw.get("intobs", NO_INTOBS), 0, LENGTH,
                                          kw.get("healpix", 0))
                    assert _same(MAPX[f].ravel(), m.ravel()) and _same(TAUX[f].ravel(), t.ravel()), (name, f, v)
    _reset(engine)


def test_a_batch_stays_resident_across_directions(engine, cases):
    case = cases("map_oct8")
    case.upload(engine, 3)
    once = [case.block(engine, v) for v in (0, 1)]
    for v in (0, 1):
        case.upload(engine, 3)
        fresh = case.block(engine, v)
        assert all(_same(a, b) for a, b in zip(once[v], fresh))
    assert not _same(once[0][0], once[1][0])
    _reset(engine)


def test_argument_errors_leave_the_engine_usable(engine, cases):
    case = cases("map_oct8")
    n = engine.map_block_max + 1
    with pytest.raises(soclib.SocError, match=str(engine.map_block_max)):
        engine.set_map_block(np.zeros((case.cloud.CELLS, n), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32))
    engine.set_map_block(None)
    with pytest.raises(soclib.SocError, match="no batch"):
        case.block(engine, 0)
    with pytest.raises(soclib.SocError):
        engine.set_map_block(np.zeros((case.cloud.CELLS + 1, 2), np.float32), np.zeros(2, np.float32), np.zeros(2, np.float32))
    m, t = case.per_frequency(engine, 0, 0)
    assert _same(m, case.ref[0][0][0]) and _same(t, case.ref[0][0][1])
    case.upload(engine, 2)
    assert _same(case.block(engine, 0)[0][0], case.ref[0][0][0])
    _reset(engine)


def test_ini_run_with_a_fourth_mapping_argument_writes_the_same_files(tmp_path):
    """a map-only run (`iterations 0`, emission from a temperature file) from an ini file with the HIP engine: `mapping 12 10
    0.8 3` and `mapping 12 10 0.8` write the same bytes"""
    from soc_amd import synth
    out = {}
    for tag, mapping in (("plain", "mapping 12 10 0.8"), ("block", "mapping 12 10 0.8 3")):
        d = str(tmp_path / tag)
        os.makedirs(d)
        cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
        files.write_temperature(os.path.join(d, "m.T"), cloud, np.asarray(np.random.default_rng(8).uniform(2500.0, 6000.0, cloud.CELLS), np.float32))
        extra = ("iterations 0\nloadtemp\ntemperature %s/m.T\nemitted %s/m.emit\n%s\ndirection 30 40\ndirection 90 0\nsavetau %s/sv -1 0.641\n"
                 % (d, d, mapping, d))
        ini = _write_model(d, cloud, extra=extra)
        txt = open(ini).read().replace("nosolve\n", "").replace("nomap\n", "").replace("absorbed %s/abs.data\n" % d, "")
        open(ini, "w").write(txt)
        os.chdir(d)
        hip = soclib.Engine(0)
        try:
            AbsorptionRun(User(ini), hip, verbose=0).run()
        finally:
            hip.close()
        names = sorted(f for f in os.listdir(d) if f.startswith("map_dir_") or f.startswith("sv_"))
        out[tag] = {f: open(os.path.join(d, f), "rb").read() for f in names}
    assert sorted(out["plain"]) == ["map_dir_00.bin", "map_dir_01.bin", "sv_colden_dir0_000.fits", "sv_colden_dir1_001.fits",
                                    "sv_tau_0.64_dir0_000.bin", "sv_tau_0.64_dir1_001.bin"]
    maps = np.frombuffer(out["plain"]["map_dir_00.bin"], np.float32, offset=8)
    assert maps.size == 3 * 120 and (maps > 0).sum() > 100
    assert out["block"] == out["plain"]
