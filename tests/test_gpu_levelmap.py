"""Per-level maps on the GPU (`mapping nx ny dx 999`): soc_map_levels against the CPU restatement of the Mapping kernel of
kernel_ASOC_map_H.c in soc mode (the math header both sides compile), bit for bit, no pixel left out, and against the recorded
reference as tests/test_levelmap.py compares it.  Reads only the repository and tests/golden/."""
import os

import numpy as np
import pytest

import levelmap_cases as lc
import levelmap_host
from levelmap_engine import LevelOracleEngine
from polmap_engine import write_model
from soc_amd import lib as soclib
from soc_amd import synth
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levelmaps.npz")


@pytest.fixture
def lev(engine):
    """the shared engine, given back without per-cell opacities, fp16 rounding or map switches"""
    yield engine
    engine.set_opt_half(False)
    engine.set_opt(None)
    engine.set_map_threshold(0)
    engine.set_map_interpolation(0)
    engine.set_map_roi(None)


def _both(eng, cloud, EMIT, OPT=None, PAR=None, **kw):
    got = eng.map_levels(EMIT, kw["DIR"], kw["RA"], kw["DE"], kw["NPIX"], kw["MAP_DX"], kw["CENTRE"], kw["ABS"], kw["SCA"], INTOBS=kw["INTOBS"])
    want = levelmap_host.levelmap("soc", cloud, EMIT, OPT=OPT, PAR=PAR, **kw)
    return got, want


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_golden_cases_equal_the_restatement(lev, name):
    g = np.load(GOLDEN)
    m, kw = lc.case_args(name, g["ODIR"], g["RA"], g["DE"])
    c = m["cloud"]
    lev.set_cloud(c)
    lev.set_opt(None)
    got, want = _both(lev, c, m["EMIT"], **kw)
    assert got.shape == (c.LEVELS, lc.NPIX[1], lc.NPIX[0])
    assert levelmap_host.same_bits(got, want), name
    assert lc.close_to_reference(name, got, g["map_" + name])
    if m["OPT"] is not None:
        # the per-cell opacities the reference never reads (tests/test_levelmap.py): with the scalars in every cell the same
        # maps; with the model's own -- as the handle keeps them, the fp16 form included -- those of the restatement
        flat = np.empty((c.CELLS, 2), np.float32)
        flat[:, 0], flat[:, 1] = m["SCA"], m["ABS"]
        lev.set_opt(flat)
        assert levelmap_host.same_bits(_both(lev, c, m["EMIT"], OPT=flat, **kw)[0], got)
        lev.set_opt_half(lc.CASES[name]["model"].endswith("h"))
        lev.set_opt(m["OPT"])
        OPT = lev.read_opt()
        assert np.array_equal(np.asarray(OPT, np.float32).reshape(c.CELLS, 2), m["OPT"])
        own, want = _both(lev, c, m["EMIT"], OPT=OPT, **kw)
        assert levelmap_host.same_bits(own, want) and not levelmap_host.same_bits(own, got)


@pytest.mark.parametrize("levels, frac", [(6, 0.2), (9, 0.2)])
def test_deep_hierarchies(lev, levels, frac):
    """8^3 roots refined to 6 and to 9 levels: the kernels with 8 and with 16 accumulators"""
    c = synth.octree_cloud(8, levels=levels, frac=frac, seed=13)
    assert c.LEVELS == levels
    EMIT = np.asarray(np.random.default_rng(3).uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
    ODIR, RA, DE = lc.views()
    lev.set_cloud(c)
    lev.set_opt(None)
    PAR = levelmap_host.parents(c)
    for idir, obs in ((0, None), (1, None), (0, (4.3, 3.6, 4.2))):
        got, want = _both(lev, c, EMIT, PAR=PAR, DIR=ODIR[idir], RA=RA[idir], DE=DE[idir], NPIX=(40, 36), MAP_DX=0.3, CENTRE=lc.centre(c),
                          ABS=4.0e-5, SCA=6.0e-5, INTOBS=obs)
        assert got.shape == (levels, 36, 40) and levelmap_host.same_bits(got, want)
        if obs is None and idir == 0:
            assert all((want[l] != 0.0).any() for l in range(levels))      # every level shows


@pytest.mark.parametrize("obs", [None, (16.3, 15.6, 16.2)], ids=["external", "perspective"])
def test_at_size(lev, obs):
    """32^3 roots with 3 levels, 256 x 192 pixels = 192 workgroups; the external view misses the model in a fifth of the
    pixels, the perspective one has rays that the step limit ends (the walk cycles)"""
    c = synth.octree_cloud(32, levels=3, frac=0.05, seed=5)
    EMIT = np.asarray(np.random.default_rng(3).uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
    ODIR, RA, DE = lc.views()
    lev.set_cloud(c)
    lev.set_opt(None)
    kw = dict(DIR=ODIR[0], RA=RA[0], DE=DE[0], NPIX=(256, 192), MAP_DX=0.2, CENTRE=lc.centre(c), ABS=1.0e-5, SCA=2.0e-5, INTOBS=obs)
    got, want = _both(lev, c, EMIT, **kw)
    assert levelmap_host.same_bits(got, want)
    assert all((want[l] != 0.0).any() for l in range(3))
    if obs is None:
        missed = (want == 0.0).all(axis=0)
        assert 0.1 * missed.size < missed.sum() < 0.5 * missed.size
    # a ragged last workgroup: 255 x 193 pixels is no multiple of 256
    kw["NPIX"] = (255, 193)
    got, want = _both(lev, c, EMIT, **kw)
    assert levelmap_host.same_bits(got, want)


def test_switches_have_no_effect(lev):
    g = np.load(GOLDEN)
    m, kw = lc.case_args("oct8_v0", g["ODIR"], g["RA"], g["DE"])
    lev.set_cloud(m["cloud"])
    lev.set_opt(None)
    first, _ = _both(lev, m["cloud"], m["EMIT"], **kw)
    lev.set_map_threshold(1)
    lev.set_map_interpolation(2)
    lev.set_map_roi([2, 5, 1, 6, 3, 4])
    assert levelmap_host.same_bits(_both(lev, m["cloud"], m["EMIT"], **kw)[0], first)


def test_error_codes(lev):
    m = lc.model("oct8")
    c = m["cloud"]
    ODIR, RA, DE = lc.views()
    fresh = soclib.Engine(0)
    try:
        fresh.CELLS, fresh.LEVELS = c.CELLS, c.LEVELS
        with pytest.raises(soclib.SocError, match=r"soc_set_grid.*code -2"):
            fresh.map_levels(m["EMIT"], ODIR[0], RA[0], DE[0], (9, 7), 1.0, lc.centre(c), 1e-5, 1e-5)      # no grid: SOC_ERR_STATE
    finally:
        fresh.close()
    lev.set_cloud(c)
    lev.set_opt(None)
    args = (m["EMIT"], ODIR[0], RA[0], DE[0], (9, 7), 1.0, lc.centre(c), 1e-5, 1e-5)
    first = lev.map_levels(*args)
    for npix in ((0, 7), (9, 0), (-3, 7), (9, -1)):
        with pytest.raises(soclib.SocError, match=r"NPIX.*code -1"):
            lev.map_levels(*args[:4], npix, *args[5:])
    h, F = lev.h, soclib._f
    v = [np.ascontiguousarray(np.asarray(a, np.float32).ravel()[:3]) for a in (ODIR[0], RA[0], DE[0], lc.centre(c))]
    E = np.ascontiguousarray(m["EMIT"], np.float32)
    out = np.zeros(4, np.float32)
    call = lev.lib.soc_map_levels
    # LEVELS * NPIX_X * NPIX_Y beyond int: refused before anything is allocated or written
    assert call(h, 40000, 40000, np.float32(1.0), F(E), F(v[0]), F(v[1]), F(v[2]), F(v[3]), None, np.float32(1e-5), np.float32(1e-5), F(out)) == -1
    assert call(h, 30000, 30000, np.float32(1.0), F(E), F(v[0]), F(v[1]), F(v[2]), F(v[3]), None, np.float32(1e-5), np.float32(1e-5), F(out)) == -1
    # null pointers
    assert call(h, 9, 7, np.float32(1.0), None, F(v[0]), F(v[1]), F(v[2]), F(v[3]), None, np.float32(1e-5), np.float32(1e-5), F(out)) == -1
    assert call(h, 9, 7, np.float32(1.0), F(E), F(v[0]), F(v[1]), F(v[2]), F(v[3]), None, np.float32(1e-5), np.float32(1e-5), None) == -1
    assert call(h, 9, 7, np.float32(1.0), F(E), None, F(v[1]), F(v[2]), F(v[3]), None, np.float32(1e-5), np.float32(1e-5), F(out)) == -1
    assert call(None, 9, 7, np.float32(1.0), F(E), F(v[0]), F(v[1]), F(v[2]), F(v[3]), None, np.float32(1e-5), np.float32(1e-5), F(out)) == -1
    with pytest.raises(soclib.SocError, match=r"MAP_DX.*code -1"):
        lev.map_levels(*args[:5], 0.0, *args[6:])
    with pytest.raises(soclib.SocError, match=r"DIR.*code -1"):                  # the walk divides by the components of -DIR
        lev.map_levels(m["EMIT"], (1.0, 0.0, 0.0), RA[0], DE[0], (9, 7), 1.0, lc.centre(c), 1e-5, 1e-5)
    with pytest.raises(soclib.SocError, match=r"INTOBS.*code -1"):
        lev.map_levels(*args, INTOBS=(3.0, np.inf, 3.0))
    with pytest.raises(soclib.SocError, match="CELLS"):
        lev.map_levels(m["EMIT"][:-1], *args[1:])
    assert (out == 0.0).all()
    # a refused call changes nothing; with an observer the direction arguments are not needed
    assert levelmap_host.same_bits(lev.map_levels(*args), first)
    inside = lev.map_levels(m["EMIT"], None, None, None, (9, 7), 1.0, None, 1e-5, 1e-5, INTOBS=(4.3, 3.6, 4.2))
    want = levelmap_host.levelmap("soc", c, m["EMIT"], None, None, None, (9, 7), 1.0, None, 1e-5, 1e-5, INTOBS=(4.3, 3.6, 4.2))
    assert levelmap_host.same_bits(inside, want)
    # an observer outside the model: zeros on every level
    assert (lev.map_levels(m["EMIT"], None, None, None, (9, 7), 1.0, None, 1e-5, 1e-5, INTOBS=(-2.0, 4.0, 4.0)) == 0.0).all()


def test_ini_run_writes_the_files_of_the_test_engine(tmp_path):
    """one run from an ini file with the HIP engine (abundances, fp16 opacities, two directions, a `wavelength` window): its
    map_dir_XX_H.bin equal those of the test engine byte for byte"""
    out = {}
    hip = soclib.Engine(0)
    for tag in ("hip", "cpu"):
        d = str(tmp_path / tag)
        os.makedirs(d)
        cloud = synth.octree_cloud(6, levels=3, frac=0.1, seed=9)
        ini = write_model(d, cloud, synth.magnetic_field(cloud, seed=2), extra="wavelength 150 350\noptishalf\n")
        np.asarray(np.random.default_rng(4).uniform(0.2, 1.0, cloud.CELLS), np.float32).tofile(os.path.join(d, "m.abu"))
        text = "".join(l for l in open(ini).read().splitlines(True) if not l.startswith("polmap "))
        text = text.replace("mapping 14 11 0.9\n", "mapping 14 11 0.9 999\n").replace("optical %s/m.dust\n" % d, "optical %s/m.dust %s/m.abu\n" % (d, d))
        with open(ini, "w") as fp:
            fp.write(text)
        os.chdir(d)
        try:
            AbsorptionRun(User(ini), hip if tag == "hip" else LevelOracleEngine("soc"), verbose=0).run()
        finally:
            if tag == "hip":
                hip.close()
        names = sorted(f for f in os.listdir(d) if f.startswith("map_dir"))
        out[tag] = {f: open(os.path.join(d, f), "rb").read() for f in names}
    assert sorted(out["hip"]) == ["map_dir_00_H.bin", "map_dir_01_H.bin"]
    assert len(out["hip"]["map_dir_00_H.bin"]) == 16 + 4 * 2 * 3 * 11 * 14
    assert out["hip"] == out["cpu"]
