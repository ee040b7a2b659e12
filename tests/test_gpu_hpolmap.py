"""All-sky polarisation maps on the GPU: soc_polmap_healpix against the CPU restatement of PolHealpixMapping in soc mode (the
math header both sides compile), bit for bit, no pixel left out.  Reads only the repository and tests/golden/."""
import os

import numpy as np
import pytest

import hpolmap_cases as hc
import hpolmap_host
import polmap_host
from hpolmap_engine import HPolOracleEngine
from polmap_engine import write_model
from soc_amd import lib as soclib
from soc_amd import synth
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpolmaps.npz")


@pytest.fixture
def pol(engine):
    """the shared engine, given back without field, per-cell opacities, fp16 rounding or threshold"""
    yield engine
    engine.set_bfield(None)
    engine.set_opt_half(False)
    engine.set_opt(None)
    engine.set_map_threshold(0)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_golden_cases_equal_the_restatement(pol, name):
    """every case of the golden file -- here the models with abundances run WITH their per-cell opacities, as the engine does"""
    k = hc.CASES[name]
    m = hc.model(k["model"])
    c = m["cloud"]
    sw = hc.switches(name)
    pol.set_cloud(c)
    pol.set_opt(m["OPT"])
    pol.set_bfield(*m["B"])
    pol.set_map_threshold(sw["threshold"])
    obs = hc.case_observer(name)
    kw = {a: b for a, b in sw.items() if a != "threshold"}
    got = pol.polmap_healpix(m["EMIT"], hc.NSIDE, obs, m["ABS"], m["SCA"], **kw)
    want = hpolmap_host.polmap("soc", c, m["B"], m["EMIT"], hc.NSIDE, obs, m["ABS"], m["SCA"], OPT=m["OPT"], **sw)
    assert got.shape == (4, 12 * hc.NSIDE ** 2) and np.isfinite(got).all()
    assert hpolmap_host.same_bits(got, want), name
    ref = np.load(GOLDEN)["map_" + name]
    assert np.array_equal(got[3] > 0.0, ref[3] > 0.0)                      # the same pixels see a column as in the reference


def test_cartesian_at_size(pol):
    """NSIDE 128 (196 608 pixels) from near the centre of a 128^3 cloud, interpolate 2"""
    c = synth.cartesian_cloud(128, seed=21)
    B = synth.magnetic_field(c, seed=6)
    EMIT = np.asarray(np.random.default_rng(3).uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
    obs = (64.3, 63.6, 64.2)
    pol.set_cloud(c)
    pol.set_opt(None)
    pol.set_bfield(*B)
    got = pol.polmap_healpix(EMIT, 128, obs, 3.0e-6, 5.0e-6, interpolate=2, polred=1, LENGTH=hc.pc.length_literal())
    want = hpolmap_host.polmap("soc", c, B, EMIT, 128, obs, 3.0e-6, 5.0e-6, interpolate=2, polred=1, LENGTH=hc.pc.length_literal())
    assert got.shape == (4, 196608) and hpolmap_host.same_bits(got, want)
    assert np.isfinite(got).all() and (got[0] > 0).all() and (got[3] > 0).all()


def test_octree_with_fp16_opacities_at_size(pol):
    """NSIDE 128 from near the centre of the 104^3-root octree (Index() in double) with per-cell opacities rounded through
    fp16, interpolate 3 and threshold 1"""
    c = synth.octree_cloud(104, levels=3, frac=0.002, seed=11)
    B = synth.magnetic_field(c, seed=6)
    rng = np.random.default_rng(3)
    EMIT = np.asarray(rng.uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
    PAR = polmap_host.parents(c)
    obs = (52.3, 51.6, 52.2)
    pol.set_cloud(c)
    pol.set_opt_half(True)
    pol.set_opt(np.asarray(rng.uniform(2.0e-6, 8.0e-6, (c.CELLS, 2)), np.float32))
    OPT = pol.read_opt()
    assert np.array_equal(OPT, np.asarray(np.asarray(OPT, np.float16), np.float32))
    pol.set_bfield(*B)
    pol.set_map_threshold(1)
    got = pol.polmap_healpix(EMIT, 128, obs, 0.0, 0.0, interpolate=3, LENGTH=hc.pc.length_literal())
    want, NST = hpolmap_host.polmap("soc", c, B, EMIT, 128, obs, 0.0, 0.0, OPT=OPT, interpolate=3, threshold=1, LENGTH=hc.pc.length_literal(),
                                    PAR=PAR, steps=True)
    assert NST.max() < 1 << 15                                             # every ray ends by itself
    assert hpolmap_host.same_bits(got, want) and np.isfinite(got).all() and (got[3] > 0).all()


def test_error_codes_and_field_lifetime(pol):
    m = hc.model("oct8")
    c = m["cloud"]
    obs = (4.3, 3.6, 4.2)
    pol.set_cloud(c)
    pol.set_opt(None)
    pol.set_bfield(None)
    args = (m["EMIT"], hc.NSIDE, obs, 1e-5, 1e-5)
    with pytest.raises(soclib.SocError, match=r"soc_set_bfield.*code -2"):
        pol.polmap_healpix(*args)                                          # no field: SOC_ERR_STATE
    pol.set_bfield(*m["B"])
    first = pol.polmap_healpix(*args)
    with pytest.raises(soclib.SocError, match=r"NSIDE.*code -1"):
        pol.polmap_healpix(m["EMIT"], 0, obs, 1e-5, 1e-5)
    for bad in (-1, 4):
        with pytest.raises(soclib.SocError, match=r"interpolate.*code -1"):
            pol.polmap_healpix(*args, interpolate=bad)
    for bad in (1, 2):                                                     # a hierarchy: level 0 is no plain grid
        with pytest.raises(soclib.SocError, match=r"interpolate.*hierarchy.*code -1"):
            pol.polmap_healpix(*args, interpolate=bad)
    with pytest.raises(soclib.SocError, match=r"y_shear.*maxlos.*code -1"):
        pol.polmap_healpix(*args, y_shear=2.5)
    with pytest.raises(soclib.SocError, match=r"y_shear.*maxlos.*code -1"):
        pol.polmap_healpix(*args, y_shear=2.5, maxlos=1e9)
    # a refused call changes nothing, and the handle stays usable
    assert hpolmap_host.same_bits(pol.polmap_healpix(*args), first)
    assert hpolmap_host.same_bits(first, hpolmap_host.polmap("soc", c, m["B"], *args))
    sheared = pol.polmap_healpix(*args, y_shear=2.5, maxlos=20.0)
    assert hpolmap_host.same_bits(sheared, hpolmap_host.polmap("soc", c, m["B"], *args, y_shear=2.5, maxlos=20.0))
    # freeing the field brings the error back; another grid drops the field of the old one
    pol.set_bfield(None)
    with pytest.raises(soclib.SocError, match="code -2"):
        pol.polmap_healpix(*args)
    pol.set_bfield(*m["B"])
    c8 = synth.cartesian_cloud(8, seed=3)
    pol.set_cloud(c8)
    with pytest.raises(soclib.SocError, match="code -2"):
        pol.polmap_healpix(np.ones(512, np.float32), hc.NSIDE, obs, 1e-5, 1e-5)
    B8 = synth.magnetic_field(c8, seed=5)
    pol.set_bfield(*B8)
    got = pol.polmap_healpix(np.ones(512, np.float32), hc.NSIDE, obs, 1e-5, 1e-5, interpolate=1)       # and 1 is fine on a plain grid
    assert hpolmap_host.same_bits(got, hpolmap_host.polmap("soc", c8, B8, np.ones(512, np.float32), hc.NSIDE, obs, 1e-5, 1e-5, interpolate=1))


def test_ini_run_writes_the_files_of_the_test_engine(tmp_path):
    """one run from an ini file with the HIP engine: its Healpix tables equal those of the test engine byte for byte"""
    out = {}
    hip = soclib.Engine(0)
    for tag in ("hip", "cpu"):
        d = str(tmp_path / tag)
        os.makedirs(d)
        cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
        ini = write_model(d, cloud, synth.magnetic_field(cloud, seed=2),
                          extra="mapping 6 -1 1.0\nperspective 3.3 2.6 3.2\npolred adhoc\nthreshold 1\ninterpolate 3\nwavelength 90 210\n")
        os.chdir(d)
        try:
            AbsorptionRun(User(ini), hip if tag == "hip" else HPolOracleEngine("soc"), verbose=0).run()
        finally:
            if tag == "hip":
                hip.close()
        names = sorted(f for f in os.listdir(d) if f.startswith("pol_healpix"))
        out[tag] = {f: open(os.path.join(d, f), "rb").read() for f in names}
    assert sorted(out["hip"]) == ["pol_healpix.fits.1", "pol_healpix.fits.2"]
    assert out["hip"] == out["cpu"]
