"""Polarisation maps on the GPU: soc_polmap against the CPU restatement of PolMapping in soc mode (the math header both
sides compile), bit for bit, NaNs compared by position, no pixel left out.  Reads only the repository and tests/golden/."""
import os

import numpy as np
import pytest

import polmap_cases as pc
import polmap_host
from polmap_engine import PolOracleEngine, write_model
from soc_amd import lib as soclib
from soc_amd import synth
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polmaps.npz")


@pytest.fixture
def pol(engine):
    """the shared engine, given back without field, per-cell opacities, fp16 rounding or threshold"""
    yield engine
    engine.set_bfield(None)
    engine.set_opt_half(False)
    engine.set_opt(None)
    engine.set_map_threshold(0)


def _both(eng, cloud, B, EMIT, DIR, RA, DE, NPIX, MAP_DX, ABS, SCA, OPT=None, polstat=0, polred=0, rho_weight=0, threshold=0, p0=0.2,
          LENGTH=1.0, PAR=None):
    eng.set_map_threshold(threshold)
    got = eng.polmap(EMIT, DIR, RA, DE, NPIX, MAP_DX, pc.centre(cloud), ABS, SCA, polstat=polstat, polred=polred, rho_weight=rho_weight,
                     p0=p0, LENGTH=LENGTH)
    want = polmap_host.polmap("soc", cloud, B, EMIT, DIR, RA, DE, NPIX, MAP_DX, pc.centre(cloud), ABS, SCA, OPT=OPT, polstat=polstat,
                              polred=polred, rho_weight=rho_weight, threshold=threshold, p0=p0, LENGTH=LENGTH, PAR=PAR)
    return got, want


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_golden_cases_equal_the_restatement(pol, name):
    g = np.load(GOLDEN)
    mname, polstat, polred, rhow, thr = pc.CASES[name]
    m = pc.model(mname)
    c = m["cloud"]
    pol.set_cloud(c)
    pol.set_opt(m["OPT"])
    pol.set_bfield(*m["B"])
    for idir in range(len(pc.VIEWS)):
        got, want = _both(pol, c, m["B"], m["EMIT"], g["ODIR"][idir], g["RA"][idir], g["DE"][idir], pc.NPIX, m["MAP_DX"], m["ABS"], m["SCA"],
                          OPT=m["OPT"], polstat=polstat, polred=polred, rho_weight=rhow, threshold=thr, p0=pc.p0_literal(pc.P0),
                          LENGTH=pc.length_literal())
        assert got.shape == (4, pc.NPIX[1], pc.NPIX[0])
        assert polmap_host.same_bits(got, want), "%s, direction %d" % (name, idir)
        # and the device stays as close to the reference's own numbers as the two math libraries are
        ref = g["map_" + name][idir]
        assert np.array_equal(np.isnan(got), np.isnan(ref))


def test_cartesian_at_size(pol):
    """500 x 333 pixels of a 128^3 cloud, POLSTAT 0 (with polred), 1 and 3"""
    c = synth.cartesian_cloud(128, seed=21)
    B = synth.magnetic_field(c, seed=6)
    EMIT = np.asarray(np.random.default_rng(3).uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
    ODIR, RA, DE = pc.views()
    pol.set_cloud(c)
    pol.set_opt(None)
    pol.set_bfield(*B)
    for polstat, polred, idir in ((0, 1, 0), (1, 0, 0), (3, 0, 1), (0, 0, 1)):
        got, want = _both(pol, c, B, EMIT, ODIR[idir], RA[idir], DE[idir], (500, 333), 0.45, 3.0e-6, 5.0e-6, polstat=polstat, polred=polred,
                          p0=0.2, LENGTH=pc.length_literal())
        assert polmap_host.same_bits(got, want), "POLSTAT %d, direction %d" % (polstat, idir)
        hit = (want[3] != 0.0) if polstat == 0 else np.isfinite(want[0])
        assert 0 < hit.sum() < hit.size                                    # some rays miss the cloud


def test_octree_with_abundances_at_size(pol):
    """300 x 300 pixels of the 104^3-root octree (Index() in double) with per-cell opacities rounded through fp16"""
    c = synth.octree_cloud(104, levels=3, frac=0.002, seed=11)
    B = synth.magnetic_field(c, seed=6)
    rng = np.random.default_rng(3)
    EMIT = np.asarray(rng.uniform(0.5e-3, 1.5e-3, c.CELLS), np.float32)
    ODIR, RA, DE = pc.views()
    PAR = polmap_host.parents(c)
    pol.set_cloud(c)
    pol.set_opt_half(True)
    pol.set_opt(np.asarray(rng.uniform(2.0e-6, 8.0e-6, (c.CELLS, 2)), np.float32))
    OPT = pol.read_opt()
    assert np.array_equal(OPT, np.asarray(np.asarray(OPT, np.float16), np.float32))
    pol.set_bfield(*B)
    for polstat, polred, thr, idir in ((0, 0, 0, 0), (1, 1, 1, 0), (3, 0, 0, 1)):
        got, want = _both(pol, c, B, EMIT, ODIR[idir], RA[idir], DE[idir], (300, 300), 0.6, 0.0, 0.0, OPT=OPT, polstat=polstat, polred=polred,
                          threshold=thr, p0=0.2, LENGTH=pc.length_literal(), PAR=PAR)
        assert polmap_host.same_bits(got, want), "POLSTAT %d, direction %d" % (polstat, idir)


def test_error_codes_and_field_lifetime(pol):
    c = synth.octree_cloud(8, levels=3, frac=0.15, seed=7)
    m = pc.model("oct8")
    ODIR, RA, DE = pc.views()
    pol.set_cloud(c)
    pol.set_opt(None)
    pol.set_bfield(None)
    args = (m["EMIT"], ODIR[0], RA[0], DE[0], (9, 7), 1.0, pc.centre(c), 1e-5, 1e-5)
    with pytest.raises(soclib.SocError, match=r"soc_set_bfield.*code -2"):
        pol.polmap(*args)                                                  # no field: SOC_ERR_STATE
    pol.set_bfield(*m["B"])
    first = pol.polmap(*args)
    for bad in (2, 4, 5, -1):
        with pytest.raises(soclib.SocError, match=r"polstat.*code -1"):
            pol.polmap(*args, polstat=bad)
    with pytest.raises(soclib.SocError, match=r"polred.*code -1"):
        pol.polmap(*args, polstat=3, polred=1)
    with pytest.raises(soclib.SocError, match=r"DIR.*code -1"):
        pol.polmap(m["EMIT"], (1.0, 0.0, 0.0), RA[0], DE[0], (9, 7), 1.0, pc.centre(c), 1e-5, 1e-5)
    with pytest.raises(soclib.SocError):
        pol.set_bfield(m["B"][0][:-1], m["B"][1], m["B"][2])
    # a refused call changes nothing; setting the field again replaces it; freeing it brings the error back
    assert polmap_host.same_bits(pol.polmap(*args), first)
    B2 = [np.ascontiguousarray(b[::-1]) for b in m["B"]]
    pol.set_bfield(*B2)
    second = pol.polmap(*args)
    assert not polmap_host.same_bits(second, first)
    assert polmap_host.same_bits(second, polmap_host.polmap("soc", c, B2, *args[:1], *args[1:4], (9, 7), 1.0, pc.centre(c), 1e-5, 1e-5))
    pol.set_bfield(*m["B"])
    assert polmap_host.same_bits(pol.polmap(*args), first)
    pol.set_bfield(None)
    pol.set_bfield(None)
    with pytest.raises(soclib.SocError, match="code -2"):
        pol.polmap(*args)
    # another grid drops the field of the old one
    pol.set_bfield(*m["B"])
    pol.set_cloud(synth.cartesian_cloud(8, seed=3))
    with pytest.raises(soclib.SocError, match="code -2"):
        pol.polmap(np.ones(512, np.float32), *args[1:])


def test_fmod_probe(pol):
    rng = np.random.default_rng(12)
    PI = np.float32(3.1415926536)
    x = np.concatenate([rng.uniform(0.0, 10.0, 100000), rng.uniform(-10.0, 0.0, 1000), np.arange(0, 40) * np.float64(PI),
                        np.nextafter(np.arange(1, 40, dtype=np.float32) * PI, np.float32(0)), [0.0, 1e-30, 3.0e6]]).astype(np.float32)
    y = np.full_like(x, PI)
    assert np.array_equal(pol.probe_math("fmod", x, y).view(np.uint32), polmap_host.fmod("soc", x, y).view(np.uint32))
    assert np.array_equal(pol.probe_math("fmod", x, y).view(np.uint32), polmap_host.fmod("libm", x, y).view(np.uint32))
    x = rng.uniform(0.0, 4.0e6, 100000).astype(np.float32)
    y = np.exp(rng.uniform(0.0, np.log(50.0), x.size)).astype(np.float32)
    assert np.array_equal(pol.probe_math("fmod", x, y).view(np.uint32), polmap_host.fmod("libm", x, y).view(np.uint32))
    with pytest.raises(soclib.SocError):
        pol.probe_math("fmod", x)


def test_ini_run_writes_the_files_of_the_test_engine(tmp_path):
    """one run from an ini file with the HIP engine: its FITS files equal those of the test engine byte for byte"""
    out = {}
    hip = soclib.Engine(0)
    for tag in ("hip", "cpu"):
        d = str(tmp_path / tag)
        os.makedirs(d)
        cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
        ini = write_model(d, cloud, synth.magnetic_field(cloud, seed=2), extra="polred adhoc\nthreshold 1\nnomap\nwavelength 90 210\n")
        os.chdir(d)
        try:
            AbsorptionRun(User(ini), hip if tag == "hip" else PolOracleEngine("soc"), verbose=0).run()
        finally:
            if tag == "hip":
                hip.close()
        names = sorted(f for f in os.listdir(d) if f.startswith("polmap_"))
        out[tag] = {f: open(os.path.join(d, f), "rb").read() for f in names}
    assert sorted(out["hip"]) == ["polmap_199.9_00.fits", "polmap_199.9_01.fits", "polmap_99.9_00.fits", "polmap_99.9_01.fits"]
    assert out["hip"] == out["cpu"]
