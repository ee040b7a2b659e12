"""Per-level maps (`mapping nx ny dx 999`) without a GPU: the CPU restatement of the Mapping kernel of kernel_ASOC_map_H.c
(tests/csrc/levelmap_host.c) against the recorded results of the reference's own kernel (tests/golden/levelmaps.npz), the host
path AbsorptionRun.write_level_maps on a test engine backed by that restatement, the file layout, the refusals and the driver.

The plain-map golden file tests/golden/maps.npz holds no case that can be compared with the sum of the levels: its models
carry another emission and other opacities, and its views and pixel grids are others.  That check is left out."""
import os

import numpy as np
import pytest

import levelmap_cases as lc
import levelmap_host
from levelmap_engine import LevelOracleEngine, LevelPipelineEngine
from oracle_engine import OracleEngine
from polmap_engine import write_model
from soc_amd import launch, synth
from soc_amd.asoc import AbsorptionRun, UnsupportedOption
from soc_amd.ini import User

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "levelmaps.npz")


def run_case(mode, name, g, OPT=None, steps=False):
    m, kw = lc.case_args(name, g["ODIR"], g["RA"], g["DE"])
    return levelmap_host.levelmap(mode, m["cloud"], m["EMIT"], OPT=OPT, steps=steps, **kw)


def test_golden_file_holds_every_case_and_its_inputs_are_reproduced():
    g = np.load(GOLDEN)
    ODIR, RA, DE = lc.views()
    assert np.array_equal(g["ODIR"], ODIR) and np.array_equal(g["RA"], RA) and np.array_equal(g["DE"], DE)
    assert tuple(g["NPIX"]) == lc.NPIX and (lc.NPIX[0] * lc.NPIX[1]) % 256 != 0
    for name, k in lc.CASES.items():
        m = lc.model(k["model"])
        assert g["map_" + name].shape == (m["cloud"].LEVELS, lc.NPIX[1], lc.NPIX[0])
        assert np.array_equal(g["fp_" + k["model"]], lc.fingerprint(m)), "the inputs of %s changed" % name
    assert os.path.getsize(GOLDEN) < 1 << 20
    K = lc.CASES.values()
    assert {k["model"] for k in K} == {"c8", "c8abu", "c8abuh", "oct8", "oct104", "r759", "oct759", "oct104x6x5", "oct6x104x5"}
    assert lc.CASES["oct8_face"]["view"] == (0.5, 3.0, 2.9)
    for model in ("c8", "oct8", "oct104"):                                  # both external views of every geometry
        assert {k["view"] for k in K if k["model"] == model and k["dx"] is None and not isinstance(k["view"], tuple)} == {0, 1}
    for name in lc.CASES:                                                   # every level of the small octree shows in every case
        if lc.CASES[name]["model"] == "oct8":
            assert all((g["map_" + name][l] != 0.0).any() for l in range(3)), name


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_restatement_equals_the_reference_bit_for_bit(name):
    """libm mode against the x86 build of the reference's Mapping: every pixel of every level.  The reference never reads
    per-cell opacities in this kernel (levelmap_host.c), so the models with abundances run without them here."""
    g = np.load(GOLDEN)
    ref = g["map_" + name]
    got, NST = run_case("libm", name, g, steps=True)
    assert levelmap_host.same_bits(got, ref), name
    # (on the octrees a few values are negative, -7e-8 at most where the images are of order 1: after a climb into a root leaf
    # that file's walk goes on with octet coordinates, and a step from a position just below 0 has a negative length -- kept)
    assert np.isfinite(ref).all() and (ref > 0.0).any() and ref.min() > -1.0e-7 * ref.max()
    missed = NST == 0
    assert (ref[:, missed] == 0.0).all()                                    # a ray that misses the model: zero on every level
    assert (ref.sum(axis=0)[~missed] > 0.0).all()
    if lc.model(lc.CASES[name]["model"])["cloud"].LEVELS == 1:
        assert ref.shape[0] == 1                                            # LEVELS = 1: one image
    if isinstance(lc.CASES[name]["view"], tuple):
        assert not missed.any()                                             # an observer inside sees the model in every pixel
    else:
        assert 0 < missed.sum() < missed.size
    if name.endswith("_wide"):
        ring = np.ones(missed.shape, bool)
        ring[1:-1, 1:-1] = False
        assert missed[ring].all() and (ref[:, ring] == 0.0).all()


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_soc_mode_agrees_with_the_reference(name):
    """the header the HIP kernel compiles against the recorded reference: levelmap_cases.close_to_reference"""
    g = np.load(GOLDEN)
    assert lc.close_to_reference(name, run_case("soc", name, g), g["map_" + name])


def test_the_face_observer_is_nudged():
    """(0.5, 3.0, 2.9): y sits on a cell face, fmod(y, 1) < 1e-5, so the walk starts from y + 2e-5 (kernel_ASOC_map_H.c:433);
    started 2e-5 below the face instead it crosses other cells"""
    g = np.load(GOLDEN)
    m, kw = lc.case_args("oct8_face", g["ODIR"], g["RA"], g["DE"])
    kw["INTOBS"] = (0.5, float(np.float32(3.0) + np.float32(2.0e-5)), 2.9)
    assert levelmap_host.same_bits(levelmap_host.levelmap("libm", m["cloud"], m["EMIT"], **kw), g["map_oct8_face"])
    kw["INTOBS"] = (0.5, float(np.float32(3.0) - np.float32(2.0e-5)), 2.9)
    assert not levelmap_host.same_bits(levelmap_host.levelmap("libm", m["cloud"], m["EMIT"], **kw), g["map_oct8_face"])


def test_per_cell_opacities_take_the_place_of_the_scalars():
    """The line under "#ifdef USE_ABU" (kernel_ASOC_map_H.c:475) cannot be recorded from the reference.  It is pinned through
    the scalars: with OPT = (SCA, ABS) in every cell the sum o.x + o.y is the float SCA + ABS, so the maps must equal the
    recorded scalar ones bit for bit; with the model's own OPT they must differ."""
    g = np.load(GOLDEN)
    for name in ("c8abu_v0", "c8abuh_v1"):
        m = lc.model(lc.CASES[name]["model"])
        OPT = np.empty((m["cloud"].CELLS, 2), np.float32)
        OPT[:, 0], OPT[:, 1] = m["SCA"], m["ABS"]
        assert levelmap_host.same_bits(run_case("libm", name, g, OPT=OPT), g["map_" + name])
        own = run_case("libm", name, g, OPT=m["OPT"])
        assert np.isfinite(own).all() and not levelmap_host.same_bits(own, g["map_" + name])
        assert np.array_equal(own != 0.0, g["map_" + name] != 0.0)


def test_restatement_refuses_more_levels_than_the_kernel_takes():
    c = synth.cartesian_cloud(4, seed=1)
    c.LEVELS = 17
    with pytest.raises(ValueError):
        levelmap_host.levelmap("soc", c, np.ones(c.CELLS, np.float32), (0.5, 0.5, 0.7), (0, 1, 0), (0, 0, 1), (4, 4), 1.0, (2, 2, 2), 1e-5, 1e-5,
                               PAR=np.zeros(1, np.int32))


# ---- host path ---------------------------------------------------------------------------------------------------------

def _model(tmp_path, extra="", levels=2, mapping="mapping 14 11 0.9 999", abundances=False):
    """the far-infrared model of the polarisation-map tests (three frequencies: 300, 200 and 100 um; emission from a
    temperature file) without its polmap line, two directions"""
    d = str(tmp_path)
    os.makedirs(d, exist_ok=True)
    cloud = synth.octree_cloud(6, levels=levels, frac=0.1, seed=9) if levels > 1 else synth.cartesian_cloud(6, seed=9)
    T = np.random.default_rng(8).uniform(10.0, 18.0, cloud.CELLS).astype(np.float32)
    ini = write_model(d, cloud, synth.magnetic_field(cloud, seed=2), extra=extra, T=T)
    text = "".join(l for l in open(ini).read().splitlines(True) if not l.startswith("polmap "))
    text = text.replace("mapping 14 11 0.9\n", mapping + "\n")
    if abundances:
        np.asarray(np.random.default_rng(4).uniform(0.2, 1.0, cloud.CELLS), np.float32).tofile(os.path.join(d, "m.abu"))
        text = text.replace("optical %s/m.dust\n" % d, "optical %s/m.dust %s/m.abu\n" % (d, d))
    with open(ini, "w") as fp:
        fp.write(text)
    os.chdir(d)
    return d, cloud, ini


def _read(path, levels):
    raw = open(path, "rb").read()
    nx, ny, nf, nl = np.frombuffer(raw[:16], np.int32)
    assert nl == levels and len(raw) == 16 + 4 * nf * nl * ny * nx
    return (int(nx), int(ny)), np.frombuffer(raw[16:], np.float32).reshape(nf, nl, ny, nx)


def test_level_map_files_header_layout_and_frequencies(tmp_path):
    d, cloud, ini = _model(tmp_path, extra="wavelength 150 350\n")
    eng = LevelOracleEngine("soc")
    run = AbsorptionRun(User(ini), eng, verbose=0)
    run.run()
    assert sorted(f for f in os.listdir(d) if f.startswith("map_dir")) == ["map_dir_00_H.bin", "map_dir_01_H.bin"]
    # 300 and 200 um are inside `wavelength`, 100 um is not: two frequencies, each with one launch per direction
    assert len(eng.level_calls) == 4
    KK = (1.0e23 / launch.FACTOR) * launch.PLANCK / (4.0 * np.pi) * (0.5 * launch.PARSEC)
    _, ODIR, RA, DE = launch.set_observer_directions(run.U.OBS_THETA, run.U.OBS_PHI)
    for idir in range(2):
        npix, data = _read(os.path.join(d, "map_dir_%02d_H.bin" % idir), cloud.LEVELS)
        assert npix == (14, 11) and data.shape == (2, 2, 11, 14)
        for k, IFREQ in enumerate((0, 1)):
            call = eng.level_calls[2 * k + idir]
            FREQ = np.float32(float(run.FFREQ[IFREQ]))
            assert np.array_equal(call["EMIT"], run.EMITTED[:, IFREQ] * np.float32(KK) * FREQ) and call["EMIT"].dtype == np.float32
            assert call["INTOBS"] is None or call["INTOBS"][0] < -1e10
            assert call["OPT"] is None and call["NPIX"] == (14, 11) and call["MAP_DX"] == 0.9 and call["CENTRE"] == (3.0, 3.0, 3.0)
            want = levelmap_host.levelmap("soc", cloud, call["EMIT"], ODIR[idir], RA[idir], DE[idir], (14, 11), 0.9, (3.0, 3.0, 3.0), call["ABS"], call["SCA"])
            assert levelmap_host.same_bits(data[k], want)
            assert all((want[l] > 0.0).any() for l in range(cloud.LEVELS))
    assert not os.path.exists(os.path.join(d, "map_dir_00.bin"))


def test_keys_without_effect_and_perspective(tmp_path):
    """`mapint`, `threshold` and `roimap` change nothing (that kernel tests none of them); `mapum` selects nothing here;
    `perspective` reaches the engine as INTOBS"""
    out = {}
    for tag, extra in (("plain", ""), ("keys", "mapint 1\nthreshold 1\nroi 1 4 1 4 1 4\nroimap\nmapum 200.0\n"), ("inside", "perspective 2.5 3.0 2.9\n")):
        d, cloud, ini = _model(tmp_path / tag, extra=extra)
        eng = LevelOracleEngine("soc")
        AbsorptionRun(User(ini), eng, verbose=0).run()
        out[tag] = (open(os.path.join(d, "map_dir_00_H.bin"), "rb").read(), eng)
    assert out["keys"][0] == out["plain"][0] and out["inside"][0] != out["plain"][0]
    assert out["inside"][1].level_calls[0]["INTOBS"] == (2.5, 3.0, 2.9)
    assert np.frombuffer(out["plain"][0][8:16], np.int32).tolist() == [3, 2]


def test_abundances_reach_the_engine_as_per_cell_opacities(tmp_path):
    for extra, half in (("", False), ("optishalf\n", True)):
        d, cloud, ini = _model(tmp_path / ("h%d" % half), extra="wavelength 150 250\n" + extra, abundances=True)
        eng = LevelOracleEngine("soc")
        run = AbsorptionRun(User(ini), eng, verbose=0)
        run.run()
        call = eng.level_calls[0]
        assert call["OPT"] is not None and call["OPT"].shape == (cloud.CELLS, 2) and (call["OPT"] > 0).all()
        assert np.array_equal(call["OPT"], np.asarray(np.asarray(call["OPT"], np.float16), np.float32)) == half
        _, ODIR, RA, DE = launch.set_observer_directions(run.U.OBS_THETA, run.U.OBS_PHI)
        _, data = _read(os.path.join(d, "map_dir_00_H.bin"), cloud.LEVELS)
        want = levelmap_host.levelmap("soc", cloud, call["EMIT"], ODIR[0], RA[0], DE[0], (14, 11), 0.9, (3.0, 3.0, 3.0), call["ABS"], call["SCA"],
                                      OPT=call["OPT"])
        assert data.shape[0] == 1 and levelmap_host.same_bits(data[0], want)


def test_single_level_model_writes_one_image_per_frequency(tmp_path):
    d, cloud, ini = _model(tmp_path, levels=1)
    AbsorptionRun(User(ini), LevelOracleEngine("soc"), verbose=0).run()
    npix, data = _read(os.path.join(d, "map_dir_01_H.bin"), 1)
    assert data.shape == (3, 1, 11, 14) and (data > 0).any()


def test_refusals(tmp_path):
    d, cloud, ini = _model(tmp_path)
    base = open(ini).read()

    def reason(extra="", engine=LevelOracleEngine, text=None):
        with open(ini, "w") as fp:
            fp.write((base if text is None else text) + extra)
        with pytest.raises(UnsupportedOption) as e:
            AbsorptionRun(User(ini), engine("soc"), verbose=0)
        return str(e.value)

    assert "no per-level map kernel" in reason(engine=OracleEngine)                                          # (a)
    assert "Healpix" in reason("perspective 3 3 3\n", text=base.replace("mapping 14 11 0.9 999", "mapping 8 -1 0.9 999"))   # (b)
    assert "savetau" in reason("savetau %s/sv 200.0\n" % d)                                                  # (c)
    assert "savetau" in reason("savetau %s/sv -1\n" % d)
    assert "libmaps" in reason("libmaps lib.txt\n")                                                          # (d)
    for extra in ("", "perspective 3 3 3\n", "mapint 2\n"):
        with open(ini, "w") as fp:
            fp.write(base + extra)
        AbsorptionRun(User(ini), LevelOracleEngine("soc"), verbose=0)
    with open(ini, "w") as fp:                                                                               # 1000 is >= 999 as well
        fp.write(base.replace(" 999\n", " 1000\n"))
    assert AbsorptionRun(User(ini), LevelOracleEngine("soc"), verbose=0).U.FAST_MAP == 1000


def test_driver_reaches_the_level_maps(tmp_path):
    """soc_amd.driver with `mapping ... 999`: transfer, emission of two dust components, then map_dir_00_H.bin with the
    per-cell opacities of the abundance file"""
    from soc_amd import driver
    from test_driver import NFREQ, write_case
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, _, _ = write_case(d, cloud)
    text = open(ini).read().replace("mapping 8 8 1.0\n", "mapping 8 8 1.0 999\n")
    with open(ini, "w") as fp:
        fp.write(text)
    os.chdir(d)
    eng = LevelPipelineEngine("soc")
    P = driver.Pipeline(ini, eng, verbose=0)
    P.run()
    npix, data = _read(os.path.join(d, "map_dir_00_H.bin"), 2)
    assert npix == (8, 8) and data.shape == (NFREQ, 2, 8, 8) and len(eng.level_calls) == NFREQ
    assert not os.path.exists(os.path.join(d, "map_dir_00.bin"))
    assert np.isfinite(data).all() and (data >= 0).all() and all((data[:, l] > 0).any() for l in range(2))
    assert eng.level_calls[0]["OPT"] is not None
