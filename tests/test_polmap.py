"""Polarisation maps without a GPU: the CPU restatement of PolMapping (tests/csrc/polmap_host.c) against the recorded
results of the reference's own kernels (tests/golden/polmaps.npz), the host path AbsorptionRun.write_polmaps on a test
engine backed by that restatement, the refusals, and a physical check that needs no reference."""
import os

import numpy as np
import pytest

import polmap_cases as pc
import polmap_host
from polmap_engine import PolOracleEngine, write_model
from soc_amd import files, launch, synth
from soc_amd.asoc import AbsorptionRun, UnsupportedOption
from soc_amd.ini import User

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polmaps.npz")


def run_case(mode, name, idir, golden):
    mname, polstat, polred, rhow, thr = pc.CASES[name]
    m = pc.model(mname)
    c = m["cloud"]
    return polmap_host.polmap(mode, c, m["B"], m["EMIT"], golden["ODIR"][idir], golden["RA"][idir], golden["DE"][idir], pc.NPIX,
                              m["MAP_DX"], pc.centre(c), m["ABS"], m["SCA"], OPT=m["OPT"], polstat=polstat, polred=polred,
                              rho_weight=rhow, threshold=thr, p0=pc.p0_literal(pc.P0), LENGTH=pc.length_literal())


def test_golden_file_holds_every_case_and_its_inputs_are_reproduced():
    g = np.load(GOLDEN)
    ODIR, RA, DE = pc.views()
    assert np.array_equal(g["ODIR"], ODIR) and np.array_equal(g["RA"], RA) and np.array_equal(g["DE"], DE)
    assert tuple(g["NPIX"]) == pc.NPIX and (pc.NPIX[0] * pc.NPIX[1]) % 256 != 0
    for name, case in pc.CASES.items():
        assert g["map_" + name].shape == (len(pc.VIEWS), 4, pc.NPIX[1], pc.NPIX[0])
        assert np.array_equal(g["fp_" + case[0]], pc.fingerprint(pc.model(case[0]))), "the inputs of %s changed" % name
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_restatement_equals_the_reference_bit_for_bit(name):
    """libm mode against the x86 build of the reference's PolMapping: every pixel of every plane, NaNs in the same pixels"""
    g = np.load(GOLDEN)
    polstat = pc.CASES[name][1]
    for idir in range(len(pc.VIEWS)):
        ref = g["map_" + name][idir]
        got = run_case("libm", name, idir, g)
        assert polmap_host.same_bits(got, ref), "%s, direction %d" % (name, idir)
        missed = np.isnan(ref).any(axis=0) if polstat else (ref[3] == 0.0)
        assert 0 < missed.sum() < missed.size, "the map should be wider than the cloud, and not miss it"
        if polstat:
            assert np.isnan(ref[:3][:, missed]).all()                 # 0/0 for a ray that misses the cloud: kept
        else:
            assert not np.isnan(ref).any() and (ref[:, missed] == 0.0).all()


def test_soc_mode_differs_from_libm_only_in_the_last_bits():
    g = np.load(GOLDEN)
    for name in ("oct8_s0", "oct104_s0"):
        ref = g["map_" + name][0]
        got = run_case("soc", name, 0, g)
        assert np.allclose(got[[0, 3]], ref[[0, 3]], rtol=1e-5, atol=0.0)
        assert np.allclose(got[1:3], ref[1:3], rtol=0.0, atol=1e-5 * np.abs(ref[0]).max())


def test_fmod_of_the_math_header_equals_libm():
    """soc_fmodf_small against glibc fmodf: exact for y > 0 and quotients below 2^22, sign of x"""
    rng = np.random.default_rng(12)
    PI = np.float32(3.1415926536)
    x = np.concatenate([rng.uniform(0.0, 10.0, 200000), rng.uniform(-10.0, 0.0, 1000), np.arange(0, 40) * np.float64(PI),
                        np.nextafter(np.arange(1, 40, dtype=np.float32) * PI, np.float32(0)),
                        np.nextafter(np.arange(1, 40, dtype=np.float32) * PI, np.float32(1e9)), [0.0, 1e-30, 3.0e6]]).astype(np.float32)
    y = np.full_like(x, PI)
    assert np.array_equal(polmap_host.fmod("soc", x, y).view(np.uint32), polmap_host.fmod("libm", x, y).view(np.uint32))
    x = rng.uniform(0.0, 4.0e6, 200000).astype(np.float32)
    y = np.exp(rng.uniform(np.log(1.0), np.log(50.0), x.size)).astype(np.float32)
    assert np.array_equal(polmap_host.fmod("soc", x, y).view(np.uint32), polmap_host.fmod("libm", x, y).view(np.uint32))
    r = polmap_host.fmod("soc", np.asarray([np.nan], np.float32), np.asarray([PI], np.float32))
    assert np.isnan(r[0])


# ---- host path ---------------------------------------------------------------------------------------------------------

def _model(tmp_path, extra="", levels=2):
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=levels, frac=0.1, seed=9) if levels > 1 else synth.cartesian_cloud(6, seed=9)
    B = synth.magnetic_field(cloud, seed=2)
    T = np.random.default_rng(8).uniform(10.0, 18.0, cloud.CELLS).astype(np.float32)
    ini = write_model(d, cloud, B, extra=extra, T=T)
    os.chdir(d)
    return d, cloud, B, T, ini


def _run_polmaps(ini, engine=None):
    eng = PolOracleEngine("soc") if engine is None else engine
    run = AbsorptionRun(User(ini), eng, verbose=0)
    run.setup_engine()
    _, EMITTED = run.emission_from_temperature_file()
    return run, eng, EMITTED, run.write_polmaps(EMITTED)


def test_polarisation_maps_files_planes_and_frequencies(tmp_path):
    d, cloud, B, T, ini = _model(tmp_path, extra="p0 0.123456\n")
    run, eng, EMITTED, names = _run_polmaps(ini)
    # all three frequencies (no `mapum`, no `wavelength`), two directions each: polmap_<um>_<dir>.fits
    um = [1.0e4 * launch.C_LIGHT / f for f in (1.0e12, 1.5e12, 3.0e12)]
    assert names == ["polmap_%.1f_%02d.fits" % (u, i) for u in um for i in range(2)]
    assert len(eng.polmap_calls) == 6 and eng.B is None                     # one launch per direction; the field is freed
    call = eng.polmap_calls[2]                                              # second frequency, first direction
    assert call["p0"] == 0.1235 and call["polstat"] == 0 and call["polred"] == 0 and call["rho_weight"] == 0
    for k in range(3):
        assert np.array_equal(call["B"][k], B[k])                           # no polred: the field as the files hold it
    KK = (1.0e23 / launch.FACTOR) * launch.PLANCK / (4.0 * np.pi) * (0.5 * launch.PARSEC)
    FREQ = float(run.FFREQ[1])
    assert np.array_equal(call["EMIT"], np.asarray(KK * FREQ * EMITTED[:, 1], np.float32)) and call["EMIT"].dtype == np.float32
    assert call["LENGTH"] == launch.kernel_literals(0.5)[1]
    # the file: four planes [4, NPIX.y, NPIX.x] in the order the engine returned them, no frequency comments
    hdr, data = files.read_fits(os.path.join(d, names[2]))
    assert data.shape == (4, 11, 14) and hdr["NAXIS"] == 3 and hdr["NAXIS3"] == 4 and "CTYPE3" not in hdr and hdr["COMMENT"] == []
    _, ODIR, RA, DE = launch.set_observer_directions(run.U.OBS_THETA, run.U.OBS_PHI)
    want = polmap_host.polmap("soc", cloud, B, call["EMIT"], ODIR[0], RA[0], DE[0], (14, 11), 0.9, (3.0, 3.0, 3.0), call["ABS"], call["SCA"],
                              p0=0.1235, LENGTH=call["LENGTH"])
    assert polmap_host.same_bits(data, want)
    assert (want[0] > 0).any() and (want[3] > 0).any() and np.abs(want[1]).max() > 0 and np.abs(want[2]).max() > 0
    assert (np.abs(want[1]) <= want[0]).all()                               # |Q| <= I


def test_frequency_selection_follows_mapum_then_wavelength(tmp_path):
    d, cloud, B, T, ini = _model(tmp_path, extra="wavelength 150 250\n")
    _, _, _, names = _run_polmaps(ini)
    assert names == ["polmap_199.9_00.fits", "polmap_199.9_01.fits"]
    # `mapum` overrides `wavelength` (ASOC.py:3757-3762): within 1 % of a listed wavelength
    with open(ini, "a") as fp:
        fp.write("mapum 100.5 301.0\n")
    _, _, _, names = _run_polmaps(ini)
    assert names == ["polmap_299.8_00.fits", "polmap_299.8_01.fits", "polmap_99.9_00.fits", "polmap_99.9_01.fits"]


def test_polred_encodings(tmp_path):
    """the three forms of `polred` (ASOC.py:3681-3719) against the numpy expressions of the reference"""
    d, cloud, B, T, ini0 = _model(tmp_path)
    base = open(ini0).read()
    Rfile = np.random.default_rng(4).uniform(-0.2, 1.2, cloud.CELLS).astype(np.float32)
    np.concatenate([np.asarray([cloud.CELLS], np.int32).view(np.float32), Rfile]).tofile(os.path.join(d, "R.bin"))
    dens = files.read_temperature(os.path.join(d, "m.cloud"), cloud)

    def expected(R):
        BB = [b.copy() for b in B]
        R = R / np.sqrt(BB[0] ** 2 + BB[1] ** 2 + BB[2] ** 2 + 1.0e-10)
        for k in range(3):
            BB[k] *= R
        return BB

    R1 = (T.copy() - 13.3) / 2.0 + 1.0e-4
    R1 = np.exp(R1) / (np.exp(R1) + np.exp(-R1))
    R2 = dens.copy()
    R2 *= 2.5
    R2 = np.clip(R2, 0.1, 1e10)
    R2 = 0.5 * (1.0 + np.tanh((np.log10(3e3) - np.log10(R2)) / 0.5))
    R3 = np.clip(Rfile, 1.0e-6, 0.999999)
    for polred, extra, R in (("adhoc", "", R1), ("rhofun_3e3_0.5", "density 2.5\n", R2), (os.path.join(d, "R.bin"), "", R3)):
        with open(ini0, "w") as fp:
            fp.write(base + "polred %s\n%s" % (polred, extra))
        _, eng, _, _ = _run_polmaps(ini0)
        call = eng.polmap_calls[0]
        assert call["polred"] == 1
        want = expected(R)
        for k in range(3):
            assert np.array_equal(call["B"][k], np.asarray(want[k], np.float32)), polred
        length = np.sqrt(sum(b.astype(np.float64) ** 2 for b in call["B"]))
        assert (length <= 1.0 + 1e-6).all() and (length > 0.0).all()              # 0 < R <= 1 became the length of the vectors
    # polstat 3 takes the vectors as they are and runs without -D POLRED
    with open(ini0, "w") as fp:
        fp.write(base + "polred adhoc\npolstat 3\n")
    _, eng, _, _ = _run_polmaps(ini0)
    assert eng.polmap_calls[0]["polred"] == 0 and eng.polmap_calls[0]["polstat"] == 3
    assert all(np.array_equal(eng.polmap_calls[0]["B"][k], B[k]) for k in range(3))


def test_switches_reach_the_engine(tmp_path):
    d, cloud, B, T, ini = _model(tmp_path, extra="polrhoweight\nthreshold 1\npolstat 1\nwavelength 90 110\n")
    run, eng, _, names = _run_polmaps(ini)
    assert eng.map_threshold == 1 and eng.polmap_calls[0]["rho_weight"] == 1 and eng.polmap_calls[0]["polstat"] == 1
    _, data = files.read_fits(names[0])
    _, ODIR, RA, DE = launch.set_observer_directions(run.U.OBS_THETA, run.U.OBS_PHI)
    c = eng.polmap_calls[0]
    want = polmap_host.polmap("soc", cloud, B, c["EMIT"], ODIR[0], RA[0], DE[0], (14, 11), 0.9, (3.0, 3.0, 3.0), c["ABS"], c["SCA"], polstat=1,
                              threshold=1, p0=0.2, LENGTH=c["LENGTH"])
    assert polmap_host.same_bits(data, want) and np.isnan(want).any() and np.isfinite(want).any()


def test_nomap_still_writes_polarisation_maps(tmp_path):
    d, cloud, B, T, ini = _model(tmp_path, extra="nomap\nwavelength 90 110\n")
    AbsorptionRun(User(ini), PolOracleEngine("soc"), verbose=0).run()
    assert os.path.exists(os.path.join(d, "polmap_99.9_00.fits")) and os.path.exists(os.path.join(d, "polmap_99.9_01.fits"))
    assert not os.path.exists(os.path.join(d, "map_dir_00.bin"))
    # without `nomap` both kinds of map are written
    text = open(ini).read().replace("nomap\n", "")
    with open(ini, "w") as fp:
        fp.write(text)
    os.remove(os.path.join(d, "polmap_99.9_00.fits"))
    AbsorptionRun(User(ini), PolOracleEngine("soc"), verbose=0).run()
    assert os.path.exists(os.path.join(d, "polmap_99.9_00.fits")) and os.path.exists(os.path.join(d, "map_dir_00.bin"))


def test_refusals(tmp_path):
    from oracle_engine import OracleEngine
    d, cloud, B, T, ini = _model(tmp_path)
    base = open(ini).read()

    def reason(extra, engine=None, text=None):
        with open(ini, "w") as fp:
            fp.write((base if text is None else text) + extra)
        with pytest.raises(UnsupportedOption) as e:
            AbsorptionRun(User(ini), PolOracleEngine("soc") if engine is None else engine, verbose=0)
        return str(e.value)

    assert "polstat 2" in reason("polstat 2\n")
    assert "polstat 4" in reason("polstat 4\n")
    assert "polstat 5" in reason("polstat 5\n")
    assert "Healpix" in reason("mapping 8 -1 1.0\nperspective 3 3 3\n")
    assert "libmaps" in reason("libmaps lib.txt\n")
    assert "polsim" in reason("", text=base.replace("polmap ", "polsim "))
    assert "polred without polmap" in reason("polred adhoc\n", text=base.replace("polmap ", "# polmap "))
    # an engine without the kernel is refused, and told why
    assert "no polarisation-map kernel" in reason("", engine=OracleEngine("soc"))
    # ... and the accepted forms are accepted
    for extra in ("", "polstat 1\n", "polstat 3\n", "polred adhoc\n", "polrhoweight\n", "threshold 1\n"):
        with open(ini, "w") as fp:
            fp.write(base + extra)
        AbsorptionRun(User(ini), PolOracleEngine("soc"), verbose=0)
    with pytest.raises(ValueError):
        polmap_host.polmap("soc", cloud, B, np.ones(cloud.CELLS), (0.5, 0.5, 0.7), (0, 1, 0), (0, 0, 1), (4, 4), 1.0, (3, 3, 3), 1e-5, 1e-5, polstat=2)


# ---- a check that needs no reference -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["libm", "soc"])
def test_uniform_field_in_the_plane_of_the_sky(mode):
    """Cartesian cloud, one field vector everywhere, in the plane of the sky, constant p0, no threshold.  Every term of Q
    is then the same constant times the corresponding term of I:  Q_k = p sz_k cos(2 Psi) cc,  I_k = sz_k (1 - p (cc - 2/3)),
    so Q/I = p cos(2 Psi) cc / (1 - p (cc - 0.6666667)) per pixel, and U/I likewise with sin(2 Psi).  The ratio of the
    computed sums differs from that by the rounding of the per-term products (three for Q_k, one for I_k, each 2^-24) and
    of the constants (cos, cc, the bracket), and by the n_steps - 1 additions of each same-signed sum: the bound is
    (n_steps + 8) 2^-24 relative, with n_steps the cells the pixel's ray crosses, counted by the walk itself (8 to 24 here).
    A ray that misses the cloud gives I = Q = U = 0 exactly."""
    cloud = synth.cartesian_cloud(8, seed=3)
    ODIR, RA, DE = pc.views()
    EMIT = np.asarray(np.random.default_rng(1).uniform(0.5e-3, 1.5e-3, cloud.CELLS), np.float32)
    p = np.float32(0.2)
    for idir in range(2):
        D, R, E = (v[idir, :3].astype(np.float64) for v in (ODIR, RA, DE))
        b = np.asarray(0.6 * (0.35 * R + 0.8 * E), np.float32)                # in the plane of the sky, 23.6 degrees from DE
        B = [np.full(cloud.CELLS, b[k], np.float32) for k in range(3)]
        MAP, NST = polmap_host.polmap(mode, cloud, B, EMIT, ODIR[idir], RA[idir], DE[idir], pc.NPIX, 0.6, pc.centre(cloud),
                                      4.0e-5, 6.0e-5, p0=p, LENGTH=1.0, steps=True)
        # the constants in float64 from the float32 inputs, with the kernel's literals
        b32 = b.astype(np.float32)
        s = np.float32(1.0) / np.sqrt(b32[0] * b32[0] + b32[1] * b32[1] + b32[2] * b32[2], dtype=np.float32)
        bn = (b32 * s).astype(np.float64)
        Psi = 0.5 * np.float64(np.float32(3.1415926536)) + np.arctan2(np.dot(bn, -R), np.dot(bn, E))
        cc = np.float64(np.float32(0.99999)) - np.float64(np.float32(0.99998)) * np.dot(bn, D) ** 2
        den = 1.0 - np.float64(p) * (cc - np.float64(np.float32(0.6666667)))
        qi = np.float64(p) * np.cos(2.0 * Psi) * cc / den
        ui = np.float64(p) * np.sin(2.0 * Psi) * cc / den
        assert abs(qi) > 0.05 and abs(ui) > 0.05
        hit = NST > 0
        assert 50 < hit.sum() < hit.size
        assert (MAP[:3][:, ~hit] == 0.0).all()
        n = NST[hit].astype(np.float64)
        assert n.min() >= 1 and n.max() <= 24
        I, Q, U = (MAP[k][hit].astype(np.float64) for k in range(3))
        bound = (n + 8.0) * 2.0 ** -24
        eq, eu = np.abs(Q / I / qi - 1.0), np.abs(U / I / ui - 1.0)
        print("direction %d (%s): steps %d..%d, max |Q/I error| / bound %.3f, max |U/I error| / bound %.3f"
              % (idir, mode, n.min(), n.max(), (eq / bound).max(), (eu / bound).max()))
        assert (eq <= bound).all() and (eu <= bound).all()
