"""All-sky (Healpix) polarisation maps without a GPU: the CPU restatement of PolHealpixMapping (tests/csrc/hpolmap_host.c)
against the recorded results of the reference's own kernel (tests/golden/hpolmaps.npz), the host path
AbsorptionRun.write_healpix_polmaps on a test engine backed by that restatement, the Healpix FITS table, the refusals, and a
physical check that needs no reference."""
import os

import numpy as np
import pytest

import hpolmap_cases as hc
import hpolmap_host
from hpolmap_engine import HPolOracleEngine
from polmap_engine import PolOracleEngine, write_model
from soc_amd import files, launch, synth
from soc_amd.asoc import AbsorptionRun, UnsupportedOption
from soc_amd.ini import User

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpolmaps.npz")


def run_case(mode, name, OPT=None):
    k = hc.CASES[name]
    m = hc.model(k["model"])
    return hpolmap_host.polmap(mode, m["cloud"], m["B"], m["EMIT"], hc.NSIDE, hc.case_observer(name), m["ABS"], m["SCA"], OPT=OPT,
                               **hc.switches(name))


def test_golden_file_holds_every_case_and_its_inputs_are_reproduced():
    g = np.load(GOLDEN)
    assert int(g["NSIDE"]) == hc.NSIDE and (12 * hc.NSIDE ** 2) % 64 != 0
    for name, k in hc.CASES.items():
        assert g["map_" + name].shape == (4, 12 * hc.NSIDE ** 2)
        assert np.array_equal(g["obs_" + name], np.asarray(hc.case_observer(name), np.float64))
        assert np.array_equal(g["fp_" + k["model"]], hc.fingerprint(hc.model(k["model"]))), "the inputs of %s changed" % name
    assert os.path.getsize(GOLDEN) < 1 << 20
    # every switch the kernel has is in some case
    K = hc.CASES.values()
    assert {k["model"] for k in K} == {"c8", "c8abu", "c8abuh", "oct8", "oct104", "r759", "oct759", "oct104x6x5", "oct6x104x5"}
    assert {k["polred"] for k in K} == {0, 1} and {k["thr"] for k in K} == {0, 1, 2} and {k["interp"] for k in K} == {0, 1, 2, 3}
    assert any(k["maxlos"] < 8 for k in K) and any(k["minlos"] > 0 for k in K) and any(k["yshear"] == 2.5 and k["maxlos"] == 20.0 for k in K)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_restatement_equals_the_reference_bit_for_bit(name):
    """libm mode against the x86 build of the reference's PolHealpixMapping: every pixel of every plane.  The reference
    never reads per-cell opacities in this kernel (hpolmap_host.c), so the models with abundances run without them here."""
    g = np.load(GOLDEN)
    ref = g["map_" + name]
    got = run_case("libm", name)
    assert hpolmap_host.same_bits(got, ref), name
    assert np.isfinite(ref).all() and (ref[0][ref[3] > 0.0] > 0.0).all()
    if hc.CASES[name]["obs"] == "outside":
        assert (ref == 0.0).all()                                          # an observer outside the cloud: four planes of zeros
    else:
        assert (ref[3] > 0.0).any() and np.abs(ref[1]).max() > 0.0 and np.abs(ref[2]).max() > 0.0


def test_per_cell_opacities_take_the_place_of_the_scalars():
    """The line under "#ifdef USE_ABU" (kernel_ASOC_map_H.c:737) cannot be recorded from the reference.  It is pinned through
    the scalars: with OPT = (SCA, ABS) in every cell the sum o.x + o.y is the float SCA + ABS, so the map must equal the
    recorded scalar one bit for bit; with the model's own OPT it must differ."""
    g = np.load(GOLDEN)
    for name in ("c8abu_centre", "c8abuh_face"):
        m = hc.model(hc.CASES[name]["model"])
        OPT = np.empty((m["cloud"].CELLS, 2), np.float32)
        OPT[:, 0], OPT[:, 1] = m["SCA"], m["ABS"]
        assert hpolmap_host.same_bits(run_case("libm", name, OPT=OPT), g["map_" + name])
        own = run_case("libm", name, OPT=m["OPT"])
        assert np.isfinite(own).all() and not hpolmap_host.same_bits(own, g["map_" + name])
        assert np.array_equal(own[3], g["map_" + name][3])                 # the column density does not see the opacity


def test_soc_mode_against_libm_mode():
    """The two math libraries differ in the last bits of sin, cos, acos, atan2 and exp.  Measured here over all cases of the
    golden file: largest relative difference 1.54e-3 in I and 8.43 in N, largest absolute difference in Q, U 1.63e-3 max|I|.
    Those figures are the octrees': there the reference's walk is discontinuous (a ray that climbs into a root leaf goes on
    from the grid's corner), and a last-bit difference sends a handful of rays (at most 11 of 432 pixels differ by more
    than 1e-4 in N) another way.  On the Cartesian grid the walk is continuous: 6.86e-6 in I and N, 1.01e-6 max|I| in Q, U.
    The bounds are twice the measured values."""
    worst = {False: [0.0, 0.0, 0.0], True: [0.0, 0.0, 0.0]}
    for name, k in hc.CASES.items():
        L, S = run_case("libm", name), run_case("soc", name)
        assert np.array_equal(L[3] > 0.0, S[3] > 0.0) and np.array_equal(L[0] > 0.0, S[0] > 0.0)
        if not (L[0] > 0.0).any():
            continue
        w = worst[hc.model(k["model"])["cloud"].LEVELS > 1]
        nz = L[0] > 0.0
        w[0] = max(w[0], float(np.max(np.abs(S[0][nz].astype(np.float64) / L[0][nz] - 1.0))))
        nz = L[3] > 0.0
        w[1] = max(w[1], float(np.max(np.abs(S[3][nz].astype(np.float64) / L[3][nz] - 1.0))))
        w[2] = max(w[2], float(np.max(np.abs(S[1:3].astype(np.float64) - L[1:3])) / np.abs(L[0]).max()))
    print("soc against libm, Cartesian: rel I %.3e, rel N %.3e, |dQ|,|dU| / max|I| %.3e" % tuple(worst[False]))
    print("soc against libm, octrees:   rel I %.3e, rel N %.3e, |dQ|,|dU| / max|I| %.3e" % tuple(worst[True]))
    assert worst[False][0] <= 2 * 6.86e-6 and worst[False][1] <= 2 * 6.86e-6 and worst[False][2] <= 2 * 1.01e-6
    assert worst[True][0] <= 2 * 1.54e-3 and worst[True][1] <= 2 * 8.43 and worst[True][2] <= 2 * 1.63e-3


def test_a_ray_that_cycles_is_ended():
    """From the centre of oct8 three rays of the reference's walk never leave (hpolmap_cases.py; with libm's last bits -- the
    walk is chaotic there, soc_math.h's send those rays out): the restatement, like the kernel, ends them after 2^15 steps
    and still returns finite planes"""
    m = hc.model("oct8")
    c = m["cloud"]
    MAP, NST = hpolmap_host.polmap("libm", c, m["B"], m["EMIT"], hc.NSIDE, (4.0, 4.0, 4.0), m["ABS"], m["SCA"], steps=True)
    assert NST.max() == 1 << 15 and 0 < (NST == 1 << 15).sum() < 10 and np.isfinite(MAP).all()


def test_restatement_refuses_what_the_kernel_refuses():
    m = hc.model("oct8")
    for mode in (1, 2, 4, -1):
        with pytest.raises(ValueError):
            hpolmap_host.polmap("soc", m["cloud"], m["B"], m["EMIT"], 2, (4.3, 3.6, 4.2), 1e-5, 1e-5, interpolate=mode)


# ---- the Healpix FITS table ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nside", [6, 16])
def test_healpix_fits_structure_and_round_trip(tmp_path, nside):
    npix = 12 * nside * nside
    cols = np.random.default_rng(nside).standard_normal((4, npix)).astype(np.float32)
    path = str(tmp_path / "h.fits")
    files.write_healpix_fits(path, cols, files.HEALPIX_POL_COLUMNS, nside)
    raw = open(path, "rb").read()
    rep = 1024 if npix % 1024 == 0 else 1
    assert (rep == 1024) == (nside == 16)
    assert len(raw) % 2880 == 0 and len(raw) == 2880 + 2880 + 2880 * ((16 * npix + 2879) // 2880)
    cards = lambda block: [block[i:i + 80].decode("ascii") for i in range(0, 2880, 80)]
    prim = cards(raw[:2880])
    assert [c[:8].strip() for c in prim[:5]] == ["SIMPLE", "BITPIX", "NAXIS", "EXTEND", "END"] and prim[2][10:30].strip() == "0"
    tab = cards(raw[2880:5760])
    assert [c[:8].strip() for c in tab[:8]] == ["XTENSION", "BITPIX", "NAXIS", "NAXIS1", "NAXIS2", "PCOUNT", "GCOUNT", "TFIELDS"]
    assert tab[0][10:20] == "'BINTABLE'"
    hdr, names, data = files.read_healpix_fits(path)
    assert names == ["I_STOKES", "Q_STOKES", "U_STOKES", "N"] and np.array_equal(data.view(np.uint32), cols.view(np.uint32))
    assert hdr["PIXTYPE"] == "HEALPIX" and hdr["ORDERING"] == "RING" and hdr["COORDSYS"] == "G" and hdr["INDXSCHM"] == "IMPLICIT"
    assert hdr["NSIDE"] == nside and hdr["FIRSTPIX"] == 0 and hdr["LASTPIX"] == npix - 1
    assert hdr["NAXIS1"] == 16 * rep and hdr["NAXIS2"] == npix // rep and hdr["TFORM1"] == ("1024E" if rep > 1 else "E")
    # big-endian, row-major: the first row holds the first `rep` values of column 1, then of column 2
    first = np.frombuffer(raw, ">f4", 2 * rep, 5760)
    assert np.array_equal(first[:rep], cols[0, :rep]) and np.array_equal(first[rep:], cols[1, :rep])
    with pytest.raises(files.FileError):
        files.write_healpix_fits(path, cols[:, :-1], files.HEALPIX_POL_COLUMNS, nside)


# ---- host path -------------------------------------------------------------------------------------------------------------

HP = "mapping 6 -1 1.0\nperspective 3.3 2.6 3.2\n"


def _model(tmp_path, extra="", levels=1):
    d = str(tmp_path)
    cloud = synth.octree_cloud(6, levels=levels, frac=0.1, seed=9) if levels > 1 else synth.cartesian_cloud(6, seed=9)
    B = synth.magnetic_field(cloud, seed=2)
    T = np.random.default_rng(8).uniform(10.0, 18.0, cloud.CELLS).astype(np.float32)
    ini = write_model(d, cloud, B, extra=HP + extra, T=T)
    os.chdir(d)
    return d, cloud, B, T, ini


def _run(ini):
    eng = HPolOracleEngine("soc")
    run = AbsorptionRun(User(ini), eng, verbose=0)
    run.setup_engine()
    _, EMITTED = run.emission_from_temperature_file()
    return run, eng, EMITTED, run.write_healpix_polmaps(EMITTED)


def test_files_frequencies_and_switches(tmp_path):
    ini0 = "p0 0.123456\ninterpolate 2\nyshear 1.5\nthreshold 0\n"
    d, cloud, B, T, ini = _model(tmp_path, extra=ini0)
    text = open(ini).read().replace("polmap %s/bx.bin %s/by.bin %s/bz.bin" % (d, d, d), "polmap %s/bx.bin %s/by.bin %s/bz.bin 0.123456 7.77777" % (d, d, d))
    with open(ini, "w") as fp:
        fp.write(text)
    run, eng, EMITTED, names = _run(ini)
    assert names == ["pol_healpix.fits.0", "pol_healpix.fits.1", "pol_healpix.fits.2"]     # every frequency, no `mapum` here
    assert len(eng.hpolmap_calls) == 3 and eng.polmap_calls == [] and eng.B is None
    call = eng.hpolmap_calls[1]
    assert call["p0"] == 0.1235 and call["minlos"] == 1.235e-01 and call["maxlos"] == 7.778 and call["y_shear"] == 1.5
    assert call["interpolate"] == 2 and call["polred"] == 0 and call["NSIDE"] == 6 and call["INTOBS"] == (3.3, 2.6, 3.2)
    for k in range(3):
        assert np.array_equal(call["B"][k], B[k])
    KK = (1.0e23 / launch.FACTOR) * launch.PLANCK / (4.0 * np.pi) * (0.5 * launch.PARSEC)
    assert np.array_equal(call["EMIT"], np.asarray(KK * float(run.FFREQ[1]) * EMITTED[:, 1], np.float32))
    assert call["LENGTH"] == launch.kernel_literals(0.5)[1]
    hdr, cols, data = files.read_healpix_fits(os.path.join(d, names[1]))
    want = hpolmap_host.polmap("soc", cloud, B, call["EMIT"], 6, (3.3, 2.6, 3.2), call["ABS"], call["SCA"], p0=0.1235, interpolate=2,
                               minlos=0.1235, maxlos=7.778, y_shear=1.5, LENGTH=call["LENGTH"])
    assert cols == ["I_STOKES", "Q_STOKES", "U_STOKES", "N"] and hdr["NSIDE"] == 6 and hpolmap_host.same_bits(data, want)
    assert (want[0] > 0).all() and (np.abs(want[1]) <= want[0]).all()
    # `wavelength` selects; `mapum` does not (ASOC.py:3911-3918)
    with open(ini, "a") as fp:
        fp.write("wavelength 150 250\nmapum 100.5\n")
    for n in names:
        os.remove(n)
    assert _run(ini)[3] == ["pol_healpix.fits.1"]


def test_nomap_suppresses_them_and_the_run_writes_them(tmp_path):
    d, cloud, B, T, ini = _model(tmp_path, extra="wavelength 90 110\n")
    AbsorptionRun(User(ini), HPolOracleEngine("soc"), verbose=0).run()
    assert os.path.exists(os.path.join(d, "pol_healpix.fits.2")) and os.path.exists(os.path.join(d, "map_dir_00_H.bin"))
    assert not [f for f in os.listdir(d) if f.startswith("polmap_")]                         # no flat polarisation maps
    os.remove(os.path.join(d, "pol_healpix.fits.2"))
    with open(ini, "a") as fp:
        fp.write("nomap\n")
    AbsorptionRun(User(ini), HPolOracleEngine("soc"), verbose=0).run()
    assert not os.path.exists(os.path.join(d, "pol_healpix.fits.2"))                          # unlike the flat ones (ASOC.py:3808)


def test_polred_encoding_of_the_healpix_branch(tmp_path):
    """ASOC.py:3867-3869: R from a file is not clipped and nothing is added under the root; the flat branch does both"""
    d, cloud, B, T, ini = _model(tmp_path)
    Rfile = np.random.default_rng(4).uniform(-0.2, 1.2, cloud.CELLS).astype(np.float32)
    np.concatenate([np.asarray([cloud.CELLS], np.int32).view(np.float32), Rfile]).tofile(os.path.join(d, "R.bin"))
    with open(ini, "a") as fp:
        fp.write("polred %s\n" % os.path.join(d, "R.bin"))
    run, eng, _, _ = _run(ini)
    call = eng.hpolmap_calls[0]
    assert call["polred"] == 1
    BB = [b.copy() for b in B]
    R = Rfile / np.sqrt(BB[0] ** 2 + BB[1] ** 2 + BB[2] ** 2)
    flat = run.polarisation_field()
    for k in range(3):
        assert np.array_equal(call["B"][k], np.asarray(BB[k] * R, np.float32))
        assert not np.array_equal(call["B"][k], flat[k])
    length = np.sqrt(sum(b.astype(np.float64) ** 2 for b in call["B"]))
    assert length.max() > 1.0 and np.allclose(length, np.abs(Rfile), rtol=1e-5)              # |R| > 1 survives: not clipped


def test_refusals(tmp_path):
    d, cloud, B, T, ini = _model(tmp_path)
    base = open(ini).read()

    def reason(extra, engine=None, text=None):
        with open(ini, "w") as fp:
            fp.write((base if text is None else text) + extra)
        with pytest.raises(UnsupportedOption) as e:
            AbsorptionRun(User(ini), HPolOracleEngine("soc") if engine is None else engine, verbose=0)
        return str(e.value)

    r = reason("", engine=PolOracleEngine("soc"))                                            # an engine without the method
    assert "Healpix" in r and "polmap_healpix" in r
    assert "polstat 1 with a Healpix map" in reason("polstat 1\n") and ":928" in reason("polstat 1\n")
    assert "polstat 3 with a Healpix map" in reason("polstat 3\n")
    assert "polstat 2" in reason("polstat 2\n")
    assert "interpolate 4" in reason("interpolate 4\n") and "interpolate -1" in reason("interpolate -1\n")
    assert "yshear" in reason("yshear 2.5\n") and "maxlos" in reason("yshear 2.5\n")
    assert "libmaps" in reason("libmaps lib.txt\n")
    # interpolate 1 and 2 on a hierarchy: known once the cloud is read
    oct6 = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    oct6.write(os.path.join(d, "m.cloud"))
    for k, b in zip("xyz", synth.magnetic_field(oct6, seed=2)):
        files.write_temperature(os.path.join(d, "b%s.bin" % k), oct6, b)
    files.write_temperature(os.path.join(d, "m.T"), oct6, np.full(oct6.CELLS, 12.0, np.float32))
    assert "hierarchy" in reason("interpolate 1\n") and "hierarchy" in reason("interpolate 2\n")
    for extra in ("", "interpolate 3\n", "threshold 1\n"):
        with open(ini, "w") as fp:
            fp.write(base + extra)
        AbsorptionRun(User(ini), HPolOracleEngine("soc"), verbose=0)
    cloud.write(os.path.join(d, "m.cloud"))
    for k, b in zip("xyz", B):
        files.write_temperature(os.path.join(d, "b%s.bin" % k), cloud, b)
    files.write_temperature(os.path.join(d, "m.T"), cloud, T)
    # ... and the accepted forms are accepted: yshear with a finite maxlos, every interpolation on a Cartesian grid
    for extra, text in (("interpolate 1\n", None), ("interpolate 2\n", None), ("polred adhoc\n", None),
                        ("yshear 2.5\n", base.replace("/bz.bin\n", "/bz.bin 20\n"))):
        with open(ini, "w") as fp:
            fp.write((base if text is None else text) + extra)
        AbsorptionRun(User(ini), HPolOracleEngine("soc"), verbose=0)


# ---- a check that needs no reference -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["libm", "soc"])
def test_uniform_cloud_with_a_uniform_field_along_z(mode):
    """Uniform density, emission and field B = z, the observer at the centre of an 8^3 cube.  Psi is measured from north
    (HDE) and B projects onto the meridian, so 2 Psi = pi + 0 or 2 pi: sin(2 Psi) = 0 and U vanishes up to the rounding of
    Psi (2^-23 rad in a float near pi/2, doubled) -- |U| <= 1e-6 I.  Q = -p cc I' has one sign everywhere; cc = cos^2 of the
    angle between B and the plane of the sky = sin^2(theta): largest on the equator, -> 0 at the poles.  With p = 0.2:
    Q/I = -p cc / (1 - p (cc - 2/3)), which is -0.2/0.9333 = -0.2143 on the equator; the pixel centres nearest the poles
    of NSIDE 6 lie at cos(theta) = 1 - 1/108, cc = 0.0184, |Q/I| = 0.0033."""
    N = 8
    cloud = synth.cartesian_cloud(N, seed=3)
    cloud.DENS[:] = 1.0
    B = [np.zeros(cloud.CELLS, np.float32), np.zeros(cloud.CELLS, np.float32), np.ones(cloud.CELLS, np.float32)]
    EMIT = np.full(cloud.CELLS, 1.0e-3, np.float32)
    MAP = hpolmap_host.polmap(mode, cloud, B, EMIT, hc.NSIDE, (4.0, 4.0, 4.0), 4.0e-5, 6.0e-5, p0=0.2)
    I, Q, U = (MAP[k].astype(np.float64) for k in range(3))
    assert (I > 0).all() and (MAP[3] > 0).all()
    assert np.abs(U / I).max() <= 1.0e-6
    assert (Q < 0).all()
    nside = hc.NSIDE
    ncap = 2 * nside * (nside - 1)
    equator = slice(ncap + 4 * nside * nside, ncap + 4 * nside * (nside + 1))                # the ring at z = 0 (ring 2 NSIDE)
    assert np.allclose(Q[equator] / I[equator], -0.2 / (1.0 - 0.2 * (1.0 - 0.6666667)), rtol=2e-4)
    poles = np.r_[0:4, 12 * nside * nside - 4:12 * nside * nside]
    assert (np.abs(Q[poles] / I[poles]) < 0.004).all() and (np.abs(Q[poles] / I[poles]) > 0.002).all()
    ratio = np.abs(Q / I)
    assert ratio[equator].min() > 10 * ratio[poles].max()
