"""`maplevels 1`: the host plumbing of the per-level planes of the plain map -- the ini key, the driver's map_dir_XX_L.bin and its
refusals -- on an engine whose map_block_levels is the definition itself (tests/maplevels_engine.py: the plain map of the oracle
with the emission of the other levels set to zero).  The plain products must be, byte for byte, those of the run without the key."""
import os

import numpy as np
import pytest

from maplevels_engine import LevelsOracleEngine, masked_emission
from oracle_engine import OracleEngine
from soc_amd import files, launch, synth
from soc_amd.asoc import AbsorptionRun, UnsupportedOption
from soc_amd.ini import User
from test_fastmap import BlockOracleEngine, _products
from test_host import _write_model

KK = (1.0e23 / launch.FACTOR) * launch.PLANCK / (4.0 * np.pi) * 0.5 * launch.PARSEC      # `gridlength 0.5` of _write_model


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_parser(tmp_path):
    d = str(tmp_path)
    cloud = synth.cartesian_cloud(4, seed=1)
    neighbours = "mapping 12 10 0.8 3\nmapint 2\nmapcentre 1.5 2.5 3.5\nmapum 0.641\nlevels 7\n"
    want = User(_write_model(d, cloud, extra=neighbours))
    assert want.MAP_LEVELS == 0
    assert User(_write_model(d, cloud, extra=neighbours + "maplevels 0\n")).MAP_LEVELS == 0
    for extra in (neighbours + "maplevels 1\n", "maplevels 1\n" + neighbours):
        U = User(_write_model(d, cloud, extra=extra))
        assert U.MAP_LEVELS == 1
        assert list(U.NPIX) == [12, 10] == list(want.NPIX) and U.MAP_DX == want.MAP_DX and U.FAST_MAP == 3
        assert U.MAP_INTERPOLATION == 2 and tuple(U.MAPCENTRE) == (1.5, 2.5, 3.5) and U.LEVELS == 7
        assert np.array_equal(U.SINGLE_MAP_FREQ, want.SINGLE_MAP_FREQ) and len(U.SINGLE_MAP_FREQ) == 1
    assert User(_write_model(d, cloud, extra="maplevels 2\n")).MAP_LEVELS == 2


FREQ4 = [4.0e14, 4.677e14, 5.4e14, 6.1e14]


def _model(d, mapping, more, nfreq):
    """the octree model of tests/test_fastmap.py (emission solved on the device path); nfreq = 4 puts a fourth frequency into the
    dust, scattering-function and background files"""
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    extra = ("noabsorbed\niterations 1\ntemperature %s/T.bin\nemitted %s/em.bin\n%s\n%s" % (d, d, mapping, more))
    ini = _write_model(d, cloud, extra=extra)
    if nfreq == 4:
        with open(os.path.join(d, "m.dust"), "w") as fp:
            fp.write("eqdust\n 1.0e-7\n 1.0e-4\n4\n")
            for f in FREQ4:
                fp.write(" %.5e  0.6  %.5e  %.5e\n" % (f, 3.0e-2, 9.0e-2))
        dsc, csc = synth.hg_scattering_table(0.6, 500)
        files.write_scattering_functions(os.path.join(d, "m.dsc"), np.tile(dsc, (4, 1)), np.tile(csc, (4, 1)))
        np.asarray([1e-13, 2e-13, 1.5e-13, 1.2e-13], np.float32).tofile(os.path.join(d, "bg.bin"))
    txt = open(ini).read().replace("nosolve\n", "").replace("nomap\n", "").replace("absorbed %s/abs.data\n" % d, "")
    open(ini, "w").write(txt)
    return ini


def _run(tmp_path, name, mapping, more, engine, nfreq):
    d = str(tmp_path / name)
    os.makedirs(d)
    os.chdir(d)
    eng = engine("soc")
    run = AbsorptionRun(User(_model(d, mapping, more.format(d=d), nfreq)), eng, verbose=0)
    run.run()
    return d, run, eng


TWO = "direction 30 40\ndirection 90 0\n"
RUNS = {
    # name: (mapping, further lines, frequencies of the model, batch sizes expected, plain products that must be there)
    "two_directions": ("mapping 12 10 0.8", TWO, 3, [1, 1, 1], ["map_dir_00.bin", "map_dir_01.bin"]),
    "perspective": ("mapping 12 10 0.8", "direction 30 40\nperspective 0.5 3.1 2.9\nmapint 1\n", 3, [1, 1, 1], ["map_dir_00.bin"]),
    "healpix": ("mapping 4 -1 1.0", "perspective 0.5 3.1 2.9\nwavelength 0.6 0.8\n", 3, None, ["map_dir_00_H.bin"]),
    "batches": ("mapping 12 10 0.8 3", TWO, 4, [3, 1], ["map_dir_00.bin", "map_dir_01.bin"]),            # a full batch and a remainder
    "fits": ("mapping 12 10 0.8 2", "direction 30 40\nfits 83.8 -5.4 img\nmapum 0.641\nsavetau {d}/sv -1 0.75\ndistance 400\n", 3, [2],
             ["img_0.64.fits", "sv_tau_0.75.fits"]),
}


@pytest.mark.parametrize("name", sorted(RUNS))
def test_driver_writes_the_level_file_and_the_same_plain_files(name, tmp_path):
    mapping, more, nfreq, sizes, must = RUNS[name]
    healpix = name == "healpix"
    dp, _, _ = _run(tmp_path, "plain", mapping, more, BlockOracleEngine, nfreq)
    dl, run, eng = _run(tmp_path, "levels", mapping, more + "maplevels 1\n", LevelsOracleEngine, nfreq)
    skip = {"m.ini"}
    want = {f: h for f, h in _products(dp).items() if f not in skip}
    got = {f: h for f, h in _products(dl).items() if f not in skip}
    NDIR = 2 if more.startswith(TWO) else 1
    lfiles = ["map_dir_%02d_L.bin" % i for i in range(NDIR)]
    for f in must:
        assert f in want, (f, sorted(want))
    # the key adds the level files and changes nothing else, byte for byte
    assert sorted(set(got) - set(want)) == lfiles and not (set(want) - set(got))
    assert {f: got[f] for f in want} == want
    if sizes is not None:
        assert eng.block_sizes == sizes
    assert eng.block is None and not eng.map_inputs            # every frequency went through the batch path; the batch was freed
    # the level file: header, then per image of the plain file LEVELS planes = the definition, on the emission the driver scales
    U, cloud, FFREQ = run.U, run.cloud, run.FFREQ
    I1 = int(np.nonzero((FFREQ >= U.REMIT_F[0]) & (FFREQ <= U.REMIT_F[1]))[0][0])
    singles = np.asarray(getattr(U, "SINGLE_MAP_FREQ", []), np.float64)
    images = [i for i in range(run.NFREQ) if U.MAP_FREQ[0] <= FFREQ[i] <= U.MAP_FREQ[1] and
              (len(singles) == 0 or np.min(np.abs(FFREQ[i] - singles)) / FFREQ[i] <= 0.005)]
    assert len(images) == {"batches": 4, "fits": 1, "healpix": 2}.get(name, 3)
    _, OD, RA, DE = launch.set_observer_directions(U.OBS_THETA, U.OBS_PHI)
    centre = (0.5 * cloud.NX, 0.5 * cloud.NY, 0.5 * cloud.NZ)
    npix = 12 * 16 if healpix else 120
    ref = OracleEngine("soc")
    ref.set_cloud(cloud)
    ref.set_map_interpolation(U.MAP_INTERPOLATION)
    lit = np.zeros(cloud.LEVELS, np.int64)
    for idir, lf in enumerate(lfiles):
        head = np.fromfile(os.path.join(dl, lf), np.int32, 4)
        assert list(head) == [int(U.NPIX[0]), int(U.NPIX[1]), len(images), cloud.LEVELS]
        planes = np.fromfile(os.path.join(dl, lf), np.float32, offset=16)
        assert planes.size == len(images) * cloud.LEVELS * npix
        planes = planes.reshape(len(images), cloud.LEVELS, npix)
        for k, i in enumerate(images):
            if healpix:
                emit = np.asarray(run.EMITTED[:, i - I1] * np.float32(KK) * np.float32(float(FFREQ[i])), np.float32)
            else:
                emit = np.asarray(KK * float(FFREQ[i]) * run.EMITTED[:, i - I1], np.float32)
            ABS, SCA = run._optical_for(i)
            for l in range(cloud.LEVELS):
                m, _ = ref.map(masked_emission(cloud, emit, l), OD[idir], RA[idir], DE[idir], U.NPIX, U.MAP_DX, centre, ABS, SCA,
                               INTOBS=U.INTOBS, healpix=int(U.NPIX[0]) if healpix else 0)
                assert np.array_equal(_bits(planes[k, l]), _bits(m.ravel())), (lf, k, l)
                lit[l] += int((m > 0).sum())
            # the frequency order is the plain file's: the planes of image k add up to image k of the plain file
            if not U.FITS:
                name_, off = ("map_dir_00_H.bin", 16) if healpix else ("map_dir_%02d.bin" % idir, 8)
                img = np.fromfile(os.path.join(dl, name_), np.float32, offset=off).reshape(len(images), npix)[k]
                total = planes[k].astype(np.float64).sum(axis=0)
                assert (img > 0).sum() > 20 and (np.abs(total - img) <= 2e-6 * img).all()
    # the planes compared are not all dark: every level is lit -- but for the all-sky map, whose observer sits in a surface cell of
    # this opaque toy cloud and sees root cells only
    assert lit[0] > 5 and (healpix or (lit > 5).all()), lit


def test_refusals(tmp_path):
    d = str(tmp_path)
    cloud = synth.cartesian_cloud(4, seed=1)
    for engine in (OracleEngine, BlockOracleEngine):           # no map_block_levels
        with pytest.raises(UnsupportedOption, match="maplevels.*no kernel for it .map_block_levels"):
            AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8\nmaplevels 1\n")), engine("soc"))

    class Both(LevelsOracleEngine):                            # an engine that has the kernel of `mapping ... 999` as well
        def map_levels(self, *a, **k):
            raise AssertionError("not reached")
    for n in (999, 1000):
        with pytest.raises(UnsupportedOption, match="maplevels together with mapping with a fourth argument >= 999 .two different per-level products"):
            AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8 %d\nmaplevels 1\n" % n)), Both("soc"))
    AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8 999\nmaplevels 0\n")), Both("soc"))
    AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8 998\nmaplevels 1\n")), Both("soc"))
    AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8\nmaplevels 1\n")), LevelsOracleEngine("soc"))
