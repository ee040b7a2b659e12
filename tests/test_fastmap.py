"""`mapping nx ny dx NF` (2 <= NF <= 998): the host plumbing of the batch map path.  The driver must write, byte for byte, the files
it writes without the fourth argument -- here on an engine whose map_block is its own per-frequency map, column by column, so
that every difference would be one of batching, scaling, ordering or file code."""
import hashlib
import os

import numpy as np
import pytest

from oracle_engine import OracleEngine
from soc_amd import synth
from soc_amd.asoc import AbsorptionRun, UnsupportedOption
from soc_amd.ini import User
from test_host import _write_model


class BlockOracleEngine(OracleEngine):
    """OracleEngine with the batch calls of soc_amd.lib.Engine: set_map_block keeps the batch, map_block maps its columns one
    by one through map().  Both record what they were handed."""
    map_block_max = 4

    def __init__(self, mode="soc"):
        OracleEngine.__init__(self, mode)
        self.block = None
        self.block_sizes = []                                  # nf of every batch uploaded
        self.block_columns = []                                # per column: (EMIT, ABS, SCA, OPT or None)
        self.map_inputs = []                                   # per map() call from outside map_block: the same tuple
        self._inside = False

    def set_map_block(self, EMITX, ABS=None, SCA=None, OPT=None):
        if EMITX is None:
            self.block = None
            return
        EMITX = np.array(EMITX, np.float32)
        nf = EMITX.shape[1]
        assert EMITX.shape == (self.cloud.CELLS, nf) and 1 <= nf <= self.map_block_max
        ABS, SCA = np.array(ABS, np.float32).ravel(), np.array(SCA, np.float32).ravel()
        assert ABS.size == nf and SCA.size == nf
        OPT = None if OPT is None else np.array(OPT, np.float32)
        assert OPT is None or OPT.shape == (self.cloud.CELLS, nf, 2)
        self.block = (EMITX, ABS, SCA, OPT)
        self.block_sizes.append(nf)
        for k in range(nf):
            self.block_columns.append((EMITX[:, k].copy(), ABS[k], SCA[k], None if OPT is None else OPT[:, k, :].copy()))

    def map_block(self, DIR, RA, DE, NPIX, MAP_DX, CENTRE, INTOBS=None, LENGTH=1.0, healpix=0):
        assert self.block is not None, "map_block without a batch"
        EMITX, ABS, SCA, OPT = self.block
        keep, M, T, C = self.OPT, [], [], None
        self._inside = True
        for k in range(EMITX.shape[1]):
            self.OPT = None if OPT is None else OPT[:, k, :]
            m, t = self.map(EMITX[:, k], DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS[k], SCA[k], INTOBS=INTOBS, save_colden=0, LENGTH=LENGTH, healpix=healpix)
            M.append(m)
            T.append(t)
            if k == 0:
                _, C = self.map(EMITX[:, k], DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS[k], SCA[k], INTOBS=INTOBS, save_colden=1, LENGTH=LENGTH, healpix=healpix)
        self._inside = False
        self.OPT = keep
        return np.stack(M), np.stack(T), C

    def map(self, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, **kw):
        if not self._inside:
            self.map_inputs.append((np.array(EMIT, np.float32), np.float32(ABS), np.float32(SCA), None if self.OPT is None else np.array(self.OPT, np.float32)))
        return OracleEngine.map(self, EMIT, DIR, RA, DE, NPIX, MAP_DX, CENTRE, ABS, SCA, **kw)


def _model(d, mapping, more="", abundances=False):
    """the octree model of test_map_files_of_the_driver (three frequencies, emission solved on the device path), two directions"""
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    extra = ("noabsorbed\niterations 1\ntemperature %s/T.bin\nemitted %s/em.bin\n%s\n%s" % (d, d, mapping, more))
    ini = _write_model(d, cloud, extra=extra)
    txt = open(ini).read().replace("nosolve\n", "").replace("nomap\n", "").replace("absorbed %s/abs.data\n" % d, "")
    if abundances:
        np.asarray(np.random.default_rng(4).uniform(0.2, 1.0, cloud.CELLS), np.float32).tofile(os.path.join(d, "m.abu"))
        txt = txt.replace("optical %s/m.dust\n" % d, "optical %s/m.dust %s/m.abu\n" % (d, d))
    open(ini, "w").write(txt)
    return ini


def _products(d):
    """name -> digest of every file of the run directory except the model's own inputs"""
    skip = {"m.ini", "m.cloud", "m.dust", "m.dsc", "bg.bin", "m.abu"}
    return {f: hashlib.sha256(open(os.path.join(d, f), "rb").read()).hexdigest() for f in sorted(os.listdir(d)) if f not in skip}


def _run(tmp_path, name, mapping, more="", engine=BlockOracleEngine, abundances=False):
    d = str(tmp_path / name)
    os.makedirs(d)
    os.chdir(d)
    eng = engine("soc")
    AbsorptionRun(User(_model(d, mapping, more, abundances)), eng, verbose=0).run()
    return _products(d), eng


TWO_DIRECTIONS = "direction 30 40\ndirection 90 0\n"


def test_block_path_writes_the_same_files(tmp_path):
    """three mapped frequencies, two directions; NF = 2: a full batch and a tail of one; NF = 7: more than the engine's
    maximum of 4 and more than there are frequencies (one batch of three); NF = 4: exactly the engine's maximum"""
    want, plain = _run(tmp_path, "plain", "mapping 12 10 0.8", TWO_DIRECTIONS)
    assert "map_dir_00.bin" in want and "map_dir_01.bin" in want and not plain.block_sizes
    assert os.path.getsize(str(tmp_path / "plain" / "map_dir_00.bin")) == 8 + 3 * 120 * 4
    for NF, sizes in ((2, [2, 1]), (4, [3]), (7, [3])):
        got, eng = _run(tmp_path, "nf%d" % NF, "mapping 12 10 0.8 %d" % NF, TWO_DIRECTIONS)
        assert eng.block_sizes == sizes and not eng.map_inputs and eng.block is None
        assert got == want, NF


def test_block_path_splits_beyond_the_engine_maximum(tmp_path):
    """an engine that holds two frequencies at most cuts NF = 7 into batches of 2 and 1"""
    class Two(BlockOracleEngine):
        map_block_max = 2
    want, _ = _run(tmp_path, "plain", "mapping 12 10 0.8", TWO_DIRECTIONS)
    got, eng = _run(tmp_path, "nf7", "mapping 12 10 0.8 7", TWO_DIRECTIONS, engine=Two)
    assert eng.block_sizes == [2, 1] and got == want


@pytest.mark.parametrize("name, mapping, more, must", [
    ("savetau", "mapping 12 10 0.8", TWO_DIRECTIONS + "savetau {d}/sv -1 0.641\n", ["sv_colden_dir0_000.fits", "sv_tau_0.64_dir1_001.bin"]),
    ("fits", "mapping 12 10 0.8", "direction 30 40\nfits 83.8 -5.4 img\nmapum 0.641\nsavetau {d}/sv -1 0.75\ndistance 400\n", ["img_0.64.fits", "sv_tau_0.75.fits"]),
    ("healpix", "mapping 4 -1 1.0", "perspective 0.5 3.1 2.9\nwavelength 0.6 0.8\n", ["map_dir_00_H.bin"]),
    ("inside", "mapping 12 10 0.8", "direction 30 40\nperspective 0.5 3.1 2.9\nmapint 1\n", ["map_dir_00.bin"]),
])
def test_block_path_same_products_in_other_modes(tmp_path, name, mapping, more, must):
    want, _ = _run(tmp_path, "plain", mapping, more.format(d=str(tmp_path / "plain")))
    got, eng = _run(tmp_path, "block", mapping + " 3", more.format(d=str(tmp_path / "block")))
    for f in must:
        assert f in want, (f, sorted(want))
    assert eng.block_sizes and got == want


def test_block_path_hands_over_the_same_emission_and_opacities(tmp_path):
    """with an abundance file: every column of EMITX and OPTX, and ABS and SCA, are bit for bit what the plain path hands to
    map() (the engine's per-cell OPT at that moment included); a frequency mapped for its optical depth only is a zero column"""
    more = TWO_DIRECTIONS + "mapum 0.641\nsavetau {d}/sv 0.75\n"
    want, plain = _run(tmp_path, "plain", "mapping 12 10 0.8", more.format(d=str(tmp_path / "plain")), abundances=True)
    got, eng = _run(tmp_path, "block", "mapping 12 10 0.8 2", more.format(d=str(tmp_path / "block")), abundances=True)
    assert got == want and eng.block_sizes == [2]
    slow = plain.map_inputs[::2]                               # two directions per frequency
    assert len(slow) == len(eng.block_columns) == 2
    zero = 0
    for (E0, A0, S0, O0), (E1, A1, S1, O1) in zip(slow, eng.block_columns):
        assert np.array_equal(E0.view(np.uint32), E1.view(np.uint32))
        assert np.float32(A0).view(np.uint32) == np.float32(A1).view(np.uint32) and np.float32(S0).view(np.uint32) == np.float32(S1).view(np.uint32)
        assert O0 is not None and O1 is not None and np.array_equal(O0.view(np.uint32), O1.view(np.uint32))
        assert (O1 > 0).all()
        zero += int(not E1.any())
    assert zero == 1                                           # 0.75 um: optical depth only


def test_block_path_refusals(tmp_path):
    d = str(tmp_path)
    cloud = synth.cartesian_cloud(4, seed=1)
    with pytest.raises(UnsupportedOption):                     # an engine without the batch kernel
        AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8 2\n")), OracleEngine("soc"))
    for engine in (OracleEngine, BlockOracleEngine):           # per-level maps stay refused
        with pytest.raises(UnsupportedOption):
            AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8 999\n")), engine("soc"))
    AbsorptionRun(User(_write_model(d, cloud, extra="mapping 12 10 0.8 998\n")), BlockOracleEngine("soc"))
    for same in ("mapping 12 10 0.8 0\n", "mapping 12 10 0.8 1\n"):   # 0 and 1 stay what they are: the plain path, any engine
        AbsorptionRun(User(_write_model(d, cloud, extra=same)), OracleEngine("soc"))
