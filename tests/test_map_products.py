"""Every map product of soc_amd.maps.MapProducts, pinned byte for byte: for each case the sha256 of every file the run leaves and
of the sequence of engine calls that made them (method name and a digest of its arguments) must equal tests/golden/map_products.json.
The engines are the CPU stand-ins of the other map tests in mode "soc" (no libm).  The fixture is rewritten by

    python tests/test_map_products.py --record

and was recorded before the map code moved out of AbsorptionRun: the public methods kept their names, so this file runs on both
sides of that move."""
import hashlib
import json
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))

from hpolmap_engine import HPolOracleEngine
from levelmap_engine import LevelOracleEngine
from maplevels_engine import LevelsOracleEngine
from polmap_engine import PolOracleEngine
from soc_amd import files, synth
from soc_amd.asoc import AbsorptionRun
from soc_amd.ini import User
from test_fastmap import TWO_DIRECTIONS, BlockOracleEngine, _model, _products

GOLDEN = os.path.join(HERE, "golden", "map_products.json")

RECORDED = ("map", "map_block", "map_block_levels", "map_levels", "set_map_block", "read_opt", "set_bfield", "polmap", "polmap_healpix",
            "ps_tau")


def _feed(h, a):
    """one argument into the digest: arrays (lists and tuples of numbers included) with dtype, shape and bytes, scalars by value"""
    if a is None:
        h.update(b"N")
    elif isinstance(a, (bool, int, np.integer)):
        h.update(b"i%d;" % int(a))
    elif isinstance(a, (float, np.floating)):
        h.update(b"f" + struct.pack("<d", float(a)))
    else:
        a = np.ascontiguousarray(a)
        assert a.dtype != object, "an argument the digest does not know"
        h.update(("a%s%s" % (a.dtype.str, a.shape)).encode() + a.tobytes())


class Recorder:
    """The engine with a log of the map-side calls: [(method, sha256 of its arguments)] in call order.  Everything else, and what
    the stand-ins call on themselves, goes straight to the engine."""

    def __init__(self, engine):
        self._engine = engine
        self.calls = []

    def __getattr__(self, name):
        attr = getattr(self._engine, name)
        if not (name in RECORDED or name.startswith("set_optical")):
            return attr

        def call(*a, **kw):
            h = hashlib.sha256()
            for x in a:
                _feed(h, x)
            for k in sorted(kw):
                h.update(k.encode() + b"=")
                _feed(h, kw[k])
            self.calls.append((name, h.hexdigest()))
            return attr(*a, **kw)
        return call


def _field(d, cloud):
    """the magnetic-field files of polmap_engine.write_model; returns the ini line that names them"""
    for name, b in zip("xyz", synth.magnetic_field(cloud, seed=2)):
        files.write_temperature(os.path.join(d, "b%s.bin" % name), cloud, b)
    return "polmap %s/bx.bin %s/by.bin %s/bz.bin\n" % (d, d, d)


def _polred_file(d, cloud):
    R = np.random.default_rng(4).uniform(-0.2, 1.2, cloud.CELLS).astype(np.float32)
    np.concatenate([np.asarray([cloud.CELLS], np.int32).view(np.float32), R]).tofile(os.path.join(d, "R.bin"))
    return "polred %s/R.bin\n" % d


def _point_source(d, cloud):
    np.asarray([1e20, 2e20, 1.5e20], np.float32).tofile(os.path.join(d, "ps.bin"))
    return "pointsource 3.3 3.2 3.1 %s/ps.bin\npspackets 4000\nglobal 128\n" % d


def _with_R(method):
    """after the run: the polarisation maps once more, with the reduction factors of an emission stage, R[CELLS, frequencies]"""
    def again(run):
        R = np.random.default_rng(6).uniform(0.05, 0.95, run.EMITTED.shape).astype(np.float32)
        assert getattr(run, method)(run.EMITTED, R=R)
    return again


HEALPIX = "perspective 0.5 3.1 2.9\n"
POLVIEW = "direction 50 35\ndirection 90 0\n"
FITS = "direction 30 40\nfits 83.8 -5.4 img\nmapum 0.641\nsavetau {d}/sv -1 0.75\ndistance 400\n"

# name: (engine, mapping, further lines, keywords); {d} in the lines is the run directory.  Keywords: abundances -- the model
# gets an abundance file; files -- functions (d, cloud) that write further inputs and return their ini lines; after -- called
# with the finished run
CASES = {
    # flat maps, one walk per frequency
    "flat": (BlockOracleEngine, "mapping 12 10 0.8", TWO_DIRECTIONS, {}),
    "flat_savetau": (BlockOracleEngine, "mapping 12 10 0.8", TWO_DIRECTIONS + "savetau {d}/sv -1 0.641\n", {}),
    "flat_fits": (BlockOracleEngine, "mapping 12 10 0.8", FITS, {}),
    "flat_perspective": (BlockOracleEngine, "mapping 12 10 0.8", "direction 30 40\nperspective 0.5 3.1 2.9\nmapint 1\n", {}),
    "flat_abu": (BlockOracleEngine, "mapping 12 10 0.8", TWO_DIRECTIONS, dict(abundances=True)),
    "pssavetau": (BlockOracleEngine, "mapping 12 10 0.8", TWO_DIRECTIONS + "pssavetau {d}/pst 0.64\n", dict(files=[_point_source])),
    # Healpix maps
    "healpix": (BlockOracleEngine, "mapping 4 -1 1.0", HEALPIX, {}),
    "healpix_nf3": (BlockOracleEngine, "mapping 4 -1 1.0 3", HEALPIX, {}),
    # batches of frequencies, and the per-level products
    "flat_nf2": (BlockOracleEngine, "mapping 12 10 0.8 2", TWO_DIRECTIONS, {}),
    "flat_nf2_abu": (BlockOracleEngine, "mapping 12 10 0.8 2", TWO_DIRECTIONS, dict(abundances=True)),
    "maplevels_flat": (LevelsOracleEngine, "mapping 12 10 0.8", TWO_DIRECTIONS + "maplevels 1\n", {}),
    "maplevels_healpix": (LevelsOracleEngine, "mapping 4 -1 1.0", HEALPIX + "maplevels 1\n", {}),
    "levels_999": (LevelOracleEngine, "mapping 12 10 0.8 999", TWO_DIRECTIONS, {}),
    # polarisation maps
    "polmap_polstat0": (PolOracleEngine, "mapping 12 10 0.8", POLVIEW, dict(files=[_field])),
    "polmap_polstat1": (PolOracleEngine, "mapping 12 10 0.8", POLVIEW + "polstat 1\n", dict(files=[_field])),
    "polmap_polstat3": (PolOracleEngine, "mapping 12 10 0.8", POLVIEW + "polstat 3\n", dict(files=[_field])),
    "polmap_polred_file": (PolOracleEngine, "mapping 12 10 0.8", POLVIEW, dict(files=[_field, _polred_file])),
    "polmap_polred_adhoc": (PolOracleEngine, "mapping 12 10 0.8", POLVIEW + "polred adhoc\n", dict(files=[_field])),
    "polmap_polred_rhofun": (PolOracleEngine, "mapping 12 10 0.8", POLVIEW + "polred rhofun_3e3_0.5\ndensity 2.5\n", dict(files=[_field])),
    "polmap_R": (PolOracleEngine, "mapping 12 10 0.8", POLVIEW, dict(files=[_field], after=_with_R("write_polmaps"))),
    "hpolmap": (HPolOracleEngine, "mapping 4 -1 1.0", HEALPIX, dict(files=[_field])),
    "hpolmap_R": (HPolOracleEngine, "mapping 4 -1 1.0", HEALPIX, dict(files=[_field], after=_with_R("write_healpix_polmaps"))),
}


def run_case(root, name):
    """the case in a fresh directory root/name: {"files": {name: sha256}, "calls": sha256 of the call log, "order": the methods}"""
    engine, mapping, more, kw = CASES[name]
    d = os.path.join(str(root), name)
    os.makedirs(d)
    os.chdir(d)
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)          # the cloud of test_fastmap._model
    more = more.format(d=d) + "".join(f(d, cloud) for f in kw.get("files", []))
    eng = Recorder(engine("soc"))
    run = AbsorptionRun(User(_model(d, mapping, more, kw.get("abundances", False))), eng, verbose=0)
    run.run()
    if "after" in kw:
        kw["after"](run)
    log = "".join("%s %s\n" % c for c in eng.calls)
    return dict(files=_products(d), calls=hashlib.sha256(log.encode()).hexdigest(), order=" ".join(c[0] for c in eng.calls))


@pytest.mark.parametrize("name", sorted(CASES))
def test_products_and_engine_calls_are_the_recorded_ones(tmp_path, name):
    with open(GOLDEN) as fp:
        golden = json.load(fp)
    assert name in golden, "tests/golden/map_products.json has no entry for this case"
    got, want = run_case(tmp_path, name), golden[name]
    assert got["order"] == want["order"]
    assert got["calls"] == want["calls"]
    assert sorted(got["files"]) == sorted(want["files"])
    assert got["files"] == want["files"], [f for f in want["files"] if got["files"][f] != want["files"][f]]


def test_the_fixture_holds_these_cases_and_no_others():
    with open(GOLDEN) as fp:
        assert sorted(json.load(fp)) == sorted(CASES)


if __name__ == "__main__":
    import tempfile
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_map_products.py --record")
    with tempfile.TemporaryDirectory() as root:
        golden = {name: run_case(root, name) for name in sorted(CASES)}
        os.chdir(HERE)
    with open(GOLDEN, "w") as fp:
        json.dump(golden, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print("%s: %d cases" % (GOLDEN, len(golden)))
