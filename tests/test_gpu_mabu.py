"""The multi-dust emission stage on the device (soc_mabu_*, soc_amd/csrc/soc_mabu.hip): the split kernel against
driver.split_absorbed to the bit, the whole stage against the host path of the same engine to the bit (one range and
several), the pipeline's report of the path it took, and the program in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

from soc_amd import files, synth                     # noqa: E402
from test_driver import NFREQ, write_case            # noqa: E402
from test_mabu import write_ini, write_third_dust    # noqa: E402

pytestmark = pytest.mark.gpu

CELLS = 3 * 256 + 77                                 # not a multiple of the workgroup (256 lanes, 1024 elements a tile)


def split_inputs(nfreq, ndust, seed, zero_column=None):
    rng = np.random.default_rng(seed)
    ABS = (rng.uniform(0.0, 1.0, (CELLS, nfreq)) * 10.0 ** rng.uniform(-12, 3, (CELLS, 1))).astype(np.float32)
    ABS[rng.uniform(size=CELLS) < 0.2] = np.float32(-1.0e20)      # parent cells, as files.scale_absorbed leaves them
    ABS[5:7, :] = 0.0                                             # (row 6 meets a zero denominator below: 0/0)
    ABU = rng.uniform(1.0e-3, 2.0, (CELLS, ndust)).astype(np.float32)
    R = rng.uniform(1.0e-3, 1.0, (nfreq, ndust)) * 10.0 ** rng.uniform(-6, 0, (nfreq, ndust))
    R = np.clip(R / R.sum(axis=1)[:, None], 1.0e-30, 1.0)
    if zero_column is not None:
        ABU[:, zero_column] = 0.0
        ABU[::3, :] = 0.0                                         # rows whose denominator is zero: x/0 and 0/0
    return ABS, ABU, R


@pytest.mark.parametrize("nfreq", [3, 50])
@pytest.mark.parametrize("ndust", [1, 2, 3])
def test_split_equals_the_host_restatement_to_the_bit(engine, nfreq, ndust):
    from soc_amd import driver
    ABS, ABU, R = split_inputs(nfreq, ndust, 100 * nfreq + ndust)
    engine.mabu_begin(CELLS, nfreq, ndust)
    try:
        engine.mabu_upload(0, ABS[:400])
        engine.mabu_upload(400, ABS[400:])
        engine.mabu_set_tables(ABU, R)
        for idust in range(ndust):
            engine.mabu_split(idust)
            got = np.concatenate([engine.mabu_read_part(0, 123), engine.mabu_read_part(123, CELLS - 123)])
            want = driver.split_absorbed(ABS, R, ABU, idust)
            assert np.isfinite(want).all()
            assert np.array_equal(got, want), (nfreq, ndust, idust, np.flatnonzero(got != want)[:8])
    finally:
        engine.mabu_end()


def test_split_divides_by_a_zero_denominator_as_ieee_does(engine):
    from soc_amd import driver
    ABS, ABU, R = split_inputs(50, 2, 7, zero_column=1)
    engine.mabu_begin(CELLS, 50, 2)
    try:
        engine.mabu_upload(0, ABS)
        engine.mabu_set_tables(ABU, R)
        for idust in range(2):
            engine.mabu_split(idust)
            got = engine.mabu_read_part(0, CELLS)
            with np.errstate(divide='ignore', invalid='ignore'):
                want = driver.split_absorbed(ABS, R, ABU, idust)
            assert np.isnan(want).any() and np.isinf(want).any()
            assert np.array_equal(got, want, equal_nan=True)
    finally:
        engine.mabu_end()


@pytest.mark.parametrize("cells, nfreq", [(45001, 50), (4200001, 3)])
def test_strided_grids_equal_the_host_to_the_bit(engine, cells, nfreq):
    """Sizes at which a workgroup takes more than one tile: the streaming kernels launch at most 2048 workgroups of 1024 elements
    (45001 x 50 is 2198 tiles, 4200001 x 3 is 12305; neither NFREQ divides 1024 and both arrays end inside a float4), the clip
    kernel at most 16384 workgroups of 256 cells (4194304 cells).  Split, clip and sum against numpy, as production sizes run them."""
    from soc_amd import driver
    rng = np.random.default_rng(cells)
    ABS = (rng.uniform(0.0, 1.0, (cells, nfreq)) * 10.0 ** rng.uniform(-12, 3, (cells, 1))).astype(np.float32)
    ABS[rng.uniform(size=cells) < 0.1] = np.float32(-1.0e20)
    ABU = rng.uniform(1.0e-3, 2.0, (cells, 2)).astype(np.float32)
    R = rng.uniform(1.0e-3, 1.0, (nfreq, 2))
    R = np.clip(R / R.sum(axis=1)[:, None], 1.0e-30, 1.0)
    FREQ = np.logspace(11.5, 15.0, nfreq).astype(np.float32)
    KABS = (1.0e-22 * (FREQ / 1.0e13) ** 1.5).astype(np.float32)
    TTT = np.linspace(3.0, 1500.0, 200).astype(np.float32)
    want_sum = np.zeros((cells, nfreq), np.float32)
    engine.mabu_begin(cells, nfreq, 2)
    try:
        engine.mabu_upload(0, ABS)
        engine.mabu_set_tables(ABU, R)
        for idust in range(2):
            engine.mabu_split(idust, clip_last=bool(idust))
            want = driver.split_absorbed(ABS, R, ABU, idust)
            if idust:                                             # A2E.py:184-185, the line of soc_amd.a2e.run
                want[:, nfreq - 1] = np.clip(want[:, nfreq - 1], 0.0, 0.2 * want[:, nfreq - 2])
            got = engine.mabu_read_part(0, cells)
            assert np.array_equal(got, want), (idust, np.flatnonzero((got != want).any(axis=1))[:8])
            del got, want
            engine.mabu_solve_eq(TTT.size, 1.0e20, 1.05, 1.0 / np.log10(1.05), 1.0e-12, FREQ, KABS, TTT)
            em = engine.a2e_resident_download(0, cells, out=np.zeros((cells, nfreq), np.float32))   # (rows of EM: include/soc_hip.h)
            assert np.isfinite(em).all() and (em > 0).any()
            engine.mabu_accumulate(idust)
            want_sum += em * ABU[:, idust:idust + 1]
            got = engine.mabu_download(0, cells)
            assert np.array_equal(got, want_sum), (idust, np.flatnonzero((got != want_sum).any(axis=1))[:8])
    finally:
        engine.mabu_end()


def test_binding_refuses_what_the_library_cannot_check(engine):
    from soc_amd.lib import SocError
    with pytest.raises(SocError, match="mabu_begin first"):
        engine.mabu_download(0, 1)
    with pytest.raises(SocError, match="mabu_begin first"):
        engine.mabu_set_tables(np.ones((1, 1), np.float32), np.ones((2, 1)))
    engine.mabu_begin(10, 4, 2)
    try:
        with pytest.raises(SocError, match=r"shape \(5, 3\)"):
            engine.mabu_upload(0, np.zeros((5, 3), np.float32))           # narrower rows: the library would read past the array
        with pytest.raises(SocError, match="C-contiguous float32"):
            engine.mabu_download(0, 5, out=np.zeros((5, 4), np.float64))
        with pytest.raises(SocError, match="C-contiguous float32"):
            engine.mabu_download(0, 5, out=np.zeros((5, 8), np.float32)[:, ::2])
    finally:
        engine.mabu_end()
    engine.a2e_resident_begin(10, 4)
    try:
        with pytest.raises(SocError, match="soc_a2e_resident_end first"):
            engine.mabu_begin(10, 4, 2)
        with pytest.raises(SocError, match=r"shape \(5, 3\)"):
            engine.a2e_resident_upload(0, np.zeros((5, 3), np.float32))   # narrower rows: the library would read past the array
        readonly = np.zeros((5, 4), np.float32)
        readonly.flags.writeable = False
        for out in (np.zeros((5, 4), np.float64), np.zeros((5, 8), np.float32)[:, ::2], readonly, np.zeros((4, 4), np.float32),
                    np.zeros((5, 5), np.float32), np.zeros(20, np.float32)):   # the library would write 5 x 4 floats to any of them
            with pytest.raises(SocError, match=r"writeable C-contiguous float32 array of shape \(5, 4\)"):
                engine.a2e_resident_download(0, 5, out=out)
        assert not readonly.any() and engine.a2e_resident_download(0, 5, out=np.ones((5, 4), np.float32)).sum() == 0
    finally:
        engine.a2e_resident_end()


REFUSED = [(8, 4), (10, 1), (-1, 1), (0, 0)]         # rows [c0, c0 + n) of 10: past the end, from the end on, from before the first, none
ACCEPTED = [(9, 1), (0, 10)]


def rows_are_checked(upload, download, want=None):
    """every range of REFUSED through the two calls (either may be None) is refused with the library's text, every one of ACCEPTED is
    taken; the rows that come down are those that went up -- or, with no upload, `want` -- to the bit"""
    from soc_amd.lib import SocError
    rows = np.random.default_rng(10).integers(0, 2 ** 32, (10, 4), dtype=np.uint64).astype(np.uint32).view(np.float32) if want is None else want
    for c0, n in REFUSED:
        for call in ([lambda: upload(c0, np.zeros((n, 4), np.float32))] if upload else []) + ([lambda: download(c0, n)] if download else []):
            with pytest.raises(SocError, match=r"cells \[%d, %d\) of 10" % (c0, c0 + n)):
                call()
    for c0, n in ACCEPTED:
        if upload:
            upload(c0, rows[c0:c0 + n])
        if download:
            got = download(c0, n)
            assert got.shape == (n, 4) and np.array_equal(got.view(np.uint32), rows[c0:c0 + n].view(np.uint32)), (c0, n)


def test_every_transfer_call_checks_its_rows(engine):
    """10 cells, 4 frequencies, 2 dusts, polarised: the one range check of the library (SOC_ROWS) as every transfer call makes it"""
    from soc_amd import mabu
    from soc_amd.lib import SocError
    zero = np.zeros((10, 4), np.float32)
    engine.a2e_resident_begin(10, 4, polarised=True)
    try:
        rows_are_checked(engine.a2e_resident_upload, None)
        rows_are_checked(None, engine.a2e_resident_download, zero)         # (the sums of a block just opened)
        rows_are_checked(None, engine.a2e_resident_download_p, zero)
        for c0, n in REFUSED[:3]:
            with pytest.raises(SocError, match=r"cells \[%d, %d\) of 10" % (c0, c0 + n)):
                engine.a2e_resident_upload_aalg(c0, np.ones(n, np.float32))
        with pytest.raises(SocError, match="one value per cell"):
            engine.a2e_resident_upload_aalg(0, np.ones(0, np.float32))
        for c0, n in ACCEPTED:
            engine.a2e_resident_upload_aalg(c0, np.ones(n, np.float32))
    finally:
        engine.a2e_resident_end()
    engine.mabu_begin(10, 4, 2, polarised=True)
    try:
        rows_are_checked(engine.a2e_resident_upload, engine.mabu_read_part)   # (the dust's share: what a2e_resident_upload fills)
        rows_are_checked(None, engine.mabu_download, zero)
        rows_are_checked(None, engine.mabu_download_p, zero)
        ABS, ABU, R = split_inputs(4, 2, 11)
        ABS, ABU = ABS[:10], ABU[:10]
        rows_are_checked(engine.mabu_upload, None, ABS)
        engine.mabu_set_tables(ABU, R)
        engine.mabu_split(1)                                                  # ... and the rows that went up are those it splits
        assert np.array_equal(engine.mabu_read_part(0, 10), mabu.split_absorbed(ABS, R, ABU, 1), equal_nan=True)
    finally:
        engine.mabu_end()
    engine.set_grid(5, 2, 1, 1, [10], np.ones(10, np.float32))
    engine.emitted_begin(4)
    try:
        rows_are_checked(engine.emitted_upload, engine.emitted_download)
    finally:
        engine.emitted_end()
    engine.absorbed_begin(4)
    try:
        rows_are_checked(None, engine.absorbed_download, zero)
    finally:
        engine.absorbed_end()


def test_calls_out_of_order_and_out_of_range_are_refused(engine):
    from soc_amd.lib import SocError
    with pytest.raises(SocError, match="soc_mabu_begin first"):
        engine.mabu_split(0)
    engine.mabu_begin(10, 4, 2)
    try:
        with pytest.raises(SocError, match="soc_mabu_set_tables first"):
            engine.mabu_split(0)
        with pytest.raises(SocError, match=r"cells \[8, 12\) of 10"):
            engine.mabu_upload(8, np.zeros((4, 4), np.float32))
        with pytest.raises(SocError, match="soc_mabu_end"):
            engine.a2e_resident_begin(10, 4)
        engine.mabu_set_tables(np.ones((10, 2), np.float32), np.full((4, 2), 0.5))
        with pytest.raises(SocError, match="dust 2 of 2"):
            engine.mabu_split(2)
    finally:
        engine.mabu_end()
    test_every_transfer_call_checks_its_rows(engine)             # (the ranges of every transfer call: the test above, here in its order)


@pytest.fixture(scope="module")
def model(tmp_path_factory, engine):
    """the dust files of tests/test_driver.py::write_case plus a third dust, and the absorptions of that pipeline on the GPU"""
    from soc_amd import driver
    d = str(tmp_path_factory.mktemp("gpumabu"))
    cloud = synth.octree_cloud(6, levels=2, frac=0.1, seed=9)
    ini, sol, abu = write_case(d, cloud)
    carb = write_third_dust(d, cloud.CELLS)
    cwd = os.getcwd()
    os.chdir(d)
    try:
        P = driver.Pipeline(ini, engine, verbose=0)
        CTABS, FABS, EMITTED = P.run(keep_files=True)
    finally:
        os.chdir(cwd)
        engine.set_exec(-1, 4)
    three = write_ini(d, "three.ini", ["%s/sil.dust %s/sil.abu" % (d, d), "%s/gs_pah.dust" % d, "%s/carb.dust %s/carb.abu" % (d, d)])
    dusts3 = [os.path.join(d, x) for x in ("sil.dust", "gs_pah.dust", "carb.dust")]
    return dict(d=d, ini=ini, three=three, cloud=cloud, FABS=FABS, EMITTED=EMITTED, timers=dict(P.timers),
                cases={2: (dusts3[:2], np.stack([abu, np.ones_like(abu)], axis=1)),
                       3: (dusts3, np.stack([abu, np.ones_like(abu), carb], axis=1))})


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_pipeline_reports_the_device_path(model):
    assert model["timers"]["emission_path"] == "device"
    assert (model["EMITTED"][model["cloud"].DENS > 0] > 0).any()


@pytest.mark.parametrize("ndust", [2, 3])
def test_device_path_equals_the_host_path_to_the_bit(engine, model, ndust):
    from soc_amd import mabu
    dusts, ABU = model["cases"][ndust]
    kinds = [mabu.dust_kind(x) for x in dusts]
    assert kinds[:2] == ['eqdust', 'gsetdust']
    host, hi = mabu.solve_emission(engine, dusts, kinds, model["FABS"], ABU, path='host')
    dev, di = mabu.solve_emission(engine, dusts, kinds, model["FABS"], ABU)
    assert (hi["path"], di["path"], di["ranges"]) == ("host", "device", 1)
    leaf = model["cloud"].DENS > 0
    assert (host[leaf] > 0).any() and np.isfinite(host[leaf]).all()
    diff = np.flatnonzero(host.view(np.uint32) != dev.view(np.uint32))
    print("ndust %d: %d of %d values differ in their bits" % (ndust, diff.size, host.size))
    assert same_bits(dev, host)
    if ndust == 2:
        assert same_bits(dev, model["EMITTED"])                    # what the pipeline returned


def test_cell_ranges_give_the_bits_of_one_range(engine, model):
    from soc_amd import mabu
    dusts, ABU = model["cases"][3]
    kinds = [mabu.dust_kind(x) for x in dusts]
    one, i1 = mabu.solve_emission(engine, dusts, kinds, model["FABS"], ABU)
    many, im = mabu.solve_emission(engine, dusts, kinds, model["FABS"], ABU, range_cells=100)
    assert i1["ranges"] == 1 and im["ranges"] == (model["cloud"].CELLS + 99) // 100 and im["ranges"] > 2
    assert same_bits(many, one)
    # two ranks' shares put together are the whole
    parts = [mabu.solve_emission(engine, dusts, kinds, model["FABS"], ABU, r, 2)[0] for r in (0, 1)]
    assert same_bits(np.concatenate(parts), one)


def test_program_in_a_child_process_writes_what_the_stage_gives(engine, model):
    from soc_amd import mabu
    d = model["d"]
    dusts, ABU = model["cases"][3]
    kinds = [mabu.dust_kind(x) for x in dusts]
    want, _ = mabu.solve_emission(engine, dusts, kinds, model["FABS"], ABU)
    out = os.path.join(d, "emitted_child.data")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "soc_amd.mabu", model["three"], os.path.join(d, "abs.data"), out],
                       env=env, cwd=d, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device path" in r.stdout
    assert list(np.fromfile(out, np.int32, 2)) == list(want.shape)
    got = np.asarray(files.mmap_emitted(out, want.shape[0], NFREQ))
    assert same_bits(got, want)
