"""Stand-ins on the CPU for the library method of a multi-dust model (soc_amd.mabu, soc_amd.driver):

MabuLibraryEngine -- the oracle-backed pipeline engine (tests/oracle_engine.py) with library_set / library_solve / library_build
backed by the restatement (tests/library_host.py), as tests/library_engine.py has them.  No resident arrays: the host paths.

ResidentLibraryStandIn -- besides, the soc_mabu_* and soc_mabu_library_* methods of soc_amd.lib.Engine restated in numpy, with a
device that holds at most `capacity` cells (DoesNotFit beyond): the device branches of mabu.solve_emission(makelib=...) and of
mabu.solve_emission_library -- their call order, the ranges after a refusal -- run without a GPU.

composition() is the look-up written out from the pinned pieces, what both paths must equal bit for bit."""
import numpy as np

import library_host
from oracle_engine import OraclePipelineEngine


class MabuLibraryEngine(OraclePipelineEngine):
    def __init__(self, mode="soc"):
        OraclePipelineEngine.__init__(self, mode)
        self.mode = mode
        self._lib = None

    def library_set(self, lib, ocol=None):
        self._lib = None if lib is None else (lib, None if ocol is None else np.asarray(ocol, np.int32))

    def library_solve(self, ABS3):
        if self._lib is None:
            raise RuntimeError("library_solve: call library_set first")
        EMI, _, miss = library_host.solve(self.mode, self._lib[0], ABS3, ocol=self._lib[1])
        return EMI, miss

    def library_build(self, N, ABS3=None, cols=None):
        assert ABS3 is not None, "no resident arrays here"
        return library_host.build(self.mode, N, ABS3)


def composition(mode, libs, ABS3, ABU, RABS3, ocol=None):
    """(SUM[n, nout], MISS[n] uint32): per dust split_absorbed, library_host.solve with missed rows zeroed, SUM += EMI * ABU[:, d]"""
    from soc_amd import mabu
    ABS3, ABU = np.ascontiguousarray(ABS3, np.float32), np.ascontiguousarray(ABU, np.float32)
    n = ABS3.shape[0]
    nout = libs[0]["E"].shape[1] if ocol is None else len(ocol)
    SUM, MISS = np.zeros((n, nout), np.float32), np.zeros(n, np.uint32)
    for d, lib in enumerate(libs):
        part = mabu.split_absorbed(ABS3, RABS3, ABU, d)
        EMI, _, miss = library_host.solve(mode, lib, part, ocol=ocol)
        EMI[miss, :] = 0.0
        SUM += EMI * ABU[:, d:d + 1]
        MISS[miss] |= np.uint32(1 << d)
    return SUM, MISS


class ResidentLibraryStandIn(MabuLibraryEngine):
    def __init__(self, capacity, mode="soc"):
        MabuLibraryEngine.__init__(self, mode)
        self.capacity, self.begun, self.open, self.lib_begun, self.lib_open = capacity, [], False, [], False

    def _refuse(self, cells):
        from soc_amd.lib import DoesNotFit
        if cells > self.capacity:
            raise DoesNotFit("%d cells need more device memory than is free (%d cells fit)" % (cells, self.capacity), self.capacity)

    # ---- soc_mabu_* (as tests/test_mabu.py's stand-in), with the two calls makelib adds
    def mabu_begin(self, cells, NFREQ, NDUST):
        assert not self.open
        self._refuse(cells)
        self.begun.append(cells)
        self.open = True
        self.ABS, self.SUM = np.zeros((cells, NFREQ), np.float32), np.zeros((cells, NFREQ), np.float32)
        self.PART = self.EM = None

    def mabu_upload(self, c0, ABS):
        self.ABS[c0:c0 + len(ABS)] = ABS

    def mabu_set_tables(self, ABU, RABS):
        self.ABU, self.RABS = np.array(ABU, np.float32), np.array(RABS, np.float64)

    def mabu_split(self, idust, clip_last=False):
        from soc_amd import mabu
        self.PART = mabu.split_absorbed(self.ABS, self.RABS, self.ABU, idust)
        if clip_last:
            self.PART[:, -1] = np.clip(self.PART[:, -1], 0.0, 0.2 * self.PART[:, -2])
        self.EM = np.zeros_like(self.PART)

    def mabu_solve_eq(self, NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT):
        _, self.EM = self.eqsolver(0, len(self.PART), NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, self.PART)

    def a2e_resident_solve(self):
        self.EM += self.a2e_solve(self.PART)

    def mabu_accumulate(self, idust):
        self.SUM += self.EM * self.ABU[:, idust:idust + 1]

    def mabu_download(self, c0, n, out=None):
        out[:] = self.SUM[c0:c0 + n]
        return out

    def mabu_end(self):
        self.open = False

    def library_build(self, N, ABS3=None, cols=None):
        if ABS3 is not None:
            return library_host.build(self.mode, N, ABS3)
        assert self.open and self.PART is not None
        return library_host.build(self.mode, N, self.PART, cols=cols)

    def mabu_gather_rows(self, idx):
        return self.EM[np.asarray(idx, np.int64)].copy()

    # ---- soc_mabu_library_*
    def mabu_library_begin(self, cells, NDUST, nout):
        assert not self.lib_open
        self._refuse(cells)
        self.lib_begun.append(cells)
        self.lib_open = True
        self.q = dict(ABS3=np.zeros((cells, 3), np.float32), libs=[None] * NDUST, ocol=[None] * NDUST, nout=nout)

    def mabu_library_set(self, idust, lib, ocol=None):
        assert (lib["E"].shape[1] if ocol is None else len(ocol)) == self.q["nout"]
        self.q["libs"][idust], self.q["ocol"][idust] = lib, ocol

    def mabu_library_upload(self, c0, ABS3):
        self.q["ABS3"][c0:c0 + len(ABS3)] = ABS3

    def mabu_library_set_tables(self, ABU, RABS3):
        assert ABU.shape == (len(self.q["ABS3"]), len(self.q["libs"])) and RABS3.shape == (3, len(self.q["libs"]))
        self.q["ABU"], self.q["RABS3"] = np.array(ABU, np.float32), np.array(RABS3, np.float64)

    def mabu_library_solve(self):
        assert all(lib is not None for lib in self.q["libs"])
        self.q["SUM"], self.q["MISS"] = composition(self.mode, self.q["libs"], self.q["ABS3"], self.q["ABU"], self.q["RABS3"], self.q["ocol"][0])

    def mabu_library_download(self, c0, n, out=None):
        if out is None:
            return self.q["SUM"][c0:c0 + n].copy()
        out[:] = self.q["SUM"][c0:c0 + n]
        return out

    def mabu_library_misses(self, c0, n):
        return self.q["MISS"][c0:c0 + n].copy()

    def mabu_library_end(self):
        self.lib_open = False
