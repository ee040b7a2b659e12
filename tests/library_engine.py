"""A stand-in for soc_amd.lib.Engine on the CPU for the library method: the A2E solvers of the oracle (tests/oracle_engine.py)
and library_set / library_solve / library_build backed by the restatement (tests/library_host.py).  It has no resident arrays,
so soc_amd.library takes its host-array paths."""
import numpy as np

import library_host
from oracle_engine import OracleA2E


class LibraryEngine(OracleA2E):
    def __init__(self, mode="soc"):
        OracleA2E.__init__(self, mode)
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

    def close(self):
        pass
