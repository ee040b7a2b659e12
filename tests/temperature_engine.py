"""Stand-ins on the CPU for the calls that hand out dust temperatures and enthalpy-level populations (soc_amd.a2e dump=,
soc_amd.mabu / soc_amd.driver temperatures=):

TemperatureEngine -- the oracle-backed pipeline engine (tests/oracle_engine.py) with a2e_solve_dump: the emission from the oracle,
the populations from the fp32 restatement tests/a2e_rows.py::find_rows (held to the oracle's bits by tests/test_a2e_shapes.py),
clamped to [1e-35, 10] as kernel_A2E.c:101-103 clamps them.  No resident arrays: the batched route of a2e.run, the host path of mabu.

ResidentStandIn -- besides, the soc_a2e_resident_* and soc_mabu_* methods of soc_amd.lib.Engine restated in numpy, the new ones
included (a2e_resident_solve_dump, a2e_resident_keep_teq, a2e_resident_download_teq, mabu_download_t), with a device that holds at
most `capacity` cells: the resident route of a2e.run and the device branch of mabu.solve_emission run without a GPU.  The temperatures
are those the engine's own eqsolver / a2e_eqtemp return.

Hide(engine, *prefixes) -- the engine without the methods whose names start with one of the prefixes."""
import numpy as np

import a2e_rows
from oracle_engine import OraclePipelineEngine


def clamp(XL):
    """fmin(fmax(x, 1e-35f), 10.0f) (kernel_A2E.c:102)"""
    return np.fmin(np.fmax(np.asarray(XL, np.float32), np.float32(1.0e-35)), np.float32(10.0)).astype(np.float32)


def populations(NE, NFREQ, size, AF, ABS):
    """X[cells, NE] of one size: the normalised XL of find_rows, clamped"""
    return clamp(a2e_rows.find_rows(NE, NFREQ, size, AF, np.ascontiguousarray(ABS, np.float32))[2])


class TemperatureEngine(OraclePipelineEngine):
    def a2e_solve_dump(self, AABS):
        AABS = np.ascontiguousarray(AABS, np.float32)
        return self.a2e_solve(AABS), populations(self.NE, self.NFREQ, self.size, self.AF, AABS)


class Hide:
    def __init__(self, engine, *prefixes):
        self._e, self._p = engine, prefixes

    def __getattr__(self, name):
        if name.startswith(self._p):
            raise AttributeError(name)
        return getattr(self._e, name)


class ResidentStandIn(TemperatureEngine):
    def __init__(self, capacity=10 ** 9, mode="soc"):
        TemperatureEngine.__init__(self, mode)
        self.capacity, self.begun, self.open = capacity, [], False
        self.PART = self.EM = self.T = self.keep = self.TEQ = self.eq = None

    # ---- soc_a2e_resident_*
    def a2e_resident_begin(self, cells, NFREQ):
        assert not self.open and self.PART is None
        self.PART, self.EM = np.zeros((cells, NFREQ), np.float32), np.zeros((cells, NFREQ), np.float32)
        self.keep = self.TEQ = None

    def a2e_resident_upload(self, c0, AABS):
        self.PART[c0:c0 + len(AABS)] = AABS

    def a2e_resident_solve(self):
        self.EM += self.a2e_solve(self.PART)

    def a2e_resident_solve_dump(self, out=None):
        assert out is None
        emit, X = self.a2e_solve_dump(self.PART)
        self.EM += emit
        return X

    def a2e_set_eq_sizes(self, NIP, FACTOR, FREQ, AF, KABS, TTT, Emin, kE, oplgkE, GD, S_FRAC, SIZE_A=None):
        assert SIZE_A is None
        self.eq = (NIP, FACTOR, FREQ, AF, KABS, TTT, Emin, kE, oplgkE, GD, S_FRAC)

    def a2e_resident_keep_teq(self, on=True):
        assert self.PART is not None
        self.keep = bool(on)

    def a2e_resident_solve_eq(self):
        NIP, FACTOR, FREQ, AF, KABS, TTT, Emin, kE, oplgkE, GD, S_FRAC = self.eq
        n = len(self.PART)
        self.TEQ = [] if self.keep else None
        for s in range(len(AF)):
            T, emit = self.a2e_eqtemp(0, n, NIP, FACTOR, kE[s], oplgkE[s], Emin[s], FREQ, KABS[s], TTT[s], np.asarray(self.PART * AF[s], np.float32))
            self.EM += emit * (np.float32(GD) * np.float32(S_FRAC[s]))
            if self.keep:
                self.TEQ.append(np.array(T, np.float32))

    def a2e_resident_download_teq(self, slot, c0, n, out=None):
        assert self.TEQ is not None, "no temperatures are kept"
        if out is None:
            return self.TEQ[slot][c0:c0 + n].copy()
        out[:] = self.TEQ[slot][c0:c0 + n]
        return out

    def a2e_resident_download(self, c0, n, out=None):
        return self.EM[c0:c0 + n].copy()

    def a2e_resident_end(self):
        assert not self.open
        self.PART = self.EM = self.keep = self.TEQ = None

    # ---- soc_mabu_* (as tests/test_mabu.py's stand-in)
    def mabu_begin(self, cells, NFREQ, NDUST):
        from soc_amd.lib import DoesNotFit
        assert not self.open
        if cells > self.capacity:
            raise DoesNotFit("%d cells need more device memory than is free (%d cells fit)" % (cells, self.capacity), self.capacity)
        self.begun.append(cells)
        self.open = True
        self.ABS, self.SUM = np.zeros((cells, NFREQ), np.float32), np.zeros((cells, NFREQ), np.float32)
        self.PART = self.EM = self.T = self.keep = self.TEQ = None

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
        self.T, self.EM = self.eqsolver(0, len(self.PART), NE, FACTOR, kE, oplgkE, Emin, FREQ, KABS, TTT, self.PART)

    def mabu_download_t(self, c0, n, out=None):
        assert self.open and self.T is not None, "no mabu_solve_eq since mabu_begin"
        if out is None:
            return np.array(self.T[c0:c0 + n], np.float32)
        out[:] = self.T[c0:c0 + n]
        return out

    def mabu_accumulate(self, idust):
        self.SUM += self.EM * self.ABU[:, idust:idust + 1]

    def mabu_download(self, c0, n, out=None):
        out[:] = self.SUM[c0:c0 + n]
        return out

    def mabu_end(self):
        self.open = False
        self.PART = self.EM = self.T = self.keep = self.TEQ = None
