#!/usr/bin/env python3
"""library -- the library method for the emission of stochastically heated grains on MI355X:

    python -m soc_amd.library  gpu_tag  solver  absorbed                   # build  <solver>.lib
    python -m soc_amd.library  gpu_tag  solver  absorbed  emitted [ofreq]  # solve with it

Drop-in for ``soc_library.py`` of the reference.  A model is simulated at three reference frequencies only (`libabs` of
soc_amd.asoc); the emission of a cell is looked up in an N x N x N table indexed by the log-absorptions at those frequencies,
built once from a run with all frequencies.  gpu_tag is accepted and ignored.  freq.dat and lfreq.dat (the frequency table and
the three reference frequencies) are read from the working directory (soc_library.py:88-92); --freq and --lfreq name other
files, --bins N sets N (default 30) when a library is built.

Build: the absorbed file must hold all NFREQ columns.  The grid and the representative cell of every bin come from the device
(Engine.library_build, with the absorptions resident where they fit), the representatives are solved in process with
soc_amd.a2e.run and <solver>.lib is written in the reference's byte layout.

Solve: the absorbed file may hold NFREQ or exactly 3 columns.  A missing library is built first when all columns are there.
Cells the library has no answer for are solved directly when all columns are there, and <solver>.lib.new then holds the library
with their bins filled in; with 3 columns their rows are zero and their count is printed.  A dust file (`eqdust`) in place of
the solver file is refused: equilibrium dusts are not part of the library here.  One GPU.
"""
import os
import sys
import time

import numpy as np

from . import a2e, files

TABLES = ("I1", "dI1", "I2", "dI2", "X", "Y", "Z")
CHUNK = 1 << 20                     # cells per transfer


def load_frequencies(path):
    return np.atleast_1d(np.loadtxt(path)).astype(np.float64)


def reference_columns(FREQ, FREF):
    """the columns of the frequency table nearest to the three reference frequencies (soc_library.py:118-119)"""
    if len(FREF) != 3:
        raise ValueError("the library method needs three reference frequencies, got %d" % len(FREF))
    return np.asarray([np.argmin(np.abs(f - FREQ)) for f in FREF], np.int32)


def write_library(path, lib):
    """soc_library.py:246-266: int32 N, NFREQ; float32 FREQ; I0, dI0; I1; dI1; I2; dI2; X; Y; Z; E[N^3, NFREQ]"""
    N, E = int(lib["N"]), np.asarray(lib["E"], np.float32)
    with open(path, "wb") as fp:
        np.asarray([N, E.shape[1]], np.int32).tofile(fp)
        np.asarray(lib["FREQ"], np.float32).tofile(fp)
        np.asarray([lib["I0"], lib["dI0"]], np.float32).tofile(fp)
        for k in TABLES:
            np.asarray(lib[k], np.float32).tofile(fp)
        E.tofile(fp)


def read_library(path):
    """soc_library.py:279-290"""
    with open(path, "rb") as fp:
        N, NFREQ = (int(v) for v in np.fromfile(fp, np.int32, 2))
        if not (2 <= N <= 64 and NFREQ >= 1):
            raise ValueError("%s: N = %d, NFREQ = %d is no library" % (path, N, NFREQ))
        lib = dict(N=N, NFREQ=NFREQ, FREQ=np.fromfile(fp, np.float32, NFREQ))
        lib["I0"], lib["dI0"] = np.fromfile(fp, np.float32, 2)
        for k, shape in zip(TABLES, [(N,), (N,), (N, N), (N, N)] + [(N, N, N)] * 3):
            lib[k] = np.fromfile(fp, np.float32, int(np.prod(shape))).reshape(shape)
        lib["E"] = np.fromfile(fp, np.float32, N ** 3 * NFREQ)
        if lib["E"].size != N ** 3 * NFREQ:
            raise ValueError("%s ends early" % path)
        lib["E"] = lib["E"].reshape(N ** 3, NFREQ)
    return lib


def _resident(engine, ABSORBED, verbose):
    """the absorptions in the resident arrays of the A2E path; False where the engine has none or they do not fit"""
    if not hasattr(engine, "a2e_resident_begin"):
        return False
    CELLS, NFREQ = ABSORBED.shape
    try:
        engine.a2e_resident_begin(CELLS, NFREQ)
    except Exception as err:
        if verbose:
            print("    library: cells not resident (%s)" % err)
        return False
    for a in range(0, CELLS, CHUNK):
        engine.a2e_resident_upload(a, ABSORBED[a:min(a + CHUNK, CELLS), :])
    return True


def build(engine, sol, ABSORBED, FREQ, IFREQ, N=30, verbose=True):
    """The library of a model: ABSORBED[CELLS, NFREQ] with all frequencies, IFREQ the three reference columns.  Returns the
    dict read_library gives, with IND[N^3] (the representative cell of every bin, -1 for none) besides."""
    CELLS, NFREQ = ABSORBED.shape
    if NFREQ != len(FREQ) or NFREQ != sol["NFREQ"]:
        raise ValueError("the absorptions hold %d frequencies, the frequency table %d, the solver %d" % (NFREQ, len(FREQ), sol["NFREQ"]))
    t0 = time.time()
    if _resident(engine, ABSORBED, verbose):
        try:
            lib = engine.library_build(N, cols=IFREQ)
        finally:
            engine.a2e_resident_end()
    else:
        lib = engine.library_build(N, ABS3=np.ascontiguousarray(ABSORBED[:, IFREQ], np.float32))
    m = np.nonzero(lib["IND"] >= 0)[0]
    if verbose:
        print("Out of (N=%d)^3 = %d bins, cells existed for %d bins  (%.3f s)" % (N, N ** 3, len(m), time.time() - t0))
    E = np.full((N ** 3, NFREQ), 1.0e32, np.float32)                  # 1e32: no data (soc_library.py:263)
    if len(m):
        t0 = time.time()
        rows = np.ascontiguousarray(ABSORBED[lib["IND"][m], :], np.float32)
        em, _ = a2e.run(engine, sol, rows, verbose=False)
        E[m, :] = np.clip(em, np.float32(1.0e-30), np.float32(1.0e30))
        if verbose:
            print("*** DIRECT SOLVE %.2f USEC PER CELL ***" % (1.0e6 * (time.time() - t0) / len(m)))
    lib.update(NFREQ=NFREQ, FREQ=np.asarray(FREQ, np.float32), E=E)
    return lib


def solve(engine, sol, lib, ABSORBED, IFREQ, EMITTED, ocol=None, verbose=True):
    """EMITTED[CELLS, nout] from the library.  ABSORBED[CELLS, NFREQ or 3]; IFREQ its three reference columns; ocol the library
    columns to write (None: all).  With all frequencies the missed cells are solved directly (sol) and the library with their
    bins filled in is returned; with three their rows are zero.  Returns (number of missed cells, that library or None)."""
    CELLS, NFF = ABSORBED.shape
    NFREQ = int(lib["E"].shape[1])
    full = NFF == NFREQ and NFF > 3
    if not full and NFF != 3:
        raise ValueError("the absorptions hold %d frequencies: 3 or the library's %d" % (NFF, NFREQ))
    nout = NFREQ if ocol is None else len(ocol)
    if EMITTED.shape != (CELLS, nout):
        raise ValueError("the emission must be [%d, %d]" % (CELLS, nout))
    t0 = time.time()
    engine.library_set(lib, ocol)
    try:
        if full and ocol is None and _resident(engine, ABSORBED, verbose):
            try:
                MIS = engine.library_solve_resident(IFREQ)
                for a in range(0, CELLS, CHUNK):
                    b = min(a + CHUNK, CELLS)
                    EMITTED[a:b, :] = engine.a2e_resident_download(a, b - a)
            finally:
                engine.a2e_resident_end()
        else:
            parts = []
            for a in range(0, CELLS, CHUNK):
                b = min(a + CHUNK, CELLS)
                EMITTED[a:b, :], miss = engine.library_solve(np.ascontiguousarray(ABSORBED[a:b, :][:, IFREQ], np.float32))
                parts.append(miss.astype(np.int64) + a)
            MIS = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    finally:
        engine.library_set(None)
    mis = len(MIS)
    if verbose:
        print("*** LIBRARY SOLVE %.2f USEC PER CELL ***" % (1.0e6 * (time.time() - t0) / max(CELLS, 1)))
    if mis < 1:
        if verbose:
            print("*** All cells matched by entries in the library ***")
        return 0, None
    if not full:                                                      # soc_library.py:484-490
        print("*** %d cells without answer in the library, and the absorptions hold %d frequencies only:" % (mis, NFF))
        print("***    the emission of those cells is set to ZERO")
        EMITTED[MIS, :] = 0.0
        return mis, None
    if verbose:
        print("*** Missing cells: %d, %.3f %% of all cells" % (mis, 100.0 * mis / CELLS))
    rows = np.ascontiguousarray(ABSORBED[MIS, :], np.float32)
    ADD, _ = a2e.run(engine, sol, rows, verbose=False)
    EMITTED[MIS, :] = ADD if ocol is None else ADD[:, ocol]
    # the library with the bins of those cells filled in, as the reference's host places them (soc_library.py:127-131, :315-320,
    # :446-464): numpy's log10 and round on the clipped reference absorptions; of several cells in a bin the last one stays
    new = dict(lib)
    for k in ("X", "Y", "Z", "E"):
        new[k] = np.array(lib[k], np.float32)
    N = int(lib["N"])
    IREF = np.log10(np.clip(rows[:, IFREQ], np.float32(1.0e-25), np.float32(1.0)))
    x = (IREF[:, 0] - lib["I0"]) / lib["dI0"]
    i = np.clip(np.round(x).astype(np.int32), 0, N - 1)
    y = (IREF[:, 1] - lib["I1"][i]) / lib["dI1"][i]
    j = np.clip(np.round(y).astype(np.int32), 0, N - 1)
    z = (IREF[:, 2] - lib["I2"][i, j]) / lib["dI2"][i, j]
    k = np.clip(np.round(z).astype(np.int32), 0, N - 1)
    new["X"][i, j, k], new["Y"][i, j, k], new["Z"][i, j, k] = x, y, z
    new["E"][k + N * (j + N * i), :] = ADD
    return mis, new


def main(argv=None, engine_factory=None):
    """the program; engine_factory() gives the engine to run on (default: soc_amd.lib.Engine on GPU 0)"""
    argv = list(sys.argv if argv is None else argv)
    opts = dict(freq="freq.dat", lfreq="lfreq.dat", bins="30")
    args = [argv[0]]
    it = iter(argv[1:])
    for a in it:
        if a.startswith("--") and a[2:] in opts:
            opts[a[2:]] = next(it, None)
            if opts[a[2:]] is None:
                print("%s needs a value" % a)
                return 1
        else:
            args.append(a)
    if len(args) not in (4, 5, 6):
        print("Usage:  python -m soc_amd.library  gpu_tag solver absorbed [emitted [ofreq.dat]]  [--freq F] [--lfreq F] [--bins N]")
        return 1
    solver, absorbed = args[2], args[3]
    emitted = args[4] if len(args) > 4 else None
    try:
        with open(solver, "rb") as fp:
            if fp.read(6) == b"eqdust":
                print("%s is a dust file (eqdust): the library of an equilibrium dust is not implemented here -- "
                      "solve it with python -m soc_amd.mabu, it needs no library" % solver)
                return 1
    except OSError as err:
        print(err)
        return 1
    N = int(opts["bins"])
    if not 2 <= N <= 64:
        print("--bins %d: 2 <= N <= 64" % N)
        return 1
    FREQ, FREF = load_frequencies(opts["freq"]), load_frequencies(opts["lfreq"])
    NFREQ = len(FREQ)
    CELLS, NFF = (int(v) for v in np.fromfile(absorbed, np.int32, 2))
    libfile = solver + ".lib"
    making = emitted is None or not os.path.exists(libfile)
    if making and NFF != NFREQ:
        print("%s holds %d frequencies, the table %d: %s" % (absorbed, NFF, NFREQ, "a library is built from all frequencies" if emitted is None
                                                               else "%s does not exist and cannot be built from these" % libfile))
        return 1
    if NFF != NFREQ and NFF != 3:
        print("Using the library... but %s has %d rather than 3 or %d frequencies" % (absorbed, NFF, NFREQ))
        return 1
    ABSORBED = np.memmap(absorbed, dtype=np.float32, mode="r", offset=8, shape=(CELLS, NFF))
    IFREQ = reference_columns(FREQ, FREF) if NFF > 3 else np.arange(3, dtype=np.int32)
    sol = files.read_solver(solver)
    if engine_factory is None:
        from .lib import Engine
        engine_factory = lambda: Engine(0)                            # noqa: E731
    engine = engine_factory()
    try:
        lib = None
        if making:
            if emitted is not None:
                print("%s does not exist yet: it is built first" % libfile)
            lib = build(engine, sol, ABSORBED, FREQ, IFREQ, N)
            write_library(libfile, lib)
        if emitted is None:
            return 0
        lib = read_library(libfile) if lib is None else lib
        if lib["E"].shape[1] != NFREQ:
            print("%s holds %d frequencies, the table %d" % (libfile, lib["E"].shape[1], NFREQ))
            return 1
        ocol = None
        if len(args) > 5:                                             # soc_library.py:298-306: the nearest library frequencies
            ocol = np.asarray([np.argmin(np.abs(f - lib["FREQ"].astype(np.float64))) for f in load_frequencies(args[5])], np.int32)
        nout = NFREQ if ocol is None else len(ocol)
        with open(emitted, "wb") as fp:
            np.asarray([CELLS, nout], np.int32).tofile(fp)
            fp.truncate(8 + 4 * CELLS * nout)
        EMITTED = np.memmap(emitted, dtype=np.float32, mode="r+", offset=8, shape=(CELLS, nout))
        mis, new = solve(engine, sol, lib, ABSORBED, IFREQ, EMITTED, ocol)
        EMITTED.flush()
        del EMITTED
        if new is not None:
            write_library(libfile + ".new", new)
    finally:
        engine.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
