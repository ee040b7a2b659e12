#!/usr/bin/env python3
"""a2e -- emission of stochastically heated grains on MI355X:

    python -m soc_amd.a2e  dust.solver  absorbed.data  emitted.data  [GPU [NSTOCH [IFREQ [aalg]]]]

Drop-in for ``A2E.py solver absorbed emitted`` (reference A2E.py:64-66): same solver file
(written by A2E_pre.py), same absorbed/emitted files.  For every grain size the absorptions of
all cells go through the HIP ``DoSolve`` (sizes < NSTOCH) or ``EqTemperature`` (sizes >= NSTOCH)
and the emission is accumulated (A2E.py:453-600).  Differences that are the point of the
rewrite: no run-time kernel build, no 266 MB global scratch matrix (the transition matrix
lives in LDS), batches are sized by memory, not by the scratch buffer.  Where the cells fit the device they stay resident while the
sizes are solved, the equilibrium sizes included: all of those in one launch that adds to the sum of the stochastic sizes
(a2e_set_eq_sizes + a2e_resident_solve_eq), with the bits of the route through a2e_eqtemp size by size and batch by batch, which
an engine without the call keeps.

With DUMP_TDUST=1 in the environment (A2E.py:108-114, 324-326, 378-400, 506-522) every grain size also leaves
<solver name without .solver>_size%03d.dump: {CELLS, NE} and the populations of the enthalpy levels X[CELLS, NE] of a stochastically
heated size, clamped to [1e-35, 10] (kernel_A2E.c:101-103), {CELLS, 1} and the temperatures T[CELLS] of an equilibrium size; one rank.

With the seventh argument, a file {CELLS} aalg[CELLS] of each cell's minimum aligned grain size, the emission of the grains larger
than that is written to <emitted>.P as well (A2E.py:28-29, 192-197, 413-429, 533-539): the polarised emission.
"""
import os
import sys
import time

import numpy as np
from scipy.interpolate import interp1d

from . import files
from .launch import FACTOR, H_K
from .synth import a2e_absorption_fraction

NIP = 5000                     # interpolation points of the E <-> T table (A2E.py:282)


def planck_safe(f, T):
    """A2E.py:206-209"""
    H_CC20 = 7.372496678e-28
    return 2.0e-20 * ((H_CC20 * f) * f) * f / (np.exp(np.clip(H_K * f / T, -100, +100)) - 1.0)


def eq_table(sol, isize):
    """E -> T lookup table of one size on the host (A2E.py:466-488): Emin, kE, oplgkE, TTT[NIP], KABS.  Built once per solver and
    size and kept: the loop is 5000 turns of Python, and a pipeline with re-emission iterations comes here in every iteration, each
    time with a dict freshly read from the solver file.  So the key is what the table is computed from -- the bits of FREQ, of the
    size's row of SK_ABS, of GD and of the size's S_FRAC -- and the arrays returned are the kept ones (not to be written to)."""
    key = tuple((a.dtype.str, a.tobytes()) for a in (np.asarray(sol["FREQ"]), np.asarray(sol["SK_ABS"][isize, :]),
                                                     np.asarray(sol["GD"]), np.asarray(sol["S_FRAC"][isize])))
    if key not in _EQ_TABLES:
        if len(_EQ_TABLES) >= 256:                 # (256 sizes x 20 KB; more than any set of dust models in one process)
            _EQ_TABLES.clear()
        _EQ_TABLES[key] = _eq_table(sol, isize)
    return _EQ_TABLES[key]


_EQ_TABLES = {}


def _eq_table(sol, isize):
    FREQ = np.asarray(sol["FREQ"], np.float64)
    KABS = sol["SK_ABS"][isize, :] / (sol["GD"] * sol["S_FRAC"][isize])
    TSTEP = 1600.0 / NIP
    TT = 4.0 + TSTEP * np.arange(NIP)
    DF = FREQ[2:] - FREQ[:-2]
    Eout = np.zeros(NIP, np.float64)
    for i in range(NIP):
        TMP = FACTOR * KABS * planck_safe(FREQ, TT[i])
        res = TMP[0] * (FREQ[1] - FREQ[0]) + TMP[-1] * (FREQ[-1] - FREQ[-2]) + np.sum(TMP[1:-1] * DF)
        Eout[i] = 4.0 * np.pi * 0.5 * res
    Emin, Emax = Eout[0], Eout[NIP - 1] * 0.9999
    kE = (Emax / Emin) ** (1.0 / (NIP - 1.0))
    oplgkE = 1.0 / np.log10(kE)
    TTT = np.asarray(interp1d(Eout, TT)(Emin * kE ** np.arange(NIP)), np.float32)
    return Emin, kE, oplgkE, TTT, np.asarray(KABS, np.float32)


def stochastic_count(sol, NSTOCH):
    """how many sizes of a solver file are solved stochastically: NSTOCH, at most the sizes the file has tables for"""
    return max(min(int(NSTOCH), len(sol["sizes"]), sol["NSIZE"]), 0)


def eq_sizes(sol, NSTOCH=999):
    """the sizes that a2e.run solves as equilibrium sizes, ascending: isize >= NSTOCH or without tables in the solver file, less those
    with S_FRAC < 1e-30, which it skips (A2E.py:466)"""
    return [isize for isize in range(stochastic_count(sol, NSTOCH), sol["NSIZE"]) if not sol["S_FRAC"][isize] < 1.0e-30]


def eq_size_tables(sol, sizes, polarised=False):
    """the arguments of engine.a2e_set_eq_sizes for these sizes of the solver: what the host route hands to a2e_eqtemp size by size
    (eq_table, a2e_absorption_fraction), stacked"""
    tabs = [eq_table(sol, isize) for isize in sizes]
    f32 = np.float32
    return (NIP, FACTOR, sol["FREQ"], np.stack([a2e_absorption_fraction(sol, isize) for isize in sizes]),
            np.stack([t[4] for t in tabs]), np.stack([t[3] for t in tabs]), np.asarray([t[0] for t in tabs], f32),
            np.asarray([t[1] for t in tabs], f32), np.asarray([t[2] for t in tabs], f32), f32(sol["GD"]),
            np.asarray([sol["S_FRAC"][isize] for isize in sizes], f32),
            np.asarray([sol["SIZE_A"][isize] for isize in sizes], f32) if polarised else None)


def dump_name(prefix, isize):
    """the file of one grain size of a DUMP_TDUST=1 run (A2E.py:379, :508)"""
    return '%s_size%03d.dump' % (prefix, isize)


def write_dump(prefix, isize, X):
    """One size's dump file: {CELLS, NE} int32 and X[CELLS, NE] float32, the populations of the enthalpy levels of a stochastically
    heated size (A2E.py:379-400); {CELLS, 1} and T[CELLS], the temperatures of an equilibrium size (A2E.py:506-522)"""
    X = np.asarray(X, np.float32)
    X = X.reshape(X.shape[0], -1)
    with open(dump_name(prefix, isize), 'wb') as fp:
        np.asarray(X.shape, np.int32).tofile(fp)
        X.tofile(fp)


def solve_sizes_resident(engine, sol, nstoch, polarised, eq=True, log=None, populations=None, keep_teq=False):
    """THE size loop on resident cells -- the block that a2e_resident_begin, or mabu_begin and mabu_split, opened: the sizes below nstoch
    one launch each, in their order (A2E.py:596-600; polarised: with the weights of A2E.py:413-429 for the kernel's epilogue), then all
    equilibrium sizes in one launch that adds them to the same sums (A2E.py:456-547; its hard mask, :533-539).  eq False leaves those to
    the caller; eq 'try' does so as well where the engine refuses their tables (no tile of this NFREQ fits the LDS), and says so
    through log.  Returns whether the equilibrium sizes were solved here.
    populations(isize, X[cells, NE]): every stochastic size is solved with a2e_resident_solve_dump and its populations handed over;
    keep_teq: the launch of the equilibrium sizes keeps their temperatures (a2e_resident_keep_teq), which the caller reads with
    a2e_resident_download_teq(slot, ...), slot counting eq_sizes(sol, nstoch).  Neither changes the sums."""
    log = log or (lambda line: None)
    for isize in range(nstoch):
        engine.a2e_set_size(sol["NE"], sol["NFREQ"], sol["sizes"][isize], a2e_absorption_fraction(sol, isize))
        if polarised:
            engine.a2e_set_size_aalg(sol["SIZE_A"], isize)
        if populations is not None:
            populations(isize, engine.a2e_resident_solve_dump())
        else:
            engine.a2e_resident_solve()
        log("    isize = %d   stochastic heating" % isize)
    sizes = eq_sizes(sol, nstoch) if eq else []
    if not sizes:
        return False
    try:
        engine.a2e_set_eq_sizes(*eq_size_tables(sol, sizes, polarised))
    except Exception as err:
        if eq != 'try':
            raise
        log("    a2e: equilibrium sizes not on the device (%s)" % err)
        return False
    if keep_teq:
        engine.a2e_resident_keep_teq(True)
    engine.a2e_resident_solve_eq()
    return True


def aalg_weights(ASIZE, isize, aalg, stochastic=True):
    """The share of size `isize` that is aligned in cells of minimum aligned size aalg (A2E.py:413-429; for an equilibrium size the
    hard mask alone, :533-539).  Returns (full, part, w): full where ASIZE[isize] >= aalg (weight 1), part where aalg lies strictly
    between this size and the next (none for the last size), w[cells] float32 the weight there (0 elsewhere):
    (log10(aalg) - log10(ASIZE[isize])) / (log10(ASIZE[isize+1]) - log10(ASIZE[isize])), float32 all the way as numpy evaluates the
    reference's line.  The weight grows towards the upper size, as the reference's does."""
    ASIZE, aalg = np.asarray(ASIZE, np.float32), np.asarray(aalg, np.float32)
    full = ASIZE[isize] >= aalg
    part = np.zeros(aalg.shape, bool)
    w = np.zeros(aalg.shape, np.float32)
    if stochastic and isize < ASIZE.size - 1:
        part = (ASIZE[isize] < aalg) & (ASIZE[isize + 1] > aalg)
        w[part] = (np.log10(aalg[part]) - np.log10(ASIZE[isize])) / (np.log10(ASIZE[isize + 1]) - np.log10(ASIZE[isize]))
    return full, part, w


def aalg_weight(ASIZE, isize, aalg, stochastic=True):
    """aalg_weights as one array W[cells]: 1, w or 0"""
    full, part, w = aalg_weights(ASIZE, isize, aalg, stochastic)
    return np.where(full, np.float32(1.0), np.where(part, w, np.float32(0.0))).astype(np.float32)


def _add_polarised(PEM, emit, full, part, w):
    """PEMITTED[m] += emit[m] and PEMITTED[m] += w * emit[m] (A2E.py:417-429) on rows of PEM; emit[rows, columns of PEM]"""
    PEM[full] += emit[full]
    if part.any():
        PEM[part] += w[part, None] * emit[part]


def run(engine, sol, ABSORBED, NSTOCH=999, IFREQ=-1, batch=65536, verbose=True, aalg=None, dump=None, teq=None):
    """ABSORBED[CELLS,NFREQ] -> EMITTED[CELLS,NFREQ or 1].  Returns (EMITTED, kernel_seconds), or with aalg[CELLS] -- the minimum
    aligned grain size of every cell -- (EMITTED, PEMITTED, kernel_seconds), PEMITTED the emission of the aligned grains.
    dump: a file prefix -- every size the run handles leaves <prefix>_size%03d.dump (write_dump: the populations of a stochastically
    heated size, the temperatures of an equilibrium size; a size with S_FRAC < 1e-30 is skipped before its file is opened, A2E.py:465),
    what the reference writes with DUMP_TDUST=1.  teq: a dict that receives {isize: T[CELLS]} of the equilibrium sizes.  Neither
    changes the emission; both need the engine's calls for them on the route taken (a2e_solve_dump / a2e_resident_solve_dump,
    a2e_resident_keep_teq), and an engine without those of the resident route is taken through the batches."""
    CELLS, NFREQ = ABSORBED.shape
    if NFREQ != sol["NFREQ"]:
        raise ValueError("absorbed file has %d frequencies, solver %d" % (NFREQ, sol["NFREQ"]))
    ABSORBED = np.array(ABSORBED, np.float32)        # A2E.py:184-185: clip the last channel
    ABSORBED[:, NFREQ - 1] = np.clip(ABSORBED[:, NFREQ - 1], 0.0, 0.2 * ABSORBED[:, NFREQ - 2])
    EMITTED = np.zeros((CELLS, 1 if IFREQ >= 0 else NFREQ), np.float32)
    PEMITTED = None
    if aalg is not None:
        aalg = np.ascontiguousarray(aalg, np.float32)
        if aalg.shape != (CELLS,):
            raise ValueError("aalg holds %s values, the absorptions %d cells" % (aalg.shape, CELLS))
        PEMITTED = np.zeros_like(EMITTED)
    cols = slice(IFREQ, IFREQ + 1) if IFREQ >= 0 else slice(None)
    ASIZE = sol["SIZE_A"]
    tker = 0.0
    want_t = dump is not None or teq is not None

    def temperatures(isize, T):
        if dump is not None:
            write_dump(dump, isize, T)
        if teq is not None:
            teq[isize] = T
    # The stochastically heated sizes with the cells resident in device memory (soc_a2e_resident_*): absorptions up once, every size a
    # launch over all cells that adds its emission to a sum on the device, the sum down once -- instead of NSIZE round trips of every
    # batch (solve_sizes_resident).  The sum is added in the order of the sizes, as the reference's host does, equilibrium sizes last,
    # so the result is the same to the bit.  An engine without a2e_resident_solve_eq gets those size by size through a2e_eqtemp.
    nstoch = stochastic_count(sol, NSTOCH)
    eq = 'try' if hasattr(engine, "a2e_resident_solve_eq") and (not want_t or hasattr(engine, "a2e_resident_keep_teq")) else False   # (a refusal of the tables: size by size, as before)
    resident = eq_done = False
    if (nstoch > 0 or (eq and eq_sizes(sol, nstoch))) and hasattr(engine, "a2e_resident_begin") and (aalg is None or hasattr(engine, "a2e_resident_upload_aalg")) \
            and (dump is None or nstoch == 0 or hasattr(engine, "a2e_resident_solve_dump")):
        try:
            if aalg is None:
                engine.a2e_resident_begin(CELLS, NFREQ)
            else:
                engine.a2e_resident_begin(CELLS, NFREQ, polarised=True)
            resident = True
        except Exception as err:                                  # not enough device memory: batches as before
            if verbose:
                print("    a2e: cells not resident (%s)" % err)
    if resident:
        try:
            t0 = time.time()
            for icell in range(0, CELLS, batch):
                engine.a2e_resident_upload(icell, ABSORBED[icell:min(icell + batch, CELLS), :])
                if aalg is not None:
                    engine.a2e_resident_upload_aalg(icell, aalg[icell:min(icell + batch, CELLS)])
            eq_done = solve_sizes_resident(engine, sol, nstoch, aalg is not None, eq, print if verbose else None,
                                           populations=None if dump is None else (lambda isize, X: write_dump(dump, isize, X)), keep_teq=want_t)
            for slot, isize in enumerate(eq_sizes(sol, nstoch)) if (eq_done and want_t) else ():
                T = np.zeros(CELLS, np.float32)
                for icell in range(0, CELLS, batch):
                    b = min(icell + batch, CELLS)
                    engine.a2e_resident_download_teq(slot, icell, b - icell, out=T[icell:b])
                temperatures(isize, T)
            for icell in range(0, CELLS, batch):
                b = min(icell + batch, CELLS)
                EMITTED[icell:b] += engine.a2e_resident_download(icell, b - icell)[:, cols]
                if aalg is not None:
                    PEMITTED[icell:b, :] += engine.a2e_resident_download_p(icell, b - icell)[:, cols]
            tker += time.time() - t0
        finally:
            engine.a2e_resident_end()
    for isize in range(sol["NSIZE"]):
        AF = a2e_absorption_fraction(sol, isize)
        if isize >= NSTOCH or isize >= len(sol["sizes"]):
            if sol["S_FRAC"][isize] < 1.0e-30 or eq_done:
                continue
            Emin, kE, oplgkE, TTT, KABS = eq_table(sol, isize)
            scale = sol["GD"] * sol["S_FRAC"][isize]
            Tall = np.zeros(CELLS, np.float32) if want_t else None
            for icell in range(0, CELLS, batch):
                b = min(icell + batch, CELLS)
                tmp = np.asarray(ABSORBED[icell:b, :] * AF, np.float32)
                t0 = time.time()
                T, emit = engine.a2e_eqtemp(icell, CELLS, NIP, FACTOR, kE, oplgkE, Emin, sol["FREQ"], KABS, TTT, tmp)
                tker += time.time() - t0
                if want_t:
                    Tall[icell:b] = T
                EMITTED[icell:b] += emit[:, cols] * scale
                if aalg is not None:                               # A2E.py:533-539: the hard mask, the reference's own product
                    full = aalg_weights(ASIZE, isize, aalg[icell:b], stochastic=False)[0]
                    PEMITTED[icell:b][full] += emit[full][:, cols] * sol["GD"] * sol["S_FRAC"][isize]
            if want_t:
                temperatures(isize, Tall)
            continue
        if resident:
            continue
        engine.a2e_set_size(sol["NE"], NFREQ, sol["sizes"][isize], AF)
        fpX = None
        if dump is not None:                                       # A2E.py:379-380, :400: the header, then the rows batch by batch
            fpX = open(dump_name(dump, isize), 'wb')
            np.asarray([CELLS, sol["NE"]], np.int32).tofile(fpX)
        try:
            for icell in range(0, CELLS, batch):
                b = min(icell + batch, CELLS)
                t0 = time.time()
                if fpX is not None:
                    emit, X = engine.a2e_solve_dump(ABSORBED[icell:b, :])
                    np.asarray(X, np.float32).tofile(fpX)
                else:
                    emit = engine.a2e_solve(ABSORBED[icell:b, :])
                tker += time.time() - t0
                EMITTED[icell:b] += emit[:, cols]
                if aalg is not None:                                   # A2E.py:413-429, on the emission of this batch and size
                    _add_polarised(PEMITTED[icell:b], emit[:, cols], *aalg_weights(ASIZE, isize, aalg[icell:b]))
        finally:
            if fpX is not None:
                fpX.close()
        if verbose:
            print("    isize = %d   stochastic heating" % isize)
    if aalg is not None:
        return EMITTED, PEMITTED, tker
    return EMITTED, tker


def read_aalg(filename, CELLS):
    """aalg file {CELLS} aalg[CELLS] float32 (A2E.py:382-386: a file for another number of cells is refused)"""
    cells = np.fromfile(filename, np.int32, 1)
    if cells.size != 1 or int(cells[0]) != CELLS:
        raise files.FileError("%s is an aalg file for %s cells, the run has %d" % (filename, int(cells[0]) if cells.size else "no", CELLS))
    if os.path.getsize(filename) < 4 + 4 * CELLS:
        raise files.FileError("%s: fewer than %d values" % (filename, CELLS))
    return np.memmap(filename, dtype=np.float32, mode='r', offset=4, shape=(CELLS,))


DUMP_ONE_RANK = ("DUMP_TDUST=1 with %d ranks: every rank solves a share of the cells, and a dump file holds all of them "
                 "(no dump from part of the cells); run it with one rank")


class DumpNeedsOneRank(RuntimeError):
    """the per-size dump files were asked for in a run of several ranks"""


def dump_prefix(solver, environ=None):
    """The reference's switch (A2E.py:108-117): with DUMP_TDUST=1 in the environment the prefix of the dump files, the solver's name
    with `.solver` removed; else None"""
    environ = os.environ if environ is None else environ
    return solver.replace('.solver', '') if environ.get("DUMP_TDUST") == "1" else None


def cell_range(CELLS, rank, world):
    """cells [c0, c1) of rank `rank`: the cells of a grid are independent in A2E, so N GPUs split them"""
    per = (CELLS + world - 1) // world
    return min(rank * per, CELLS), min((rank + 1) * per, CELLS)


def run_sharded(engine_factory, solver, absorbed, emitted, NSTOCH=999, IFREQ=-1, comm=None, verbose=True, aalg=None, dump=None):
    """The whole program for one rank of `comm` (or alone): memory-map the absorbed file, solve this rank's cells,
    write them into this rank's part of the emitted file.  No collective on the data path -- the ranks only wait
    for rank 0 to have created the file, and for each other at the end.  aalg: the file of the minimum aligned grain sizes; the
    polarised emission then goes to <emitted>.P in the same way.  dump: the prefix of the per-size dump files (run); refused with
    several ranks.  Returns (cells solved, kernel seconds)."""
    rank, world = (comm.rank, comm.world) if comm else (0, 1)
    if dump is not None and world > 1:                         # (before rank 0 creates the emitted file)
        raise DumpNeedsOneRank(DUMP_ONE_RANK % world)
    sol = files.read_solver(solver)
    dims = np.fromfile(absorbed, np.int32, 2)
    CELLS, NFREQ = int(dims[0]), int(dims[1])
    ABS = np.memmap(absorbed, dtype=np.float32, mode='r', offset=8, shape=(CELLS, NFREQ))
    nout = 1 if IFREQ >= 0 else NFREQ
    AALG = read_aalg(aalg, CELLS) if aalg else None
    outs = [emitted] + ([emitted + '.P'] if aalg else [])
    if rank == 0:
        for name in outs:
            with open(name, 'wb') as fp:
                np.asarray([CELLS, nout], np.int32).tofile(fp)
                fp.truncate(8 + 4 * CELLS * nout)
    if comm:
        comm.barrier()
    c0, c1 = cell_range(CELLS, rank, world)
    tker = 0.0
    if c1 > c0:
        eng = engine_factory()
        try:
            res = run(eng, sol, ABS[c0:c1, :], NSTOCH, IFREQ, verbose=verbose and rank == 0, aalg=None if AALG is None else AALG[c0:c1], dump=dump)
            tker = res[-1]
        finally:
            if hasattr(eng, "close"):
                eng.close()
        for name, EM in zip(outs, res[:-1]):
            out = np.memmap(name, dtype=np.float32, mode='r+', offset=8, shape=(CELLS, nout))
            out[c0:c1, :] = EM
            out.flush()
            del out
    if comm:
        comm.barrier()
    return c1 - c0, tker


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 4:
        print("Usage:  python -m soc_amd.a2e  solver absorbed emitted [GPU [NSTOCH [IFREQ [aalg]]]]")
        print("        (N GPUs: python -m torch.distributed.run --nproc-per-node N -m soc_amd.a2e ...)")
        return 1
    from .lib import Engine
    from .dist import Comm
    NSTOCH = int(argv[5]) if len(argv) > 5 else 999
    IFREQ = int(argv[6]) if len(argv) > 6 else -1
    aalg = argv[7] if len(argv) > 7 else None                  # A2E.py:104
    t0 = time.time()
    comm = Comm()
    try:
        n, tker = run_sharded(lambda: Engine(comm.local_rank), argv[1], argv[2], argv[3], NSTOCH, IFREQ,
                              comm if comm.world > 1 else None, aalg=aalg, dump=dump_prefix(argv[1]))
    except DumpNeedsOneRank as err:
        print(err)
        comm.close()
        return 1
    DT = time.time() - t0
    if comm.rank == 0:
        print('@@  a2e %.3f SECONDS   (solver calls %.3f s on rank 0, %d ranks)' % (DT, tker, comm.world))
        print('  %4d  -- %.3e SECONDS PER CELL  -- %8.3f CELLS PER SECOND' % (n * comm.world, DT / max(n * comm.world, 1), n * comm.world / DT))
    comm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
