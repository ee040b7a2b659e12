"""The round trip of the library method on a synthetic solver, as a run of the program soc_amd.library in a directory of its own:
build <solver>.lib from one set of absorptions, solve that set with it, solve it again for a subset of the frequencies, then
solve a second set that leaves the library's cube -- once with all frequencies (the missed cells are solved directly and
<solver>.lib.new is written), once with the three reference columns only (their rows become zero).  Shared by the CPU test
(stand-in engine) and the GPU test (the same calls on the device; the files must be equal)."""
import os

import numpy as np

from soc_amd import files, library, synth

NFREQ, CELLS, N = 7, 5000, 6
REF = (1, 3, 5)                    # the columns of the reference frequencies
OFREQ = (6, 2, 3)                  # the columns the `ofreq` run asks for, in this order


def solver():
    return synth.synth_solver(NFREQ=NFREQ, NE=24, NSIZE=2, seed=5)


def absorptions(sol, seed, lo, hi, cells=CELLS, scatter=0.1):
    """[cells, NFREQ]: a power law in frequency with a level spread over 10**lo .. 10**hi and some scatter in slope and per channel"""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = lo + (hi - lo) * rng.random(cells)
    slope = -1.0 + scatter * rng.standard_normal(cells)
    A = 10.0 ** u[:, None] * (sol["FREQ"][None, :].astype(np.float64) / 1.0e13) ** slope[:, None] * rng.lognormal(0.0, scatter, (cells, NFREQ))
    return A.astype(np.float32)


def sets(sol):
    """The first set holds every cell twice.  A cell that is alone in its (i, j) window gets no grid on axis 2 (`< 2`,
    soc_library.py:162), so no bin represents it and the library built from its own set misses it; with a twin no window that
    holds a cell holds fewer than two."""
    first = absorptions(sol, 11, -9.0, -6.0)
    first[CELLS // 2:] = first[:CELLS // 2]
    second = absorptions(sol, 12, -11.0, -4.0, 600, 0.2)       # wider than the first: part of it lies outside the cube
    return first, second


def read_emitted(path):
    cells, nf = np.fromfile(path, np.int32, 2)
    return np.fromfile(path, np.float32, offset=8).reshape(cells, nf)


def run_program(tmp, engine_factory=None):
    """Returns dict(lib, first, ofreq, second, new, three): the library files as read_library gives them and the emitted arrays."""
    sol = solver()
    first, second = sets(sol)
    p = lambda name: os.path.join(str(tmp), name)                     # noqa: E731
    synth.write_solver(p("dust.solver"), sol)
    np.savetxt(p("freq.dat"), sol["FREQ"].astype(np.float64))
    np.savetxt(p("lfreq.dat"), sol["FREQ"].astype(np.float64)[list(REF)] * 1.02)     # (the nearest table entries are REF)
    np.savetxt(p("ofreq.dat"), sol["FREQ"].astype(np.float64)[list(OFREQ)] * 0.99)
    files.write_absorbed(p("first.abs"), first)
    files.write_absorbed(p("second.abs"), second)
    files.write_absorbed(p("second3.abs"), np.ascontiguousarray(second[:, list(REF)]))
    common = ["--freq", p("freq.dat"), "--lfreq", p("lfreq.dat"), "--bins", str(N)]

    def prog(*args):
        assert library.main(["library", "1", p("dust.solver")] + [p(a) for a in args] + common, engine_factory) == 0

    out = {}
    prog("first.abs")
    out["lib"] = library.read_library(p("dust.solver.lib"))
    prog("first.abs", "first.emit")
    assert not os.path.exists(p("dust.solver.lib.new"))               # no miss: no new library
    prog("first.abs", "ofreq.emit", "ofreq.dat")
    prog("second.abs", "second.emit")
    out["new"] = library.read_library(p("dust.solver.lib.new"))
    prog("second3.abs", "three.emit")
    for k in ("first", "ofreq", "second", "three"):
        out[k] = read_emitted(p(k + ".emit"))
    return out
