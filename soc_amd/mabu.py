#!/usr/bin/env python3
"""mabu -- emission of a model with several dust components from its absorptions:

    python -m soc_amd.mabu  soc.ini  absorbed.data  emitted.data  [ofreq.dat]  [--makelib LFREQ [--bins N]]  [--uselib LFREQ]  [--temperatures]

Counterpart of ``A2E_MABU.py ini absorbed.data emitted.data`` (reference A2E_MABU.py:236-342, 700-1180): the dust list,
the abundance files and `singleabu` come from the ini, an equilibrium dust is solved from its dust file, a
stochastically heated one (gsetdust) from its <dust>.solver file (soc_amd.a2e_pre writes it).  For every dust the
absorptions are split in proportion to cross section x abundance (kernel_A2E_MABU_aux.c:3-23), the emission of that
share is solved, and the emissions are summed weighted by the abundances (A2E_MABU.py:1128-1140).

solve_emission is that stage, shared with soc_amd.driver.  With an engine that has the soc_mabu_* calls the arrays stay
in device memory from the absorbed file to the sum (the absorptions go up once, the sum comes down once); with any
other engine the stage runs as numpy around the engine's per-dust solvers.  The two give the same bits.

A gsetdust file's line ``nstoch N`` (A2E_MABU.py:124-143; DustLib writes it at the first size above amin_equ) is honoured as the
reference honours it: the sizes below N are solved stochastically, those from N on -- and sizes without tables in the solver file --
at their equilibrium temperature (A2E.py:456-547), on either path; on the device path all equilibrium sizes of a dust in one launch
on the resident cells (engine.a2e_set_eq_sizes + a2e_resident_solve_eq), which an engine needs to be offered that path for such a
dust.  A negative N or no line: every size is stochastically heated.  (Before, the line was not read; a file with N below its number
of sizes is the one input whose result this changed.)

Ini lines ``polarisation <dust> <aalg file>`` (A2E_MABU.py:158-167; the key is matched by its prefix `polari`) name, for a dust of
the ini, the file {CELLS} aalg[CELLS] of each cell's minimum aligned grain size.  Such a dust gets a polarised emission beside its
emission -- a stochastically heated one from the solver (soc_amd.a2e with aalg, A2E_MABU.py:971-984), an equilibrium one from the
table <dust>.rpol (A2E_MABU.py:615-637) -- these are summed weighted by the abundances like the emission (:1139-1147), and
<emitted>.R = polarised / (total + 1e-32) is written: {CELLS}, then [CELLS, NFREQ] float32 (:1182, :1188-1198), the polarisation
reduction factor that `polred` of a map run reads.  The reference compares the dust names with `.dust` stripped in one place and
unstripped in others (:585, :972, :1111), so that whether a line takes effect depends on how the name is written; here the names
are compared with `.dust` stripped on both sides.  Without such lines nothing changes and no .R file appears.

With N GPUs (python -m torch.distributed.run --nproc-per-node N -m soc_amd.mabu ...) every rank solves its share of
the cells and writes its rows of the emitted file.  The reference's optional fourth argument (ofreq.dat: emission on a
subset of the frequencies) is refused for a direct run, as are the neural-network shortcuts.

The library method for several dusts (the `uselib` / `makelib` of ASOC_driver.py's usage line): every dust of the ini, equilibrium or
stochastically heated, has a library <dust name without .dust>.mlib (library_name) in the byte layout of soc_amd.library's .lib,
indexed by the log of that dust's share split_absorbed(...) of the absorptions at three reference frequencies.  --makelib LFREQ
[--bins N] (run(makelib=(LFREQ, N))) writes them as a by-product of the normal solve, whose products do not change: the grid and the
representative cells from engine.library_build on the share, the rows from the emission that dust's solve has just left, no second
solve; one rank and, on the device path, one cell range, else it is refused.  An ini with `libabs FILE` and an absorbed file of exactly
three columns takes the look-up (solve_emission_library: one fused kernel on the device, the composition split -> library_solve ->
weighted sum on the host, the same bits); a (cell, dust) without an answer adds zero, the counts are printed per dust; ofreq.dat then
selects the library columns nearest to its frequencies.  --uselib LFREQ with an absorbed file of all frequencies does the same look-up
from its reference columns and then solves every cell with a miss in any dust directly, overwriting those rows: a library checked
against the direct solve on one run.  <dust>.mlib.new is not written.

--temperatures (run(temperatures=True), solve_emission(temperatures=True)): the dust temperatures that the solvers compute on the way
to the emission are written as the reference writes them -- '<dust>.T', raw float32 [CELLS], for every equilibrium dust
(A2E_MABU.py:551), and <solver name without .solver>_size%03d.dump, {CELLS, 1} then T[CELLS], for every equilibrium size of a
stochastically heated dust (A2E.py:506-522 with DUMP_TDUST=1).  On the device path they are read back after each dust's solve (4 bytes
per cell and dust or size); the emission does not change.  One rank, and no library look-up (nothing is solved there), else refused.
The populations of stochastically heated sizes are the dump of python -m soc_amd.a2e, not of this program.
"""
import os
import sys
import time

import numpy as np
from scipy.interpolate import interp1d

from . import a2e, files, library
from .asoc import ResidentAbsorptions, UnsupportedOption
from .ini import User
from .launch import FACTOR
from .lib import DoesNotFit

NE_EQ = 30000                    # A2E_MABU.py:478
NSTOCH_ALL = 9999                # A2E_MABU.py:124: a gsetdust file without an `nstoch` line -- every size is stochastically heated
REFUSED_KEYS = ('nnmake', 'nnsolve', 'nnabs', 'nnemit', 'nnthin', 'absthin', 'aalg', 'crheating')
CHUNK = 1 << 20                  # cells per upload / download call


def refuse(U, pol=None, world=1):
    """what the in-memory pipeline does not take; with `libabs` (a library run) also what a library cannot give, each with its reason.
    pol: polarisation_lines' list; world: the number of ranks"""
    if 'libmaps' in U.KEYS and 'libabs' not in U.KEYS:
        raise UnsupportedOption("libmaps without libabs: the maps of a library's frequencies come from a library run (`libabs FILE` with it); "
                                "python -m soc_amd.asoc maps an emitted file that holds only those columns")
    if 'libabs' in U.KEYS:
        bad = []
        if U.ITERATIONS > 0 and U.CLPAC > 0:
            bad.append("iterations > 0 with cellpackets (the dust re-emission needs the emission at every frequency sent from the cells and "
                       "absorptions at every frequency to solve it again; a library run simulates three)")
        if pol is not None:
            bad.append("polarisation lines (the libraries hold the total emission only: no polarised emission comes from a library)")
        if 'saveint' in U.KEYS:
            bad.append("saveint (the intensity file holds all frequencies, a library run simulates three)")
        for k in ('nnmake', 'absthin'):
            if k in U.KEYS:
                bad.append("%s (the thinned absorptions train a network on all frequencies; a library run has three)" % k)
        if world > 1:
            bad.append("more than one rank (%d: the look-up is one memory-bound pass over the cells of one device)" % world)
        if bad:
            raise UnsupportedOption("libabs (a library run) together with " + "; ".join(bad))
    bad = [k for k in REFUSED_KEYS if k in U.KEYS]
    if bad:
        raise UnsupportedOption("ini options outside the in-memory pipeline (neural-network shortcuts, "
                                "cosmic-ray heating): " + ", ".join(bad))


def dust_kind(name):
    """'gsetdust' (stochastically heated: needs <name>.solver) or 'eqdust' (ASOC_driver.py:66-68)"""
    with open(name) as fp:
        return fp.readline().split()[0]


def simple_name(name):
    """the dust file the transfer run uses for a gsetdust (ASOC_driver.py:247-248: prefix gs_ dropped, _simple added)"""
    d, b = os.path.split(name)
    return os.path.join(d, '%s_simple.dust' % b.replace('.dust', '').replace('gs_', ''))


def solver_name(name):
    """ASOC_driver.py:199-201 / A2E_MABU.py:264"""
    d, b = os.path.split(name)
    b = b.replace('.dust', '')
    if b.startswith('gs_'):
        b = b[3:]
    return os.path.join(d, b + '.solver')


def library_name(name):
    """the library of a dust of a multi-dust model: <dust name without .dust>.mlib, beside the dust file.  Not <solver>.lib of
    soc_amd.library, which is built from unsplit absorptions"""
    return strip_dust(name) + '.mlib'


def read_nstoch(name, kind=None):
    """The number of stochastically heated sizes of a gsetdust file (A2E_MABU.py:124-136): the value of its line `nstoch N` (the last
    one, should there be several; only lines of at least two tokens whose first is `nstoch` count), NSTOCH_ALL where it is negative
    or there is no such line.  The sizes from N on are solved at their equilibrium temperature.  An eqdust file is not searched."""
    nstoch = NSTOCH_ALL
    if (kind or dust_kind(name)) != 'eqdust':
        with open(name) as fp:
            for line in fp:
                s = line.split()
                if len(s) > 1 and s[0] == 'nstoch':
                    nstoch = int(s[1])
                    if nstoch < 0:
                        nstoch = NSTOCH_ALL
    return nstoch


def stochastic_sizes(sol):
    """how many sizes of a solver file (read by _tables) are solved stochastically: its dust file's `nstoch`, at most the sizes the
    file has tables for; the rest are equilibrium sizes"""
    return a2e.stochastic_count(sol, sol.get("nstoch", NSTOCH_ALL))


def require_solvers(dusts, kinds):
    """a solver file per stochastically heated dust -- soc_amd.a2e_pre writes them (ASOC_driver.py:196-228 calls A2E_pre.py there)"""
    for d, k in zip(dusts, kinds):
        if k == 'gsetdust' and not os.path.exists(solver_name(d)):
            raise FileNotFoundError("%s: the solver file of %s is missing; write it with python -m soc_amd.a2e_pre %s <frequency file> %s"
                                    % (solver_name(d), d, d, solver_name(d)))


def planck_safe(f, T):
    """A2E_MABU.py PlanckSafe: 2h f^3 / c^2 / (exp(hf/kT) - 1), overflow-safe"""
    H_K, H_CC = 4.79924335e-11, 7.372496678e-48
    return 2.0 * H_CC * f * f * f / (np.exp(np.clip(H_K * f / T, -100.0, 100.0)) - 1.0)


def eq_dust_table(dust):
    """E -> T table of an equilibrium dust (A2E_MABU.py:470-490): FREQ, KABS per unit density, Emin, kE, oplgkE, TTT[NE]"""
    with open(dust) as fp:
        lines = fp.readlines()
    gd, gr = float(lines[1].split()[0]), float(lines[2].split()[0])
    d = np.loadtxt(dust, skiprows=4, ndmin=2)
    FREQ = np.asarray(d[:, 0], np.float32)
    KABS = np.asarray(d[:, 2] * gd * np.pi * gr ** 2.0, np.float32)
    TSTEP = 1600.0 / NE_EQ
    TT = 1.0 + TSTEP * np.arange(NE_EQ)
    F64 = np.asarray(FREQ, np.float64)
    DF = FREQ[2:] - FREQ[:-2]
    Eout = np.zeros(NE_EQ, np.float64)
    # vectorised over the temperatures (the reference loops): same sums, frequency by frequency
    B = KABS[None, :] * planck_safe(F64[None, :], TT[:, None])
    res = B[:, 0] * (FREQ[1] - FREQ[0]) + B[:, -1] * (FREQ[-1] - FREQ[-2]) + np.sum(B[:, 1:-1] * DF[None, :], axis=1)
    Eout[:] = (4.0 * np.pi * FACTOR) * 0.5 * res
    Emin, Emax = Eout[0], Eout[NE_EQ - 1] * 0.9999
    kE = (Emax / Emin) ** (1.0 / (NE_EQ - 1.0))
    oplgkE = 1.0 / np.log10(kE)
    TTT = np.asarray(interp1d(Eout, TT)(Emin * kE ** np.arange(NE_EQ)), np.float32)
    return FREQ, KABS, Emin, kE, oplgkE, TTT


def relative_cross_sections(dusts, kinds):
    """RABS[NFREQ, NDUST] (A2E_MABU.py:245-342): absorption cross section per unit density of every component --
    from the dust file (eqdust) or summed over the sizes of the solver file -- normalised per frequency, float64"""
    cols, FREQ = [], None
    for name, kind in zip(dusts, kinds):
        if kind == 'eqdust':
            with open(name) as fp:
                lines = fp.readlines()
            gd, radius = float(lines[1].split()[0]), float(lines[2].split()[0])
            d = np.loadtxt(name, skiprows=4, ndmin=2)
            FREQ = d[:, 0]
            cols.append(np.pi * radius ** 2.0 * gd * d[:, 2])
        else:
            sol = files.read_solver(solver_name(name))
            FREQ = np.asarray(sol["FREQ"], np.float64)
            cols.append(np.sum(np.asarray(sol["SK_ABS"], np.float64), axis=0))
    RABS = np.clip(np.asarray(cols, np.float64).T, 1.0e-40, 1.0e30)
    RABS /= (1.0e-40 + RABS.sum(axis=1))[:, None]
    return np.clip(RABS, 1.0e-30, 1.0), FREQ


def split_absorbed(ABSORBED, RABS, ABU, idust):
    """kernel_A2E_MABU_aux.c:3-23: OUT[c, f] = IN[c, f] * RABS[f, idust] / sum_j ABU[c, j] * RABS[f, j], with the kernel's
    types: the denominator accumulates in float (each product formed in double), the quotient is taken in double"""
    cells, nfreq = ABSORBED.shape
    ndust = RABS.shape[1]
    den = np.zeros((cells, nfreq), np.float32)
    for j in range(ndust):
        den = (den.astype(np.float64) + ABU[:, j:j + 1].astype(np.float64) * RABS[None, :, j]).astype(np.float32)
    return (ABSORBED.astype(np.float64) * RABS[None, :, idust] / den.astype(np.float64)).astype(np.float32)


# ---- polarisation <dust> <aalg file> ----------------------------------------------------------------------------------
def strip_dust(name):
    return name.replace('.dust', '')


def polarisation_lines(ini, dusts):
    """The `polarisation <dust> <aalg file>` lines of the ini (A2E_MABU.py:161-167) as a list along `dusts`: the aalg file of a
    dust, None for a dust without a line; None where the ini has no such line.  Names are compared with `.dust` stripped on both
    sides (a later line for the same dust replaces the earlier, as the reference's dict does)."""
    AALG, where = {}, {}
    with open(ini) as fp:
        for line in fp:
            s = line.split('#')[0].split()
            if len(s) > 0 and s[0][0:6] == 'polari':
                if len(s) < 3:
                    raise ValueError("%s: `%s`: the line must be `polarisation dust_name aalg_file_name`" % (ini, line.strip()))
                AALG[strip_dust(s[1])] = s[2]
                where[strip_dust(s[1])] = line.strip()
    if not AALG:
        return None
    known = [strip_dust(d) for d in dusts]
    for name in AALG:
        if name not in known:
            raise ValueError("%s: `%s` names a dust that is not in the ini (its dusts: %s)" % (ini, where[name], ", ".join(dusts)))
    return [AALG.get(k) for k in known]


def rpol_table(dust, FREQ):
    """<dust>.rpol (first row frequencies, first column sizes: R[a, freq], the share of the cross section in grains larger than a)
    interpolated to the frequencies FREQ (float32, as SolveEquilibriumDust holds them) as A2E_MABU.py:621-633 does per frequency: the
    column pick, the weight wj in log frequency -- 0 where the pick is the last column, negative below the first column -- and
    tmp = (1 - wj) * R[:, i] + wj * R[:, j].  Returns (apol[NA] increasing, tab[NFREQ, NA]) float64; the sizes are sorted as
    interp1d sorts them."""
    FREQ = np.asarray(FREQ, np.float32)
    d = np.loadtxt('%s.rpol' % strip_dust(dust), ndmin=2)
    Rpol, apol, fpol = d[1:, 1:], d[1:, 0], d[0, 1:]
    if len(apol) < 2 or len(fpol) < 1:
        raise ValueError("%s.rpol: at least two sizes and one frequency" % strip_dust(dust))
    order = np.argsort(apol, kind='mergesort')
    apol, Rpol = apol[order], Rpol[order]
    tab = np.zeros((len(FREQ), len(apol)), np.float64)
    for ifreq in range(len(FREQ)):
        i = np.argmin(abs(fpol - FREQ[ifreq]))
        if fpol[i] > FREQ[ifreq]:
            i = max([i - 1, 0])
        j = min([i + 1, len(fpol) - 1])
        if i == j:
            wj = 0.0
        else:
            wj = (np.log(FREQ[ifreq]) - np.log(fpol[i])) / (np.log(fpol[j]) - np.log(fpol[i]))
        tab[ifreq] = (1.0 - wj) * Rpol[:, i] + wj * Rpol[:, j]
    return np.ascontiguousarray(apol, np.float64), tab


def interp_rpol(apol, y, a):
    """interp1d(apol, y, bounds_error=False, fill_value=0.0)(a) written out (A2E_MABU.py:635): linear between the nodes --
    slope = (y1 - y0) / (x1 - x0), slope * (a - x0) + y0 in float64 --, the node's value on a node, 0 outside the nodes"""
    x = np.asarray(a, np.float64)
    j = np.clip(np.searchsorted(apol, x, side='right') - 1, 0, len(apol) - 2)
    with np.errstate(invalid='ignore', divide='ignore'):
        slope = (y[j + 1] - y[j]) / (apol[j + 1] - apol[j])
        out = slope * (x - apol[j]) + y[j]
    out = np.where(x == apol[j], y[j], out)
    out = np.where(x == apol[-1], y[-1], out)
    out = np.where((x < apol[0]) | (x > apol[-1]), 0.0, out)
    return np.where(np.isnan(x), x, out)


def polarised_eq(EM, aalg, apol, tab):
    """PEMITTED[:, f] = EMITTED[:, f] * ipR_f(aalg) (A2E_MABU.py:637): float32 times float64, rounded to float32 once"""
    PEM = np.zeros(EM.shape, np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for f in range(EM.shape[1]):
            PEM[:, f] = EM[:, f] * interp_rpol(apol, tab[f], aalg)
    return PEM


def reduction_factor(PSUM, SUM):
    """A2E_MABU.py:1182: polarised intensity -> polarisation reduction factor, float32"""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        return np.asarray(PSUM / (SUM + 1.0e-32), np.float32)


def abundance_table(ABU, single, CELLS, NDUST):
    """ABU[CELLS, NDUST] float32 from what files.read_abundances gave (None: no abundance file; with `singleabu` the first
    column x and 1-x for the two dusts, ASOC.py:1148-1153): ones where no file is given"""
    if ABU is None:
        return np.ones((CELLS, NDUST), np.float32)
    if single:
        if NDUST != 2:
            raise ValueError("singleabu assumes exactly two dust components")
        x = np.ravel(np.asarray(ABU, np.float32).reshape(CELLS, -1)[:, 0])
        return np.stack([x, 1.0 - x], axis=1).astype(np.float32)
    return np.asarray(ABU, np.float32).reshape(CELLS, NDUST)


# ---- the stage ------------------------------------------------------------------------------------------------------
MAKELIB_ONE_RANK = ("makelib with %d ranks: every rank holds a share of the cells, and a library is built from all of them "
                    "(from one rank and one cell range); build it with one rank")
MAKELIB_ONE_RANGE = ("makelib: the libraries are built on the device from one cell range, and the %d cells of this run need several (%s); "
                     "a library from part of the model would miss the rest: build it on a device that holds the cells, or with an engine "
                     "that takes the host path")


def _tables(dusts, kinds, NFREQ):
    """per dust what its solver needs: eq_dust_table of an equilibrium dust, the solver file of a stochastically heated one with
    the `nstoch` of its dust file (read_nstoch) under that key"""
    out = []
    for d, k in zip(dusts, kinds):
        if k == 'eqdust':
            out.append(eq_dust_table(d))
        else:
            sol = files.read_solver(solver_name(d))
            if sol["NFREQ"] != NFREQ:
                raise ValueError("absorbed file has %d frequencies, solver %d" % (NFREQ, sol["NFREQ"]))
            sol["nstoch"] = read_nstoch(d, k)
            out.append(sol)
    return out


def offers_device_path(engine, kinds, tables, polarised=False):
    """THE probe of the stage: the engine has the soc_mabu_* calls (with `polarisation` lines those too) and, where a size of a solver
    file is an equilibrium size (from the dust file's `nstoch` on, or without its tables in the solver file), a2e_resident_solve_eq,
    which solves those on the resident cells (without it they go through a2e.run's equilibrium branch, which works on host arrays)"""
    return hasattr(engine, "mabu_begin") and (not polarised or hasattr(engine, "mabu_pol_eq")) and \
        (hasattr(engine, "a2e_resident_solve_eq") or
         all(k == 'eqdust' or stochastic_sizes(t) >= t["NSIZE"] for k, t in zip(kinds, tables)))


def device_path_offered(engine, dusts, kinds, NFREQ, pol=None):
    """offers_device_path for a caller that has not read the tables: whether solve_emission will take its device path"""
    polarised = pol is not None and any(p is not None for p in pol)
    return offers_device_path(engine, kinds, _tables(dusts, kinds, NFREQ), polarised)


def _library_rows(grid, rows_of, NFREQ, FREQ):
    """the library of one dust from its grid (engine.library_build on its share) and rows_of(cells) -> the emission its solve left
    for those cells: clipped to [1e-30, 1e30], 1e32 in the bins without a representative (library.build does the same)"""
    N = int(grid["N"])
    m = np.nonzero(grid["IND"] >= 0)[0]
    E = np.full((N ** 3, NFREQ), 1.0e32, np.float32)
    if len(m):
        E[m, :] = np.clip(rows_of(grid["IND"][m]), np.float32(1.0e-30), np.float32(1.0e30))
    lib = dict(grid)
    lib.update(NFREQ=NFREQ, FREQ=np.asarray(FREQ, np.float32), E=E)
    return lib


def _solve_host(engine, dusts, kinds, tables, FABS, ABU, RABS, c0, CELLS, EM, log, AALG=None, ptabs=None, PEM=None, makelib=None, libs=None, TEMP=None):
    """TEMP: temperature_arrays' list, filled from what eqsolver and a2e.run's equilibrium sizes return"""
    n, NFREQ = FABS.shape
    for idust in range(len(dusts)):
        t0 = time.time()
        aalg = AALG[idust] if AALG else None
        pem = None
        teq = {} if (TEMP is not None and kinds[idust] != 'eqdust') else None
        part = split_absorbed(FABS, RABS, ABU, idust)
        if kinds[idust] == 'eqdust':
            Fq, KABS, Emin, kE, oplgkE, TTT = tables[idust]
            em = np.zeros((n, NFREQ), np.float32)
            B = 32768                                          # A2E_MABU.py:493 (any batch gives the same cells)
            for a in range(0, n, B):
                b = min(a + B, n)
                T, em[a:b] = engine.eqsolver(c0 + a, CELLS, NE_EQ, FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT, part[a:b])
                if TEMP is not None:
                    TEMP[idust][a:b] = T                       # A2E_MABU.py:543-551
            if aalg is not None:
                pem = polarised_eq(em, aalg, *ptabs[idust])    # A2E_MABU.py:615-637
        elif aalg is not None:                                 # (NSTOCH: the dust file's `nstoch`, A2E_MABU.py:938)
            em, pem, _ = a2e.run(engine, tables[idust], part, NSTOCH=tables[idust].get("nstoch", NSTOCH_ALL), verbose=False, aalg=aalg,
                                 teq=teq)   # A2E_MABU.py:971-984
        else:
            em, _ = a2e.run(engine, tables[idust], part, NSTOCH=tables[idust].get("nstoch", NSTOCH_ALL), verbose=False, teq=teq)
        for isize, T in (teq or {}).items():
            TEMP[idust][isize][:] = T
        if makelib is not None:                                # (cols, N, FREQ): the library of this dust, from what is at hand
            grid = engine.library_build(makelib[1], ABS3=np.ascontiguousarray(part[:, makelib[0]], np.float32))
            libs.append(_library_rows(grid, lambda cells: em[cells], NFREQ, makelib[2]))
        EM += em * ABU[:, idust:idust + 1]                     # A2E_MABU.py:1128-1140
        if pem is not None:
            PEM += pem * ABU[:, idust:idust + 1]               # A2E_MABU.py:1139-1147
        log("  dust %d/%d %-24s %s  %.2f s" % (idust + 1, len(dusts), dusts[idust], kinds[idust], time.time() - t0))
    return 1


def _solve_device(engine, dusts, kinds, tables, FABS, ABU, RABS, EM, range_cells, log, AALG=None, ptabs=None, R=None, resident_c0=None,
                  download=True, absorbed=None, makelib=None, libs=None, TEMP=None):
    """the cells in ranges that fit the device (one range where all do): cells are independent, so this is a loop.  With AALG (per
    dust the minimum aligned sizes of these cells, or None) the two more resident arrays of the polarised emission are asked for,
    the rows of a dust's aalg follow the cell range, and R receives polarised / total.  resident_c0 (the model's cell of row 0): the
    sum of every range also goes, device to device, to the engine's resident emission (emitted_begin); download=False: nowhere else.
    absorbed = (c0, K, nnnlimit): FABS is the engine's resident absorptions (absorbed_begin), row 0 the model's cell c0, and every
    range takes its rows from there, device to device, scaled on the way (absorbed_to_mabu), in place of the uploads.
    makelib = (cols, N, FREQ): after every dust's solve its library goes to libs -- the grid from library_build on the resident share
    (the plain split: where a reference column is the last channel, which clip_last changes, the share is split once more for the
    solver), the rows gathered from the resident emission.  One range then, or UnsupportedOption.
    TEMP: temperature_arrays' list -- after every dust's solve the rows of this range are read into it (mabu_download_t,
    a2e_resident_download_teq), before the next dust's solve reuses the device arrays they come from."""
    n, NFREQ = FABS.shape
    NDUST = len(dusts)
    if makelib is not None and range_cells and int(range_cells) < n:
        raise UnsupportedOption(MAKELIB_ONE_RANGE % (n, "the caller limits a range to %d" % int(range_cells)))

    def upload_aalg(aalg, a, b):
        for i in range(a, b, CHUNK):
            engine.a2e_resident_upload_aalg(i - a, aalg[i:min(i + CHUNK, b)])

    step = n if not range_cells else max(1, min(n, int(range_cells)))
    a = ranges = 0
    while a < n:
        b = min(a + step, n)
        t0 = time.time()
        try:
            if AALG:
                engine.mabu_begin(b - a, NFREQ, NDUST, polarised=True)
            else:
                engine.mabu_begin(b - a, NFREQ, NDUST)
        except DoesNotFit as err:
            if makelib is not None:
                raise UnsupportedOption(MAKELIB_ONE_RANGE % (n, "%d fit the free device memory" % err.cells_fit))
            step = err.cells_fit
            log("  %s" % err)
            continue
        try:
            if absorbed is not None:
                engine.absorbed_to_mabu(absorbed[0] + a, absorbed[1], absorbed[2])
            for i in range(a, b, CHUNK) if absorbed is None else ():
                engine.mabu_upload(i - a, FABS[i:min(i + CHUNK, b)])
            engine.mabu_set_tables(ABU[a:b], RABS)
            for idust in range(NDUST):
                aalg = AALG[idust] if AALG else None
                grid = None
                if kinds[idust] == 'eqdust':
                    Fq, KABS, Emin, kE, oplgkE, TTT = tables[idust]
                    engine.mabu_split(idust)
                    if makelib is not None:
                        grid = engine.library_build(makelib[1], cols=makelib[0])
                    engine.mabu_solve_eq(NE_EQ, FACTOR, kE, oplgkE, Emin, Fq, KABS, TTT)
                    for i in range(a, b, CHUNK) if TEMP is not None else ():
                        m = min(i + CHUNK, b) - i
                        engine.mabu_download_t(i - a, m, out=TEMP[idust][i:i + m])
                    if aalg is not None:                                           # A2E_MABU.py:615-637
                        upload_aalg(aalg, a, b)
                        engine.mabu_pol_eq(*ptabs[idust])
                else:
                    sol = tables[idust]
                    if makelib is not None and (NFREQ - 1) in list(makelib[0]):    # (the grid wants the share before the clip)
                        engine.mabu_split(idust)
                        grid = engine.library_build(makelib[1], cols=makelib[0])
                    engine.mabu_split(idust, clip_last=True)                       # A2E.py:184-185
                    if makelib is not None and grid is None:
                        grid = engine.library_build(makelib[1], cols=makelib[0])
                    if aalg is not None:
                        upload_aalg(aalg, a, b)
                    a2e.solve_sizes_resident(engine, sol, stochastic_sizes(sol), aalg is not None,   # (a refusal of a call ends the stage)
                                             keep_teq=TEMP is not None and len(TEMP[idust]) > 0)
                    for slot, isize in enumerate(a2e.eq_sizes(sol, stochastic_sizes(sol))) if TEMP is not None else ():
                        for i in range(a, b, CHUNK):
                            m = min(i + CHUNK, b) - i
                            engine.a2e_resident_download_teq(slot, i - a, m, out=TEMP[idust][isize][i:i + m])
                if grid is not None:
                    libs.append(_library_rows(grid, engine.mabu_gather_rows, NFREQ, makelib[2]))
                engine.mabu_accumulate(idust)
                if aalg is not None:
                    engine.mabu_accumulate_p(idust)                                # A2E_MABU.py:1139-1147
            if AALG:
                engine.mabu_ratio()                                                # A2E_MABU.py:1182
            if resident_c0 is not None:
                engine.emitted_from_mabu(resident_c0 + a)
            for i in range(a, b, CHUNK) if download else ():
                m = min(i + CHUNK, b) - i
                engine.mabu_download(i - a, m, out=EM[i:i + m])
                if AALG:
                    engine.mabu_download_p(i - a, m, out=R[i:i + m])
        finally:
            engine.mabu_end()
        ranges += 1
        log("  cells %d-%d of this rank: %d dusts  %.2f s" % (a, b, NDUST, time.time() - t0))
        a = b
    return ranges


def temperature_arrays(kinds, tables, n):
    """what solve_emission(temperatures=True) fills for n cells, a list along the dusts: T[n] of an equilibrium dust; {isize: T[n]} of a
    stochastically heated one, for its equilibrium sizes only (a2e.eq_sizes: from the dust file's `nstoch` on or without tables in the
    solver file, less those with S_FRAC < 1e-30) -- empty where every size is stochastically heated"""
    return [np.zeros(n, np.float32) if k == 'eqdust' else {isize: np.zeros(n, np.float32) for isize in a2e.eq_sizes(t, stochastic_sizes(t))}
            for k, t in zip(kinds, tables)]


def offers_temperatures(engine, kinds, tables):
    """whether the device path can hand out the temperatures: mabu_download_t, and a2e_resident_keep_teq where a size is an equilibrium size"""
    return hasattr(engine, "mabu_download_t") and \
        (hasattr(engine, "a2e_resident_keep_teq") or all(k == 'eqdust' or not a2e.eq_sizes(t, stochastic_sizes(t)) for k, t in zip(kinds, tables)))


def solve_emission(engine, dusts, kinds, FABSORBED, ABU, rank=0, world=1, *, path=None, range_cells=None, log=None, pol=None,
                   keep_resident=False, download=True, absorbed_scale=None, makelib=None, temperatures=False):
    """Stage 2 of a multi-dust run for the cells a2e.cell_range(CELLS, rank, world) of this rank.  FABSORBED[CELLS, NFREQ] as the
    absorbed file holds it (scaled, files.scale_absorbed; a memory map will do), ABU[CELLS, NDUST] float32.  Or FABSORBED a
    ResidentAbsorptions -- the engine holds them unscaled (absorbed_begin) -- with absorbed_scale = (K[LEVELS], nnnlimit)
    (files.absorbed_scale_factors): the device path alone, which scales them on their way to its rows.
    Returns (EM[c1 - c0, NFREQ], info) with info["path"] 'device' or 'host' and info["ranges"], the number of cell ranges.
    path: None = the device path where the engine offers it, or 'device' / 'host' to insist (tests, measurements);
    range_cells: an upper limit for the cells resident at a time (default: what the free device memory takes);
    pol: polarisation_lines' list -- per dust its aalg file or None; info["R"] is then R[c1 - c0, NFREQ], polarised / total;
    keep_resident: on the device path the sum also goes to the engine's resident emission (engine.emitted_begin was called: the
    cell-emission launches of a re-emission iteration take it from there) -- info["resident"] says whether it did; download=False:
    where it did, the sum is not read back (EM, and R, stay zero: an intermediate iteration needs neither on the host);
    makelib = (cols[3], N): info["libraries"] is, per dust, its library (the dict library.write_library takes, with IND besides), a
    by-product of the solve, which it does not change -- one rank and, on the device path, one cell range, else UnsupportedOption;
    temperatures: info["T"] is temperature_arrays' list for the cells of this rank -- what the solvers compute on the way to the
    emission (A2E_MABU.py:551, A2E.py:506-522), 4 bytes per cell and dust or equilibrium size read back on the device path, the same
    bits on both paths; the emission does not change.  The populations of stochastically heated sizes are not offered here (CELLS x NE
    floats per size: soc_amd.a2e's dump).  An engine whose device path lacks the calls for them is refused by name."""
    log = log or (lambda *a: None)
    CELLS, NFREQ = FABSORBED.shape
    RABS, FREQ = relative_cross_sections(dusts, kinds)
    libs = None
    if makelib is not None:
        if world > 1:
            raise UnsupportedOption(MAKELIB_ONE_RANK % world)
        cols, N = np.asarray(makelib[0], np.int32), int(makelib[1])
        if cols.size != 3 or cols.min() < 0 or cols.max() >= NFREQ or not 2 <= N <= 64:
            raise ValueError("makelib: three reference columns below %d and 2 <= N <= 64 (got %s, %d)" % (NFREQ, cols, N))
        makelib, libs = (cols, N, FREQ), []
    if RABS.shape[0] != NFREQ:
        raise ValueError("the dusts have %d frequencies, the absorptions %d" % (RABS.shape[0], NFREQ))
    tables = _tables(dusts, kinds, NFREQ)
    c0, c1 = a2e.cell_range(CELLS, rank, world)
    AALG = ptabs = None
    if pol is not None and any(p is not None for p in pol):
        AALG = [None if p is None else a2e.read_aalg(p, CELLS)[c0:c1] for p in pol]
        ptabs = [rpol_table(d, t[0]) if (p is not None and k == 'eqdust') else None for d, k, t, p in zip(dusts, kinds, tables, pol)]
    offered = offers_device_path(engine, kinds, tables, AALG is not None)
    if path not in (None, 'device', 'host') or (path == 'device' and not offered):
        raise ValueError("solve_emission: path %r is not available with this engine and these solver files" % (path,))
    device = offered if path is None else path == 'device'
    if temperatures and device and not offers_temperatures(engine, kinds, tables):
        raise UnsupportedOption("temperatures: the engine's device path has no mabu_download_t / a2e_resident_keep_teq "
                                "(path='host' takes them from the host solvers)")
    from_resident = isinstance(FABSORBED, ResidentAbsorptions)
    if from_resident and (not device or absorbed_scale is None):
        raise ValueError("solve_emission: the resident absorptions need the device path and absorbed_scale = (K, nnnlimit)")
    EM = np.zeros((c1 - c0, NFREQ), np.float32)
    R = np.zeros((c1 - c0, NFREQ), np.float32) if AALG else None
    TEMP = temperature_arrays(kinds, tables, c1 - c0) if temperatures else None
    ranges = 0
    resident = bool(keep_resident) and device and c1 > c0
    if c1 > c0 and device:
        ranges = _solve_device(engine, dusts, kinds, tables, ResidentAbsorptions(engine, c1 - c0, NFREQ) if from_resident else FABSORBED[c0:c1],
                               ABU[c0:c1], RABS, EM, range_cells, log, AALG, ptabs, R, resident_c0=c0 if resident else None,
                               download=download or not resident, absorbed=(c0,) + tuple(absorbed_scale) if from_resident else None,
                               makelib=makelib, libs=libs, TEMP=TEMP)
    elif c1 > c0:
        ranges = _solve_host(engine, dusts, kinds, tables, FABSORBED[c0:c1], ABU[c0:c1], RABS, c0, CELLS, EM, log, AALG, ptabs, R,
                             makelib=makelib, libs=libs, TEMP=TEMP)
        if AALG:
            R[:] = reduction_factor(R, EM)                         # (R held the sum of the polarised emission)
    info = dict(path='device' if device else 'host', ranges=ranges, resident=resident)
    if AALG:
        info["R"] = R
    if libs is not None:
        info["libraries"] = libs
    if TEMP is not None:
        info["T"] = TEMP
    return EM, info


TEMPERATURES_ONE_RANK = ("temperatures with %d ranks: every rank solves a share of the cells, and a temperature file holds all of them; "
                         "run it with one rank")
TEMPERATURES_NO_LIBRARY = ("temperatures together with a library look-up (%s): a library answers with the emission, nothing is solved, "
                           "so there is no temperature")


def temperature_files(dusts, kinds, TEMP):
    """[(file name, header or None, T[CELLS])] of info["T"]: '<dust>.T' with the name as the ini gives it, raw float32 (A2E_MABU.py:551),
    for an equilibrium dust; <solver name without .solver>_size%03d.dump with the header {CELLS, 1} (A2E.py:506-522, run there by
    A2E_MABU.py:938 on the dust's solver file) for every equilibrium size of a stochastically heated one"""
    out = []
    for d, k, T in zip(dusts, kinds, TEMP):
        if k == 'eqdust':
            out.append(('%s.T' % d, None, T))
        else:
            out += [(a2e.dump_name(solver_name(d).replace('.solver', ''), isize), (len(T[isize]), 1), T[isize]) for isize in sorted(T)]
    return out


def write_temperatures(dusts, kinds, TEMP, log=None):
    for name, header, T in temperature_files(dusts, kinds, TEMP):
        with open(name, 'wb') as fp:
            if header is not None:
                np.asarray(header, np.int32).tofile(fp)
            np.asarray(T, np.float32).tofile(fp)
        if log:
            log("  %s: %d temperatures" % (name, len(T)))


# ---- the look-up: a library per dust ------------------------------------------------------------------------------------
def write_libraries(dusts, libs, log=None):
    """<dust>.mlib of every dust, what solve_emission(makelib=...) left in info["libraries"]"""
    for d, lib in zip(dusts, libs):
        library.write_library(library_name(d), lib)
        if log:
            log("  %s: (N=%d)^3 = %d bins, cells existed for %d" % (library_name(d), lib["N"], lib["N"] ** 3, int(np.sum(lib["IND"] >= 0))))


def require_libraries(dusts, lfreq='lfreq.dat'):
    """a library per dust, or an error that names the missing file and says how it is made"""
    for d in dusts:
        if not os.path.exists(library_name(d)):
            raise FileNotFoundError("%s: the library of %s is missing; a run with all frequencies writes it: "
                                    "python -m soc_amd.mabu soc.ini absorbed.data emitted.data --makelib %s" % (library_name(d), d, lfreq))


def read_libraries(dusts, NFREQ, lfreq='lfreq.dat'):
    """the libraries of the dusts (require_libraries first)"""
    require_libraries(dusts, lfreq)
    libs = []
    for d in dusts:
        name = library_name(d)
        lib = library.read_library(name)
        if lib["E"].shape[1] != NFREQ:
            raise ValueError("%s holds %d frequencies, the dusts %d" % (name, lib["E"].shape[1], NFREQ))
        libs.append(lib)
    return libs


def _lookup_host(engine, ABS3, ABU, RABS3, libs, ocol, EM, MISS):
    """the composition the fused kernel equals bit for bit: per dust the split, the look-up with missed rows zeroed, the weighted sum"""
    for d, lib in enumerate(libs):
        part = split_absorbed(ABS3, RABS3, ABU, d)
        engine.library_set(lib, ocol)
        try:
            for a in range(0, len(part), CHUNK):
                EMI, miss = engine.library_solve(part[a:a + CHUNK])
                EMI[miss, :] = 0.0
                EM[a:a + CHUNK] += EMI * ABU[a:a + CHUNK, d:d + 1]
                MISS[a + np.asarray(miss, np.int64)] |= np.uint32(1 << d)
        finally:
            engine.library_set(None)


def _lookup_device(engine, ABS3, ABU, RABS3, libs, ocol, EM, MISS, range_cells, log):
    n, nout = EM.shape
    step = n if not range_cells else max(1, min(n, int(range_cells)))
    a = ranges = 0
    while a < n:
        b = min(a + step, n)
        try:
            engine.mabu_library_begin(b - a, len(libs), nout)
        except DoesNotFit as err:
            step = err.cells_fit
            log("  %s" % err)
            continue
        try:
            for d, lib in enumerate(libs):
                engine.mabu_library_set(d, lib, ocol)
            for i in range(a, b, CHUNK):
                engine.mabu_library_upload(i - a, ABS3[i:min(i + CHUNK, b)])
            engine.mabu_library_set_tables(ABU[a:b], RABS3)
            engine.mabu_library_solve()
            for i in range(a, b, CHUNK):
                m = min(i + CHUNK, b) - i
                engine.mabu_library_download(i - a, m, out=EM[i:i + m])
                MISS[i:i + m] = engine.mabu_library_misses(i - a, m)
        finally:
            engine.mabu_library_end()
        ranges += 1
        a = b
    return ranges


def solve_emission_library(engine, dusts, kinds, ABS3, ABU, libs, cols, ocol=None, full=None, *, path=None, range_cells=None, log=None):
    """Stage 2 from the libraries of the dusts (read_libraries): ABS3[CELLS, 3], the absorptions at the reference frequencies -- the
    columns cols[3] of the dusts' frequency table --, as a `libabs` run's absorbed file holds them; ABU[CELLS, NDUST] float32.
    Returns (EM[CELLS, nout], info): nout the libraries' frequencies, or those ocol selects and orders.  info["missed"] holds per dust
    the number of cells its library had no answer for -- such a (cell, dust) adds zero --, info["miss"] the uint32 mask per cell (bit d:
    dust d), info["path"] 'device' (the fused kernel, where the engine has mabu_library_begin) or 'host' (the composition around
    engine.library_solve), with the same bits; path insists on one.  full = FABSORBED[CELLS, NFREQ], the absorptions at all
    frequencies: every cell with a miss in any dust is then solved directly, all dusts (solve_emission on the gathered rows), and
    its row overwritten; info["solved"] are those cells."""
    log = log or (lambda *a: None)
    ABS3 = np.asarray(ABS3)
    CELLS = ABS3.shape[0]
    NDUST = len(dusts)
    if ABS3.ndim != 2 or ABS3.shape[1] != 3 or ABU.shape != (CELLS, NDUST) or len(libs) != NDUST:
        raise ValueError("solve_emission_library: ABS3[CELLS, 3], ABU[CELLS, %d] and a library per dust" % NDUST)
    if NDUST > 32:
        raise UnsupportedOption("%d dusts: a library run takes at most 32 (the width of the miss mask)" % NDUST)
    RABS, FREQ = relative_cross_sections(dusts, kinds)
    cols = np.asarray(cols, np.int64)
    if cols.size != 3 or cols.min() < 0 or cols.max() >= RABS.shape[0]:
        raise ValueError("solve_emission_library: three reference columns below %d" % RABS.shape[0])
    RABS3 = np.ascontiguousarray(RABS[cols])
    NFREQ = int(libs[0]["E"].shape[1])
    if any(int(lib["E"].shape[1]) != NFREQ for lib in libs):
        raise ValueError("the libraries hold different numbers of frequencies: %s" % [int(lib["E"].shape[1]) for lib in libs])
    oc = None if ocol is None else np.asarray(ocol, np.int32)
    nout = NFREQ if oc is None else int(oc.size)
    offered = hasattr(engine, "mabu_library_begin")
    if path not in (None, 'device', 'host') or (path == 'device' and not offered):
        raise ValueError("solve_emission_library: path %r is not available with this engine" % (path,))
    device = offered if path is None else path == 'device'
    EM, MISS = np.zeros((CELLS, nout), np.float32), np.zeros(CELLS, np.uint32)
    ranges = 1
    if CELLS > 0 and device:
        ranges = _lookup_device(engine, ABS3, np.ascontiguousarray(ABU, np.float32), RABS3, libs, oc, EM, MISS, range_cells, log)
    elif CELLS > 0:
        _lookup_host(engine, np.ascontiguousarray(ABS3, np.float32), ABU, RABS3, libs, oc, EM, MISS)
    missed = [int(np.count_nonzero(MISS & np.uint32(1 << d))) for d in range(NDUST)]
    info = dict(path='device' if device else 'host', ranges=ranges, missed=missed, miss=MISS, resident=False)
    if full is not None:
        cells = np.flatnonzero(MISS)
        info["solved"] = cells
        if len(cells):
            rows = np.ascontiguousarray(np.asarray(full)[cells, :], np.float32)
            direct, _ = solve_emission(engine, dusts, kinds, rows, np.ascontiguousarray(ABU[cells]), log=log)
            EM[cells, :] = direct if oc is None else direct[:, oc]
    return EM, info


def print_misses(dusts, info, CELLS, full, out=print):
    """per dust what soc_library.py:484-490 prints for its one"""
    for d, m in zip(dusts, info["missed"]):
        if m < 1:
            out("*** %s: all cells matched by entries in the library ***" % d)
        elif full:
            out("*** %s: %d cells without answer in the library, %.3f %% of all cells: solved directly" % (d, m, 100.0 * m / max(CELLS, 1)))
        else:
            out("*** %s: %d cells without answer in the library, and the absorptions hold 3 frequencies only:" % (d, m))
            out("***    the emission of this dust in those cells is set to ZERO")


def reference_columns_ascending(FREQ, FREF, what):
    """library.reference_columns for the columns of an absorbed file, which follow the frequency table: they must ascend"""
    cols = library.reference_columns(FREQ, FREF)
    if not (cols[0] < cols[1] < cols[2]):
        raise ValueError("%s: the three reference frequencies must be distinct frequencies of the dusts' table in its order "
                         "(columns %s): the three columns of a libabs run's absorbed file follow the table" % (what, list(cols)))
    return cols


# ---- the program ----------------------------------------------------------------------------------------------------
def run(ini, absorbed, emitted, engine, comm=None, ofreq=None, verbose=False, makelib=None, uselib=None, temperatures=False, **stage):
    """The whole program for one rank of `comm` (or alone): memory-map the absorbed file, solve this rank's cells, write them
    into this rank's rows of the emitted file.  No collective on the data path (as a2e.run_sharded): the ranks only wait for
    rank 0 to have created the file, and for each other at the end.  Returns solve_emission's info.
    makelib = (lfreq file, N): the libraries <dust>.mlib are written besides; uselib = lfreq file, or `libabs` in the ini with an
    absorbed file of three columns: the emission comes from those libraries (solve_emission_library; ofreq selects its columns).
    temperatures: the temperature files are written besides (temperature_files); one rank and no library look-up, else refused."""
    rank, world = (comm.rank, comm.world) if comm else (0, 1)
    U = User(ini)
    dusts = list(U.file_optical)
    if len(dusts) < 1:
        raise ValueError("%s names no dust (keyword optical)" % ini)
    pol = polarisation_lines(ini, dusts)
    dims = np.fromfile(absorbed, np.int32, 2)
    CELLS, NFREQ = int(dims[0]), int(dims[1])
    lookup = uselib is not None or ('libabs' in U.KEYS and NFREQ == 3)
    if ofreq is not None and not lookup:
        raise UnsupportedOption("a fourth argument (%s: emission on a subset of the frequencies, A2E_MABU.py ofreq.dat) is not supported "
                                "for a direct run: the emitted file holds every frequency of the absorbed file" % ofreq)
    refuse(U, pol, world)
    if temperatures and world > 1:                                 # (before rank 0 creates the emitted file)
        raise UnsupportedOption(TEMPERATURES_ONE_RANK % world)
    if temperatures and lookup:
        raise UnsupportedOption(TEMPERATURES_NO_LIBRARY % ("uselib" if uselib is not None else "libabs"))
    if uselib is not None and (pol is not None or world > 1):
        raise UnsupportedOption("uselib together with %s" % ("polarisation lines (no polarised emission comes from a library)"
                                                               if pol is not None else "more than one rank"))
    kinds = [dust_kind(d) for d in dusts]
    require_solvers(dusts, kinds)
    ABU = abundance_table(files.read_abundances(U.file_abundance, CELLS), U.SINGLE_ABU, CELLS, len(dusts))
    log = print if (verbose and rank == 0) else None
    if lookup:
        if makelib is not None:
            raise UnsupportedOption("makelib in a run that takes its emission from the libraries: they are built from a direct solve")
        FREQ = relative_cross_sections(dusts, kinds)[1]
        FABS = np.memmap(absorbed, dtype=np.float32, mode='r', offset=8, shape=(CELLS, NFREQ))
        if NFREQ == 3:
            if 'libabs' not in U.KEYS:
                raise UnsupportedOption("%s holds three columns: the ini must name their frequencies (`libabs FILE`)" % absorbed)
            if U.FSELECT_ERROR:
                raise ValueError(U.FSELECT_ERROR)
            fsel = U.FSELECT_LIB_ABS if U.FSELECT_LIB_ABS is not None else U.FSELECT
            cols, ABS3, full = reference_columns_ascending(FREQ, np.asarray(fsel, np.float64), "libabs"), FABS, None
        else:
            if NFREQ != len(FREQ):
                raise ValueError("%s holds %d frequencies: 3 or the dusts' %d" % (absorbed, NFREQ, len(FREQ)))
            cols = reference_columns_ascending(FREQ, library.load_frequencies(uselib), "uselib")
            ABS3, full = np.ascontiguousarray(FABS[:, cols], np.float32), FABS
        libs = read_libraries(dusts, len(FREQ), "lfreq.dat" if uselib is None else uselib)
        ocol = None
        if ofreq is not None:                                      # soc_library.py:298-306: the nearest library frequencies
            ocol = np.asarray([np.argmin(np.abs(f - libs[0]["FREQ"].astype(np.float64))) for f in library.load_frequencies(ofreq)], np.int32)
        EM, info = solve_emission_library(engine, dusts, kinds, ABS3, ABU, libs, cols, ocol, full, log=log, **stage)
        if rank == 0:
            print_misses(dusts, info, CELLS, full is not None)
        files.write_emitted(emitted, EM)
        return info
    if 'libabs' in U.KEYS and log:
        log("mabu: `libabs` in the ini, but %s holds %d columns: a direct run" % (absorbed, NFREQ))
    FABS = np.memmap(absorbed, dtype=np.float32, mode='r', offset=8, shape=(CELLS, NFREQ))
    if makelib is not None:
        if world > 1:                                              # (before rank 0 creates the emitted file)
            raise UnsupportedOption(MAKELIB_ONE_RANK % world)
        FREQ = relative_cross_sections(dusts, kinds)[1]
        stage["makelib"] = (library.reference_columns(FREQ, library.load_frequencies(makelib[0])), int(makelib[1]))
    if world == 1:
        EM, info = solve_emission(engine, dusts, kinds, FABS, ABU, log=log, pol=pol, temperatures=bool(temperatures), **stage)
        files.write_emitted(emitted, EM)
        if temperatures:
            write_temperatures(dusts, kinds, info["T"], log)
        if makelib is not None:
            write_libraries(dusts, info.pop("libraries"), log)
        if pol is not None:
            write_reduction(emitted + '.R', info.pop("R"))
        return info
    if rank == 0:
        files.create_absorbed(emitted, CELLS, NFREQ)            # (the emitted file has the layout of the absorbed file)
        if pol is not None:
            with open(emitted + '.R', 'wb') as fp:
                np.asarray([CELLS], np.int32).tofile(fp)
                fp.truncate(4 + 4 * CELLS * NFREQ)
    comm.barrier()
    EM, info = solve_emission(engine, dusts, kinds, FABS, ABU, rank, world, log=log, pol=pol, **stage)
    c0, c1 = a2e.cell_range(CELLS, rank, world)
    if c1 > c0:
        for name, offset, rows in [(emitted, 8, EM)] + ([(emitted + '.R', 4, info.pop("R"))] if pol is not None else []):
            out = np.memmap(name, dtype=np.float32, mode='r+', offset=offset, shape=(CELLS, NFREQ))
            out[c0:c1, :] = rows
            out.flush()
            del out
    comm.barrier()
    return info


def write_reduction(filename, R):
    """<emitted>.R (A2E_MABU.py:1188-1198): the header is {CELLS} alone (the layout of a `polred` file), then R[CELLS, NFREQ] float32"""
    with open(filename, 'wb') as fp:
        np.asarray([R.shape[0]], np.int32).tofile(fp)
        np.asarray(R, np.float32).tofile(fp)


def parse_options(argv, names):
    """(positional arguments, {name: value}) of a command line with `--name VALUE` options; None for one without its value"""
    opts, args = {}, []
    it = iter(argv)
    for a in it:
        if a.startswith("--") and a[2:] in names:
            opts[a[2:]] = next(it, None)
            if opts[a[2:]] is None:
                print("%s needs a value" % a)
                return None, None
        else:
            args.append(a)
    return args, opts


def makelib_option(opts):
    """(lfreq file, N) of --makelib LFREQ [--bins N], or None; ValueError for an N outside 2..64"""
    if "makelib" not in opts:
        if "bins" in opts:
            raise ValueError("--bins goes with --makelib")
        return None
    N = int(opts.get("bins", 30))
    if not 2 <= N <= 64:
        raise ValueError("--bins %d: 2 <= N <= 64" % N)
    return opts["makelib"], N


def main(argv=None):
    argv = sys.argv if argv is None else argv
    args, opts = parse_options(argv, ("makelib", "bins", "uselib"))
    temperatures = args is not None and "--temperatures" in args
    if temperatures:
        args = [a for a in args if a != "--temperatures"]
    if args is None or len(args) < 4:
        print("Usage:  python -m soc_amd.mabu  soc.ini absorbed emitted [ofreq.dat] [--makelib LFREQ [--bins N]] [--uselib LFREQ] [--temperatures]")
        print("        (N GPUs: python -m torch.distributed.run --nproc-per-node N -m soc_amd.mabu ...)")
        return 1
    try:
        makelib = makelib_option(opts)
    except ValueError as err:
        print(err)
        return 1
    from .dist import Comm
    comm = Comm()                      # (imports torch first when there are several ranks: see lib.load_library)
    from .lib import Engine
    t0 = time.time()
    eng = Engine(comm.local_rank)
    try:
        info = run(args[1], args[2], args[3], eng, comm if comm.world > 1 else None, ofreq=args[4] if len(args) > 4 else None,
                   verbose=True, makelib=makelib, uselib=opts.get("uselib"), temperatures=temperatures)
    except UnsupportedOption as err:
        if not temperatures:
            raise
        print(err)
        return 1
    finally:
        eng.close()
        comm.close()
    if comm.rank == 0:
        print('@@  mabu %.3f SECONDS   (%s path, %d cell range%s on rank 0, %d ranks)'
              % (time.time() - t0, info["path"], info["ranges"], "" if info["ranges"] == 1 else "s", comm.world))
    return 0


if __name__ == "__main__":
    sys.exit(main())
