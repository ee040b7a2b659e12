#!/usr/bin/env python3
"""driver -- the three stages of a SOC run with several dust components, in one process and in memory:

    python -m soc_amd.driver soc.ini [--keep-files] [--makelib LFREQ [--bins N]] [--temperatures]

Counterpart of ``ASOC_driver.py soc.ini`` + ``A2E_MABU.py`` (reference ASOC_driver.py:200-473, A2E_MABU.py:236-342,
700-1180): the reference chains three programs with os.system and hands the absorptions (CELLS x NFREQ floats: 5-17 GB
at config 3) and the emission over through files.  Here

  1. the radiative-transfer run (soc_amd.asoc.AbsorptionRun with the simple dusts, absorptions kept per frequency,
     `nomap`, `nosolve`: what rt_simple.ini asks for, ASOC_driver.py:230-252) returns FABSORBED[CELLS, NFREQ];
  2. for every dust component the absorptions are split in proportion to cross section x abundance
     (split_absorbed, kernel_A2E_MABU_aux.c:3-23; RABS as A2E_MABU.py:245-342) and the emission is solved -- an
     equilibrium component with soc_eqsolver (SolveEquilibriumDust, A2E_MABU.py:436-640 -> kernel_eqsolver.c), a
     stochastically heated one with soc_amd.a2e.run on its <dust>.solver file (A2E.py) -- and summed weighted by the
     abundances (A2E_MABU.py:1128-1140): soc_amd.mabu.solve_emission, the stage that python -m soc_amd.mabu runs alone -- on
     the device from the absorptions to the sum where the engine has the soc_mabu_* calls; the sizes from the `nstoch N` of a
     gsetdust file on (A2E_MABU.py:124-143) are solved at their equilibrium temperature, on the device as well
     (a2e_resident_solve_eq), so such a dust takes neither stage 2 nor the resident emission and absorptions below off the device;
  3. the maps are written from that emission array (AbsorptionRun.write_maps: maps.ini of ASOC_driver.py:447-473).

Same ini keys, same dust / solver / abundance / cloud files.  `emitted` is written (it is a product); the
`absorbed` file only with --keep-files.  `polarisation <dust> <aalg file>` lines (A2E_MABU.py:158-167) go to the same stage 2: the
polarisation reduction factor R[CELLS, NFREQ] stays in memory, and where the ini asks for `polmap` without `polred` every polarisation
map is made with the column of its own frequency (the reference writes <emitted>.R and needs one column copied into a `polred` file by
hand, A2E_MABU.py:1190-1195); with `polred` the file wins; --keep-files writes <emitted>.R as well.  The neural-network
shortcuts (nnmake, nnsolve ...) and cosmic-ray heating are not part of this path and are refused.  With several ranks the
first stage shards work items (soc_amd.dist), the second the cells; rank 0 writes.

The library method (`ASOC_driver.py soc-ini [uselib] [makelib]`): --makelib LFREQ [--bins N] writes a library <dust>.mlib per dust as a
by-product of the full run (soc_amd.mabu), whose products do not change; not with re-emission iterations (build the libraries from the
absorbed file of the finished model with python -m soc_amd.mabu --makelib).  With `libabs FILE` in the ini stage 1 simulates the three
frequencies of FILE only, their absorptions go to stage 2 as a host array [CELLS, 3] (12 bytes per cell; the resident-absorptions
sink holds all frequencies and is not used), stage 2 is the look-up in those libraries (mabu.solve_emission_library) and stage 3
writes all frequencies -- or, with `libmaps FILE2` as well, the maps of the frequencies of FILE2 from an emission array of just
those columns, the bytes python -m soc_amd.asoc with `libmaps` writes from the emitted file written here.  `libmaps` without
`libabs` is refused; with a library run also re-emission iterations, `polarisation` lines, saveint, nnmake / absthin and several ranks.

--temperatures (Pipeline(temperatures=True)): stage 2 also hands out the dust temperatures it computes (mabu.solve_emission with
temperatures: 4 bytes per cell and equilibrium dust or equilibrium size, read back after each dust's solve on the device path, which
stays in use, as do the resident emission and absorptions), and rank 0 writes the files python -m soc_amd.mabu --temperatures writes
from the absorbed file: '<dust>.T' and <solver name>_size%03d.dump (A2E_MABU.py:551, A2E.py:506-522).  With re-emission iterations the
temperatures of every step's solve are kept and those of the step whose emission is the product -- the last, or the one `convergence`
stopped at -- are written, once, after the loop.  One rank, and not in a library run (nothing is solved there), else refused.

Dust re-emission (`iterations N` with `cellpackets`): the constant sources are simulated once and their absorptions C kept unscaled;
E_0 is solved from them; then, N times, the emission E_(k-1) is sent from the cells at every simulated frequency (SimRAM_CL, as a run
with `iterations 1` and `nosolve` that reads the emitted file of the iteration before: the same packet seeds, the host generator of
`emweight` made anew), its absorptions are added to a copy of C, and E_k is solved from the sum -- the chain
soc_amd.asoc, soc_amd.mabu, soc_amd.asoc ... without its files.  The products are those of the last iteration.  Where the engine has
the soc_emitted_* calls, stage 2 took its device path, there is one rank and `emweight 0`, the emission does not leave the device
between the iterations: stage 2 leaves it transposed, ET[NFREQ][CELLS], and every launch makes its EMIT[CELLS] from one contiguous
row (soc_set_emission_column); otherwise it goes through the host array and soc_set_emission, with the same bits.  The absorptions
stay there as well, with or without iterations, where the engine has the soc_absorbed_* calls, there is one rank, no `saveint` and
stage 2 offers its device path: every INT tally is added to its row of AT[NFREQ][CELLS], a second plane keeps the constant sources'
share, and stage 2 takes its rows from there scaled with the bits of files.scale_absorbed (open_absorbed).  `convergence eps [kmin]`
(not a key of the reference, which has no criterion: N is what the ini says) ends the loop after the first step k >= kmin whose
luminosity-weighted relative change of the emission d_l1 (soc_amd.converge) is below eps; the products are then those of `iterations k`,
the figures of every step go to convergence.dat, timers["convergence"] and the log, and `converged` is the step or None.  The figures
come from the resident emission (engine.emitted_change: one pass, one plane of CELLS doubles kept) where the step left it there, else
from the host array.  Refused with
iterations: `ali` (the escape probability feeds a temperature solve that this pipeline does not do), `reference` (the reference field
needs the previous emission and its absorptions carried across the iterations) and a `remit` that cuts frequencies.
"""
import sys
import time

import numpy as np

from . import a2e, converge, files, launch, library, mabu
from .asoc import AbsorptionRun, ResidentAbsorptions, UnsupportedOption
from .ini import User
from .lib import DoesNotFit

# the stage-2 arithmetic lives in soc_amd.mabu (the program that runs it alone); the names stay importable from here
from .mabu import (NE_EQ, dust_kind, eq_dust_table, planck_safe, relative_cross_sections, simple_name, solver_name,   # noqa: F401
                   split_absorbed)


class Pipeline:
    """soc.ini -> maps.  engine: soc_amd.lib.Engine (or an object with its methods); comm: soc_amd.dist.Comm"""

    def __init__(self, ini, engine, comm=None, verbose=None, emission_source=None, absorbed_source=None, makelib=None, temperatures=False):
        """makelib = (lfreq file, N): the libraries <dust>.mlib are written besides (mabu.solve_emission(makelib=...));
        temperatures: the temperature files of soc_amd.mabu are written besides (mabu.write_temperatures), from stage 2;
        emission_source: None -- the re-emission iterations take the resident emission where they can (see iterate) -- or 'host' to
        keep them on the host statements (tests, measurements); absorbed_source: the same for the absorptions on their way from the
        transfer stage to stage 2 (see open_absorbed)"""
        if emission_source not in (None, 'host'):
            raise ValueError("emission_source: None or 'host'")
        if absorbed_source not in (None, 'host'):
            raise ValueError("absorbed_source: None or 'host'")
        self.emission_source = emission_source
        self.absorbed_source = absorbed_source
        self.comm = comm
        self.rank = comm.rank if comm else 0
        self.world = comm.world if comm else 1
        self.eng = engine
        U = User(ini)
        self.U = U
        # dust list as the user wrote it, and the simple dusts the transfer run works with (ASOC_driver.py:240-250)
        self.dusts = list(U.file_optical)
        self.pol = mabu.polarisation_lines(ini, self.dusts)       # per dust its aalg file or None; None without such lines
        self.refuse(U, self.pol, self.world)
        self.kinds = [dust_kind(d) for d in self.dusts]
        # the library method: `libabs` makes this a library run (run_library); `libmaps` names the frequencies it maps.  The transfer
        # run sees `libabs` alone (one list of frequencies serves both keys there, and it refuses the two together)
        self.library = 'libabs' in U.KEYS
        self.makelib = makelib
        self.temperatures, self.T = bool(temperatures), None
        if self.temperatures and self.world > 1:
            raise UnsupportedOption(mabu.TEMPERATURES_ONE_RANK % self.world)
        if self.temperatures and self.library:
            raise UnsupportedOption(mabu.TEMPERATURES_NO_LIBRARY % "libabs")
        self.fmaps = None
        if makelib is not None and (self.library or (U.ITERATIONS > 0 and U.CLPAC > 0)):
            raise UnsupportedOption("makelib %s" % ("in a library run (libabs): the libraries are built from a run with all frequencies" if self.library else
                                                    "with dust re-emission iterations (iterations with cellpackets): no step of the loop knows that it is "
                                                    "the last; build the libraries from the absorbed file of the finished model (--keep-files) with "
                                                    "python -m soc_amd.mabu --makelib"))
        if self.library:
            if U.FSELECT_ERROR:
                raise ValueError(U.FSELECT_ERROR)
            if U.LIB_MAPS:
                if getattr(U, "MAP_LEVELS", 0) > 0:
                    raise UnsupportedOption("libmaps with maplevels (the per-level maps go through the batch path, libmaps through the plain one)")
                self.fmaps = np.asarray(U.FSELECT_LIB_MAPS, np.float64)
            U.LIB_MAPS, U.FSELECT = False, U.FSELECT_LIB_ABS
            mabu.require_libraries(self.dusts)
        self.R = None
        U.file_optical = [d if k != 'gsetdust' else simple_name(d) for d, k in zip(self.dusts, self.kinds)]
        self.want_maps = not U.NOMAP
        self.want_solve = True
        # what stage 2 needs, checked before any GPU work (the transfer run of a large model takes minutes): a solver file per
        # stochastically heated dust -- soc_amd.a2e_pre writes them (ASOC_driver.py:196-228 calls A2E_pre.py there) -- and, with dust
        # re-emission iterations (`iterations N` with `cellpackets`), none of what the loop does not carry from one iteration to the next
        if U.ITERATIONS > 0 and U.CLPAC > 0:
            if U.WITH_ALI:
                raise UnsupportedOption("ali with dust re-emission iterations (iterations with cellpackets) inside the pipeline: the escape "
                                        "probability feeds a temperature solve, which the pipeline does not do (its emission comes from "
                                        "the per-dust solvers)")
            if int(U.WITH_REFERENCE) > 0:
                raise UnsupportedOption("reference (the reference field) with dust re-emission iterations inside the pipeline: it needs the "
                                        "previous emission and its absorptions, OEMITTED and OTABS, carried across the iterations; run "
                                        "soc_amd.asoc per iteration")
        mabu.require_solvers(self.dusts, self.kinds)
        U.NOABSORBED, U.NOMAP, U.NOSOLVE = 0, 1, 1            # rt_simple.ini: absorptions per frequency, nomap, nosolve
        # `convergence eps [kmin]` is this loop's key: the transfer run refuses it (its own temperature loop has no criterion) and gets none
        self.eps, self.kmin = float(U.CONVERGENCE), int(U.CONVERGENCE_MIN)
        U.CONVERGENCE = -1.0
        self.converged = None                                  # the step the iterations were ended at by the criterion
        self.verbose = U.VERBOSE if verbose is None else verbose
        self.timers = {}

    refuse = staticmethod(mabu.refuse)

    def log(self, *a):
        if self.verbose and self.rank == 0:
            print(*a)

    # ---- stage 2 ----------------------------------------------------------------------------------------------
    def solve_emission(self, FABSORBED, ABU, keep_resident=False, download=True, absorbed_scale=None, makelib=None):
        """FABSORBED[CELLS, NFREQ] as the absorbed file holds it (scaled, files.scale_absorbed) -> EMITTED[CELLS, NFREQ]; with
        `polarisation` lines self.R[CELLS, NFREQ] is the polarisation reduction factor.  keep_resident, download: as
        mabu.solve_emission; self.resident says whether the engine now holds this emission (then, with download=False, the arrays
        returned are not filled).  FABSORBED a ResidentAbsorptions with absorbed_scale: as mabu.solve_emission"""
        em, info = mabu.solve_emission(self.eng, self.dusts, self.kinds, FABSORBED, ABU, self.rank, self.world, log=self.log, pol=self.pol,
                                       keep_resident=keep_resident, download=download, absorbed_scale=absorbed_scale, makelib=makelib,
                                       temperatures=self.temperatures)
        self.T = info.get("T")                                 # (of this solve: after the loop, of the step whose emission is the product)
        if makelib is not None and self.rank == 0:
            mabu.write_libraries(self.dusts, info["libraries"], self.log)
        self.timers["emission_path"] = info["path"]            # 'device' (soc_mabu_*) or 'host'
        self.resident = info["resident"]
        self.on_host = download or not self.resident           # whether the array returned is filled
        self.R = info.get("R")
        if not (self.comm and self.world > 1):
            return em
        CELLS, NFREQ = FABSORBED.shape
        c0, c1 = a2e.cell_range(CELLS, self.rank, self.world)

        def whole(part):
            A = np.zeros((CELLS, NFREQ), np.float32)               # every rank solved its cells: put the array together
            A[c0:c1] = part
            for f in range(NFREQ):
                A[:, f] = self.comm.all_reduce_host(np.ascontiguousarray(A[:, f]))
            return A
        if self.R is not None:
            self.R = whole(self.R)
        return whole(em)

    # ---- dust re-emission iterations ------------------------------------------------------------------------------------
    def open_resident(self, NFREQ):
        """The emission of an iteration can stay on the device for the next one's launches (engine.emitted_*: held transposed, a
        frequency a contiguous row) where the engine has the calls, there is one rank (several: every rank solves its cells, and all
        need all), `emweight 0` (the host draws the weights from the emission) and the array fits.  Reserves it; False: the host source."""
        if self.emission_source == 'host' or not hasattr(self.eng, "emitted_begin") or self.world > 1 or self.U.USE_EMWEIGHT > 0:
            return False
        try:
            self.eng.emitted_begin(NFREQ)
        except DoesNotFit as err:
            self.log("  %s" % err)
            return False
        return True

    def open_absorbed(self, rt, N):
        """The absorptions can stay on the device from the launches that tally them to stage 2 (engine.absorbed_*: held transposed, a
        frequency's tally added to a contiguous row, scaled on their way into the rows of stage 2) where the engine has the calls, there
        is one rank, no `nnmake` thinning, no `saveint` (the intensity file wants every tally on the host), stage 2 offers its device
        path and the planes fit: one, with iterations a second for the constant sources' share.  Reserves them and returns the sink of
        the transfer stage; None, with the condition that failed logged: the host array."""
        why = "asked for (absorbed_source='host')" if self.absorbed_source == 'host' else rt.resident_absorptions_refused()
        if not why and not hasattr(self.eng, "absorbed_to_mabu"):
            why = "the engine has no absorbed_* calls"
        if not why and not mabu.device_path_offered(self.eng, self.dusts, self.kinds, rt.NFREQ, self.pol):
            why = "stage 2 does not offer its device path"
        if not why:
            try:
                self.eng.absorbed_begin(rt.NFREQ, keep_constant=N > 0)
            except DoesNotFit as err:
                why = str(err)
        if why:
            self.log("driver: the absorptions go through the host: %s" % why)
            return None
        self.scale = (files.absorbed_scale_factors(rt.cloud, self.U.GL), self.U.NNNLIMIT)
        return ResidentAbsorptions(self.eng, rt.cloud.CELLS, rt.NFREQ)

    # ---- `convergence eps [kmin]` ----------------------------------------------------------------------------------------
    def measure(self, rt, k, EMITTED, want):
        """The change of the emission of step k against step k-1 (soc_amd.converge): from the engine's resident copy where the step
        left it there and the engine has emitted_change, else from EMITTED on the host (read back where it is not there: an engine
        whose plane of luminosities does not fit).  Appends to timers["convergence"] and to convergence.dat, logs a line and returns
        (whether the criterion ends the iterations after this step, EMITTED).  With several ranks every rank holds the whole emission
        and finds the same figures; they act on rank 0's decision all the same, so that none is left alone in a collective."""
        t0 = time.time()
        c = rt.cloud
        W = np.asarray([launch.trapezoid_weight(rt.FFREQ, f) for f in range(rt.NFREQ)], np.float64)
        COEFF = np.asarray([self.U.GL * launch.PARSEC / (8.0 ** level) / launch.FACTOR for level in range(c.LEVELS)], np.float32)
        stats = None
        if want and self.resident and not self.host_every:
            try:
                stats, source = self.eng.emitted_change(W, COEFF), 'resident'
            except DoesNotFit as err:                              # (at the first call or never: the plane stays reserved)
                self.log("  %s: the figures of `convergence` come from the host array, which every iteration now reads back" % err)
                self.host_every = True
        if stats is None:
            if not self.on_host:
                EMITTED, self.on_host = self.eng.emitted_download(0, c.CELLS), True
            L, bad = converge.luminosity(EMITTED, W, c.DENS, c.OFF, c.LCELLS, COEFF)
            stats, source = converge.change(L, np.zeros_like(L) if self.Lp is None else self.Lp), 'host'
            stats["bad"], self.Lp = bad, L
        fig = converge.figures(stats)
        stop = k >= max(1, self.kmin) and 0.0 < self.eps and fig["d_l1"] < self.eps       # (step 0 primes Lp: its d_l1 is 1, no decision)
        if self.comm and self.world > 1:
            stop = bool(self.comm.all_reduce_host(np.asarray([1.0 if (stop and self.rank == 0) else 0.0]))[0] > 0.0)
        self.timers["convergence"].append(dict(k=k, bad=stats["bad"], source=source, seconds=time.time() - t0, **fig))
        if self.rank == 0:
            with open("convergence.dat", "w" if k == 0 else "a") as fp:
                fp.write("%d %.17e %.17e %.17e\n" % (k, fig["d_l1"], fig["d_total"], fig["d_max"]))
        self.log("driver: convergence step %d (%s): d_l1 %.4e  d_total %.4e  d_max %.4e%s%s"
                 % (k, source, fig["d_l1"], fig["d_total"], fig["d_max"], "  (%d cells with a negative or non-finite luminosity count as 0)"
                    % stats["bad"] if stats["bad"] else "", "  < eps %.4e: the iterations end here" % self.eps if stop else ""))
        return stop, EMITTED

    def iterate(self, rt, k, N, CONSTANT, EMITTED, ABU, want, conv=False):
        """Iteration k of N as a run of its own with `iterations 1`, `nosolve`, reading the emitted file of iteration k-1, and
        soc_amd.mabu on the absorbed file it writes: the emission of k-1 is sent from the cells at every simulated frequency, its
        absorptions join those of the constant sources, and the emission is solved from the sum.  The source of the launches is the
        engine's resident copy where stage 2 left one (want, and the stage took the device path), else EMITTED on the host.
        CONSTANT a ResidentAbsorptions: the constant sources' share is the engine's second plane (absorbed_keep), the sum is made on
        the device and stage 2 reads it there.  conv (`convergence`): no step knows that it is the last, so the emission of every
        step stays resident where it can and is read back by run() once the loop has ended (every step only with host_every)."""
        t0 = time.time()
        source = 'resident' if (want and self.resident) else 'host'
        sink = isinstance(CONSTANT, ResidentAbsorptions)
        self.log("driver: iteration %d/%d takes the emission from the %s source, the absorptions go through the %s"
                 % (k, N, source, 'device' if sink else 'host'))
        if sink:
            self.eng.absorbed_restore()
            FABSORBED = CONSTANT
        else:
            FABSORBED = CONSTANT.copy() if k < N else CONSTANT
        rt.simulate_cell_emission(EMITTED, FABSORBED, resident=source == 'resident')
        if not sink:
            files.scale_absorbed(FABSORBED, rt.cloud, self.U.GL, self.U.NNNLIMIT)
        t1 = time.time()
        # (an emission that stays on the device is read back only after the last iteration, for the products; where stage 2 does not
        # leave it there -- its host path -- the array returned is filled whatever `download` says)
        EMITTED = self.solve_emission(FABSORBED, ABU, keep_resident=want and (k < N or conv), download=self.host_every if conv else k == N,
                                      absorbed_scale=self.scale if sink else None)
        self.timers["iterations"].append(dict(transfer=t1 - t0, emission=time.time() - t1, source=source,
                                              absorbed='resident' if sink else 'host'))
        return FABSORBED, EMITTED

    # ---- the three stages -----------------------------------------------------------------------------------------
    def run_library(self, keep_files=False):
        """A library run (`libabs FILE`): returns CTABS, the absorptions at the three reference frequencies [CELLS, 3] (scaled, as the
        absorbed file holds them) and EMITTED[CELLS, NFREQ] -- with `libmaps FILE2` [CELLS, the frequencies of FILE2 in table order]"""
        U = self.U
        t0 = time.time()
        rt = AbsorptionRun(U, self.eng, self.comm, verbose=self.verbose)
        rt.write_packet_info()
        rt.setup_engine()
        self.log("driver: library run: the absorptions at the reference frequencies go to stage 2 as a host array, 12 bytes per cell "
                 "(the resident absorptions are not used: %s)" % (rt.resident_absorptions_refused() or "they hold every frequency"))
        self.timers["absorbed_source"] = 'host'
        CTABS, ABS3 = rt.simulate_constant_sources()
        cols = [f for f, _ in sorted(rt.lib_col.items(), key=lambda fk: fk[1])]
        if len(cols) != 3 or ABS3.shape[1] != 3:
            raise ValueError("libabs: the library method needs three reference frequencies of the dust file's table, the file selects %d" % len(cols))
        files.scale_absorbed(ABS3, rt.cloud, U.GL, U.NNNLIMIT)
        self.timers["transfer"] = time.time() - t0
        t0 = time.time()
        CELLS = rt.cloud.CELLS
        ABU = mabu.abundance_table(rt.ABU, U.SINGLE_ABU, CELLS, len(self.dusts))
        libs = mabu.read_libraries(self.dusts, rt.NFREQ)
        ocol = lib_col = None
        if self.fmaps is not None:                                 # the table frequencies within 0.1 % of one of `libmaps`, in table order
            hit = [f for f in range(rt.NFREQ) if np.min(np.abs((float(rt.FFREQ[f]) - self.fmaps) / float(rt.FFREQ[f]))) <= 0.001]
            if len(hit) < 1 or len(hit) > len(self.fmaps):
                raise ValueError("libmaps lists %d frequencies, %d of the dust file's lie within 0.1 %% of one" % (len(self.fmaps), len(hit)))
            ocol, lib_col = np.asarray(hit, np.int32), {f: k for k, f in enumerate(hit)}
        EMITTED, info = mabu.solve_emission_library(self.eng, self.dusts, self.kinds, ABS3, ABU, libs, cols, ocol, log=self.log)
        self.timers["emission_path"], self.timers["missed"] = info["path"], info["missed"]
        self.timers["emission"] = time.time() - t0
        self.timers["iterations"] = []
        if self.rank == 0:
            if self.verbose:
                mabu.print_misses(self.dusts, info, CELLS, False)
            if len(U.file_emitted) > 0:
                files.write_emitted(U.file_emitted, EMITTED)
            if keep_files and len(U.file_absorbed) > 0:
                files.write_absorbed(U.file_absorbed, ABS3)
        t0 = time.time()
        if self.want_maps:
            U.NOMAP = 0
            if lib_col is not None:                                # what a run of soc_amd.asoc with `libmaps` sets up (ASOC.py:124-129)
                U.LIB_ABS, U.LIB_MAPS, U.FSELECT, rt.lib_col = False, True, self.fmaps, lib_col
                U.ITERATIONS, U.NOSOLVE, U.FAST_MAP = 0, 1, 0
                U.MAP_FREQ = [1.0e-10, 1.0e30]
            else:
                U.LIB_ABS = False                                  # (all frequencies: an emission array like any other)
            rt.write_maps(EMITTED)
        self.timers["maps"] = time.time() - t0
        self.log("@@ driver: library run: transfer %.2f s, emission %.2f s (%s path), maps %.2f s"
                 % (self.timers["transfer"], self.timers["emission"], info["path"], self.timers["maps"]))
        return CTABS, ABS3, EMITTED

    def run(self, keep_files=False, want_absorbed=True):
        """Returns CTABS, FABSORBED (scaled, as the absorbed file holds it) and EMITTED.  want_absorbed=False: where the absorptions
        stayed on the device they are not read back, and FABSORBED is None (keep_files reads them back for the file)"""
        if self.library:
            return self.run_library(keep_files)
        U = self.U
        t0 = time.time()
        rt = AbsorptionRun(U, self.eng, self.comm, verbose=self.verbose)
        rt.write_packet_info()
        rt.setup_engine()
        N = U.ITERATIONS if rt.CLPAC > 0 else 0                   # dust re-emission iterations
        if N > 0:
            rt.require_emission_at_every_frequency()               # (`remit` cutting frequencies, before minutes of transfer)
        sink = self.open_absorbed(rt, N)
        self.timers["absorbed_source"] = 'resident' if sink else 'host'
        want = False
        try:
            CTABS, FABSORBED = rt.simulate_constant_sources(absorbed=sink)
            if sink:
                CONSTANT = sink                                    # (the second plane keeps the constant sources' share)
                if N > 0:
                    self.eng.absorbed_keep()
            else:
                CONSTANT = FABSORBED.copy() if N > 0 else None     # the constant sources' absorptions, unscaled: every iteration adds to them
                files.scale_absorbed(FABSORBED, rt.cloud, U.GL, U.NNNLIMIT)
            self.timers["transfer"] = time.time() - t0
            # abundances: the columns of the transfer run (ASOC_aux.py read_abundances), ones where no file is given
            CELLS = rt.cloud.CELLS
            ABU = mabu.abundance_table(rt.ABU, U.SINGLE_ABU, CELLS, len(self.dusts))
            t0 = time.time()
            want = N > 0 and self.open_resident(rt.NFREQ)
            conv = N > 0 and self.eps >= 0.0                       # `convergence`: the figures after every step, k = 0 .. N
            # ... which come from the resident emission; the host array is filled at every step only where something needs it there
            self.host_every, self.Lp = False, None
            if conv and want and not hasattr(self.eng, "emitted_change"):
                self.host_every = True
                self.log("driver: the engine has no emitted_change: with `convergence` every iteration reads its emission back")
            elif conv and want and self.pol is not None:
                self.host_every = True
                self.log("driver: `polarisation` lines with `convergence`: every iteration reads its emission and R back (any step may be the last)")
            makelib = None
            if self.makelib is not None:                           # (lfreq file, N) -> (the reference columns, N); N == 0 here
                makelib = (library.reference_columns(np.asarray(rt.FFREQ, np.float64), library.load_frequencies(self.makelib[0])), int(self.makelib[1]))
            EMITTED = self.solve_emission(FABSORBED, ABU, keep_resident=want, download=N == 0 or self.host_every,
                                          absorbed_scale=self.scale if sink else None, makelib=makelib)
            self.timers["emission"] = time.time() - t0
            self.timers["iterations"] = []
            stop = False
            if conv:
                self.timers["convergence"] = []
                stop, EMITTED = self.measure(rt, 0, EMITTED, want)
            for k in range(1, N + 1):
                FABSORBED, EMITTED = self.iterate(rt, k, N, CONSTANT, EMITTED, ABU, want, conv)
                if conv:
                    stop, EMITTED = self.measure(rt, k, EMITTED, want)
                    if stop:
                        self.converged = k
                        break
            if conv and not stop and self.eps > 0.0:
                self.log("driver: convergence: %d iterations done and d_l1 = %.4e is not below eps = %.4e"
                         % (N, self.timers["convergence"][-1]["d_l1"], self.eps))
            if not self.on_host:                                   # (`convergence` on the resident source: read back once, now)
                EMITTED = self.eng.emitted_download(0, CELLS)
            if sink:                                               # read back once, scaled, and only where somebody wants them
                FABSORBED = None
                if want_absorbed or (keep_files and len(U.file_absorbed) > 0):
                    FABSORBED = self.eng.absorbed_download(0, CELLS, *self.scale)
        finally:
            if want:
                self.eng.emitted_end()
            if sink:
                self.eng.absorbed_end()
        if self.rank == 0:
            if len(U.file_emitted) > 0:
                files.write_emitted(U.file_emitted, EMITTED)
            if keep_files and len(U.file_absorbed) > 0 and FABSORBED is not None:
                files.write_absorbed(U.file_absorbed, FABSORBED)
            if keep_files and self.R is not None and len(U.file_emitted) > 0:
                mabu.write_reduction(U.file_emitted + '.R', self.R)
            if self.T is not None:
                mabu.write_temperatures(self.dusts, self.kinds, self.T, self.log)
        t0 = time.time()
        if self.want_maps:
            U.NOMAP = 0
            rt.write_maps(EMITTED)
        if U.POLMAP:                                               # also under `nomap` (ASOC.py:3655)
            if self.R is not None and len(getattr(U, "file_polred", "")) > 0:
                self.log("driver: polmap takes the polarisation reduction factor from the `polred` file %s, not from the `polarisation` lines" % U.file_polred)
            rt.write_polmaps(EMITTED, R=self.R)
            if self.R is not None:                                 # (all-sky polarisation maps are a product of this path with R only)
                rt.write_healpix_polmaps(EMITTED, R=self.R)
        self.timers["maps"] = time.time() - t0
        self.log("@@ driver: transfer %.2f s, emission %.2f s, maps %.2f s" % (self.timers["transfer"], self.timers["emission"], self.timers["maps"])
                 + "".join(";  iteration %d (%s): transfer %.2f s, emission %.2f s" % (k + 1, it["source"], it["transfer"], it["emission"])
                           for k, it in enumerate(self.timers["iterations"])))
        return CTABS, FABSORBED, EMITTED


def main(argv=None):
    argv = sys.argv if argv is None else argv
    args, opts = mabu.parse_options(argv, ("makelib", "bins"))
    if args is None or len(args) < 2:
        print("Usage:  python -m soc_amd.driver soc.ini [--keep-files] [--makelib LFREQ [--bins N]] [--temperatures]")
        return 1
    try:
        makelib = mabu.makelib_option(opts)
    except ValueError as err:
        print(err)
        return 1
    from .dist import Comm
    comm = Comm()                      # (imports torch first when there are several ranks: see lib.load_library)
    from .lib import Engine
    eng = Engine(comm.local_rank)
    try:
        keep = "--keep-files" in args
        Pipeline(args[1], eng, comm, makelib=makelib, temperatures="--temperatures" in args).run(keep_files=keep, want_absorbed=keep)
    except UnsupportedOption as err:
        if "--temperatures" not in args:
            raise
        print(err)
        return 1
    finally:
        eng.close()
        comm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
