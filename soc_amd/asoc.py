#!/usr/bin/env python3
"""asoc -- the absorption run of SOC on MI355X:  python -m soc_amd.asoc my.ini

Drop-in for the photon-packet part of ``ASOC.py <ini>`` (reference ASOC.py:77-1560): reads
the same ini file and the same cloud / dust / dsc / background / point-source / diffuse
files, simulates the constant radiation sources frequency by frequency on the HIP engine
and writes the same products of that stage: ``packet.info``, the ``absorbed`` file
(unless ``noabsorbed``) and the ``csave`` file of frequency-integrated absorptions.
Temperature solve, emission and maps are downstream of the tallies and
not part of this engine; with ``noabsorbed`` the integrated absorptions are written to
``<prefix>.ctabs`` so a downstream solver can pick them up.

The host loop is the reference's (source block II -> frequency IFREQ, ASOC.py:1028-1545);
what runs inside is new: geometry and feature switches are run-time arguments of one
ahead-of-time compiled library (no per-run kernel build), and with several ranks each
launch is split by logical work-item id with one all-reduce of the tallies
(soc_amd/dist.py).
"""
import functools
import sys
import time

import numpy as np

from . import files, launch
from .ini import User
from .launch import PARSEC
from .maps import MapProducts


class UnsupportedOption(RuntimeError):
    pass


def _check_supported(USER, NDUST, WITH_MSF, engine=None):
    bad = []
    if USER.DO_SPLIT:
        # packet splitting of the background (SimBgSplit, kernel_ASOC.c:2117-2851; with a Healpix sky SimHpSplit, :2871-3550) on an
        # engine that has the kernel
        if not hasattr(engine, "sim_bg_split"):
            bad.append("split (the engine has no sim_bg_split)")
        if len(USER.file_hpbg) > 2 and USER.BGPAC > 0 and not hasattr(engine, "sim_hp_split"):
            bad.append("split with a Healpix background (SimHpSplit, kernel_ASOC.c:2871 on, has split rules of its own): this engine has no sim_hp_split")
        if launch.mirror_mask(USER.MIRROR):
            bad.append("split with mirror (SimBgSplit and SimHpSplit have no Mirror() call)")
        if int(USER.STEP_WEIGHT[2]) > 0:
            bad.append("split with stepweight (SimBgSplit and SimHpSplit draw unweighted free paths only)")
        if USER.WITH_ROI_SAVE:
            bad.append("split with roisave (SimBgSplit and SimHpSplit keep no region-of-interest record)")
        if USER.MAX_SPLIT != 0 and USER.MAX_SPLIT < 14:
            bad.append("maxsplit %d (at least 14: a split adds 4 entries above the kernel's NBUF > MAX_SPLIT-10 test)" % USER.MAX_SPLIT)
    if int(USER.STEP_WEIGHT[2]) > 2:
        bad.append("stepweight with a third argument > 2 (the kernel then uses an uninitialised free path, kernel_ASOC.c:516-535)")
    if USER.DIR_WEIGHT[0] > 0:
        bad.append("direweight (-D DIR_WEIGHT > 0 does not compile in the reference: pweight, pind undeclared, kernel_ASOC.c:770-775)")
    if USER.PS_METHOD == 3:
        bad.append("psmethod 3 (does not compile in the reference either)")
    if USER.WITH_REFERENCE and USER.SAVE_INTENSITY > 0:
        bad.append("saveint with the reference field (ASOC.py:994 asserts against it: the tallies hold differences)")
    if 'SUBITERATIONS' in USER.KEYS:
        bad.append("SUBITERATIONS (sub-iterations of the reference field, ASOC.py:2261-2720; there the branch starts from "
                   "`TOLD = 0.0*TNEW` with TNEW = None unless `loadtemp` is given, ASOC.py:700, :2282)")
    # keys the parser knows (soc_amd/ini.py keeps the reference's keyword set) whose effect is not built: refused, so that
    # an ini file using them stops here instead of finishing with products missing or different
    if 'nnmake' in USER.KEYS and USER.ABSTHIN > 1 and USER.MMAP_ABSORBED > 0:
        bad.append("nnmake with absthin and mmapabs (the reference adds thinned rows to a full-size memory map there and stops, ASOC.py:623-630, :1496)")
    if 'nnmake' in USER.KEYS and USER.ABSTHIN > 1 and USER.WITH_REFERENCE and not USER.NOABSORBED:
        bad.append("nnmake with absthin and the reference field (not built)")
    # polarisation maps (ASOC.py:3651-3801): PolMapping with -D POLSTAT 0, 1, 3 on an engine that has the kernel
    if USER.POLSIM:
        bad.append("polsim (polarised scattered light, kernel_ASOC_pol.c)")
    if USER.POLMAP:
        if not (hasattr(engine, "polmap") and hasattr(engine, "set_bfield")):
            bad.append("polmap / polred / magnetic-field files (polarisation maps): this engine has no polarisation-map kernel (polmap, set_bfield)")
        if USER.POLSTAT == 2:
            bad.append("polstat 2 (perspective polarisation images with cube replication, kernel_ASOC_map.c:1397-1590)")
        elif USER.POLSTAT in (4, 5):
            bad.append("polstat %d (the 2025 variants of PolMapping, kernel_ASOC_map.c:1698 on)" % USER.POLSTAT)
        elif USER.POLSTAT not in (0, 1, 3):
            bad.append("polstat %d (PolMapping knows 0..5)" % USER.POLSTAT)
        if USER.NPIX[1] < 0:                                  # ASOC.py:3808-3958 -> PolHealpixMapping, kernel_ASOC_map_H.c
            if not hasattr(engine, "polmap_healpix"):
                bad.append("polmap with a Healpix map (mapping with a negative second argument: PolHealpixMapping, kernel_ASOC_map_H.c): "
                           "this engine has no polmap_healpix")
            if USER.POLSTAT in (1, 3):
                bad.append("polstat %d with a Healpix map (kernel_ASOC_map_H.c does not compile with -D POLSTAT > 0: a ';' is missing at :928 "
                           "and Y_SHEAR is no argument of that kernel)" % USER.POLSTAT)
            if int(USER.INTERPOLATE) not in (0, 1, 2, 3):
                bad.append("interpolate %s with a Healpix polarisation map (kernel_ASOC_map_H.c:646-733 knows 0..3)" % USER.INTERPOLATE)
            if USER.Y_SHEAR != 0.0 and not (float("%.3e" % USER.MAXLOS) < 1.0e9):
                bad.append("yshear with a Healpix polarisation map and no finite maxlos (polmap bx by bz maxlos: without it a ray near "
                           "the equator wraps ~NZ/1e-5 root cells)")
        if any(k.startswith('libmap') for k in USER.KEYS):
            bad.append("polmap together with libmaps (ASOC.py:3666-3667 stops there as well)")
    elif len(getattr(USER, "file_polred", "")) > 0:
        bad.append("polred without polmap (the factor is encoded in the magnetic field of a polarisation map)")
    # `mapping nx ny dx NF`, 2 <= NF <= 998 (ASOC.py:3442-3568: NF frequencies per kernel call): the maps of the plain path, NF
    # frequencies per walk, on an engine that has the kernel (write_maps, _map_blocks)
    # `mapping nx ny dx 999` (a fourth argument >= 999; ASOC.py:2903, :3323-3438): one image per hierarchy level from the Mapping of
    # kernel_ASOC_map_H.c, on an engine that has the kernel (write_level_maps)
    if USER.FAST_MAP >= 999:
        if not hasattr(engine, "map_levels"):
            bad.append("mapping with a fourth argument >= 999 (one map per hierarchy level, kernel_ASOC_map_H.c): this engine has no "
                       "per-level map kernel (map_levels)")
        if USER.NPIX[1] < 0:
            bad.append("mapping with a fourth argument >= 999 and a Healpix map (negative second argument): the HealpixMapping of "
                       "kernel_ASOC_map_H.c writes one map into a buffer sized for LEVELS and does not separate the levels")
        if len(getattr(USER, "savetau_freq", [])) > 0 or len(getattr(USER, "file_savetau", "")) > 0:
            bad.append("savetau with a fourth mapping argument >= 999 (ASOC.py:3337 hands pyopencl np.float, and the kernel writes COLDEN "
                       "only under WITH_COLDEN, which ASOC.py never defines: the file would hold an uninitialised buffer)")
        if any(k.startswith('libmap') for k in USER.KEYS):
            bad.append("libmaps with a fourth mapping argument >= 999 (ASOC.py:3325-3326 stops there as well)")
    elif USER.FAST_MAP >= 2 and not (hasattr(engine, "map_block") and hasattr(engine, "set_map_block")):
        bad.append("mapping with a fourth argument >= 2 (FAST_MAP 2..998: kernel_ASOC_map_X.c, all frequencies per launch -- the reference's "
                   "own branch stops at ASOC.py:3553, a list compared with a float): this engine has no batch map kernel (map_block, set_map_block)")
    # `maplevels 1` (not a key of the reference): the plain map split by hierarchy level, from the walk of the plain map
    # (write_maps, write_healpix_maps -> map_block_levels)
    if getattr(USER, "MAP_LEVELS", 0) > 0:
        if not (hasattr(engine, "map_block_levels") and hasattr(engine, "map_block") and hasattr(engine, "set_map_block")):
            bad.append("maplevels (the plain map split by hierarchy level): this engine has no kernel for it (map_block_levels, with "
                       "set_map_block and map_block)")
        if USER.FAST_MAP >= 999:
            bad.append("maplevels together with mapping with a fourth argument >= 999 (two different per-level products: that mode "
                       "never reaches the walk of the plain map, whose levels maplevels writes)")
    # the library method (ASOC.py:116-130): `libabs` simulates the frequencies of its file only, `libmaps` maps them from an emitted
    # file that holds only them
    if USER.LIB_ABS:
        if USER.LIB_MAPS:
            bad.append("libabs together with libmaps (one run either simulates the reference frequencies or maps the library's emission: "
                       "both keys fill the same list of frequencies, ASOC.py:116-117)")
        if USER.SAVE_INTENSITY > 0:
            bad.append("libabs with saveint (the intensity file holds all frequencies, the run simulates a few: ASOC.py:2852 stops there as well)")
        if USER.ITERATIONS > 0 and USER.CLPAC > 0:
            bad.append("libabs with iterations > 0 and cellpackets (the dust emission cannot be solved from the reference frequencies "
                       "alone; ASOC.py:2364 calls the combination senseless)")
        if USER.ABSTHIN > 1 or 'nnmake' in USER.KEYS:
            bad.append("libabs with absthin or nnmake (the thinned absorptions train a network on all frequencies; the library needs "
                       "the reference frequencies of every cell)")
    if USER.LIB_MAPS and getattr(USER, "MAP_LEVELS", 0) > 0:
        bad.append("libmaps with maplevels (the per-level maps go through the batch path, libmaps through the plain one: ASOC.py:127 "
                   "sets FAST_MAP = 0)")
    # `convergence eps [kmin]` (not a key of the reference) is the criterion of soc_amd.driver's loop, which takes it off the ini it hands
    # to its transfer run; this program's own iterations solve temperatures and have none
    if getattr(USER, "CONVERGENCE", -1.0) >= 0.0 and USER.ITERATIONS > 0 and USER.CLPAC > 0:
        bad.append("convergence with iterations > 0 and cellpackets in this program (its temperature loop has no convergence criterion: "
                   "the key ends the dust re-emission iterations of soc_amd.driver)")
    if USER.MAP_INTERPOLATION > 2 or USER.MAP_INTERPOLATION < 0:
        bad.append("mapint other than 0, 1, 2 (kernel_ASOC_map.c:656-810 knows those: a larger value leaves Adens, Aemit ... unset there)")
    if len(USER.kernel_defs.strip()) > 0:
        bad.append("DEFS (extra -D options for the OpenCL compiler)")
    # `interpolate` and `yshear` have an effect in one branch only, the Healpix polarisation map (write_healpix_polmaps);
    # elsewhere they are accepted without effect, because they have none in the reference either (kernel_ASOC_map_H.c is
    # otherwise built for FAST_MAP >= 999 only, and its Mapping tests neither).  Likewise without effect: `externalmask` reaches only the SUBITERATIONS
    # branch (refused above), `sourcemap` is parsed and never read (ASOC_aux.py:322), `bgmethod` is a -D that no kernel tests
    # (`loadtemp` with iterations > 0 has no effect in the reference: the temperatures read are replaced before any use --
    # the block that would use them with ALI, ASOC.py:2062-2071, is switched off there -- so it has none here)
    if bad:
        raise UnsupportedOption("ini options not supported by this engine: " + ", ".join(bad))


def _local_routing(abu=True):
    """Decorator of a transfer stage of AbsorptionRun: with an abundance file the engine's `abu_local` routing is on while it runs (see
    AbsorptionRun.ABU_LOCAL), on a hierarchy whose Index() runs in float its `float_local` routing (AbsorptionRun.FLOAT_LOCAL), and the
    engine has its built-in routing back afterwards, in reverse order.  A run with neither issues no tuning call.  abu=False: the
    `float_local` half alone, for the scattered-light driver (soc_amd.asocs), whose launches with per-cell opacities have no sweep to go to."""
    def wrap(method):
        @functools.wraps(method)
        def stage(self, *a, **kw):
            keys = []
            if abu and self.WITH_ABU and self.ABU_LOCAL:
                keys.append("abu_local")
            if self.FLOAT_LOCAL and float_index(self.cloud):
                keys.append("float_local")
            for k in keys:
                self._tune(**{k: 1})
            try:
                return method(self, *a, **kw)
            finally:
                for k in reversed(keys):
                    self._tune(**{k: 0})
        return stage
    return wrap


def float_index(cloud):
    """a hierarchy on which the reference evaluates Index() with float3 POS (kernel_ASOC_aux.c:25-37): NX <= 399 with two levels,
    NX <= 100 with three or more"""
    return cloud.LEVELS > 1 and cloud.NX <= (399 if cloud.LEVELS < 3 else 100)


class ResidentAbsorptions:
    """The engine's resident absorptions (Engine.absorbed_begin) as the sink of a transfer stage, in place of the host array
    FABSORBED[CELLS, NFREQ]: where a stage does FABSORBED[:, col] += tally on the host, it adds the same buffer to row `col` on the device."""

    def __init__(self, engine, CELLS, NFREQ):
        self.eng = engine
        self.shape = (int(CELLS), int(NFREQ))

    def add_tally(self, col):
        self.eng.absorbed_add_tally(col)

    def add_slot(self, col, slot):
        self.eng.absorbed_add_slot(col, slot)


class AbsorptionRun(MapProducts):
    """The constant-source part of an ASOC run.  ``engine`` is a soc_amd.lib.Engine (or an
    object with the same methods); ``comm`` a soc_amd.dist.Comm."""
    _hpbg_launch = staticmethod(launch.hpbg_launch)           # the Healpix background's launch shape, see _constant_launch

    def __init__(self, USER, engine, comm=None, verbose=None, workdir=".", shard="items"):
        """shard (several ranks): "items" -- every launch is split by work-item ranges (identical packets and events per rank, one
        all-reduce of the per-cell buffer per frequency when absorptions are saved); "launches" -- the launches themselves are
        dealt out: a run that keeps the per-frequency absorptions gives every frequency to ONE rank, which owns that column of
        the absorbed file (no collective for INT at all; TABS is reduced once); a TABS-only run gives every rank a contiguous
        share of the launch sequence (launch.shard_launches).  Same packets and streams either way."""
        self.U = USER
        self.eng = engine
        self.comm = comm
        if shard not in ("items", "launches"):
            raise ValueError("shard: 'items' or 'launches'")
        self.shard = shard
        self.rank = comm.rank if comm else 0
        self.world = comm.world if comm else 1
        self.verbose = USER.VERBOSE if verbose is None else verbose
        self.timers = dict(Tkernel=0.0, Tpush=0.0, Tpull=0.0)
        self.packets = 0
        self.freq_owner = None                 # {IFREQ: rank} where shard == "launches" gives frequencies to ranks (_plan)
        self._load_inputs()

    def log(self, *a):
        if self.verbose and self.rank == 0:
            print(*a)

    # ---------------------------------------------------------------------------------
    def _load_inputs(self):
        U = self.U
        if not U.Validate():
            raise ValueError("check the ini file: no cloud defined")
        if U.GL <= 0.0:
            raise ValueError("gridlength must be given")
        self.FFREQ, self.AFG, self.AFABS, self.AFSCA = files.read_dust(U.file_optical, U.GL)
        self.NFREQ = U.NFREQ = len(self.FFREQ)
        self.NDUST = len(self.AFABS)
        if self.NFREQ < 2:
            raise ValueError("the dust file needs >= 2 frequencies (trapezoid weights, ASOC.py:1220); "
                             "restrict the simulated range with `simum` instead")
        self.FDSC, self.FCSC = files.read_scattering_functions(U.file_scafunc, self.NFREQ, U.DSC_BINS)
        self.WITH_MSF = WITH_MSF = len(self.FDSC) > 1
        _check_supported(U, self.NDUST, WITH_MSF, self.eng)
        # the library method: {IFREQ: column} of the frequencies within 0.1 % of one of `libabs file` / `libmaps file`, counted in table
        # order (OIFREQ of ASOC.py:1126-1140 -- before the `simum` test -- and :3032-3046); None without either key
        self.lib_col = None
        if U.LIB_ABS or U.LIB_MAPS:
            if U.FSELECT_ERROR or len(U.FSELECT) < 1:
                raise ValueError(U.FSELECT_ERROR or "the file of libabs / libmaps lists no frequency")
            fsel = np.asarray(U.FSELECT, np.float64)
            hit = [f for f in range(self.NFREQ) if np.min(np.abs((float(self.FFREQ[f]) - fsel) / float(self.FFREQ[f]))) <= 0.001]
            if len(hit) > len(fsel):
                raise ValueError("%s lists %d frequencies, %d of the dust file's lie within 0.1 %% of one" % ("libabs" if U.LIB_ABS else "libmaps", len(fsel), len(hit)))
            self.lib_col = {f: k for k, f in enumerate(hit)}
        if U.LIB_MAPS:                                             # ASOC.py:124-129 (after the check: it looks at the `mapping` of the ini file)
            U.ITERATIONS, U.NOSOLVE, U.FAST_MAP = 0, 1, 0
            U.MAP_FREQ = [1.0e-10, 1.0e30]
        self.IBG = files.read_background_intensity(U.file_background, self.NFREQ, U.scale_background) \
            if U.BGPAC > 0 else []
        self.LPS = files.read_source_luminosities(U.file_pointsource[:U.NO_PS], self.NFREQ, U.PS_SCALING) \
            if U.NO_PS > 0 else []
        self.HPBG = []
        if len(U.file_hpbg) > 2:                                   # ASOC.py:291-297, NSIDE 64 fixed
            self.HPBG = np.fromfile(U.file_hpbg, np.float32).reshape(self.NFREQ, 49152) * np.float32(U.scale_background)
        self.cloud = files.read_cloud(U.file_cloud, U.KDENSITY, U.LEVELS)
        c = self.cloud
        U.AREA, U.CELLS = float(c.AREA), c.CELLS
        self.log("NX %d, NY %d, NZ %d LEVELS %d, CELLS %d" % (c.NX, c.NY, c.NZ, c.LEVELS, c.CELLS))
        if U.POLMAP and U.NPIX[1] < 0 and int(U.INTERPOLATE) in (1, 2) and c.LEVELS > 1:      # known only now that the cloud is read
            raise UnsupportedOption("ini options not supported by this engine: interpolate %d with a Healpix polarisation map of a hierarchy "
                                    "(kernel_ASOC_map_H.c:654-707 indexes level 0 as a plain grid there and reads links as densities; 0 or 3)"
                                    % int(U.INTERPOLATE))
        self.ABU = files.read_abundances(U.file_abundance, c.CELLS)
        self.WITH_ABU = self.ABU is not None
        if self.WITH_ABU and U.SINGLE_ABU:
            if self.NDUST != 2:
                raise ValueError("singleabu assumes exactly two dust components")
            if self.WITH_MSF:
                raise ValueError("singleabu cannot be used with several scattering functions (ASOC.py:159-161)")
            self.ABU = np.ravel(self.ABU[:, 0])
        if self.WITH_MSF and not self.WITH_ABU:
            raise ValueError("cannot have multiple scattering functions without multiple dusts with variable abundances (ASOC.py:168-170)")
        if self.WITH_MSF and len(self.FDSC) != self.NDUST:
            raise ValueError("%d dsc files for %d dust species" % (len(self.FDSC), self.NDUST))
        self.DIFFUSERAD = files.mmap_diffuserad(U.file_diffuse, c.CELLS) if len(U.file_diffuse) > 0 else []

        # LOCAL only enters through the rounding of packet counts (ASOC.py:221-227)
        LOCAL = 8 if 'c' in U.DEVICES else 32
        if 'local' in U.KEYS:
            LOCAL = int(U.KEYS['local'][0])
        self.LOCAL = LOCAL
        pc = launch.packet_counts(U.BGPAC, U.PSPAC, U.CLPAC, U.DFPAC, int(U.AREA), c.CELLS, LOCAL, U.USE_EMWEIGHT)
        self.PSPAC, self.BGPAC, self.CLPAC, self.DFPAC = pc["PSPAC"], pc["BGPAC"], pc["CLPAC"], pc["DFPAC"]
        if U.ITERATIONS < 1:
            U.NOABSORBED = 1
        self.SPLIT = bool(U.DO_SPLIT) and U.BGPAC > 0 and len(self.HPBG) == 0
        # `split 1` with a Healpix sky (SimHpSplit): packet.info keeps the rounded BGPAC above, which is what the reference writes
        # for this combination (ASOC.py:251 comes before the launch loop that recomputes BGPAC, :1050-1059)
        self.HP_SPLIT = bool(U.DO_SPLIT) and U.BGPAC > 0 and len(self.HPBG) > 0
        if self.SPLIT:
            # `split 1`: BATCH rays from every surface element; the corrected BGPAC = AREA*BATCH (ASOC.py:1073-1074)
            self.BGPAC = launch.bg_split_launch(U.BGPAC, int(U.AREA), LOCAL)["PACKETS"]
        self.log('PACKETS: PSPAC %d   BGPAC %d  CLPAC %d  DFPAC %d' % (self.PSPAC, self.BGPAC, self.CLPAC, self.DFPAC))
        self.XPS = files.analyse_external_point_sources(c.NX, c.NY, c.NZ, U.PSPOS, int(U.NO_PS), int(U.PS_METHOD))
        # launch size for point-source / cell-emission launches: reference default 32768
        # (ASOC.py:86), `global` keyword overrides (more work items fill an MI355X better)
        self.GLOBAL_0 = U.GLOBAL if U.GLOBAL > 0 else launch.GLOBAL_0
        self.with_int = 2 if U.SAVE_INTENSITY == 2 else int((U.SAVE_INTENSITY == 1) or (not U.NOABSORBED))
        if U.SAVE_INTENSITY > 0 and self.WITH_ABU:
            # ASOC.py:1499-1515 divides by ABS, which the abundance branch never sets (:1146-1165 fill OPT only)
            raise UnsupportedOption("saveint with an abundance file (the reference scales the intensity by 1/ABS = 1/0 there)")
        self.INTENSITY = None

    def write_packet_info(self, path="packet.info"):
        """int32 [BGPAC, PSPAC, DFPAC, CLPAC] (ASOC.py:251).  BGPAC is the count rounded to multiples of AREA and LOCAL (ASOC.py:235),
        also for `split 1` with a Healpix sky, whose launch sends GLOBAL_SPLIT*100 rays: the reference writes the file before its
        launch loop recomputes BGPAC.  Only `split 1` with the isotropic background carries the corrected count AREA*BATCH."""
        if self.rank == 0:
            np.asarray([self.BGPAC, self.PSPAC, self.DFPAC, self.CLPAC], np.int32).tofile(path)

    # ---------------------------------------------------------------------------------
    def setup_engine(self):
        e, c, U = self.eng, self.cloud, self.U
        e.set_cloud(c)
        e.set_features(with_int=self.with_int, ps_method=U.PS_METHOD, use_emweight=min(max(U.USE_EMWEIGHT, 0), 2))
        e.set_mirror(launch.mirror_mask(U.MIRROR))
        # `stepweight a b c`: the reference hands the kernels -D SW_A=int(a) -D SW_B=b -D STEP_WEIGHT=int(c), each float
        # written with %.3e (ASOC.py:348,357) -- the drop-in passes the same values
        e.set_step_weight(int(U.STEP_WEIGHT[2]), float("%.3e" % int(U.STEP_WEIGHT[0])), float("%.3e" % U.STEP_WEIGHT[1]))
        # -D CR_HEATING=%d -D CR_HEATING_RATE=%.3ef with (USER.CR_HEATING>0), USER.CR_HEATING (ASOC.py:352,362): device solve only,
        # as in the reference (its host loop, used with ALI, has no such term)
        e.set_cr_heating(float("%.3e" % U.CR_HEATING) if U.CR_HEATING > 0 else 0.0)
        e.set_map_roi(U.ROI if U.ROI_MAP else None)                  # -D ROI_MAP (ASOC.py:345,354; :3126-3133)
        e.set_map_threshold(max(0, int(U.LEVEL_THRESHOLD)))          # -D LEVEL_THRESHOLD (ASOC.py:349,359)
        e.set_map_interpolation(int(U.MAP_INTERPOLATION))            # -D MAP_INTERPOLATION (ini key mapint; ASOC.py:352,362)
        if self.WITH_ABU:
            e.set_opt_half(bool(U.OPT_IS_HALF))                # OPT as fp16 (ASOC.py:1158-1159)
            e.set_abundances(self.ABU, single=bool(U.SINGLE_ABU))
        if self.comm:
            self.comm.attach(e, c.CELLS)

    def _tune(self, **kw):
        """Engine.set_tuning, where the engine has sweeps to shape (the oracle's stand-in has one path)"""
        tune = getattr(self.eng, "set_tuning", None)
        if tune is not None:
            tune(**kw)

    def _log_form(self, name):
        """verbosity >= 1: what the segment's last sweep ran as (Engine.last_form / last_variant)"""
        form = getattr(self.eng, "last_form", None)
        if form is None or not (self.verbose and self.rank == 0):
            return
        f = form()
        v = self.eng.last_variant() if f else None
        names = ("direct kernels", "Cartesian brick sweep", "sweep of the hierarchy in global memory", "brick-local sweep")
        print("      %s: last launches ran as form %d (%s)%s" % (name, f, names[f], ", per-cell opacities" if (v and v.get("abu")) else ""))

    def _optical_for(self, IFREQ):
        """scalar ABS,SCA summed over species, or OPT[CELLS,2] with abundances (ASOC.py:1146-1175)"""
        e = self.eng
        if self.WITH_ABU:
            # OPT = sum over species of ABU * (AFABS, AFSCA) is built on the device from the abundances uploaded
            # once (setup_engine); the reference uploads 8*CELLS bytes per frequency (ASOC.py:1146-1160,1177)
            e.set_optical_abu([a[IFREQ] for a in self.AFABS], [a[IFREQ] for a in self.AFSCA])
            ABS = np.float32(sum(a[IFREQ] for a in self.AFABS))
            SCA = np.float32(sum(a[IFREQ] for a in self.AFSCA))
        else:
            ABS, SCA = np.float32(0.0), np.float32(0.0)
            for idust in range(self.NDUST):
                ABS += self.AFABS[idust][IFREQ]
                SCA += self.AFSCA[idust][IFREQ]
            e.set_opt(None)
        e.set_optical(ABS, SCA)
        return ABS, SCA

    def _scatter_tables_for(self, IFREQ):
        """DSC, CSC of the frequency; one pair per species with WITH_MSF (ASOC.py:1234-1243)"""
        if self.WITH_MSF:
            self.eng.set_scatter_tables(self.FDSC[:, IFREQ, :], self.FCSC[:, IFREQ, :])
        else:
            self.eng.set_scatter_table(self.FDSC[0, IFREQ, :], self.FCSC[0, IFREQ, :])

    def _save_intensity(self, IFREQ, FREQ, ABS, TMP):
        """saveint 1|2: the per-frequency INT tally (already summed over ranks) becomes the mean intensity of the cells,
        INTENSITY += (h*f/ABS) * 8^level * INT / n; saveint 2 adds the vector sums INTX, INTY, INTZ the same way
        (ASOC.py:1499-1515, :1895-1908)"""
        U, c, e = self.U, self.cloud, self.eng
        comps = [TMP]
        if U.SAVE_INTENSITY == 2:
            for which in (3, 4, 5):
                v = e.read_tally(which)
                if self.comm and self.world > 1:
                    v = self.comm.all_reduce_host(v)
                comps.append(v)
        if self.rank != 0:
            return
        if self.INTENSITY is None:
            self.INTENSITY = files.create_intensity_file(U.SAVE_INTENSITY_FILE, c.CELLS, self.NFREQ, U.SAVE_INTENSITY == 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            for icomp, v in enumerate(comps):
                for level in range(c.LEVELS):
                    # float32 throughout, as numpy evaluates KDEV*(PLANCK*FREQ/ABS)*(8.0**level) with ABS a float32 array
                    coeff = np.float32(launch.PLANCK * FREQ) / np.float32(ABS) * np.float32(8.0 ** level)
                    a, b = int(c.OFF[level]), int(c.OFF[level] + c.LCELLS[level])
                    if U.SAVE_INTENSITY == 2:
                        self.INTENSITY[a:b, IFREQ, icomp] += coeff * v[a:b] / c.DENS[a:b]
                    else:
                        self.INTENSITY[a:b, IFREQ] += coeff * v[a:b] / c.DENS[a:b]

    def _constant_launch(self, II):
        """Launch shape of source block II (ASOC.py:1036-1110), or None when the block is not simulated."""
        U, c = self.U, self.cloud
        if II == 0:
            if (self.PSPAC < 1) or (U.NO_PS < 1):
                return None
            return launch.ps_launch(self.PSPAC, U.NO_PS, U.GL, self.GLOBAL_0)
        if II == 1:
            if self.BGPAC < 1:
                return None
            if self.SPLIT:
                return launch.bg_split_launch(U.BGPAC, int(U.AREA), self.LOCAL)
            if self.HP_SPLIT:
                return launch.hp_split_launch(self.BGPAC, c.NX, c.NY, c.NZ, int(U.AREA), self.LOCAL)
            return self._hpbg_launch(self.BGPAC, c.NX, c.NY, c.NZ) if len(self.HPBG) > 0 else launch.bg_launch(self.BGPAC, int(U.AREA))
        if II == 2:
            if len(self.DIFFUSERAD) < 1 or self.DFPAC < 1:
                return None
            return launch.cl_launch(self.DFPAC, c.CELLS, self.GLOBAL_0)
        if U.ROIPAC < 1 or self.ROI_LOAD is None:
            return None
        return launch.roi_launch(U.ROIPAC, files.roi_elements(self.ROI_DIM), U.ROI_NSIDE)

    def _launch_shares(self, by_frequency):
        """shard == "launches": {(II, IFREQ): (first, count)} for this rank over the sequence of launches of the constant sources.
        by_frequency: whole launches, the k-th simulated frequency to rank k % world (the rank then owns that frequency's INT)."""
        U = self.U
        seq = []
        for II in range(4):
            L = self._constant_launch(II)
            if L is None:
                continue
            for IFREQ in range(self.NFREQ):
                if not self._simulated(IFREQ):
                    continue
                seq.append((II, IFREQ, L))
        if by_frequency:
            sim = sorted({f for _, f, _ in seq})
            owner = {f: k % self.world for k, f in enumerate(sim)}
            return {(II, f): ((0, L["GLOBAL"]) if owner[f] == self.rank else (0, 0)) for II, f, L in seq}, owner
        parts = launch.shard_launches([L["GLOBAL"] for _, _, L in seq], [L["PACKETS"] for _, _, L in seq], self.rank, self.world)
        return {(II, f): pc for (II, f, _), pc in zip(seq, parts)}, None

    def _simulated(self, IFREQ):
        """the frequency is one the constant sources are simulated at: inside `simum`, and with `libabs` one of its file"""
        FREQ = float(self.FFREQ[IFREQ])
        if self.U.LIB_ABS and IFREQ not in self.lib_col:
            return False
        return self.U.SIM_F[0] <= FREQ <= self.U.SIM_F[1]

    def _abs_col(self, IFREQ):
        """the column of the absorbed file that holds IFREQ (`libabs`: only the selected frequencies have one)"""
        return self.lib_col[IFREQ] if self.U.LIB_ABS else IFREQ

    def emitted_range(self):
        """(I1, I2): the first and the last frequency inside `remit`, the columns of the emitted file (ASOC.py:199-200)"""
        m = np.nonzero((self.FFREQ >= self.U.REMIT_F[0]) & (self.FFREQ <= self.U.REMIT_F[1]))[0]
        return int(m[0]), int(m[-1])

    def _seed(self, IFREQ, rng):
        """seed of the launches at IFREQ (ASOC.py:1247); with seed <= 0 a random one, the same on every rank"""
        if self.U.SEED > 0:
            return launch.launch_seed(self.U.SEED, IFREQ, 1, 0)       # sharded launches reproduce ONE device (ASOC.py:179-181)
        seed = float(rng.random())
        if self.comm and self.world > 1:          # every rank must use the same streams
            seed = self._bcast_seed(seed)
        return seed

    def _launch(self, II, L, IFREQ, seed, first, count):
        """Issue the launch of source block II (shape L) at frequency IFREQ on the work items [first, first+count)
        (ASOC.py:1196-1461): the block's inputs of the frequency -- source weights, the diffuse emission, a loaded
        region-of-interest record, the Healpix sky -- then the sim_* call.  Returns the launch's (TW, BG, PS), or None
        where the block sends nothing at this frequency (no DIFFUSERAD column for it, an empty sky)."""
        U, e, c = self.U, self.eng, self.cloud
        t0 = time.time()
        FREQ = float(self.FFREQ[IFREQ])
        FF = np.float32(launch.trapezoid_weight(self.FFREQ, IFREQ))
        PS = (self.LPS[:, IFREQ] * np.float32(L["WPS"])) / np.float32(FREQ) if II == 0 else np.zeros(1, np.float32)
        BG = np.float32(float(self.IBG[IFREQ]) * L["WBG"] / FREQ) if (II == 1 and len(self.IBG) == self.NFREQ) else np.float32(0.0)
        if II == 2:
            dr_ind = IFREQ + (self.DIFFUSERAD.shape[1] - self.NFREQ)
            if dr_ind < 0 or dr_ind >= self.DIFFUSERAD.shape[1]:
                return None
            EMIT = np.zeros(c.CELLS, np.float32)
            for level in range(c.LEVELS):
                coeff = U.GL * PARSEC / (8.0 ** level) * U.K_DIFFUSE
                a, b = int(c.OFF[level]), int(c.OFF[level] + c.LCELLS[level])
                EMIT[a:b] = self.DIFFUSERAD[a:b, dr_ind] * coeff
            e.set_emission(EMIT, None)
        if II == 3:
            # scale in again the dependence on the grid length (ASOC.py:1419-1421)
            e.set_roi_load(self.ROI_DIM, U.ROI_NSIDE,
                           np.asarray(self.ROI_LOAD[IFREQ, :] * U.ROI_LOAD_SCALE / (U.GL * U.GL), np.float32))
        hp = (II == 1) and len(self.HPBG) > 0
        if hp:
            sky = files.hpbg_for_frequency(self.HPBG[IFREQ], L["WBG"] / FREQ, U.HPBG_WEIGHTED)
            if sky is None:
                return None                                    # empty sky (ASOC.py:1200)
            e.set_hpbg(*sky)
        self.timers["Tpush"] += time.time() - t0
        t0 = time.time()
        if II == 2:
            e.sim_cl(II, L["PACKETS"], L["BATCH"], seed, FF, L["GLOBAL"], gid_first=first, gid_count=count)
        elif hp and "GLOBAL_W" in L:                           # `split 1` with a Healpix sky: kernel_hp_split (ASOC.py:1336-1340)
            e.sim_hp_split(L["PACKETS"], L["BATCH"], seed, FF, int(U.MAX_SPLIT), GLOBAL=L["GLOBAL"], gid_first=first, gid_count=count)
        elif hp:
            e.sim_hp(L["PACKETS"], L["BATCH"], seed, FF, L["GLOBAL"], gid_first=first, gid_count=count)
        elif II == 1 and "SELEM" in L:                         # `split 1`: kernel_bg_split (ASOC.py:1343-1347)
            e.sim_bg_split(L["PACKETS"], L["BATCH"], seed, BG, FF, L["SELEM"], int(U.MAX_SPLIT), GLOBAL=L["GLOBAL"], gid_first=first, gid_count=count)
        else:
            e.sim_pb(II, L["PACKETS"], L["BATCH"], seed, BG, FF, PSPOS=U.PSPOS[:max(U.NO_PS, 1), :3], PS=PS, XPS=self.XPS,
                     GLOBAL=L["GLOBAL"], gid_first=first, gid_count=count)
        self.timers["Tkernel"] += time.time() - t0
        self.packets += L["PACKETS"]
        return FF, BG, PS

    # The batch policies of the constant-source launches (_plan).
    ONE_BATCH, FREQ_GROUPS, LAUNCH_GROUPS, SEQUENTIAL = "one batch", "INT groups per frequency", "INT groups per launch", "sequential"

    # Frequencies of an absorbed-file run on a hierarchy that share a sweep (an INT tally and, for cell emission, a copy of the emission each).
    # Measured on config 3 (bench.py --workload C3INT --int-groups 4): 2.00e8 packets/s against 2.09e8 with one frequency per sweep -- the
    # brick queues are per frequency (a workgroup's LDS tallies belong to one INT array), so more frequencies mean more queues of the same
    # length, not longer ones; the default stays 1.
    FREQS_PER_SWEEP = 1

    # Runs with an abundance file (per-cell opacities): the engine's tuning key `abu_local`, which takes their launches to the brick-local
    # walk of a hierarchy that has one (the opacities of a brick's cells in LDS) instead of the sweep that reads the hierarchy and OPT
    # from global memory.  Measured on config 3 with two species of variable abundance, 9 launches in one sweep (tools/exp_abu.py,
    # profiles/abu_local_lines.json): 9.67e9 cell steps/s against 6.58e9, 1.47x with a spread of 0.14 % over the repeats, equal event
    # counts -- so the key is on.  with_int 2 and ALI are not part of that walk; the engine routes them as before either way.
    ABU_LOCAL = True

    # Hierarchies whose Index() the reference evaluates in float (NX <= 100, or <= 399 with two levels): the engine's tuning key
    # `float_local`, which takes their launches to the brick-local walk in its float form (soc_ltree.h) instead of the sweep that reads
    # the hierarchy from global memory -- and mirror, `saveint 2`, ROI records and ALI launches to a sweep at all.  The rule for this
    # switch: on only if tools/exp_float_local.py (profiles/float_local_lines.json) shows the float form faster on both of its geometries
    # by more than the spread of the repeats.  Measured, 9 launches in one batch, equal event counts: octree_cloud(64, levels=4) 1.65e10
    # cell steps/s against 1.02e10 (1.61x), octree_cloud(256, levels=2) 5.71e10 against 1.74e10 (3.28x), spread 0.7 % -- so the key is on.
    # (The float form runs the nine launches as one sweep, the older path as one sweep per kind of launch: part of the ratio, not
    # measured apart.  What the key also reroutes in automatic mode -- batched scattered-light launches to the sweep of rays, lone
    # launches of 1e6 work items and more, launches with mirror, saveint 2, ROI records or ALI to form 3 -- is tested for results but was
    # NOT measured against the direct kernels it replaces.)
    FLOAT_LOCAL = True

    def _sends(self, II, IFREQ):
        """False where _launch sends nothing: no DIFFUSERAD column for the frequency, an empty Healpix sky (files.hpbg_for_frequency)"""
        if II == 2:
            return 0 <= IFREQ + self.DIFFUSERAD.shape[1] - self.NFREQ < self.DIFFUSERAD.shape[1]
        if II == 1 and len(self.HPBG) > 0 and self.U.HPBG_WEIGHTED:
            return bool(np.max(np.asarray(self.HPBG[IFREQ], np.float64)) >= 1.0e-40)
        return True

    def _plan(self, absorbed, thin):
        """The launches of the constant sources on this rank and how they are batched, decided before any engine call.
        Returns (segments, owner).  segments: [(policy, name, steps)]; TABS is zeroed before a segment and read after it (name:
        its source block or "all source blocks").  steps: [(IFREQ, launches, summed)] in issue order, the launches
        [(II, L, first, count)] that share the frequency's optical data, scatter tables and seed; count is this rank's work
        items (0: another rank's launch).  summed: the step's tallies are summed over the ranks, so every rank enters its
        collectives, also a rank with no work items in it -- derived from rank-independent data only.  owner: {IFREQ: rank}
        where shard == "launches" gives every frequency to one rank (no collective for INT then), else None.
        The policies:
          ONE_BATCH      TABS-only runs: all launches one batch (soc_batch_begin); on brick-local hierarchies the point-source,
                         background and diffuse launches of all frequencies share brick sweeps (up to 128 launches per sweep),
                         elsewhere the engine starts a new sweep where the kind changes.  TABS is read once.
          FREQ_GROUPS    absorbed file on a hierarchy: frequency outside, the launches of one frequency an INT group
                         (soc_batch_begin_int_groups / soc_batch_next_int), FREQS_PER_SWEEP groups per batch, so that the
                         blocks of a frequency share brick sweeps and brick queues.  TABS is read once.
          LAUNCH_GROUPS  absorbed file on a Cartesian grid: block outside, every launch an INT group, 16 per batch.
          SEQUENTIAL     the rest (intensity file, region-of-interest records, a Healpix sky on a hierarchy): INT, the
                         intensity and the ROI record read after every launch."""
        U, c = self.U, self.cloud
        if U.ITERATIONS < 1:
            return [], None
        blocks = [(II, self._constant_launch(II)) for II in range(4)]
        blocks = [(II, L) for II, L in blocks if L is not None]
        freqs = [f for f in range(self.NFREQ) if self._simulated(f)]
        # shard == "launches" (see __init__): runs that keep the per-frequency absorptions give a frequency to one rank (not with the
        # intensity file, region-of-interest records or emission iterations, which need every frequency on every rank -- those keep
        # the work-item split); TABS-only runs deal out the launch sequence
        shares, owner = None, None
        if self.shard == "launches" and self.world > 1:
            own_freq = self.with_int
            if (not own_freq) or (absorbed and U.SAVE_INTENSITY == 0 and (not U.WITH_ROI_SAVE) and self.CLPAC < 1 and thin == 1):
                shares, owner = self._launch_shares(by_frequency=own_freq)
        summed = self.world > 1 and owner is None and bool(self.with_int or U.WITH_ROI_SAVE)

        def step(IFREQ, blocks):
            launches = [(II, L) + (shares.get((II, IFREQ), (0, 0)) if shares else launch.shard_range(L["GLOBAL"], self.rank, self.world))
                        for II, L in blocks]
            return IFREQ, launches, summed and any(self._sends(II, IFREQ) for II, _ in blocks)
        if absorbed and c.LEVELS > 1 and U.SAVE_INTENSITY == 0 and not U.WITH_ROI_SAVE and not U.WITH_ROI_LOAD and len(self.HPBG) == 0:
            return [(self.FREQ_GROUPS, "all source blocks", [step(f, blocks) for f in freqs])], owner
        if not self.with_int and not U.WITH_ROI_SAVE:
            return [(self.ONE_BATCH, "all source blocks", [step(f, [b]) for b in blocks for f in freqs])], owner
        return [(self.LAUNCH_GROUPS if (absorbed and c.LEVELS == 1 and U.SAVE_INTENSITY == 0 and not U.WITH_ROI_SAVE and II != 3)
                 else self.SEQUENTIAL, ['PS', 'BG', 'DE', 'ROI'][II], [step(f, [(II, L)]) for f in freqs]) for II, L in blocks], owner

    def resident_absorptions_refused(self):
        """why this run cannot tally into the engine's resident absorptions (None: it can): they hold every cell at every frequency
        of one rank, and the intensity file wants each tally on the host anyway"""
        U = self.U
        if not all(hasattr(self.eng, m) for m in ("absorbed_begin", "absorbed_add_tally", "absorbed_add_slot")):
            return "the engine has no absorbed_* calls"
        if self.world > 1:
            return "several ranks"
        if U.NOABSORBED or U.LIB_ABS:
            return "noabsorbed or libabs"
        if 'nnmake' in U.KEYS:
            return "nnmake (absthin thinning)"
        if U.SAVE_INTENSITY > 0:
            return "saveint"
        return None

    @_local_routing()
    def simulate_constant_sources(self, absorbed=None):
        """for II in (point sources, background, diffuse): for IFREQ: launch (ASOC.py:1028-1545), in the order and batches of _plan.
        Returns CTABS[CELLS] and FABSORBED[CELLS,NFREQ] (or None with noabsorbed).  absorbed: a ResidentAbsorptions (zeroed, of this run's
        CELLS and NFREQ) that takes the tallies in place of a host array, and is what is returned as FABSORBED."""
        U, e, c = self.U, self.eng, self.cloud
        CELLS, NFREQ, FFREQ = c.CELLS, self.NFREQ, self.FFREQ
        CTABS = np.zeros(CELLS, np.float32)
        # `nnmake` with `absthin N`: the absorptions of every N-th cell only (ASOC.py:100-105, :632-638)
        thin = U.ABSTHIN if (U.ABSTHIN > 1 and 'nnmake' in U.KEYS) else 1
        self.absthin = thin
        if absorbed is not None:
            why = self.resident_absorptions_refused()
            if why or absorbed.shape != (CELLS, NFREQ):
                raise ValueError("the resident absorptions cannot be the sink of this run: %s" % (why or "%s for %d cells, %d frequencies" % (absorbed.shape, CELLS, NFREQ)))
        # (`libabs`: a column per frequency of its file, ASOC.py:621)
        FABSORBED = absorbed if absorbed is not None else None if U.NOABSORBED else \
            np.zeros(((CELLS + thin - 1) // thin, len(U.FSELECT) if U.LIB_ABS else NFREQ), np.float32)
        if len(U.file_constant_load) > 0:
            self.log("=== CLOAD => %s" % U.file_constant_load)
            return np.fromfile(U.file_constant_load, np.float32, CELLS), FABSORBED
        rng = np.random.default_rng()
        # region of interest (ASOC.py:909-944): record what enters ROI / send in what an enclosing run recorded
        self.ROI_SAVE = self.ROI_LOAD = None
        if U.WITH_ROI_LOAD:
            self.ROI_DIM, self.ROI_LOAD = files.open_roi_load(U.FILE_ROI_LOAD, U.ROI_NSIDE, NFREQ)
        if U.WITH_ROI_SAVE:
            n = e.set_roi_save(U.ROI, U.ROI_STEP, U.ROI_NSIDE)
            self.ROI_SAVE = files.create_roi_save(U.FILE_ROI_SAVE, U.ROI, U.ROI_STEP, U.ROI_NSIDE, NFREQ) if self.rank == 0 \
                else np.zeros((NFREQ, n), np.float32)
        segments, self.freq_owner = self._plan(FABSORBED is not None, thin)
        for policy, name, steps in segments:
            grouped = policy in (self.FREQ_GROUPS, self.LAUNCH_GROUPS)
            per_batch = self.FREQS_PER_SWEEP if policy == self.FREQ_GROUPS else 16
            e.zero(0)
            if policy == self.ONE_BATCH:
                e.batch_begin(0)
            elif policy == self.LAUNCH_GROUPS:
                e.batch_begin_int_groups(per_batch)
            shown, pend = set(), []
            for IFREQ, launches, summed in steps:
                for II, L, _, _ in launches:
                    if II not in shown:
                        shown.add(II)
                        self.log("=== %s  GLOBAL %d x BATCH %d = %d" % (['PS', 'BG', 'DE', 'ROI'][II], L["GLOBAL"], L["BATCH"], L["PACKETS"]))
                t0 = time.time()
                ABS, _ = self._optical_for(IFREQ)
                if self.with_int and policy == self.SEQUENTIAL:
                    e.zero(1)
                self._scatter_tables_for(IFREQ)
                seed = self._seed(IFREQ, rng)
                mine = [m for m in launches if m[3] > 0]
                if not mine and not summed:
                    continue                                   # another rank's launches
                if self.ROI_SAVE is not None:
                    e.roi_zero()                               # per frequency (ASOC.py:1301-1302)
                if policy == self.FREQ_GROUPS and not pend:
                    e.batch_begin_int_groups(per_batch)
                if grouped:
                    e.batch_next_int()
                self.timers["Tpush"] += time.time() - t0
                sent = [self._launch(II, L, IFREQ, seed, first, count) for II, L, first, count in mine]
                sent = [w for w in sent if w is not None]
                if not sent and not summed:
                    continue                                   # nothing to send at this frequency
                if grouped:
                    pend.append((IFREQ, len(sent) > 0, summed))
                    if len(pend) >= per_batch:
                        self._read_int_groups(pend, FABSORBED, policy == self.FREQ_GROUPS)
                        if policy == self.LAUNCH_GROUPS:
                            e.batch_begin_int_groups(per_batch)
                else:
                    t0 = time.time()
                    if self.with_int and summed:
                        self.comm.all_reduce_tally(e, 1)      # one all-reduce of the per-cell buffer per frequency
                    if policy == self.SEQUENTIAL:
                        e.sync()
                    self.timers["Tkernel"] += time.time() - t0
                    t0 = time.time()
                    if absorbed is not None:
                        absorbed.add_tally(self._abs_col(IFREQ))
                    elif FABSORBED is not None or U.SAVE_INTENSITY > 0:
                        TMP = e.read_tally(1)
                        if FABSORBED is not None:
                            FABSORBED[:, self._abs_col(IFREQ)] += TMP[0::thin]
                        if U.SAVE_INTENSITY > 0:
                            self._save_intensity(IFREQ, float(FFREQ[IFREQ]), ABS, TMP)
                    if self.ROI_SAVE is not None:
                        # += : point sources, background and a loaded record all pass here; GL^2 scales away the
                        # dependence on the current grid length (ASOC.py:1466-1475)
                        rec = e.roi_read()
                        if summed:
                            rec = self.comm.all_reduce_host(rec)
                        self.ROI_SAVE[IFREQ, :] += rec * np.float32(U.GL * U.GL)
                    self.timers["Tpull"] += time.time() - t0
                if self.verbose and self.rank == 0 and sent:
                    FF, BG, PS = sent[0]
                    if policy == self.FREQ_GROUPS:
                        print("  FREQ %3d/%3d  %10.3e   TW %10.3e" % (IFREQ + 1, NFREQ, FFREQ[IFREQ], FF))
                    else:
                        print("  FREQ %3d/%3d  %10.3e   BG %12.4e  PS %12.4e   TW %10.3e" % (IFREQ + 1, NFREQ, FFREQ[IFREQ], BG, PS[0], FF))
            if pend or policy == self.LAUNCH_GROUPS:
                self._read_int_groups(pend, FABSORBED, policy == self.FREQ_GROUPS)
            if policy == self.ONE_BATCH:
                t0 = time.time()
                e.batch_end()
                e.sync()
                self.timers["Tkernel"] += time.time() - t0
            self._log_form(name)
            if self.comm:
                self.comm.all_reduce_tally(e, 0)              # TABS: integrated over frequency (and the segment's blocks) on the device
            t0 = time.time()
            CTABS += e.read_tally(0)
            self.timers["Tpull"] += time.time() - t0
            self.log("******  CONSTANT   %10s   CTABS -> %12.4e" % (name, float(np.mean(CTABS))))
        if self.ROI_LOAD is not None:
            e.set_roi_load(None, 0, None)
        if isinstance(self.ROI_SAVE, np.memmap):
            self.ROI_SAVE.flush()
        return CTABS, FABSORBED

    def _read_int_groups(self, pend, FABSORBED, sync):
        """End the batch of INT groups pend = [(IFREQ, launched, summed)] and add each group's tally to FABSORBED: summed over the
        ranks where the plan says so, zeros where this rank launched nothing in the group (the group has no tally slot).  FABSORBED a
        ResidentAbsorptions: every slot is added to its row on the device (one rank: nothing is summed)."""
        e = self.eng
        t0 = time.time()
        e.batch_end()
        if sync:
            e.sync()
        self.timers["Tkernel"] += time.time() - t0
        t0 = time.time()
        slot = 0
        resident = isinstance(FABSORBED, ResidentAbsorptions)
        for IFREQ, launched, summed in pend:
            if resident:
                if launched:
                    FABSORBED.add_slot(self._abs_col(IFREQ), slot)
                    slot += 1
                continue
            arr = np.zeros(self.cloud.CELLS, np.float32)
            if launched:
                arr, slot = e.batch_read_int(slot), slot + 1
            if summed:
                arr = self.comm.all_reduce_host(arr)
            FABSORBED[:, self._abs_col(IFREQ)] += arr[0::self.absthin]
        del pend[:]
        self.timers["Tpull"] += time.time() - t0

    # ---------------------------------------------------------------------------------
    def require_emission_at_every_frequency(self):
        I1, I2 = self.emitted_range()
        if (I2 - I1 + 1 < self.NFREQ) and self.U.ITERATIONS > 0 and self.CLPAC > 0:
            raise ValueError("remit cannot restrict the frequencies when cell emission is simulated (ASOC.py:209-211)")

    @_local_routing()
    def simulate_cell_emission(self, EMITTED, FABSORBED, resident=False):
        """One dust re-emission iteration as a run of its own with `iterations 1` does it (soc_amd.driver's loop): TABS zeroed, the host
        generator made anew, the emission EMITTED[CELLS, NFREQ] of the previous iteration sent from the cells at every simulated
        frequency, each frequency's INT tally added to its column of FABSORBED (a host array, or a ResidentAbsorptions: its row on the
        device).  resident: see _cell_emission_pass."""
        self.require_emission_at_every_frequency()
        if isinstance(FABSORBED, ResidentAbsorptions) and self.resident_absorptions_refused():
            raise ValueError("the resident absorptions cannot be the sink of this run: %s" % self.resident_absorptions_refused())
        self.eng.zero(0)
        hostrng = np.random.default_rng(int(self.U.SEED * 2 ** 31) if self.U.SEED > 0 else None)
        self._cell_emission_pass(EMITTED, hostrng, FABSORBED, True, resident=resident)

    def _cell_emission_pass(self, EMITTED, hostrng, FABSORBED=None, read_int=False, OEMITTED=None, XEM=None, resident=False):
        """One iteration's SimRAM_CL launches (ASOC.py:1700-1910): the dust emission EMITTED[CELLS, emitted_range()] of the previous
        iteration, sent with `cellpackets` packets at every simulated frequency.  The absorptions go to the engine's TABS (zeroed by the
        caller) and, with read_int, the INT tally of every frequency is added to its column of FABSORBED (and goes to the intensity file).
        hostrng: the host generator of `emweight` and of the seeds of a run without `seed`; the iterations of one run share it.
        OEMITTED (reference field): the packets carry EMITTED - OEMITTED, and OEMITTED becomes EMITTED; XEM (ALI): receives the integral
        of the emitted energy.
        resident: the engine holds EMITTED itself (emitted_begin ... emitted_from_mabu) and makes a frequency's emission from it
        (set_emission_column) -- the bits the host statements below hand to set_emission; EMITTED is not looked at (`emweight 0` only)."""
        U, e, c = self.U, self.eng, self.cloud
        CELLS, NFREQ, FFREQ = c.CELLS, self.NFREQ, self.FFREQ
        I1, I2 = self.emitted_range()
        ali = XEM is not None
        if resident and (U.USE_EMWEIGHT > 0 or ali or OEMITTED is not None):
            raise ValueError("the resident emission serves `emweight 0` without ALI and without the reference field")
        COEFF = [U.GL * PARSEC / (8.0 ** level) / launch.FACTOR for level in range(c.LEVELS)]
        EMWEI = np.ones(CELLS, np.float32) * np.float32(self.CLPAC / CELLS) if U.USE_EMWEIGHT > 0 else None
        EMPAC = None
        EMIT = None if resident else np.zeros(CELLS, np.float32)
        GLOBAL, BATCH = self.GLOBAL_0, max(1, int(self.CLPAC / CELLS))
        first, count = self.comm.shard(GLOBAL) if self.comm else (0, GLOBAL)
        skip = U.EMWEIGHT_SKIP - 1
        # TABS-only iterations: the frequencies are handed to the engine together; with `global` raised to
        # about the number of cells they share brick sweeps (include/soc_hip.h: soc_batch_begin, soc_sim_cl)
        deferred = (not self.with_int) and (not ali) and U.USE_EMWEIGHT < 2
        if deferred:
            e.batch_begin(0)
        for IFREQ in range(NFREQ):
            FREQ = float(FFREQ[IFREQ])
            if self.with_int:
                e.zero(1)
            if (FREQ < U.SIM_F[0]) or (FREQ > U.SIM_F[1]):
                continue
            t0 = time.time()
            ABS_f, _ = self._optical_for(IFREQ)
            FF = np.float32(launch.trapezoid_weight(FFREQ, IFREQ))
            self._scatter_tables_for(IFREQ)
            if IFREQ < I1 or IFREQ > I2:
                continue
            if resident:
                e.set_emission_column(IFREQ - I1, np.asarray(COEFF, np.float32))
            else:
                if OEMITTED is not None:                       # ASOC.py:1728-1735
                    EMIT[:] = EMITTED[:, IFREQ - I1] - OEMITTED[:, IFREQ - I1]
                    OEMITTED[:, IFREQ - I1] = EMITTED[:, IFREQ - I1]
                else:
                    EMIT[:] = EMITTED[:, IFREQ - I1]
                for level in range(c.LEVELS):
                    a, b = int(c.OFF[level]), int(c.OFF[level] + c.LCELLS[level])
                    EMIT[a:b] *= COEFF[level] * c.DENS[a:b]
                EMIT[c.DENS < 1.0e-10] = 0.0
            if ali:
                XEM += EMIT * np.float64(FF)                   # integral of the emitted energy (ASOC.py:1741)
            if U.USE_EMWEIGHT > 0:                             # ASOC.py:1745-1771
                skip += 1
                if skip % U.EMWEIGHT_SKIP == 0:
                    tmp = np.asarray(EMITTED[:, IFREQ - I1], np.float64).copy()
                    tmp[~np.isfinite(tmp)] = 0.0
                    tmp[:] = self.CLPAC * tmp / (np.sum(tmp) + 1.0e-65)
                    EMWEI[:] = np.clip(tmp, U.EMWEIGHT_LIM[0], U.EMWEIGHT_LIM[1])
                    EMWEI[hostrng.random(CELLS) > EMWEI] = 0.0
                    if U.EMWEIGHT_LIM[2] > 0.0:
                        EMWEI[EMWEI < U.EMWEIGHT_LIM[2]] = 0.0
                    if U.USE_EMWEIGHT == 2:                    # packets per cell in multiples of 100 (ASOC.py:1773-1780)
                        EMPAC = np.asarray(100 * np.round(tmp / 100), np.int32)
                        EMWEI[:] = 1.0 / (EMPAC + 1e-10)
            if not resident:
                e.set_emission(EMIT, EMWEI)
            if U.SEED > 0:
                seed = float(np.fmod(U.SEED + IFREQ * launch.SEED1, 1.0))      # ASOC.py:1807 (no SEED0 here)
            else:
                seed = float(hostrng.random())
                if self.comm and self.world > 1:
                    seed = self._bcast_seed(seed)
            self.timers["Tpush"] += time.time() - t0
            t0 = time.time()
            if U.USE_EMWEIGHT == 2 and EMPAC is not None:
                # the host lists the cells that still owe packets, 100 per cell and launch (ASOC.py:1811-1840)
                EMDONE = np.zeros(CELLS, np.int32)
                EMINDEX = np.zeros(CELLS, np.int32)
                f2, c2 = self.comm.shard(8192) if self.comm else (0, 8192)
                while True:
                    mm = np.nonzero(EMDONE < EMPAC)[0]
                    if len(mm) < 1:
                        break
                    EMINDEX[:len(mm)] = mm
                    EMINDEX[len(mm):] = -1
                    e.set_emindex(EMINDEX)
                    e.sim_cl(2, self.CLPAC, BATCH, seed, FF, 8192, gid_first=f2, gid_count=c2)
                    EMDONE[mm] += 100
                    self.packets += 100 * len(mm)
            else:
                e.sim_cl(2, self.CLPAC, BATCH, seed, FF, GLOBAL, gid_first=first, gid_count=count)
            if self.with_int and self.comm:
                self.comm.all_reduce_tally(e, 1)
            if not deferred:
                e.sync()
            self.timers["Tkernel"] += time.time() - t0
            self.packets += CELLS * BATCH
            if read_int and isinstance(FABSORBED, ResidentAbsorptions):
                FABSORBED.add_tally(IFREQ)
            elif read_int and (FABSORBED is not None or U.SAVE_INTENSITY > 0):
                TMP = e.read_tally(1)
                if FABSORBED is not None:
                    FABSORBED[:, IFREQ] += TMP[0::self.absthin]
                if U.SAVE_INTENSITY > 0:                       # ASOC.py:1885-1908
                    self._save_intensity(IFREQ, FREQ, ABS_f, TMP)
        if deferred:
            t0 = time.time()
            e.batch_end()
            e.sync()
            self.timers["Tkernel"] += time.time() - t0
        if self.comm:
            self.comm.all_reduce_tally(e, 0)
            if ali:
                self.comm.all_reduce_tally(e, 2)

    @_local_routing()
    def emission_iterations(self, CTABS, FABSORBED):
        """Simulation <-> temperature cycles (ASOC.py:1593-2260, the paths without reference field and
        ALI): per iteration the dust emission of the previous one is simulated with SimRAM_CL
        (`cellpackets`), the integrated absorptions TABS + CTABS give the equilibrium temperature of
        every cell and that the emission at every frequency -- EqTemperature and Emission on the device
        with the keys `CLT` / `CLE` in the ini, else the reference's host formulas (its host temperature loop uses
        a different interpolation weight, ASOC.py:2060).  Writes the temperature and emitted files.
        Returns (TNEW or None, EMITTED[CELLS, REMIT_NFREQ])."""
        U, e, c = self.U, self.eng, self.cloud
        CELLS, NFREQ, FFREQ = c.CELLS, self.NFREQ, self.FFREQ
        I1, I2 = self.emitted_range()
        solve = (not U.NOSOLVE) and bool(U.NOABSORBED)
        if solve and self.NDUST > 1:
            raise ValueError("temperatures can be solved here for a single dust component only (ASOC.py:260-263)")
        self.require_emission_at_every_frequency()
        EMITTED = None
        try:
            EMITTED = np.array(files.mmap_emitted(U.file_emitted, CELLS, I2 - I1 + 1))
        except (OSError, files.FileError, ValueError):
            EMITTED = np.zeros((CELLS, I2 - I1 + 1), np.float32)
        TNEW = None
        if solve:
            Emin, kE, TTT = launch.temperature_table(FFREQ, self.AFABS[0], U.GL)
            FACTOR_f, LENGTH_f = launch.kernel_literals(U.GL)
        ali = bool(U.WITH_ALI)
        if ali:
            e.set_ali(1)
        beta = None
        hostrng = np.random.default_rng(int(U.SEED * 2 ** 31) if U.SEED > 0 else None)
        # reference field (`reference` key, ASOC.py:796-812, :1571-1586): the packets of an iteration carry the CHANGE of
        # the emission since the previous one, EMITTED - OEMITTED; the absorptions the previous emission caused, OTABS,
        # are added back on the host.  Both are damped by k = iteration/ITERATIONS at the start of an iteration, so the
        # first one simulates the full field.  reference = AABB continues a run of AA iterations at iteration BB.
        ref = int(U.WITH_REFERENCE)
        OEMITTED = OTABS = OXAB = OXEM = None
        if ref > 0 and self.CLPAC > 0:
            if I2 - I1 + 1 != NFREQ:
                raise ValueError("the reference field needs emission at every simulated frequency (ASOC.py:797)")
            OEMITTED = np.zeros((CELLS, NFREQ), np.float32)
            OTABS = np.zeros(CELLS, np.float32)
            if ref > 1 and ref % 100 > 0:
                OEMITTED[:, :] = np.fromfile('OEMITTED.save', np.float32).reshape(CELLS, NFREQ)
                OTABS[:] = np.fromfile('OTABS.save', np.float32)
            if ali:
                OXAB, OXEM = np.zeros(CELLS, np.float32), np.zeros(CELLS, np.float32)
        for iteration in range(U.ITERATIONS):
            self.log("ITERATION %d/%d" % (iteration + 1, U.ITERATIONS))
            e.zero(0)
            XEM = np.full(CELLS, 1.0e-32, np.float64) if ali else None      # ASOC.py:1606
            if OEMITTED is not None:                                         # ASOC.py:1607-1632
                k = iteration / float(U.ITERATIONS) if ref == 1 else (iteration + ref % 100) / float(ref // 100)
                OEMITTED *= np.float32(k)
                OTABS *= np.float32(k)
            if self.CLPAC > 0:
                self._cell_emission_pass(EMITTED, hostrng, FABSORBED, iteration == U.ITERATIONS - 1, OEMITTED, XEM)
                if OEMITTED is not None:
                    # the device holds the absorptions of EMITTED - OEMITTED: add what OEMITTED caused (ASOC.py:1965-1975)
                    EABS = e.read_tally(0) + OTABS
                    OTABS[:] = EABS
                    EABS = EABS + CTABS
                    if ali:                                        # ASOC.py:1925-1936
                        OXAB += e.read_tally(2)
                        OXEM += np.asarray(XEM, np.float32)
                        beta = (OXEM - OXAB) / OXEM
                else:
                    EABS = e.read_tally(0) + CTABS
                    if ali:
                        beta = (XEM - e.read_tally(2)) / XEM       # escape probability (ASOC.py:1939-1942)
            else:
                EABS = np.array(CTABS, np.float32)
            if solve:
                t0 = time.time()
                # the ini keys pick the solver as in the reference: `CLT` (without ALI) = the EqTemperature kernel,
                # otherwise its host loop, the only one that knows beta (ASOC.py:2027, :2042; `MPT` = the same
                # formula on several processes); `CLE` = the Emission kernel, otherwise the host formula (:2159, :2199)
                if ('CLT' in U.KEYS) and not ali:
                    TNEW = e.solve_temperature(launch.ADHOC, kE, Emin, TTT, FACTOR_f, LENGTH_f, EABS)
                else:
                    TNEW = launch.solve_temperature_host(EABS, c, Emin, kE, TTT, U.GL, beta if ali else None,
                                                         empty_below=0.0 if 'MPT' in U.KEYS else 1.0e-10)
                if CELLS < 1e8:                                    # ASOC.py:2122-2136
                    TNEW[~np.isfinite(TNEW)] = 10.0
                    mok = c.DENS > 1.0e-8
                    TNEW[mok] = np.clip(TNEW[mok], 3.0, 1600.0)
                if 'CLE' in U.KEYS:
                    e.set_temperature(TNEW)                        # ASOC.py:2160: the host's TNEW goes to the device
                    EMITTED[:, :] = e.emission(FFREQ[I1:I2 + 1], self.AFABS[0][I1:I2 + 1], FACTOR_f, LENGTH_f)
                else:
                    if I1 > 0:
                        raise ValueError("the host emission loop indexes EMITTED with the frequency index (ASOC.py:2215, :2226): "
                                         "with `remit` cutting the low frequencies it fails in the reference; add `CLE`")
                    if 'MPE' in U.KEYS:
                        TNEW[TNEW < 3.0] = 10.0                    # ASOC.py:2211
                    EMITTED[:, :] = launch.emission_host(FFREQ[I1:I2 + 1], self.AFABS[0][I1:I2 + 1], TNEW, U.GL)
                self.timers["Tsolve"] = self.timers.get("Tsolve", 0.0) + time.time() - t0
        if self.rank == 0 and solve and U.ITERATIONS > 0:
            if len(U.file_temperature) > 0:
                files.write_temperature(U.file_temperature, c, TNEW)
            files.write_emitted(U.file_emitted, EMITTED)
            if OEMITTED is not None and ref > 1:                   # for the run that continues this one (ASOC.py:2251-2253)
                OEMITTED.tofile('OEMITTED.save')
                OTABS.tofile('OTABS.save')
        return TNEW, EMITTED

    def emission_from_temperature_file(self):
        """`loadtemp` with `iterations 0` (ASOC.py:700-764): the emission of an equilibrium dust from a stored temperature
        file, through the Emission kernel; written to the `emitted` file and used for the maps"""
        U, e, c = self.U, self.eng, self.cloud
        if self.NDUST > 1:
            raise ValueError("loadtemp recomputes the emission of a single equilibrium dust (ASOC.py:757-760 uses AFABS[0])")
        I1, I2 = self.emitted_range()
        TNEW = files.read_temperature(U.file_temperature, c)
        FACTOR_f, LENGTH_f = launch.kernel_literals(U.GL)
        e.set_temperature(TNEW)
        EMITTED = np.asarray(e.emission(self.FFREQ[I1:I2 + 1], self.AFABS[0][I1:I2 + 1], FACTOR_f, LENGTH_f), np.float32)
        if self.rank == 0 and len(U.file_emitted) > 0:
            files.write_emitted(U.file_emitted, EMITTED)
        return TNEW, EMITTED

    # ---------------------------------------------------------------------------------
    def _bcast_seed(self, seed):
        t = self.comm.torch.tensor([seed], dtype=self.comm.torch.float64,
                                   device="cuda" if self.comm.backend == "nccl" else "cpu")
        self.comm.dist.broadcast(t, 0)
        return float(t[0])

    # ---------------------------------------------------------------------------------
    def run(self):
        t00 = time.time()
        self.write_packet_info()
        self.setup_engine()
        CTABS, FABSORBED = self.simulate_constant_sources()
        U = self.U
        self.TNEW, self.EMITTED = None, None
        if U.ITERATIONS > 0 and (self.CLPAC > 0 or ((not U.NOSOLVE) and U.NOABSORBED)):
            self.TNEW, self.EMITTED = self.emission_iterations(CTABS, FABSORBED)
        elif U.LIB_MAPS:                                           # the emission of the library, its frequencies only (ASOC.py:601-603)
            self.EMITTED = files.mmap_emitted(U.file_emitted, self.cloud.CELLS, len(U.FSELECT))
        elif U.LOAD_TEMPERATURE and U.ITERATIONS < 1:
            self.TNEW, self.EMITTED = self.emission_from_temperature_file()
        if (not U.NOMAP) and self.EMITTED is not None:
            self.write_maps(self.EMITTED)
        if U.POLMAP and self.EMITTED is not None:                 # also under `nomap` (ASOC.py:3655)
            self.write_polmaps(self.EMITTED)
            self.write_healpix_polmaps(self.EMITTED)              # NPIX.y < 0, and not under `nomap` (:3808)
        if U.NO_PS > 0 and U.pssavetau_freq > 0.0 and U.NPIX[1] > 0:
            self.write_ps_tau()
        if self.rank == 0 and self.INTENSITY is not None:          # ASOC.py:2733-2757
            files.finish_intensity_file(U.SAVE_INTENSITY_FILE, self.INTENSITY, self.cloud.CELLS, self.NFREQ, U.SAVE_INTENSITY == 2)
            self.INTENSITY = None
        if self.rank == 0:
            if len(U.file_constant_save) > 0:
                CTABS.tofile(U.file_constant_save)                 # ASOC.py:1547-1549
            if FABSORBED is not None and self.freq_owner is None:
                files.scale_absorbed(FABSORBED, self.cloud, U.GL, U.NNNLIMIT, self.absthin)
                files.write_absorbed(U.file_absorbed, FABSORBED)   # ASOC.py:2866-2875
            elif FABSORBED is None:
                prefix = U.KEYS.get('prefix', ['soc'])[0] if U.KEYS.get('prefix') else 'soc'
                CTABS.tofile(prefix + ".ctabs")
        if FABSORBED is not None and self.freq_owner is not None:
            # every rank holds the columns of the frequencies it simulated and writes them itself: no collective (as a2e.run_sharded)
            files.scale_absorbed(FABSORBED, self.cloud, U.GL, U.NNNLIMIT, self.absthin)
            if self.rank == 0:
                files.create_absorbed(U.file_absorbed, FABSORBED.shape[0], FABSORBED.shape[1])
            self.comm.barrier()
            mine = [self._abs_col(f) for f, r in self.freq_owner.items() if r == self.rank]
            if self.rank == 0:
                owned = {self._abs_col(f) for f in self.freq_owner}
                mine += [k for k in range(FABSORBED.shape[1]) if k not in owned]               # frequencies outside `simum`: nobody's
            files.write_absorbed_columns(U.file_absorbed, FABSORBED, mine)
            self.comm.barrier()
        wall = time.time() - t00
        if self.rank == 0 and self.verbose:
            print("Tkernel %.3f  Tpush %.3f  Tpull %.3f" % (self.timers["Tkernel"], self.timers["Tpush"], self.timers["Tpull"]))
            if self.timers["Tkernel"] > 0:
                print("%.4e photon packets / s (simulation section, %d GPU%s)" % (
                    self.packets / self.timers["Tkernel"], self.world, "s" if self.world > 1 else ""))
            print("@@ asoc %.2f seconds WC" % wall)
        return CTABS, FABSORBED


def main(argv=None):
    argv = sys.argv if argv is None else argv
    if len(argv) < 2:
        print("Usage:  python -m soc_amd.asoc ini-file")
        return 1
    from .dist import Comm
    from .lib import Engine
    USER = User(argv[1])
    comm = Comm()
    eng = Engine(comm.local_rank)
    try:
        AbsorptionRun(USER, eng, comm).run()
    finally:
        eng.close()
        comm.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
