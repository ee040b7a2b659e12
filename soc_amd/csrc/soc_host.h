// soc_host.h -- what the host units of libsoc_hip.so share (soc_capi.hip, soc_capi_post.hip, soc_capi_a2e.hip, soc_capi_reemit.hip, soc_capi_absorbed.hip, soc_capi_library.hip, soc_capi_mabu_library.hip, soc_capi_probe.hip):
// the handle, the error and flush idioms.  Every device allocation of a handle is a DevBuf (soc_devbuf.h) that the handle owns: its
// members, and the packet records, queues and bricks of its brick sweeps (SocSweepState, soc_brick.hip).  Kernels do not include it.
#pragma once
#include "../../include/soc_hip.h"
#include "soc_dev.h"
#include "soc_devbuf.h"
#include "soc_rows.h"

#include <string>
#include <vector>

struct soc_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // model
    bool have_grid = false;
    SocGrid G{};
    DevBuf<float> dDENS;
    DevBuf<int>   dPAR;
    int64_t npar = 0;
    // tables / per-frequency data
    DevBuf<float> dCSC, dDSC;
    int    BINS = 0;
    bool   have_dsc = false;
    // scattered-light view (soc_sca_*)
    SocSca view{};
    DevBuf<float4> dODIR, dORA, dODE;
    DevBuf<float>  dOUT;               // the image: the library's own, or a caller's (soc_sca_bind_out)
    bool   have_view = false;
    float  ABS = 0.0f, SCA = 0.0f;
    bool   have_optical = false;
    DevBuf<float2> dOPT;
    DevBuf<float>  dEMIT, dEMWEI, dXAB;
    DevBuf<float>  dINTV;              // -D SAVE_INTENSITY=2: INTX | INTY | INTZ, CELLS floats each (with_int == 2)
    DevBuf<int>    dEMINDEX;
    bool   have_emit = false, have_emindex = false, with_ali = false;
    DevBuf<float> dHPBG, dHPBGP;       // Healpix sky of the current frequency (NSIDE 64)
    DevBuf<float> dABU, dAF;           // abundances [CELLS, NDUST] (or [CELLS]), cross sections of the frequency
    int    abu_ndust = 0, abu_single = 0;
    int    map_level_threshold = 0;    // -D LEVEL_THRESHOLD (soc_set_map_threshold)
    int    map_interpolation = 0;      // -D MAP_INTERPOLATION (soc_set_map_interpolation)
    int    map_roi_on = 0, map_roi[6] = { 0, 0, 0, 0, 0, 0 };   // -D ROI_MAP (soc_set_map_roi)
    float  cr_rate = 0.0f;             // -D CR_HEATING_RATE with -D CR_HEATING=1 (soc_set_cr_heating); 0 = off
    bool   opt_half = false;          // -D OPT_IS_HALF: OPT rounded through fp16 (soc_set_opt_half)
    bool   opt_from_abu = false;       // dOPT and dAF hold the current frequency's soc_set_optical_abu values
    int    msf_ndust = 1;              // > 1: -D WITH_MSF, dCSC/dDSC hold [msf_ndust][BINS] (soc_set_scatter_tables)
    int    step_weight = 0;            // -D STEP_WEIGHT (soc_set_step_weight)
    float  sw_a = 0.0f, sw_b = 0.0f;
    size_t abu_cells = 0;              // the cell count the abundances were set for; 0: none are set (dABU may still be allocated)
    SocRoi roi{};                      // region of interest (host copy of *dRoi)
    DevBuf<SocRoi> dRoi;
    DevBuf<float>  dRoiSave, dRoiLoad; // the record written (its entries: dRoiSave.n) and the one loaded
    bool   have_hpbg = false, hpbg_weighted = false;
    // tallies: the library's own, or a caller's (soc_bind_tally)
    DevBuf<float> dTABS, dINT;
    // deferred launches (soc_batch_begin .. soc_batch_end): executed together in one brick sweep (scattered light: one sweep of rays)
    bool   batching = false;
    int    batch_max = 4;
    std::vector<SocSim> pending;
    // Device copies of launch inputs, one buffer (of bytes) per store and launch slot (slot_buf): a deferred launch keeps in its slot
    // what the caller overwrites for the next frequency; slot 0 also holds the point sources of a launch that runs at once.  SLOT_INT
    // holds the INT tallies of a batch by group (soc_batch_read_int), SLOT_OPT one buffer in slot 0 (the sweep strides through it).  A
    // buffer is allocated when its slot first needs more than it holds (128 slots of a 5e7-cell model up front would be 50 GB).
    enum SlotStore { SLOT_SRC, SLOT_CSC, SLOT_DSC, SLOT_OPT, SLOT_EMIT, SLOT_HP, SLOT_INT, SLOT_STORES };
    DevBuf<char> slots[SLOT_STORES][SOC_MAXLAUNCH];
    DevBuf<float> dOUTslots;                                  // soc_sca_batch_images: several images, one per frequency of a batch
    int    out_slots = 0, out_slot_cur = 0;
    size_t out_slot_pixels = 0;
    unsigned long long emit_gen = 0;              // bumped by soc_set_emission: launches deferred without a change in between share one copy
    unsigned long long emit_slot_gen = 0;
    int    emit_slot_last = -1;
    unsigned long long opt_gen = 0;               // bumped by soc_set_opt / soc_set_optical_abu: on brick-local hierarchies the launches deferred
    unsigned long long opt_slot_gen = 0;          // without a change in between share one copy of the per-cell opacities (keep_inputs)
    int    opt_used = 0;                          // ... the copies the pending launches hold: slots [0, opt_used) of SLOT_OPT
    int    int_slots_done = 0;                    // launches of the last executed sweep whose INT can be read
    // the INT tally of the launches of a batch (set by the soc_batch_begin* call that opened it):
    //   INT_OFF        soc_batch_begin: launches with the INT tally are not deferred
    //   INT_SHARED     soc_batch_begin_shared_int: all tally into the handle's dINT
    //   INT_PER_LAUNCH soc_batch_begin_int: every launch a zeroed slot of its own (SLOT_INT)
    //   INT_PER_GROUP  soc_batch_begin_int_groups: the launches up to the next soc_batch_next_int share a slot
    enum IntMode { INT_OFF, INT_SHARED, INT_PER_LAUNCH, INT_PER_GROUP } int_mode = INT_OFF;
    bool   int_group_open = false;                // INT_PER_GROUP: the current group has its slot
    // rng
    DevBuf<uint64_t> dSeedTab;
    DevBuf<unsigned long long> dStats;
    DevBuf<float> dSplitStack;                               // soc_sim_bg_split / soc_sim_hp_split: the ray stacks, kept from the first launch on
    DevBuf<unsigned long long> dSplitStats;                  // soc_split_stats: 6 sums, the maximum stack depth, the skipped splits
    unsigned long long split_depth = 0;                      // that maximum, as of the last soc_split_stats
    unsigned long long split_skipped = 0;                    // the skipped splits of soc_sim_hp_split, as of the last soc_split_stats
    unsigned long long ray_steps = 0;                      // cell steps of the rays of the scattered-light sweeps, as of the last soc_stats
    // features
    int with_int = 0, ps_method = 0, use_emweight = 0, mirror = 0;
    // execution
    int exec_mode = -1, brick_log2 = 4;
    SocSweepResult last;                          // the last sweep's passes and form; variant: soc_last_variant, the absorption kernel last launched (-1: none yet)
    SocBrickTune tune{};
    SocSweepState *sweep = soc_sweep_new();       // what the handle's brick sweeps keep on the device (soc_brick.hip); goes with the handle
    ~soc_ctx() { soc_sweep_delete(sweep); }
    // equilibrium temperature / emission (soc_emit.hip)
    DevBuf<float> dT, dTTT, dEbuf, dEF;
    bool   have_T = false;
    // map making (soc_map.hip)
    DevBuf<float>  dMapEmit, dMap, dMapTau;
    // the resident batch of soc_map_set_block: emission [CELLS][mapx_nf], ABS | SCA [2 * mapx_nf], per-cell opacities (or none);
    // the planes of soc_map_block: MAPX | TAUX | COLDEN; those of soc_map_block_levels: MAPL[mapx_nf][LEVELS][npix], freed with the batch
    DevBuf<float>  dMapXEmit, dMapXOpa, dMapXOut, dMapLOut;
    DevBuf<float2> dMapXOpt;
    int     mapx_nf = 0;               // 0: no batch
    DevBuf<float4> dBfield;            // magnetic field, one (Bx, By, Bz, pad) per cell (soc_set_bfield)
    DevBuf<float>  dPolMap;            // the four planes of a polarisation map
    // A2E
    int a2e_NE = 0, a2e_NFREQ = 0, a2e_npair = 0, a2e_noIw = 0;
    DevBuf<float> aIw, aTdown, aEA, aAF;
    DevBuf<float> aABS, aEMIT;                               // a batch of cells, a2e_NFREQ floats each (soc_a2e_set_size with another NFREQ releases them)
    DevBuf<float> aAll, aSum;                                // soc_a2e_resident_*: absorptions of all cells, emission summed over the sizes
    DevBuf<float> aPSum, aAalg;                              // polarised output (soc_a2e_resident_begin_pol, soc_mabu_begin_pol): the weighted sum over
                                                             // the sizes, and a_alg with its log10 per cell ([cells][2])
    bool    a2e_pol_set = false;                             // soc_a2e_set_size_aalg has given the weights of the current size
    float   a2e_pol[4] = { 0, 0, 0, 0 };                     // ASIZE[isize], ASIZE[isize+1] or 0, log10(ASIZE[isize]), the difference of the logarithms
    int64_t a2e_cells = 0;                                   // cells resident in aAll and aSum, a2e_res_nfreq floats each: the rows a call may address
    int     a2e_res_nfreq = 0;
    DevBuf<int> aFirst, aLast, aIwOff, aDst, aIbeg;
    // the equilibrium sizes of a dust (soc_a2e_set_eq_sizes): aEqTab = FREQ[NFREQ] | AF | KABS [nsizes][NFREQ] | TTT[nsizes][NIP],
    // aEqPar = Emin | kE | oplgkE | GD * S_FRAC | S_FRAC | SIZE_A, nsizes floats each
    DevBuf<float> aEqTab, aEqPar;
    int     eq_nsizes = 0, eq_NFREQ = 0, eq_NIP = 0;         // eq_nsizes 0: none are set
    float   eq_FACTOR = 0.0f, eq_GD = 0.0f;
    bool    eq_pol = false;                                  // SIZE_A was given: the sizes also add to the polarised sum
    // temperatures and populations on request: aTeq[teq_nsizes][a2e_cells] of the last soc_a2e_resident_solve_eq (teq_nsizes 0: none
    // kept; teq_keep: soc_a2e_resident_keep_teq is on), aXX the clamped populations of one batch or one chunk of cells, a2e_NE floats
    // each (soc_a2e_solve_dump, soc_a2e_resident_solve_dump).  The resident block's end releases them and the switch
    DevBuf<float> aTeq, aXX;
    bool    teq_keep = false;
    int     teq_nsizes = 0;
    bool    mabu_t_set = false;                              // a soc_mabu_solve_eq has filled mT since soc_mabu_begin
    // the multi-dust stage (soc_mabu_*): absorptions as the absorbed file holds them, the sum over the dusts, abundances, relative cross
    // sections, temperatures and tables of an equilibrium dust; the current dust's share and its emission are aAll and aSum
    DevBuf<float>  mABS, mSUM, mABU, mT, mTab;
    DevBuf<double> mRABS, mPol;                              // (mPol: APOL[NA] and TAB[NFREQ][NA] of soc_mabu_pol_eq)
    DevBuf<float>  mPSUM;                                    // soc_mabu_begin_pol: the abundance-weighted sum of the polarised emission, then R
    int     mabu_ndust = 0;
    bool    mabu_tables = false;
    // the resident emission of the re-emission iterations (soc_emitted_*): ET[et_nfreq][CELLS], transposed so that a frequency is a
    // contiguous row; eRows stages the rows of an upload or a download.  soc_set_grid releases both
    DevBuf<float> eET, eRows;
    int     et_nfreq = 0;              // 0: not open
    // soc_emitted_change, reserved at its first call after soc_emitted_begin: the luminosities L[CELLS] of the call before, its scratch
    // (W[et_nfreq] | STATS[4] | the partials [blocks][4]) and the count of bad cells.  Released wherever eET is (release_change)
    DevBuf<double> eLp, eChange;
    DevBuf<unsigned long long> eBad;
    void release_change() { eLp.release();  eChange.release();  eBad.release(); }
    // the resident absorptions, their mirror image (soc_absorbed_*): AT[at_nfreq][CELLS], a frequency's INT tally added to its row;
    // bAC a second plane of the same size (soc_absorbed_keep / _restore: the constant sources' share), bRows stages a download.
    // soc_set_grid releases all three
    DevBuf<float> bAT, bAC, bRows;
    int     at_nfreq = 0;              // 0: not open
    bool    ac_kept = false;           // bAC holds what soc_absorbed_keep copied
    // the library method (soc_library_*): the resident table -- I1 | dI1 | I2 | dI2 | X | Y | Z | E0 in one block, the selected emission
    // columns [N^3][lib_nout] -- and the miss list of a look-up
    int     lib_N = 0, lib_nout = 0;
    float   lib_I0 = 0.0f, lib_dI0 = 0.0f;
    DevBuf<float> lTab, lE;
    DevBuf<int>   lMiss;
    DevBuf<unsigned long long> lCount;
    // the library method for several dusts (soc_mabu_library_*): the reference absorptions, abundances, sum and miss masks of the
    // resident cells, RABS3[3][ndust], and per dust the tables of soc_library_set (qTab: I1 | dI1 | I2 | dI2 | X | Y | Z | E0; qE the
    // selected emission columns) with their device addresses in qLib[ndust]
    DevBuf<float>    qABS3, qABU, qSUM;
    DevBuf<unsigned> qMISS;
    DevBuf<double>   qRABS3;
    DevBuf<float>    qTab[SOC_MABU_LIB_DUSTS], qE[SOC_MABU_LIB_DUSTS];
    DevBuf<SocLibTables> qLib;
    int64_t mlib_cells = 0;            // 0: not open
    int     mlib_ndust = 0, mlib_nout = 0;
    unsigned mlib_have = 0;            // bit d: dust d has its library
    bool    mlib_tables = false;
};

// the error text of a refused call, for soc_last_error (c == nullptr: of soc_create); returns code
SOC_HIDDEN int fail(soc_ctx *c, int code, const char *fmt, ...);

#define HIPCHK(c, call)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((c), SOC_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));     \
    } while (0)

// Rows [c0, c0 + n) of a resident block of `cells` rows, or the call is refused: THE range check of every transfer call (soc_a2e_resident_*,
// soc_mabu_*, soc_emitted_*, soc_absorbed_*).  The sum is formed for the text alone, unsigned, so a refused huge range prints without overflow
#define SOC_ROWS(c, who, c0, n, cells)                                                                      \
    do {                                                                                                    \
        if (!soc_rows_ok((c0), (n), (cells)))                                                               \
            return fail((c), SOC_ERR_ARG, who ": cells [%lld, %lld) of %lld", (long long)(c0),              \
                        (long long)((unsigned long long)(c0) + (unsigned long long)(n)), (long long)(cells));   \
    } while (0)

// Execute the launches deferred since soc_batch_begin (soc_capi.hip)
SOC_HIDDEN int flush_pending(soc_ctx *c);
#define FLUSH(c)                                    \
    do {                                            \
        int f_ = flush_pending(c);                  \
        if (f_) return f_;                          \
    } while (0)
