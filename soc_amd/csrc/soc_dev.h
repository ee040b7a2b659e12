// soc_dev.h -- structures shared by the C-ABI host code (soc_capi.hip) and the kernels.
#ifndef SOC_DEV_H
#define SOC_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#define SOC_MAXL 16            /* hierarchy levels supported (reference models use <= 8) */

// Model geometry.  The reference bakes these into the kernel with -D NX= ... -D CELLS=
// (ASOC.py:344-362); here they are run-time kernel arguments.
struct SocGrid {
    int NX, NY, NZ, LEVELS, CELLS, NXYZ;
    int OFF[SOC_MAXL];         /* first cell of each level (ASOC_aux.py:772)            */
    int LCELLS[SOC_MAXL];      /* cells per level                                        */
    const float *DENS;         /* [CELLS] density (>0) or child link (<=0)               */
    const int   *PAR;          /* [CELLS-NXYZ] parent cell index within its level        */
};

// Region of interest of nested runs (kernel_ASOC.c:44-51, 1250-1254; -D ROI_STEP, ROI_NSIDE, WITH_ROI_SAVE,
// WITH_ROI_LOAD): packets entering ROI are recorded per surface element and Healpix direction; SOURCE == 3 sends
// such a record in from the model surface.  Lives in device memory, SocSim points at it.
struct SocRoi {
    int   save, load;          /* WITH_ROI_SAVE, WITH_ROI_LOAD                                          */
    int   ROI[6];              /* x0, x1, y0, y1, z0, z1: root cells, inclusive                         */
    int   STEP, NSIDE;         /* surface elements per root-cell edge (save); Healpix NSIDE of the records */
    int   DIM[3], NELEM;       /* discretisation of the record to load; its number of surface elements  */
    float *SAVE;               /* [elements * 12 * NSIDE^2]                                             */
    const float *LOAD;         /* [NELEM * 12 * NSIDE^2] photons                                        */
};

// One launch of SimRAM_PB / SimRAM_CL (argument lists: kernel_ASOC.c:15-52, 1223-1256).
struct SocSim {
    int   SOURCE, BATCH, GLOBAL, PS_METHOD, NO_PS, BINS, USE_EMWEIGHT;
    int   MIRROR;              /* reflecting faces x,X,y,Y,z,Z = 1,2,4,8,16,32 (ASOC.py:319-321) */
    uint32_t gid0, gid_count;  /* this device runs logical work items [gid0, gid0+gid_count) */
    uint64_t seed_mul;         /* BASEID * A^base mod M for this SEED                     */
    const uint64_t *seed_tab;  /* 4 x 256 table of G^(b*256^k), see soc_rng.h             */
    float ABS, SCA, BG, TW;
    const float  *CSC;         /* [BINS] cumulative scattering function, current frequency */
    const float2 *OPT;         /* [CELLS] (abs, sca) per cell when WITH_ABU               */
    const float4 *PSPOS;       /* point-source positions (cl float3 = 16 bytes)           */
    const float  *PS;
    const int    *XPS_NSIDE, *XPS_SIDE;
    const float  *XPS_AREA;
    const float  *EMIT, *EMWEI;
    const int    *EMINDEX;     /* USE_EMWEIGHT == 2: cells to emit from, -1 terminated        */
    float        *XAB;         /* WITH_ALI: absorptions in the emitting cell (else NULL)      */
    int    HPBG_WEIGHTED;      /* SimRAM_HP: pixel chosen by cumulative probability       */
    const float  *HPBG, *HPBGP; /* [49152] sky (photons per package), cumulative probability */
    float *TABS, *INT;
    unsigned long long *stats; /* [0] tally events  [1] packets  [2] scatterings          */
    const SocRoi *ROI;         /* NULL without roisave / roiload                          */
    int    ROILOAD;            /* SOURCE == 3: surface elements of the loaded record (host copy of ROI->NELEM; 0: none loaded) */
    int    ROISAVE;            /* the record of packets entering ROI is kept (host copy of ROI->save: the sweep's queues depend on it) */
    int    STEP_WEIGHT;        /* -D STEP_WEIGHT: 0 none, 1 | 2 weighted free paths (kernel_ASOC.c:516-535) */
    float  SW_A, SW_B;
    int    NDUST;              /* > 1: -D WITH_MSF, CSC holds [NDUST][BINS] (kernel_ASOC.c:777-795)          */
    const float  *MSF_SCA;     /* [NDUST] scattering cross sections of the species, current frequency       */
    const float  *ABU;         /* [CELLS][NDUST] abundances                                                  */
    float  *INTV;              /* -D SAVE_INTENSITY=2: INTX | INTY | INTZ (CELLS each), else NULL; direct kernels only */
    int     CELLS;             /* stride of INTV                                                             */
    /* a launch of the scattered-light kernels run as a sweep of rays (soc_brick.hip: soc_sca_events): which kernel, its
     * discrete scattering function and the image it adds to (launches of one sweep may belong to several frequencies) */
    int          SCAKIND;      /* SOC_SCA_* + 1; 0: an absorption launch                                     */
    const float *DSC;          /* [BINS]                                                                     */
    float       *OUT;          /* [NDIR*NPIX_Y*NPIX_X]                                                       */
};

#define SOC_SOURCE_HP 4        /* brick sweep only: the launch is a SimRAM_HP one (Healpix sky instead of BG) */
#define SOC_SOURCE_CL 5        /* brick sweep only: a SimRAM_CL launch (cell emission)                        */

// Several launches of SimRAM_PB executed in one brick sweep (soc_brick.hip): launch l owns the
// sweep's work items [first[l], first[l+1]); geometry and tallies are shared.  Lives in device memory
// (16 launches exceed the 4 KB of kernel arguments).  128: the two source blocks of a 50-frequency run (ASOC.py:1028-1545) fit one sweep.
#define SOC_MAXLAUNCH 128
struct SocSimPack {
    int      n;
    // launches that tally into one INT array form a group (the source blocks of one frequency): with several groups in a sweep the
    // brick queues are per group -- a workgroup's LDS tallies then belong to one INT array -- queue = group * NB + brick
    int      grp[SOC_MAXLAUNCH];         // group of every launch
    int      gfirst[SOC_MAXLAUNCH];      // a launch of every group (for its INT / INTV pointers)
    uint32_t first[SOC_MAXLAUNCH + 1];
    SocSim   S[SOC_MAXLAUNCH];
};

// feature switches that the reference selects with #if; compiled ahead of time here
struct SocVariant {
    int octree;                /* LEVELS > 1                                              */
    int dbl;                   /* Index() in double: NX > DIMLIM (kernel_ASOC_aux.c:25-37) */
    int abu;                   /* WITH_ABU                                                */
    int wint;                  /* INT tally: SAVE_INTENSITY in (1,2) or NOABSORBED==0     */
};

hipError_t soc_launch_sim_pb(const SocGrid &G, const SocSim &S, const SocVariant &V, hipStream_t st);
hipError_t soc_launch_sim_cl(const SocGrid &G, const SocSim &S, const SocVariant &V, hipStream_t st);
hipError_t soc_launch_sim_hp(const SocGrid &G, const SocSim &S, const SocVariant &V, hipStream_t st);
// SimBgSplit and SimHpSplit (soc_split.hip; kernel_ASOC.c:2117-2143, :2871-2894): what a split launch has beyond SocSim
struct SocSplit {
    int    SELEM, max_split;   /* -D SELEM (SimBgSplit only), -D MAX_SPLIT                                     */
    float *stack;              /* per wave a tile of max_split x 10 x 64 words: word (slot, field, lane) at (slot*10 + field)*64 + lane */
    unsigned long long *counters;   /* soc_split_stats: six sums, [6] the maximum stack depth, [7] SimHpSplit's skipped splits */
};
hipError_t soc_launch_sim_bg_split(const SocGrid &G, const SocSim &S, const SocSplit &P, const SocVariant &V, hipStream_t st);
hipError_t soc_launch_sim_hp_split(const SocGrid &G, const SocSim &S, const SocSplit &P, const SocVariant &V, hipStream_t st);
hipError_t soc_launch_parents(const SocGrid &G, int *PAR, hipStream_t st);
hipError_t soc_launch_seed_probe(uint64_t seed_mul, const uint64_t *tab, uint32_t gid0, uint32_t n,
                                 int ndraw, uint32_t *out_state, uint32_t *out_draws, hipStream_t st);
hipError_t soc_launch_math_probe(int fn, const float *x, const float *x2, float *y, long n, hipStream_t st);
hipError_t soc_launch_trace(const SocGrid &G, const SocVariant &V, const float *pos, const float *dir,
                            int maxsteps, int *levels, int *inds, float *dss, float *endpos, int *nsteps,
                            hipStream_t st);


// scattered-light images (soc_sca.hip): observers and image of one launch of the
// kernel_ASOC_sca.c kernels (argument lists :471-501, :1098-1122, :1462-1489)
enum { SOC_SCA_PB = 0, SOC_SCA_CL = 1, SOC_SCA_PS = 2, SOC_SCA_HP = 3 };
struct SocSca {
    int   kind, NDIR, NPIX_X, NPIX_Y, FFS;   /* NDIR < 0: Healpix map of NSIDE = -NDIR seen from ODIRS[0] (a position) */
    float MAP_DX, CX, CY, CZ;
    const float4 *ODIRS, *ORA, *ODE;   /* [NDIR] cl float3 = 16 bytes                      */
    const float  *DSC;                 /* [BINS] discrete scattering function              */
    float *OUT;                        /* [NDIR*NPIX_Y*NPIX_X]                             */
};
hipError_t soc_launch_sca(const SocGrid &G, const SocSim &S, const SocSca &V, const SocVariant &X, hipStream_t st);

// equilibrium temperature and thermal emission (soc_emit.hip)
hipError_t soc_launch_eqtemp(const SocGrid &G, float adhoc, float kE, float Emin, int NE, float FACTOR, float LENGTH, float cr_rate,
                             const float *TTT, const float *EABS, float *TNEW, hipStream_t st);
hipError_t soc_launch_emission(int c0, int c1, int nfreq, float FACTOR, float LENGTH, const float *FREQ, const float *FABS,
                               const float *T, float *EMIT, hipStream_t st);

// solver-file preprocessing (soc_a2e_pre.hip): integration weights and cooling rates of one grain size
#define SOC_A2E_PRE_NFREQ_MAX 639      // the weights kernel keeps 64 columns of NFREQ floats and 64 ints in LDS: (639*64 + 64)*4 B = 160 KB
hipError_t soc_launch_a2e_pre(int NFREQ, int NE, float FACTOR, const float *FREQ, const float *Ef, const float *SKABS, const float *E, const float *T,
                              int *L1, int *L2, float *IW, float *wrk, int *noIw, float *Tdown, hipStream_t st);

// OPT from abundances on the device (soc_emit.hip)
hipError_t soc_launch_opt(int cells, int ndust, int single, const float *ABU, const float *AF, float2 *OPT, hipStream_t st);
hipError_t soc_launch_opt_half(int cells, float2 *OPT, hipStream_t st);

// map making (soc_map.hip): one launch of Mapping / HealpixMapping (kernel_ASOC_map.c:496-516, 890-910)
// what fixes the lines of sight of a map, whatever is integrated along them
struct SocMapView {
    int   mode;                    // 0 Mapping, 1 HealpixMapping (NSIDE = NPIX_X)
    int   NPIX_X, NPIX_Y;
    int   ROI_MAP, ROI[6];         // -D ROI_MAP: only the emission of cells inside ROI = [x0,x1,y0,y1,z0,z1] (root cells, inclusive)
    int   LEVEL_THRESHOLD;         // Mapping: no emission from levels below it (-D LEVEL_THRESHOLD, kernel_ASOC_map.c:825-834)
    int   MAPINT;                  // Mapping: -D MAP_INTERPOLATION 0 | 1 | 2 (kernel_ASOC_map.c:656-810)
    float MAP_DX, LENGTH;
    float DIR[3], RA[3], DE[3], CENTRE[3], INTOBS[3];
};
struct SocMapArgs : SocMapView {
    int   SAVE_COLDEN;
    float ABS, SCA;
    const float  *EMIT;
    const float2 *OPT;
    float *MAP, *SAVETAU;
};
hipError_t soc_launch_map(const SocGrid &G, const SocMapArgs &A, bool abu, hipStream_t st);
// the maps of a batch of frequencies from one walk per pixel (soc_map.hip: soc_mapx_kernel; the `mapping nx ny dx NF` of
// ASOC.py:3442-3568, whose kernel_ASOC_map_X.c the reference does not ship): nf <= SOC_MAPX_MAX frequencies, cell-major inputs
#define SOC_MAPX_MAX 32
struct SocMapXArgs : SocMapView {
    int   nf;
    const float  *EMIT;            // [CELLS][nf]
    const float  *ABS, *SCA;       // [nf]: the scalar opacities (OPT == nullptr)
    const float2 *OPT;             // [CELLS][nf] per-cell opacities, or nullptr
    float *MAP, *TAU;              // [nf][npix]
    float *COLDEN;                 // [npix] column density x LENGTH
};
hipError_t soc_launch_mapx(const SocGrid &G, const SocMapXArgs &A, hipStream_t st);
// the levels of the plain map (soc_map.hip: soc_maplevx_kernel, `maplevels 1`): the batch of SocMapXArgs, one plane per frequency and level
struct SocMapLXArgs : SocMapView {
    int   nf;                      // frequencies of the batch = row stride of EMIT and OPT
    int   f0, kf;                  // one launch: its first column and its columns (set by soc_launch_maplevx)
    const float  *EMIT;            // [CELLS][nf]
    const float  *ABS, *SCA;       // [nf]: the scalar opacities (OPT == nullptr)
    const float2 *OPT;             // [CELLS][nf] per-cell opacities, or nullptr
    float *MAPL;                   // [nf][LEVELS][npix]
};
hipError_t soc_launch_maplevx(const SocGrid &G, const SocMapLXArgs &A, hipStream_t st);
int soc_maplevx_width(int LEVELS);     // the most columns one launch takes
// polarisation maps (soc_map.hip): one launch of PolMapping (kernel_ASOC_map.c:974-994, :1164-1184, :1600-1620)
struct SocPolArgs {
    int   polstat;                 // -D POLSTAT: 0 = I, Q, U, column density; 1 = rT, rI, jT, jI; 3 = <B>, <B_LOS>, <B_POS>, tau
    int   polred, rho_weight;      // -D POLRED (p = |B| per cell), -D POL_RHO_WEIGHT
    int   LEVEL_THRESHOLD;
    int   NPIX_X, NPIX_Y;
    float p0;                      // -D p00
    float MAP_DX, ABS, SCA, LENGTH;
    float DIR[3], RA[3], DE[3], CENTRE[3];
    const float  *EMIT;
    const float2 *OPT;
    const float4 *B;               // [CELLS] (Bx, By, Bz, pad)
    float *MAP;                    // [4 * NPIX_Y * NPIX_X]
};
hipError_t soc_launch_polmap(const SocGrid &G, const SocPolArgs &A, bool abu, hipStream_t st);
// all-sky polarisation map (soc_map.hip): one launch of PolHealpixMapping (kernel_ASOC_map_H.c:576-597), -D POLSTAT=0
#define SOC_HPOL_MAXSTEPS (1 << 15)    // cell steps after which a ray is ended: on hierarchies the reference's walk can cycle for ever
struct SocHPolArgs {
    int   NSIDE, polred, LEVEL_THRESHOLD;
    int   INTERPOLATE;             // -D INTERPOLATE 0..3 (kernel_ASOC_map_H.c:646-733)
    float p0;                      // -D p00
    float MINLOS, MAXLOS;          // -D MINLOS, -D MAXLOS [root cells]
    float Y_SHEAR;                 // periodic in x and y, y shifted by this many root cells across the x faces (:800-826)
    float ABS, SCA, LENGTH;
    float INTOBS[3];
    const float  *EMIT;
    const float2 *OPT;
    const float4 *B;               // [CELLS] (Bx, By, Bz, pad)
    float *MAP;                    // [4 * 12 * NSIDE^2]
};
hipError_t soc_launch_hpolmap(const SocGrid &G, const SocHPolArgs &A, bool abu, hipStream_t st);
// per-level maps (soc_map.hip): one launch of the Mapping of kernel_ASOC_map_H.c (:380-398), `mapping nx ny dx 999`
#define SOC_MAPLEV_MAXSTEPS SOC_HPOL_MAXSTEPS   // the walk is that file's: the same end of a ray that cycles
struct SocMapLevArgs {
    int   NPIX_X, NPIX_Y;
    float MAP_DX, ABS, SCA;
    float DIR[3], RA[3], DE[3], CENTRE[3];
    float INTOBS[3];               // INTOBS[0] > -1e10: the longitude x latitude image seen from there
    const float  *EMIT;
    const float2 *OPT;
    float *MAP;                    // [LEVELS * NPIX_Y * NPIX_X]
};
hipError_t soc_launch_maplev(const SocGrid &G, const SocMapLevArgs &A, bool abu, hipStream_t st);
hipError_t soc_launch_pack_bfield(int cells, const float *Bx, const float *By, const float *Bz, float4 *B, hipStream_t st);
hipError_t soc_launch_pstau(const SocGrid &G, int no, const float4 *PSPOS, const float *DIR, float ABS, float SCA, const float2 *OPT, float LENGTH,
                            float *pscolden, float *pstau, hipStream_t st);

// stochastic-heating solver (soc_a2e.hip)
struct SocA2EArgs {
    int NE, NFREQ, npair, batch;
    const float *Iw;                 // integration weights, in (l,u,i) loop order
    const int   *pair_first;         // [npair] L1[l*NE+u]
    const int   *pair_last;          // [npair] L2[l*NE+u]
    const int   *pair_iw;            // [npair] offset of the pair's first weight in Iw
    const int   *pair_dst;           // [npair] (u*u-u)/2 + l
    const float *Tdown;              // [NE]
    const float *EA;                 // [NE*NFREQ]: transposed by soc_a2e_set_size (bin-major)
    const int   *Ibeg;               // [NFREQ]
    const float *AF;                 // [NFREQ]
    const float *AABS;               // [batch*NFREQ]
    float       *AEMIT;              // [batch*NFREQ]
    int          accumulate;         // 1: AEMIT += the emission of this size (the sum over the sizes stays on the device: soc_a2e_resident_*)
    // polarised emission (A2E.py:413-429), NULL without: PEMIT += W * the emission, W from the cell's minimum aligned size and these scalars
    float       *PEMIT;              // [batch*NFREQ]
    const float *AALG;               // [batch][2]: a_alg and log10(a_alg) of the cell
    float        p_size, p_next;     // ASIZE[isize]; ASIZE[isize+1], or 0 for the last size (no partial arm)
    float        p_lgsize, p_lgden;  // log10(ASIZE[isize]); log10(ASIZE[isize+1]) - log10(ASIZE[isize])
    float       *XX;                 // [batch*NE], NULL without: the clamped populations of the enthalpy levels (kernel_A2E.c:101-103)
};

struct SocEqTArgs {
    int batch, icell, CELLS, NFREQ, NIP;
    float FACTOR, kE, oplgkE, Emin;
    const float *FREQ, *KABS, *TTT, *ABS;
    float *T, *EMIT;
};

// all equilibrium sizes of a dust on the resident cells (soc_a2e_eqsizes_kernel): the per-size tables and the arrays it works on
struct SocEqSizesArgs {
    long long cells;
    int NFREQ, NIP, nsizes;
    int TC, stride;                  // cells per tile and the row stride of its absorptions in LDS: set by soc_launch_a2e_eqsizes
    float FACTOR, GD;
    const float *FREQ;               // [NFREQ]
    const float *AF, *KABS;          // [nsizes][NFREQ]
    const float *TTT;                // [nsizes][NIP]
    const float *Emin, *kE, *oplgkE; // [nsizes]
    const float *scale;              // [nsizes] GD * S_FRAC, formed in fp32
    const float *SFRAC, *SIZEA;      // [nsizes] (the polarised sum alone)
    const float *ABS;                // [cells*NFREQ]
    float       *SUM;                // [cells*NFREQ]
    float       *PSUM;               // [cells*NFREQ], NULL without polarised output
    const float *AALG;               // [cells][2]: a_alg and log10(a_alg) of the cell
    float       *TOUT;               // [nsizes][cells], NULL without: the temperature of every (size, cell) (A2E.py:506-522)
};

#define SOC_A2E_LDS (160 * 1024)     // bytes of LDS a DoSolve workgroup may take (the CU's)
// cells per workgroup, threads per workgroup and dynamic LDS bytes of DoSolve at this size; false: one cell does not fit (it needs out[2] bytes)
bool soc_a2e_shape(int NE, int NFREQ, int out[3]);
hipError_t soc_launch_a2e_dosolve(const SocA2EArgs &A, hipStream_t st);
hipError_t soc_launch_a2e_eqtemp(const SocEqTArgs &A, hipStream_t st);
// cells per tile and dynamic LDS bytes of the equilibrium-sizes kernel; false: the row of one cell does not fit (it needs out[1] bytes)
bool soc_a2e_eq_shape(int NFREQ, int nsizes, int out[2]);
hipError_t soc_launch_a2e_eqsizes(SocEqSizesArgs A, hipStream_t st);
hipError_t soc_launch_eqsolver(const SocEqTArgs &A, hipStream_t st);

// the multi-dust emission stage (soc_mabu.hip): split of the absorptions between the dust components, clip of the last channel
// in front of the stochastic solver, abundance-weighted sum of the emission.  RABS[NFREQ][NDUST] (double) must fit SOC_MABU_LDS.
#define SOC_MABU_LDS (64 * 1024)
hipError_t soc_launch_mabu_split(long long cells, int NFREQ, int NDUST, int idust, const float *ABS, const float *ABU, const double *RABS,
                                 float *PART, hipStream_t st);
hipError_t soc_launch_mabu_clip(long long cells, int NFREQ, float *PART, hipStream_t st);
hipError_t soc_launch_mabu_sum(long long cells, int NFREQ, int NDUST, int idust, const float *EM, const float *ABU, float *SUM, hipStream_t st);
// `polarisation`: PEM = EM * ipR_f(a_alg) of an equilibrium dust (AALG[cells][2]: a_alg and its log10; APOL[NA], TAB[NFREQ][NA] double),
// and PSUM = PSUM / (SUM + 1e-32)
hipError_t soc_launch_mabu_poleq(long long cells, int NFREQ, int NA, const float *EM, const float *AALG, const double *APOL, const double *TAB,
                                 float *PEM, hipStream_t st);
hipError_t soc_launch_mabu_ratio(long long cells, int NFREQ, const float *SUM, float *PSUM, hipStream_t st);

// the resident emission of the re-emission iterations (soc_reemit.hip): ROWS[n][NFREQ] <-> cells [c0, c0 + n) of ET[NFREQ][CELLS], and
// EMIT[c] = COL[c] * (COEFF[level(c)] * DENS[c]), 0 where DENS[c] < 1e-10 (COEFF: LEVELS host floats, COL: a row of ET)
hipError_t soc_launch_reemit_to_columns(long long n, int NFREQ, long long CELLS, long long c0, const float *ROWS, float *ET, hipStream_t st);
hipError_t soc_launch_reemit_to_rows(long long n, int NFREQ, long long CELLS, long long c0, const float *ET, float *ROWS, hipStream_t st);
hipError_t soc_launch_reemit_column(const SocGrid &G, const float *COEFF, const float *COL, float *EMIT, hipStream_t st);
// the change of the resident emission between two iterations (soc_reemit.hip): L[c] = (sum_f (double)ET[f][c] * W[f]) * (double)(COEFF[level]
// * DENS[c]) replaces LP[c]; STATS = sum |L - LP|, sum L, sum LP, max |L - LP| / max(L, LP); BAD += the live cells whose L is negative or
// not finite.  PART: soc_emitted_change_blocks(CELLS) x 4 doubles of scratch.  W, LP, PART, STATS, BAD on the device, COEFF on the host
long long soc_emitted_change_blocks(long long CELLS);
hipError_t soc_launch_emitted_change(const SocGrid &G, int NFREQ, const float *COEFF, const float *ET, const double *W, double *LP, double *PART,
                                     double *STATS, unsigned long long *BAD, hipStream_t st);
// the resident absorptions, their mirror image (soc_reemit.hip): ROW[c] += TALLY[c] over CELLS cells, and the same tile walk from
// AT[NFREQ][CELLS] to ROWS[n][NFREQ] with ROWS[c][f] = AT[f][c0+c] * (K[level] / DENS), -1e20 where DENS <= nnnlimit (K: LEVELS host
// floats; NULL: the bits as they are)
hipError_t soc_launch_absorbed_add(long long CELLS, const float *TALLY, float *ROW, hipStream_t st);
hipError_t soc_launch_absorbed_to_rows(const SocGrid &G, long long n, int NFREQ, long long c0, const float *AT, float *ROWS, const float *K,
                                       float nnnlimit, hipStream_t st);

// the library method (soc_library.hip).  The reference columns of cell `c` are ABS[c * stride + c0 | c1 | c2].
struct SocLibSolve {
    long long    n;                  // cells
    int          N, nout;            // bins per axis; emission columns of E and of a row of EMI
    float        I0, dI0;
    const float *I1, *dI1;           // [N]
    const float *I2, *dI2;           // [N*N]
    const float *X, *Y, *Z;          // [N^3]
    const float *E0;                 // [N^3] the first stored emission value of every bin (> 1e31: the bin is empty)
    const float *E;                  // [N^3][nout]
    const float *ABS;
    long long    stride;
    int          c0, c1, c2;
    float       *EMI;                // [n][nout]
    int         *miss;               // [n] the cells without an answer, in the order they were found
    unsigned long long *nmiss;       // their count (0 before the launch)
};
struct SocLibBuild {
    long long    cells;
    int          N;
    const float *ABS;
    long long    stride;
    int          c0, c1, c2;
    float        I0, dI0;
    const float *I1, *dI1, *I2, *dI2;
};
hipError_t soc_launch_library_solve(const SocLibSolve &A, hipStream_t st);
// level 0 | 1 | 2: TAB = 1 | N | N^2 minima, maxima and counts (keys 0xffffffff, 0, 0 before the launch) of axis `level`
hipError_t soc_launch_library_range(const SocLibBuild &A, int level, unsigned *TAB, hipStream_t st);
// BEST[N^3] all ones before the launch; IND, XX, YY, ZZ [N^3]
hipError_t soc_launch_library_pick(const SocLibBuild &A, unsigned long long *BEST, int *IND, float *XX, float *YY, float *ZZ, hipStream_t st);

// the library method for several dust components (soc_mabu_library.hip): a library per dust, indexed by that dust's share of the
// absorptions at the three reference frequencies; one kernel looks every dust up and forms the abundance-weighted sum
#define SOC_MABU_LIB_DUSTS 32        // the width of the miss mask
// the tables of one resident library: what a look-up reads of it
struct SocLibTables {
    int          N, nout;            // bins per axis; emission columns of E
    float        I0, dI0;
    const float *I1, *dI1;           // [N]
    const float *I2, *dI2;           // [N*N]
    const float *X, *Y, *Z;          // [N^3]
    const float *E0;                 // [N^3] the first stored emission value of every bin (> 1e31: the bin is empty)
    const float *E;                  // [N^3][nout]
};
struct SocMabuLib {
    long long    n;                  // cells
    int          NDUST, nout;        // dust components; emission columns of every library's E and of a row of SUM
    const float *ABS3;               // [n][3] the absorptions at the reference frequencies
    const float *ABU;                // [n][NDUST]
    const double *RABS3;             // [3][NDUST] relative cross sections at the reference frequencies
    const SocLibTables *LIB;         // [NDUST], in device memory
    float       *SUM;                // [n][nout]
    unsigned    *MISS;               // [n] bit d: dust d had no answer
};
hipError_t soc_launch_mabu_library(const SocMabuLib &A, hipStream_t st);
// OUT[n][NFREQ] = rows IDX[n] of EM[cells][NFREQ] (the caller checks the indices)
hipError_t soc_launch_mabu_gather_rows(long long n, int NFREQ, const float *EM, const int *IDX, float *OUT, hipStream_t st);

// Shape of the brick sweep; 0 = the built-in choice for the grid (measured).  Set per context with
// soc_set_tuning (include/soc_hip.h); the parity tests use small CAP / HS values to exercise brick boundaries.
struct SocBrickTune {
    int T, P, KCAP, FTH, CTH, CAP, TAIL, POP, HS;
    int global_tree;           // hierarchies: the walk that reads the hierarchy from global memory, also where brick-local ones apply
    int park;                  // brick-local hierarchies: brick queues shorter than this (and than the mean queue) wait for more packets (0 = built-in 4096, 1 = never)
    int slow_every;            // brick-local hierarchies, test knob: every n-th step below the root grid goes through the slow-step queue
    int nolean;                // keep the general SimRAM_PB kernel for background-only sweeps
    int oversub;               // experiment: background work items beyond 8*AREA are not clipped
    int verbose;
    int abu_local;             // brick-local hierarchies: launches with per-cell opacities (WITH_ABU) take the brick-local walk too (0 = built-in choice: off)
    int partition;             // brick-local hierarchies: how the root grid is cut into bricks (soc_lbricks.h).  0 = built-in choice: of the tiles and the slabs the
                               // partition with the smaller total face area; 1 = the tiles alone (16^3 root cells, halved); 2 = as 0
    int float_local;           // hierarchies with Index() in float (NX <= DIMLIM) take the brick-local walk too, in its float form (0 = built-in choice: off)
};

// KIND of a launch's source: 0 SimRAM_PB, 1 SimRAM_HP, 2 SimRAM_CL
static inline int soc_source_kind(int source) { return (source == SOC_SOURCE_CL) ? 2 : (source == SOC_SOURCE_HP) ? 1 : 0; }

// the grid's kernels: octree for hierarchies, Index() in double beyond DIMLIM (kernel_ASOC_aux.c:25-37)
static inline SocVariant soc_grid_variant(const SocGrid &G, bool abu = false, int wint = 0)
{
    SocVariant V;
    V.octree = G.LEVELS > 1;
    V.dbl = G.NX > ((G.LEVELS < 3) ? 399 : 100);
    V.abu = abu;
    V.wint = wint;
    return V;
}

// Grids on which the brick sweep walks brick-local hierarchies (soc_brick.hip, soc_ltree.h): 2-8 levels with Index() in double,
// cell coordinates within 24 bits and root-cell numbers from 24-bit multiplies (SOC_MAD24) -- unless
// soc_set_tuning("global_tree", 1) asks for the sweep that reads the hierarchy from global memory.  Per-cell opacities (WITH_ABU): only
// with soc_set_tuning("abu_local", 1), and not with with_int 2 (the abundance kernels are built for WINT 0, 1 and 3); launches with the
// XAB tally of WITH_ALI stay off it too (plan_sweep in soc_brick.hip, lt_capable in soc_capi.hip).  Without the key such launches are
// routed as they always were: the sweep that reads the hierarchy and OPT from global memory.
// Hierarchies with Index() in float (!V.dbl): only with soc_set_tuning("float_local", 1) -- the float form of soc_ltree.h -- and only with
// scalar opacities (no kernel combines the float form with per-cell opacities); without the key, and with per-cell opacities, they are
// routed as they always were.  On a grid with Index() in double the key changes nothing.
static inline bool soc_brick_local(const SocGrid &G, const SocVariant &V, const SocBrickTune &tune)
{
    const int n = std::max(G.NX, std::max(G.NY, G.NZ));
    return V.octree && (V.dbl || (tune.float_local && !V.abu)) && (!V.abu || (tune.abu_local && V.wint != 2)) && !tune.global_tree && G.LEVELS <= 8 && ((long long)n << (G.LEVELS - 1)) < (1LL << 24) && n < 4096;
}

// Single-level (Cartesian) grids on which the scattered-light launches run as a sweep of rays (soc_brick.hip: the CART arm of
// soc_lbrick_walk, bricks from soc_cbricks_build): scalar opacities, root-cell numbers from 24-bit multiplies (SOC_MAD24: rows of
// root cells below 2^23).  A sibling of soc_brick_local: absorption launches on such grids keep the Cartesian sweep (form 1).
static inline bool soc_brick_cart(const SocGrid &G, const SocVariant &V)
{
    const int n = std::max(G.NX, std::max(G.NY, G.NZ));
    return !V.octree && !V.abu && G.LEVELS == 1 && n < 4096 && ((long long)G.NY * G.NZ) < (1LL << 23);
}
// Rays on single-level grids: cells along the edge of a brick, measured (profiles/sca_cartesian_lines.json; rays
// against the direct kernel, background launches): 128^3 -- 8: 0.13x, 16: 0.29x, 24: 0.23x; 256^3 -- 8: 0.09x, 16: 0.45x, 24: 0.66x,
// 32: 0.57x; 512^3 -- 16: 0.46x, 24: 0.97x, 32: 0.77x.  A sweep needs as many passes as its longest chain of brick visits, and a pass
// costs three kernel launches: larger bricks, fewer passes -- until a brick's 4 B per cell leave one workgroup per CU (32^3 = 128 KB).
// 24^3 cells are 54 KB of LDS (two workgroups per CU), 16^3 are 16 KB.
#define SOC_CART_BRICK_EDGE 16                               /* grids below SOC_CART_BRICK_WIDE cells along their longest edge */
#define SOC_CART_BRICK_EDGE_WIDE 24
#define SOC_CART_BRICK_WIDE 256
static inline int soc_cart_default_edge(const SocGrid &G)
{
    return (std::max(G.NX, std::max(G.NY, G.NZ)) >= SOC_CART_BRICK_WIDE) ? SOC_CART_BRICK_EDGE_WIDE : SOC_CART_BRICK_EDGE;
}
// cells along the edge of such a brick: the largest cube within `cells` (soc_set_tuning("brick_cells"))
static inline int soc_cart_edge(int cells)
{
    int e = 1;
    while ((long long)(e + 1) * (e + 1) * (e + 1) <= cells) e++;
    return e;
}

// What a brick sweep runs, decided before it runs (soc_brick.hip: plan_sweep, completed by plan_kernel once the launches are packed).
// Form 0 describes a launch of the direct kernels (soc_capi.hip: run_direct).
struct SocSweepPlan {
    int  form;                 // 0 direct kernel, 1 Cartesian sweep, 2 sweep of a hierarchy in global memory, 3 brick-local sweep
                               // (form 3 with octree == false: the sweep of rays on a Cartesian grid, whose bricks hold root cells only)
    int  kind;                 // the KIND template argument: 0 SimRAM_PB, 1 _HP, 2 _CL, 3 background packets only, 4 several (brick-local); rays: 0
    int  wint;                 // the WINT template argument: 0, 1, 2 (brick-local), 3 the INT-only form of the brick-local walk
    bool octree, dbl, abu;     // the grid's kernels (dbl: octree and Index() in double)
    bool ali;                  // brick-local: every launch a SimRAM_CL one with the XAB tally (WITH_ALI)
    bool rays, hpx, hpsky;     // the scattered-light sweep of rays; its image a Healpix map seen from a position; SimRAM_HP launches in it
    bool roi;                  // brick-local: the record of packets entering ROI (a fourth event queue per launch)
    int  capl;                 // brick-local: cells per brick (rays on a Cartesian grid: the cube of the brick's edge)
    bool tiles;                // brick-local: the bricks are the tiles of soc_lbricks.h alone (soc_set_tuning("brick_partition", 1))
    // SocBrickArgs: the form's defaults with soc_set_tuning applied (CAP: leaves per brick of a hierarchy in global memory)
    int  T, P, KCAP, FTH, CTH, CAP, TAIL, PARK, EQ, slow_every;
    size_t lds;                // dynamic LDS of the pass kernel
};

// the plan of the grid's own kernels: the direct ones (form 0), the Cartesian and global-tree sweeps
static inline SocSweepPlan soc_grid_plan(int form, int kind, const SocVariant &V)
{
    SocSweepPlan p{};
    p.form = form;
    p.kind = kind;
    p.wint = V.wint ? 1 : 0;
    p.octree = V.octree;
    p.dbl = V.octree && V.dbl;
    p.abu = V.abu;
    return p;
}

// The compiled absorption kernel a plan runs, as soc_last_variant reports it (bit layout: include/soc_hip.h, SOC_VAR_*)
#define SOC_VAR_HEALPIX (1 << 12)   // sweeps of rays: the image was a Healpix map seen from a position
#define SOC_VAR_HPSKY   (1 << 13)   // sweeps of rays: the sweep held a SimRAM_HP launch (the Healpix sky as the source)
static inline int soc_variant_code(const SocSweepPlan &p)
{
    return p.form | (p.kind << 2) | (p.wint << 5) | (p.octree ? 1 << 7 : 0) | (p.dbl ? 1 << 8 : 0) | (p.abu ? 1 << 9 : 0) | (p.ali ? 1 << 10 : 0)
           | (p.rays ? 1 << 11 : 0) | (p.hpx ? SOC_VAR_HEALPIX : 0) | (p.hpsky ? SOC_VAR_HPSKY : 0);
}

// The packet-splitting kernels (soc_split.hip): the instance <OCT, DBL, ABU, WINT> a launch runs, as the integer both launch wrappers
// switch on -- octree 8, Index() in double 4 (cleared on Cartesian grids: Index() touches no double arithmetic at level 0), per-cell
// opacities 2, the INT tally 1 -- and the same instance as soc_last_variant reports it: form 0, kind 0 SimBgSplit / 1 SimHpSplit, the
// key's bits in their usual places, and bit 14
#define SOC_VAR_SPLIT   (1 << 14)   // a launch of the packet-splitting kernels
static inline int soc_split_key(const SocVariant &V)
{
    return (V.octree ? 8 : 0) | ((V.octree && V.dbl) ? 4 : 0) | (V.abu ? 2 : 0) | (V.wint ? 1 : 0);
}
static inline int soc_split_variant_code(int kind, const SocVariant &V)
{
    const int key = soc_split_key(V);
    SocSweepPlan p{};
    p.kind = kind;
    p.wint = key & 1;
    p.octree = (key & 8) != 0;
    p.dbl = (key & 4) != 0;
    p.abu = (key & 2) != 0;
    return soc_variant_code(p) | SOC_VAR_SPLIT;
}

// The direct scattered-light kernel (soc_sca.hip): the instance <OCT, DBL, ABU, KIND> a launch runs, as soc_last_variant reports it --
// form 0, kind the SOC_SCA_* value, octree, Index() in double and per-cell opacities as sca_dispatch takes them from the variant
// (dbl is not cleared on a Cartesian grid: NX > 399 there runs the <0, 1, *, *> instances), and bit 15
#define SOC_VAR_SCA     (1 << 15)   // a launch of the direct scattered-light kernel
static inline int soc_sca_variant_code(int kind, const SocVariant &V)
{
    SocSweepPlan p{};
    p.kind = kind;
    p.octree = V.octree != 0;
    p.dbl = V.dbl != 0;
    p.abu = V.abu != 0;
    return soc_variant_code(p) | SOC_VAR_SCA;
}

// What a brick sweep reports: passes (0 when no launch had work items), form (0 unless the sweep ran), variant (untouched when no kernel ran)
struct SocSweepResult {
    int passes = 0, form = 0, variant = -1;
};

// brick-sweep execution (soc_brick.hip): LDS-resident tallies, packets sorted by brick; sca: the launches are ones of the
// scattered-light kernels (rays, soc_sca_events).  SocSweepState: the packet records, queues and bricks that a handle's sweeps keep
// on the device, every one an owning DevBuf; soc_sweep_delete frees them.
struct SocSweepState;
SocSweepState *soc_sweep_new();
void soc_sweep_delete(SocSweepState *sw);
void soc_sweep_invalidate(SocSweepState *sw);      // the grid changed: its bricks are rebuilt at the next sweep (nothing is freed)
hipError_t soc_brick_run_pb(SocSweepState &sw, const SocGrid &G, const SocSim *S, int nlaunch, const SocVariant &V, int LB,
                            const SocBrickTune &tune, hipStream_t st, SocSweepResult *res, const struct SocSca *sca = nullptr);

#endif
