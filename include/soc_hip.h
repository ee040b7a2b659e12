/*
 * soc_hip.h -- C ABI of libsoc_hip.so, the MI355X (gfx950) engine for SOC's photon-packet path.
 *
 * The reference has no FFI layer: its host scripts drive OpenCL kernels through pyopencl
 * (cl.Buffer / enqueue_copy / kernel(queue,[GLOBAL],[LOCAL],args...)).  Each entry point
 * below replaces one group of those calls; file:line citations are into /root/reference.
 * Conventions:
 *   - every function returns 0 on success, a negative code on error; the message is
 *     available from soc_last_error().  Nothing throws or exits.
 *   - host pointers are only read/written during the call; the library owns all device
 *     memory behind the handle (NULL is allowed for unused optional arrays).
 *   - scalars have the types pyopencl passes (set_scalar_arg_dtypes, ASOC.py:846-858):
 *     int32 / float32.  SEED, BG, TW are float32 at the boundary.
 *   - a handle is bound to one GPU and is not thread-safe; launches are asynchronous on the
 *     handle's stream; soc_read_tally() and soc_sync() synchronise.
 *   - the scratch of the brick sweep (packet queues, the brick tables of the current grid) is kept per GPU, shared by
 *     the handles of that GPU and freed when the last of them is destroyed: calls on DIFFERENT handles of one GPU must
 *     not overlap in time either (one process drives one GPU from one thread -- the layout of soc_amd/dist.py).
 */
#ifndef SOC_HIP_H
#define SOC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct soc_ctx soc_ctx;

#define SOC_OK            0
#define SOC_ERR_ARG      -1   /* invalid argument / inconsistent model        */
#define SOC_ERR_STATE    -2   /* call order: grid / tables not set yet         */
#define SOC_ERR_HIP      -3   /* HIP runtime error (message has the details)   */

/* tallies selectable in soc_zero / soc_read_tally / soc_tally_ptr */
#define SOC_TALLY_TABS    0   /* absorbed energy integrated over frequency (TABS, kernel arg 15) */
#define SOC_TALLY_INT     1   /* per-frequency absorptions (INT, kernel arg 20)                  */
#define SOC_TALLY_XAB     2   /* WITH_ALI: absorptions inside the emitting cell (XAB, kernel arg 19) */
#define SOC_TALLY_INTX    3   /* SAVE_INTENSITY==2: sum of delta*DIR.x per cell (INTX, kernel arg 21); soc_zero(1) clears  */
#define SOC_TALLY_INTY    4   /*   INT and these three, as ZeroAMC tag 1 does (kernel_ASOC_aux.c:676-681)                   */
#define SOC_TALLY_INTZ    5

/* replaces ASOC_aux.py:1188-1256 opencl_init(): create a context on GPU `device` */
int  soc_create(int device, soc_ctx **out);
void soc_destroy(soc_ctx *ctx);
const char *soc_last_error(const soc_ctx *ctx);   /* ctx may be NULL: last creation error */
const char *soc_version(void);
/* bytes of device memory the library's handles hold at the moment, all handles of the process together: what they allocated themselves.
 * Memory of the caller (soc_bind_tally, soc_sca_bind_out) and the scratch of the brick sweep do not count.  A counter on the host:
 * it reads no device state.  After the last soc_destroy it is back where it was before the first soc_create. */
int64_t soc_device_bytes(void);

/* run on an externally owned HIP stream (e.g. the stream of the caller's framework); NULL = own stream.
 * NOTE: a framework's "default stream" is the null handle too -- pass a stream the framework created
 * (torch.cuda.Stream().cuda_stream) and make it the current one, or the collectives of the framework
 * are not ordered with the kernels (soc_amd/dist.py does that). */
int soc_set_stream(soc_ctx *ctx, void *hip_stream);

/* replaces the -D NX,NY,NZ,LEVELS,CELLS macros (ASOC.py:344-362), the LCELLS/OFF/DENS
 * uploads (ASOC.py:524-539) and the Parents kernel launch (ASOC.py:585,
 * kernel_ASOC_aux.c:688-718).  DENS is the concatenated hierarchy as read_cloud() returns
 * it (ASOC_aux.py:716-803): value > 0 leaf density, value <= 0 link to 8 children.
 * The hierarchy is validated (links in range, octets aligned) before anything is uploaded. */
int soc_set_grid(soc_ctx *ctx, int NX, int NY, int NZ, int LEVELS, const int32_t *LCELLS, const float *DENS);

/* feature switches the reference compiles in with -D (ASOC.py:344-362):
 *   with_int     : 1 = SAVE_INTENSITY==1 or NOABSORBED==0 -> INT tally is updated; 2 = SAVE_INTENSITY==2 -> INT and the
 *                  vector sums INTX, INTY, INTZ (kernel_ASOC.c:604-612, :724-732; needs soc_set_grid first; such launches
 *                  run on the direct kernels)
 *   ps_method    : PS_METHOD 0,1,2,4,5 (3 does not compile in the reference)
 *   use_emweight : USE_EMWEIGHT 0, 1, or 2 = cells listed by soc_set_emindex (SimRAM_CL)     */
int soc_set_features(soc_ctx *ctx, int with_int, int ps_method, int use_emweight);

/* replaces -D MIRROR=%d (ASOC.py:319-321,352; ASOCS.py:119-122): reflecting model faces, bits
 * x,X,y,Y,z,Z = 1,2,4,8,16,32 (lower/upper face per axis); 0 = none (default) */
int soc_set_mirror(soc_ctx *ctx, int mask);

/* how launches are executed (no counterpart in the reference; results are the same packets):
 *   mode 0  direct: one lane per work item, one global float atomic per tally event
 *   mode 1  brick sweep (SimRAM_PB): packets sorted by brick, tallies accumulated in LDS and flushed per
 *           brick; a brick is 2^brick_log2 root cells per edge on Cartesian grids, a set of <= 8192
 *           neighbouring leaves on hierarchies (built at the first sweep after soc_set_grid)
 *   mode -1 automatic (default): brick sweep where it pays -- Cartesian grids from 65536 work items on,
 *           hierarchies for launches deferred by soc_batch_begin (two or more per sweep) -- direct
 *           otherwise (reflecting faces, region-of-interest records, SOURCE 3)                     */
int soc_set_exec(soc_ctx *ctx, int mode, int brick_log2);

/* Shape of the brick sweep (no counterpart in the reference; results are the same packets whatever the values).
 * value 0 = the built-in choice for the grid.  Names: "threads" (workgroup size of the walk, 64..512; ..1024 on brick-local
 * hierarchies), "chunk" (packets per workgroup, <= 4096; <= 32768 on brick-local hierarchies), "steps_per_visit" (cell steps
 * before a packet goes back to its queue), "swap_lanes" (lanes of a wave that must wait before the packet swap runs),
 * "climb_lanes" (the same for the deferred Index() of the global-tree form), "brick_cells" (cells per brick on hierarchies,
 * <= 36864; rays on single-level grids: bricks of the largest cube within), "brick_partition" (brick-local hierarchies: how the root
 * grid is cut into the boxes of the bricks.  0, the built-in choice, and 2: of two partitions -- tiles of 16^3 root cells halved until
 * they fit, and slabs / columns / boxes sized by the cells they hold -- the one whose boxes have the smaller total face area;
 * 1: the tiles alone.  A change rebuilds the handle's bricks at its next sweep, as a change of "brick_cells" does), "tail_lanes", "park_below" (hierarchies: brick queues shorter than this and than the mean wait a pass; 1 = never), "population" (packets in flight), "hash_slots" (per-workgroup
 * arrival table, power of two), "general_kernel" (1: no background-only kernel), "global_tree" (1: hierarchies are walked in
 * global memory also where the brick-local form applies), "slow_every" (test knob of that form),
 * "oversubscribe", "verbose", "abu_local" (1: launches with per-cell opacities -- soc_set_opt, soc_set_optical_abu -- take the
 * brick-local form of a hierarchy that has one too, the opacities of a brick's cells in LDS; 0, the built-in choice: they are routed as
 * without the key, through the sweep that reads the hierarchy and OPT from global memory.  Not with with_int 2 or soc_set_ali, which
 * keep today's paths.  Launches deferred between two soc_set_opt / soc_set_optical_abu calls then share one copy of the opacities,
 * and a batch holds at most 16 such copies), "float_local" (1: hierarchies on which Index() runs in float -- NX <= 100, or NX <= 399
 * with two levels -- take the brick-local form too, in its float form: absorption launches, also with mirror, with_int 2, ROI records
 * and ALI, and the sweep of rays of the scattered-light launches; 0, the built-in choice: such grids are routed as without the key.
 * Launches with per-cell opacities on such a grid, and every launch on a grid with Index() in double, are routed the same either way). */
int soc_set_tuning(soc_ctx *ctx, const char *name, int value);

/* replaces the per-frequency uploads of ABS, SCA (ASOC.py:1171-1175); ndust must be 1
 * (the host sums the species, ASOC.py:1166-1170) */
int soc_set_optical(soc_ctx *ctx, const float *ABS, const float *SCA, int ndust);

/* replaces the OPT upload for abundance runs (WITH_ABU, ASOC.py:1146-1160):
 * OPT[CELLS][2] = (abs, sca) per cell; NULL switches back to scalar ABS/SCA */
int soc_set_opt(soc_ctx *ctx, const float *OPT);

/* The same OPT without the 8*CELLS-byte upload per frequency (ASOC.py:1146-1160, "0.43 s / 2.5 s" :1177): the
 * abundances go to the device once -- ABU[CELLS][NDUST], or with single != 0 ABU[CELLS] for two species with
 * abundances ABU and 1-ABU (USER.SINGLE_ABU, :1148-1153); ABU = NULL forgets them -- and for every frequency
 * soc_set_optical_abu(AFABS[NDUST], AFSCA[NDUST]) computes OPT = sum ABU * AF on the device, in the order and
 * precision of the numpy expressions (bit-identical to the host's OPT).  soc_read_opt copies OPT back. */
int soc_set_abundances(soc_ctx *ctx, int NDUST, int single, const float *ABU);
int soc_set_optical_abu(soc_ctx *ctx, const float *AFABS, const float *AFSCA, int ndust);
int soc_read_opt(soc_ctx *ctx, float *OPT);

/* -D OPT_IS_HALF (ini key `optishalf`; kernel_ASOC_aux.c:12-18, ASOC.py:1158-1159): the reference stores OPT as fp16.
 * on != 0: every later soc_set_opt / soc_set_optical_abu rounds OPT to fp16 (nearest even) -- the kernels then compute
 * with exactly the values vload_half would give them. */
int soc_set_opt_half(soc_ctx *ctx, int on);

/* replaces the DSC/CSC row uploads (ASOC.py:1234-1243, ASOCS.py:625-626); DSC may be NULL
 * (unused by the absorption kernels, required by soc_sca_sim_ps/pb); BINS = USER.DSC_BINS */
int soc_set_scatter_table(soc_ctx *ctx, const float *DSC, const float *CSC, int BINS);

/* -D WITH_MSF (ASOC.py:132-138, :1239-1243; kernel_ASOC.c:777-795, :1654-1668): one scattering function per dust species,
 * DSC[NDUST][BINS] and CSC[NDUST][BINS]; NDUST == 1 is soc_set_scatter_table.  With NDUST > 1 a launch needs the
 * abundances of the same NDUST species (soc_set_abundances, not the one-abundance form) and this frequency's
 * soc_set_optical_abu -- whose AFSCA are the per-species SCA the kernels draw the scatterer with -- and is not deferred. */
int soc_set_scatter_tables(soc_ctx *ctx, int NDUST, const float *DSC, const float *CSC, int BINS);

/* -D STEP_WEIGHT / SW_A / SW_B (ASOC.py:348,357; kernel_ASOC.c:516-535, :752-763, :941-955, :1444-1462, :1625-1640):
 * free paths from p(t) = A*exp(-A*t) (mode 1) or B*A*exp(-A*t) + (1-B)*2A*exp(-2A*t) (mode 2) with the packet weight
 * corrected; mode <= 0 switches the weighting off.  The arguments are the VALUES OF THE -D MACROS; the reference's host
 * fills them from the ini key `stepweight a b c` as STEP_WEIGHT=int(c), SW_A=int(a), SW_B=b (ASOC.py:357). */
int soc_set_step_weight(soc_ctx *ctx, int mode, float SW_A, float SW_B);

/* replaces the EMIT / EMWEI uploads (ASOC.py:1276, 1291); arrays of CELLS floats */
int soc_set_emission(soc_ctx *ctx, const float *EMIT, const float *EMWEI);

/* replaces the EMINDEX upload of the USE_EMWEIGHT==2 loop (ASOC.py:1809-1840): EMINDEX[CELLS], the cells to
 * emit 100 packets from in the next soc_sim_cl launch, terminated by -1 */
int soc_set_emindex(soc_ctx *ctx, const int32_t *EMINDEX);

/* replaces -D WITH_ALI=1 (ASOC.py:344): what a cell absorbs of its own emission is tallied in XAB
 * (SOC_TALLY_XAB) instead of TABS (kernel_ASOC.c:1486-1491); soc_zero(ctx, 0) clears both */
int soc_set_ali(soc_ctx *ctx, int with_ali);

/* replaces ZeroAMC (kernel_ASOC_aux.c:657-683; ASOC.py:1115,1183): tag 0 clears TABS,
 * tag 1 clears INT */
int soc_zero(soc_ctx *ctx, int tag);

/* replaces the kernel_ram_pb launch (ASOC.py:1360-1372 -> SimRAM_PB, kernel_ASOC.c:15-52).
 * SOURCE 0 = point sources, 1 = isotropic background.  PSPOS holds 4 floats per source
 * (cl float3).  GLOBAL is the logical launch size; this call executes the logical work
 * items [gid_first, gid_first+gid_count) so that several GPUs can share one launch with
 * exactly the streams a single device would use (get_global_id -> logical id). */
int soc_sim_pb(soc_ctx *ctx, int SOURCE, int PACKETS, int BATCH, float SEED, float BG, float TW,
               const float *PSPOS, const float *PS, int NO_PS,
               const int32_t *XPS_NSIDE, const int32_t *XPS_SIDE, const float *XPS_AREA,
               int GLOBAL, int gid_first, int gid_count);

/* replaces the kernel_ram_cl launch (ASOC.py:1308-1316, 1847 -> SimRAM_CL,
 * kernel_ASOC.c:1223-1256); uses EMIT/EMWEI from soc_set_emission().  Executed by the direct kernel, or -- with at
 * least 262144 work items that own a cell (GLOBAL ~ CELLS), USE_EMWEIGHT 0/1, no ALI, no roisave -- by the brick sweep;
 * deferred inside soc_batch_begin/end with its own copy of EMIT and EMWEI */
int soc_sim_cl(soc_ctx *ctx, int SOURCE, int PACKETS, int BATCH, float SEED, float TW,
               int GLOBAL, int gid_first, int gid_count);

/* Deferred execution of consecutive soc_sim_pb launches (no counterpart in the reference, which
 * runs one kernel per frequency and waits for it, ASOC.py:1360-1461).  Between soc_batch_begin and
 * soc_batch_end a launch that qualifies for the brick sweep and runs without the per-frequency INT
 * tally is recorded with a snapshot of its inputs (ABS, SCA or the per-cell OPT, scattering table,
 * BG, TW, seed, sources) and executed together with up to max_launches-1 others (0 = default = at most: 16;
 * on Cartesian grids 2.7e6 packets are in flight at a time and the later launches' work items are admitted as earlier
 * ones finish): the same packets, the same per-launch RNG streams, the same tallies -- more packets in
 * flight per pass.  Any other call that reads or changes engine state executes what is pending
 * first; launches that do not qualify run immediately as always. */
int soc_batch_begin(soc_ctx *ctx, int max_launches);
int soc_batch_end(soc_ctx *ctx);
/* The same for runs that keep the per-frequency INT tally (the absorbed file, ASOC.py:1482-1498): every deferred
 * launch gets its own, zeroed INT tally instead of the shared one (TABS stays shared).  At most max_launches (<= 16)
 * launches per batch; where the next launch cannot share the pending launches' sweep (another kind), they run first, as in
 * soc_batch_begin, and their INT tallies stay readable.  After soc_batch_end, soc_batch_read_int(k) copies the INT tally of
 * the k-th launch of the batch (n = CELLS).  Replaces K x [kernel launch + enqueue_copy(INT)] by K launches + K copies. */
int soc_batch_begin_int(soc_ctx *ctx, int max_launches);
/* The launches of ONE frequency that keep the INT tally (the source blocks of ASOC.py:1028-1545 at one IFREQ: point sources,
 * background, diffuse emission): deferred until soc_batch_end like soc_batch_begin's, all tallying into the handle's INT buffer
 * (soc_zero(ctx, 1) before, soc_read_tally(ctx, 1) after), so that they share brick sweeps -- and, where the walk keeps tallies
 * in LDS per workgroup, the same brick queues.  Replaces the per-launch enqueue + finish() + enqueue_copy(INT) of ASOC.py:1360-1372,
 * :1461, :1482-1498 for the launches of one frequency. */
int soc_batch_begin_shared_int(soc_ctx *ctx, int max_launches);
/* Several frequencies in one sweep, each with its own INT tally: as soc_batch_begin_int, but the launches between two
 * soc_batch_next_int calls -- the source blocks of ONE frequency -- share a tally (soc_batch_read_int(k) reads the k-th group's).
 * On brick-local hierarchies the brick queues are per group, so a workgroup's LDS tallies belong to one frequency; point-source,
 * background and cell-emission launches mix freely.  At most max_groups groups (0: 128) until soc_batch_end. */
int soc_batch_begin_int_groups(soc_ctx *ctx, int max_groups);
int soc_batch_next_int(soc_ctx *ctx);
int soc_batch_read_int(soc_ctx *ctx, int k, float *out, long n);

/* ---- region of interest of nested runs (ini keys roi, roisave, roiload, roipac, roinside) ---- */

/* replaces -D WITH_ROI_SAVE -D ROI_STEP -D ROI_NSIDE and ROI_buf / ROI_SAVE_buf (ASOC.py:346,927-944): from now on
 * soc_sim_pb and soc_sim_cl add every packet that steps into ROI = [x0,x1,y0,y1,z0,z1] (root cells, inclusive) to a
 * record [surface element, Healpix pixel of its direction] (kernel_ASOC.c:547-562,615-642, 1436-1535; InRoi
 * kernel_ASOC_aux.c:1031-1048), ROI_STEP elements per root-cell edge, NSIDE = ROI_NSIDE, RING order.
 * The record is zeroed here; ROI = NULL turns recording off.  Direct kernel only (the brick sweep stands aside). */
int soc_set_roi_save(soc_ctx *ctx, const int32_t *ROI, int ROI_STEP, int ROI_NSIDE);
/* replaces enqueue_copy(ROI_SAVE_buf, zeros) per frequency (ASOC.py:1301-1302) */
int soc_roi_zero(soc_ctx *ctx);
/* replaces enqueue_copy(tmp, ROI_SAVE_buf) (ASOC.py:1468-1471); n = (nx*ny + ny*nz + nz*nx) * 12 * ROI_NSIDE^2 with
 * n? = (ROI[2?+1] - ROI[2?] + 1) * ROI_STEP */
int soc_roi_read(soc_ctx *ctx, float *out, long n);
/* replaces -D WITH_ROI_LOAD and ROI_DIM_buf / ROI_LOAD_buf (ASOC.py:909-925,1419-1421): the record of one frequency,
 * LOAD[nelem, 12*ROI_NSIDE^2] photons (already scaled by the host) with nelem = DIM[0]*DIM[1] + DIM[1]*DIM[2] +
 * DIM[2]*DIM[0] surface elements, sent by soc_sim_pb(SOURCE = 3, PACKETS = nelem, BATCH = k * 12*ROI_NSIDE^2,
 * GLOBAL >= 100 * nelem) (kernel_ASOC.c:97-105,141-179,469-501).  LOAD = NULL turns it off. */
int soc_set_roi_load(soc_ctx *ctx, const int32_t *DIM, int ROI_NSIDE, const float *LOAD);

/* replaces the HPBG_buf / HPBGP_buf uploads (ASOC.py:1196-1214): the Healpix sky of the current
 * frequency in photons per package, 49152 floats (NSIDE 64, RING order); HPBGP = cumulative
 * pixel probability for `hpbg ... weighted` runs (-D HPBG_WEIGHTED=1) or NULL */
int soc_set_hpbg(soc_ctx *ctx, const float *BG, const float *HPBGP);

/* replaces the kernel_ram_hp launch (ASOC.py:1349-1354 -> SimRAM_HP, kernel_ASOC.c:826-850); executed like
 * soc_sim_pb (direct kernel or brick sweep, deferred inside soc_batch_begin/end with its own copy of the sky) */
int soc_sim_hp(soc_ctx *ctx, int PACKETS, int BATCH, float SEED, float TW, int GLOBAL, int gid_first, int gid_count);

/* replaces the kernel_bg_split launch of `split 1` runs (ASOC.py:1343-1347 -> SimBgSplit, kernel_ASOC.c:2117-2851): the
 * isotropic background with packet splitting.  Each work item sends BATCH root rays from each of its SELEM surface elements
 * (element id + elem*GLOBAL, the work item returns at the first one >= AREA, :2194-2198); a ray that steps into a refined cell
 * becomes four, one per sub-element of the face it entered through (:2566-2709; a ray born in a refined boundary cell at once,
 * :2300-2428), the others waiting on a stack of max_split entries per work item (-D MAX_SPLIT; max_split <= 0: 4300,
 * ASOC_aux.py:54).  The stack -- gid_count (rounded up to 64) x max_split x 10 words of device memory, laid out so that a wave's
 * pushes and pops coalesce -- is allocated on first use, kept for the handle and freed with it.  GLOBAL is the logical launch
 * size (GLOBAL_SPLIT, ASOC.py:311-315) and the work-item range works as in soc_sim_pb.  Always the direct kernel: the brick sweep
 * stands aside, and inside soc_batch_begin/end the launch runs at once, after what was deferred before it.
 * Refused (SOC_ERR_ARG / SOC_ERR_STATE, the handle stays usable): no grid, max_split < 14 (a split needs 4 free entries above
 * the reference's NBUF > MAX_SPLIT-10 test), SELEM < 1, a range outside GLOBAL, a stack that does not fit in device memory (the
 * message carries its size), and what SimBgSplit has no branch for: reflecting faces (soc_set_mirror), weighted free paths
 * (soc_set_step_weight), a region-of-interest record (soc_set_roi_save).  A single-level grid never splits but is accepted.
 * A split whose 4^d entries would not fit the stack -- the reference writes them without looking -- is an overflow drop. */
int soc_sim_bg_split(soc_ctx *ctx, int PACKETS, int BATCH, float SEED, float BG, float TW, int SELEM, int max_split,
                     int GLOBAL, int gid_first, int gid_count);
/* replaces the kernel_hp_split launch of `split 1` runs with a Healpix sky (ASOC.py:1336-1340 -> SimHpSplit,
 * kernel_ASOC.c:2871-3550).  Work item id sends BATCH root rays, each created like a SimRAM_HP packet -- sky pixel uniform or by
 * HPBGP, entry face with probability ~ |DIR_i| -- except that the face is chosen on the direction as it comes from the pixel and
 * the clamp to DEPS follows IndexG (:2963-2988).  No work item returns early (SimRAM_HP's do at id >= 8*AREA).  Splitting, stack,
 * max_split and the work-item range are soc_sim_bg_split's, with two rules of the reference's own: inside the walk a ray splits
 * only where (NBUF+4) < (MAX_SPLIT-1) -- on a nearly full stack it goes on unsplit on the finer level with PHOTONS unscaled
 * (:3263; counted, soc_split_skipped) -- and the replicas of a jump over two or more levels are written level by level where
 * (NBUF + 4*no) < MAX_SPLIT (:3352).  GLOBAL is the number of work items launched (GLOBAL_SPLIT, ASOC.py:311-315; the weight of
 * the sky counts Fix(GLOBAL_SPLIT, 64), launch.hp_split_launch).
 * Like soc_sim_bg_split the launch is not deferred: inside soc_batch_begin/end it runs at once, after what was deferred before
 * it, on the handle's stream, and reads the sky that is current at the call.  A following soc_set_hpbg cannot overtake the
 * kernel: its copies go to the same stream and it synchronises that stream.
 * Refused as soc_sim_bg_split refuses (max_split < 14, mirror, step weight, roi save, range, memory), and without a sky:
 * "call soc_set_hpbg first".  Whether the sky is weighted is soc_set_hpbg's decision (HPBGP given or not). */
int soc_sim_hp_split(soc_ctx *ctx, int PACKETS, int BATCH, float SEED, float TW, int max_split, int GLOBAL, int gid_first, int gid_count);
/* counters of the soc_sim_bg_split and soc_sim_hp_split launches since the last reset, summed over work items: out[0] root rays started,
 * out[1] split events, out[2] those over two or more levels, out[3] rays ended on reaching a level below the one they were
 * created on, out[4] stack-overflow drops (the ray and all on its stack), out[5] work items that returned at 30000 steps */
int soc_split_stats(soc_ctx *ctx, uint64_t out[6], int reset);
/* the largest number of stack entries a work item of those launches held, as of the last soc_split_stats call; -1: no handle */
int64_t soc_split_max_depth(soc_ctx *ctx);
/* splits that soc_sim_hp_split launches skipped because the stack was nearly full, as of the last soc_split_stats call (the
 * isotropic kernel never counts here); -1: no handle */
int64_t soc_split_skipped(soc_ctx *ctx);

/* replaces queue.finish() (ASOC.py:1461) */
int soc_sync(soc_ctx *ctx);

/* replaces cl.enqueue_copy(host, TABS_buf / INT_buf) (ASOC.py:1482, 1533); n = CELLS */
int soc_read_tally(soc_ctx *ctx, int which, float *out, int64_t n);
/* the inverse (e.g. `cload` restart files, ASOC.py:1013-1018) */
int soc_write_tally(soc_ctx *ctx, int which, const float *in, int64_t n);

/* device address of a tally (for an RCCL all-reduce by the caller), or bind caller-owned
 * device memory (n = CELLS floats, checked) as the tally so a framework tensor can be reduced in place;
 * device_ptr = NULL gives the tally back to memory of the library.  A grid with another cell count cannot
 * be set while a caller-owned tally is bound. */
void *soc_tally_ptr(soc_ctx *ctx, int which);
int   soc_bind_tally(soc_ctx *ctx, int which, void *device_ptr, int64_t n);

/* PAR table computed by soc_set_grid (CELLS - NX*NY*NZ entries), for verification */
int soc_read_par(soc_ctx *ctx, int32_t *out, int64_t n);

/* counters accumulated by the kernels since the last reset:
 * out[0] tally events, out[1] packets created, out[2] scattering events */
int soc_stats(soc_ctx *ctx, uint64_t out[3], int reset);
/* cell steps of all rays (look-ahead, packet, peel-off) of the scattered-light launches that ran as sweeps of rays (brick-local
 * hierarchies, single-level grids), as of the last soc_stats call (what the read-only roofline of SURVEY 8(d) counts: 4 B per step); -1: no handle */
int64_t soc_sca_ray_steps(soc_ctx *ctx);

/* number of brick-sweep passes of the last launch (0 if it ran in direct mode) */
int soc_last_passes(soc_ctx *ctx);
/* how the last launch was executed: 0 direct kernel, 1 brick sweep on a Cartesian grid, 2 on a hierarchy read from global
 * memory, 3 on brick-local hierarchies (soc_ltree.h: hierarchies whose Index() the reference evaluates in double) -- and, for the
 * scattered-light launches, the sweep of rays on a single-level (Cartesian) grid, whose bricks hold root cells only (form 3 with the
 * octree bit of soc_last_variant clear; absorption launches on Cartesian grids stay form 1) */
int soc_last_form(soc_ctx *ctx);
/* the compiled absorption kernel the last launch or sweep of the handle ran on (-1 before any ran), for verification:
 *   bits 0-1  form: 0 direct kernel, 1-3 as soc_last_form
 *   bits 2-4  kind: direct 0 SimRAM_PB, 1 SimRAM_HP, 2 SimRAM_CL; sweeps the pass kernel's KIND -- 0 PB, 1 HP, 2 CL,
 *             3 PB with background packets only (the lean kernel), 4 launches of several kinds (brick-local only)
 *   bits 5-6  WINT: 0 TABS only, 1 INT tally, 2 INT and INTX/Y/Z (brick-local), 3 the INT tally alone in LDS (brick-local)
 *   bit 7 octree, bit 8 Index() in double, bit 9 per-cell opacities, bit 10 ALI (brick-local), bit 11 the sweep of rays of
 *   the scattered-light kernels (then the other fields are 0 but form 3, octree, double, and bits 12-13; on a single-level grid
 *   form 3 with octree = 0: the field has two bits, there is no form 4)
 *   bit 12 (sweeps of rays) the image was a Healpix map seen from a position (soc_sca_set_healpix)
 *   bit 13 (sweeps of rays) the sweep held a SimRAM_HP launch (soc_sca_sim_hp: the Healpix sky as the source)
 *   bit 14 a launch of the packet-splitting kernels (soc_sim_bg_split, soc_sim_hp_split): then form 0, kind 0 SimBgSplit or
 *          1 SimHpSplit, WINT 0 or 1, and octree, double (never on a Cartesian grid) and per-cell opacities name the compiled
 *          instance; a split launch without work items leaves the code as it was
 *   bit 15 a launch of the direct scattered-light kernel (soc_sca_sim_* that did not run as a sweep of rays): then form 0, kind 0
 *          SimRAM_PB, 1 SimRAM_CL, 2 SimRAM_PS or 3 SimRAM_HP (the scattered-light kernels' own numbering), WINT 0, and octree, double
 *          and per-cell opacities name the compiled instance -- double as the kernel got it, which on a single-level grid with
 *          NX > 399 is 1; a launch without work items leaves the code as it was */
int soc_last_variant(soc_ctx *ctx);

/* HIP-event timing on the handle's stream: bracket launches, then read elapsed ms */
int soc_timer_start(soc_ctx *ctx);
int soc_timer_stop(soc_ctx *ctx, float *elapsed_ms);

/* ---- scattered-light images: ASOCS.py / kernel_ASOC_sca.c ---- */

/* replaces the ODIR/RA/DE buffers and the NDIR, NPIX, MAP_DX, MAPCENTRE scalars of every
 * kernel_ASOC_sca.c launch (ASOCS.py:247-262, 655-708) and the -D FFS= build option
 * (ASOCS.py:139).  ODIR, RA, DE hold 4 floats per direction (cl float3), as returned by
 * set_observer_directions (ASOC_aux.py:1129-1183); CENTRE = 3 floats.  Allocates the image
 * OUT[NDIR][NPIX_Y][NPIX_X] on the device (ASOCS.py:246).  Healpix output (NDIR<0) is not
 * supported. */
int soc_sca_set_view(soc_ctx *ctx, int NDIR, const float *ODIR, const float *RA, const float *DE,
                     int NPIX_X, int NPIX_Y, float MAP_DX, const float *CENTRE, int FFS);

/* the other form of the view: one Healpix map (RING, NSIDE = USER.OUT_NSIDE) seen by an observer at a
 * position in root-grid units (`perspective x y z`; ASOCS.py:44-48: NDIR = -NSIDE, ODIR[0] = the
 * position).  The image has 12*NSIDE^2 pixels; each contribution carries 1/d^2. */
int soc_sca_set_healpix(soc_ctx *ctx, int NSIDE, const float *OBSERVER, int FFS);

/* replaces zero_out (kernel_ASOC_sca.c:14-35; ASOCS.py:515, 781) */
int soc_sca_zero(soc_ctx *ctx);

/* replaces the kernel_PS launch (ASOCS.py:665-671 -> SimRAM_PS, kernel_ASOC_sca.c:1462-1489):
 * point sources.  XPS_* are the int32/float32 arrays of AnalyseExternalPointSources exactly as
 * ASOCS.py uploads them; the reference kernel declares the two integer arrays as float and
 * that reading is reproduced.  Work-item range as in soc_sim_pb. */
int soc_sca_sim_ps(soc_ctx *ctx, int PACKETS, int BATCH, float SEED, float BG, const float *PSPOS, const float *PS,
                   int NO_PS, const int32_t *XPS_NSIDE, const int32_t *XPS_SIDE, const float *XPS_AREA,
                   int GLOBAL, int gid_first, int gid_count);

/* replaces the kernel_PB launch (ASOCS.py:681-688 -> SimRAM_PB, kernel_ASOC_sca.c:471-501):
 * SOURCE 1 = isotropic background (what ASOCS.py uses it for), 0 = point sources */
int soc_sca_sim_pb(soc_ctx *ctx, int SOURCE, int PACKETS, int BATCH, float SEED, float BG, const float *PSPOS,
                   const float *PS, int NO_PS, const int32_t *XPS_NSIDE, const int32_t *XPS_SIDE,
                   const float *XPS_AREA, int GLOBAL, int gid_first, int gid_count);

/* replaces the kernel_CL launches (ASOCS.py:692-698, 862-868 -> SimRAM_CL,
 * kernel_ASOC_sca.c:1098-1122); uses EMIT/EMWEI from soc_set_emission() */
int soc_sca_sim_cl(soc_ctx *ctx, int SOURCE, int PACKETS, int BATCH, float SEED, int GLOBAL, int gid_first, int gid_count);

/* replaces the kernel_HP launch (ASOCS.py:673-679 -> SimRAM_HP, kernel_ASOC_sca.c:40-63): background from
 * the Healpix sky given to soc_set_hpbg (49152 pixels, photons per package) */
int soc_sca_sim_hp(soc_ctx *ctx, int PACKETS, int BATCH, float SEED, int GLOBAL, int gid_first, int gid_count);

/* replaces cl.enqueue_copy(OUT, OUT_buf) (ASOCS.py:715, 874); n = NDIR*NPIX_Y*NPIX_X, or 12*NSIDE^2 */
int soc_sca_read_out(soc_ctx *ctx, float *out, int64_t n);

/* device address of the image, or bind caller-owned device memory as the image (for an RCCL
 * all-reduce over the GPUs that shared a launch); NULL gives the image back to memory of the library */
void *soc_sca_out_ptr(soc_ctx *ctx);

/* Scattered-light launches in batches.  The reference runs one kernel after the other per frequency and source (ASOCS.py:655-708)
 * and reads the image after each frequency (:710-716).  Between soc_batch_begin and soc_batch_end (above) the soc_sca_sim_ps / _pb /
 * _cl launches that can run as rays (flat or Healpix image, scalar opacities, one scattering function; a hierarchy whose Index() the
 * reference evaluates in double, or a single-level grid -- there in automatic mode only from 8 bricks of 16^3 cells on, and the batch
 * runs as a sweep from 2.5e7 work items on, as the direct kernel below) are deferred, each with a snapshot of its inputs, and run together in one sweep
 * -- more rays per brick and pass than any single launch has; every other launch runs at once, as without the batch.
 * soc_sca_batch_images(n) gives the batch n zeroed images (n = 0: the one image of soc_sca_set_view again); the launches that
 * follow soc_sca_batch_select(k) add to image k -- one image per frequency -- and soc_sca_batch_read(k, ...) replaces the
 * enqueue_copy of that frequency's image after soc_batch_end. */
int soc_sca_batch_images(soc_ctx *ctx, int n);
int soc_sca_batch_select(soc_ctx *ctx, int k);
int soc_sca_batch_read(soc_ctx *ctx, int k, float *out, int64_t n);
int   soc_sca_bind_out(soc_ctx *ctx, void *device_ptr);

/* ---- equilibrium dust temperature and emission (ASOC.py `CLT`/`CLE` paths) ---- */

/* -D CR_HEATING=1 -D CR_HEATING_RATE=<rate> (ini key CR_HEATING; ASOC.py:352,362; kernel_ASOC_aux.c:769-773): soc_solve_temperature
 * adds 1e-27 * FACTOR * rate to the energy a cell absorbs.  rate = 0 switches it off. */
int soc_set_cr_heating(soc_ctx *ctx, float rate);

/* -D LEVEL_THRESHOLD=<level> (ini key threshold; kernel_ASOC_map.c:825-834): soc_map (flat maps; HealpixMapping has no such
 * test) leaves out the emission of cells on levels below `level`; they still absorb.  0 switches it off. */
int soc_set_map_threshold(soc_ctx *ctx, int level);

/* -D MAP_INTERPOLATION=<mode> (ini key mapint; ASOC.py:352,362; kernel_ASOC_map.c:656-810): soc_map (flat maps and the
 * longitude x latitude image; HealpixMapping has no such block) blends the density and the emission of every cell on the
 * ray with those of two neighbours across the ray; mode 2 also limits a step to 0.22 cells.  0 switches it off. */
int soc_set_map_interpolation(soc_ctx *ctx, int mode);

/* -D ROI_MAP=1 and the ROI argument of Mapping / HealpixMapping (ini key roimap with roi; ASOC.py:2941-2956,3126-3133;
 * kernel_ASOC_map.c:37-56,821-823,947-949): soc_map counts the emission of cells whose root cell lies inside
 * ROI = [x0,x1,y0,y1,z0,z1] (inclusive) only; extinction as usual.  NULL switches it off. */
int soc_set_map_roi(soc_ctx *ctx, const int32_t *ROI);

/* replaces the EqTemperature launches per level (ASOC.py:2024-2040 -> kernel_ASOC_aux.c:745-790):
 * EABS[CELLS] = integrated absorbed energy per cell (the array the reference calls EMIT at this
 * point: TABS of the dust-emission iteration + CTABS), TTT[NE] the host's E->T table with
 * E[i] = Emin*kE^i (ASOC.py:643-689); FACTOR and LENGTH = GL*PARSEC are the -D FACTOR / -D LENGTH
 * literals (ASOC.py:345,348: %.4e and %.5e).  Temperatures stay on the device for soc_emission and
 * are copied to TNEW[CELLS] unless NULL. */
int soc_solve_temperature(soc_ctx *ctx, float adhoc, float kE, float Emin, int NE, const float *TTT, float FACTOR,
                          float LENGTH, const float *EABS, float *TNEW);

/* temperatures from elsewhere (`loadtemp`, ASOC.py:744-760) */
int soc_set_temperature(soc_ctx *ctx, const float *T);

/* replaces the Emission / Emission2 launches (ASOC.py:2154-2197 -> kernel_ASOC_aux.c:795-808, 862-888):
 * EMITTED[CELLS][nfreq] = FACTOR x photons / Hz / cm3 of the modified black body at the device
 * temperatures, for the nfreq frequencies FREQ with absorption cross sections FABS */
int soc_emission(soc_ctx *ctx, int nfreq, const float *FREQ, const float *FABS, float FACTOR, float LENGTH, float *EMITTED);

/* ---- map making ---- */

/* replaces the kernel_map launch + copies (ASOC.py:3113-3128 -> Mapping / HealpixMapping, kernel_ASOC_map.c:496-516,
 * 890-910): line-of-sight integral of EMIT[CELLS] (x density, with extinction ABS+SCA or the per-cell OPT of soc_set_opt)
 * for one map.  healpix = 0: orthographic map of NPIX_X x NPIX_Y pixels of MAP_DX root cells towards DIR with image axes
 * RA (right), DE (up) through CENTRE -- or, with INTOBS given (INTOBS[0] > -1e10), the longitude x latitude image seen
 * from that position; healpix = 1: Healpix map of NSIDE = NPIX_X seen from INTOBS.  MAP gets the surface brightness
 * integral, SAVETAU the optical depth or (save_colden) column density x LENGTH.  -D MAP_INTERPOLATION, ROI_MAP and
 * LEVEL_THRESHOLD: soc_set_map_interpolation, soc_set_map_roi, soc_set_map_threshold.  Polarisation maps: soc_polmap. */
int soc_map(soc_ctx *ctx, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *EMIT, const float *DIR,
            const float *RA, const float *DE, const float *CENTRE, const float *INTOBS, float ABS, float SCA,
            int save_colden, float LENGTH, float *MAP, float *SAVETAU);

/* `mapping nx ny dx 999` (a fourth argument >= 999): replaces the kernel_map launch + copy of ASOC.py:3409-3418 -> the Mapping
 * of kernel_ASOC_map_H.c (:380-497): one image per hierarchy level.  MAP holds LEVELS planes of NPIX_Y*NPIX_X floats; plane l
 * is the line-of-sight integral of EMIT[CELLS] (x density) over the cells of level l only, attenuated by everything in
 * front of them -- the planes add up to one map.  The view is soc_map's with healpix = 0: the orthographic map towards DIR
 * with image axes RA, DE through CENTRE, or with INTOBS given (INTOBS[0] > -1e10; NULL: external view) the longitude x
 * latitude image seen from there.  That file has its own ray entry and its own Index() (see soc_polmap_healpix), restated as
 * written: on a Cartesian grid the one plane is soc_map's image up to the entry point (an EPS apart); on a hierarchy a ray that
 * climbs out of an octet into a root leaf goes on from the corner of the grid and usually ends there, so the planes hold only
 * what lies in front of that point (DESIGN.md section 5 has figures).  Extinction is ABS+SCA or the per-cell OPT of
 * soc_set_opt* (the line that file keeps under "#ifdef USE_ABU", :474-478, which ASOC.py never defines: the reference itself
 * always takes the scalars).  That kernel tests neither -D MAP_INTERPOLATION, LEVEL_THRESHOLD nor ROI_MAP:
 * soc_set_map_interpolation, soc_set_map_threshold and soc_set_map_roi have no effect here.  A pixel whose ray misses the
 * model is 0 on every level.  A ray is ended after 2^15 cell steps, as in soc_polmap_healpix.
 * SOC_ERR_STATE without a grid; SOC_ERR_ARG for NPIX_X or NPIX_Y < 1, LEVELS*NPIX_X*NPIX_Y beyond int, EMIT or MAP NULL, an
 * external view without DIR, RA, DE, CENTRE or MAP_DX > 0 or with a component of DIR that is zero (the walk divides by it). */
int soc_map_levels(soc_ctx *ctx, int NPIX_X, int NPIX_Y, float MAP_DX, const float *EMIT, const float *DIR, const float *RA,
                   const float *DE, const float *CENTRE, const float *INTOBS, float ABS, float SCA, float *MAP);

/* `mapping nx ny dx NF`, 2 <= NF <= 998 (ASOC.py:3442-3568: "this many frequencies per kernel call"; the reference's branch
 * asks for a kernel_ASOC_map_X.c that it does not ship and stops): the maps of a batch of frequencies from one walk per pixel.
 * The products are defined as those of soc_map, frequency by frequency, bit for bit.
 * soc_map_block_max: the most frequencies one batch may hold. */
int soc_map_block_max(void);

/* stands in for the EMITX upload of ASOC.py:3520-3545: one batch of nf frequencies into device memory the handle owns, where it
 * stays for any number of soc_map_block calls (the directions of a run).  EMITX[CELLS][nf] is the emission, cell-major;
 * ABSX[nf] and SCAX[nf] the scalar opacities; OPTX, when not NULL, [CELLS][nf][2] per-cell opacities (absorption,
 * scattering) that are used instead -- the per-cell OPT of soc_set_opt* plays no part in soc_map_block.  nf = 0 frees the
 * batch; soc_set_grid with another cell count drops it.  nf < 0 or nf > soc_map_block_max() is SOC_ERR_ARG. */
int soc_map_set_block(soc_ctx *ctx, int nf, const float *EMITX, const float *ABSX, const float *SCAX, const float *OPTX);

/* stands in for the kernel_map_X launch + copies of ASOC.py:3546-3568: the maps of the resident batch for one view, with the
 * arguments of soc_map (healpix, NPIX_X, NPIX_Y, MAP_DX, DIR, RA, DE, CENTRE, INTOBS, LENGTH) and its switches
 * (soc_set_map_threshold, soc_set_map_interpolation, soc_set_map_roi).  MAPX[nf][npix] and TAUX[nf][npix] get, plane by
 * plane, what soc_map gives as MAP and (save_colden = 0) SAVETAU for that frequency; COLDEN[npix] what it gives as SAVETAU
 * with save_colden = 1.  Without a resident batch: SOC_ERR_ARG. */
int soc_map_block(soc_ctx *ctx, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *DIR, const float *RA,
                  const float *DE, const float *CENTRE, const float *INTOBS, float LENGTH, float *MAPX, float *TAUX,
                  float *COLDEN);

/* `maplevels 1`: the levels of the plain map -- the resident batch of soc_map_set_block for one view, one plane per frequency
 * and hierarchy level.  It stands in for nothing in the reference: what the reference offers per level is the Mapping of
 * kernel_ASOC_map_H.c, and that is soc_map_levels, on that file's own walk.
 * Definition: MAPL[f][l][npix] is, bit for bit, the MAP that soc_map (equally soc_map_block) gives for frequency f under the
 * same view and switches when the emission of every cell that is not on level l is set to 0.0f; densities and opacities are
 * left as they are.  Plane l is what the cells of level l emit towards the pixel, attenuated by everything in front of them;
 * the planes of a pixel add up to its plain-map value up to the order of the fp32 additions.  With soc_set_map_interpolation
 * 1 | 2 the blend of a step is evaluated per level with the contributors of other levels replaced by 0.0f (a neighbour on
 * another level feeds that level's plane); whether a step emits at all (soc_set_map_roi, soc_set_map_threshold) and the
 * blended density stay properties of the cell being crossed.  The optical depth is that of the plain map: opacity is not masked.
 * The arguments are those of soc_map_block (healpix = 1: a map of NSIDE = NPIX_X seen from INTOBS).  The batch is read, never
 * changed: a soc_map_block after the call gives what it gave before.  The planes are staged in device memory the handle owns,
 * freed with the batch and with the handle.
 * SOC_ERR_STATE without a grid; SOC_ERR_ARG without a resident batch, for MAPL NULL, NPIX_X or NPIX_Y < 1, a view soc_map_block
 * refuses, and for nf * LEVELS * npix floats that do not fit the free device memory (the message states the size).  A refused
 * call leaves tallies, batch and handle as they were.
 * soc_map_block_levels_width: the most frequencies one kernel launch of the handle's model takes (8 up to 8 levels, else 4);
 * wider batches run as several launches. */
int soc_map_block_levels(soc_ctx *ctx, int healpix, int NPIX_X, int NPIX_Y, float MAP_DX, const float *DIR, const float *RA,
                         const float *DE, const float *CENTRE, const float *INTOBS, float *MAPL);
int soc_map_block_levels_width(soc_ctx *ctx);

/* replaces the Bx_buf, By_buf, Bz_buf uploads of ASOC.py:3722-3727: the magnetic field of the polarisation maps, CELLS
 * floats per component in the order of the cloud file (all cells, parents included).  The device keeps one 16-byte record
 * (Bx, By, Bz, pad) per cell.  A polarisation reduction factor is encoded in the length of the vectors by the caller
 * (ASOC.py:3681-3719).  Three NULL pointers free the field; soc_set_grid with another cell count drops it. */
int soc_set_bfield(soc_ctx *ctx, const float *Bx, const float *By, const float *Bz);

/* replaces the PolMapping launch + copy of ASOC.py:3790-3796 -> kernel_ASOC_map.c:972-1137 (-D POLSTAT=0: MAP = I, Q, U,
 * column density x LENGTH), :1147-1384 (POLSTAT=1: rT, rI, jT, jI, two passes along the ray), :1594-1693 (POLSTAT=3: <B>,
 * <B_LOS>, <B_POS>, tau): one orthographic map of NPIX_X x NPIX_Y pixels of MAP_DX root cells towards DIR with image axes
 * RA (right), DE (up) through CENTRE; MAP holds the four planes, 4*NPIX_X*NPIX_Y floats.  polred = -D POLRED (the
 * polarisation fraction of a cell is |B| instead of p0), rho_weight = -D POL_RHO_WEIGHT (POLSTAT 0: density instead of
 * emission weights), p0 = -D p00.  Extinction is ABS+SCA or the per-cell OPT of soc_set_opt*; -D LEVEL_THRESHOLD is
 * soc_set_map_threshold.  A ray that misses the cloud gives 0/0 = NaN for POLSTAT 1 and 3, as in the reference.
 * Refused with an error code: no field set (SOC_ERR_STATE); polstat other than 0, 1, 3, polred with polstat 3, or a
 * component of DIR that is zero -- the walk divides by it (SOC_ERR_ARG). */
int soc_polmap(soc_ctx *ctx, int polstat, int polred, int rho_weight, float p0, int NPIX_X, int NPIX_Y, float MAP_DX,
               const float *EMIT, const float *DIR, const float *RA, const float *DE, const float *CENTRE, float ABS,
               float SCA, float LENGTH, float *MAP);

/* replaces the PolHealpixMapping launch + copy of ASOC.py:3946-3952 -> kernel_ASOC_map_H.c:576-841 (-D POLSTAT=0): the all-sky
 * polarisation map of NSIDE seen from the position INTOBS[3] (root-grid coordinates) inside the model; MAP holds four planes
 * of 12*NSIDE^2 floats in RING order: I, Q, U and column density x LENGTH.  The field is that of soc_set_bfield.  polred =
 * -D POLRED, p0 = -D p00, interpolate = -D INTERPOLATE (0: the cell's density; 1: four-point and 2: 3x3x3 blends on a
 * Cartesian grid; 3: 27 look-ups around the middle of the step, also on hierarchies), minlos / maxlos = -D MINLOS / MAXLOS
 * [root cells]: nothing is registered before minlos and the ray ends at maxlos; y_shear = the Y_SHEAR argument (periodic in
 * x and y, y shifted by that many root cells across the x faces).  Extinction is ABS+SCA or the per-cell OPT of
 * soc_set_opt* (the line that file keeps under "#ifdef USE_ABU", :736-740, which ASOC.py never defines: the reference itself
 * always takes the scalars); -D LEVEL_THRESHOLD is soc_set_map_threshold.  That file has its own Index() (:216-289): on a
 * hierarchy a ray keeps octet coordinates when it climbs into a root leaf, restated as written.  An observer outside the
 * model gives four planes of zeros.  A ray is ended after 2^15 cell steps: on a hierarchy that walk can
 * cycle without end, and the reference then does not return.
 * Refused with an error code, nothing changed: no field set (SOC_ERR_STATE); NSIDE < 1, interpolate outside 0..3, interpolate
 * 1 or 2 on a hierarchy (LEVELS > 1: the reference indexes level 0 as a plain grid there and reads links as densities),
 * y_shear != 0 with maxlos >= 1e9 (a ray near the equator would wrap ~NZ/1e-5 root cells) (SOC_ERR_ARG).  -D POLSTAT > 0
 * does not compile in that file (:928) and is not offered. */
int soc_polmap_healpix(soc_ctx *ctx, int NSIDE, int polred, float p0, int interpolate, float minlos, float maxlos,
                       float y_shear, const float *EMIT, const float *INTOBS, float ABS, float SCA, float LENGTH, float *MAP);

/* ---- stochastically heated grains: A2E.py / kernel_A2E.c ---- */

/* replaces the PSTau launch of ASOC.py:3576-3645 (ini key pssavetau; kernel_ASOC_map.c:1545-1584): for every point source
 * the column density (x LENGTH) and the optical depth (ABS + SCA, or the per-cell OPT of soc_set_opt) along the ray from the
 * source towards the observer direction DIR[3].  PSPOS: 4 floats per source (cl float3). */
int soc_ps_tau(soc_ctx *ctx, int NO_PS, const float *PSPOS, const float *DIR, float ABS, float SCA, float LENGTH,
               float *pscolden, float *pstau);

/* replaces the per-size uploads of A2E.py:338-371 (AF, Iw, L1, L2, Tdown, EA, Ibeg) and the
 * -D NE -D NFREQ build of A2E.py:283-304.  L1/L2 are [NE*NE] indexed l*NE+u, Iw holds noIw
 * weights in (l, u, i) loop order, EA is [NFREQ*NE]. */
int soc_a2e_set_size(soc_ctx *ctx, int NE, int NFREQ, int noIw, const float *Iw, const int32_t *L1,
                     const int32_t *L2, const float *Tdown, const float *EA, const int32_t *Ibeg, const float *AF);

/* how DoSolve is launched for the size last given to soc_a2e_set_size (read-only; nothing runs): out[0] cells per workgroup
 * (4, 2 or 1), out[1] threads per workgroup (256 or 1024), out[2] bytes of dynamic LDS.  SOC_ERR_STATE before any
 * soc_a2e_set_size.  A size of which not one cell fits the 160 KB of LDS is refused by soc_a2e_set_size itself. */
int soc_a2e_launch_shape(soc_ctx *ctx, int out[3]);

/* replaces enqueue_copy(ABS_buf) + DoSolve(...) + enqueue_copy(emit, EMIT_buf) for one batch of
 * cells (A2E.py:387-412 -> kernel_A2E.c:2-104): AABS, AEMIT are [batch*NFREQ] host arrays */
int soc_a2e_solve(soc_ctx *ctx, int batch, const float *AABS, float *AEMIT);
/* the same in three steps with the batch resident on the device (timing the kernel alone) */
int soc_a2e_upload(soc_ctx *ctx, int batch, const float *AABS);
int soc_a2e_run(soc_ctx *ctx, int batch);
int soc_a2e_download(soc_ctx *ctx, int batch, float *AEMIT);

/* The same with the cells RESIDENT in device memory.  The reference uploads every batch of cells once per grain size and adds the
 * sizes' emission up on the host (A2E.py:520-600: NSIZE x (absorptions in + emission out) over PCIe); a model's absorptions are
 * 4*NFREQ bytes per cell (config 3: 9.9 GB) and fit the device many times over.  soc_a2e_resident_begin(cells, NFREQ) allocates them
 * and a zeroed emission sum; _upload(c0, n, ABS) fills rows [c0, c0+n) (any chunking, e.g. from a memory-mapped absorbed file);
 * after every soc_a2e_set_size, _solve() runs DoSolve over all cells and ADDS the emission of that size to the sum -- the same fp32
 * additions in the same order as the host's EMITTED += emit; _download(c0, n, EMIT) reads rows of the sum; _end() frees both. */
int soc_a2e_resident_begin(soc_ctx *ctx, int64_t cells, int NFREQ);
int soc_a2e_resident_upload(soc_ctx *ctx, int64_t c0, int64_t n, const float *AABS);
int soc_a2e_resident_solve(soc_ctx *ctx);
int soc_a2e_resident_download(soc_ctx *ctx, int64_t c0, int64_t n, float *AEMIT);
int soc_a2e_resident_end(soc_ctx *ctx);

/* Polarised emission beside the emission: the emission of the grains larger than each cell's minimum aligned size a_alg, which the
 * reference's host adds up per batch and size (A2E.py:192-197 the second array, :413-429 the weights of a stochastic size).  Here the
 * sum over the sizes lives on the device, so the solver kernel's epilogue adds W * emission to a second sum:
 *   soc_a2e_resident_begin_pol(cells, NFREQ, polarised) is soc_a2e_resident_begin that, with polarised != 0, also allocates that
 *       second sum (zeroed; 4*cells*NFREQ bytes more, counted in the memory check) and 8 bytes per cell for a_alg and log10(a_alg);
 *   soc_a2e_resident_upload_aalg(c0, n, aalg, lgaalg) fills rows [c0, c0+n) of both (the file of A2E.py:415 and its log10 as numpy
 *       takes it, :425); rows never uploaded are aligned for no size;
 *   soc_a2e_set_size_aalg(ASIZE[isize], ASIZE[isize+1] or 0 for the last size, log10(ASIZE[isize]),
 *       log10(ASIZE[isize+1]) - log10(ASIZE[isize])) gives the weights of the size of the last soc_a2e_set_size (A2E.py:417, :423-425):
 *       W = 1 where ASIZE[isize] >= a_alg, (log10(a_alg) - log10(ASIZE[isize])) / the difference where a_alg lies strictly between the
 *       two sizes, else 0 -- one float subtraction, one float division, then the float product W * emission and the float sum, each
 *       rounded as numpy's float32 expressions are.  soc_a2e_set_size clears the weights: a size solved without this call adds
 *       nothing to the polarised sum;
 *   soc_a2e_resident_download_p(c0, n, PEMIT) reads rows of the polarised sum (SOC_ERR_STATE where it was not asked for).
 * Without these calls the family behaves as before. */
int soc_a2e_resident_begin_pol(soc_ctx *ctx, int64_t cells, int NFREQ, int polarised);
int soc_a2e_resident_upload_aalg(soc_ctx *ctx, int64_t c0, int64_t n, const float *aalg, const float *lgaalg);
int soc_a2e_set_size_aalg(soc_ctx *ctx, float asize, float asize_next, float lg_asize, float lg_step);
int soc_a2e_resident_download_p(soc_ctx *ctx, int64_t c0, int64_t n, float *PEMIT);

/* The equilibrium sizes of a dust (isize >= NSTOCH, A2E.py:456-547 -> kernel_A2E.c:110-154) on the RESIDENT cells: all of them in one
 * sweep that reads the absorptions and reads and writes the sum once (12*NFREQ bytes per cell; 20*NFREQ + 8 with the polarised sum),
 * with the bits of soc_a2e_eqtemp per size and the host statements around it.
 *   soc_a2e_set_eq_sizes(nsizes, NFREQ, NIP, FACTOR, FREQ[NFREQ], AF[nsizes][NFREQ], KABS[nsizes][NFREQ], TTT[nsizes][NIP],
 *       Emin[nsizes], kE[nsizes], oplgkE[nsizes], GD, S_FRAC[nsizes], SIZE_A[nsizes] or NULL) copies the tables of the sizes to the
 *       device, in the order in which their emission is to be added (ascending sizes; the caller leaves out a size it skips).  A size
 *       sees the absorptions a[i] * AF[size][i] (one float product), its emission is added to the sum as emit * (GD * S_FRAC[size]) and,
 *       where SIZE_A is given, to the polarised sum as (emit * GD) * S_FRAC[size] in the cells with SIZE_A[size] >= a_alg (the hard
 *       mask of A2E.py:533-539).  SOC_ERR_ARG where the row of one cell (NFREQ | 1 + nsizes floats, and NFREQ more) does not fit the
 *       160 KB of LDS; the sizes set before then stay.
 *   soc_a2e_resident_solve_eq() runs them over the resident cells of soc_a2e_resident_begin or soc_mabu_begin, after the stochastic
 *       sizes' soc_a2e_resident_solve calls.  SOC_ERR_STATE without resident cells, without sizes set for their NFREQ, and where
 *       SIZE_A was given but polarised output was not asked for. */
int soc_a2e_set_eq_sizes(soc_ctx *ctx, int nsizes, int NFREQ, int NIP, float FACTOR, const float *FREQ, const float *AF,
                         const float *KABS, const float *TTT, const float *Emin, const float *kE, const float *oplgkE, float GD,
                         const float *S_FRAC, const float *SIZE_A);
int soc_a2e_resident_solve_eq(soc_ctx *ctx);

/* replaces kernel_T(...) = EqTemperature for one batch (A2E.py:511-530 -> kernel_A2E.c:110-154);
 * TTT holds NIP temperatures, ABS is [batch*NFREQ] (already multiplied by AF on the host),
 * outputs T[batch] and EMIT[batch*NFREQ] */
int soc_a2e_eqtemp(soc_ctx *ctx, int batch, int icell, int CELLS, int NFREQ, int NIP, float FACTOR, float kE,
                   float oplgkE, float Emin, const float *FREQ, const float *KABS, const float *TTT,
                   const float *ABS, float *T, float *EMIT);

/* What A2E_pre.py computes per grain size for a <dust>.solver file (A2E_pre.py:233-256; kernel_A2E_pre.c:580-736
 * PrepareIntegrationWeightsTrapezoid, :123-212 PrepareTdown; -D FACTOR of A2E_pre.py:134 is an argument).
 * In:  FREQ[NFREQ], Ef[NFREQ] = PLANCK*FREQ, SKABS[NFREQ] = pi a^2 Q_abs of ONE grain of this size, the enthalpy grid E[NE+1]
 *      with its temperatures T[NE+1].  2 <= NFREQ <= 639 (the weights kernel keeps 64 columns of NFREQ floats in the 160 KB of
 *      LDS of a workgroup; a larger NFREQ is SOC_ERR_ARG before anything is allocated), 2 <= NE <= 4096.
 * Out: L1, L2[NE*NE] (first and last frequency feeding the transition l -> u at [l*NE+u]; -1, -2 = none; entries with
 *      u <= l are 0 -- the caller sets [0] = -2 as A2E_pre.py:246,249 does), Iw[NE*NE*NFREQ] (the weights of lower bin l
 *      start at l*NE*NFREQ, noIw[l] of them: the file holds them back to back), noIw[NE-1], Tdown[NE]. */
int soc_a2e_pre(soc_ctx *ctx, int NFREQ, int NE, float FACTOR, const float *FREQ, const float *Ef, const float *SKABS,
                const float *E, const float *T, int32_t *L1, int32_t *L2, float *Iw, int32_t *noIw, float *Tdown);

/* ---- equilibrium dust components of a multi-dust run: A2E_MABU.py / kernel_eqsolver.c ---- */

/* replaces kernel_T(...) + the per-frequency kernel_emission(...) launches of SolveEquilibriumDust for one batch of cells
 * (A2E_MABU.py:520-560,608 -> kernel_eqsolver.c EqTemperature :5-62, Emission :66-79): ABS is [batch*NFREQ], the share of
 * the absorptions taken by this dust component (split_absorbed, kernel_A2E_MABU_aux.c:3-23, is done by the caller:
 * soc_amd/mabu.py, host path); TTT holds NE temperatures; outputs T[batch] and EMIT[batch*NFREQ] per unit density and abundance */
int soc_eqsolver(soc_ctx *ctx, int batch, int icell, int CELLS, int NFREQ, int NE, float FACTOR, float kE,
                 float oplgkE, float Emin, const float *FREQ, const float *KABS, const float *TTT,
                 const float *ABS, float *T, float *EMIT);

/* ---- the whole multi-dust stage with the cells RESIDENT in device memory: A2E_MABU.py:700-1140 ---- */

/* The reference keeps the absorptions on the host, and for every dust component uploads them in batches, splits them
 * (kernel_A2E_MABU_aux.c:3-23 through A2E_MABU.py:760-800), writes the share to a file, runs a solver program on it and adds
 * the emission it reads back, weighted by the abundances (A2E_MABU.py:1128-1140).  Here the arrays stay on the device from the
 * absorbed file to the sum:
 *   soc_mabu_begin(cells, NFREQ, NDUST, &fit) reserves the absorptions as the absorbed file holds them, the current dust's share
 *       PART and its emission EM (the arrays of soc_a2e_resident_*: that family's _solve works on them in place, its _upload
 *       and _download write rows of PART and read rows of EM, its _begin and _end are refused with SOC_ERR_STATE until
 *       soc_mabu_end -- as soc_mabu_begin is while a soc_a2e_resident_begin is open; a second soc_mabu_begin replaces the
 *       first), the zeroed sum SUM (cells*NFREQ floats each), ABU[cells*NDUST] and
 *       RABS[NFREQ*NDUST] (double).  *fit (may be NULL) receives the number of cells that fit the free device memory; when
 *       `cells` do not, the call fails with SOC_ERR_STATE and the caller solves the cells in ranges of at most *fit;
 *   soc_mabu_upload(c0, n, ABS) fills rows [c0, c0+n) of the absorptions (any chunking: a memory-mapped absorbed file);
 *   soc_mabu_set_tables(ABU, RABS) uploads the abundances of the resident cells and the relative cross sections
 *       (A2E_MABU.py:245-342), once;
 *   soc_mabu_split(idust, clip_last) computes PART = ABS * RABS[:, idust] / sum_j ABU[:, j] * RABS[:, j] with the types of
 *       kernel_A2E_MABU_aux.c:3-23 (products in double, the sum rounded to float after every dust, the quotient in double) and
 *       zeroes EM; clip_last != 0 then clips the last channel of PART as A2E.py:184-185 does in front of the stochastic solver;
 *   soc_mabu_solve_eq(...) is soc_eqsolver (A2E_MABU.py:520-560,608 -> kernel_eqsolver.c:5-79) on PART, its emission left in EM;
 *       a stochastically heated dust is solved with soc_a2e_set_size + soc_a2e_resident_solve per grain size instead
 *       (A2E.py:520-600), which add to EM;
 *   soc_mabu_accumulate(idust) adds EM * ABU[:, idust] to SUM: float product, float sum (A2E_MABU.py:1128-1140);
 *   soc_mabu_download(c0, n, SUM) reads rows of the sum; soc_mabu_read_part rows of PART (tests); soc_mabu_end frees it all. */
int soc_mabu_begin(soc_ctx *ctx, int64_t cells, int NFREQ, int NDUST, int64_t *cells_fit);
int soc_mabu_upload(soc_ctx *ctx, int64_t c0, int64_t n, const float *ABS);
int soc_mabu_set_tables(soc_ctx *ctx, const float *ABU, const double *RABS);
int soc_mabu_split(soc_ctx *ctx, int idust, int clip_last);
int soc_mabu_solve_eq(soc_ctx *ctx, int NE, float FACTOR, float kE, float oplgkE, float Emin, const float *FREQ,
                      const float *KABS, const float *TTT);
int soc_mabu_accumulate(soc_ctx *ctx, int idust);
int soc_mabu_download(soc_ctx *ctx, int64_t c0, int64_t n, float *SUM);
int soc_mabu_read_part(soc_ctx *ctx, int64_t c0, int64_t n, float *PART);
int soc_mabu_end(soc_ctx *ctx);

/* `polarisation <dust> <aalg file>` of A2E_MABU.py (:158-167): the polarisation reduction factor R = polarised / total emission.
 *   soc_mabu_begin_pol(cells, NFREQ, NDUST, polarised, &fit) is soc_mabu_begin that, with polarised != 0, also reserves the current
 *       dust's polarised emission PEM (the polarised sum of soc_a2e_resident_*), its zeroed sum PSUM and a_alg with its log10
 *       (8*NFREQ + 8 bytes more per cell, counted in *fit); soc_mabu_split then zeroes PEM as well;
 *   soc_a2e_resident_upload_aalg fills the rows of a_alg of the current dust's aalg file (the rows of the resident cell range);
 *   a stochastically heated dust gets PEM from soc_a2e_set_size_aalg before every soc_a2e_resident_solve (A2E_MABU.py:971-984 runs
 *       A2E.py with the aalg file);
 *   soc_mabu_pol_eq(NA, APOL, TAB) gives an equilibrium dust's PEM = EM * ipR_f(a_alg) (A2E_MABU.py:615-637): APOL[NA] the sizes of
 *       <dust>.rpol (not decreasing), TAB[NFREQ][NA] its columns interpolated to the frequencies (:626-633, done by the caller);
 *       ipR_f is linear between the nodes (slope = (y1-y0)/(x1-x0), y = slope*(a-x0) + y0 in double, the node value on a node) and
 *       0 outside them (:635), the product with EM is taken in double and rounded to float once (:637);
 *   soc_mabu_accumulate_p(idust) adds PEM * ABU[:, idust] to PSUM as soc_mabu_accumulate does for the emission (:1139-1147);
 *   soc_mabu_ratio() turns PSUM into R = PSUM / (SUM + 1e-32) in float (:1182), once, after the last dust;
 *   soc_mabu_download_p(c0, n, R) reads rows of it (:1195-1197). */
int soc_mabu_begin_pol(soc_ctx *ctx, int64_t cells, int NFREQ, int NDUST, int polarised, int64_t *cells_fit);
int soc_mabu_pol_eq(soc_ctx *ctx, int NA, const double *APOL, const double *TAB);
int soc_mabu_accumulate_p(soc_ctx *ctx, int idust);
int soc_mabu_ratio(soc_ctx *ctx);
int soc_mabu_download_p(soc_ctx *ctx, int64_t c0, int64_t n, float *R);

/* ---- dust temperatures and enthalpy-level populations: what the solvers above compute on the way to the emission ----
 * Opt-in, each call beside the one it extends; without them nothing above changes.
 *   soc_mabu_download_t(c0, n, T) reads rows [c0, c0+n) of the temperatures that the last soc_mabu_solve_eq left, one float per cell:
 *       what A2E_MABU.py:551 writes to <dust>.T (kernel_eqsolver.c:5-62).  The next soc_mabu_solve_eq overwrites them.  SOC_ERR_STATE
 *       outside soc_mabu_begin ... soc_mabu_end and before any soc_mabu_solve_eq.
 *   soc_a2e_resident_keep_teq(on): with on != 0 every soc_a2e_resident_solve_eq from now on also keeps the temperature of every
 *       (size, cell), [nsizes][cells] floats of device memory; soc_a2e_resident_end / soc_mabu_end free them and switch this off again.
 *       SOC_ERR_STATE without resident cells (soc_a2e_resident_begin or soc_mabu_begin).
 *   soc_a2e_resident_download_teq(slot, c0, n, T) reads rows [c0, c0+n) of size number `slot`, counted in the order in which
 *       soc_a2e_set_eq_sizes got the sizes: T[CELLS] of A2E.py:506-522 (kernel_A2E.c:110-154).  SOC_ERR_STATE before a
 *       soc_a2e_resident_solve_eq that kept them.
 *   soc_a2e_solve_dump(batch, AABS, AEMIT, X) is soc_a2e_solve that also returns X[batch][NE], the populations of the enthalpy levels
 *       clamped to [1e-35, 10]: the DUMP_TDUST=1 build of DoSolve (A2E.py:393-400 -> kernel_A2E.c:14-16, 101-103).  AEMIT has the bits
 *       of soc_a2e_solve.
 *   soc_a2e_resident_solve_dump(X) is soc_a2e_resident_solve that also returns X[cells][NE] (host memory).  The cells are solved in
 *       chunks and X is read back chunk by chunk, so the device holds the populations of one chunk only (65536 cells x NE floats);
 *       SOC_ERR_STATE, naming the bytes, where even that cannot be allocated.  The sums get the bits soc_a2e_resident_solve gives. */
int soc_mabu_download_t(soc_ctx *ctx, int64_t c0, int64_t n, float *T);
int soc_a2e_resident_keep_teq(soc_ctx *ctx, int on);
int soc_a2e_resident_download_teq(soc_ctx *ctx, int slot, int64_t c0, int64_t n, float *T);
int soc_a2e_solve_dump(soc_ctx *ctx, int batch, const float *AABS, float *AEMIT, float *X);
int soc_a2e_resident_solve_dump(soc_ctx *ctx, float *X);

/* ---- the emission of one dust re-emission iteration, RESIDENT for the cell-emission launches of the next ---- */

/* With `iterations N` and `cellpackets` the emission solved from the absorptions of iteration k-1 is what SimRAM_CL sends at every
 * frequency of iteration k (ASOC.py:1593-1810).  The multi-dust stage leaves it as SUM[cells][NFREQ], a launch wants EMIT[CELLS] of one
 * frequency: a column, 4 useful bytes per 128-byte line, at every one of NFREQ launches.  So the resident copy is held transposed,
 * ET[NFREQ][CELLS], filled by one tiled transpose per iteration, and a launch's EMIT is made from one contiguous row of it:
 *   soc_emitted_begin(NFREQ) reserves ET for the cells of the grid (after soc_set_grid), zeroed.  Where it does not fit the free device
 *       memory the call fails with SOC_ERR_STATE and nothing is reserved or released; a second soc_emitted_begin replaces the first;
 *       soc_set_grid, soc_emitted_end and soc_destroy release it;
 *   soc_emitted_upload(c0, n, rows) writes rows[n][NFREQ], as the emitted file holds them, to cells [c0, c0+n) (any chunking);
 *   soc_emitted_from_mabu(c0) writes SUM of the open soc_mabu_begin, device to device, to cells [c0, c0 + its cells): before
 *       soc_mabu_end, after the last soc_mabu_accumulate.  SOC_ERR_STATE without an open soc_mabu_begin, SOC_ERR_ARG where its NFREQ
 *       differs or its cells run past CELLS;
 *   soc_emitted_download(c0, n, rows) reads rows back, bit for bit what went in;
 *   soc_set_emission_column(ifreq, COEFF) fills the EMIT of the next soc_sim_cl as soc_set_emission would from the host statement
 *       (ASOC.py:1737-1740): EMIT[c] = ET[ifreq][c] * (COEFF[level(c)] * DENS[c]), COEFF[LEVELS] = GL*PARSEC/8^level/FACTOR as float,
 *       both products rounded to float, no fused multiply-add; exactly 0 where DENS[c] < 1e-10 (links, empty cells), by selection: a NaN
 *       or the -1e20 of a link's row does not survive.  EMWEI stays what it is.  Like soc_set_emission it does not wait for deferred
 *       launches, which keep their own copy;
 *   soc_read_emission(EMIT, n) reads the first n values of what the next soc_sim_cl would use (tests);
 *   soc_emitted_end() frees it.
 * Every call but _begin and _end is SOC_ERR_STATE before soc_emitted_begin; ifreq outside [0, NFREQ), c0 < 0, n < 1 or c0 + n > CELLS
 * are SOC_ERR_ARG.  A refused call leaves ET as it was. */
int soc_emitted_begin(soc_ctx *ctx, int NFREQ);
int soc_emitted_upload(soc_ctx *ctx, int64_t c0, int64_t n, const float *rows);
int soc_emitted_from_mabu(soc_ctx *ctx, int64_t c0);
int soc_emitted_download(soc_ctx *ctx, int64_t c0, int64_t n, float *rows);
int soc_set_emission_column(soc_ctx *ctx, int ifreq, const float *COEFF);
int soc_read_emission(soc_ctx *ctx, float *EMIT, int64_t n);
int soc_emitted_end(soc_ctx *ctx);

/* How much the resident emission changed since the iteration before: what a convergence criterion of the iterations needs, in one pass
 * over ET (4 NFREQ + 16 bytes per cell) and without a second ET -- the frequency-integrated luminosity of every cell is kept instead:
 *   soc_emitted_change(W, COEFF, stats, bad): for every cell B = sum_f (double)ET[f][c] * W[f], in double with f ascending, every product
 *       and every sum rounded (no fused multiply-add); W[NFREQ] doubles, the integration weights (launch.trapezoid_weight).
 *       L[c] = B * (double)(float)(COEFF[level(c)] * DENS[c]), the float product of soc_set_emission_column, COEFF[LEVELS] as there;
 *       L[c] = 0 where DENS[c] < 1e-10 (links, empty cells), by selection, whatever the row holds; a live cell whose L is negative or not
 *       finite is counted in *bad and gives 0.  With Lp the plane the call before left (all zero after soc_emitted_begin):
 *       stats[0] = sum |L - Lp|, stats[1] = sum L, stats[2] = sum Lp, stats[3] = max |L - Lp| / max(L, Lp) over the cells where
 *       max(L, Lp) > 0 (0 without such a cell).  L then replaces Lp.  One lane per cell, a block's partials reduced in a fixed order and
 *       the blocks' by one workgroup in a fixed order: the same bits on every run and every device.  The plane (8 CELLS bytes) and the
 *       scratch are reserved at the first call after soc_emitted_begin; where they do not fit the free device memory (1 GB kept back, as
 *       soc_emitted_begin) the call fails with SOC_ERR_STATE, the size in GB in the message, and nothing is reserved.
 *       soc_emitted_begin, soc_emitted_end, soc_set_grid and soc_destroy release them;
 *   soc_emitted_read_luminosity(c0, n, L) reads L of cells [c0, c0+n) as the last soc_emitted_change left it, zeros before the first (tests).
 * Both are SOC_ERR_STATE before soc_emitted_begin, SOC_ERR_ARG for a NULL argument or cells outside the grid.  A refused call leaves ET and
 * Lp as they were. */
int soc_emitted_change(soc_ctx *ctx, const double *W, const float *COEFF, double stats[4], int64_t *bad);
int soc_emitted_read_luminosity(soc_ctx *ctx, int64_t c0, int64_t n, double *L);

/* ---- the absorptions of the transfer stage, RESIDENT between the launches that tally them and the multi-dust stage ---- */

/* The mirror image of the above.  A launch leaves the absorptions of one frequency as an INT tally of CELLS floats; the multi-dust stage
 * wants ABS[cells][NFREQ], scaled as the absorbed file holds them (ASOC.py:2793-2809).  Through the host that is, per iteration, a
 * read-back per frequency, a strided add into a row-major array, a copy, a scaling pass and an upload (9.9 GB at 4.95e7 cells x 50
 * frequencies).  Here the sum is held transposed, AT[NFREQ][CELLS]: a frequency is a contiguous row that its tally is added to, and one
 * tiled transpose that scales on the way fills the rows of the multi-dust stage:
 *   soc_absorbed_begin(NFREQ, keep_constant) reserves AT for the cells of the grid (after soc_set_grid), zeroed; with keep_constant != 0
 *       also a second plane AC of the same size.  Where that does not fit the free device memory (1 GB kept back, as soc_emitted_begin)
 *       the call fails with SOC_ERR_STATE, the size in GB in the message, and nothing is reserved or released; a second
 *       soc_absorbed_begin replaces the first; soc_set_grid, soc_absorbed_end and soc_destroy release both planes;
 *   soc_absorbed_add_tally(ifreq) AT[ifreq][:] += the INT tally (what soc_read_tally(SOC_TALLY_INT) reads), one float add per cell,
 *       after deferred launches have run; the tally stays as it is;
 *   soc_absorbed_add_slot(ifreq, k) the same from INT slot k of an ended batch, the buffer soc_batch_read_int(k) reads, with that
 *       call's state checks (SOC_ERR_STATE before soc_batch_end, SOC_ERR_ARG for a slot the batch does not have);
 *   soc_absorbed_keep() copies AT to AC, soc_absorbed_restore() AC to AT, device to device: the constant sources' absorptions, which
 *       every re-emission iteration starts from.  SOC_ERR_STATE without the second plane; _restore also before any _keep;
 *   soc_absorbed_to_mabu(c0, K, nnnlimit) fills all rows of the open soc_mabu_begin from cells [c0, c0 + its cells):
 *       ABS[c][f] = AT[f][c0+c] * (K[level(c0+c)] / DENS[c0+c]), K[LEVELS] = 8^level * FACTOR / (GL*PARSEC) as float, one IEEE division
 *       per cell and one product per value, both rounded to float, no fused multiply-add; -1e20 where DENS <= nnnlimit (a float
 *       comparison: links, cells counted as empty), by selection.  The bits of files.scale_absorbed.  SOC_ERR_STATE without an open
 *       soc_mabu_begin, SOC_ERR_ARG where its NFREQ differs, its cells run past CELLS or K is NULL;
 *   soc_absorbed_download(c0, n, rows, K, nnnlimit) reads rows[n][NFREQ] of cells [c0, c0+n) back through the same kernel; K == NULL:
 *       unscaled, bit for bit what was accumulated;
 *   soc_absorbed_end() frees both planes.
 * Every call but _begin and _end is SOC_ERR_STATE before soc_absorbed_begin; ifreq outside [0, NFREQ), c0 < 0, n < 1 or c0 + n > CELLS
 * are SOC_ERR_ARG.  A refused call leaves AT and AC as they were. */
int soc_absorbed_begin(soc_ctx *ctx, int NFREQ, int keep_constant);
int soc_absorbed_add_tally(soc_ctx *ctx, int ifreq);
int soc_absorbed_add_slot(soc_ctx *ctx, int ifreq, int k);
int soc_absorbed_keep(soc_ctx *ctx);
int soc_absorbed_restore(soc_ctx *ctx);
int soc_absorbed_to_mabu(soc_ctx *ctx, int64_t c0, const float *K, float nnnlimit);
int soc_absorbed_download(soc_ctx *ctx, int64_t c0, int64_t n, float *rows, const float *K, float nnnlimit);
int soc_absorbed_end(soc_ctx *ctx);

/* ---- the library method for dust emission: soc_library.py with kernel_soc_library.c ---- */

/* A model with stochastically heated grains is simulated at three reference frequencies only; the emission of a cell is then
 * looked up in an N x N x N table (2 <= N <= 64, a run-time value: the .lib file carries it) indexed by the log10 of the
 * absorptions at those frequencies.  All arithmetic is fp32 in the order the reference writes it.
 *
 * soc_library_set makes a library resident (the arrays of a .lib file, soc_library.py:279-290): I0, dI0 the first bin centre
 * and the bin width of axis 0, I1[N], dI1[N] those of axis 1 for every i, I2[N*N], dI2[N*N] those of axis 2 for every (i, j),
 * X, Y, Z [N^3] the coordinates of every bin's representative cell, E[N^3][NFREQ] its emission (first value > 1e31: the bin is
 * empty).  ocol, when given, selects and orders nout of the NFREQ emission columns once, at upload (the ofreq.dat subset of
 * soc_library.py:298-306, :392-396); without it nout is taken as NFREQ.  N = 0 forgets the library.
 *
 * soc_library_solve is LibrarySolve with METHOD 0 (kernel_soc_library.c:27-51) with the host loop around it
 * (soc_library.py:379-406) on host arrays: ABS3[n][3] -> EMI[n][nout].  Per cell x = (log10(clamp(a0, 1e-29, 1e10)) - I0) / dI0,
 * i = clamp((int)round(x), 0, N-1) with halves away from zero (a value no int holds clamps by its sign), then y, j from
 * I1[i], dI1[i] and z, k from I2[i*N+j], dI2[i*N+j].  A cell is a miss if one of |x-X|, |y-Y|, |z-Z| at bin k+N*(j+N*i) exceeds
 * 1.1 or the bin is empty; the reference writes element 0 of such a row only, here the row is 1e32 followed by zeros.  miss (room
 * for n entries; may be NULL) receives the missed cells in ascending order, *nmiss their count.
 *
 * soc_library_solve_resident reads the three reference columns col[3] straight out of the absorptions of
 * soc_a2e_resident_begin / _upload and leaves the emission in that family's sum array (soc_a2e_resident_download fetches it):
 * the library's nout must be the row length of the resident arrays. */
int soc_library_set(soc_ctx *ctx, int N, int NFREQ, float I0, float dI0, const float *I1, const float *dI1, const float *I2,
                    const float *dI2, const float *X, const float *Y, const float *Z, const float *E, int nout, const int32_t *ocol);
int soc_library_solve(soc_ctx *ctx, int64_t n, const float *ABS3, float *EMI, int32_t *miss, int64_t *nmiss);
int soc_library_solve_resident(soc_ctx *ctx, const int32_t *col, int32_t *miss, int64_t *nmiss);

/* The grid of a library and the representative cell of every bin (soc_library.py:127-217; there N + N^2 masked passes over all
 * cells on the host and a Python loop over every cell, here four sweeps on the device).  ABS3[cells][3] holds the reference
 * columns, or is NULL and col[3] names them in the resident absorptions (cells must be the resident count).
 *   IREF = log10(clip(a, 1e-25, 1)); I0, dI0 from the minimum and maximum of axis 0 (:137-142); I1[i], dI1[i] from those of
 *   axis 1 over the cells with |IREF0 - (I0 + i*dI0)| < 0.5*dI0 (100, 0.001 without a cell, :146-157); I2, dI2 [N*N] the same on
 *   axis 2 over the cells inside both windows (100, 0.001 with fewer than two cells, :159-170), an undefined (i, j) then taking
 *   the grid of the last defined one in raster order (:178-185); per cell X, I = clip(rint(X)), Y, J, Z, K with halves to even
 *   (numpy's round; the indices are clipped before they index I1 and I2) and dis = |X-I| + |Y-J| + |Z-K| in fp32; per bin the
 *   cell of least dis wins, the lowest index on a tie (:206-213).  IND[N^3] is that cell, -1 where dis > 1.5 or no cell fell
 *   (:217); XX, YY, ZZ [N^3] are the winner's coordinates (0 where no cell fell). */
int soc_library_build(soc_ctx *ctx, int N, int64_t cells, const float *ABS3, const int32_t *col, float *I0, float *dI0, float *I1,
                      float *dI1, float *I2, float *dI2, int32_t *IND, float *XX, float *YY, float *ZZ);

/* ---- the library method for a model with several dust components: a library per dust, one fused look-up ---- */

/* Every dust d of a multi-dust model has its own library (a <dust>.mlib file in the byte layout of .lib), indexed by the log10 of
 * that dust's share of the absorptions at the three reference frequencies,
 * share_f = ABS3[f] * RABS3[f][d] / sum_j ABU[j] * RABS3[f][j] with the types of soc_mabu_split (every product in double, the sum
 * rounded to float after every dust, the quotient in double, rounded once).  One kernel forms the shares, looks every dust up
 * with the arithmetic of soc_library_solve and writes SUM = ((0 + E_0*ABU_0) + E_1*ABU_1) + ...: float products, float sums, in
 * dust order, a dust without an answer adding 0 * ABU_d (what a zeroed row adds on the host).
 *   soc_mabu_library_begin(cells, NDUST, nout, &fit) reserves ABS3[cells][3], ABU[cells][NDUST], SUM[cells][nout] and MISS[cells]
 *       (12 + 4*NDUST + 4*nout + 4 bytes per cell).  1 <= NDUST <= 32, the width of the miss mask, and 1 <= nout <= 4096, else
 *       SOC_ERR_ARG.  *fit (may be NULL) receives the number of cells that fit the free device memory; when `cells` do not, the call
 *       fails with SOC_ERR_STATE and the caller loops over ranges of at most *fit, as with soc_mabu_begin.  A second _begin replaces
 *       the first, the libraries included;
 *   soc_mabu_library_set(idust, N, NFREQ, I0, ..., E, nout, ocol) makes the library of dust idust resident: the arguments of
 *       soc_library_set, E reduced to the nout columns ocol[nout] at upload (ocol NULL: all, and nout is taken as NFREQ); the
 *       number of columns must be the nout of _begin.  2 <= N <= 64;
 *   soc_mabu_library_upload(c0, n, ABS3) fills rows [c0, c0+n) of the absorptions at the reference frequencies (any chunking);
 *   soc_mabu_library_set_tables(ABU, RABS3) uploads ABU[cells][NDUST] and RABS3[3][NDUST] (double), once;
 *   soc_mabu_library_solve() runs the kernel over all cells: SOC_ERR_STATE unless every dust has its library and the tables are set;
 *   soc_mabu_library_download(c0, n, SUM) reads rows [c0, c0+n) of SUM[cells][nout];
 *   soc_mabu_library_misses(c0, n, MISS) reads MISS of those cells: bit d set where dust d had no answer;
 *   soc_mabu_library_end() frees it all.
 * Every call but _begin and _end is SOC_ERR_STATE before soc_mabu_library_begin; rows outside [0, cells) are SOC_ERR_ARG.  The
 * family shares nothing with soc_mabu_begin or soc_library_set: either may be open beside it. */
int soc_mabu_library_begin(soc_ctx *ctx, int64_t cells, int NDUST, int nout, int64_t *cells_fit);
int soc_mabu_library_set(soc_ctx *ctx, int idust, int N, int NFREQ, float I0, float dI0, const float *I1, const float *dI1,
                         const float *I2, const float *dI2, const float *X, const float *Y, const float *Z, const float *E, int nout,
                         const int32_t *ocol);
int soc_mabu_library_upload(soc_ctx *ctx, int64_t c0, int64_t n, const float *ABS3);
int soc_mabu_library_set_tables(soc_ctx *ctx, const float *ABU, const double *RABS3);
int soc_mabu_library_solve(soc_ctx *ctx);
int soc_mabu_library_download(soc_ctx *ctx, int64_t c0, int64_t n, float *SUM);
int soc_mabu_library_misses(soc_ctx *ctx, int64_t c0, int64_t n, uint32_t *MISS);
int soc_mabu_library_end(soc_ctx *ctx);

/* Building such a library is a by-product of the full solve: after a dust's emission is in EM of the open soc_mabu_begin (and
 * soc_library_build has named the representative cells from its share PART),
 *   soc_mabu_gather_rows(idx, n, out) reads out[n][NFREQ] = the rows idx[n] of EM (repeats allowed; an index outside the resident
 *       cells is SOC_ERR_ARG, no open soc_mabu_begin SOC_ERR_STATE). */
int soc_mabu_gather_rows(soc_ctx *ctx, const int32_t *idx, int64_t n, float *out);

/* ---- verification probes (used by the parity tests only) ---- */
/* RNG stream states and first draws of logical work items [gid_first, gid_first+n)
 * (MWC64X_SeedStreams + MWC64X_NextUint, mwc64x_rng.cl:35-48) */
int soc_probe_rng(soc_ctx *ctx, float SEED, uint32_t gid_first, uint32_t n, int ndraw,
                  uint32_t *state_xc, uint32_t *draws);
/* device math header, y[i] = f(x[i]): fn 0 exp, 1 log, 2 sin, 3 cos, 4 acos, 5 sqrt, 6 fmod(x,1), 7 1/x, 8 expm1 (x <= 0),
 * 9 x^1.5, 10 log in fp64, 11 exp_small (-0.34 < x <= 0), 12 log10, 13 floor: the functions of soc_math.h the kernels call */
int soc_probe_math(soc_ctx *ctx, int fn, const float *x, float *y, int64_t n);
/* the two-argument functions, y[i] = f(x[i], x2[i]): fn 14 pown(x, (int)x2), 15 atan2(y = x, x = x2), 16 fmod(x, x2) for
 * x2 > 0 and a quotient below 2^22.  With x2 == NULL
 * this is soc_probe_math; a function called with the wrong number of arguments is refused. */
int soc_probe_math2(soc_ctx *ctx, int fn, const float *x, const float *x2, float *y, int64_t n);
/* follow one ray (IndexG + GetStep until exit); returns the number of steps in *nsteps */
int soc_probe_trace(soc_ctx *ctx, const float pos[3], const float dir[3], int maxsteps,
                    int32_t *levels, int32_t *inds, float *ds, float endpos[3], int32_t *nsteps);

#ifdef __cplusplus
}
#endif
#endif /* SOC_HIP_H */
