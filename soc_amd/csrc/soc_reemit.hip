// soc_reemit.hip -- the dust emission of one iteration, resident for the next one's cell-emission launches (soc_emitted_*), and how
// much it changed since the iteration before (soc_emitted_change_kernel, further down).
//
// The emission leaves the multi-dust stage as SUM[cell][frequency], row-major like the emitted file; SimRAM_CL wants, per frequency,
// EMIT[CELLS].  A column of the row-major array costs a 128-byte line per useful 4 bytes, at every one of NFREQ launches, so the
// resident copy is held transposed, ET[frequency][CELLS], and one tiled transpose per iteration replaces NFREQ strided gathers.
//
// A tile is 64 cells x up to 64 frequencies and goes through LDS.  With NFREQ <= 64 the rows of 64 cells are one contiguous span of
// the row-major side, which the 256 lanes take flat -- consecutive lanes consecutive words, whatever NFREQ is; the transposed side is
// taken one frequency per wave, its 64 lanes 64 consecutive cells (256 bytes).  The LDS row stride is the tile's width made odd: a
// wave's column access then has its 32-lane halves on 32 different banks (ds_read_b32 / ds_write_b32 bank = word address mod 32),
// and the flat access is the identity (odd width) or shifts by one word per row (even width).
#include "soc_dev.h"

#define REEMIT_T  256
#define REEMIT_TC 64            // cells of a tile
#define REEMIT_TF 64            // frequencies of a tile

// level tables of a hierarchy for a kernel that works per cell: the level of cell c is the number of offsets OFF[1..] it has reached
struct SocReemitLevels {
    int   LEVELS;
    int   OFF[SOC_MAXL];
    float COEFF[SOC_MAXL];
};

__device__ __forceinline__ int reemit_level(const SocReemitLevels &L, int c)
{
    int level = 0;
    for (int l = 1; l < L.LEVELS; l++) level += (c >= L.OFF[l]);
    return level;
}

// The element operation of the tile walk on its way from ET into the tile: cell(c) once per lane, apply(that, value) per frequency.
// ReemitCopy: the bits as they are (soc_emitted_*, the unscaled absorptions).
struct ReemitCopy {
    struct Cell {};
    __device__ __forceinline__ Cell cell(long long) const { return Cell{}; }
    __device__ __forceinline__ float apply(const Cell &, float v) const { return v; }
};

// ReemitScale: the absorptions as the absorbed file holds them (files.scale_absorbed, ASOC.py:2793-2809):
// v * (K[level(c)] / DENS[c]), one IEEE division per cell and one product per value, both rounded to float (-ffp-contract=off, and
// hipcc's correctly rounded fp32 division, its default); -1e20 by selection where DENS[c] <= nnnlimit (links, cells counted as empty).
struct ReemitScale {
    SocReemitLevels L;
    const float *DENS;
    float nnnlimit;
    struct Cell { float w;  bool dead; };
    __device__ __forceinline__ Cell cell(long long c) const
    {
        const float d = DENS[c];
        return Cell{ L.COEFF[reemit_level(L, (int)c)] / d, d <= nnnlimit };
    }
    __device__ __forceinline__ float apply(const Cell &k, float v) const { return k.dead ? -1.0e20f : v * k.w; }
};

// ROWS[n][NFREQ] <-> ET[NFREQ][CELLS] at cells [c0, c0 + n).  blockIdx.x: the tile's cells, blockIdx.y: its frequencies.  TO_ROWS
// takes every value through op on its way into the tile (the lane of a cell holds op.cell() of it for all its frequencies)
template <bool TO_ROWS, typename Op>
__global__ __launch_bounds__(REEMIT_T) void soc_reemit_transpose_kernel(long long n, int NFREQ, long long CELLS, long long c0,
                                                                        float *__restrict__ ROWS, float *__restrict__ ET, Op op)
{
    __shared__ float tile[REEMIT_TC * (REEMIT_TF + 1)];
    const long long cb = (long long)blockIdx.x * REEMIT_TC;             // first cell of the tile, counted from c0
    const int f0 = blockIdx.y * REEMIT_TF;
    const int fw = min(REEMIT_TF, NFREQ - f0), cw = (int)min((long long)REEMIT_TC, n - cb);
    const int S = min(REEMIT_TF, NFREQ) | 1;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    float *rows = ROWS + (size_t)cb * NFREQ + f0;
    float *cols = ET + (size_t)f0 * CELLS + c0 + cb;
    if (TO_ROWS) {
        if (tx < cw) {
            const typename Op::Cell k = op.cell(c0 + cb + tx);
            for (int f = ty; f < fw; f += REEMIT_T / 64) tile[tx * S + f] = op.apply(k, cols[(size_t)f * CELLS + tx]);
        }
    } else {
        for (int e = threadIdx.x; e < cw * fw; e += REEMIT_T) {
            const int c = e / fw, f = e - c * fw;
            tile[c * S + f] = rows[(size_t)c * NFREQ + f];
        }
    }
    __syncthreads();
    if (TO_ROWS) {
        for (int e = threadIdx.x; e < cw * fw; e += REEMIT_T) {
            const int c = e / fw, f = e - c * fw;
            rows[(size_t)c * NFREQ + f] = tile[c * S + f];
        }
    } else {
        if (tx < cw)
            for (int f = ty; f < fw; f += REEMIT_T / 64) cols[(size_t)f * CELLS + tx] = tile[tx * S + f];
    }
}

// EMIT[c] = ET[ifreq][c] * (COEFF[level(c)] * DENS[c]), both products rounded to float (the build has -ffp-contract=off): the host's
// EMIT[a:b] *= coeff * DENS[a:b] per level (ASOC.py:1737-1739).  A link or an empty cell (DENS < 1e-10) gets 0 by selection, whatever
// its row holds (ASOC.py:1740: EMIT[DENS < 1e-10] = 0).
__global__ __launch_bounds__(REEMIT_T) void soc_reemit_column_kernel(int CELLS, SocReemitLevels L, const float *__restrict__ DENS,
                                                                     const float *__restrict__ COL, float *__restrict__ EMIT)
{
    for (long long i = blockIdx.x * (long long)REEMIT_T + threadIdx.x; i < CELLS; i += (long long)gridDim.x * REEMIT_T) {
        const int c = (int)i;
        const float d = DENS[c];
        const float w = L.COEFF[reemit_level(L, c)] * d;
        const float v = COL[c] * w;
        EMIT[c] = (d < 1.0e-10f) ? 0.0f : v;
    }
}

// ROW[c] += TALLY[c]: a frequency's INT tally joins its row of the resident absorptions AT[NFREQ][CELLS], one float add per cell
// (FABSORBED[:, f] += TMP on the host).  Row f starts 4 f CELLS bytes into AT -- no 16-byte boundary unless CELLS is a multiple of 4 --
// while the tally starts on one, so the two sides never share an alignment that a wider access could use: one word per lane, a wave
// 256 contiguous bytes of either side.
__global__ __launch_bounds__(REEMIT_T) void soc_absorbed_add_kernel(long long CELLS, const float *__restrict__ TALLY, float *__restrict__ ROW)
{
    for (long long i = blockIdx.x * (long long)REEMIT_T + threadIdx.x; i < CELLS; i += (long long)gridDim.x * REEMIT_T)
        ROW[i] = ROW[i] + TALLY[i];
}

// The change of the emission between two iterations (soc_emitted_change), one pass over ET[NFREQ][CELLS].  One lane per cell, no
// grid-stride loop: the grid, and with it the order of every sum, is a function of CELLS alone.  The lane walks its cell down the rows --
// a wave reads 256 contiguous bytes per row, one word per lane (a row starts on no 16-byte boundary unless CELLS is a multiple of 4, see
// soc_absorbed_add_kernel) -- CHANGE_U rows loaded before the first is used, and accumulates B = sum_f (double)E[c][f] * W[f] in double
// with f ascending, every product and every sum rounded (-ffp-contract=off).  L = B * (double)(float)(COEFF[level] * DENS), the float
// product of soc_reemit_column_kernel; 0 by selection in a link or an empty cell (DENS < 1e-10) whatever its row holds; a live cell
// whose L is negative or not finite counts into BAD and gives 0.  LP[c] is read and replaced by L.  Per block four partials --
// sum |L - LP|, sum L, sum LP, max |L - LP| / max(L, LP) -- reduced in a fixed order: within a wave lane i takes lane i + 32, 16 .. 1,
// then thread 0 takes the waves in their order through LDS.  PART[block][4].
#define CHANGE_T 256            // cells of a block
#define CHANGE_U 8              // rows in flight per lane

__device__ __forceinline__ double change_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ double change_wave_max(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

__global__ __launch_bounds__(CHANGE_T) void soc_emitted_change_kernel(long long CELLS, int NFREQ, SocReemitLevels L, const float *__restrict__ DENS,
                                                                      const float *__restrict__ ET, const double *__restrict__ W,
                                                                      double *__restrict__ LP, double *__restrict__ PART,
                                                                      unsigned long long *__restrict__ BAD)
{
    __shared__ double red[4][CHANGE_T / 64];
    const long long c = (long long)blockIdx.x * CHANGE_T + threadIdx.x;
    double s_abs = 0.0, s_new = 0.0, s_old = 0.0, m = 0.0;
    bool bad = false;
    if (c < CELLS) {
        const float *col = ET + c;
        double B = 0.0;
        int f = 0;
        for (; f + CHANGE_U <= NFREQ; f += CHANGE_U) {
            float e[CHANGE_U];
#pragma unroll
            for (int u = 0; u < CHANGE_U; u++) e[u] = col[(size_t)(f + u) * (size_t)CELLS];
#pragma unroll
            for (int u = 0; u < CHANGE_U; u++) B = B + (double)e[u] * W[f + u];
        }
        for (; f < NFREQ; f++) B = B + (double)col[(size_t)f * (size_t)CELLS] * W[f];
        const float d = DENS[c];
        const float w = L.COEFF[reemit_level(L, (int)c)] * d;
        const double lum = B * (double)w;
        const bool dead = d < 1.0e-10f;
        const bool fine = (lum >= 0.0) && (lum <= 1.7976931348623157e308);       // (false for a NaN)
        bad = !dead && !fine;
        const double l = (dead || !fine) ? 0.0 : lum;
        const double lp = LP[c];
        LP[c] = l;
        const double diff = fabs(l - lp), top = fmax(l, lp);
        s_abs = diff;  s_new = l;  s_old = lp;
        m = (top > 0.0) ? diff / top : 0.0;
    }
    const unsigned long long nbad = __popcll(__ballot(bad));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0 && nbad) atomicAdd(BAD, nbad);
    s_abs = change_wave_sum(s_abs);  s_new = change_wave_sum(s_new);  s_old = change_wave_sum(s_old);  m = change_wave_max(m);
    if (lane == 0) { red[0][wave] = s_abs;  red[1][wave] = s_new;  red[2][wave] = s_old;  red[3][wave] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < CHANGE_T / 64; k++) {
            s_abs = s_abs + red[0][k];  s_new = s_new + red[1][k];  s_old = s_old + red[2][k];  m = fmax(m, red[3][k]);
        }
        double *out = PART + (size_t)blockIdx.x * 4;
        out[0] = s_abs;  out[1] = s_new;  out[2] = s_old;  out[3] = m;
    }
}

// STATS[4] from PART[blocks][4], one workgroup: thread t takes the blocks t, t + CHANGE_T, ... in ascending order, then the threads
// combine as the lanes and waves of the first kernel do -- an order that depends on `blocks` alone.
__global__ __launch_bounds__(CHANGE_T) void soc_emitted_change_final_kernel(long long blocks, const double *__restrict__ PART, double *__restrict__ STATS)
{
    __shared__ double red[4][CHANGE_T / 64];
    double s_abs = 0.0, s_new = 0.0, s_old = 0.0, m = 0.0;
    for (long long b = threadIdx.x; b < blocks; b += CHANGE_T) {
        const double *p = PART + (size_t)b * 4;
        s_abs = s_abs + p[0];  s_new = s_new + p[1];  s_old = s_old + p[2];  m = fmax(m, p[3]);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s_abs = change_wave_sum(s_abs);  s_new = change_wave_sum(s_new);  s_old = change_wave_sum(s_old);  m = change_wave_max(m);
    if (lane == 0) { red[0][wave] = s_abs;  red[1][wave] = s_new;  red[2][wave] = s_old;  red[3][wave] = m; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < CHANGE_T / 64; k++) {
            s_abs = s_abs + red[0][k];  s_new = s_new + red[1][k];  s_old = s_old + red[2][k];  m = fmax(m, red[3][k]);
        }
        STATS[0] = s_abs;  STATS[1] = s_new;  STATS[2] = s_old;  STATS[3] = m;
    }
}

template <bool TO_ROWS, typename Op>
static hipError_t reemit_transpose(long long n, int NFREQ, long long CELLS, long long c0, float *ROWS, float *ET, const Op &op, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (NFREQ < 1 || c0 < 0 || c0 + n > CELLS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + REEMIT_TC - 1) / REEMIT_TC), (unsigned)((NFREQ + REEMIT_TF - 1) / REEMIT_TF));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    soc_reemit_transpose_kernel<TO_ROWS, Op><<<grid, REEMIT_T, 0, st>>>(n, NFREQ, CELLS, c0, ROWS, ET, op);
    return hipGetLastError();
}

hipError_t soc_launch_reemit_to_columns(long long n, int NFREQ, long long CELLS, long long c0, const float *ROWS, float *ET, hipStream_t st)
{
    return reemit_transpose<false>(n, NFREQ, CELLS, c0, const_cast<float *>(ROWS), ET, ReemitCopy{}, st);
}

hipError_t soc_launch_reemit_to_rows(long long n, int NFREQ, long long CELLS, long long c0, const float *ET, float *ROWS, hipStream_t st)
{
    return reemit_transpose<true>(n, NFREQ, CELLS, c0, ROWS, const_cast<float *>(ET), ReemitCopy{}, st);
}

static SocReemitLevels reemit_levels(const SocGrid &G, const float *COEFF)
{
    SocReemitLevels L{};
    L.LEVELS = G.LEVELS;
    for (int l = 0; l < G.LEVELS; l++) { L.OFF[l] = G.OFF[l];  L.COEFF[l] = COEFF[l]; }
    return L;
}

hipError_t soc_launch_absorbed_to_rows(const SocGrid &G, long long n, int NFREQ, long long c0, const float *AT, float *ROWS, const float *K,
                                       float nnnlimit, hipStream_t st)
{
    if (G.CELLS < 1 || G.LEVELS < 1 || G.LEVELS > SOC_MAXL) return hipErrorInvalidValue;
    if (!K) return reemit_transpose<true>(n, NFREQ, G.CELLS, c0, ROWS, const_cast<float *>(AT), ReemitCopy{}, st);
    return reemit_transpose<true>(n, NFREQ, G.CELLS, c0, ROWS, const_cast<float *>(AT), ReemitScale{ reemit_levels(G, K), G.DENS, nnnlimit }, st);
}

hipError_t soc_launch_absorbed_add(long long CELLS, const float *TALLY, float *ROW, hipStream_t st)
{
    if (CELLS < 1 || !TALLY || !ROW) return hipErrorInvalidValue;
    const long long blocks = (CELLS + REEMIT_T - 1) / REEMIT_T;
    soc_absorbed_add_kernel<<<(int)(blocks < 16384 ? blocks : 16384), REEMIT_T, 0, st>>>(CELLS, TALLY, ROW);
    return hipGetLastError();
}

hipError_t soc_launch_reemit_column(const SocGrid &G, const float *COEFF, const float *COL, float *EMIT, hipStream_t st)
{
    if (G.CELLS < 1 || G.LEVELS < 1 || G.LEVELS > SOC_MAXL) return hipErrorInvalidValue;
    const SocReemitLevels L = reemit_levels(G, COEFF);
    const long long blocks = ((long long)G.CELLS + REEMIT_T - 1) / REEMIT_T;
    soc_reemit_column_kernel<<<(int)(blocks < 16384 ? blocks : 16384), REEMIT_T, 0, st>>>(G.CELLS, L, G.DENS, COL, EMIT);
    return hipGetLastError();
}

long long soc_emitted_change_blocks(long long CELLS) { return (CELLS + CHANGE_T - 1) / CHANGE_T; }

hipError_t soc_launch_emitted_change(const SocGrid &G, int NFREQ, const float *COEFF, const float *ET, const double *W, double *LP, double *PART,
                                     double *STATS, unsigned long long *BAD, hipStream_t st)
{
    if (G.CELLS < 1 || G.LEVELS < 1 || G.LEVELS > SOC_MAXL || NFREQ < 1 || !COEFF || !ET || !W || !LP || !PART || !STATS || !BAD) return hipErrorInvalidValue;
    const SocReemitLevels L = reemit_levels(G, COEFF);
    const long long blocks = soc_emitted_change_blocks(G.CELLS);
    soc_emitted_change_kernel<<<(unsigned)blocks, CHANGE_T, 0, st>>>(G.CELLS, NFREQ, L, G.DENS, ET, W, LP, PART, BAD);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    soc_emitted_change_final_kernel<<<1, CHANGE_T, 0, st>>>(blocks, PART, STATS);
    return hipGetLastError();
}
