// soc_reemit.hip -- the dust emission of one iteration, resident for the next one's cell-emission launches (soc_emitted_*).
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
