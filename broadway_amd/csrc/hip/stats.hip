// Picture statistics (include/h264mi.h): moments, extremes, a
// 256-bin histogram and the differences against a reference picture of one
// window (x, y, cw, ch -- all even) per item, as exact integers -- P plane
// records of L = STATS_WORDS (+ STATS_BINS) int64 words each:
//   count, sum, sumsq, min, max, sad, ssd, 0, [hist[0 .. 256)]
// Plane sets: Y (P = 1), YUV (3: chroma at its own 4:2:0 resolution) and RGB
// (3: exactly the uint8 samples of tensor.hip for the same colour set, through
// the same rgba_group_px / rgba_group_px_set).  Input as in tensor.hip: luma
// rows `width` apart, chroma rows `cpitch` apart, item k's picture in_off[k]
// bytes after `in` (and ref_off[k] after `ref`), its window win[k], its record
// out_off[k] bytes after `out`.
//
// The first reduction of the export set.  One pass over the source: a *unit*
// is two rows of STATS_UNIT_COLS columns (and the chroma samples under them),
// 16 bytes per lane, row and picture where the rows start on multiples of 16
// (chroma: 8), else tensor.hip's aligned dwords through v_alignbyte; the last
// unit of a row pair is 2 .. 14 columns wide and loads only what it holds.  An
// item's units in raster order are cut into *strips* of STATS_STRIP_UNITS, one
// workgroup of STATS_THREADS lanes each, grid (strips, items): lane t takes
// units t, t + 256, ... of its strip, so a wave's loads are contiguous and the
// work per workgroup does not depend on the window's width.
//
// Everything is integer.  Per dword of four samples: sum = v_dot4_u32_u8
// against 0x01010101, sumsq = the dword dotted with itself, sad = v_sad_u8,
// ssd = dot(a, a) - 2 dot(a, b) + dot(b, b), min / max on 16-bit pairs
// (v_pk_min_u16 / v_pk_max_u16).  Partials are 32-bit up to the workgroup:
// a strip holds at most STATS_STRIP_UNITS * 2 * STATS_UNIT_COLS samples of a
// plane and 65025 times that is below 2^32 (static_assert below), as is every
// bin.  Lanes reduce through __shfl_xor, waves through LDS words, and a
// workgroup issues one 64-bit global atomic per word it touched.  Histogram:
// wave-private 32-bit LDS bins under ds_add, summed once per workgroup; before
// the add, a dword of four equal bytes is one add of 4, and a wave whose lanes
// all hold that same dword is one add by one lane (a flat region would
// otherwise serialise 64 lanes on one bin).
//
// k_stats_init, ahead of k_stats on the same stream, writes every word of every
// record -- count, min = 255, zeros, empty bins --, so the result does not
// depend on what the destination held.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "color.hip"
#include "crop.hip"
#include "tensor.hip"

#define STATS_WORDS 8               // words of a plane record ahead of the histogram
#define STATS_BINS 256
#define STATS_THREADS 256
#define STATS_UNIT_COLS 16          // a unit: two rows of 16 columns
#define STATS_LANE_UNITS 4          // units a lane takes
#define STATS_STRIP_UNITS (STATS_THREADS * STATS_LANE_UNITS)      // units a workgroup takes
#define STATS_MAX_ITEMS TENSOR_MAX_PICS

static_assert((unsigned long long)STATS_STRIP_UNITS * 2 * STATS_UNIT_COLS * 255 * 255 < (1ull << 32),
              "a workgroup's sums of squares and products fit 32 bits");

enum { STATS_Y = 0, STATS_YUV = 1, STATS_RGB = 2 };
// words of a plane record; a workgroup's LDS totals use the same indices, with 6 and 7 the two products ssd is made of
enum { STATS_COUNT = 0, STATS_SUM = 1, STATS_SUMSQ = 2, STATS_MIN = 3, STATS_MAX = 4, STATS_SAD = 5, STATS_SSD = 6,
       STATS_T_AB = 6, STATS_T_BB = 7 };

struct stats_args {
    const uint8_t *in, *ref;        // ref: REF kernels only
    uint8_t *out;
    int width, height, cpitch;
    colour_set col;                 // COL kernels only (tensor_colour_sets[id], id != 0)
    unsigned long long in_off[STATS_MAX_ITEMS], ref_off[STATS_MAX_ITEMS], out_off[STATS_MAX_ITEMS];
    int win[STATS_MAX_ITEMS][4];    // grid row k's window (x, y, cw, ch)
};

typedef unsigned short stats_u16x2 __attribute__((ext_vector_type(2)));

// a lane's partials of one plane
struct stats_part {
    uint32_t sum, sq, mn, mx, sad, ab, bb;      // mn, mx: two 16-bit lanes
};

__device__ __forceinline__ uint32_t stats_dot(uint32_t a, uint32_t b, uint32_t c)
{
    return __builtin_amdgcn_udot4(a, b, c, false);
}

// the first c bytes (0 .. 4) at s, the rest zero; nothing else is read beyond the aligned dwords holding them
__device__ __forceinline__ uint32_t stats_load_bytes(const uint8_t *s, int c)
{
    if (c >= 4) return crop_load4(s);
    if (c == 3) return crop_load2(s) | (uint32_t)s[2] << 16;
    if (c == 2) return crop_load2(s);
    return c == 1 ? (uint32_t)s[0] : 0u;
}

// the n bytes (1 .. 4 * NW) at s into d, zero behind them; vec: s is a multiple of 4 * NW
template <int NW>
__device__ __forceinline__ void stats_load(const uint8_t *s, int n, bool vec, uint32_t (&d)[NW])
{
    static_assert(NW == 2 || NW == 4, "8 or 16 bytes per lane");
    if (n == 4 * NW) {
        if (vec) {
            if constexpr (NW == 4) {
                const crop_u32x4 q = *(const crop_u32x4 *)s;
                d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
            } else {
                const crop_u32x2 q = *(const crop_u32x2 *)s;
                d[0] = q.x; d[1] = q.y;
            }
        } else {
            tensor_load<NW>(s, d);
        }
    } else {
#pragma unroll
        for (int j = 0; j < NW; j++) d[j] = stats_load_bytes(s + 4 * j, n - 4 * j);
    }
}

// four samples a (and r of the reference), the first c (1 .. 4) of them in the window -- the others zero in both --,
// into a lane's partials and (HIST) the wave's bins
template <bool HIST, bool REF>
__device__ __forceinline__ void stats_dword(stats_part &P, uint32_t *bins, uint32_t a, uint32_t r, int c)
{
    if (c <= 0) return;
    const uint32_t m = c >= 4 ? 0xFFFFFFFFu : (1u << (8 * c)) - 1u;
    P.sum = stats_dot(a, 0x01010101u, P.sum);
    P.sq = stats_dot(a, a, P.sq);
    const uint32_t lo = a | ~m;                 // (a sample outside the window never is the minimum)
    P.mn = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(stats_u16x2, P.mn),
                                                                  __builtin_bit_cast(stats_u16x2, lo & 0x00FF00FFu)));
    P.mn = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(stats_u16x2, P.mn),
                                                                  __builtin_bit_cast(stats_u16x2, (lo >> 8) & 0x00FF00FFu)));
    P.mx = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(stats_u16x2, P.mx),
                                                                  __builtin_bit_cast(stats_u16x2, a & 0x00FF00FFu)));
    P.mx = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(stats_u16x2, P.mx),
                                                                  __builtin_bit_cast(stats_u16x2, (a >> 8) & 0x00FF00FFu)));
    if constexpr (REF) {
        P.sad = __builtin_amdgcn_sad_u8(a, r, P.sad);
        P.ab = stats_dot(a, r, P.ab);
        P.bb = stats_dot(r, r, P.bb);
    }
    if constexpr (HIST) {
        const bool flat = c >= 4 && a == (a & 255u) * 0x01010101u;
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
        const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
        if (__builtin_amdgcn_ballot_w64(flat && a == first) == act) {
            // the wave's active lanes hold one value four times each: one add, by the first of them
            if ((int)(threadIdx.x & 63u) == __ffsll(act) - 1) atomicAdd(&bins[first & 255u], 4u * (uint32_t)__popcll(act));
        } else if (flat) {
            atomicAdd(&bins[a & 255u], 4u);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (i < c) atomicAdd(&bins[(a >> (8 * i)) & 255u], 1u);
        }
    }
}

__device__ __forceinline__ uint32_t stats_wave_add(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ uint32_t stats_wave_min(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) { const uint32_t w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}

__device__ __forceinline__ uint32_t stats_wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o; o >>= 1) { const uint32_t w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}

// plane p's four samples of pixel words o[0 .. 4) (bytes R G B A), each an opaque value first: as in tensor_store,
// the compiler would otherwise form v_ashr_pk_u8_i32 from the converter's clamps and OR bytes 2 and 3 into it
__device__ __forceinline__ uint32_t stats_plane_dword(const uint32_t (&o)[4], int p)
{
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint32_t v = (o[i] >> (8 * p)) & 255u;
        asm("" : "+v"(v));
        w |= v << (8 * i);
    }
    return w;
}

// one picture's unit at (row pair y2, group g), n columns (even, 2 .. 16): d[p][row][k] = plane p's dword k of the
// unit's row (chroma planes of YUV: row 0, dwords 0 and 1, n / 2 samples); bytes outside the window are zero
template <int PLANES, bool COL>
__device__ __forceinline__ void stats_unit(const stats_args &a, const uint8_t *Y, const uint8_t *U, const uint8_t *V,
                                           bool vy, bool vc, int y2, int g, int n, uint32_t (&d)[3][2][4])
{
    const uint8_t *sy = Y + (size_t)(2 * y2) * a.width + STATS_UNIT_COLS * g;
    uint32_t y0[4], y1[4], u[2], v[2];
    stats_load<4>(sy, n, vy, y0);
    stats_load<4>(sy + a.width, n, vy, y1);
    if constexpr (PLANES != STATS_Y) {
        const size_t co = (size_t)y2 * a.cpitch + (STATS_UNIT_COLS / 2) * g;
        stats_load<2>(U + co, n >> 1, vc, u);
        stats_load<2>(V + co, n >> 1, vc, v);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if constexpr (PLANES == STATS_RGB) {
            uint32_t o0[4], o1[4];
            const uint32_t u2 = (u[k >> 1] >> (16 * (k & 1))) & 0xFFFFu, v2 = (v[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
            if constexpr (COL) rgba_group_px_set(a.col, y0[k], y1[k], u2, v2, o0, o1);
            else rgba_group_px(y0[k], y1[k], u2, v2, o0, o1);
            // (the converter makes pixels of the zeros outside the window too)
            const int c = n - 4 * k;
            const uint32_t m = c >= 4 ? 0xFFFFFFFFu : c == 2 ? 0xFFFFu : 0u;
#pragma unroll
            for (int p = 0; p < 3; p++) {
                d[p][0][k] = stats_plane_dword(o0, p) & m;
                d[p][1][k] = stats_plane_dword(o1, p) & m;
            }
        } else {
            d[0][0][k] = y0[k];
            d[0][1][k] = y1[k];
        }
    }
    if constexpr (PLANES == STATS_YUV) {
        d[1][0][0] = u[0]; d[1][0][1] = u[1];
        d[2][0][0] = v[0]; d[2][0][1] = v[1];
    }
}

// every word of the records of grid row k: blocks (items of this launch), STATS_THREADS lanes
__global__ __launch_bounds__(STATS_THREADS) void k_stats_init(const stats_args a, int planes, int hist)
{
    const int item = blockIdx.x;
    const int L = STATS_WORDS + (hist ? STATS_BINS : 0), np = planes == STATS_Y ? 1 : 3;
    const unsigned long long cw = (unsigned long long)a.win[item][2], ch = (unsigned long long)a.win[item][3];
    unsigned long long *O = (unsigned long long *)(a.out + a.out_off[item]);
    for (int i = (int)threadIdx.x; i < np * L; i += STATS_THREADS) {
        const int p = i / L, w = i - p * L;
        unsigned long long v = 0;
        if (w == STATS_COUNT) v = planes == STATS_YUV && p ? (cw >> 1) * (ch >> 1) : cw * ch;
        else if (w == STATS_MIN) v = 255;
        O[i] = v;
    }
}

// grid: (strips, items of this launch), STATS_THREADS lanes; behind k_stats_init of the same items
template <int PLANES, bool HIST, bool REF, bool COL = false>
__global__ __launch_bounds__(STATS_THREADS) void k_stats(const stats_args a)
{
    static_assert(!COL || PLANES == STATS_RGB, "a colour set goes with RGB");
    constexpr int NP = PLANES == STATS_Y ? 1 : 3;
    constexpr int L = STATS_WORDS + (HIST ? STATS_BINS : 0);
    constexpr int WAVES = STATS_THREADS / 64;
    __shared__ uint32_t tot[3][STATS_WORDS];
    __shared__ uint32_t bins[HIST ? WAVES * NP * STATS_BINS : 1];
    const int item = blockIdx.y, tid = (int)threadIdx.x;
    const int x = a.win[item][0], y = a.win[item][1], cw = a.win[item][2], ch = a.win[item][3];
    const int ni = (cw + STATS_UNIT_COLS - 1) / STATS_UNIT_COLS;       // units per row pair
    const int nf = ni * (ch >> 1);
    const int f0 = (int)blockIdx.x * STATS_STRIP_UNITS;
    if (f0 >= nf) return;               // (the grid covers the launch's largest item)
    if (tid < 3 * STATS_WORDS) tot[tid / STATS_WORDS][tid % STATS_WORDS] = tid % STATS_WORDS == STATS_MIN ? 255u : 0u;
    if constexpr (HIST)
        for (int i = tid; i < WAVES * NP * STATS_BINS; i += STATS_THREADS) bins[i] = 0;
    __syncthreads();

    const size_t cplane = (size_t)a.cpitch * (a.height >> 1);
    const size_t yo = (size_t)y * a.width + x, co = (size_t)a.width * a.height + (size_t)(y >> 1) * a.cpitch + (x >> 1);
    const uint8_t *Y = a.in + a.in_off[item] + yo, *U = a.in + a.in_off[item] + co, *V = U + cplane;
    const bool vy = !(((uintptr_t)Y | (uintptr_t)a.width) & 15u);
    const bool vc = !(((uintptr_t)U | (uintptr_t)V | (uintptr_t)a.cpitch) & 7u);
    const uint8_t *RY = Y, *RU = U, *RV = V;
    bool rvy = false, rvc = false;
    if constexpr (REF) {
        RY = a.ref + a.ref_off[item] + yo; RU = a.ref + a.ref_off[item] + co; RV = RU + cplane;
        rvy = !(((uintptr_t)RY | (uintptr_t)a.width) & 15u);
        rvc = !(((uintptr_t)RU | (uintptr_t)RV | (uintptr_t)a.cpitch) & 7u);
    }

    stats_part P[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) P[p] = {0u, 0u, 0x00FF00FFu, 0u, 0u, 0u, 0u};
    uint32_t *wbins = bins + (HIST ? (tid >> 6) * NP * STATS_BINS : 0);
#pragma unroll 1
    for (int j = 0; j < STATS_LANE_UNITS; j++) {
        const int f = f0 + j * STATS_THREADS + tid;
        if (f >= nf) break;
        const int y2 = f / ni, g = f - y2 * ni;
        const int n = cw - STATS_UNIT_COLS * g < STATS_UNIT_COLS ? cw - STATS_UNIT_COLS * g : STATS_UNIT_COLS;
        uint32_t s[3][2][4], r[3][2][4];
        stats_unit<PLANES, COL>(a, Y, U, V, vy, vc, y2, g, n, s);
        if constexpr (REF) stats_unit<PLANES, COL>(a, RY, RU, RV, rvy, rvc, y2, g, n, r);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const bool chroma = PLANES == STATS_YUV && p > 0;
#pragma unroll
            for (int h = 0; h < (chroma ? 1 : 2); h++)
#pragma unroll
                for (int k = 0; k < (chroma ? 2 : 4); k++)
                    stats_dword<HIST, REF>(P[p], wbins + (HIST ? p * STATS_BINS : 0), s[p][h][k], REF ? r[p][h][k] : 0u,
                                           (chroma ? n >> 1 : n) - 4 * k);
        }
    }

    // lanes -> wave (cross-lane), waves -> workgroup (LDS words)
#pragma unroll
    for (int p = 0; p < NP; p++) {
        const uint32_t mn = P[p].mn & 0xFFFFu, mn1 = P[p].mn >> 16, mx = P[p].mx & 0xFFFFu, mx1 = P[p].mx >> 16;
        const uint32_t sum = stats_wave_add(P[p].sum), sq = stats_wave_add(P[p].sq);
        const uint32_t lo = stats_wave_min(mn < mn1 ? mn : mn1), hi = stats_wave_max(mx > mx1 ? mx : mx1);
        uint32_t sad = 0, ab = 0, bb = 0;
        if constexpr (REF) { sad = stats_wave_add(P[p].sad); ab = stats_wave_add(P[p].ab); bb = stats_wave_add(P[p].bb); }
        if ((tid & 63) == 0) {
            atomicAdd(&tot[p][STATS_SUM], sum);
            atomicAdd(&tot[p][STATS_SUMSQ], sq);
            atomicMin(&tot[p][STATS_MIN], lo);
            atomicMax(&tot[p][STATS_MAX], hi);
            if constexpr (REF) {
                atomicAdd(&tot[p][STATS_SAD], sad);
                atomicAdd(&tot[p][STATS_T_AB], ab);
                atomicAdd(&tot[p][STATS_T_BB], bb);
            }
        }
    }
    __syncthreads();

    // workgroup -> record: one global atomic per word this strip touched
    unsigned long long *O = (unsigned long long *)(a.out + a.out_off[item]);
    if (tid < NP * STATS_WORDS) {
        const int p = tid / STATS_WORDS, w = tid % STATS_WORDS;
        unsigned long long *o = O + (size_t)p * L + w;
        const unsigned long long t = tot[p][w];
        if (w == STATS_SUM || w == STATS_SUMSQ || (REF && w == STATS_SAD)) atomicAdd(o, t);
        else if (w == STATS_MIN) atomicMin(o, t);
        else if (w == STATS_MAX) atomicMax(o, t);
        else if (REF && w == STATS_SSD)     // exact: each term is below 2^32 and the whole is a sum of squares
            atomicAdd(o, (unsigned long long)tot[p][STATS_SUMSQ] + tot[p][STATS_T_BB] - 2ull * tot[p][STATS_T_AB]);
    }
    if constexpr (HIST) {
        for (int i = tid; i < NP * STATS_BINS; i += STATS_THREADS) {
            uint32_t c = 0;
#pragma unroll
            for (int w = 0; w < WAVES; w++) c += bins[w * NP * STATS_BINS + i];
            if (c) atomicAdd(O + (size_t)(i / STATS_BINS) * L + STATS_WORDS + (i % STATS_BINS), (unsigned long long)c);
        }
    }
}

// the two launches for n items whose largest has `strips` strips
static void stats_launch(int planes, bool hist, bool ref, bool col, int strips, int n, hipStream_t st, const stats_args &a)
{
    hipLaunchKernelGGL(k_stats_init, dim3(n), dim3(STATS_THREADS), 0, st, a, planes, (int)hist);
    const dim3 grid(strips, n), block(STATS_THREADS);
#define STATS_CASE(P, C)                                                                                  \
    if (planes == P && col == C) {                                                                        \
        if (hist && ref) hipLaunchKernelGGL((k_stats<P, true, true, C>), grid, block, 0, st, a);          \
        else if (hist) hipLaunchKernelGGL((k_stats<P, true, false, C>), grid, block, 0, st, a);           \
        else if (ref) hipLaunchKernelGGL((k_stats<P, false, true, C>), grid, block, 0, st, a);            \
        else hipLaunchKernelGGL((k_stats<P, false, false, C>), grid, block, 0, st, a);                    \
        return;                                                                                           \
    }
    STATS_CASE(STATS_Y, false) STATS_CASE(STATS_YUV, false) STATS_CASE(STATS_RGB, false) STATS_CASE(STATS_RGB, true)
#undef STATS_CASE
}
