// Resized accumulated-motion and accumulated-residual exports (include/h264mi.h,
// DESIGN 3.5i): the integer field v of accmv.hip's / accres.hip's export over
// its window, filtered to (oh, ow) samples per channel or plane by resize.hip's
// triangle filter (its taps, unchanged) with no intermediate rounding, then the
// field exports' elements:
//   acc = sum_l qy_l * (sum_k qx_k * s[l][k])      (inner sum < 2^29: 32 bits; acc < 2^43: 64 bits)
//   r   = (acc + 2^23) >> 24                       (the filtered value in units of 1 / 16)
//   int16 (r + 8) >> 4;  float types fma((float)r * 0.0625f, scale[c], bias[c])
// The source grid is the window's, cw x ch samples, or for accres' UV planes its
// half-resolution grid, cw / 2 x ch / 2.
//
// k_field_resize is k_tensor_resize's skeleton with two sample sources.  A
// workgroup of 256 threads makes one RESIZE_TW x RESIZE_TH tile of one
// picture's output:
//   taps      resize_taps into LDS, as in k_tensor_resize;
//   per chunk of 1..16 source rows (as many as fit the staging buffer):
//   stage     one dword per source sample, rows an odd number of dwords apart;
//             an item is 4 consecutive samples of a row, NIT items per thread
//             and round, their map loads issued together.
//             accmv: the map word itself (one 16-byte load on a 4-byte boundary).
//             accres: the planes' v, each + 255, in three 10-bit fields, from
//             accres_group -- the map, current and key fetches, the clamp, the
//             policy and the colour conversion of the unresized export.
//             A group that would reach past the window's last column takes its
//             samples one by one, the last column repeated (no tap reads the
//             repeats), so nothing outside the window's words is read and
//             accres.hip's argument about what a fetch may touch holds as it is;
//   horizontal  one lane per (source row, output column), rows fastest, four
//             taps per iteration, 32-bit sums.  The channels are linear in the
//             sample, so accmv sums q * JX, q * JY, q * ANCHORED and q * k (k the
//             tap's index: the sample's x is known from its position) and
//             derives ADX = sum q JX - sum q x and ADY = sum q JY - 16384 y from
//             them (sum q = 16384); accres sums the biased fields and takes 255
//             * 16384 off.  t is int32 [plane][column][row], unrounded, columns
//             FRESIZE_TPITCH (odd) dwords apart: the vertical pass's lanes over
//             columns read different banks;
//   vertical  one lane per (output row, output column), two per thread and
//             plane, adds the chunk's rows of its taps to 64-bit accumulators
//             in registers (v_mad_i64_i32); only the planes some output channel
//             needs are written and read;
//   at the end: round, fresize_elem<DT>, one non-temporal store per element.
// A picture without a key (accres) skips the chunks: it reads nothing and
// stores fma(0, scale, bias).

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "crop.hip"
#include "tensor.hip"
#include "resize.hip"
#include "field_store.h"
#include "accmv.hip"
#include "accres.hip"
#define FRESIZE_TPITCH (RESIZE_ROWS + 1)    // int32 per column of t
#define FRESIZE_STAGE_DW 5120               // staging buffer: 4 rows of the widest tile (32 : 1, 1065 dwords a row), 16 rows of
                                            // 1080p -> 224 (293); with it accmv's 37.9 KB of LDS leave room for 4 workgroups per CU

// r (the filtered value in units of 1 / 16) as the element type's bits
template <int DT>
__device__ __forceinline__ uint32_t fresize_elem(int r, float s, float b)
{
    if constexpr (DT == TENSOR_I16) {
        return (uint32_t)((r + 8) >> 4) & 0xFFFFu;
    } else {
        float f = __builtin_fmaf((float)r * 0.0625f, s, b);
        // the fp32 result as the definition has it, rounded, before the conversion:
        // left to itself the compiler folds fma and conversion into one
        // v_fma_mixlo_f16, which rounds the exact sum to fp16 once
        asm volatile("" : "+v"(f));
        return tensor_float_bits<DT>(f);
    }
}

// The two sample sources.  NB: planes of t; NH: sums of the horizontal pass;
// NIT: items per thread and staging round; MAX_OUT: output channels at most.
struct fresize_accmv {
    typedef accmv_args args;
    static constexpr int NB = ACC_NCHANNELS, NH = 4, NIT = 4, MAX_OUT = ACCMV_MAX_CH;

    static __device__ __forceinline__ int hs(const args &) { return 0; }
    static __device__ __forceinline__ bool has_source(const args &, int) { return true; }
    static __device__ __forceinline__ int nout(const args &a) { return a.nch; }
    static __device__ __forceinline__ int plane_of(const args &a, int c) { return a.id[c]; }
    static __device__ __forceinline__ unsigned mask(const args &a)
    {
        unsigned m = 0;
        for (int c = 0; c < a.nch; c++) m |= 1u << a.id[c];
        return m;
    }

    // items it0 + tid + 256 u, u < NIT, of the chunk's nit (rows r0.., ng groups from window column xs0 each)
    static __device__ __forceinline__ void stage(const args &a, int pic, uint32_t *stage, int pitch, int ng, int nit,
                                                 int it0, int xs0, int r0, int tid)
    {
        accmv_gu32 *M = (accmv_gu32 *)(uintptr_t)(a.maps + a.off[pic]) + (size_t)a.y * a.W + a.x;
        crop_u32x4 w[NIT];
        int so[NIT];
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int t = it0 + tid + RESIZE_THREADS * i, it = t < nit ? t : nit - 1;
            const int pr = it / ng, g = it - pr * ng, c = xs0 + 4 * g;
            accmv_gu32 *row = M + (size_t)(r0 + pr) * a.W;
            if (c + 4 <= a.cw) {
                w[i] = *(accmv_gu32x4 *)(row + c);
            } else {
                const int l = a.cw - 1;
                w[i].x = row[c];
                w[i].y = row[c + 1 < l ? c + 1 : l];
                w[i].z = row[c + 2 < l ? c + 2 : l];
                w[i].w = row[l];
            }
            so[i] = pr * pitch + 4 * g;
        }
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            if (it0 + tid + RESIZE_THREADS * i < nit) {
                uint32_t *s = stage + so[i];
                s[0] = w[i].x; s[1] = w[i].y; s[2] = w[i].z; s[3] = w[i].w;
            }
        }
    }

    // tap k (weight q) of a staged sample d into the sums h
    static __device__ __forceinline__ void tap(int (&h)[NH], int q, uint32_t d, int k)
    {
        h[0] += q * (int)(d & 0x7FFFu);
        h[1] += q * (int)((d >> 16) & 0x7FFFu);
        h[2] += q * (int)(d >> 31);
        h[3] += q * k;
    }

    // the planes' sums t of an output whose first tap is the sample (X, Y) of the picture
    static __device__ __forceinline__ void planes(const int (&h)[NH], int X, int Y, int (&t)[NB])
    {
        t[ACC_ADX] = h[0] - (16384 * X + h[3]);
        t[ACC_ADY] = h[1] - 16384 * Y;
        t[ACC_JX] = h[0];
        t[ACC_JY] = h[1];
        t[ACC_ANCHORED] = h[2];
    }
};

struct fresize_accres {
    typedef accres_args args;
    static constexpr int NB = 3, NH = 3, NIT = 2, MAX_OUT = 3;

    static __device__ __forceinline__ int hs(const args &a) { return a.planes == ACCRES_UV ? 1 : 0; }
    static __device__ __forceinline__ bool has_source(const args &a, int pic) { return a.key_off[pic] != ACCRES_NO_KEY; }
    static __device__ __forceinline__ int nout(const args &a) { return a.planes == ACCRES_Y ? 1 : a.planes == ACCRES_UV ? 2 : 3; }
    static __device__ __forceinline__ int plane_of(const args &, int c) { return c; }
    static __device__ __forceinline__ unsigned mask(const args &a) { return (1u << nout(a)) - 1u; }

    static __device__ __forceinline__ void stage(const args &a, int pic, uint32_t *stage, int pitch, int ng, int nit,
                                                 int it0, int xs0, int r0, int tid)
    {
        const int sh = hs(a), gw = a.cw >> sh;
        const accres_frame C = accres_planes(a.cur, a.cur_off[pic], a.W, a.H, a.cpitch);
        const accres_frame K = accres_planes(a.key, a.key_off[pic], a.W, a.H, a.cpitch);
        accres_gu32 *M = (accres_gu32 *)(uintptr_t)(a.maps + a.map_off[pic]);
        uint32_t w[NIT][4];
        int so[NIT], X[NIT], Y[NIT], c[NIT];
        // the map words of every item first: the key fetches depend on them
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            const int t = it0 + tid + RESIZE_THREADS * i, it = t < nit ? t : nit - 1;
            const int pr = it / ng, g = it - pr * ng;
            c[i] = xs0 + 4 * g;
            X[i] = a.x + (c[i] << sh); Y[i] = a.y + ((r0 + pr) << sh);
            accres_gu32 *src = M + (size_t)Y[i] * a.W + X[i];
            if (c[i] + 4 <= gw) {
                if (sh) {
                    const crop_u32x4 lo = *(accres_gu32x4 *)src, hi = *(accres_gu32x4 *)(src + 4);
                    w[i][0] = lo.x; w[i][1] = lo.z; w[i][2] = hi.x; w[i][3] = hi.z;
                } else {
                    const crop_u32x4 v = *(accres_gu32x4 *)src;
                    w[i][0] = v.x; w[i][1] = v.y; w[i][2] = v.z; w[i][3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) w[i][k] = src[(c[i] + k < gw ? k : gw - 1 - c[i]) << sh];
            }
            so[i] = pr * pitch + 4 * g;
        }
#pragma unroll
        for (int i = 0; i < NIT; i++) {
            int v[3][4];
            if (c[i] + 4 <= gw) {
                accres_group<4>(a, C, K, w[i], X[i], Y[i], v);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint32_t w1[1] = {w[i][k]};
                    int q[3][1];
                    accres_group<1>(a, C, K, w1, X[i] + ((c[i] + k < gw ? k : gw - 1 - c[i]) << sh), Y[i], q);
                    v[0][k] = q[0][0]; v[1][k] = q[1][0]; v[2][k] = q[2][0];
                }
            }
            if (it0 + tid + RESIZE_THREADS * i < nit) {
                uint32_t *s = stage + so[i];
#pragma unroll
                for (int k = 0; k < 4; k++)
                    s[k] = (uint32_t)(v[0][k] + 255) | (uint32_t)(v[1][k] + 255) << 10 | (uint32_t)(v[2][k] + 255) << 20;
            }
        }
    }

    static __device__ __forceinline__ void tap(int (&h)[NH], int q, uint32_t d, int)
    {
        h[0] += q * (int)(d & 1023u);
        h[1] += q * (int)((d >> 10) & 1023u);
        h[2] += q * (int)((d >> 20) & 1023u);
    }

    static __device__ __forceinline__ void planes(const int (&h)[NH], int, int, int (&t)[NB])
    {
#pragma unroll
        for (int p = 0; p < NB; p++) t[p] = h[p] - 255 * 16384;
    }
};

template <class S>
struct fresize_args {
    typename S::args f;
    int ow, oh;
};

// grid: (tiles of RESIZE_TW x RESIZE_TH outputs in raster order, pictures of
// this launch), 256 threads
template <class S, int DT>
__global__ __launch_bounds__(RESIZE_THREADS) void k_field_resize(const fresize_args<S> ra)
{
    constexpr int ES = tensor_elem_size(DT);
    constexpr int NB = S::NB;
    static_assert(RESIZE_TW == 32 && RESIZE_TH * RESIZE_TW == 2 * RESIZE_THREADS, "item -> (row, column) below");
    static_assert(ES == 2 || ES == 4, "a field element is 16 or 32 bits");
    __shared__ uint32_t stage[FRESIZE_STAGE_DW + 4];         // (+ 4: the zero-weight taps behind the last row's last)
    __shared__ uint16_t qx[RESIZE_MAX_TAPS * RESIZE_TW], qy[RESIZE_MAX_TAPS * RESIZE_TH];
    __shared__ int32_t tb[NB * RESIZE_TW * FRESIZE_TPITCH];
    __shared__ int fx[RESIZE_TW], cx[RESIZE_TW], fy[RESIZE_TH], cy[RESIZE_TH];
    const typename S::args &a = ra.f;
    const int tid = (int)threadIdx.x, pic = (int)blockIdx.y;
    const int sh = S::hs(a), gw = a.cw >> sh, gh = a.ch >> sh, ow = ra.ow, oh = ra.oh;
    const int ntx = (ow + RESIZE_TW - 1) / RESIZE_TW;
    const int ty = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - ty * ntx;
    const int ox0 = tx * RESIZE_TW, oy0 = ty * RESIZE_TH;
    const int nx = ow - ox0 < RESIZE_TW ? ow - ox0 : RESIZE_TW, ny = oh - oy0 < RESIZE_TH ? oh - oy0 : RESIZE_TH;
    const unsigned mask = S::mask(a);

    long long acc[NB][2];
#pragma unroll
    for (int b = 0; b < NB; b++) acc[b][0] = acc[b][1] = 0;

    if (S::has_source(a, pic)) {
        if (tid < RESIZE_TW + RESIZE_TH) {
            const bool isx = tid < RESIZE_TW;
            const int l = isx ? tid : tid - RESIZE_TW;
            int f = 0, c = 0;
            if (l < (isx ? nx : ny))
                resize_taps((uint32_t)(isx ? gw : gh), (uint32_t)(isx ? ow : oh), (uint32_t)((isx ? ox0 : oy0) + l),
                            (isx ? qx : qy) + l, isx ? RESIZE_TW : RESIZE_TH, f, c);
            (isx ? fx : fy)[l] = f;
            (isx ? cx : cy)[l] = c;
        }
        __syncthreads();

        // the tile's source columns [xs0, xs0 + segw) (4-column groups of the
        // grid) and rows [ys0, ye): first taps and tap ends grow with the output index
        const int xs0 = fx[0] & ~3, segw = (fx[nx - 1] + cx[nx - 1] - xs0 + 3) & ~3, pitch = segw | 1, ng = segw >> 2;
        const int ys0 = fy[0], ye = fy[ny - 1] + cy[ny - 1];
        int lrc = 4;                                    // log2 of the chunk's rows
        while (lrc > 0 && (pitch << lrc) > FRESIZE_STAGE_DW) lrc--;
        const int rc = 1 << lrc;

        for (int r0 = ys0; r0 < ye; r0 += rc) {
            const int nr = ye - r0 < rc ? ye - r0 : rc;         // source rows of this chunk
            // stage: (row, 4-column group) items, groups fastest
            const int nit = nr * ng;
            for (int it0 = 0; it0 < nit; it0 += RESIZE_THREADS * S::NIT)
                S::stage(a, pic, stage, pitch, ng, nit, it0, xs0, r0, tid);
            __syncthreads();
            // horizontal: (source row, output column) items, rows fastest
            for (int it = tid; it < (RESIZE_TW << lrc); it += RESIZE_THREADS) {
                const int r = it & (rc - 1), j = it >> lrc;
                if (r >= nr || j >= nx) continue;
                const uint32_t *s = stage + r * pitch + (fx[j] - xs0);
                const int n = cx[j];
                int h[S::NH];
#pragma unroll
                for (int p = 0; p < S::NH; p++) h[p] = 0;
                // four taps at a time, their LDS reads in flight together; behind
                // the last tap: weight 0 times whatever the buffer holds
                for (int k = 0; k < n; k += 4) {
                    uint32_t d[4];
                    int q[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        d[u] = s[k + u];
                        q[u] = (int)qx[(k + u) * RESIZE_TW + j];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) S::tap(h, q[u], d[u], k + u);
                }
                int t[NB];
                S::planes(h, a.x + (fx[j] << sh), a.y + ((r0 + r) << sh), t);
#pragma unroll
                for (int b = 0; b < NB; b++)
                    if ((mask >> b) & 1u) tb[(b * RESIZE_TW + j) * FRESIZE_TPITCH + r] = t[b];
            }
            __syncthreads();
            // vertical: outputs (row (tid >> 5) + 8 e, column tid & 31), e < 2, of
            // every plane: the chunk's rows among the output's taps, each tap once
            // over the chunks
#pragma unroll
            for (int b = 0; b < NB; b++) {
                if (!((mask >> b) & 1u)) continue;
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int i = (tid >> 5) + 8 * e, j = tid & 31;
                    if (i >= ny || j >= nx) continue;
                    const int f = fy[i];
                    const int lo = f > r0 ? f : r0, hi = f + cy[i] < r0 + nr ? f + cy[i] : r0 + nr;
                    const int32_t *t = tb + (b * RESIZE_TW + j) * FRESIZE_TPITCH;
                    for (int row = lo; row < hi; row++)
                        acc[b][e] += (long long)(int)qy[(row - f) * RESIZE_TH + i] * (long long)t[row - r0];
                }
            }
            // (the next chunk's stage writes only `stage`; its barrier orders this
            // chunk's reads of tb before the next horizontal pass)
        }
    }

    int rr[NB][2];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int e = 0; e < 2; e++) rr[b][e] = (int)((acc[b][e] + (1ll << 23)) >> 24);
    uint8_t *O = a.out + blockIdx.y * a.out_stride;
    const int nout = S::nout(a);
#pragma unroll
    for (int c = 0; c < S::MAX_OUT; c++) {
        if (c >= nout) break;
        const int pl = S::plane_of(a, c);
        const float sc = a.scale[c], bb = a.bias[c];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int i = (tid >> 5) + 8 * e, j = tid & 31;
            if (i >= ny || j >= nx) continue;
            int r = rr[0][e];
#pragma unroll
            for (int b = 1; b < NB; b++) r = pl == b ? rr[b][e] : r;
            const uint32_t v = fresize_elem<DT>(r, sc, bb);
            const size_t o = ((size_t)c * oh + (size_t)(oy0 + i)) * ow + (size_t)(ox0 + j);
            if (ES == 2) __builtin_nontemporal_store((uint16_t)v, (uint16_t *)O + o);
            else __builtin_nontemporal_store(v, (uint32_t *)O + o);
        }
    }
}

template <class S>
static void fresize_launch(int dt, int npics, hipStream_t st, const fresize_args<S> &a)
{
    const unsigned ntx = (unsigned)(a.ow + RESIZE_TW - 1) / RESIZE_TW, nty = (unsigned)(a.oh + RESIZE_TH - 1) / RESIZE_TH;
    const dim3 grid(ntx * nty, npics), block(RESIZE_THREADS);
#define FRESIZE_CASE(D) \
    if (dt == D) hipLaunchKernelGGL((k_field_resize<S, D>), grid, block, 0, st, a);
    FRESIZE_CASE(TENSOR_F16) FRESIZE_CASE(TENSOR_BF16) FRESIZE_CASE(TENSOR_F32) FRESIZE_CASE(TENSOR_I16)
#undef FRESIZE_CASE
}
