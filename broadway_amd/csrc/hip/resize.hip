// Resized tensor export: the window of tensor.hip, filtered to
// (oh, ow) samples per plane by an antialiased triangle filter (bilinear with
// the support stretched by the downscale ratio) in integer arithmetic, then
// tensor.hip's elements: resized tensor == convert(resize(samples(window))).
//
// One axis, n source samples -> m outputs: R = 2 max(m, n); output j has
// C = (2 j + 1) n - m (its centre (j + 0.5) n / m - 0.5 in units of 1 / (2 m));
// source sample k, 0 <= k < n, weighs w_k = R - |2 m k - C| where that is
// positive (taps outside the window are dropped, the rest are contiguous, at
// most 64 with n <= 32 m); q_k = (w_k * 16384 + W / 2) / W with W = sum w_k, and
// 16384 - sum q_k goes to the first tap of largest weight.  Two passes:
//   t   = (sum_k qx_k * s[row][k] + 128) >> 8          (6 fractional bits, 16 bits)
//   out = (sum_l qy_l * t[l] + (1 << 19)) >> 20        (<= 255, no clamp)
//
// The bicubic filter (the kernel's CUBIC flag) is the same kernel
// with other taps and signed passes: the Keys kernel with a = -0.5 over
// |2 m k - C| < 2 R (at most 64 taps with n <= 16 m), its weights cut to 16 bits
// by one shift, q by a floor division and possibly negative (resize_taps_cubic);
// the tables and t are int16, the multiply-adds signed, t's shift arithmetic,
// and the output is clamped to 0..255 (any sum |q| < 32768 keeps t in int16 and
// the vertical sum in int32).  Without the flag the code is the triangle's,
// instruction for instruction what it was before there was a second filter.
//
// A workgroup of 256 threads makes one RESIZE_TW x RESIZE_TH tile of one
// picture's output:
//   taps      lanes 0..47 of wave 0 derive first tap, count and the q of one
//             tile column or row each (32-bit unsigned divisions; CUBIC: 64-bit
//             multiply-adds and a shift per weight in front of them) into LDS,
//             k-major, so that lanes over columns / rows read without conflicts;
//   per chunk of 2..16 source rows (as many as the tile's source columns leave
//   room for in the staging buffer):
//   stage     the chunk's columns, converted once per source pixel (tensor.hip's
//             loads, color.hip's rgba_group_px), one dword per pixel, rows an
//             odd number of dwords apart; at most 3 items per thread, their
//             loads issued together;
//   horizontal  one lane per (source row, output column), rows fastest: lanes
//             of a half-wave read different rows (odd pitch: different banks)
//             of the same few columns; all planes of a pixel from one dword,
//             four taps per iteration (the tables are zero-padded to that);
//             t as uint16 (CUBIC: int16), [plane][column][row], columns 9 dwords apart;
//   vertical  one lane per (plane, output row, output column), 6 (RGB) or 2
//             (GRAY) per thread, adds the chunk's rows of its taps to a 32-bit
//             accumulator in a register;
//   at the end: round, tensor_elem<DT>, one non-temporal store per element
//   (rows are short and start on any element).
//
// Regions of interest: with the kernel's ROIS flag a grid row is
// a box -- the window is the row's own, from a table in the kernel arguments,
// and box r is the resized tensor of its window.  Everything above is per row.
//
// Letterboxing: with the FIT flag (on top of ROIS) the grid's
// tiles are those of a canvas, and the row's resized tensor, rw x rh outputs,
// lies at (px, py) of it -- the placement comes with the row, from the host's
// letterbox_fit.  A tile resizes its part of the content (the axes' outputs are
// the content's: j = canvas column - px over m = rw) and stores the pad element
// in the rest; a tile with no content stores pad elements and is done.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "crop.hip"
#include "tensor.hip"
#define RESIZE_TW 32                // output columns of a tile
#define RESIZE_TH 16                // output rows of a tile
#define RESIZE_THREADS 256
#define RESIZE_MAX_TAPS 64          // n <= 32 m (triangle), n <= 16 m (bicubic)
#define RESIZE_ROWS 16              // source rows per chunk, at most
#define RESIZE_STAGE_DW 6144        // staging buffer; 2 rows of the widest tile (32 : 1) are 2130 dwords
#define RESIZE_TPITCH (RESIZE_ROWS + 2)     // uint16 per column of t: 9 dwords
#define RESIZE_MAX_DIM 16384        // ow, oh (and cw, ch): w * 16384 <= 2^29

struct resize_args {
    tensor_args t;
    int ow, oh;
};

// the same over a list of boxes: grid row r is box r, the window
// win[r] = (x, y, cw, ch) of the picture at t.in_off[r]; t's own window is unused
struct rois_args {
    resize_args r;
    int win[TENSOR_MAX_PICS][4];
};

// and fitted into a canvas: r.ow x r.oh is the canvas, row r's
// content place[r] = (px, py, rw, rh) inside it, pad[p] plane p's sample outside
struct fit_args : rois_args {
    int place[TENSOR_MAX_PICS][4];
    uint32_t pad[3];
};

// the taps of output j of an axis n -> m: q[k * qpitch], k < count, for source
// samples first + k, and zeros up to the next multiple of 4 taps.  Every
// intermediate fits 32 bits for m, n <= 16384.
__device__ __forceinline__ void resize_taps(uint32_t n, uint32_t m, uint32_t j, uint16_t *q, int qpitch, int &first,
                                            int &count)
{
    const uint32_t R = 2u * (m > n ? m : n), m2 = 2u * m;
    const int32_t C = (int32_t)((2u * j + 1u) * n) - (int32_t)m;
    // w_k > 0: C - R < 2 m k < C + R
    const int32_t lo = C - (int32_t)R;
    const uint32_t k0 = lo < 0 ? 0u : (uint32_t)lo / m2 + 1u;
    uint32_t k1 = ((uint32_t)(C + (int32_t)R) - 1u) / m2;
    k1 = k1 < n - 1u ? k1 : n - 1u;
    uint32_t W = 0, wmax = 0, kmax = 0;
    for (uint32_t k = k0; k <= k1; k++) {
        const int32_t d = (int32_t)(m2 * k) - C;
        const uint32_t w = R - (uint32_t)(d < 0 ? -d : d);
        W += w;
        if (w > wmax) { wmax = w; kmax = k - k0; }
    }
    int32_t rest = 16384;
    for (uint32_t k = k0; k <= k1; k++) {
        const int32_t d = (int32_t)(m2 * k) - C;
        const uint32_t w = R - (uint32_t)(d < 0 ? -d : d);
        const uint32_t qk = (w * 16384u + (W >> 1)) / W;
        q[(k - k0) * qpitch] = (uint16_t)qk;
        rest -= (int32_t)qk;
    }
    first = (int)k0;
    count = (int)k1 - (int)k0 + 1;
    if (count > 0) q[kmax * qpitch] = (uint16_t)((int32_t)q[kmax * qpitch] + rest);
    // (the horizontal pass takes its taps four at a time)
    for (int k = count > 0 ? count : 0; k < ((count + 3) & ~3); k++) q[k * qpitch] = 0;
}

// The bicubic taps in the same form, q signed: source sample k is
// kept where d = |2 m k - C| < 2 R and weighs the Keys kernel with a = -0.5 at
// d / R, times 2 R^3 -- an integer polynomial, exact in 64 bits (d < 2^16, R <=
// 2^15) -- shifted down by sh = max(0, bitlen(2 R^3) - 16) bits (floor), so
// |w'| < 2^16 and everything after it is 32-bit; q_k = floor((w'_k * 16384 + W
// / 2) / W) by one unsigned division on the numerator's magnitude.
__device__ __forceinline__ int32_t resize_cubic_weight(uint32_t d, uint32_t R, int sh)
{
    const int64_t D = d, Rl = R, R3 = 2 * Rl * Rl * Rl;
    const int64_t w = d < R ? (3 * D - 5 * Rl) * D * D + R3 : ((5 * Rl - D) * D - 8 * Rl * Rl) * D + 2 * R3;
    return (int32_t)(w >> sh);
}

__device__ __forceinline__ void resize_taps_cubic(uint32_t n, uint32_t m, uint32_t j, int16_t *q, int qpitch, int &first,
                                                  int &count)
{
    const uint32_t R = 2u * (m > n ? m : n), m2 = 2u * m;
    const int32_t C = (int32_t)((2u * j + 1u) * n) - (int32_t)m;
    int sh = 48 - (int)__builtin_clzll(2ull * R * R * R);
    sh = sh > 0 ? sh : 0;
    // kept: C - 2 R < 2 m k < C + 2 R
    const int32_t lo = C - (int32_t)(2u * R);
    const uint32_t k0 = lo < 0 ? 0u : (uint32_t)lo / m2 + 1u;
    uint32_t k1 = ((uint32_t)(C + (int32_t)(2u * R)) - 1u) / m2;
    k1 = k1 < n - 1u ? k1 : n - 1u;
    int32_t W = 0, wmax = 0;
    uint32_t kmax = 0;
    for (uint32_t k = k0; k <= k1; k++) {
        const int32_t d = (int32_t)(m2 * k) - C;
        const int32_t w = resize_cubic_weight((uint32_t)(d < 0 ? -d : d), R, sh);
        W += w;
        if (w > wmax) { wmax = w; kmax = k - k0; }
    }
    int32_t rest = 16384;
    for (uint32_t k = k0; k <= k1; k++) {
        const int32_t d = (int32_t)(m2 * k) - C;
        const int32_t num = resize_cubic_weight((uint32_t)(d < 0 ? -d : d), R, sh) * 16384 + (W >> 1);
        // floor(num / W), W > 0: for a negative numerator, minus the magnitude's quotient rounded up
        const uint32_t mag = ((uint32_t)(num < 0 ? -num : num) + (num < 0 ? (uint32_t)W - 1u : 0u)) / (uint32_t)W;
        const int32_t qk = num < 0 ? -(int32_t)mag : (int32_t)mag;
        q[(k - k0) * qpitch] = (int16_t)qk;
        rest -= qk;
    }
    first = (int)k0;
    count = (int)k1 - (int)k0 + 1;
    if (count > 0) q[kmax * qpitch] = (int16_t)((int32_t)q[kmax * qpitch] + rest);
    for (int k = count > 0 ? count : 0; k < ((count + 3) & ~3); k++) q[k * qpitch] = 0;
}

// Stage items tid + 256 u, u < NIT, of a chunk: the loads of all NIT items are
// issued before the first conversion (one straight-line block: a thread past
// the last item repeats it and stores nothing).  The window's last group can
// be 2 columns wide: its luma dword is still read whole (the bytes behind a
// luma row are the next row's or the chroma planes'), its one chroma sample is
// the upper byte of the pair that ends with it (the byte in front of a chroma
// plane is the plane's in front of it); columns 2 and 3 of that group hold
// garbage no tap reads.  The window's width is a.cw or, for a grid row with a
// window of its own (win != NULL: k_tensor_resize's ROIS), win[2].
template <int MODE, int NIT, bool COL>
__device__ __forceinline__ void resize_stage(const tensor_args &a, const int *win, const uint8_t *Y, const uint8_t *U,
                                             const uint8_t *V, uint32_t *stage, int pitch, int ng, int nit, int xs0,
                                             int r0, int tid)
{
    uint32_t y0[NIT][1], y1[NIT][1], u[NIT], v[NIT];
    int so[NIT];
#pragma unroll
    for (int i = 0; i < NIT; i++) {
        const int it = tid + RESIZE_THREADS * i < nit ? tid + RESIZE_THREADS * i : nit - 1;
        const int pr = it / ng, g = it - pr * ng;
        const int c = xs0 + 4 * g, ry = r0 + 2 * pr;
        const uint8_t *sy = Y + (size_t)ry * a.width + c;
        tensor_load<1>(sy, y0[i]);
        tensor_load<1>(sy + a.width, y1[i]);
        if (MODE == TENSOR_RGB) {
            const int part = c + 4 <= (win ? win[2] : a.cw) ? 0 : 1;
            const size_t co = (size_t)(ry >> 1) * a.cpitch + (c >> 1) - part;
            u[i] = crop_load2(U + co) >> (8 * part);
            v[i] = crop_load2(V + co) >> (8 * part);
        }
        so[i] = (2 * pr) * pitch + 4 * g;
    }
#pragma unroll
    for (int i = 0; i < NIT; i++) {
        uint32_t o0[4], o1[4];
        if (MODE == TENSOR_RGB) {
            if constexpr (COL) rgba_group_px_set(a.col, y0[i][0], y1[i][0], u[i], v[i], o0, o1);
            else rgba_group_px(y0[i][0], y1[i][0], u[i], v[i], o0, o1);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                o0[k] = (y0[i][0] >> (8 * k)) & 255u;
                o1[k] = (y1[i][0] >> (8 * k)) & 255u;
            }
        }
        if (tid + RESIZE_THREADS * i < nit) {
            uint32_t *s0 = stage + so[i], *s1 = s0 + pitch;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                s0[k] = o0[k];
                s1[k] = o1[k];
            }
        }
    }
}

// the bits v of an element as the element o bytes (a multiple of the element
// size) into the output at O: one non-temporal store
template <int DT>
__device__ __forceinline__ void resize_store(uint8_t *O, size_t o, uint32_t v)
{
    constexpr int ES = tensor_elem_size(DT);
    if (ES == 1) __builtin_nontemporal_store((uint8_t)v, O + o);
    else if (ES == 2) __builtin_nontemporal_store((uint16_t)v, (uint16_t *)(O + o));
    else __builtin_nontemporal_store(v, (uint32_t *)(O + o));
}

// where element (p, i, j) of an item lies, in bytes from its start, by the
// destination's strides a.row and a.plane: planar, or (HWC,
// DESIGN §3.5m) interleaved, NP elements per column
template <bool HWC, int NP, int DT>
__device__ __forceinline__ size_t resize_out_index(const tensor_args &a, int p, int i, int j)
{
    constexpr int ES = tensor_elem_size(DT);
    if constexpr (HWC) return (size_t)i * a.row + ((size_t)j * NP + p) * ES;
    return (size_t)p * a.plane + (size_t)i * a.row + (size_t)j * ES;
}

// the arguments of k_tensor_resize<.., ROIS, FIT>, and their resize_args
template <bool ROIS, bool FIT> struct resize_kernel_args { typedef resize_args type; };
template <> struct resize_kernel_args<true, false> { typedef rois_args type; };
template <> struct resize_kernel_args<true, true> { typedef fit_args type; };
__device__ __forceinline__ const resize_args &resize_part(const resize_args &a) { return a; }
__device__ __forceinline__ const resize_args &resize_part(const rois_args &a) { return a.r; }

// grid: (tiles of RESIZE_TW x RESIZE_TH outputs in raster order, pictures of
// this launch), 256 threads; COL (RGB only): the pixels of the colour set
// ra.t.col instead of the reference's.  ROIS: a grid row is a box, and its
// window is the row's own, ka.win[blockIdx.y] = (x, y, cw, ch), read from the
// kernel arguments like ra.t's (uniform over the workgroup either way); the
// tile's position depends on (oh, ow) only, so the rows share the grid's x extent.
// FIT (with ROIS): (oh, ow) is a canvas, and the row's outputs are the rw x rh
// at (px, py) of it, ka.place[blockIdx.y] = (px, py, rw, rh); a tile holds the
// content's columns [jx0, jx1) and rows [iy0, iy1) of its own (without FIT: all
// of the tile), the rest of it is ka.pad.  HWC (RGB, with FIT -- the table form
// serves every interleaved resized export, a stretch being a content that
// fills the canvas): every store's index is the interleaved one, nothing else.
// CUBIC: resize_taps_cubic's taps, and with them signed tables,
// a signed t, signed multiply-adds and a clamp at the end; everything else --
// the stage, the chunks, the forms above, the stores -- does not know the filter.
template <int MODE, int DT, bool COL = false, bool ROIS = false, bool FIT = false, bool HWC = false, bool CUBIC = false>
__global__ __launch_bounds__(RESIZE_THREADS) void k_tensor_resize(const typename resize_kernel_args<ROIS, FIT>::type ka)
{
    static_assert(ROIS || !FIT, "the placement is a per-row table, like the window");
    static_assert(!HWC || (FIT && MODE == TENSOR_RGB), "interleaved: RGB, and the table form only");
    typedef typename std::conditional<CUBIC, int16_t, uint16_t>::type q_t;      // a tap, and t
    typedef typename std::conditional<CUBIC, int32_t, uint32_t>::type acc_t;    // a sum of their products
    constexpr int NP = MODE == TENSOR_RGB ? 3 : 1;
    constexpr int NE = NP * RESIZE_TW * RESIZE_TH / RESIZE_THREADS;     // outputs per thread
    static_assert(RESIZE_TW == 32 && RESIZE_TH * RESIZE_TW == 2 * RESIZE_THREADS, "item -> (plane, row, column) below");
    __shared__ uint32_t stage[RESIZE_STAGE_DW + 4];         // (+ 4: the zero-weight taps behind the last row's last)
    __shared__ q_t qx[RESIZE_MAX_TAPS * RESIZE_TW], qy[RESIZE_MAX_TAPS * RESIZE_TH];
    __shared__ q_t tb[NP * RESIZE_TW * RESIZE_TPITCH];
    __shared__ int fx[RESIZE_TW], cx[RESIZE_TW], fy[RESIZE_TH], cy[RESIZE_TH];
    const resize_args &ra = resize_part(ka);
    const int *win = nullptr;
    if constexpr (ROIS) win = ka.win[blockIdx.y];
    const tensor_args &a = ra.t;
    const int tid = (int)threadIdx.x;
    const int width = a.width, cpitch = a.cpitch, cw = ROIS ? win[2] : a.cw, ch = ROIS ? win[3] : a.ch;
    const int ow = ra.ow, oh = ra.oh;
    const int ntx = (ow + RESIZE_TW - 1) / RESIZE_TW;
    const int ty = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - ty * ntx;
    const int ox0 = tx * RESIZE_TW, oy0 = ty * RESIZE_TH;
    const int nx = ow - ox0 < RESIZE_TW ? ow - ox0 : RESIZE_TW, ny = oh - oy0 < RESIZE_TH ? oh - oy0 : RESIZE_TH;
    // the axes' outputs: the content's (FIT) or the tile's grid's
    int px0 = 0, py0 = 0, rw = ow, rh = oh, jx0 = 0, jx1 = nx, iy0 = 0, iy1 = ny;
    if constexpr (FIT) {
        const int *pl = ka.place[blockIdx.y];
        px0 = pl[0]; py0 = pl[1]; rw = pl[2]; rh = pl[3];
        jx0 = px0 > ox0 ? px0 - ox0 : 0;
        jx1 = px0 + rw - ox0 < nx ? px0 + rw - ox0 : nx;
        iy0 = py0 > oy0 ? py0 - oy0 : 0;
        iy1 = py0 + rh - oy0 < ny ? py0 + rh - oy0 : ny;
        if (jx0 >= jx1 || iy0 >= iy1) {             // all bar (uniform over the workgroup)
            uint8_t *O = a.out + a.out_off[blockIdx.y];
#pragma unroll
            for (int e = 0; e < NE; e++) {
                const int p = e >> 1, i = (tid >> 5) + 8 * (e & 1), j = tid & 31;
                if (i >= ny || j >= nx) continue;
                const uint32_t v = tensor_elem<DT>(ka.pad[p], a.scale[p], a.bias[p]);
                const size_t o = resize_out_index<HWC, NP, DT>(a, p, oy0 + i, ox0 + j);
                resize_store<DT>(O, o, v);
            }
            return;
        }
    }

    if (tid < RESIZE_TW + RESIZE_TH) {
        const bool isx = tid < RESIZE_TW;
        const int l = isx ? tid : tid - RESIZE_TW;
        int f = 0, c = 0;
        if (l >= (isx ? jx0 : iy0) && l < (isx ? jx1 : iy1)) {
            if constexpr (CUBIC)
                resize_taps_cubic((uint32_t)(isx ? cw : ch), (uint32_t)(isx ? rw : rh),
                                  (uint32_t)((isx ? ox0 - px0 : oy0 - py0) + l), (isx ? qx : qy) + l,
                                  isx ? RESIZE_TW : RESIZE_TH, f, c);
            else
                resize_taps((uint32_t)(isx ? cw : ch), (uint32_t)(isx ? rw : rh),
                            (uint32_t)((isx ? ox0 - px0 : oy0 - py0) + l), (isx ? qx : qy) + l,
                            isx ? RESIZE_TW : RESIZE_TH, f, c);
        }
        (isx ? fx : fy)[l] = f;
        (isx ? cx : cy)[l] = c;
    }
    __syncthreads();

    // the tile's source columns [xs0, xs0 + segw) (4-column groups of the
    // window) and rows [ys0, ye) (row pairs): first taps and tap ends grow with
    // the output index
    const int xs0 = fx[jx0] & ~3, segw = (fx[jx1 - 1] + cx[jx1 - 1] - xs0 + 3) & ~3, pitch = segw | 1, ng = segw >> 2;
    const int ys0 = fy[iy0] & ~1, ye = fy[iy1 - 1] + cy[iy1 - 1];
    int lrc = 4;                                    // log2 of the chunk's rows
    while (lrc > 1 && (pitch << lrc) > RESIZE_STAGE_DW) lrc--;
    if ((pitch << lrc) > RESIZE_STAGE_DW) return;   // (not with n <= 32 m, nor with the bicubic's n <= 16 m)
    const int rc = 1 << lrc;

    const int x = ROIS ? win[0] : a.x, y = ROIS ? win[1] : a.y;
    const uint8_t *Y = a.in + a.in_off[blockIdx.y];
    const uint8_t *U = Y + (size_t)width * a.height + (size_t)(y >> 1) * cpitch + (x >> 1);
    const uint8_t *V = U + (size_t)cpitch * (a.height >> 1);
    Y += (size_t)y * width + x;

    acc_t acc[NE];
#pragma unroll
    for (int e = 0; e < NE; e++) acc[e] = 0;

    for (int r0 = ys0; r0 < ye; r0 += rc) {
        const int nr = ye - r0 < rc ? ye - r0 : rc;         // source rows of this chunk
        // stage: (row pair, 4-column group) items, groups fastest, at most 3 per thread
        const int nit = ((nr + 1) >> 1) * ng;
        if (nit <= RESIZE_THREADS) resize_stage<MODE, 1, COL>(a, win, Y, U, V, stage, pitch, ng, nit, xs0, r0, tid);
        else if (nit <= 2 * RESIZE_THREADS) resize_stage<MODE, 2, COL>(a, win, Y, U, V, stage, pitch, ng, nit, xs0, r0, tid);
        else resize_stage<MODE, 3, COL>(a, win, Y, U, V, stage, pitch, ng, nit, xs0, r0, tid);
        __syncthreads();
        // horizontal: (source row, output column) items, rows fastest
        for (int it = tid; it < (RESIZE_TW << lrc); it += RESIZE_THREADS) {
            const int r = it & (rc - 1), j = it >> lrc;
            if (r >= nr || j < jx0 || j >= jx1) continue;
            const uint32_t *s = stage + r * pitch + (fx[j] - xs0);
            const int n = cx[j];
            acc_t h[NP];
#pragma unroll
            for (int p = 0; p < NP; p++) h[p] = 0;
            // four taps at a time, their LDS reads in flight together; behind
            // the last tap: weight 0 times whatever the buffer holds
            for (int k = 0; k < n; k += 4) {
                uint32_t px[4];
                acc_t q[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    px[u] = s[k + u];
                    q[u] = qx[(k + u) * RESIZE_TW + j];
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int p = 0; p < NP; p++) h[p] += q[u] * (acc_t)((px[u] >> (8 * p)) & 255u);
            }
#pragma unroll
            for (int p = 0; p < NP; p++) tb[(p * RESIZE_TW + j) * RESIZE_TPITCH + r] = (q_t)((h[p] + (acc_t)128) >> 8);
        }
        __syncthreads();
        // vertical: item tid + 256 e = (plane e >> 1, row (tid >> 5) + 8 (e & 1), column tid & 31):
        // the chunk's rows among the item's taps, each tap once over the chunks
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int p = e >> 1, i = (tid >> 5) + 8 * (e & 1), j = tid & 31;
            if (i < iy0 || i >= iy1 || j < jx0 || j >= jx1) continue;
            const int f = fy[i];
            const int lo = f > r0 ? f : r0, hi = f + cy[i] < r0 + nr ? f + cy[i] : r0 + nr;
            const q_t *t = tb + (p * RESIZE_TW + j) * RESIZE_TPITCH;
            for (int row = lo; row < hi; row++) acc[e] += (acc_t)qy[(row - f) * RESIZE_TH + i] * (acc_t)t[row - r0];
        }
        // (the next chunk's stage writes only `stage`; its barrier orders this
        // chunk's reads of tb before the next horizontal pass)
    }

    // The destination's strides are the table forms' (ROIS): the single-window form writes packed
    // pictures out_stride apart, with the index arithmetic it always had -- with the strides as arguments its
    // legs measured 3 to 13 % slower, the table forms' did not -- and a strided single window runs as a table.
    uint8_t *O;
    if constexpr (ROIS) O = a.out + a.out_off[blockIdx.y];
    else O = a.out + blockIdx.y * a.out_stride;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const int p = e >> 1, i = (tid >> 5) + 8 * (e & 1), j = tid & 31;
        if (i >= ny || j >= nx) continue;
        uint32_t c;
        if constexpr (CUBIC) {
            const int32_t r = ((int32_t)acc[e] + (1 << 19)) >> 20;       // (arithmetic; the overshoot is cut here, once)
            c = (uint32_t)(r < 0 ? 0 : r > 255 ? 255 : r);
        } else {
            c = ((uint32_t)acc[e] + (1u << 19)) >> 20;
        }
        if constexpr (FIT)
            if (i < iy0 || i >= iy1 || j < jx0 || j >= jx1) c = ka.pad[p];
        const uint32_t v = tensor_elem<DT>(c, a.scale[p], a.bias[p]);
        size_t o;
        if constexpr (ROIS) o = resize_out_index<HWC, NP, DT>(a, p, oy0 + i, ox0 + j);
        else o = (((size_t)p * oh + (size_t)(oy0 + i)) * ow + (size_t)(ox0 + j)) * tensor_elem_size(DT);
        resize_store<DT>(O, o, v);
    }
}

// the twelve instantiations by (mode, dt, col) with ROIS and FIT as given, each for the
// triangle and (`cubic`) the bicubic filter, over NROWS grid rows of the tiles of
// (OH, OW); A: the kernel's arguments
#define RESIZE_LAUNCH(ROIS, FIT, NROWS, OW, OH, A)                                                                  \
    do {                                                                                                            \
        const unsigned ntx = (unsigned)((OW) + RESIZE_TW - 1) / RESIZE_TW;                                          \
        const unsigned nty = (unsigned)((OH) + RESIZE_TH - 1) / RESIZE_TH;                                          \
        const dim3 grid(ntx * nty, NROWS), block(RESIZE_THREADS);                                                   \
        RESIZE_COL_CASE(ROIS, FIT, TENSOR_U8, A) RESIZE_COL_CASE(ROIS, FIT, TENSOR_F16, A)                          \
        RESIZE_COL_CASE(ROIS, FIT, TENSOR_BF16, A) RESIZE_COL_CASE(ROIS, FIT, TENSOR_F32, A)                        \
        RESIZE_CASE(ROIS, FIT, TENSOR_RGB, TENSOR_U8, A) RESIZE_CASE(ROIS, FIT, TENSOR_RGB, TENSOR_F16, A)          \
        RESIZE_CASE(ROIS, FIT, TENSOR_RGB, TENSOR_BF16, A) RESIZE_CASE(ROIS, FIT, TENSOR_RGB, TENSOR_F32, A)        \
        RESIZE_CASE(ROIS, FIT, TENSOR_GRAY, TENSOR_U8, A) RESIZE_CASE(ROIS, FIT, TENSOR_GRAY, TENSOR_F16, A)        \
        RESIZE_CASE(ROIS, FIT, TENSOR_GRAY, TENSOR_BF16, A) RESIZE_CASE(ROIS, FIT, TENSOR_GRAY, TENSOR_F32, A)      \
    } while (0)
#define RESIZE_CASE(ROIS, FIT, M, D, A)                                                                             \
    if (mode == M && dt == D) {                                                                                     \
        if (cubic) hipLaunchKernelGGL((k_tensor_resize<M, D, false, ROIS, FIT, false, true>), grid, block, 0, st, A); \
        else hipLaunchKernelGGL((k_tensor_resize<M, D, false, ROIS, FIT>), grid, block, 0, st, A);                  \
    }
#define RESIZE_COL_CASE(ROIS, FIT, D, A)                                                                            \
    if (mode == TENSOR_RGB && dt == D && col) {                                                                     \
        if (cubic) hipLaunchKernelGGL((k_tensor_resize<TENSOR_RGB, D, true, ROIS, FIT, false, true>), grid, block, 0, st, A); \
        else hipLaunchKernelGGL((k_tensor_resize<TENSOR_RGB, D, true, ROIS, FIT>), grid, block, 0, st, A);          \
        return;                                                                                                     \
    }

static void resize_launch(int mode, int dt, bool col, bool cubic, int npics, hipStream_t st, const resize_args &a)
{
    RESIZE_LAUNCH(false, false, npics, a.ow, a.oh, a);
}

// nrois <= TENSOR_MAX_PICS boxes: a.win[r] and a.r.t.in_off[r], r < nrois
static void rois_launch(int mode, int dt, bool col, bool cubic, int nrois, hipStream_t st, const rois_args &a)
{
    RESIZE_LAUNCH(true, false, nrois, a.r.ow, a.r.oh, a);
}

// the same, row r fitted into the canvas (a.r.oh, a.r.ow) at a.place[r]
static void fit_launch(int mode, int dt, bool col, bool cubic, int nrois, hipStream_t st, const fit_args &a)
{
    RESIZE_LAUNCH(true, true, nrois, a.r.ow, a.r.oh, a);
}

// the same with the elements interleaved (RGB)
static void fit_hwc_launch(int dt, bool col, bool cubic, int nrois, hipStream_t st, const fit_args &a)
{
    const unsigned ntx = (unsigned)(a.r.ow + RESIZE_TW - 1) / RESIZE_TW, nty = (unsigned)(a.r.oh + RESIZE_TH - 1) / RESIZE_TH;
    const dim3 grid(ntx * nty, nrois), block(RESIZE_THREADS);
#define RESIZE_HWC_CASE(D, C)                                                                                       \
    if (dt == D && col == C) {                                                                                      \
        if (cubic) hipLaunchKernelGGL((k_tensor_resize<TENSOR_RGB, D, C, true, true, true, true>), grid, block, 0, st, a); \
        else hipLaunchKernelGGL((k_tensor_resize<TENSOR_RGB, D, C, true, true, true>), grid, block, 0, st, a);      \
    }
    RESIZE_HWC_CASE(TENSOR_U8, false) RESIZE_HWC_CASE(TENSOR_F16, false) RESIZE_HWC_CASE(TENSOR_BF16, false)
    RESIZE_HWC_CASE(TENSOR_F32, false) RESIZE_HWC_CASE(TENSOR_U8, true) RESIZE_HWC_CASE(TENSOR_F16, true)
    RESIZE_HWC_CASE(TENSOR_BF16, true) RESIZE_HWC_CASE(TENSOR_F32, true)
#undef RESIZE_HWC_CASE
}
#undef RESIZE_LAUNCH
#undef RESIZE_COL_CASE
#undef RESIZE_CASE
