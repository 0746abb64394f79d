// Affine-warped tensor export (include/h264mi.h): every output
// element of a warp is a bilinear blend, in integers, of four samples of the
// window a.(x, y, cw, ch) of its picture -- the R, G, B (or luma) samples of
// tensor.hip, converted per tap, then blended, then tensor.hip's elements:
// warped tensor == convert(warp(samples(window))).  Where the taps lie comes
// from common/warp_geom.h (warp_taps): every position it names is inside the
// window for every matrix (tests/warp_geom_check.c), and a lane loads only
// positions it names; a tap that is not in its mask counts as the pad sample
// whatever its (clamped, in-window) position holds.
//
// A direct gather: a workgroup of 256 threads makes one WARP_TW x WARP_TH tile
// of one warp's output, one lane one output position (all planes of it), j
// fastest along the wave, so that a near-upright map touches few lines per
// load instruction; the four taps' reuse between neighbours is left to the
// vector cache and L2.  The grid's row is the warp: its matrix and picture
// offset come from a table in the kernel arguments (wave-uniform: SGPRs).
// A lane issues the luma and chroma byte loads of all four taps together, then
// converts (rgba_px / rgba_px_set), blends and stores (resize.hip's
// resize_store at resize_out_index).  A tile that lies outside the window by
// more than a sample on one side (warp_tile_outside, uniform) stores the pad
// elements and is done; with H264MI_WARP_BORDER_REPLICATE such a tile takes
// the general path, whose clamped taps are the edge samples.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "color.hip"
#include "tensor.hip"
#include "resize.hip"
#include "../common/warp_geom.h"
#define WARP_TW 32                  // output columns of a tile
#define WARP_TH 8                   // output rows of a tile
#define WARP_THREADS (WARP_TW * WARP_TH)

// t: the pictures, the window the taps are confined to (t.x, t.y, t.cw, t.ch),
// the elements and the colour set; grid row r is the matrix m[r] over the
// picture at t.in_off[r]
struct warp_args {
    tensor_args t;
    int ow, oh, border;
    uint32_t pad[3];                // plane p's sample outside the window (H264MI_WARP_BORDER_CONSTANT)
    int m[TENSOR_MAX_PICS][6];
};

// grid: (tiles of WARP_TW x WARP_TH outputs in raster order, warps of this
// launch), 256 threads; COL (RGB only): the pixels of the colour set a.col;
// HWC (RGB only): the elements interleaved.  The border is a uniform branch.
template <int MODE, int DT, bool COL = false, bool HWC = false>
__global__ __launch_bounds__(WARP_THREADS) void k_tensor_warp(const warp_args ka)
{
    static_assert(!(COL || HWC) || MODE == TENSOR_RGB, "one plane has one order and no colour set");
    constexpr int NP = MODE == TENSOR_RGB ? 3 : 1;
    const tensor_args &a = ka.t;
    const int tid = (int)threadIdx.x;
    const int ow = ka.ow, oh = ka.oh, cw = a.cw, ch = a.ch;
    const int ntx = (ow + WARP_TW - 1) / WARP_TW;
    const int ty = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - ty * ntx;
    const int i = ty * WARP_TH + (tid >> 5), j = tx * WARP_TW + (tid & 31);
    const int *m = ka.m[blockIdx.y];
    uint8_t *O = a.out + a.out_off[blockIdx.y];
    const bool mine = i < oh && j < ow;

    if (ka.border == H264MI_WARP_BORDER_CONSTANT &&
        warp_tile_outside(m, ty * WARP_TH, ty * WARP_TH + WARP_TH - 1, tx * WARP_TW, tx * WARP_TW + WARP_TW - 1, cw, ch)) {
        if (mine) {
#pragma unroll
            for (int p = 0; p < NP; p++)
                resize_store<DT>(O, resize_out_index<HWC, NP, DT>(a, p, i, j), tensor_elem<DT>(ka.pad[p], a.scale[p], a.bias[p]));
        }
        return;
    }
    if (!mine) return;

    const warp_tap t = warp_taps(m, i, j, cw, ch, ka.border);
    const int width = a.width, cpitch = a.cpitch;
    const uint8_t *Y = a.in + a.in_off[blockIdx.y];
    const uint8_t *U = Y + (size_t)width * a.height + (size_t)(a.y >> 1) * cpitch + (a.x >> 1);
    const uint8_t *V = U + (size_t)cpitch * (a.height >> 1);
    Y += (size_t)a.y * width + a.x;

    // the loads of all four taps, luma and chroma, ahead of the first conversion,
    // in one straight-line block (a branch per tap would wait for each tap's
    // loads in turn): a tap that is not in the mask is loaded from its clamped
    // position, which is inside the window like every position named, and its
    // value is replaced below
    // (x and y of the window are even: the chroma sample of (c, r) is (c >> 1, r >> 1) of the window's)
    uint32_t ly[4], lu[4], lv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = t.x[k & 1], r = t.y[k >> 1];
        ly[k] = Y[(size_t)r * width + c];
        lu[k] = lv[k] = 0;
        if (MODE == TENSOR_RGB) {
            const size_t co = (size_t)(r >> 1) * cpitch + (c >> 1);
            lu[k] = U[co];
            lv[k] = V[co];
        }
    }

    // plane p of tap k in bits 8 p .. 8 p + 7
    uint32_t px[4];
    const uint32_t padpx = MODE == TENSOR_RGB ? ka.pad[0] | ka.pad[1] << 8 | ka.pad[2] << 16 : ka.pad[0];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t s = ly[k];
        if (MODE == TENSOR_RGB) {
            const int u = (int)lu[k] - 128, v = (int)lv[k] - 128;
            if constexpr (COL) {
                const colour_set &cs = a.col;
                s = rgba_px_set((int)ly[k], cs.ky, __mul24(cs.crv, v) + cs.k0,
                                __mul24(-cs.cgv, v) + (__mul24(-cs.cgu, u) + cs.k0), __mul24(cs.cbu, u) + cs.k0);
            } else {
                s = rgba_px((int)ly[k], 1634 * v, -832 * v - 400 * u, 2066 * u);
            }
        }
        px[k] = (t.mask >> k) & 1 ? s : padpx;
    }

    const uint32_t fx = (uint32_t)t.fx, fy = (uint32_t)t.fy;
    const uint32_t w[4] = {(256u - fx) * (256u - fy), fx * (256u - fy), (256u - fx) * fy, fx * fy};
#pragma unroll
    for (int p = 0; p < NP; p++) {
        uint32_t acc = 32768u;                      // (the weights add up to 65536: acc < 2^24 + 2^15)
#pragma unroll
        for (int k = 0; k < 4; k++) acc += w[k] * ((px[k] >> (8 * p)) & 255u);
        resize_store<DT>(O, resize_out_index<HWC, NP, DT>(a, p, i, j), tensor_elem<DT>(acc >> 16, a.scale[p], a.bias[p]));
    }
}

// nwarps <= TENSOR_MAX_PICS warps: a.m[r] and a.t.in_off[r], r < nwarps; the 20
// instantiations by (mode, dt, col, hwc)
static void warp_launch(int mode, int dt, bool col, bool hwc, int nwarps, hipStream_t st, const warp_args &a)
{
    const unsigned ntx = (unsigned)(a.ow + WARP_TW - 1) / WARP_TW, nty = (unsigned)(a.oh + WARP_TH - 1) / WARP_TH;
    const dim3 grid(ntx * nty, nwarps), block(WARP_THREADS);
#define WARP_RGB_CASE(D, C, H)                                                                                      \
    if (mode == TENSOR_RGB && dt == D && col == C && hwc == H)                                                      \
        hipLaunchKernelGGL((k_tensor_warp<TENSOR_RGB, D, C, H>), grid, block, 0, st, a);
#define WARP_RGB_CASES(D)                                                                                           \
    WARP_RGB_CASE(D, false, false) WARP_RGB_CASE(D, false, true) WARP_RGB_CASE(D, true, false) WARP_RGB_CASE(D, true, true)
    WARP_RGB_CASES(TENSOR_U8) WARP_RGB_CASES(TENSOR_F16) WARP_RGB_CASES(TENSOR_BF16) WARP_RGB_CASES(TENSOR_F32)
#undef WARP_RGB_CASES
#undef WARP_RGB_CASE
#define WARP_GRAY_CASE(D)                                                                                           \
    if (mode == TENSOR_GRAY && dt == D) hipLaunchKernelGGL((k_tensor_warp<TENSOR_GRAY, D>), grid, block, 0, st, a);
    WARP_GRAY_CASE(TENSOR_U8) WARP_GRAY_CASE(TENSOR_F16) WARP_GRAY_CASE(TENSOR_BF16) WARP_GRAY_CASE(TENSOR_F32)
#undef WARP_GRAY_CASE
}
