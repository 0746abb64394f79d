// Accumulated motion as device tensors (include/h264mi.h): origin
// maps -- one 32-bit word per luma sample of the MB-aligned picture, JX | JY <<
// 16 | ANCHORED << 31, where the sample sat in the key picture of its GOP -- and
// their export as planar channels.
//
// k_accmv_step makes a picture's map from its MbRec batch and the maps of the
// slots it references: a gather.  One 256-thread workgroup per (ACCMV_TILE_MBS
// MBs of an MB row, one of the MB row's four rows of 4x4 blocks, picture): at
// most one item per thread, so that every load of the launch is in flight at
// once (with the four block rows in one workgroup, four dependent iterations
// per thread, a 1080p picture's launch was latency-bound at 9.3 us).  It reads
// its MBs' records (again per block row: 96 bytes per MB) as contiguous
// 16-byte pieces into LDS, as k_mbinfo does (ACCMV_LDS_STRIDE = 25 dwords
// apart: an odd stride keeps the one-dword fields of the 16 MBs a wave reads on
// different banks), and the picture's slot table from the kernel arguments.
// An item is a row piece: the 4 samples of one row of one 4x4 block, which
// share one motion vector and one reference slot.  Items go to lanes in raster
// order, so a wave stores 1 KB of one row, 16 bytes a lane.  The piece's source
// is 4 consecutive words of one row of the reference map, at any sample offset:
// one 16-byte load that is 4-byte aligned.  Where the clamp bites inside the
// piece (the picture's left and right edges) the 4 words have their own
// addresses.  A sample whose slot has no map, and every sample of an intra
// record, is computed and nothing is read for it.
//
// k_accmv streams a window of maps to planar channels: an item is 16 bytes of an
// output row under the alignment rule of k_mbinfo (V16: 8 or 4 elements, from 8
// or 4 consecutive map words, again 4-byte aligned) or one element; each item
// reads its words once and stores every channel, non-temporally.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/h264mi_records.h"
#include "crop.hip"
#include "tensor.hip"
#include "field_store.h"
#define ACCMV_MAX_PICS 32           // pictures per export launch (their offsets travel in the kernel arguments)
#define ACCMV_MAX_CH 8
#define ACCMV_STEP_PICS 8           // pictures per step launch (their slot tables travel in the kernel arguments)
#define ACCMV_MAX_SLOTS 32
#define ACCMV_TILE_MBS 16           // MBs of a row per step workgroup
#define ACCMV_LDS_STRIDE 25         // dwords between records in LDS
#define ACCMV_ANCHORED 0x80000000u

enum { ACC_ADX = 0, ACC_ADY, ACC_JX, ACC_JY, ACC_ANCHORED, ACC_NCHANNELS };
// a picture of a step launch: a step, a key picture (x, y, 1), or a slot without a map (x, y, 0)
enum { ACCMV_STEP = 0, ACCMV_KEY = 1, ACCMV_CLEAR = 2 };

typedef crop_u32x4 accmv_u32x4_a4 __attribute__((aligned(4)));     // 16 bytes on a 4-byte boundary
// a reference map's words, in the global address space: the pointers come out of
// LDS, where the compiler no longer knows that, and would be read with flat loads
typedef __attribute__((address_space(1))) const uint32_t accmv_gu32;
typedef __attribute__((address_space(1))) const accmv_u32x4_a4 accmv_gu32x4;

struct accmv_step_args {
    const uint8_t *rec;
    int w_mbs, W, H, nslots;
    unsigned long long rec_off[ACCMV_STEP_PICS];                // picture p's records start rec_off[p] bytes after rec
    uint32_t *out[ACCMV_STEP_PICS];
    const uint32_t *ref[ACCMV_STEP_PICS][ACCMV_MAX_SLOTS];      // NULL: the slot has no map
    uint8_t mode[ACCMV_STEP_PICS];
};

// grid: (ceil(w_mbs / ACCMV_TILE_MBS), 4 * h_mbs, pictures of this launch)
__global__ __launch_bounds__(256) void k_accmv_step(const accmv_step_args a)
{
    __shared__ uint32_t lds[ACCMV_TILE_MBS * ACCMV_LDS_STRIDE];
    __shared__ const uint32_t *tab[ACCMV_MAX_SLOTS];
    const int p = (int)blockIdx.z, R = (int)blockIdx.y >> 2, by = (int)blockIdx.y & 3;
    const int m0 = (int)blockIdx.x * ACCMV_TILE_MBS;
    const int nmb = a.w_mbs - m0 < ACCMV_TILE_MBS ? a.w_mbs - m0 : ACCMV_TILE_MBS;
    const int np = 4 * nmb;                         // row pieces per sample row of this tile
    const int mode = a.mode[p];
    uint32_t *out = a.out[p];
    if (mode != ACCMV_STEP) {
        const uint32_t top = mode == ACCMV_KEY ? ACCMV_ANCHORED : 0u;
        for (int i = (int)threadIdx.x; i < 4 * np; i += 256) {
            const int r4 = i / np, x = 16 * m0 + 4 * (i - r4 * np), y = 16 * R + 4 * by + r4;
            const uint32_t v = (uint32_t)y << 16 | (uint32_t)x | top;
            const crop_u32x4 o = {v, v + 1, v + 2, v + 3};
            *(crop_u32x4 *)(out + (size_t)y * a.W + x) = o;
        }
        return;
    }
    const crop_u32x4 *src = (const crop_u32x4 *)(a.rec + a.rec_off[p] + ((size_t)R * a.w_mbs + m0) * sizeof(MbRec));
    for (int j = (int)threadIdx.x; j < 6 * nmb; j += 256) {
        const crop_u32x4 v = src[j];
        uint32_t *d = lds + (j / 6) * ACCMV_LDS_STRIDE + (j % 6) * 4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    if (threadIdx.x < ACCMV_MAX_SLOTS) tab[threadIdx.x] = (int)threadIdx.x < a.nslots ? a.ref[p][threadIdx.x] : nullptr;
    __syncthreads();
    const int W = a.W, H = a.H;
    for (int i = (int)threadIdx.x; i < 4 * np; i += 256) {
        const int r4 = i / np, g = i - r4 * np;
        const int x = 16 * m0 + 4 * g, y = 16 * R + 4 * by + r4;
        // MbRec as dwords: type qp qpc avail | pred dbf offA offB | cbits | coef | i4[8] | ref[4] | mv[16] | slice refidx
        const uint32_t *r = lds + (g >> 2) * ACCMV_LDS_STRIDE;
        const int bx = g & 3;
        const int b = (by >> 1) * 8 + (bx >> 1) * 4 + (by & 1) * 2 + (bx & 1);
        const bool inter = (r[0] & 255u) <= MBT_SKIP;
        const uint32_t mv = r[7 + b];
        const int dx = ((int)(int16_t)(mv & 0xFFFFu) + 2) >> 2, dy = ((int)(int16_t)(mv >> 16) + 2) >> 2;
        const uint32_t s = (r[6] >> (8 * (b >> 2))) & 255u;
        const uint32_t *M = s < ACCMV_MAX_SLOTS ? tab[s] : nullptr;      // (tab is NULL from nslots on)
        const int x0 = x + dx, yq = y + dy;
        const int qy = yq < 0 ? 0 : yq > H - 1 ? H - 1 : yq;
        int q[4];
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = x0 + k < 0 ? 0 : x0 + k > W - 1 ? W - 1 : x0 + k;
        const uint32_t id = (uint32_t)y << 16 | (uint32_t)x;
        crop_u32x4 o = {id, id + 1, id + 2, id + 3};
        if (inter) {
            if (M) {
                accmv_gu32 *row = (accmv_gu32 *)(uintptr_t)M + (size_t)qy * W;
                if (x0 >= 0 && x0 + 3 <= W - 1) {
                    o = *(accmv_gu32x4 *)(row + x0);
                } else {
                    o.x = row[q[0]]; o.y = row[q[1]]; o.z = row[q[2]]; o.w = row[q[3]];
                }
            } else {
                const uint32_t hi = (uint32_t)qy << 16;
                o.x = hi | (uint32_t)q[0]; o.y = hi | (uint32_t)q[1]; o.z = hi | (uint32_t)q[2]; o.w = hi | (uint32_t)q[3];
            }
        }
        *(crop_u32x4 *)(out + (size_t)y * W + x) = o;
    }
}

static void accmv_step_launch(int npics, hipStream_t st, const accmv_step_args &a)
{
    const dim3 grid((a.w_mbs + ACCMV_TILE_MBS - 1) / ACCMV_TILE_MBS, a.H / 4, npics);
    hipLaunchKernelGGL(k_accmv_step, grid, dim3(256), 0, st, a);
}

struct accmv_args {
    const uint8_t *maps;
    uint8_t *out;
    int W, x, y, cw, ch, nch;
    size_t out_stride;
    uint8_t id[ACCMV_MAX_CH];
    float scale[ACCMV_MAX_CH], bias[ACCMV_MAX_CH];
    unsigned long long off[ACCMV_MAX_PICS];
};

// channel `id`'s value of the map word w of sample (x, y)
__device__ __forceinline__ int accmv_value(int id, uint32_t w, int x, int y)
{
    const int jx = (int)(w & 0x7FFFu), jy = (int)((w >> 16) & 0x7FFFu);
    switch (id) {
    case ACC_ADX: return jx - x;
    case ACC_ADY: return jy - y;
    case ACC_JX: return jx;
    case ACC_JY: return jy;
    default: return (int)(w >> 31);         // ACC_ANCHORED
    }
}

// grid: (ceil(items of a picture / 256), 1, pictures of this launch)
template <int DT, bool V16>
__global__ __launch_bounds__(256) void k_accmv(const accmv_args a)
{
    constexpr int ES = tensor_elem_size(DT);
    constexpr int NE = V16 ? 16 / ES : 1;           // elements per item
    const int ng = a.cw / NE;                       // items per row (V16: cw is a multiple of NE)
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= ng * a.ch) return;
    const int yy = i / ng, col = (i - yy * ng) * NE;
    const int X = a.x + col, Y = a.y + yy;
    const uint32_t *src = (const uint32_t *)(a.maps + a.off[blockIdx.z]) + (size_t)Y * a.W + X;
    uint32_t w[NE];
    if constexpr (V16) {
#pragma unroll
        for (int k = 0; k < NE; k += 4) {
            const crop_u32x4 v = *(const accmv_u32x4_a4 *)(src + k);
            w[k] = v.x; w[k + 1] = v.y; w[k + 2] = v.z; w[k + 3] = v.w;
        }
    } else {
        w[0] = src[0];
    }
    uint8_t *O = a.out + blockIdx.z * a.out_stride;
    for (int c = 0; c < a.nch; c++) {
        const int id = a.id[c];
        const float s = a.scale[c], bb = a.bias[c];
        uint8_t *d = O + (((size_t)c * a.ch + yy) * a.cw + col) * ES;
        uint32_t e[NE];
#pragma unroll
        for (int k = 0; k < NE; k++) e[k] = field_elem<DT>(accmv_value(id, w[k], X + k, Y), s, bb);
        field_store<DT, V16>(e, d);
    }
}

// launch for (dtype, v16)
static void accmv_launch(int dt, bool v16, int npics, hipStream_t st, const accmv_args &a)
{
    const int ne = v16 ? 16 / tensor_elem_size(dt) : 1;
    const unsigned ni = (unsigned)(a.cw / ne) * (unsigned)a.ch;
    const dim3 grid((ni + 255) / 256, 1, npics), block(256);
    FIELD_LAUNCH(k_accmv, dt, v16, grid, block, 0, st, a);
}
