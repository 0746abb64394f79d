// Motion vectors and MB side information as device tensors: the MbRec batches
// (include/h264mi_records.h, AoS, 4x4 blocks in z-scan order) of a list of
// pictures as planar (nch, bh, bw) fields on the luma 4x4-block grid, raster
// order.  Block (X, Y) of the MB-aligned picture belongs to record (Y >> 2) *
// w_mbs + (X >> 2) and is its z-scan block b = (y >> 1) * 8 + (x >> 1) * 4 +
// (y & 1) * 2 + (x & 1), (x, y) = (X & 3, Y & 3).  One integer v per block and
// channel (MBI_*, the table in include/h264mi.h), gated on the record's type:
// an inter record's i4 bytes hold reference rows and an intra record's mv / ref
// / refidx are whatever the parser left there; a record of type 255 carries no
// information.  int16 elements hold v's low 16 bits; the float types
// fma((float)v, scale[c], bias[c]) of channel position c, converted as in
// tensor.hip.  Picture k's records start off[k] bytes after `rec` and its field
// goes to out + k * out_stride.
//
// One 64-thread workgroup per (MBINFO_COLS window columns, MB row, picture):
// it reads the MB row's records it covers as contiguous 16-byte pieces (6 per
// record) into LDS and then produces, channel by channel, the (block row,
// column) items of its part in raster order, so that both the loads and the
// non-temporal stores of consecutive lanes are consecutive.  An item is
//   V16   16 bytes of a row (out, out_stride and bw * element size are
//         multiples of 16, so every row starts 16-byte aligned and holds whole
//         items): 8 int16 / fp16 / bf16 or 4 fp32 elements, one store;
//   else  one element.
// Records are MBINFO_LDS_STRIDE = 25 dwords apart in LDS, not 24: the lanes of
// a ds_read_b32 group read 8 consecutive MBs (4 blocks each, banks = dword
// mod 32), and 24 * m mod 32 repeats after 4 MBs -- the one-dword fields (type,
// qp, pred, ref, slice | refidx: one address per MB) would conflict 2-way; with
// an odd stride they do not.  The mv reads (dwords {0, 1, 4, 5} + const of 8
// MBs) stay 2-way for every linear stride 24 .. 40, and the fill's ds_write_b32
// become 2-way, which costs a store nothing.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/h264mi_records.h"
#include "crop.hip"
#include "tensor.hip"
#include "field_store.h"
#define MBINFO_MAX_PICS 32          // pictures per launch (their offsets travel in the kernel arguments)
#define MBINFO_MAX_CH 16
#define MBINFO_COLS 128             // window columns (4x4 blocks) per workgroup; a multiple of every item width
#define MBINFO_LDS_STRIDE 25        // dwords between records in LDS (above)
#define MBINFO_LDS_MBS (MBINFO_COLS / 4 + 1)    // a window can start inside an MB

enum { MBI_MVX = 0, MBI_MVY, MBI_REF_IDX, MBI_REF_SLOT, MBI_MB_TYPE, MBI_QP, MBI_INTRA_MODE, MBI_CODED, MBI_SLICE,
       MBI_NCHANNELS };

struct mbinfo_args {
    const uint8_t *rec;
    uint8_t *out;
    int w_mbs, bx, by, bw, bh, nch;
    size_t out_stride;
    uint8_t ch[MBINFO_MAX_CH];
    float scale[MBINFO_MAX_CH], bias[MBINFO_MAX_CH];
    unsigned long long off[MBINFO_MAX_PICS];
};

// channel `id`'s value of z-scan block b of the record at r (LDS, MbRec as
// dwords: type qp qpc avail | pred dbf offA offB | cbits | coef | i4[8] |
// ref[4] | mv[16] | slice refidx)
__device__ __forceinline__ int mbinfo_value(int id, const uint32_t *r, int b)
{
    // every dword is read whatever the type says and the gate is a select: a
    // load under the condition becomes a divergent branch around a ds_read
    const uint32_t d0 = r[0], type = d0 & 255u;
    const bool inter = type <= MBT_SKIP, none = type == 255u;
    switch (id) {
    case MBI_MVX: { const uint32_t mv = r[7 + b]; return inter ? (int)(int16_t)(mv & 0xFFFFu) : 0; }
    case MBI_MVY: { const uint32_t mv = r[7 + b]; return inter ? (int)(int16_t)(mv >> 16) : 0; }
    case MBI_REF_IDX: {
        const int v = (int)((r[23] >> (16 + 4 * (b >> 2))) & 15u);
        return type == MBT_INTER ? v : type == MBT_SKIP ? 0 : -1;
    }
    case MBI_REF_SLOT: { const int v = (int)((r[6] >> (8 * (b >> 2))) & 255u); return inter ? v : -1; }
    case MBI_MB_TYPE: return none ? -1 : (int)type;
    case MBI_QP: return none ? -1 : (int)((d0 >> 8) & 255u);
    case MBI_INTRA_MODE: {
        const int m4 = (int)((r[4 + (b >> 3)] >> (4 * (b & 7))) & 15u), m16 = 16 + (int)(r[1] & 3u);
        return type == MBT_I4x4 ? m4 : type == MBT_I16 ? m16 : -1;
    }
    case MBI_CODED: { const int v = (int)((r[2] >> b) & 1u); return none ? 0 : v; }
    default: { const int v = (int)(r[23] & 0xFFFFu); return none ? -1 : v; }          // MBI_SLICE
    }
}

// a V16 item: the 16 / ES elements from column S (= its first column's
// position inside its MB, a compile-time constant, the same for every item of
// a launch: bx & 3) of the MB whose record is r0, block row bits yb = (y >> 1)
// * 8 + (y & 1) * 2, as one 16-byte store at d.  Unrolled, every element's MB
// and x are constants: the type dword is read and gated once per MB and the
// field reads take immediate offsets.
template <int DT, int S>
__device__ __forceinline__ void mbinfo_item16(int id, const uint32_t *r0, int yb, float s, float bb, uint8_t *d)
{
    constexpr int ES = tensor_elem_size(DT), NE = 16 / ES;
    uint32_t e[NE];
#pragma unroll
    for (int k = 0; k < NE; k++) {
        const int x = (S + k) & 3;
        e[k] = field_elem<DT>(mbinfo_value(id, r0 + ((S + k) >> 2) * MBINFO_LDS_STRIDE, yb + ((x & 2) << 1) + (x & 1)), s, bb);
    }
    field_store<DT, true>(e, d);
}

// grid: (ceil(bw / MBINFO_COLS), MB rows the window touches, pictures of this launch)
template <int DT, bool V16>
__global__ __launch_bounds__(64) void k_mbinfo(const mbinfo_args a)
{
    constexpr int ES = tensor_elem_size(DT);
    constexpr int NE = V16 ? 16 / ES : 1;           // elements per item
    static_assert(MBINFO_COLS % (16 / ES) == 0, "a workgroup's part holds whole items");
    __shared__ uint32_t lds[MBINFO_LDS_MBS * MBINFO_LDS_STRIDE];
    const int c0 = (int)blockIdx.x * MBINFO_COLS;                    // first window column of this part
    const int ncols = a.bw - c0 < MBINFO_COLS ? a.bw - c0 : MBINFO_COLS;
    const int R = (a.by >> 2) + (int)blockIdx.y;                     // MB row
    const int y0 = a.by > 4 * R ? a.by : 4 * R;                      // its block rows inside the window: y0 .. y1 - 1
    const int y1 = a.by + a.bh < 4 * R + 4 ? a.by + a.bh : 4 * R + 4;
    const int m0 = (a.bx + c0) >> 2;                                 // MBs m0 .. m0 + nmb - 1 of the row
    const int nmb = ((a.bx + c0 + ncols - 1) >> 2) - m0 + 1;
    const crop_u32x4 *src = (const crop_u32x4 *)(a.rec + a.off[blockIdx.z] + ((size_t)R * a.w_mbs + m0) * sizeof(MbRec));
    for (int j = (int)threadIdx.x; j < 6 * nmb; j += 64) {
        const crop_u32x4 v = src[j];
        uint32_t *d = lds + (j / 6) * MBINFO_LDS_STRIDE + (j % 6) * 4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    const int ng = ncols / NE;                      // items per row (V16: bw, hence ncols, is a multiple of NE)
    const int ni = ng * (y1 - y0);
    uint8_t *O = a.out + blockIdx.z * a.out_stride;
    for (int c = 0; c < a.nch; c++) {
        const int id = a.ch[c];
        const float s = a.scale[c], bb = a.bias[c];
        for (int i = (int)threadIdx.x; i < ni; i += 64) {
            const int yy = i / ng, col = c0 + (i - yy * ng) * NE, Y = y0 + yy;
            const int X = a.bx + col, yb = ((Y & 2) << 2) + ((Y & 1) << 1);
            const uint32_t *r = lds + ((X >> 2) - m0) * MBINFO_LDS_STRIDE;
            uint8_t *d = O + (((size_t)c * a.bh + (Y - a.by)) * a.bw + col) * ES;
            if constexpr (V16) {
                // (col is a multiple of 4: X & 3 = bx & 3, uniform)
                switch (a.bx & 3) {
                case 0: mbinfo_item16<DT, 0>(id, r, yb, s, bb, d); break;
                case 1: mbinfo_item16<DT, 1>(id, r, yb, s, bb, d); break;
                case 2: mbinfo_item16<DT, 2>(id, r, yb, s, bb, d); break;
                default: mbinfo_item16<DT, 3>(id, r, yb, s, bb, d); break;
                }
            } else {
                const uint32_t e[1] = {field_elem<DT>(mbinfo_value(id, r, yb + ((X & 2) << 1) + (X & 1)), s, bb)};
                field_store<DT, false>(e, d);
            }
        }
    }
}

// launch for (dtype, v16)
static void mbinfo_launch(int dt, bool v16, int npics, hipStream_t st, const mbinfo_args &a)
{
    const dim3 grid((a.bw + MBINFO_COLS - 1) / MBINFO_COLS, ((a.by + a.bh - 1) >> 2) - (a.by >> 2) + 1, npics), block(64);
    FIELD_LAUNCH(k_mbinfo, dt, v16, grid, block, 0, st, a);
}
