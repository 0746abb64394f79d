// The decoded residual as device tensors: the prediction error the stream
// carries, per sample of the MB-aligned picture (the field: include/h264mi.h,
// DESIGN 3.5e), from the MbRec batches and coefficient pools of a list of
// pictures.  A sample of record r's 4x4 block b (the cbits bit index: 0..15
// luma z-scan, 16..19 Cb, 20..23 Cr) is the block's inverse transform -- the
// arithmetic of mb_residual (recon_kernels.hip), restated here because the
// field clamps to int16 where mb_residual keeps the low 16 bits and flags the
// picture -- when r.type is MBT_INTER, MBT_I4x4 or MBT_I16 and b is in
// res_mask(r.type, r.cbits); every other sample is 0.  The gate is the type:
// a skip or I_PCM record's cbits and coef are never used, and an MB whose
// blocks would end beyond the pool (coef_blocks) reads nothing and is 0.
//
// One 256-thread workgroup per (RESID_COLS luma columns of the window, MB row,
// picture).  Wave w takes the MBs m0 + w, m0 + w + 4 of the up to RESID_LDS_MBS
// the columns touch: lane b < 24 holds block b as mb_residual's lanes do,
// computes its own DC term (no exchange between lanes) and writes its 16
// clamped samples as four 8-byte rows into an int16 raster image of the MB row
// in LDS -- rows 0..15 luma, rows 16..23 chroma with Cb in columns 0..39 and Cr
// in 40..79.  An MB with nothing to transform (type, res_mask == 0, pool bound)
// is a wave-uniform branch that loads no coefficient and writes zeros.  After
// the barrier all 256 threads produce the items of every output plane in
// raster order, consecutive lanes consecutive row pieces:
//   V16   16 bytes of a plane row (d_out, out_stride and the row bytes are
//         multiples of 16): 8 int16 / fp16 / bf16 or 4 fp32, one non-temporal
//         store;
//   else  one element.
// Image rows are RESID_LDS_STRIDE = 84 int16 = 42 dwords apart, not 40: a
// ds_write_b64 is served in groups of 16 consecutive lanes on banks = dword mod
// 32.  The 16 luma lanes of an MB write dwords (4 * by + row) * S + 2 * bx +
// {0, 1} (+ const): 2 * bx covers 8 banks, and 4 * S * by mod 32 must put the
// four block rows on the four disjoint octets, so S = 2 or 6 mod 8; 40 would
// put all four on one (4-way).  The 8 chroma lanes (the next group) write (4 *
// by + row) * S + 20 * comp + 2 * bx + {0, 1}: {0..3} + {0, 20} + {0, 8} with
// S = 42, disjoint as well.  The item reads are 2-byte reads of 16-byte pieces
// and stay 2-way for every even S (S * row mod 4 takes two values); an odd S
// would misalign the 8-byte writes.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/h264mi_records.h"
#include "mb_shared.h"
#include "crop.hip"
#include "tensor.hip"
#include "field_store.h"
#define RESID_MAX_PICS 32           // pictures per launch (their offsets travel in the kernel arguments)
#define RESID_COLS 64               // luma window columns per workgroup: 4 MBs, a multiple of every item width
#define RESID_LDS_MBS (RESID_COLS / 16 + 1)     // a window can start inside an MB
#define RESID_LDS_STRIDE 84         // int16 between image rows in LDS (above)
#define RESID_LDS_CR (RESID_LDS_MBS * 8)        // Cr's first column in a chroma row
static_assert(RESID_LDS_STRIDE >= RESID_LDS_MBS * 16 && RESID_LDS_STRIDE % 4 == 0 && (RESID_LDS_STRIDE / 2) % 8 == 2,
              "rows hold the MBs, 8-byte aligned, on disjoint bank octets");

enum { RESID_Y = 0, RESID_UV = 1, RESID_YUV = 2 };

struct residual_args {
    const uint8_t *rec;
    const int16_t *coef;
    uint8_t *out;
    unsigned long long coef_blocks;
    size_t out_stride;
    int w_mbs, x, y, cw, ch, planes;
    float scale[3], bias[3];
    unsigned long long off[RESID_MAX_PICS];
    uint32_t cbase[RESID_MAX_PICS];
};

__device__ __forceinline__ int resid_clamp(int v) { return min(max(v, -32768), 32767); }

// the 16 samples (raster) of block `lane` of an MB with something to
// transform: type, cb = cbits, m = res_mask, qp the lane's plane's, c the MB's
// first pool block
__device__ __forceinline__ void resid_block(int type, uint32_t cb, uint32_t m, int qp, int lane, const int16_t *c,
                                            int (&o)[16])
{
    // raster position of scan position s
    constexpr int zz[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
    const bool luma = lane < 16, i16 = type == MBT_I16;
    const int q6 = qp / 6, qm = qp % 6;
    const int ls0 = cLevelScale[qm][0], ls1 = cLevelScale[qm][1], ls2 = cLevelScale[qm][2];
    int d[16];
#pragma unroll
    for (int i = 0; i < 16; i++) d[i] = 0;
    if ((m >> lane) & 1) {
        if ((cb >> lane) & 1) {
            const crop_u32x4 *q = (const crop_u32x4 *)(c + __popc(cb & ((1u << lane) - 1)) * 16);
            const crop_u32x4 lo = q[0], hi = q[1];
            const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int s = 0; s < 16; s++) {
                const int rr = zz[s];
                const int lv = (int)(int16_t)(w[s >> 1] >> (16 * (s & 1)));
                const int sc = (!(rr & 1) && !(rr & 4)) ? ls0 : ((rr & 1) && (rr & 4)) ? ls1 : ls2;
                d[rr] = lv * (sc << q6);
            }
        }
        if (luma) {
            if (i16) {
                // position 0 is the luma DC transform's output for this block:
                // f = A c A at (i, j) = the block's (row, column), A[i][k] =
                // (-1)^popcount(k & m(i)), m = {0, 2, 3, 1}
                int v = 0;
                if ((cb >> 24) & 1) {
                    const crop_u32x4 *q = (const crop_u32x4 *)(c + __popc(cb & 0xFFFFFFu) * 16);
                    const crop_u32x4 lo = q[0], hi = q[1];
                    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                    const int i = blk_y(lane), j = blk_x(lane);
                    const int mi = i == 1 ? 2 : i == 2 ? 3 : i == 3 ? 1 : 0;
                    const int mj = j == 1 ? 2 : j == 2 ? 3 : j == 3 ? 1 : 0;
                    int s = 0;
#pragma unroll
                    for (int sp = 0; sp < 16; sp++) {
                        const int rr = zz[sp];
                        const int lv = (int)(int16_t)(w[sp >> 1] >> (16 * (sp & 1)));
                        const int neg = (__popc((rr >> 2) & mi) + __popc((rr & 3) & mj)) & 1;
                        s += neg ? -lv : lv;
                    }
                    const int x = s * ls0;
                    v = q6 >= 2 ? x << (q6 - 2) : ((x << q6) + 2) >> 2;
                }
                d[0] = v;
            }
        } else {
            // position 0 is the chroma DC transform's output
            const int comp = (lane - 16) >> 2, b = lane & 3;
            const uint32_t bit = 1u << (25 + comp);
            int f = 0;
            if (cb & bit) {
                const uint32_t *q = (const uint32_t *)(c + __popc(cb & (bit - 1)) * 16);
                const uint32_t w0 = q[0], w1 = q[1];
                const int c0 = (int16_t)w0, c1 = (int16_t)(w0 >> 16), c2 = (int16_t)w1, c3 = (int16_t)(w1 >> 16);
                f = b == 0 ? c0 + c1 + c2 + c3 : b == 1 ? c0 - c1 + c2 - c3 : b == 2 ? c0 + c1 - c2 - c3 : c0 - c1 - c2 + c3;
                f = ((f * ls0) << q6) >> 1;
            }
            d[0] = f;
        }
    }
    int t[16];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int a = d[4 * i] + d[4 * i + 2], b = d[4 * i] - d[4 * i + 2];
        const int cc = (d[4 * i + 1] >> 1) - d[4 * i + 3], e = d[4 * i + 1] + (d[4 * i + 3] >> 1);
        t[4 * i] = a + e; t[4 * i + 1] = b + cc; t[4 * i + 2] = b - cc; t[4 * i + 3] = a - e;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int a = t[j] + t[8 + j], b = t[j] - t[8 + j];
        const int cc = (t[4 + j] >> 1) - t[12 + j], e = t[4 + j] + (t[12 + j] >> 1);
        o[j] = resid_clamp((a + e + 32) >> 6); o[4 + j] = resid_clamp((b + cc + 32) >> 6);
        o[8 + j] = resid_clamp((b - cc + 32) >> 6); o[12 + j] = resid_clamp((a - e + 32) >> 6);
    }
}

// grid: (ceil(cw / RESID_COLS), MB rows the window touches, pictures of this launch)
template <int DT, bool V16>
__global__ __launch_bounds__(256) void k_residual(const residual_args a)
{
    constexpr int ES = tensor_elem_size(DT);
    constexpr int NE = V16 ? 16 / ES : 1;           // elements per item
    static_assert((RESID_COLS / 2) % (16 / ES) == 0, "a workgroup's part of a UV row holds whole items");
    __shared__ __attribute__((aligned(16))) int16_t img[24 * RESID_LDS_STRIDE];
    const int c0 = (int)blockIdx.x * RESID_COLS;                     // first luma window column of this part
    const int ncols = a.cw - c0 < RESID_COLS ? a.cw - c0 : RESID_COLS;
    const int R = (a.y >> 4) + (int)blockIdx.y;                      // MB row
    const int m0 = (a.x + c0) >> 4;                                  // MBs m0 .. m0 + nmb - 1 of the row
    const int nmb = ((a.x + c0 + ncols - 1) >> 4) - m0 + 1;
    const int lane = (int)threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const bool want_y = a.planes != RESID_UV, want_c = a.planes != RESID_Y;
    const uint8_t *recs = a.rec + a.off[blockIdx.z] + ((size_t)R * a.w_mbs + m0) * sizeof(MbRec);
    const unsigned long long cbase = a.cbase[blockIdx.z];
    for (int mb = wave; mb < nmb; mb += 4) {
        // type qp qpc avail | pred dbf offA offB | cbits | coef
        const crop_u32x4 h = *(const crop_u32x4 *)(recs + (size_t)mb * sizeof(MbRec));
        const int type = (int)(h.x & 255u);
        const uint32_t cb = h.z;
        const bool coded = type == MBT_INTER || type == MBT_I4x4 || type == MBT_I16;
        const unsigned long long first = cbase + h.w;
        uint32_t m = coded && first + (unsigned)__popc(cb & 0x7FFFFFFu) <= a.coef_blocks ? res_mask(type, cb) : 0u;
        m = (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
        if (lane < 24 && (lane < 16 ? want_y : want_c)) {
            int o[16];
            if (m) {
                resid_block(type, cb, m, (int)((lane < 16 ? h.x >> 8 : h.x >> 16) & 255u), lane, a.coef + first * 16, o);
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++) o[i] = 0;
            }
            int16_t *d;
            if (lane < 16) d = img + blk_y(lane) * 4 * RESID_LDS_STRIDE + mb * 16 + blk_x(lane) * 4;
            else d = img + (16 + ((lane >> 1) & 1) * 4) * RESID_LDS_STRIDE + ((lane - 16) >> 2) * RESID_LDS_CR + mb * 8 + (lane & 1) * 4;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint2 v;
                v.x = ((uint32_t)o[4 * i] & 0xFFFFu) | (uint32_t)o[4 * i + 1] << 16;
                v.y = ((uint32_t)o[4 * i + 2] & 0xFFFFu) | (uint32_t)o[4 * i + 3] << 16;
                *(uint2 *)(d + i * RESID_LDS_STRIDE) = v;
            }
        }
    }
    __syncthreads();
    // output geometry: UV planes are at half resolution, everything else at luma resolution
    const int hs = a.planes == RESID_UV ? 1 : 0;
    const int OW = a.cw >> hs, OH = a.ch >> hs;
    const int oc0 = c0 >> hs, onc = ncols >> hs;                     // this part's output columns
    const int ya = a.y > 16 * R ? a.y : 16 * R;                      // its luma rows inside the window: ya .. yb - 1
    const int yb = a.y + a.ch < 16 * R + 16 ? a.y + a.ch : 16 * R + 16;
    const int or0 = ya >> hs, nrows = (yb - ya) >> hs;               // output rows, in picture coordinates of the plane
    const int ng = onc / NE;                        // items per row (V16: OW, hence onc, is a multiple of NE)
    const int ni = ng * nrows;
    const int np = a.planes == RESID_Y ? 1 : a.planes == RESID_UV ? 2 : 3;
    uint8_t *O = a.out + blockIdx.z * a.out_stride;
    for (int c = 0; c < np; c++) {
        const float s = a.scale[c], bb = a.bias[c];
        // plane c's samples: image row ((Y >> sh) - rb), column ((X >> sh) - cb0) of (X, Y) in output coordinates
        const bool chroma = a.planes == RESID_UV || c > 0;
        const int sh = chroma && a.planes == RESID_YUV ? 1 : 0;
        const int comp = a.planes == RESID_UV ? c : c - 1;
        const int16_t *src = chroma ? img + 16 * RESID_LDS_STRIDE + comp * RESID_LDS_CR : img;
        const int rb = chroma ? 8 * R : 16 * R, cb0 = chroma ? 8 * m0 : 16 * m0;
        for (int i = (int)threadIdx.x; i < ni; i += 256) {
            const int yy = i / ng, col = oc0 + (i - yy * ng) * NE;
            const int Y = or0 + yy, X = (a.x >> hs) + col;
            const int16_t *row = src + ((Y >> sh) - rb) * RESID_LDS_STRIDE - cb0;
            uint8_t *d = O + (((size_t)c * OH + (Y - (a.y >> hs))) * OW + col) * ES;
            uint32_t e[NE];
#pragma unroll
            for (int k = 0; k < NE; k++) e[k] = field_elem<DT>(row[(X + k) >> sh], s, bb);
            field_store<DT, V16>(e, d);
        }
    }
}

// launch for (dtype, v16)
static void residual_launch(int dt, bool v16, int npics, hipStream_t st, const residual_args &a)
{
    const dim3 grid((a.cw + RESID_COLS - 1) / RESID_COLS, ((a.y + a.ch - 1) >> 4) - (a.y >> 4) + 1, npics), block(256);
    FIELD_LAUNCH(k_residual, dt, v16, grid, block, 0, st, a);
}
