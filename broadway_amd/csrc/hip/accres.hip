// The accumulated residual as device tensors (include/h264mi.h):
// every sample of a picture minus its origin in the key picture of its GOP,
// cur(p) - key(J(p)), from the picture's frame C, its key frame K and its
// origin map M (accmv.hip's words), as planes Y, UV, YUV or RGB.
//
// k_accres streams a window like k_accmv: an item is 16 bytes of an output row
// under the alignment rule of k_mbinfo (V16: 8 or 4 elements) or one element.
// An item reads its map words (16-byte loads on a 4-byte boundary; UV: the
// words of twice as many luma columns, of which it uses the even ones) and its
// current samples (aligned dwords through v_alignbyte) once, computes every
// plane in registers and stores each plane's elements non-temporally.
//
// The key samples are a gather.  A V16 item takes its elements four at a time:
// the four samples of a row piece of a 4x4 block usually moved together, so
// their origins are a run -- the same row of K, consecutive columns -- and the
// four bytes are one fetch (accres_fetch4: the aligned dword that holds the
// first byte, the next one only when the run crosses into it, one
// v_alignbyte); after several hops, across block borders and at the clamp they
// are not, and the lane takes four global_load_ubyte per plane instead.  The
// choice is per lane and per group; both paths give the same bytes.
//
// What a fetch may read: accres_fetch4(row, off, need) needs the bytes off ..
// off + need - 1 of a row of samples and loads only dwords that hold at least
// one of them.  Rows start on multiples of 4 (the frame does -- the entry point
// refuses others --, W is a multiple of 16, the chroma pitch of 128 and W * H
// of 256) and hold a multiple of 4 samples (W luma, W / 2 = 8 * w_mbs chroma),
// so a dword that holds one sample of a row lies inside that row's samples:
// not in the pitch padding behind a chroma row, and for the last row of Cr --
// whose last sample is the last byte of the three planes when 8 * w_mbs is a
// multiple of 128 -- not behind the frame.  The needed bytes are samples
// because the coordinates are clamped to W - 1 / H - 1 first, a run of luma
// columns jx .. jx + 3 then ends at W - 1 at most, its chroma columns jx >> 1
// .. (jx + 3) >> 1 at W / 2 - 1, and a run of chroma columns (UV) likewise.
// The per-sample path reads row * pitch + column of clamped coordinates.
//
// A picture without a key (key_off == ~0) is a uniform branch that stores
// fma(0, scale, bias) and reads neither K nor anything else.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mb_shared.h"
#include "color.hip"
#include "crop.hip"
#include "tensor.hip"
#include "field_store.h"
#include "accmv.hip"
#define ACCRES_MAX_PICS 32          // pictures per launch (their offsets travel in the kernel arguments)

enum { ACCRES_Y = 0, ACCRES_UV = 1, ACCRES_YUV = 2, ACCRES_RGB = 3 };
#define ACCRES_NO_KEY (~0ull)

// frames and maps in the global address space: the pointers are sums of kernel
// arguments and table entries, and would be read with flat loads otherwise
typedef __attribute__((address_space(1))) const uint8_t accres_gu8;
typedef __attribute__((address_space(1))) const uint32_t accres_gu32;
typedef __attribute__((address_space(1))) const accmv_u32x4_a4 accres_gu32x4;

struct accres_args {
    const uint8_t *cur, *key, *maps;
    uint8_t *out;
    int W, H, cpitch, x, y, cw, ch, planes, zero;
    size_t out_stride;
    colour_set col;
    float scale[3], bias[3];
    unsigned long long cur_off[ACCRES_MAX_PICS], key_off[ACCRES_MAX_PICS], map_off[ACCRES_MAX_PICS];
};

// the three planes of a frame
struct accres_frame {
    accres_gu8 *y, *cb, *cr;
};

__device__ __forceinline__ accres_frame accres_planes(const uint8_t *base, unsigned long long off, int W, int H, int cpitch)
{
    accres_frame f;
    f.y = (accres_gu8 *)(uintptr_t)(base + off);
    f.cb = f.y + (size_t)W * H;
    f.cr = f.cb + (size_t)cpitch * (H >> 1);
    return f;
}

// 4 bytes from byte `off` of the row of samples at `row` (a multiple of 4), of
// which the first `need` (1..4) are samples of the row: only dwords that hold
// one of those are loaded (above)
__device__ __forceinline__ uint32_t accres_fetch4(accres_gu8 *row, int off, int need)
{
    const uint32_t sh = (uint32_t)off & 3u;
    accres_gu32 *q = (accres_gu32 *)(row + (off - (int)sh));
    const uint32_t lo = q[0];
    uint32_t hi = lo;
    if ((int)sh + need > 4) hi = q[1];
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

__device__ __forceinline__ int accres_byte(uint32_t d, int k) { return (int)((d >> (8 * k)) & 255u); }

// channel c of the pixel (y, u, v) under colour set cs (color.hip's arithmetic)
__device__ __forceinline__ void accres_rgb(const colour_set &cs, int y, int u, int v, int (&o)[3])
{
    u -= 128; v -= 128;
    const int a0 = cs.ky * y + cs.k0;
    o[0] = med3i((a0 + cs.crv * v) >> 10, 0, 255);
    o[1] = med3i((a0 - cs.cgu * u - cs.cgv * v) >> 10, 0, 255);
    o[2] = med3i((a0 + cs.cbu * u) >> 10, 0, 255);
}

// N (4, or 1: the element path) consecutive elements of an output row from
// their map words w: (X, Y) is the luma position of the first one, consecutive
// ones 1 << hs luma columns apart (hs = 1: UV).  v[c][k]: plane c's value of
// element k.
template <int N>
__device__ __forceinline__ void accres_group(const accres_args &a, const accres_frame &C, const accres_frame &K,
                                             const uint32_t (&w)[N], int X, int Y, int (&v)[3][N])
{
    const int planes = a.planes, W = a.W, H = a.H, cp = a.cpitch;
    const bool uv = planes == ACCRES_UV, luma = !uv, chroma = planes != ACCRES_Y;
    int jx[N], jy[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        jx[k] = min((int)(w[k] & 0x7FFFu), W - 1);
        jy[k] = min((int)((w[k] >> 16) & 0x7FFFu), H - 1);
    }
    int cy[N], cu[N], cv[N], ky[N], ku[N], kv[N];
#pragma unroll
    for (int k = 0; k < N; k++) cy[k] = cu[k] = cv[k] = ky[k] = ku[k] = kv[k] = 0;
    if constexpr (N == 4) {
        // the current samples: 4 luma bytes from X, the chroma bytes under them (UV: 4 chroma bytes from X >> 1)
        if (luma) {
            const uint32_t d = accres_fetch4(C.y + (size_t)Y * W, X, 4);
#pragma unroll
            for (int k = 0; k < 4; k++) cy[k] = accres_byte(d, k);
        }
        if (chroma) {
            const int c0 = X >> 1, need = uv ? 4 : ((X + 3) >> 1) - c0 + 1;
            const size_t ro = (size_t)(Y >> 1) * cp;
            const uint32_t du = accres_fetch4(C.cb + ro, c0, need), dv = accres_fetch4(C.cr + ro, c0, need);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int i = uv ? k : ((X + k) >> 1) - c0;
                cu[k] = accres_byte(du, i); cv[k] = accres_byte(dv, i);
            }
        }
        // the key samples: a run in the plane the elements live on?
        int gx[4], gy[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { gx[k] = uv ? jx[k] >> 1 : jx[k]; gy[k] = uv ? jy[k] >> 1 : jy[k]; }
        const bool run = gy[1] == gy[0] && gy[2] == gy[0] && gy[3] == gy[0] && gx[1] == gx[0] + 1 &&
                         gx[2] == gx[0] + 2 && gx[3] == gx[0] + 3;
        if (run) {
            if (luma) {
                const uint32_t d = accres_fetch4(K.y + (size_t)gy[0] * W, gx[0], 4);
#pragma unroll
                for (int k = 0; k < 4; k++) ky[k] = accres_byte(d, k);
            }
            if (chroma) {
                const int c0 = uv ? gx[0] : gx[0] >> 1, need = uv ? 4 : ((gx[0] + 3) >> 1) - c0 + 1;
                const size_t ro = (size_t)(uv ? gy[0] : gy[0] >> 1) * cp;
                const uint32_t du = accres_fetch4(K.cb + ro, c0, need), dv = accres_fetch4(K.cr + ro, c0, need);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int i = uv ? k : ((gx[0] + k) >> 1) - c0;
                    ku[k] = accres_byte(du, i); kv[k] = accres_byte(dv, i);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (luma) ky[k] = K.y[(size_t)jy[k] * W + jx[k]];
                if (chroma) {
                    const size_t o = (size_t)(jy[k] >> 1) * cp + (jx[k] >> 1);
                    ku[k] = K.cb[o]; kv[k] = K.cr[o];
                }
            }
        }
    } else {
        if (luma) { cy[0] = C.y[(size_t)Y * W + X]; ky[0] = K.y[(size_t)jy[0] * W + jx[0]]; }
        if (chroma) {
            const size_t co = (size_t)(Y >> 1) * cp + (X >> 1), ko = (size_t)(jy[0] >> 1) * cp + (jx[0] >> 1);
            cu[0] = C.cb[co]; cv[0] = C.cr[co];
            ku[0] = K.cb[ko]; kv[0] = K.cr[ko];
        }
    }
#pragma unroll
    for (int k = 0; k < N; k++) {
        int o[3];
        if (planes == ACCRES_RGB) {
            int c[3], r[3];
            accres_rgb(a.col, cy[k], cu[k], cv[k], c);
            accres_rgb(a.col, ky[k], ku[k], kv[k], r);
            o[0] = c[0] - r[0]; o[1] = c[1] - r[1]; o[2] = c[2] - r[2];
        } else if (uv) {
            o[0] = cu[k] - ku[k]; o[1] = cv[k] - kv[k]; o[2] = 0;
        } else {
            o[0] = cy[k] - ky[k]; o[1] = cu[k] - ku[k]; o[2] = cv[k] - kv[k];
        }
        const bool keep = !a.zero || (w[k] >> 31);
#pragma unroll
        for (int c = 0; c < 3; c++) v[c][k] = keep ? o[c] : 0;
    }
}

// grid: (ceil(items of a picture / 256), 1, pictures of this launch)
template <int DT, bool V16>
__global__ __launch_bounds__(256) void k_accres(const accres_args a)
{
    constexpr int ES = tensor_elem_size(DT);
    constexpr int NE = V16 ? 16 / ES : 1;           // elements per item
    const int hs = a.planes == ACCRES_UV ? 1 : 0;   // UV planes are at half resolution
    const int OW = a.cw >> hs, OH = a.ch >> hs;
    const int ng = OW / NE;                         // items per row (V16: OW is a multiple of NE)
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= ng * OH) return;
    const int yy = i / ng, col = (i - yy * ng) * NE;
    int v[3][NE];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < NE; k++) v[c][k] = 0;
    const unsigned long long ko = a.key_off[blockIdx.z];
    if (ko != ACCRES_NO_KEY) {
        const int X = a.x + (col << hs), Y = a.y + (yy << hs);
        const accres_frame C = accres_planes(a.cur, a.cur_off[blockIdx.z], a.W, a.H, a.cpitch);
        const accres_frame K = accres_planes(a.key, ko, a.W, a.H, a.cpitch);
        accres_gu32 *src = (accres_gu32 *)(uintptr_t)(a.maps + a.map_off[blockIdx.z]) + (size_t)Y * a.W + X;
        if constexpr (V16) {
#pragma unroll
            for (int g = 0; g < NE / 4; g++) {
                uint32_t w[4];
                int q[3][4];
                if (hs) {
                    const crop_u32x4 lo = *(accres_gu32x4 *)(src + 8 * g), hi = *(accres_gu32x4 *)(src + 8 * g + 4);
                    w[0] = lo.x; w[1] = lo.z; w[2] = hi.x; w[3] = hi.z;
                } else {
                    const crop_u32x4 t = *(accres_gu32x4 *)(src + 4 * g);
                    w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
                }
                accres_group<4>(a, C, K, w, X + ((4 * g) << hs), Y, q);
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int k = 0; k < 4; k++) v[c][4 * g + k] = q[c][k];
            }
        } else {
            const uint32_t w[1] = {src[0]};
            int q[3][1];
            accres_group<1>(a, C, K, w, X, Y, q);
            v[0][0] = q[0][0]; v[1][0] = q[1][0]; v[2][0] = q[2][0];
        }
    }
    const int np = a.planes == ACCRES_Y ? 1 : a.planes == ACCRES_UV ? 2 : 3;
    uint8_t *O = a.out + blockIdx.z * a.out_stride;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (c >= np) break;
        const float s = a.scale[c], bb = a.bias[c];
        uint8_t *d = O + (((size_t)c * OH + yy) * OW + col) * ES;
        uint32_t e[NE];
#pragma unroll
        for (int k = 0; k < NE; k++) e[k] = field_elem<DT>(v[c][k], s, bb);
        field_store<DT, V16>(e, d);
    }
}

// launch for (dtype, v16)
static void accres_launch(int dt, bool v16, int npics, hipStream_t st, const accres_args &a)
{
    const int hs = a.planes == ACCRES_UV ? 1 : 0;
    const int ne = v16 ? 16 / tensor_elem_size(dt) : 1;
    const unsigned ni = (unsigned)((a.cw >> hs) / ne) * (unsigned)(a.ch >> hs);
    const dim3 grid((ni + 255) / 256, 1, npics), block(256);
    FIELD_LAUNCH(k_accres, dt, v16, grid, block, 0, st, a);
}
