// Decoded pictures as device tensors: the window (x, y, cw, ch -- all even) of
// each of a list of pictures as contiguous planes, (3, ch, cw) R G B with the
// pixel values of color.hip (rgba_group_px, or rgba_group_px_set with one of
// the colour sets below; x and y are even, so the RGB of the crop is the crop
// of the RGB) or (1, ch, cw) luma, as uint8, fp16, bf16 or
// fp32.  The float types hold fma((float)c, scale[p], bias[p]) of plane p: one
// fp32 fused multiply-add, then (16-bit types) one round-to-nearest-even
// conversion (v_cvt_f16_f32 / v_cvt_pk_bf16_f32).  Input as in crop.hip: luma
// rows `width` apart, chroma rows `cpitch` apart (an engine slot, or packed
// I420 with cpitch = width / 2); picture k starts in_off[k] bytes after `in`
// and goes to out + out_off[k], its rows `row` bytes and (planar) its planes
// `plane` bytes apart (the host resolves an h264mi_tensor_dest,
// or the packed item of a call without one, into these).
//
// HBM-bound elementwise kernels, 64 threads per block, work items in raster
// order (no lane idles at row ends), non-temporal stores.  A work item is two
// rows of 4 * NG columns, NG the 4-column groups of color.hip it holds:
//   V16   row starts are 16-byte aligned (out, every out_off, row, plane and
//         cw * element size are multiples of 16): NG = 4 / element size, so a lane stores
//         16 bytes per plane row, 6 stores (RGB) or 2 (GRAY) per item;
//   else  NG = 1 and every element is stored on its own (a row can start on
//         any element, and a row pair's last group is 2 columns wide when
//         cw = 2 mod 4).
// HWC (RGB): the same elements interleaved, (ch, cw, 3): an item's
// row is 12 * NG contiguous elements, with V16 three 16-byte stores per row.
// Luma and chroma bytes come from aligned dwords through v_alignbyte, as in
// crop.hip (x can be 2 mod 4, x / 2 odd, a picture can start on any byte).

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "color.hip"
#include "crop.hip"
#define TENSOR_MAX_PICS 32          // pictures per launch (their offsets travel in the kernel arguments)

enum { TENSOR_RGB = 0, TENSOR_GRAY = 1 };
enum { TENSOR_U8 = 0, TENSOR_F16 = 1, TENSOR_BF16 = 2, TENSOR_F32 = 3,
       TENSOR_I16 = 4 };            // int16: mbinfo.hip only (the pixel exports refuse it)

struct tensor_args {
    const uint8_t *in;
    uint8_t *out;
    int width, height, cpitch, x, y, cw, ch;
    size_t out_stride;              // k_tensor_resize without a table only: picture k goes to out + k * out_stride
    size_t row, plane;              // bytes between two rows and (planar) two planes of an item
    float scale[3], bias[3];
    colour_set col;                 // COL kernels only (tensor_colour_sets[id], id != 0)
    unsigned long long in_off[TENSOR_MAX_PICS];
    unsigned long long out_off[TENSOR_MAX_PICS];    // grid row k's item starts out_off[k] bytes after `out`
};

// the colour sets of the RGB exports by id (include/h264mi.h):
// (ky, k0, crv, cgu, cgv, cbu).  Set 0 is color.hip's rgba_px (the reference's
// converter, no rounding term) and runs as literals (COL = false); 1..3 round
// to nearest, k0 = 512 - ky * yoff, and each coefficient is 1024 c rounded to
// nearest of BT.601 full, BT.709 limited, BT.709 full.
#define TENSOR_COLOUR_SETS 4
static const colour_set tensor_colour_sets[TENSOR_COLOUR_SETS] = {
    {1192, -1192 * 16, 1634, 400, 832, 2066},
    {1024, 512, 1436, 352, 731, 1815},
    {1192, 512 - 1192 * 16, 1836, 218, 546, 2163},
    {1024, 512, 1613, 192, 479, 1900},
};

typedef float tensor_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 tensor_f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 tensor_bf16x2 __attribute__((ext_vector_type(2)));

__host__ __device__ constexpr int tensor_elem_size(int dt) { return dt == TENSOR_U8 ? 1 : dt == TENSOR_F32 ? 4 : 2; }

// the 4 * NW source bytes at s (any alignment, all inside the picture): the
// aligned dwords holding them, realigned.  The last dword is read only when
// s is not aligned (it then holds the last byte).
template <int NW>
__device__ __forceinline__ void tensor_load(const uint8_t *s, uint32_t (&d)[NW])
{
    const uint32_t sh = (uint32_t)(uintptr_t)s & 3u;
    const uint32_t *q = (const uint32_t *)(s - sh);
    uint32_t e[NW + 1];
#pragma unroll
    for (int j = 0; j < NW; j++) e[j] = q[j];
    e[NW] = q[sh ? NW : NW - 1];
#pragma unroll
    for (int j = 0; j < NW; j++) d[j] = __builtin_amdgcn_alignbyte(e[j + 1], e[j], sh);
}

// the fp32 value f as a float element type's bits (16-bit types: one
// round-to-nearest-even conversion)
template <int DT>
__device__ __forceinline__ uint32_t tensor_float_bits(float f)
{
    if constexpr (DT == TENSOR_F16) return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
    if constexpr (DT == TENSOR_BF16) return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)f);
    return __builtin_bit_cast(uint32_t, f);
}

// element i of a plane row: the sample c as the element type's bits
template <int DT>
__device__ __forceinline__ uint32_t tensor_elem(uint32_t c, float s, float b)
{
    if constexpr (DT == TENSOR_U8) return c;
    return tensor_float_bits<DT>(__builtin_fmaf((float)c, s, b));
}

// one plane row of an item: the samples c[0 .. n) as elements at d.  V16:
// n = N = 16 / element size and d is 16-byte aligned.
template <int DT, int N, bool V16>
__device__ __forceinline__ void tensor_store(const uint32_t (&c)[N], int n, float s, float b, uint8_t *d)
{
    constexpr int ES = tensor_elem_size(DT);
    if constexpr (V16) {
        static_assert(N * ES == 16, "a lane stores 16 bytes");
        constexpr int PER = 4 / ES;                 // elements per dword
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if constexpr (ES == 2) {
                // both halves of a dword in one packed conversion
                const tensor_f32x2 f = {__builtin_fmaf((float)c[2 * j], s, b), __builtin_fmaf((float)c[2 * j + 1], s, b)};
                if constexpr (DT == TENSOR_F16) w[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, tensor_f16x2));
                else w[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, tensor_bf16x2));
            } else {
                w[j] = 0;
#pragma unroll
                for (int i = 0; i < PER; i++) {
                    uint32_t v = tensor_elem<DT>(c[PER * j + i], s, b);
                    // the sample as an opaque value: from clamp(x >> 10, 0, 255) | clamp(..) << 8 the
                    // compiler forms v_ashr_pk_u8_i32 and ORs bytes 2 and 3 into its result as if the
                    // upper half were zero, but on gfx950 the instruction leaves the destination's
                    // upper 16 bits as they were (here: those of x, its first source)
                    if constexpr (DT == TENSOR_U8) asm("" : "+v"(v));
                    w[j] |= v << (8 * ES * i);
                }
            }
        }
        const crop_u32x4 o = {w[0], w[1], w[2], w[3]};
        __builtin_nontemporal_store(o, (crop_u32x4 *)d);
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (i >= n) break;
            const uint32_t v = tensor_elem<DT>(c[i], s, b);
            if (ES == 1) __builtin_nontemporal_store((uint8_t)v, d + i);
            else if (ES == 2) __builtin_nontemporal_store((uint16_t)v, (uint16_t *)d + i);
            else __builtin_nontemporal_store(v, (uint32_t *)d + i);
        }
    }
}

// one row of an RGB item interleaved: the samples c[p][0 .. n)
// of the three planes as elements r0 g0 b0 r1 ... at d, each under its own
// plane's s[p], b[p].  V16: n = N = 16 / element size, the row's 3 * N elements
// are 48 bytes and d is 16-byte aligned: three stores.  Element k of the row is
// plane k % 3 of column k / 3, so the two halves of a 16-bit pair are of
// different planes, and a u8 dword holds four samples of three planes.
template <int DT, int N, bool V16>
__device__ __forceinline__ void tensor_store_hwc(const uint32_t (&c)[3][N], int n, const float (&s)[3],
                                                 const float (&b)[3], uint8_t *d)
{
    constexpr int ES = tensor_elem_size(DT);
    if constexpr (V16) {
        static_assert(N * ES == 16, "a lane stores 48 bytes");
        constexpr int PER = 4 / ES;                 // elements per dword
        uint32_t w[12];
#pragma unroll
        for (int j = 0; j < 12; j++) {
            if constexpr (ES == 2) {
                const int k0 = 2 * j, k1 = 2 * j + 1;
                const tensor_f32x2 f = {__builtin_fmaf((float)c[k0 % 3][k0 / 3], s[k0 % 3], b[k0 % 3]),
                                        __builtin_fmaf((float)c[k1 % 3][k1 / 3], s[k1 % 3], b[k1 % 3])};
                if constexpr (DT == TENSOR_F16) w[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, tensor_f16x2));
                else w[j] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, tensor_bf16x2));
            } else {
                w[j] = 0;
#pragma unroll
                for (int i = 0; i < PER; i++) {
                    const int k = PER * j + i;
                    uint32_t v = tensor_elem<DT>(c[k % 3][k / 3], s[k % 3], b[k % 3]);
                    // (opaque, as in tensor_store: v_ashr_pk_u8_i32 keeps its destination's upper half)
                    if constexpr (DT == TENSOR_U8) asm("" : "+v"(v));
                    w[j] |= v << (8 * ES * i);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const crop_u32x4 o = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
            __builtin_nontemporal_store(o, (crop_u32x4 *)d + q);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; i++) {
            if (i >= n) break;
#pragma unroll
            for (int p = 0; p < 3; p++) {
                const uint32_t v = tensor_elem<DT>(c[p][i], s[p], b[p]);
                if (ES == 1) __builtin_nontemporal_store((uint8_t)v, d + 3 * i + p);
                else if (ES == 2) __builtin_nontemporal_store((uint16_t)v, (uint16_t *)d + 3 * i + p);
                else __builtin_nontemporal_store(v, (uint32_t *)d + 3 * i + p);
            }
        }
    }
}

// grid: (ceil(items / 128) blocks of 64 threads, pictures of this launch),
// items = the window's (row pair, 4 * NG-column group) pairs in raster order;
// COL (RGB only): the pixels of a.col (rgba_group_px_set) instead of the
// reference's literal constants; HWC (RGB only): the picture's elements
// interleaved, (ch, cw, 3) -- V16 then asks for rows of 3 * cw elements that
// start on multiples of 16 bytes, which makes cw a multiple of NC as before
template <int MODE, int DT, bool V16, bool COL = false, bool HWC = false>
__global__ __launch_bounds__(64) void k_tensor(const tensor_args a)
{
    static_assert(!HWC || MODE == TENSOR_RGB, "one plane has one order");
    constexpr int ES = tensor_elem_size(DT);
    constexpr int NG = V16 ? 4 / ES : 1;            // 4-column groups per item
    constexpr int NC = 4 * NG;                      // columns per item
    constexpr int NP = MODE == TENSOR_RGB ? 3 : 1;
    const int width = a.width, cpitch = a.cpitch, cw = a.cw;
    const int ni = (cw + NC - 1) / NC;              // items per row pair
    const int nf = ni * (a.ch >> 1);
    const uint8_t *Y = a.in + a.in_off[blockIdx.y];
    const uint8_t *U = Y + (size_t)width * a.height + (size_t)(a.y >> 1) * cpitch + (a.x >> 1);
    const uint8_t *V = U + (size_t)cpitch * (a.height >> 1);
    Y += (size_t)a.y * width + a.x;
    uint8_t *O = a.out + a.out_off[blockIdx.y];
    const size_t plane = a.plane, row = a.row;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = blockIdx.x * 128 + h * 64 + (int)threadIdx.x;
        if (f >= nf) continue;
        const int y2 = f / ni, g = f - y2 * ni;
        const uint8_t *sy = Y + (size_t)(2 * y2) * width + NC * g;
        const size_t co = (size_t)y2 * cpitch + (NC / 2) * g;
        // V16: cw is a multiple of NC; else the row pair's last group can be 2 columns wide
        const bool full = V16 || NC * g + NC <= cw;
        uint32_t y0[NG], y1[NG], u[(NG + 1) / 2], v[(NG + 1) / 2];
        if (full) {
            tensor_load<NG>(sy, y0);
            tensor_load<NG>(sy + width, y1);
        } else {
            y0[0] = crop_load2(sy);
            y1[0] = crop_load2(sy + width);
        }
        if (MODE == TENSOR_RGB) {
            if (NG >= 2) {
                tensor_load<(NG + 1) / 2>(U + co, u);
                tensor_load<(NG + 1) / 2>(V + co, v);
            } else if (full) {
                u[0] = crop_load2(U + co);
                v[0] = crop_load2(V + co);
            } else {
                u[0] = U[co];
                v[0] = V[co];
            }
        }
        // c[row][plane][column]: the samples of the item
        uint32_t c[2][NP][NC];
#pragma unroll
        for (int k = 0; k < NG; k++) {
            if (MODE == TENSOR_RGB) {
                uint32_t o0[4], o1[4];
                const uint32_t u2 = (u[k >> 1] >> (16 * (k & 1))) & 0xFFFFu, v2 = (v[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                if constexpr (COL) rgba_group_px_set(a.col, y0[k], y1[k], u2, v2, o0, o1);
                else rgba_group_px(y0[k], y1[k], u2, v2, o0, o1);
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        c[0][p][4 * k + i] = (o0[i] >> (8 * p)) & 255u;
                        c[1][p][4 * k + i] = (o1[i] >> (8 * p)) & 255u;
                    }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    c[0][0][4 * k + i] = (y0[k] >> (8 * i)) & 255u;
                    c[1][0][4 * k + i] = (y1[k] >> (8 * i)) & 255u;
                }
            }
        }
        const int n = full ? NC : 2;
        if constexpr (HWC) {
            uint8_t *d = O + (size_t)(2 * y2) * row + (size_t)(NC * g) * (3 * ES);
            tensor_store_hwc<DT, NC, V16>(c[0], n, a.scale, a.bias, d);
            tensor_store_hwc<DT, NC, V16>(c[1], n, a.scale, a.bias, d + row);
            continue;
        }
        uint8_t *d = O + (size_t)(2 * y2) * row + (size_t)(NC * g) * ES;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            tensor_store<DT, NC, V16>(c[0][p], n, a.scale[p], a.bias[p], d + p * plane);
            tensor_store<DT, NC, V16>(c[1][p], n, a.scale[p], a.bias[p], d + p * plane + row);
        }
    }
}

// launch for (mode, dtype, v16); items per row pair as in the kernel; col: the
// RGB pixels of a.col; hwc (RGB only): interleaved
static void tensor_launch(int mode, int dt, bool v16, bool col, bool hwc, int npics, hipStream_t st, const tensor_args &a)
{
    const int nc = v16 ? 16 / tensor_elem_size(dt) : 4;
    const int nf = ((a.cw + nc - 1) / nc) * (a.ch >> 1);
    const dim3 grid((nf + 127) >> 7, npics), block(64);
#define TENSOR_HWC_CASE(D, C)                                                                            \
    if (mode == TENSOR_RGB && dt == D && col == C && hwc) {                                               \
        if (v16) hipLaunchKernelGGL((k_tensor<TENSOR_RGB, D, true, C, true>), grid, block, 0, st, a);     \
        else hipLaunchKernelGGL((k_tensor<TENSOR_RGB, D, false, C, true>), grid, block, 0, st, a);        \
        return;                                                                                           \
    }
    TENSOR_HWC_CASE(TENSOR_U8, false) TENSOR_HWC_CASE(TENSOR_F16, false) TENSOR_HWC_CASE(TENSOR_BF16, false)
    TENSOR_HWC_CASE(TENSOR_F32, false) TENSOR_HWC_CASE(TENSOR_U8, true) TENSOR_HWC_CASE(TENSOR_F16, true)
    TENSOR_HWC_CASE(TENSOR_BF16, true) TENSOR_HWC_CASE(TENSOR_F32, true)
#undef TENSOR_HWC_CASE
#define TENSOR_CASE(M, D)                                                                 \
    if (mode == M && dt == D) {                                                           \
        if (v16) hipLaunchKernelGGL((k_tensor<M, D, true>), grid, block, 0, st, a);       \
        else hipLaunchKernelGGL((k_tensor<M, D, false>), grid, block, 0, st, a);          \
    }
#define TENSOR_COL_CASE(D)                                                                        \
    if (mode == TENSOR_RGB && dt == D && col) {                                                   \
        if (v16) hipLaunchKernelGGL((k_tensor<TENSOR_RGB, D, true, true>), grid, block, 0, st, a); \
        else hipLaunchKernelGGL((k_tensor<TENSOR_RGB, D, false, true>), grid, block, 0, st, a);   \
        return;                                                                                   \
    }
    TENSOR_COL_CASE(TENSOR_U8) TENSOR_COL_CASE(TENSOR_F16) TENSOR_COL_CASE(TENSOR_BF16) TENSOR_COL_CASE(TENSOR_F32)
#undef TENSOR_COL_CASE
    TENSOR_CASE(TENSOR_RGB, TENSOR_U8) TENSOR_CASE(TENSOR_RGB, TENSOR_F16)
    TENSOR_CASE(TENSOR_RGB, TENSOR_BF16) TENSOR_CASE(TENSOR_RGB, TENSOR_F32)
    TENSOR_CASE(TENSOR_GRAY, TENSOR_U8) TENSOR_CASE(TENSOR_GRAY, TENSOR_F16)
    TENSOR_CASE(TENSOR_GRAY, TENSOR_BF16) TENSOR_CASE(TENSOR_GRAY, TENSOR_F32)
#undef TENSOR_CASE
}
