// Display cropping on the device: the SPS crop window (x, y, cw, ch -- all
// even) of a picture, as packed I420 with the byte layout of the reference
// testbench's CropPicture (DecTestBench.c:588-666: luma cw x ch from
// y * width + x, then Cb and Cr (cw / 2) x (ch / 2) from (y / 2) * cpitch +
// x / 2 of their planes) or as RGBA (cw * ch * 4 bytes, color.hip's
// arithmetic: x and y are even, so the RGBA of the crop is the crop of the
// RGBA).  Input: luma rows `width` apart, chroma rows `cpitch` apart (an
// engine slot, or packed I420 with cpitch = width / 2).
//
// HBM-bound elementwise kernels, 64 threads per block, work items in raster
// order (no lane idles at row ends), non-temporal stores.
//
// I420: output rows are packed and cw is only even, so a luma row can start
// 2 mod 4 and a chroma row on any byte.  Rows are not walked: each output
// plane is a flat byte array cut into the 16-byte chunks that are aligned in
// memory, one chunk per lane.  A chunk that lies in one source row is five
// aligned source dwords realigned with v_alignbyte (four when the source is
// aligned too); a chunk that straddles a row end does the same per dword, and
// only the dword on the row end gathers its bytes.  Only a plane's first and
// last chunk can be partial (the plane starts / ends inside them): their
// bytes are stored one by one by the lanes that own them.  A plane whose rows
// are contiguous in the source (pitch == row width) is one long row.
//
// RGBA: the 2-row x 4-column groups of color.hip, over the window; the two
// luma dwords and the chroma pairs come from aligned dwords through
// v_alignbyte (x can be 2 mod 4, x / 2 odd).  With cw a multiple of 4 and a
// 16-byte aligned output a lane stores 2 x 16 bytes as k_yuv2rgba does; else
// 4 x 8 bytes (row starts are 8 mod 16 in odd rows), and a row pair's last
// group is 2 columns wide.

#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "color.hip"
typedef uint32_t crop_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t crop_u32x2 __attribute__((ext_vector_type(2)));

// the 4 source bytes at s (any alignment; all four inside the picture): the
// aligned dwords holding them, realigned.  The second dword is read only
// when s is not aligned (it then holds s + 3).
__device__ __forceinline__ uint32_t crop_load4(const uint8_t *s)
{
    const uint32_t sh = (uint32_t)(uintptr_t)s & 3u;
    const uint32_t *q = (const uint32_t *)(s - sh);
    const uint32_t lo = q[0], hi = q[sh ? 1 : 0];
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

// the 2 source bytes at s (any alignment, both inside the picture), in bits 0..15
__device__ __forceinline__ uint32_t crop_load2(const uint8_t *s)
{
    const uint32_t sh = (uint32_t)(uintptr_t)s & 3u;
    const uint32_t *q = (const uint32_t *)(s - sh);
    const uint32_t lo = q[0], hi = q[sh == 3u ? 1 : 0];
    return __builtin_amdgcn_alignbyte(hi, lo, sh) & 0xFFFFu;
}

// one aligned 16-byte chunk of an output plane: plane bytes [p0, p0 + 16)
// clipped to [0, n).  src = the window's first byte in the source plane, rows
// `pitch` apart and w bytes wide; dst = the plane's first output byte
// (dst + p0 is 16-byte aligned).
__device__ __forceinline__ void crop_chunk(const uint8_t *src, int pitch, int w, int n, uint8_t *dst, int p0)
{
    const int lo = p0 < 0 ? 0 : p0, hi = p0 + 16 < n ? p0 + 16 : n;
    const int row = lo / w;
    int col = lo - row * w;
    const uint8_t *s = src + (size_t)row * pitch + col;
    if (hi - lo < 16) {
        // the plane's first or last chunk: only the bytes that belong to it
        for (int p = lo; p < hi; p++) {
            __builtin_nontemporal_store(*s, dst + p);
            s++;
            if (++col == w) { col = 0; s += pitch - w; }
        }
        return;
    }
    crop_u32x4 o;
    if (col + 16 <= w) {
        const uint32_t sh = (uint32_t)(uintptr_t)s & 3u;
        const uint32_t *q = (const uint32_t *)(s - sh);
        const uint32_t e0 = q[0], e1 = q[1], e2 = q[2], e3 = q[3], e4 = q[sh ? 4 : 3];
        o.x = __builtin_amdgcn_alignbyte(e1, e0, sh);
        o.y = __builtin_amdgcn_alignbyte(e2, e1, sh);
        o.z = __builtin_amdgcn_alignbyte(e3, e2, sh);
        o.w = __builtin_amdgcn_alignbyte(e4, e3, sh);
    } else {
        uint32_t d[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (col + 4 <= w) {
                d[j] = crop_load4(s);
                s += 4;
                col += 4;
                if (col == w) { col = 0; s += pitch - w; }
            } else {
                uint32_t v = 0;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    v |= (uint32_t)*s << (8 * i);
                    s++;
                    if (++col == w) { col = 0; s += pitch - w; }
                }
                d[j] = v;
            }
        }
        o.x = d[0]; o.y = d[1]; o.z = d[2]; o.w = d[3];
    }
    __builtin_nontemporal_store(o, (crop_u32x4 *)(dst + p0));
}

// chunks a plane of n bytes starting at d covers
__device__ __forceinline__ int crop_nchunks(const uint8_t *d, int n) { return ((int)((uintptr_t)d & 15u) + n + 15) >> 4; }

// grid: (ceil(chunks / 128) blocks of 64 threads, npics), chunks = the three
// output planes' aligned 16-byte chunks in raster order (how many depends on
// the picture's output alignment; the launch covers the most); picture k at in + k * in_stride ->
// out + k * out_stride
__global__ __launch_bounds__(64) void k_crop_i420(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int width,
                                                  int height, int cpitch, int x, int y, int cw, int ch,
                                                  size_t in_stride, size_t out_stride)
{
    const int cw2 = cw >> 1, ny = cw * ch, nc = cw2 * (ch >> 1);
    const uint8_t *sY = in + blockIdx.y * in_stride;
    const uint8_t *sU = sY + (size_t)width * height + (size_t)(y >> 1) * cpitch + (x >> 1);
    const uint8_t *sV = sU + (size_t)cpitch * (height >> 1);
    sY += (size_t)y * width + x;
    uint8_t *dY = out + blockIdx.y * out_stride, *dU = dY + ny, *dV = dU + nc;
    const int kY = crop_nchunks(dY, ny), kU = crop_nchunks(dU, nc), kV = crop_nchunks(dV, nc);
    // rows that are contiguous in the source: one long row
    const int wY = cw == width ? ny : cw, wC = cw2 == cpitch ? nc : cw2;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        int c = blockIdx.x * 128 + h * 64 + (int)threadIdx.x;
        if (c < kY) {
            crop_chunk(sY, width, wY, ny, dY, c * 16 - (int)((uintptr_t)dY & 15u));
        } else if ((c -= kY) < kU) {
            crop_chunk(sU, cpitch, wC, nc, dU, c * 16 - (int)((uintptr_t)dU & 15u));
        } else if ((c -= kU) < kV) {
            crop_chunk(sV, cpitch, wC, nc, dV, c * 16 - (int)((uintptr_t)dV & 15u));
        }
    }
}

// grid: (ceil(groups / 128) blocks of 64 threads, npics), groups = the
// window's (row pair, 4-column group) pairs in raster order, ceil(cw / 4) per
// row pair.  V16: cw is a multiple of 4 and the output 16-byte aligned.
template <bool V16>
__global__ __launch_bounds__(64) void k_crop_rgba(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int width,
                                                  int height, int cpitch, int x, int y, int cw, int ch,
                                                  size_t in_stride, size_t out_stride)
{
    const int ng = (cw + 3) >> 2;
    const int nf = ng * (ch >> 1);
    const uint8_t *Y = in + blockIdx.y * in_stride;
    const uint8_t *U = Y + (size_t)width * height + (size_t)(y >> 1) * cpitch + (x >> 1);
    const uint8_t *V = U + (size_t)cpitch * (height >> 1);
    Y += (size_t)y * width + x;
    uint8_t *O = out + blockIdx.y * out_stride;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int f = blockIdx.x * 128 + h * 64 + (int)threadIdx.x;
        if (f >= nf) continue;
        const int y2 = f / ng, g = f - y2 * ng;
        const uint8_t *sy = Y + (size_t)(2 * y2) * width + 4 * g;
        const size_t co = (size_t)y2 * cpitch + 2 * g;
        const bool full = V16 || 4 * g + 4 <= cw;
        uint32_t y0, y1, u2, v2;
        if (full) {
            y0 = crop_load4(sy);
            y1 = crop_load4(sy + width);
            u2 = crop_load2(U + co);
            v2 = crop_load2(V + co);
        } else {
            // the row pair's last 2 columns
            y0 = crop_load2(sy);
            y1 = crop_load2(sy + width);
            u2 = U[co];
            v2 = V[co];
        }
        uint32_t o0[4], o1[4];
        rgba_group_px(y0, y1, u2, v2, o0, o1);
        uint8_t *d0 = O + ((size_t)(2 * y2) * cw + 4 * g) * 4, *d1 = d0 + (size_t)cw * 4;
        if (V16) {
            const crop_u32x4 w0 = {o0[0], o0[1], o0[2], o0[3]}, w1 = {o1[0], o1[1], o1[2], o1[3]};
            __builtin_nontemporal_store(w0, (crop_u32x4 *)d0);
            __builtin_nontemporal_store(w1, (crop_u32x4 *)d1);
        } else {
            const crop_u32x2 a0 = {o0[0], o0[1]}, a1 = {o1[0], o1[1]};
            __builtin_nontemporal_store(a0, (crop_u32x2 *)d0);
            __builtin_nontemporal_store(a1, (crop_u32x2 *)d1);
            if (full) {
                const crop_u32x2 b0 = {o0[2], o0[3]}, b1 = {o1[2], o1[3]};
                __builtin_nontemporal_store(b0, (crop_u32x2 *)(d0 + 8));
                __builtin_nontemporal_store(b1, (crop_u32x2 *)(d1 + 8));
            }
        }
    }
}
