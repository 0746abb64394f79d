// The device definitions the reconstruction kernels (recon_kernels.hip) share
// with the export kernels (color.hip, residual.hip, accres.hip): stated once
// here, so that no export file includes recon_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../../include/h264mi_records.h"
#include "../common/mc_window.h"

// (internal linkage: engine.o and exports.o each carry it, and two objects of
// one library may not both define the host shadow of an external device variable)
static __constant__ uint8_t cLevelScale[6][3] = {
    {10, 16, 13}, {11, 18, 14}, {13, 20, 16}, {14, 23, 18}, {16, 25, 20}, {18, 29, 23}};

__device__ __forceinline__ int blk_x(int b) { return mcw_blk_x(b); }
__device__ __forceinline__ int blk_y(int b) { return mcw_blk_y(b); }

// Residual hand-off k_prep -> k_wgpp, compact: only the 4x4 blocks that can
// carry a residual travel, 32 B each, in cbits bit order, from the start of
// the MB's 768-B slot.  res_mask: AC-coded blocks plus every block of a plane
// whose DC transform is coded (I16 luma DC, chroma DC of that plane).
__device__ __forceinline__ uint32_t res_mask(int type, uint32_t cbits)
{
    uint32_t m = cbits & 0xFFFFFFu;
    if (type == MBT_I16 && ((cbits >> 24) & 1)) m |= 0xFFFFu;
    if ((cbits >> 25) & 1) m |= 0xF0000u;
    if ((cbits >> 26) & 1) m |= 0xF00000u;
    return m;
}

// median of three = clamp lo <= x <= hi for lo <= hi, in this form one
// v_med3_i32 (min(max(x, lo), hi) is two instructions unless both bounds are
// constants)
__device__ __forceinline__ int med3i(int x, int lo, int hi) { return min(max(x, lo), max(min(x, lo), hi)); }
