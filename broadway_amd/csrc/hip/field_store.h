// What the four field exports (k_mbinfo, k_residual, k_accmv, k_accres: signed
// values as int16 / fp16 / bf16 / fp32 with a per-channel fma) share: an
// element's bits, an item's store and the launch for (dtype, v16).  From
// tensor.hip it takes tensor_float_bits and tensor_elem_size, from crop.hip
// crop_u32x4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "crop.hip"
#include "tensor.hip"

// v as the element type's bits: int16 keeps v's low 16 bits, the float types
// hold fma((float)v, s, b), converted as in tensor.hip
template <int DT>
__device__ __forceinline__ uint32_t field_elem(int v, float s, float b)
{
    if constexpr (DT == TENSOR_I16) return (uint32_t)v & 0xFFFFu;
    else return tensor_float_bits<DT>(__builtin_fmaf((float)v, s, b));
}

// an item's elements e (field_elem's bits) to d, non-temporally: V16 is 16
// bytes of a row, 8 16-bit or 4 32-bit elements in one store (d is 16-byte
// aligned: the entry points ask that of the output, the picture stride and the
// row bytes); else one element
template <int DT, bool V16, int NE>
__device__ __forceinline__ void field_store(const uint32_t (&e)[NE], uint8_t *d)
{
    constexpr int ES = tensor_elem_size(DT);
    static_assert(NE == (V16 ? 16 / ES : 1), "an item is 16 bytes or one element");
    if constexpr (V16) {
        crop_u32x4 o;
        if constexpr (ES == 2) {
            o.x = e[0] | e[1] << 16; o.y = e[2] | e[3] << 16;
            o.z = e[4] | e[5] << 16; o.w = e[6] | e[7] << 16;
        } else {
            o.x = e[0]; o.y = e[1]; o.z = e[2]; o.w = e[3];
        }
        __builtin_nontemporal_store(o, (crop_u32x4 *)d);
    } else {
        if constexpr (ES == 2) __builtin_nontemporal_store((uint16_t)e[0], (uint16_t *)d);
        else __builtin_nontemporal_store(e[0], (uint32_t *)d);
    }
}

// launch K<dtype, v16> (a field kernel template) with (grid, block, 0, stream, arguments)
#define FIELD_LAUNCH_CASE(K, D, dt, v16, ...)                         \
    if ((dt) == D) {                                                  \
        if (v16) hipLaunchKernelGGL((K<D, true>), __VA_ARGS__);       \
        else hipLaunchKernelGGL((K<D, false>), __VA_ARGS__);          \
    }
#define FIELD_LAUNCH(K, dt, v16, ...)                                 \
    do {                                                              \
        FIELD_LAUNCH_CASE(K, TENSOR_F16, dt, v16, __VA_ARGS__)        \
        FIELD_LAUNCH_CASE(K, TENSOR_BF16, dt, v16, __VA_ARGS__)       \
        FIELD_LAUNCH_CASE(K, TENSOR_F32, dt, v16, __VA_ARGS__)        \
        FIELD_LAUNCH_CASE(K, TENSOR_I16, dt, v16, __VA_ARGS__)        \
    } while (0)
