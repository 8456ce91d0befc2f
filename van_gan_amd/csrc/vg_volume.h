// vg_volume.h -- what the preprocessing kernels share (vg_preproc.hip, vg_filters.hip, vg_labelprep.hip): the dtype codes of a
// raw volume and the launch by dtype code, the grid of a streaming pass, the packed load, the non-finite test and the order-preserving
// key of a float.  Everything assumes 256-thread workgroups (4 wave64) on a one-dimensional grid.  The grid-strided loops themselves
// ("four per 16-byte load where aligned, scalar tail") and the wave / LDS / one-atomic counter sum stay written out in their kernels:
// as inline functions taking a lambda they compiled to reordered instruction sequences, which a refactor may not cost.
#pragma once
#include "vg_common.h"

#define VOL_MAX_BLOCKS 2048                 // a streaming pass is grid-strided over at most this many workgroups

static inline bool vol_dtype_ok(int dtype) { return dtype == VG_PP_U8 || dtype == VG_PP_U16 || dtype == VG_PP_F32; }
static inline int vol_esz(int dtype) { return dtype == VG_PP_U8 ? 1 : dtype == VG_PP_U16 ? 2 : 4; }
static inline bool vol_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 60); }
static inline int vol_blocks(int64_t items, int64_t per_block = 256) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (int)(b > VOL_MAX_BLOCKS ? VOL_MAX_BLOCKS : (b < 1 ? 1 : b));
}
// the grid of a flat pass over n elements: a thread per four elements where vec, else per element
static inline dim3 vol_grid(int64_t n, int vec) { return dim3(vol_blocks(vec ? (n + 3) / 4 : n)); }

// f(const T* vol) with T the element type of the dtype code, so that a kernel template is launched by one statement
template <typename F>
static inline void vol_dispatch(const void* vol, int dtype, F&& f) {
    if (dtype == VG_PP_U8) f((const uint8_t*)vol);
    else if (dtype == VG_PP_U16) f((const uint16_t*)vol);
    else f((const float*)vol);
}
template <typename P> struct vol_elem_of;
template <typename T> struct vol_elem_of<const T*> { typedef T type; };
template <typename P> using vol_elem_t = typename vol_elem_of<P>::type;      // vol_elem_t<decltype(v)> inside the lambda

template <typename T, int V> struct alignas(sizeof(T) * V) vol_pack { T v[V]; };    // one load of V elements (up to 16 bytes)

__device__ __forceinline__ unsigned vol_nonfinite_bits(unsigned b) { return (b & 0x7f800000u) == 0x7f800000u; }       // an infinity or a NaN
__device__ __forceinline__ unsigned vol_nonfinite(float x) { return vol_nonfinite_bits(__float_as_uint(x)); }

// key: unsigned order == float order (negatives: all bits flipped; non-negatives: sign bit set), -0.0 directly below +0.0.
__device__ __forceinline__ unsigned vol_key_bits(unsigned b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ unsigned vol_key(float f) { return vol_key_bits(__float_as_uint(f)); }
__device__ __forceinline__ float vol_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

__device__ __forceinline__ double vol_load1(const void* vol, int dtype, int64_t i) {
    if (dtype == VG_PP_U8) return (double)((const uint8_t*)vol)[i];
    if (dtype == VG_PP_U16) return (double)((const uint16_t*)vol)[i];
    return (double)((const float*)vol)[i];
}
