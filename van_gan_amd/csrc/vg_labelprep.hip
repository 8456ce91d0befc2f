// vg_labelprep.hip -- label-domain preprocessing (van_gan_amd/preprocess.py prepare_segmentation; include/vangan_hip.h "Label-volume
// preprocessing"): the exact mode of an fp32 array -- optionally of its min-max normalisation formed on the fly -- by an
// open-addressing hash table in the caller's scratch behind a per-workgroup combiner in LDS, and the label recipe on top of it (min-max,
// inversion when the mode is 1, binarise to {-1, +1}).  Nothing here depends on the 16-bit storage format of the build.
// 256-thread workgroups (4 wave64), grid-strided.  Only integer atomics, and every reduction is a sum or a maximum of integers: the result
// words are bitwise reproducible whatever slot a key lands in.  Every probe loop is bounded by the slot count of its table; no workgroup
// waits on another.
#include "vg_volume.h"

#pragma clang fp contract(off)             // the whole file: every fp32 operation below is rounded on its own, as numpy rounds it

#define LP_EMPTY 0xffffffffu                // a NaN bit pattern: non-finite values are counted, never inserted, so no key equals it
#define LP_HDR_WORDS 16                     // scratch: this header, then slots of (key, count)
#define LP_C0 0                             // count of the value 0 (both signs)
#define LP_C1 1                             // count of the value 1
#define LP_STATUS 2
#define LP_BAD 3                            // non-finite values met
#define LP_BEST 4                           // 64-bit, words 4 and 5: max over the table of (count << 32 | ~order key)
#define LP_LDS_PROBES 16                    // a value that finds no place in the combiner within this many probes goes to the global table
#define LP_BLOCK_ELEMS 8192                 // a workgroup is given at least this many elements (one combiner flush per workgroup)
#define LP_ONE 0x3f800000u

static inline bool lp_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }
static inline int64_t lp_slots(int64_t n) { int64_t s = 2; while (s < 2 * n) s <<= 1; return s; }      // a power of two >= 2 n: load <= 0.5

// murmur3's finaliser: every input bit reaches every output bit, so keys that differ in one byte or in the exponent alone spread out
__device__ __forceinline__ unsigned lp_hash(unsigned k) {
    k ^= k >> 16; k *= 0x85ebca6bu; k ^= k >> 13; k *= 0xc2b2ae35u; k ^= k >> 16;
    return k;
}
// the order key (vol_key_bits) inverted, so that the larger packed word is the SMALLER value
__device__ __forceinline__ unsigned long long lp_pack(unsigned bits, unsigned count) {
    return ((unsigned long long)count << 32) | (unsigned)~vol_key_bits(bits);
}

// count[key] += c in the global table: linear probing from the key's hash, at most one probe per slot.  A slot's key never changes once
// it is set, so a key read as neither empty nor ours is final; only an empty-looking slot is claimed by compare-and-swap.
__device__ __forceinline__ void lp_global_add(unsigned* __restrict__ tab, unsigned mask, unsigned key, unsigned c, unsigned* status) {
    unsigned s = lp_hash(key) & mask;
    for (unsigned long long p = 0; p <= (unsigned long long)mask; ++p) {
        unsigned* slot = tab + (size_t)s * 2;
        unsigned old = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == LP_EMPTY) old = atomicCAS(slot, LP_EMPTY, key);
        if (old == LP_EMPTY || old == key) { atomicAdd(slot + 1, c); return; }
        s = (s + 1) & mask;
    }
    atomicOr(status, 1u);                                           // every slot holds another key: reported, never spun on
}

__global__ __launch_bounds__(256) void lp_init_kernel(unsigned* __restrict__ scratch, int64_t npairs) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    if (tid < LP_HDR_WORDS) scratch[tid] = 0u;
    uint4* tab = (uint4*)(scratch + LP_HDR_WORDS);
    for (int64_t i = tid; i < npairs; i += nthr) tab[i] = make_uint4(LP_EMPTY, 0u, LP_EMPTY, 0u);
}

struct lp_acc { unsigned c0, c1, bad; };

__device__ __forceinline__ void lp_count1(float v, bool norm, float mn, float rng, unsigned* lkey, unsigned* lcnt, unsigned* __restrict__ tab,
                                          unsigned mask, unsigned* hdr, lp_acc& a) {
    const float y = norm ? (v - mn) / rng : v;                      // numpy's (x - min) / (max - min): three roundings, no reciprocal
    unsigned b = __float_as_uint(y);
    if (vol_nonfinite_bits(b)) { ++a.bad; return; }
    if ((b << 1) == 0u) { ++a.c0; return; }                         // -0.0 and +0.0 are one value
    if (b == LP_ONE) { ++a.c1; return; }
    unsigned s = lp_hash(b) & (VG_MODE_LDS_SLOTS - 1);
    for (int p = 0; p < LP_LDS_PROBES; ++p) {
        unsigned old = __hip_atomic_load(&lkey[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == LP_EMPTY) old = atomicCAS(&lkey[s], LP_EMPTY, b);
        if (old == LP_EMPTY || old == b) { atomicAdd(&lcnt[s], 1u); return; }
        s = (s + 1) & (VG_MODE_LDS_SLOTS - 1);
    }
    lp_global_add(tab, mask, b, 1u, hdr + LP_STATUS);
}

// The values 0 and 1 -- nearly everything in a label volume -- are counted in registers and reach the header as one atomic each per
// workgroup; every other finite value goes through the LDS combiner, which is flushed with one global insert per occupied slot.
// V == 4: 16-byte loads, tail through the scalar loop.
template <int V>
__global__ __launch_bounds__(256) void lp_count_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ mm4,
                                                       unsigned* __restrict__ hdr, unsigned* __restrict__ tab, unsigned mask) {
    __shared__ unsigned lkey[VG_MODE_LDS_SLOTS], lcnt[VG_MODE_LDS_SLOTS];
    __shared__ unsigned wred[3][4];
    const int t = threadIdx.x;
    for (int i = t; i < VG_MODE_LDS_SLOTS; i += 256) { lkey[i] = LP_EMPTY; lcnt[i] = 0u; }
    const bool norm = mm4 != nullptr;
    float mn = 0.f, rng = 1.f;
    if (norm) {
        const float mx = mm4[1];
        mn = mm4[0];
        rng = mx - mn;
        if (blockIdx.x == 0 && t == 0 && !(mx > mn)) atomicOr(hdr + LP_STATUS, 2u);
    }
    __syncthreads();
    lp_acc a = {0u, 0u, 0u};
    const int64_t tid = (int64_t)blockIdx.x * 256 + t, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = V == 4 ? n / 4 : 0;
    for (int64_t i = tid; i < nv; i += nthr) {
        const f32x4 v = *(const f32x4*)(x + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) lp_count1(v[j], norm, mn, rng, lkey, lcnt, tab, mask, hdr, a);
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) lp_count1(x[e], norm, mn, rng, lkey, lcnt, tab, mask, hdr, a);
    __syncthreads();
    for (int i = t; i < VG_MODE_LDS_SLOTS; i += 256) {
        const unsigned c = lcnt[i];
        if (c) lp_global_add(tab, mask, lkey[i], c, hdr + LP_STATUS);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a.c0 += __shfl_xor(a.c0, o); a.c1 += __shfl_xor(a.c1, o); a.bad += __shfl_xor(a.bad, o); }
    if ((t & 63) == 0) { wred[0][t >> 6] = a.c0; wred[1][t >> 6] = a.c1; wred[2][t >> 6] = a.bad; }
    __syncthreads();
    if (t < 3) {
        const unsigned tot = wred[t][0] + wred[t][1] + wred[t][2] + wred[t][3];
        if (tot) atomicAdd(hdr + (t == 0 ? LP_C0 : t == 1 ? LP_C1 : LP_BAD), tot);
    }
}

// max over the occupied slots of (count << 32 | ~order key): the highest count, and among equal counts the smallest value
__global__ __launch_bounds__(256) void lp_reduce_kernel(const unsigned* __restrict__ scratch, int64_t npairs, unsigned long long* best) {
    __shared__ unsigned long long wmax[4];
    const uint4* tab = (const uint4*)(scratch + LP_HDR_WORDS);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    unsigned long long m = 0ull;
    for (int64_t i = tid; i < npairs; i += nthr) {
        const uint4 q = tab[i];
        if (q.y) { const unsigned long long c = lp_pack(q.x, q.y); m = c > m ? c : m; }
        if (q.w) { const unsigned long long c = lp_pack(q.z, q.w); m = c > m ? c : m; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(m >> 32), o), lo = __shfl_xor((unsigned)m, o);
        const unsigned long long c = ((unsigned long long)hi << 32) | lo;
        m = c > m ? c : m;
    }
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) m = wmax[i] > m ? wmax[i] : m;
        if (m) atomicMax(best, m);
    }
}

__global__ void lp_final_kernel(const unsigned* __restrict__ hdr, unsigned* __restrict__ result4) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long m = *(const unsigned long long*)(hdr + LP_BEST);
    if (hdr[LP_C0]) { const unsigned long long c = lp_pack(0u, hdr[LP_C0]); m = c > m ? c : m; }
    if (hdr[LP_C1]) { const unsigned long long c = lp_pack(LP_ONE, hdr[LP_C1]); m = c > m ? c : m; }
    const unsigned count = (unsigned)(m >> 32);
    result4[0] = count ? __float_as_uint(vol_unkey(~(unsigned)m)) : 0x7fc00000u;      // no finite value at all: count 0 and a NaN
    result4[1] = count;
    result4[2] = hdr[LP_STATUS];
    result4[3] = hdr[LP_BAD];
}

extern "C" int64_t vg_value_mode_scratch_bytes(int64_t n) {
    if (!lp_n_ok(n)) return VG_EINVAL;
    return (int64_t)LP_HDR_WORDS * 4 + lp_slots(n) * 8;
}

extern "C" int vg_value_mode(const float* x, int64_t n, const float* mm4_or_null, uint32_t* result4, void* scratch, int64_t scratch_bytes,
                             vg_stream_t stream) {
    vg_begin();
    if (!x || !result4 || !scratch || !lp_n_ok(n)) return VG_EINVAL;
    if ((uintptr_t)x % 4 != 0 || (uintptr_t)mm4_or_null % 4 != 0 || (uintptr_t)result4 % 4 != 0) return VG_EINVAL;
    if (scratch_bytes < vg_value_mode_scratch_bytes(n) || (uintptr_t)scratch % 16 != 0) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    unsigned* hdr = (unsigned*)scratch;
    unsigned* tab = hdr + LP_HDR_WORDS;
    const int64_t slots = lp_slots(n), npairs = slots / 2;
    const unsigned mask = (unsigned)(slots - 1);
    const dim3 block(256), sweep(vol_blocks(npairs, 256 * 8));
    hipLaunchKernelGGL(lp_init_kernel, sweep, block, 0, s, hdr, npairs);
    const dim3 grid(vol_blocks(n, LP_BLOCK_ELEMS));
    if ((uintptr_t)x % 16 == 0) hipLaunchKernelGGL(lp_count_kernel<4>, grid, block, 0, s, x, n, mm4_or_null, hdr, tab, mask);
    else hipLaunchKernelGGL(lp_count_kernel<1>, grid, block, 0, s, x, n, mm4_or_null, hdr, tab, mask);
    hipLaunchKernelGGL(lp_reduce_kernel, sweep, block, 0, s, hdr, npairs, (unsigned long long*)(hdr + LP_BEST));
    hipLaunchKernelGGL(lp_final_kernel, dim3(1), dim3(64), 0, s, hdr, result4);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ min-max, inversion, binarise
__device__ __forceinline__ float lp_label1(float v, float mn, float rng, bool inv) {
    float y = (v - mn) / rng;
    if (inv) y = fabsf(y - 1.0f);
    const float z = (y - 0.5f) / 0.5f;
    return z < 0.f ? -1.0f : 1.0f;
}

// x and out may be the same buffer: every element is read and written by the same thread, in that order.
__global__ __launch_bounds__(256) void lp_finish_kernel(const float* x, int64_t n, const float* __restrict__ mm4,
                                                        const unsigned* __restrict__ result4, float* out, unsigned* __restrict__ state, int vec) {
    const float mn = mm4[0], mx = mm4[1];
    const float rng = mx - mn;
    const bool inv = result4[0] == LP_ONE && result4[2] == 0u;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    if (tid == 0) {
        state[1] = inv ? 1u : 0u; state[2] = __float_as_uint(mn); state[3] = __float_as_uint(mx);
        state[4] = result4[0]; state[5] = result4[1]; state[6] = result4[2]; state[7] = result4[3];
    }
    const int64_t nv = vec ? n / 4 : 0;
    for (int64_t i = tid; i < nv; i += nthr) {
        const f32x4 v = *(const f32x4*)(x + i * 4);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = lp_label1(v[j], mn, rng, inv);
        *(f32x4*)(out + i * 4) = o;
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) out[e] = lp_label1(x[e], mn, rng, inv);
}

extern "C" int vg_label_finish(const float* x, int64_t n, const float* mm4, const uint32_t* result4, float* out, uint32_t* state,
                               vg_stream_t stream) {
    vg_begin();
    if (!x || !mm4 || !result4 || !out || !state || !lp_n_ok(n)) return VG_EINVAL;
    if ((uintptr_t)x % 4 != 0 || (uintptr_t)mm4 % 4 != 0 || (uintptr_t)result4 % 4 != 0 || (uintptr_t)out % 4 != 0 || (uintptr_t)state % 4 != 0)
        return VG_EINVAL;
    const int vec = (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0;
    hipLaunchKernelGGL(lp_finish_kernel, vol_grid(n, vec), dim3(256), 0, (hipStream_t)stream, x, n, mm4, result4, out, state, vec);
    return vg_check_launch();
}
