// vg_preproc.hip -- raw-volume preprocessing (van_gan_amd/preprocess.py; include/vangan_hip.h "Raw-volume preprocessing"):
// per-z-slice moments and z-score of a uint8 / uint16 / float32 volume [X][Y][Z] (Z innermost), the moments of a whole volume (DESIGN.md
// 3.15), exact order statistics of an fp32 array by radix select, and the percentile clip with the rescale to [-1, 1].  What is shared
// with vg_filters.hip and vg_labelprep.hip is in vg_volume.h.  Nothing here depends on the 16-bit storage format of the build.
// All kernels are streaming passes of 256-thread workgroups (4 wave64), grid-strided, a handful of operations per byte moved (times and
// rates: DESIGN.md 3.12); only integer atomics are used, so every result is bitwise reproducible.
#include "vg_volume.h"

static inline bool pp_dims_ok(int64_t nxy, int Z) { return nxy >= 1 && nxy < ((int64_t)1 << 40) && Z >= 1 && Z <= (1 << 20); }

// ------------------------------------------------------------------------------------------------ slice moments
// A thread owns V consecutive z (V: the widest power of two <= 16 bytes, and <= 8 elements, that divides Z and the base alignment, so a
// row start never splits a vector) and walks rows r = (x, y): thread t of the workgroup is column t % ZC of row t / ZC, with
// ZC = min(Z / V, 256) columns and RB = 256 / ZC rows per step, so a step of the workgroup reads RB * ZC * V contiguous elements when ZC
// covers the row.  blockIdx.y selects the column chunk when Z / V > 256.  The fp64 accumulators hold the sums of d = x - pivot and d * d,
// pivot = vol[0][0][z].  The RB threads of a column are added through LDS in ascending row order; the workgroup's partial goes to
// slab[blockIdx.x][z][2].
template <typename T, int V>
__global__ __launch_bounds__(256) void slice_moments_kernel(const T* __restrict__ vol, int64_t nxy, int Z, int ZV, int ZC, int RB,
                                                            double* __restrict__ slab) {
    __shared__ double red[2][256];
    const int t = threadIdx.x, zvl = t % ZC, rloc = t / ZC;
    const int zv = blockIdx.y * ZC + zvl;
    const bool active = rloc < RB && zv < ZV;
    double s[V], q[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = q[j] = 0.0;
    if (active) {
        const T* col = vol + (size_t)zv * V;
        const vol_pack<T, V> p0 = *(const vol_pack<T, V>*)col;
        double piv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) piv[j] = (double)p0.v[j];
#pragma unroll 2
        for (int64_t r = (int64_t)blockIdx.x * RB + rloc; r < nxy; r += (int64_t)gridDim.x * RB) {
            const vol_pack<T, V> p = *(const vol_pack<T, V>*)(col + (size_t)r * Z);
#pragma unroll
            for (int j = 0; j < V; ++j) { const double d = (double)p.v[j] - piv[j]; s[j] += d; q[j] += d * d; }
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        red[0][t] = s[j]; red[1][t] = q[j];
        __syncthreads();
        if (active && rloc == 0)
            for (int rr = 1; rr < RB; ++rr) { s[j] += red[0][rr * ZC + zvl]; q[j] += red[1][rr * ZC + zvl]; }
        __syncthreads();
    }
    if (active && rloc == 0) {
        double* o = slab + ((size_t)blockIdx.x * Z + (size_t)zv * V) * 2;
#pragma unroll
        for (int j = 0; j < V; ++j) { o[2 * j] = s[j]; o[2 * j + 1] = q[j]; }
    }
}

// One wave per z: lane l adds the partials of workgroups l, l + 64, ... in ascending order, then a butterfly (both partners form the same
// sum, a + b == b + a) -- a fixed association.  mean = pivot + S / n, var = Q / n - (S / n)^2, each rounded once to fp32.
// FLAT: the one slice of a flat array (vg_volume_moments), Z = 1 and z = 0 known to the compiler.
template <bool FLAT>
__global__ __launch_bounds__(64) void slice_moments_final_kernel(const double* __restrict__ slab, int nb, int Zrt, int64_t nxy,
                                                                 const void* __restrict__ vol, int dtype, float* __restrict__ mean_std) {
    const int Z = FLAT ? 1 : Zrt, z = FLAT ? 0 : blockIdx.x, lane = threadIdx.x;
    double s = 0.0, q = 0.0;
    for (int b = lane; b < nb; b += 64) { const double* p = slab + ((size_t)b * Z + z) * 2; s += p[0]; q += p[1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
    if (lane == 0) {
        const double n = (double)nxy, ms = s / n;
        double var = q / n - ms * ms;
        if (var < 0.0) var = 0.0;                                   // a NaN stays a NaN
        mean_std[2 * z] = (float)(vol_load1(vol, dtype, z) + ms);
        mean_std[2 * z + 1] = (float)sqrt(var);
    }
}

template <typename T, int V>
static void moments_launch(const void* vol, int64_t nxy, int Z, double* slab, int* nbx_out, hipStream_t s) {
    const int ZV = Z / V, ZC = ZV < 256 ? ZV : 256, RB = 256 / ZC, nzc = (ZV + ZC - 1) / ZC;
    int64_t nbx = cdiv64(nxy, RB);
    const int cap = 1024 / nzc < 1 ? 1 : 1024 / nzc;                // <= min(nxy, 1024): what vg_slice_moments_scratch_bytes provides for
    if (nbx > cap) nbx = cap;
    *nbx_out = (int)nbx;
    hipLaunchKernelGGL((slice_moments_kernel<T, V>), dim3((unsigned)nbx, (unsigned)nzc), dim3(256), 0, s, (const T*)vol, nxy, Z, ZV, ZC, RB, slab);
}

template <typename T>
static void moments_dispatch(const T* vol, int64_t nxy, int Z, double* slab, int* nbx, hipStream_t s) {
    constexpr int VM = sizeof(T) == 1 ? 8 : 16 / (int)sizeof(T);      // u8 stops at 8 bytes: 16 fp64 accumulator pairs per lane cost 176 VGPRs
    int V = VM;
    while (V > 1 && (Z % V != 0 || (uintptr_t)vol % (V * sizeof(T)) != 0)) V >>= 1;
    if (V == 1) moments_launch<T, 1>(vol, nxy, Z, slab, nbx, s);
    else if (V == 2) moments_launch<T, 2>(vol, nxy, Z, slab, nbx, s);
    else if (V == 4) moments_launch<T, 4>(vol, nxy, Z, slab, nbx, s);
    else if constexpr (VM >= 8) moments_launch<T, 8>(vol, nxy, Z, slab, nbx, s);
}

extern "C" int64_t vg_slice_moments_scratch_bytes(int64_t nxy, int Z) {
    if (!pp_dims_ok(nxy, Z)) return VG_EINVAL;
    return (nxy < 1024 ? nxy : 1024) * (int64_t)Z * 2 * (int64_t)sizeof(double);
}

extern "C" int vg_slice_moments(const void* vol, int dtype, int64_t nxy, int Z, float* mean_std, void* scratch, int64_t scratch_bytes,
                                vg_stream_t stream) {
    vg_begin();
    if (!vol || !mean_std || !scratch || !pp_dims_ok(nxy, Z) || !vol_dtype_ok(dtype)) return VG_EINVAL;
    if (scratch_bytes < vg_slice_moments_scratch_bytes(nxy, Z) || (uintptr_t)scratch % 16 != 0) return VG_EINVAL;
    if ((dtype == VG_PP_U16 && (uintptr_t)vol % 2 != 0) || (dtype == VG_PP_F32 && (uintptr_t)vol % 4 != 0)) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    double* slab = (double*)scratch;
    int nbx = 0;
    vol_dispatch(vol, dtype, [&](auto* v) { moments_dispatch(v, nxy, Z, slab, &nbx, s); });
    hipLaunchKernelGGL(slice_moments_final_kernel<false>, dim3(Z), dim3(64), 0, s, slab, nbx, Z, nxy, vol, dtype, mean_std);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ moments of the whole volume
// The same accumulation on one flat array: fp64 sums of d = x - vol[0] and of d * d per thread (grid-strided, four elements per load
// where the pointer allows), added through LDS in a
// fixed tree; the workgroup's pair goes to part[blockIdx.x], which is slab[blockIdx.x][z = 0] of a volume with Z = 1 and nxy = n, so
// slice_moments_final_kernel finishes it with one workgroup.
template <typename T>
__global__ __launch_bounds__(256) void volume_moments_kernel(const T* __restrict__ vol, int64_t n, int vec, double* __restrict__ part) {
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    const int64_t tid = (int64_t)blockIdx.x * 256 + t, nthr = (int64_t)gridDim.x * 256;
    const double piv = (double)vol[0];
    const int64_t nv = vec ? n / 4 : 0;
    double s = 0.0, q = 0.0;
    for (int64_t i = tid; i < nv; i += nthr) {
        const vol_pack<T, 4> p = *(const vol_pack<T, 4>*)(vol + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { const double d = (double)p.v[j] - piv; s += d; q += d * d; }
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) { const double d = (double)vol[e] - piv; s += d; q += d * d; }
    red[0][t] = s; red[1][t] = q;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { red[0][t] += red[0][t + o]; red[1][t] += red[1][t + o]; }
        __syncthreads();
    }
    if (t == 0) { part[2 * blockIdx.x] = red[0][0]; part[2 * blockIdx.x + 1] = red[1][0]; }
}

extern "C" int64_t vg_volume_moments_scratch_bytes(int64_t n) {
    if (!vol_n_ok(n)) return VG_EINVAL;
    return (int64_t)VOL_MAX_BLOCKS * 2 * (int64_t)sizeof(double);
}

extern "C" int vg_volume_moments(const void* vol, int dtype, int64_t n, float* mean_std, void* scratch, int64_t scratch_bytes,
                                 vg_stream_t stream) {
    vg_begin();
    if (!vol || !mean_std || !scratch || !vol_n_ok(n) || !vol_dtype_ok(dtype)) return VG_EINVAL;
    if (scratch_bytes < vg_volume_moments_scratch_bytes(n) || (uintptr_t)scratch % 16 != 0 || (uintptr_t)mean_std % 4 != 0) return VG_EINVAL;
    const int esz = vol_esz(dtype);
    if ((uintptr_t)vol % esz != 0) return VG_EINVAL;
    const int vec = (uintptr_t)vol % (4 * esz) == 0;
    const dim3 grid = vol_grid(n, vec);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)scratch;
    vol_dispatch(vol, dtype, [&](auto* v) {
        hipLaunchKernelGGL(volume_moments_kernel<vol_elem_t<decltype(v)>>, grid, dim3(256), 0, s, v, n, vec, part);
    });
    hipLaunchKernelGGL(slice_moments_final_kernel<true>, dim3(1), dim3(64), 0, s, part, (int)grid.x, 1, n, vol, dtype, mean_std);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ z-score
__device__ __forceinline__ float zscore1(float x, const float* __restrict__ ms, int z, unsigned& bad) {
    const float2 p = *(const float2*)(ms + 2 * z);
    const float d = x - p.x;
    const float r = p.y > 0.f ? d / p.y : d;                        // the reference's zero-std branch (utils.py:79-82)
    bad += vol_nonfinite(r);
    return r;
}

// Flat over the volume, four elements per lane: a 16-byte store and a 4 / 8 / 16-byte load (u8 / u16 / f32); z of an element is its flat
// index mod Z, taken once per thread (64-bit) and advanced by the grid stride mod Z.  vec == 0 (Z < 4 or a misaligned pointer): one
// element per lane.  The elements past the last whole vector go through the scalar loop.
template <typename T>
__global__ __launch_bounds__(256) void zscore_kernel(const T* __restrict__ vol, int64_t n, int Z, const float* __restrict__ ms,
                                                     float* __restrict__ out, unsigned* nonfinite, int vec) {
    __shared__ unsigned wbad[4];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = vec ? n / 4 : 0;
    unsigned bad = 0;
    if (nv) {
        int z = (int)((tid * 4) % Z);
        const int adv = (int)((nthr * 4) % Z);
        for (int64_t i = tid; i < nv; i += nthr) {
            const vol_pack<T, 4> p = *(const vol_pack<T, 4>*)(vol + i * 4);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int zz = z + j;
                zz -= zz >= Z ? Z : 0;                              // Z >= 4 on this path: at most one wrap
                o[j] = zscore1((float)p.v[j], ms, zz, bad);
            }
            *(f32x4*)(out + i * 4) = o;
            z += adv;
            z -= z >= Z ? Z : 0;
        }
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) out[e] = zscore1((float)vol[e], ms, (int)(e % Z), bad);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0) wbad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = wbad[0] + wbad[1] + wbad[2] + wbad[3];
        if (tot) atomicAdd(nonfinite, tot);                         // result unused: a non-returning atomic
    }
}

extern "C" int vg_zscore_slices(const void* vol, int dtype, int64_t nxy, int Z, const float* mean_std, float* out, uint32_t* nonfinite,
                                vg_stream_t stream) {
    vg_begin();
    if (!vol || !mean_std || !out || !nonfinite || !pp_dims_ok(nxy, Z) || !vol_dtype_ok(dtype)) return VG_EINVAL;
    if ((uintptr_t)mean_std % 8 != 0 || (uintptr_t)out % 4 != 0 || (uintptr_t)nonfinite % 4 != 0) return VG_EINVAL;
    const int64_t n = nxy * Z;
    const int esz = vol_esz(dtype);
    if ((uintptr_t)vol % esz != 0) return VG_EINVAL;
    const int vec = Z >= 4 && (uintptr_t)vol % (4 * esz) == 0 && (uintptr_t)out % 16 == 0;
    vol_dispatch(vol, dtype, [&](auto* v) {
        hipLaunchKernelGGL(zscore_kernel<vol_elem_t<decltype(v)>>, vol_grid(n, vec), dim3(256), 0, (hipStream_t)stream, v, n, Z, mean_std, out,
                           nonfinite, vec);
    });
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ order statistics (radix select)
// On the keys of vg_volume.h (vol_key: unsigned order == float order).
// scratch, in 32-bit words: hist[VG_PP_MAX_RANKS][256] | prefix[4] (the key digits chosen so far, in place) | rem[4] (rank among the
// elements that share the prefix).  Kernel boundaries on the stream are the only synchronisation.
#define PP_HIST_WORDS (VG_PP_MAX_RANKS * 256)
#define PP_STATE_WORDS (PP_HIST_WORDS + 2 * VG_PP_MAX_RANKS)
struct pp_ranks { unsigned r[VG_PP_MAX_RANKS]; };

__global__ __launch_bounds__(256) void os_init_kernel(unsigned* __restrict__ st, pp_ranks rk, int R) {
    const int t = threadIdx.x;
    for (int i = t; i < PP_HIST_WORDS; i += 256) st[i] = 0u;
    if (t < VG_PP_MAX_RANKS) { st[PP_HIST_WORDS + t] = 0u; st[PP_HIST_WORDS + VG_PP_MAX_RANKS + t] = t < R ? rk.r[t] : 0u; }
}

// Ranks whose prefixes are equal so far count the same elements: only the first of them (src[r] == r) is counted, the others read its row.
__device__ __forceinline__ void os_load_state(const unsigned* __restrict__ st, int R, unsigned* pre, int* src) {
#pragma unroll
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r) {
        pre[r] = r < R ? st[PP_HIST_WORDS + r] : 0u;
        src[r] = r;
#pragma unroll
        for (int p = r - 1; p >= 0; --p) if (pre[p] == pre[r]) src[r] = p;
    }
}

__device__ __forceinline__ void os_count(unsigned (*h)[256], float v, int R, int shift, unsigned mask, const unsigned* pre, const int* src) {
    const unsigned key = vol_key(v), d = (key >> shift) & 255u;
#pragma unroll
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r)
        if (r < R && src[r] == r && ((key ^ pre[r]) & mask) == 0u) atomicAdd(&h[r][d], 1u);
}

// Histogram of digit (key >> shift) & 255 over the elements whose higher digits equal the rank's prefix: LDS counters per workgroup,
// non-zero bins flushed with integer atomics (at most R * 256 per workgroup).  V == 4: 16-byte loads, tail through the scalar loop.
template <int V>
__global__ __launch_bounds__(256) void os_hist_kernel(const float* __restrict__ x, int64_t n, int R, int shift, unsigned* __restrict__ st) {
    __shared__ unsigned h[VG_PP_MAX_RANKS][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r) h[r][t] = 0u;
    unsigned pre[VG_PP_MAX_RANKS]; int src[VG_PP_MAX_RANKS];
    os_load_state(st, R, pre, src);
    const unsigned mask = shift >= 24 ? 0u : 0xffffffffu << (shift + 8);
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * 256 + t, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = V == 4 ? n / 4 : 0;
    for (int64_t i = tid; i < nv; i += nthr) {
        const f32x4 v = *(const f32x4*)(x + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) os_count(h, v[j], R, shift, mask, pre, src);
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) os_count(h, x[e], R, shift, mask, pre, src);
    __syncthreads();
    for (int r = 0; r < R; ++r) { const unsigned c = h[r][t]; if (c) atomicAdd(&st[r * 256 + t], c); }
}

// One workgroup, thread t = bin t.  Per rank: exclusive scan of the 256 counts; the one bin with excl <= rem < excl + count is the next
// digit.  Everything is read before anything is written (first barrier); the histogram is cleared for the next pass.  After the last
// digit (shift == 0) the prefix is the whole key of the selected value.
__global__ __launch_bounds__(256) void os_scan_kernel(unsigned* __restrict__ st, int R, int shift, float* __restrict__ out) {
    __shared__ unsigned wsum[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned pre[VG_PP_MAX_RANKS], rem[VG_PP_MAX_RANKS], c[VG_PP_MAX_RANKS]; int src[VG_PP_MAX_RANKS];
    os_load_state(st, R, pre, src);
#pragma unroll
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r) {
        rem[r] = r < R ? st[PP_HIST_WORDS + VG_PP_MAX_RANKS + r] : 0u;
        c[r] = 0u;
    }
#pragma unroll
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r)
#pragma unroll
        for (int p = 0; p <= r; ++p) if (r < R && src[r] == p) c[r] = st[p * 256 + t];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r) st[r * 256 + t] = 0u;
#pragma unroll
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r) {
        if (r >= R) break;                                          // uniform
        unsigned inc = c[r];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned y = __shfl_up(inc, o); if (lane >= o) inc += y; }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        unsigned excl = inc - c[r];
        for (int ww = 0; ww < w; ++ww) excl += wsum[ww];
        if (c[r] != 0u && rem[r] >= excl && rem[r] - excl < c[r]) {
            const unsigned np = pre[r] | ((unsigned)t << shift);
            st[PP_HIST_WORDS + r] = np;
            st[PP_HIST_WORDS + VG_PP_MAX_RANKS + r] = rem[r] - excl;
            if (shift == 0) out[r] = vol_unkey(np);
        }
        __syncthreads();
    }
}

extern "C" int64_t vg_order_stats_scratch_bytes(int64_t n, int R) {
    if (n < 1 || n >= ((int64_t)1 << 31) || R < 1 || R > VG_PP_MAX_RANKS) return VG_EINVAL;
    return (int64_t)PP_STATE_WORDS * 4;
}

extern "C" int vg_order_stats(const float* x, int64_t n, const int64_t* ranks_host, int R, float* out, void* scratch, int64_t scratch_bytes,
                              vg_stream_t stream) {
    vg_begin();
    if (!x || !ranks_host || !out || !scratch) return VG_EINVAL;
    if (n < 1 || n >= ((int64_t)1 << 31) || R < 1 || R > VG_PP_MAX_RANKS) return VG_EINVAL;     // n < 2^31: 32-bit bin counts cannot overflow
    if (scratch_bytes < vg_order_stats_scratch_bytes(n, R) || (uintptr_t)scratch % 16 != 0 || (uintptr_t)x % 4 != 0 || (uintptr_t)out % 4 != 0)
        return VG_EINVAL;
    pp_ranks rk;
    for (int r = 0; r < VG_PP_MAX_RANKS; ++r) {
        if (r < R && (ranks_host[r] < 0 || ranks_host[r] >= n)) return VG_EINVAL;
        rk.r[r] = r < R ? (unsigned)ranks_host[r] : 0u;
    }
    hipStream_t s = (hipStream_t)stream;
    unsigned* st = (unsigned*)scratch;
    const bool vec = (uintptr_t)x % 16 == 0;
    const dim3 grid = vol_grid(n, vec), block(256);
    hipLaunchKernelGGL(os_init_kernel, dim3(1), block, 0, s, st, rk, R);
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (vec) hipLaunchKernelGGL(os_hist_kernel<4>, grid, block, 0, s, x, n, R, shift, st);
        else hipLaunchKernelGGL(os_hist_kernel<1>, grid, block, 0, s, x, n, R, shift, st);
        hipLaunchKernelGGL(os_scan_kernel, dim3(1), block, 0, s, st, R, shift, out);
    }
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ percentile clip + rescale
// Why no min / max reduction follows the clip (the reference's min_max_norm, utils.py:20-24, takes one): a percentile of a sample lies in
// [min, max] of that sample -- it is a convex combination of two of its order statistics -- and rounding to fp32 is monotonic, so the
// rounded lp still has an fp32 sample value <= it and the rounded up one >= it.  After c = clip(z, lp, up) the minimum of c is therefore
// exactly lp and its maximum exactly up, which are already in registers.  lp maps to (0 - 0.5) / 0.5 = -1 and up to (1 - 0.5) / 0.5 = 1.
// The limits follow scipy.stats.scoreatpercentile ('fraction'): a[i] * (1 - f) + a[i+1] * f in fp64, every operation rounded (no FMA).
__device__ __forceinline__ float pp_limit(float a, float b, double f) {
    return (float)__dadd_rn(__dmul_rn((double)a, 1.0 - f), __dmul_rn((double)b, f));
}
__device__ __forceinline__ float clip1(float v, float lp, float up, float rng, int rescale) {
#pragma clang fp contract(off)
    const float c = v < lp ? lp : (v > up ? up : v);                // numpy's img[img < lp] = lp; img[img > up] = up: a NaN passes through
    if (!rescale) return c;
    const float u = (c - lp) / rng;
    return (u - 0.5f) / 0.5f;
}

__global__ __launch_bounds__(256) void clip_rescale_kernel(const float* z, int64_t n, const float* __restrict__ stats4, double f_lo, double f_hi,
                                                           int rescale, float* __restrict__ limits2, float* out, int vec) {
    const float lp = pp_limit(stats4[0], stats4[1], f_lo), up = pp_limit(stats4[2], stats4[3], f_hi);
    const float rng = up - lp;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    if (tid == 0) { limits2[0] = lp; limits2[1] = up; }
    const int64_t nv = vec ? n / 4 : 0;
    for (int64_t i = tid; i < nv; i += nthr) {
        const f32x4 v = *(const f32x4*)(z + i * 4);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = clip1(v[j], lp, up, rng, rescale);
        *(f32x4*)(out + i * 4) = o;
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) out[e] = clip1(z[e], lp, up, rng, rescale);
}

extern "C" int vg_clip_rescale(const float* z, int64_t n, const float* stats4, double f_lo, double f_hi, int rescale, float* limits2,
                               float* out, vg_stream_t stream) {
    vg_begin();
    if (!z || !stats4 || !limits2 || !out || !vol_n_ok(n)) return VG_EINVAL;
    if (!(f_lo >= 0.0 && f_lo <= 1.0) || !(f_hi >= 0.0 && f_hi <= 1.0) || (rescale != 0 && rescale != 1)) return VG_EINVAL;
    if ((uintptr_t)z % 4 != 0 || (uintptr_t)out % 4 != 0 || (uintptr_t)stats4 % 4 != 0 || (uintptr_t)limits2 % 4 != 0) return VG_EINVAL;
    const int vec = (uintptr_t)z % 16 == 0 && (uintptr_t)out % 16 == 0;
    hipLaunchKernelGGL(clip_rescale_kernel, vol_grid(n, vec), dim3(256), 0, (hipStream_t)stream, z, n, stats4, f_lo, f_hi, rescale, limits2, out,
                       vec);
    return vg_check_launch();
}
