// vg_filters.hip -- imaging filters (van_gan_amd/preprocess.py; include/vangan_hip.h "Imaging filters"): the 3-D / slice-wise
// median of a uint8 / uint16 / float32 volume [X][Y][Z] (Z innermost) with scipy's 'reflect' boundary, and the selection half of
// threshold_outliers (utils.py:108-133): the extreme values within `threshold` standard deviations of the mean (the moments of the whole
// volume, vg_volume_moments, are in vg_preproc.hip beside the slice moments).  What is shared with the other preprocessing files: vg_volume.h.
// Nothing here depends on the 16-bit storage format of the build.  256-thread workgroups (4 wave64); only integer atomics are used, so
// every result is bitwise reproducible.
#include "vg_volume.h"

// ------------------------------------------------------------------------------------------------ median
// A workgroup owns a tile of MF_TY x MF_TZ outputs in (y, z) -- thread t is (y, z) = (t / MF_TZ, t % MF_TZ), so a wave covers two rows of 32
// consecutive z and loads and stores run along the contiguous axis -- and marches along x over MF_XC planes.  Every plane it meets is
// staged once in LDS with its one-voxel halo in y and z (converted to fp32; the halo indices are clamped, which for a window of 3 is
// scipy's 'reflect': -1 reads 0 and n reads n - 1), double-buffered, one barrier per plane; the loads run MF_DEPTH planes ahead of the
// selection, each plane in a register set of its own (the plane loop is unrolled by MF_DEPTH, so no set is ever copied), because a
// workgroup's plane is only about 1 KiB and one plane in flight per workgroup leaves the kernel waiting on load latency.  A thread keeps
// the SX planes of its window in registers (SY * SZ values each, read from LDS once and ordered once: mf_prep), shifts them by one plane
// per step, and takes the median of the M = SX * SY * SZ values with min / max / med3 on registers (mf_median): about 140 of them per
// output for 3x3x3, 13 for the slice-wise 3x3.
#define MF_TY 8
#define MF_TZ 32
#define MF_XC 32
#define MF_DEPTH 4                 // planes whose loads are in flight per workgroup

__device__ __forceinline__ void mf_cx(float& a, float& b) {        // compare-exchange: a <= b afterwards
    const float lo = __builtin_fminf(a, b), hi = __builtin_fmaxf(a, b);
    a = lo; b = hi;
}

// Selection by discarding extremes: among any K = N / 2 + 2 of N values neither the smallest nor the largest is the median of the N, so
// both are dropped and one further value joins; the set shrinks by one per round until three are left, whose median is the answer.  A
// round pairs a[i] with a[K - 1 - i], which leaves the minimum among the lower and the maximum among the upper partners, and moves them
// to a[0] and a[K - 1] by compare-exchanges.  Branch-free min / max on registers: every loop bound is a template constant.
template <int M, int K, int NEXT>
__device__ __forceinline__ float mf_round(float (&a)[M / 2 + 2], const float (&v)[M]) {
    if constexpr (K == 3) {
        return __builtin_amdgcn_fmed3f(a[0], a[1], a[2]);
    } else {
        constexpr int p = K / 2;
#pragma unroll
        for (int i = 0; i < p; ++i) mf_cx(a[i], a[K - 1 - i]);
#pragma unroll
        for (int i = 1; i < p; ++i) mf_cx(a[0], a[i]);
#pragma unroll
        for (int i = 1; i < p; ++i) mf_cx(a[K - 1 - i], a[K - 1]);
        if constexpr (K % 2 == 1) { mf_cx(a[0], a[p]); mf_cx(a[p], a[K - 1]); }      // the unpaired middle value
        a[0] = v[NEXT];                                                            // a[0] and a[K - 1] are dropped, v[NEXT] joins
        return mf_round<M, K - 1, NEXT + 1>(a, v);
    }
}

template <int M>
__device__ __forceinline__ float mf_select(const float (&v)[M]) {
    if constexpr (M == 1) return v[0];
    else if constexpr (M == 3) return __builtin_amdgcn_fmed3f(v[0], v[1], v[2]);
    else {
        constexpr int K0 = M / 2 + 2;
        float a[K0];
#pragma unroll
        for (int i = 0; i < K0; ++i) a[i] = v[i];
        return mf_round<M, K0, K0>(a, v);
    }
}

// The two required windows do less work than a selection among all their values, because a thread meets every plane three times
// (as the newest, the middle and the oldest plane of its window) and can order it once.
__device__ __forceinline__ float mf_min3(float a, float b, float c) { return __builtin_fminf(__builtin_fminf(a, b), c); }     // v_min3_f32
__device__ __forceinline__ float mf_max3(float a, float b, float c) { return __builtin_fmaxf(__builtin_fmaxf(a, b), c); }     // v_max3_f32
__device__ __forceinline__ float mf_med3(float a, float b, float c) { return __builtin_amdgcn_fmed3f(a, b, c); }
__device__ __forceinline__ void mf_sort3(float& a, float& b, float& c) {           // three instructions
    const float lo = mf_min3(a, b, c), md = mf_med3(a, b, c), hi = mf_max3(a, b, c);
    a = lo; b = md; c = hi;
}

// What a plane's P = SY * SZ values become when they enter the window (v[dy * SZ + dz] on entry).
//   SX == 3, P == 3 (the slice-wise 3x3 median and its transposes): the sorted triple.
//   SX == 3, P == 9 (3x3x3): each of the three z-triples is sorted into (lo, mid, hi); then the three lo, the three mid and the three hi are
//     sorted among themselves: v = (L0 <= L1 <= L2, M0 <= M1 <= M2, H0 <= H1 <= H2).
//   otherwise: unchanged, and the median is selected among all M values.
template <int SX, int P>
__device__ __forceinline__ void mf_prep(float (&v)[P]) {
    if constexpr (SX == 3 && P == 3) {
        mf_sort3(v[0], v[1], v[2]);
    } else if constexpr (SX == 3 && P == 9) {
        mf_sort3(v[0], v[1], v[2]); mf_sort3(v[3], v[4], v[5]); mf_sort3(v[6], v[7], v[8]);
        float l0 = v[0], l1 = v[3], l2 = v[6], m0 = v[1], m1 = v[4], m2 = v[7], h0 = v[2], h1 = v[5], h2 = v[8];
        mf_sort3(l0, l1, l2); mf_sort3(m0, m1, m2); mf_sort3(h0, h1, h2);
        v[0] = l0; v[1] = l1; v[2] = l2; v[3] = m0; v[4] = m1; v[5] = m2; v[6] = h0; v[7] = h1; v[8] = h2;
    }
}

// The median of the window w = SX planes of P prepared values.
//   P == 3: three sorted columns; the median of the nine is the median of (largest low, middle mid, smallest high).
//   P == 9: the 27 values are nine sorted triples (lo, mid, hi).  The k-th smallest lo has the 9 - k lo above it, their mid and hi, and its
//     own mid and hi above it: 3 (9 - k) + 2 >= 14 values for k <= 5, so the five smallest lo lie below the median (rank 13); so do the
//     two smallest mid (2 (9 - k) + 1 >= 14 for k <= 2), and by symmetry the five largest hi and the two largest mid lie above it.  Seven
//     dropped on either side leave the four largest lo, the five middle mid and the four smallest hi, and the median of the 27 is the
//     median of these 13.  Each group of nine is three sorted triples (one per plane); sorting across the planes rank by rank gives a 3 x 3
//     table T[i][j] ordered along both axes, in which (i + 1)(j + 1) - 1 values lie below T[i][j] and (3 - i)(3 - j) - 1 above: the four
//     largest are T22, T21, T12 and the largest of (T02, T11, T20); the two smallest are T00 and the smaller of (T01, T10).
template <int SX, int P>
__device__ __forceinline__ float mf_median(const float (&w)[SX * P]) {
    if constexpr (SX == 3 && P == 3) {
        return mf_med3(mf_max3(w[0], w[3], w[6]), mf_med3(w[1], w[4], w[7]), mf_min3(w[2], w[5], w[8]));
    } else if constexpr (SX == 3 && P == 9) {
        const float* a = w; const float* b = w + 9; const float* c = w + 18;
        float s[13];
        // lo: the four largest
        s[0] = mf_max3(a[2], b[2], c[2]);
        s[1] = mf_med3(a[2], b[2], c[2]);
        s[2] = mf_max3(a[1], b[1], c[1]);
        s[3] = mf_max3(mf_max3(a[0], b[0], c[0]), mf_med3(a[1], b[1], c[1]), mf_min3(a[2], b[2], c[2]));
        // hi: the four smallest
        s[4] = mf_min3(a[6], b[6], c[6]);
        s[5] = mf_med3(a[6], b[6], c[6]);
        s[6] = mf_min3(a[7], b[7], c[7]);
        s[7] = mf_min3(mf_min3(a[8], b[8], c[8]), mf_med3(a[7], b[7], c[7]), mf_max3(a[6], b[6], c[6]));
        // mid: all but the two smallest and the two largest
        s[8] = __builtin_fmaxf(mf_med3(a[3], b[3], c[3]), mf_min3(a[4], b[4], c[4]));
        s[9] = __builtin_fminf(mf_med3(a[5], b[5], c[5]), mf_max3(a[4], b[4], c[4]));
        s[10] = mf_max3(a[3], b[3], c[3]);
        s[11] = mf_med3(a[4], b[4], c[4]);
        s[12] = mf_min3(a[5], b[5], c[5]);
        return mf_select<13>(s);
    } else {
        return mf_select<SX * P>(w);
    }
}

template <typename T, int SX, int SY, int SZ>
__global__ __launch_bounds__(256) void median3_kernel(const T* __restrict__ vol, int X, int Y, int Z, int nyt, int nzt, int64_t ntiles,
                                                      float* __restrict__ out, unsigned* nonfinite) {
    constexpr int HX = SX / 2, HY = SY / 2, HZ = SZ / 2, PW = MF_TZ + 2 * HZ, PH = MF_TY + 2 * HY, PE = PW * PH, P = SY * SZ, M = SX * P;
    constexpr int NL = (PE + 255) / 256;                            // elements of a plane per thread
    __shared__ float plane[2][NL * 256];                           // PE used; the rest takes the surplus threads' stores
    __shared__ unsigned wbad[4];
    const int t = threadIdx.x, tz = t % MF_TZ, ty = t / MF_TZ;
    const int64_t plane_elems = (int64_t)Y * Z;
    unsigned bad = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int zt = (int)(tile % nzt);
        const int64_t rest = tile / nzt;
        const int yt = (int)(rest % nyt), xc = (int)(rest / nyt);
        const int z0 = zt * MF_TZ, xs = xc * MF_XC, xe = xs + MF_XC < X ? xs + MF_XC : X;
        const int64_t y0 = (int64_t)yt * MF_TY;
        // what this thread stages of every plane: elements t, t + 256, ... of the PH x PW halo plane, at clamped indices -- always valid,
        // also for the surplus threads past the plane's end, so that neither the loads nor the LDS stores sit behind a per-lane branch
        // (a branch there makes the compiler wait for every load in flight instead of the oldest plane's)
        int64_t off[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const int e = t + 256 * l;
            int64_t gy = y0 - HY + e / PW;
            int gz = z0 - HZ + e % PW;
            gy = gy < 0 ? 0 : (gy > Y - 1 ? Y - 1 : gy);
            gz = gz < 0 ? 0 : (gz > Z - 1 ? Z - 1 : gz);
            off[l] = gy * Z + gz;
        }
        const bool active = y0 + ty < Y && z0 + tz < Z;
        const int64_t oidx = (y0 + ty) * Z + z0 + tz;
        T pf[MF_DEPTH][NL];
        float w[M];
#pragma unroll
        for (int i = 0; i < M; ++i) w[i] = 0.f;
        const int np = xe - xs + 2 * HX;
        // plane sp of the tile (x = xs - HX + sp, clamped) into one register set, as loaded: the conversion waits until the set is stored
        auto fetch = [&](int sp, T (&r)[NL]) {
            int gx = xs - HX + sp;
            gx = gx < 0 ? 0 : (gx > X - 1 ? X - 1 : gx);
            const T* base = vol + (int64_t)gx * plane_elems;
#pragma unroll
            for (int l = 0; l < NL; ++l) r[l] = base[off[l]];
        };
        auto step = [&](int s, T (&r)[NL]) {
            float* buf = plane[s & 1];
#pragma unroll
            for (int l = 0; l < NL; ++l) buf[t + 256 * l] = (float)r[l];
            if (s + MF_DEPTH < np) fetch(s + MF_DEPTH, r);          // the set is free again: MF_DEPTH planes stay in flight
            __syncthreads();
            float nw[P];
#pragma unroll
            for (int dy = 0; dy < SY; ++dy)
#pragma unroll
                for (int dz = 0; dz < SZ; ++dz) nw[dy * SZ + dz] = buf[(ty + dy) * PW + tz + dz];
            if constexpr (sizeof(T) == 4)                           // the voxel itself, counted once: in the planes this tile writes
                if (active && s >= HX && s < np - HX) bad += vol_nonfinite(nw[HY * SZ + HZ]);
            mf_prep<SX, P>(nw);
#pragma unroll
            for (int i = 0; i < M - P; ++i) w[i] = w[i + P];
#pragma unroll
            for (int i = 0; i < P; ++i) w[M - P + i] = nw[i];
            if (s >= 2 * HX && active) out[(int64_t)(xs + s - 2 * HX) * plane_elems + oidx] = mf_median<SX, P>(w);
        };
#pragma unroll
        for (int d = 0; d < MF_DEPTH; ++d) if (d < np) fetch(d, pf[d]);
        for (int s0 = 0; s0 < np; s0 += MF_DEPTH) {
#pragma unroll
            for (int d = 0; d < MF_DEPTH; ++d) if (s0 + d < np) step(s0 + d, pf[d]);       // uniform
        }
        __syncthreads();                                            // the next tile's first plane goes into a buffer still being read
    }
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
        if ((t & 63) == 0) wbad[t >> 6] = bad;
        __syncthreads();
        if (t == 0) {
            const unsigned tot = wbad[0] + wbad[1] + wbad[2] + wbad[3];
            if (tot) atomicAdd(nonfinite, tot);                     // result unused: a non-returning atomic
        }
    }
}

template <typename T, int SX, int SY, int SZ>
static void median3_launch(const void* vol, int X, int Y, int Z, float* out, uint32_t* nonfinite, hipStream_t s) {
    const int nzt = (Z + MF_TZ - 1) / MF_TZ, nyt = (int)(((int64_t)Y + MF_TY - 1) / MF_TY), nxc = (int)(((int64_t)X + MF_XC - 1) / MF_XC);
    const int64_t ntiles = (int64_t)nzt * nyt * nxc;
    const unsigned grid = (unsigned)(ntiles < (1 << 20) ? ntiles : (1 << 20));
    hipLaunchKernelGGL((median3_kernel<T, SX, SY, SZ>), dim3(grid), dim3(256), 0, s, (const T*)vol, X, Y, Z, nyt, nzt, ntiles, out, nonfinite);
}

template <typename T>
static void median3_dispatch(const T* vol, int X, int Y, int Z, int sx, int sy, int sz, float* out, uint32_t* nonfinite, hipStream_t s) {
    switch ((sx == 3 ? 4 : 0) | (sy == 3 ? 2 : 0) | (sz == 3 ? 1 : 0)) {
    case 0: median3_launch<T, 1, 1, 1>(vol, X, Y, Z, out, nonfinite, s); break;
    case 1: median3_launch<T, 1, 1, 3>(vol, X, Y, Z, out, nonfinite, s); break;
    case 2: median3_launch<T, 1, 3, 1>(vol, X, Y, Z, out, nonfinite, s); break;
    case 3: median3_launch<T, 1, 3, 3>(vol, X, Y, Z, out, nonfinite, s); break;
    case 4: median3_launch<T, 3, 1, 1>(vol, X, Y, Z, out, nonfinite, s); break;
    case 5: median3_launch<T, 3, 1, 3>(vol, X, Y, Z, out, nonfinite, s); break;
    case 6: median3_launch<T, 3, 3, 1>(vol, X, Y, Z, out, nonfinite, s); break;
    default: median3_launch<T, 3, 3, 3>(vol, X, Y, Z, out, nonfinite, s); break;
    }
}

extern "C" int vg_median3(const void* vol, int dtype, int X, int Y, int Z, int sx, int sy, int sz, float* out, uint32_t* nonfinite,
                          vg_stream_t stream) {
    vg_begin();
    if (!vol || !out || !nonfinite || !vol_dtype_ok(dtype) || X < 1 || Y < 1 || Z < 1 || Z > (1 << 20)) return VG_EINVAL;
    if ((int64_t)X * Y >= ((int64_t)1 << 40)) return VG_EINVAL;
    if ((sx != 1 && sx != 3) || (sy != 1 && sy != 3) || (sz != 1 && sz != 3)) return VG_EINVAL;
    const int64_t n = (int64_t)X * Y * Z;
    const uintptr_t v0 = (uintptr_t)vol, o0 = (uintptr_t)out;
    if (v0 % vol_esz(dtype) != 0 || o0 % 4 != 0 || (uintptr_t)nonfinite % 4 != 0) return VG_EINVAL;
    if (v0 < o0 + (uintptr_t)n * 4 && o0 < v0 + (uintptr_t)n * vol_esz(dtype)) return VG_EINVAL;        // out overlaps vol
    hipStream_t s = (hipStream_t)stream;
    vol_dispatch(vol, dtype, [&](auto* v) { median3_dispatch(v, X, Y, Z, sx, sy, sz, out, nonfinite, s); });
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ outlier limits
// While the scan runs, stats4[0] and stats4[2] hold the smallest and the largest key met (vol_key: unsigned order == float order), as
// integers; the last kernel turns them into values.
__global__ void outlier_init_kernel(unsigned* __restrict__ keys, unsigned* __restrict__ kn2) {
    keys[0] = 0xffffffffu; keys[1] = 0xffffffffu; keys[2] = 0u; keys[3] = 0u;
    kn2[0] = 0u;
}

struct mf_keep { unsigned kmin, kmax, bad; unsigned long long kept; };

// kept: |(x - m) / s| <= threshold in fp32, every operation rounded and the division correctly rounded (HIP's default, which the build's
// flags leave alone; nothing can contract).  A NaN compares false, so neither a NaN voxel nor any voxel under s == 0 or a non-finite s is kept.
__device__ __forceinline__ void mf_keep1(float x, float m, float s, float thr, mf_keep& k) {
    const float z = __builtin_fabsf((x - m) / s);
    if (z <= thr) {
        const unsigned key = vol_key(x);
        k.kmin = key < k.kmin ? key : k.kmin;
        k.kmax = key > k.kmax ? key : k.kmax;
        ++k.kept;
    }
    k.bad += vol_nonfinite(x);
}

template <typename T>
__global__ __launch_bounds__(256) void outlier_scan_kernel(const T* __restrict__ vol, int64_t n, int vec, const float* __restrict__ mean_std,
                                                           float thr, unsigned* keys, unsigned* kn2) {
    __shared__ unsigned wmin[4], wmax[4], wbad[4];
    __shared__ unsigned long long wkept[4];
    const float m = mean_std[0], s = mean_std[1];
    const int t = threadIdx.x;
    const int64_t tid = (int64_t)blockIdx.x * 256 + t, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = vec ? n / 4 : 0;
    mf_keep k = {0xffffffffu, 0u, 0u, 0ull};
    for (int64_t i = tid; i < nv; i += nthr) {
        const vol_pack<T, 4> p = *(const vol_pack<T, 4>*)(vol + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) mf_keep1((float)p.v[j], m, s, thr, k);
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) mf_keep1((float)vol[e], m, s, thr, k);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = __shfl_xor(k.kmin, o), b = __shfl_xor(k.kmax, o);
        k.kmin = a < k.kmin ? a : k.kmin;
        k.kmax = b > k.kmax ? b : k.kmax;
        k.bad += __shfl_xor(k.bad, o);
        k.kept += __shfl_xor(k.kept, o);
    }
    if ((t & 63) == 0) { wmin[t >> 6] = k.kmin; wmax[t >> 6] = k.kmax; wbad[t >> 6] = k.bad; wkept[t >> 6] = k.kept; }
    __syncthreads();
    if (t == 0) {
        unsigned kmin = wmin[0], kmax = wmax[0], bad = wbad[0];
        unsigned long long kept = wkept[0];
        for (int w = 1; w < 4; ++w) {
            kmin = wmin[w] < kmin ? wmin[w] : kmin;
            kmax = wmax[w] > kmax ? wmax[w] : kmax;
            bad += wbad[w]; kept += wkept[w];
        }
        if (kept) {
            atomicMin(&keys[0], kmin);
            atomicMax(&keys[2], kmax);
            const unsigned add = kept > 0xffffffffull ? 0xffffffffu : (unsigned)kept;
            // A saturating add without a retry loop: whoever makes the word wrap sees it (old + add < old) and raises the word to its
            // largest value afterwards.  Any add that follows that maximum wraps again and is followed by its own maximum, so the last
            // operation on a word that ever wrapped is a maximum; a word that never wrapped holds the plain sum.
            const unsigned old = atomicAdd(&kn2[0], add);
            if (old + add < old) atomicMax(&kn2[0], 0xffffffffu);
        }
        if (bad) atomicAdd(&kn2[1], bad);
    }
}

__global__ void outlier_finish_kernel(float* __restrict__ stats4, const unsigned* __restrict__ kn2) {
    const unsigned* keys = (const unsigned*)stats4;
    const unsigned k0 = keys[0], k2 = keys[2];
    const bool any = kn2[0] != 0u;
    const float lo = any ? vol_unkey(k0) : __builtin_inff(), hi = any ? vol_unkey(k2) : -__builtin_inff();
    stats4[0] = lo; stats4[1] = lo; stats4[2] = hi; stats4[3] = hi;
}

extern "C" int vg_outlier_limits(const void* vol, int dtype, int64_t n, const float* mean_std, float threshold, float* stats4,
                                 uint32_t* kept_nonfinite2, vg_stream_t stream) {
    vg_begin();
    if (!vol || !mean_std || !stats4 || !kept_nonfinite2 || !vol_n_ok(n) || !vol_dtype_ok(dtype)) return VG_EINVAL;
    if (!(threshold > 0.f) || !(threshold < __builtin_inff())) return VG_EINVAL;
    const int esz = vol_esz(dtype);
    if ((uintptr_t)vol % esz != 0 || (uintptr_t)mean_std % 4 != 0 || (uintptr_t)stats4 % 4 != 0 || (uintptr_t)kept_nonfinite2 % 4 != 0) return VG_EINVAL;
    const int vec = (uintptr_t)vol % (4 * esz) == 0;
    hipStream_t s = (hipStream_t)stream;
    unsigned* keys = (unsigned*)stats4;
    hipLaunchKernelGGL(outlier_init_kernel, dim3(1), dim3(1), 0, s, keys, kept_nonfinite2);
    vol_dispatch(vol, dtype, [&](auto* v) {
        hipLaunchKernelGGL(outlier_scan_kernel<vol_elem_t<decltype(v)>>, vol_grid(n, vec), dim3(256), 0, s, v, n, vec, mean_std, threshold, keys,
                           kept_nonfinite2);
    });
    hipLaunchKernelGGL(outlier_finish_kernel, dim3(1), dim3(1), 0, s, stats4, kept_nonfinite2);
    return vg_check_launch();
}
