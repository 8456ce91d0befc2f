// vg_edt.hip -- measuring a vessel mask (van_gan_amd/postprocess.py; include/vangan_hip.h "Prediction post-processing"):
// the exact 3-D Euclidean distance transform of a uint8 mask, and the two kernels that turn the labels of the inverted mask into a
// hole-filled mask.  Nothing here depends on the 16-bit storage format of the build.  256-thread workgroups (4 wave64) on a
// one-dimensional grid.  No atomics, no LDS shared between waves, no workgroup barrier: every loop is bounded by an axis length.
//
// The transform is the separable one: the squared distance along Z, then min over p' of (f(p') + w (p - p')^2) along Y and along X.  The
// cost type T is int32 (voxel units, w = 1, the sentinel INF = 2^31 - 1 for "no background yet") or fp64 (w = sampling^2 per axis, the
// sentinel +inf).  X^2 + Y^2 + Z^2 < 2^31 (checked by the entries), so no finite int32 cost plus a step overflows.
#include "vg_volume.h"

#define EDT_MAXC 728                       // 64-voxel pieces of a row: Z^2 < 2^31 gives Z <= 46340, 725 pieces
#define EDT_ROWS 4                         // rows per workgroup of the Z pass: one per wave
#define EDT_KEEP 0                         // the axis pass hands T to the next pass
#define EDT_OUT_SQ 1                       // ... writes VG_EDT_SQUARED_I32
#define EDT_OUT_DIST 2                     // ... writes VG_EDT_DIST_F32

template <typename T> __device__ __forceinline__ T edt_inf();
template <> __device__ __forceinline__ int edt_inf<int>() { return 0x7fffffff; }
template <> __device__ __forceinline__ double edt_inf<double>() { return __builtin_huge_val(); }
// the cost of a step of d voxels along an axis of weight w; d^2 < 2^31 is exact in both types
template <typename T> __device__ __forceinline__ T edt_step(int d, double w);
template <> __device__ __forceinline__ int edt_step<int>(int d, double) { return d * d; }
template <> __device__ __forceinline__ double edt_step<double>(int d, double w) { return w * (double)(d * d); }

static inline int64_t edt_al16(int64_t b) { return (b + 15) & ~(int64_t)15; }
// n = X * Y * Z where the shape is served (1 <= n < 2^31 and X^2 + Y^2 + Z^2 < 2^31), else 0
static inline int64_t edt_voxels(int X, int Y, int Z) {
    if (X < 1 || Y < 1 || Z < 1) return 0;
    if ((int64_t)X * X + (int64_t)Y * Y + (int64_t)Z * Z >= ((int64_t)1 << 31)) return 0;       // every axis is below 2^15.5 from here on
    const int64_t n = (int64_t)X * Y * Z;
    return n < ((int64_t)1 << 31) ? n : 0;
}

static inline unsigned edt_z_lds_bytes(int Z) { return (unsigned)(EDT_ROWS * ((Z + 63) / 64) * 12); }      // at most 34 944: EDT_MAXC pieces

// ------------------------------------------------------------------------------------------------ pass Z: one wave per row
// The row is cut into pieces of 64 voxels, lane = z % 64, so every access is coalesced.  First loop: the ballot of "background" of
// every piece, kept in the wave's own slice of LDS.  Second loop (every lane the same scalar work): for every piece the first
// background voxel to its right.  Third loop: the nearest background at or left of z is the highest set bit at or below the lane, else
// the last one seen in an earlier piece; the nearest at or right of z is the lowest set bit at or above the lane, else the second
// loop's.  A wave only reads the LDS words it wrote itself, in program order: no barrier.  The LDS is sized by the launch for the row
// length (12 bytes per piece and row: 144 bytes at Z = 140), so that it does not cap the occupancy.
template <typename T>
__global__ __launch_bounds__(256) void edt_z_kernel(const uint8_t* __restrict__ mask, int64_t rows, int Z, double w, T* __restrict__ f) {
#pragma clang fp contract(off)
    extern __shared__ unsigned long long edt_lds[];                 // EDT_ROWS * nc ballots, then as many ints: edt_z_lds_bytes(Z)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * EDT_ROWS + wv;
    if (row >= rows) return;                                        // the whole wave leaves
    const uint8_t* m = mask + row * Z;
    T* o = f + row * Z;
    const int nc = (Z + 63) >> 6;                                   // <= EDT_MAXC: the entry checked Z
    unsigned long long* bal = edt_lds + wv * nc;                    // this wave's slices
    int* right = (int*)(edt_lds + EDT_ROWS * nc) + wv * nc;
    for (int c = 0; c < nc; ++c) {
        const int z = c * 64 + lane;
        bal[c] = __builtin_amdgcn_ballot_w64(z < Z && m[z] == 0);
    }
    __builtin_amdgcn_wave_barrier();
    int r = -1;
    for (int c = nc - 1; c >= 0; --c) {
        right[c] = r;
        const unsigned long long b = bal[c];
        if (b) r = c * 64 + __builtin_ctzll(b);
    }
    __builtin_amdgcn_wave_barrier();
    int l = -1;
    for (int c = 0; c < nc; ++c) {
        const unsigned long long b = bal[c];
        const int z = c * 64 + lane;
        const unsigned long long le = b & (~0ull >> (63 - lane)), ge = b >> lane;
        const int pl = le ? c * 64 + 63 - __builtin_clzll(le) : l;
        const int pr = ge ? z + __builtin_ctzll(ge) : right[c];
        T best = edt_inf<T>();
        if (pl >= 0) best = edt_step<T>(z - pl, w);
        if (pr >= 0) { const T d = edt_step<T>(pr - z, w); best = d < best ? d : best; }
        if (z < Z) o[z] = best;
        if (b) l = c * 64 + 63 - __builtin_clzll(b);
    }
}

// ------------------------------------------------------------------------------------------------ passes Y and X: one thread per voxel
// Consecutive threads are consecutive z, so the loads at distance d along the axis (stride voxels apart) are coalesced.  A voxel looks
// at p - 1, p + 1, p - 2, ... and stops at the first d with w d^2 >= best: every candidate from there on is f + w d^2 >= best.  Exact,
// no stack of parabolas, and the work is proportional to the distance found; at most L - 1 steps.
template <typename T, int OUT>
__global__ __launch_bounds__(256) void edt_axis_kernel(const T* __restrict__ in, unsigned n, int L, unsigned stride, double w, void* __restrict__ out) {
#pragma clang fp contract(off)             // f + w d^2 is rounded as the restatement rounds it: a product, then a sum
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= (int64_t)n) return;
    const int p = (int)(((unsigned)v / stride) % (unsigned)L);
    const T inf = edt_inf<T>();
    T best = in[v];
    for (int d = 1; d < L; ++d) {
        const T dd = edt_step<T>(d, w);
        if (dd >= best) break;
        const bool lo = p - d >= 0, hi = p + d < L;
        if (!lo && !hi) break;
        const T a = lo ? in[v - (int64_t)d * stride] : inf;         // both loads before either is used
        const T b = hi ? in[v + (int64_t)d * stride] : inf;
        if (a != inf) { const T c = a + dd; best = c < best ? c : best; }
        if (b != inf) { const T c = b + dd; best = c < best ? c : best; }
    }
    if constexpr (OUT == EDT_KEEP) ((T*)out)[v] = best;
    else if constexpr (OUT == EDT_OUT_SQ) ((int*)out)[v] = (int)best;
    else ((float*)out)[v] = best == inf ? __builtin_huge_valf() : (float)sqrt((double)best);       // fp64 sqrt, then one rounding to fp32
}

extern "C" int64_t vg_edt_scratch_bytes(int X, int Y, int Z, int weighted) {
    const int64_t n = edt_voxels(X, Y, Z);
    if (!n || (weighted != 0 && weighted != 1)) return VG_EINVAL;
    return 2 * edt_al16(n * (weighted ? 8 : 4));
}

template <typename T>
static void edt_launch(const uint8_t* mask, int X, int Y, int Z, const double* w3, void* out, int out_kind, void* scratch, hipStream_t s) {
    const int64_t n = (int64_t)X * Y * Z, rows = (int64_t)X * Y;
    T* a = (T*)scratch;
    T* b = (T*)((char*)scratch + edt_al16(n * (int64_t)sizeof(T)));
    const dim3 block(256), flat((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(edt_z_kernel<T>, dim3((unsigned)((rows + EDT_ROWS - 1) / EDT_ROWS)), block, edt_z_lds_bytes(Z), s, mask, rows, Z, w3[2], a);
    hipLaunchKernelGGL((edt_axis_kernel<T, EDT_KEEP>), flat, block, 0, s, (const T*)a, (unsigned)n, Y, (unsigned)Z, w3[1], (void*)b);
    const unsigned sx = (unsigned)((int64_t)Y * Z);
    if (out_kind == VG_EDT_DIST_F32)
        hipLaunchKernelGGL((edt_axis_kernel<T, EDT_OUT_DIST>), flat, block, 0, s, (const T*)b, (unsigned)n, X, sx, w3[0], out);
    else if constexpr (sizeof(T) == 4)
        hipLaunchKernelGGL((edt_axis_kernel<T, EDT_OUT_SQ>), flat, block, 0, s, (const T*)b, (unsigned)n, X, sx, w3[0], out);
}

extern "C" int vg_edt(const uint8_t* mask, int X, int Y, int Z, const double* sampling3_or_null, void* out, int out_kind, void* scratch,
                      int64_t scratch_bytes, vg_stream_t stream) {
    vg_begin();
    if (!mask || !out || !scratch || !edt_voxels(X, Y, Z)) return VG_EINVAL;
    if (out_kind != VG_EDT_SQUARED_I32 && out_kind != VG_EDT_DIST_F32) return VG_EINVAL;
    if (sampling3_or_null && out_kind == VG_EDT_SQUARED_I32) return VG_EINVAL;     // the squared distances are the integer form's
    const int weighted = sampling3_or_null ? 1 : 0;
    if ((uintptr_t)out % 4 != 0 || (uintptr_t)scratch % 16 != 0 || scratch_bytes < vg_edt_scratch_bytes(X, Y, Z, weighted)) return VG_EINVAL;
    double w3[3] = {1.0, 1.0, 1.0};
    for (int a = 0; weighted && a < 3; ++a) {
        const double sa = sampling3_or_null[a];
        if (!(sa > 0.0) || sa > 1.7976931348623157e308) return VG_EINVAL;         // a NaN, a non-positive or an infinite spacing
        w3[a] = sa * sa;
    }
    hipStream_t s = (hipStream_t)stream;
    if (weighted) edt_launch<double>(mask, X, Y, Z, w3, out, out_kind, scratch, s);
    else edt_launch<int>(mask, X, Y, Z, w3, out, out_kind, scratch, s);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ hole filling
// labels: vg_cc_label of the INVERTED mask at connectivity 1, so a label >= 1 is a component of the background.  A hole is one that
// reaches none of the six faces.  Marking: a thread per face voxel (edges and corners come more than once) stores 1 at its label -- plain
// byte stores of one value, so their order does not matter.  A label outside [1, cap) is never used as an index.
__global__ __launch_bounds__(256) void fh_mark_kernel(const int* __restrict__ labels, int X, int Y, int Z, int64_t cap, uint8_t* flags) {
    const int64_t yz = (int64_t)Y * Z, xz = (int64_t)X * Z, xy = (int64_t)X * Y;
    int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int x, y, z;
    if (t < 2 * yz) { x = t < yz ? 0 : X - 1; t %= yz; y = (int)(t / Z); z = (int)(t % Z); }
    else if ((t -= 2 * yz) < 2 * xz) { y = t < xz ? 0 : Y - 1; t %= xz; x = (int)(t / Z); z = (int)(t % Z); }
    else if ((t -= 2 * xz) < 2 * xy) { z = t < xy ? 0 : Z - 1; t %= xy; x = (int)(t / Y); y = (int)(t % Y); }
    else return;
    const int l = labels[((int64_t)x * Y + y) * Z + z];
    if (l >= 1 && l < cap) flags[l] = 1;
}

template <int V>
__global__ __launch_bounds__(256) void fh_apply_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, const uint8_t* __restrict__ flags,
                                                       int64_t n, int64_t cap, uint8_t* __restrict__ out) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = V == 4 ? n / 4 : 0;
    for (int64_t i = tid; i < nv; i += nthr) {
        const int4 l = *(const int4*)(labels + i * 4);
        const unsigned mw = *(const unsigned*)(mask + i * 4);
        const int lj[4] = {l.x, l.y, l.z, l.w};
        unsigned word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned fg = ((mw >> (8 * j)) & 0xffu) != 0u;
            const unsigned hole = !fg && lj[j] >= 1 && lj[j] < cap && !flags[lj[j]];
            word |= (fg | hole) << (8 * j);
        }
        *(unsigned*)(out + i * 4) = word;
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) {
        const int l = labels[e];
        out[e] = (uint8_t)(mask[e] != 0 || (l >= 1 && l < cap && !flags[l]));
    }
}

static inline int64_t fh_cap(int64_t n) { return n / 2 + 2; }      // the words of vg_cc_label's sizes: no label reaches it

extern "C" int vg_fill_holes_mark(const int32_t* labels, int X, int Y, int Z, uint8_t* flags, vg_stream_t stream) {
    vg_begin();
    if (!labels || !flags || X < 1 || Y < 1 || Z < 1 || (uintptr_t)labels % 4 != 0) return VG_EINVAL;
    if ((int64_t)X * Y >= ((int64_t)1 << 31)) return VG_EINVAL;             // so that the product below cannot overflow
    const int64_t n = (int64_t)X * Y * Z;
    if (n >= ((int64_t)1 << 31)) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(flags, 0, (size_t)fh_cap(n), s) != hipSuccess) return VG_ELAUNCH;
    const int64_t faces = 2 * ((int64_t)Y * Z + (int64_t)X * Z + (int64_t)X * Y);                // each product is below 2^31
    hipLaunchKernelGGL(fh_mark_kernel, dim3((unsigned)((faces + 255) / 256)), dim3(256), 0, s, labels, X, Y, Z, fh_cap(n), flags);
    return vg_check_launch();
}

extern "C" int vg_fill_holes_apply(const uint8_t* mask, const int32_t* labels, const uint8_t* flags, int64_t n, uint8_t* out, vg_stream_t stream) {
    vg_begin();
    if (!mask || !labels || !flags || !out || n < 1 || n >= ((int64_t)1 << 31) || (uintptr_t)labels % 4 != 0) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int vec = (uintptr_t)labels % 16 == 0 && (uintptr_t)mask % 4 == 0 && (uintptr_t)out % 4 == 0;
    if (vec) hipLaunchKernelGGL(fh_apply_kernel<4>, vol_grid(n, 1), dim3(256), 0, s, mask, labels, flags, n, fh_cap(n), out);
    else hipLaunchKernelGGL(fh_apply_kernel<1>, vol_grid(n, 0), dim3(256), 0, s, mask, labels, flags, n, fh_cap(n), out);
    return vg_check_launch();
}
