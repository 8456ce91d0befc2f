// vg_resample.hip -- one separable pass of the Lanczos-4 volume resize (van_gan_amd/preprocess.py resize_volume; include/vangan_hip.h
// "Volume resize"): out[o][j][i] = sum_k w8[j][k] * x[o][clamp(first[j] + k, 0, L - 1)][i] over a volume seen as
// [outer][L][inner] -> [outer][T][inner], fp32 in both storage builds.  The 8-tap table (first, w8) is built on the host; the clamp (the
// replicated edge) is applied here, so no table content can make a read leave the row.  acc = w_0 * x_0, then fmaf in tap order: a fixed
// association and no atomics, so equal inputs give equal bits.  Two access patterns, two kernels:
//   inner >= 2  the resized axis is strided; neighbouring lanes take neighbouring i and a lane's 8 taps lie `inner` floats apart.
//   inner == 1  the resized axis is the contiguous one (the Z pass); whole rows are staged in LDS.
// Both passes move 4 bytes per 8 FMAs: they are bound by memory (times: DESIGN.md 3.13).
#include "vg_common.h"

#define RS_TAPS 8
#define RS_MAX_LEN (1 << 20)
#define RS_MAX_BLOCKS 32768                 // a multiple of 8 (the XCD count)

__device__ __forceinline__ int rs_clamp(int r, int L) { return r < 0 ? 0 : (r >= L ? L - 1 : r); }

// ------------------------------------------------------------------------------------------------ inner >= 2
// A workgroup serves ONE output index j -- its table row is uniform, nine scalar loads -- for RB neighbouring o and IC * V neighbouring i:
// thread t is column t % IC (V consecutive i: one 16-byte access when V == 4) of sub-volume t / IC, so a workgroup whose inner extent is
// short (Z = 140: 35 vectors) still fills its lanes with rows of other o.  Work items are (j fastest, i chunk, o block): items that are
// neighbours in j read source rows that overlap in 7 of 8 taps.  Workgroups go round-robin to the 8 XCDs, each with an L2 of its own, so
// workgroup b of a sweep of G takes item (b % 8) * (G / 8) + b / 8: every XCD then walks a contiguous run of items and finds the shared
// rows in its own L2.
template <int V>
__global__ __launch_bounds__(256) void resample_strided_kernel(const float* __restrict__ x, int64_t outer, int L, int64_t inner, int T,
                                                               const int32_t* __restrict__ first, const float* __restrict__ w8,
                                                               float* __restrict__ out, int IC, int RB, int64_t nchunk, int64_t items) {
    const int t = threadIdx.x, il = t % IC, ol = t / IC;
    const int64_t G = gridDim.x, per = G >> 3;
    for (int64_t base = 0; base < items; base += G) {
        const int64_t item = base + (int64_t)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if (item >= items) continue;                                // uniform
        const int j = (int)(item % T);
        const int64_t rest = item / T, c = rest % nchunk, ob = rest / nchunk;
        const int64_t i = (c * IC + il) * V, o = ob * RB + ol;
        if (ol >= RB || i >= inner || o >= outer) continue;
        const int f = first[j];
        const float* w = w8 + (size_t)j * RS_TAPS;
        const float* src = x + (size_t)o * L * inner + i;
        float* dst = out + ((size_t)o * T + j) * inner + i;
        if (V == 4) {
            f32x4 acc = w[0] * *(const f32x4*)(src + (size_t)rs_clamp(f, L) * inner);
#pragma unroll
            for (int k = 1; k < RS_TAPS; ++k) {
                const f32x4 v = *(const f32x4*)(src + (size_t)rs_clamp(f + k, L) * inner);
                const float wk = w[k];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = fmaf(wk, v[e], acc[e]);
            }
            *(f32x4*)dst = acc;
        } else {
            float acc = w[0] * src[(size_t)rs_clamp(f, L) * inner];
#pragma unroll
            for (int k = 1; k < RS_TAPS; ++k) acc = fmaf(w[k], src[(size_t)rs_clamp(f + k, L) * inner], acc);
            *dst = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ inner == 1, rows in LDS
// The volume is `outer` contiguous rows of L floats.  A workgroup stages R whole rows -- R * L contiguous floats, read with 16-byte loads
// when the tile starts on a 16-byte boundary (R is a multiple of 4, so it does whenever x does), else one float per lane -- into LDS at a
// row pitch of L | 1 floats: an odd pitch, so the rows start on different banks.  Thread t then owns output j = t % TC (+ 256 per chunk
// when T > 256) and walks the rows t / TC, t / TC + RB, ...: its table row stays in nine registers for as long as j does not change, the
// 8 taps are LDS reads at nearly consecutive addresses across a wave, and a wave's stores are consecutive j of one row.
#define RS_LDS_FLOATS 4096                  // 16 KiB: 8 workgroups per CU are limited by their waves, not by LDS
#define RS_MAX_ROWS 64
__global__ __launch_bounds__(256) void resample_rows_kernel(const float* __restrict__ x, int64_t outer, int L, int T,
                                                            const int32_t* __restrict__ first, const float* __restrict__ w8,
                                                            float* __restrict__ out, int R, int pitch, int TC, int RB, int vec) {
    __shared__ float tile[RS_LDS_FLOATS];
    const int t = threadIdx.x, jl = t % TC, rsub = t / TC;
    const int64_t ntiles = (outer + R - 1) / R;
    int jcur = -1, f = 0;
    float w[RS_TAPS];
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int64_t r0 = tl * R;
        const int rows = (int)(outer - r0 < R ? outer - r0 : R), n = rows * L;       // n <= R * L < RS_LDS_FLOATS
        const float* src = x + (size_t)r0 * L;
        const int nv = vec ? n / 4 : 0;
        for (int v = t; v < nv; v += 256) {
            const f32x4 p = *(const f32x4*)(src + 4 * v);
            int row = (4 * v) / L, col = 4 * v - row * L;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                tile[row * pitch + col] = p[e];
                if (++col == L) { col = 0; ++row; }
            }
        }
        for (int e = nv * 4 + t; e < n; e += 256) { const int row = e / L; tile[row * pitch + (e - row * L)] = src[e]; }
        __syncthreads();
        if (rsub < RB)
            for (int j = jl; j < T; j += TC) {
                if (j != jcur) {
                    f = first[j];
#pragma unroll
                    for (int k = 0; k < RS_TAPS; ++k) w[k] = w8[(size_t)j * RS_TAPS + k];
                    jcur = j;
                }
                int idx[RS_TAPS];
#pragma unroll
                for (int k = 0; k < RS_TAPS; ++k) idx[k] = rs_clamp(f + k, L);
                for (int r = rsub; r < rows; r += RB) {
                    const float* row = tile + r * pitch;
                    float acc = w[0] * row[idx[0]];
#pragma unroll
                    for (int k = 1; k < RS_TAPS; ++k) acc = fmaf(w[k], row[idx[k]], acc);
                    out[(size_t)(r0 + r) * T + j] = acc;
                }
            }
        __syncthreads();
    }
}

// inner == 1 and a row too long for the tile (L | 1 > RS_LDS_FLOATS / 4): one output per lane straight from global memory; neighbouring
// lanes take neighbouring j, whose taps are neighbouring addresses.
__global__ __launch_bounds__(256) void resample_rows_direct_kernel(const float* __restrict__ x, int64_t outer, int L, int T,
                                                                   const int32_t* __restrict__ first, const float* __restrict__ w8,
                                                                   float* __restrict__ out) {
    const int64_t n = outer * T, nthr = (int64_t)gridDim.x * 256;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += nthr) {
        const int64_t o = e / T;
        const int j = (int)(e - o * T), f = first[j];
        const float* row = x + (size_t)o * L;
        const float* w = w8 + (size_t)j * RS_TAPS;
        float acc = w[0] * row[rs_clamp(f, L)];
#pragma unroll
        for (int k = 1; k < RS_TAPS; ++k) acc = fmaf(w[k], row[rs_clamp(f + k, L)], acc);
        out[e] = acc;
    }
}

extern "C" int vg_resample_axis(const float* x, int64_t outer, int L, int64_t inner, int T, const int32_t* first, const float* w8, float* out,
                                vg_stream_t stream) {
    vg_begin();
    if (!x || !first || !w8 || !out || out == x) return VG_EINVAL;
    if (outer < 1 || inner < 1 || L < 1 || T < 1 || L > RS_MAX_LEN || T > RS_MAX_LEN) return VG_EINVAL;
    const int64_t lim = (int64_t)1 << 40, mx = L > T ? L : T;
    if (outer >= lim || inner >= lim || outer * mx >= lim || outer * mx > (lim - 1) / inner) return VG_EINVAL;      // outer * mx * inner >= 2^40
    if ((uintptr_t)x % 4 != 0 || (uintptr_t)out % 4 != 0 || (uintptr_t)first % 4 != 0 || (uintptr_t)w8 % 4 != 0) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool al16 = (uintptr_t)x % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (inner == 1) {
        const int pitch = L | 1;
        int R = (RS_LDS_FLOATS / pitch) & ~3;
        if (R > RS_MAX_ROWS) R = RS_MAX_ROWS;
        if (R >= 4) {
            const int TC = T < 256 ? T : 256, RB = 256 / TC;
            const int64_t ntiles = cdiv64(outer, R);
            hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)(ntiles < RS_MAX_BLOCKS ? ntiles : RS_MAX_BLOCKS)), dim3(256), 0, s, x, outer, L,
                               T, first, w8, out, R, pitch, TC, RB, (uintptr_t)x % 16 == 0 ? 1 : 0);
        } else {
            const int64_t nb = cdiv64(outer * T, 256);
            hipLaunchKernelGGL(resample_rows_direct_kernel, dim3((unsigned)(nb < RS_MAX_BLOCKS ? nb : RS_MAX_BLOCKS)), dim3(256), 0, s, x, outer, L, T,
                               first, w8, out);
        }
        return vg_check_launch();
    }
    const int V = inner % 4 == 0 && al16 ? 4 : 1;
    const int64_t ncol = inner / V;                                 // V == 4 only where it divides inner
    const int IC = (int)(ncol < 256 ? ncol : 256), RB = 256 / IC;
    const int64_t nchunk = cdiv64(ncol, IC), items = (int64_t)T * nchunk * cdiv64(outer, RB);
    int64_t G = (items + 7) & ~(int64_t)7;
    if (G > RS_MAX_BLOCKS) G = RS_MAX_BLOCKS;
    if (V == 4) hipLaunchKernelGGL(resample_strided_kernel<4>, dim3((unsigned)G), dim3(256), 0, s, x, outer, L, inner, T, first, w8, out, IC, RB, nchunk, items);
    else hipLaunchKernelGGL(resample_strided_kernel<1>, dim3((unsigned)G), dim3(256), 0, s, x, outer, L, inner, T, first, w8, out, IC, RB, nchunk, items);
    return vg_check_launch();
}
