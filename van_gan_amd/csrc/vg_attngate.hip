// vg_attngate.hip -- the attention gate of the ResUNet decoder (ResUNet(use_attention_gate=True), resunet_model.py:178-179 with
// vnet_model.py:24-77; Oktay et al., Attention U-Net), restated:
//   theta = skip . W_theta + b_theta        skip [N][D][H][W][Cs], W_theta [Cs][Ci] (Keras [1,1,1,Cs,Ci])
//   q     = relu(theta + phi(parent))       phi  [N][D/2][H/2][W/2][Ci]: the 1x1x1 convolution of the LOW-resolution tensor (it
//                                           commutes with UpSampling3D(2)), bias included, read through the parent index
//   h     = sigmoid(q . w_psi + b_psi)      one value per voxel, kept as fp32 for the backward
//   gated = skip * h
//
// Everything lives in the accumulator layout of the 16x16 MFMA: lane l = (v = l & 15, g = l >> 4) owns voxel v of the wave's
// 16-voxel tile and, of every 16-channel chunk t, the channels 16 t + 4 g + {0..3}.  That is at once
//   * the C/D layout of a product whose columns are the tile's voxels (theta^T = W_theta^T . skip^T, d_skip^T = W_theta . dq^T),
//   * the B operand of v_mfma_f32_16x16x16_{bf16,f16} (k = 4 g + j), so skip feeds the theta product and dq -- an accumulator --
//     feeds the d_skip product with no lane movement, and q / dq never leave registers,
//   * four contiguous channels per lane in memory (8 B in the 16-bit builds, 16 B in the exact-parity f32 mode), the four lane groups
//     of a voxel covering 32 / 64 contiguous bytes.
// A summation index may be permuted freely as long as both operands agree, so the f32 mode runs the same code on four
// v_mfma_f32_16x16x4_f32 per chunk (MFMA j takes element j of both fragments, k = g).
// A tile is the 2 x 8 children of two consecutive low-resolution voxels (v = 8 * which + 4 a + 2 b + c), so the sum of dq over the
// children of a low voxel (d_phi) is a reduction over 8 neighbouring lanes (three DPP adds), not an atomic.
// dW_theta = skip^T . dq sums over VOXELS: the workgroup's four waves transpose their skip and dq fragments through LDS ([channel]
// [voxel]) and share the Cs/16 x Ci/16 output tiles; the accumulators stay in registers over the workgroup's whole voxel loop.
// Parameter gradients: on chip per workgroup, then one float atomic per workgroup and destination (not bit-stable run to run).
#include "vg_common.h"

#define AG_WAVES 4
#define AG_THREADS (AG_WAVES * 64)

#ifdef VG_FP16
typedef __attribute__((ext_vector_type(4))) _Float16 ag_h4;
#endif

template <typename T> struct AgT;
template <> struct AgT<bf16_t> {
    typedef bf16x4 frag;
    static constexpr int SV = 64;          // voxels staged per transpose round (dW_theta); halved where the LDS image would pass 64 KiB
    static constexpr int NQ = 2;           // dq enters the dW_theta product as hi + lo (two 16-bit parts: 16 mantissa bits)
    static __device__ __forceinline__ frag zero() { return (frag){0, 0, 0, 0}; }
    static __device__ __forceinline__ frag load(const bf16_t* p) { return *(const __attribute__((address_space(1))) frag*)(uintptr_t)p; }
    static __device__ __forceinline__ void store(bf16_t* p, frag f) { *(frag*)p = f; }
    static __device__ __forceinline__ frag pack(f32x4 v) { return (frag){(short)f2bf(v[0]), (short)f2bf(v[1]), (short)f2bf(v[2]), (short)f2bf(v[3])}; }
    static __device__ __forceinline__ f32x4 unpack(frag f) { return (f32x4){bf2f((bf16_t)f[0]), bf2f((bf16_t)f[1]), bf2f((bf16_t)f[2]), bf2f((bf16_t)f[3])}; }
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
#ifdef VG_FP16
        return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(ag_h4, a), __builtin_bit_cast(ag_h4, b), c, 0, 0, 0);
#else
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
#endif
    }
};
template <> struct AgT<float> {
    typedef f32x4 frag;
    static constexpr int SV = 32;
    static constexpr int NQ = 1;
    static __device__ __forceinline__ frag zero() { return (frag){0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ frag load(const float* p) { return *(const __attribute__((address_space(1))) frag*)(uintptr_t)p; }
    static __device__ __forceinline__ void store(float* p, frag f) { *(frag*)p = f; }
    static __device__ __forceinline__ frag pack(f32x4 v) { return v; }
    static __device__ __forceinline__ f32x4 unpack(frag f) { return f; }
    static __device__ __forceinline__ f32x4 mma(frag a, frag b, f32x4 c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
        return c;
    }
};

template <int CTRL> __device__ __forceinline__ float ag_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// sum over the 8 lanes 8 i .. 8 i + 7 (every one of them ends with it): quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror
__device__ __forceinline__ float ag_sum8(float v) {
    v += ag_dpp<0xB1>(v); v += ag_dpp<0x4E>(v); v += ag_dpp<0x141>(v);
    return v;
}
__device__ __forceinline__ float ag_sum16(float v) { v = ag_sum8(v); return v + ag_dpp<0x140>(v); }       // + row_mirror
// sum over the four lane groups of a voxel
__device__ __forceinline__ float ag_sum_groups(float v) { v += __shfl_xor(v, 16); return v + __shfl_xor(v, 32); }

struct AgParams {
    const void *skip, *phi, *dg;
    const float *h_in, *wth, *bth, *wpsi, *bpsi;
    void *gated, *dskip, *dphi;
    float *h_out, *sums, *dwth, *dbth, *dwpsi, *dbpsi;
    int N, D, H, W, LH, LW, nlow, niter, acc_skip;
};

// the wave's tile: which voxel this lane owns
struct AgVox { bool valid; int64_t vox, low; };
__device__ __forceinline__ AgVox ag_locate(const AgParams& p, int n, int tile, int v) {
    AgVox r;
    const int j = 2 * tile + (v >> 3);
    r.valid = j < p.nlow;
    const int jj = r.valid ? j : 0;
    const int ld = jj / (p.LH * p.LW), rem = jj - ld * (p.LH * p.LW), lh = rem / p.LW, lw = rem - lh * p.LW;
    const int d = 2 * ld + ((v >> 2) & 1), hh = 2 * lh + ((v >> 1) & 1), w = 2 * lw + (v & 1);
    r.vox = (((int64_t)n * p.D + d) * p.H + hh) * p.W + w;
    r.low = (int64_t)n * p.nlow + jj;
    return r;
}

// W_theta as the A operand of the theta product: row = output channel 16 ti + (l & 15), k = input channels 16 tc + 4 g + {0..3}
template <typename T, int CI> __device__ __forceinline__ typename AgT<T>::frag ag_a_theta(const float* w, int ti, int tc, int lane) {
    const float* q = w + (size_t)(16 * tc + 4 * (lane >> 4)) * CI + 16 * ti + (lane & 15);
    return AgT<T>::pack((f32x4){q[0], q[CI], q[2 * CI], q[3 * CI]});
}
// ... and of the d_skip product: row = input channel 16 tc + (l & 15), k = output channels 16 ti + 4 g + {0..3}
template <typename T, int CI> __device__ __forceinline__ typename AgT<T>::frag ag_a_dskip(const float* w, int tc, int ti, int lane) {
    const float* q = w + (size_t)(16 * tc + (lane & 15)) * CI + 16 * ti + 4 * (lane >> 4);
    return AgT<T>::pack((f32x4){q[0], q[1], q[2], q[3]});
}

// four consecutive floats of a parameter vector (the flat parameter buffer aligns its tensors to 4 bytes only)
__device__ __forceinline__ f32x4 ag_ld4(const float* q) { return (f32x4){q[0], q[1], q[2], q[3]}; }

// theta + b_theta + phi(parent) of the lane's voxel, BEFORE the relu, in the accumulator layout
template <typename T, int CS, int CI, bool HOIST>
__device__ __forceinline__ void ag_preact(const AgParams& p, const AgVox& x, const typename AgT<T>::frag* s,
                                          const typename AgT<T>::frag (*ath)[CS / 16], int lane, f32x4* pre) {
    typedef AgT<T> A;
    constexpr int NTC = CS / 16, NTI = CI / 16;
    const int g = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) {
        f32x4 acc = ag_ld4(p.bth + 16 * ti + 4 * g);
        if (x.valid) acc += A::unpack(A::load((const T*)p.phi + x.low * CI + 16 * ti + 4 * g));
#pragma unroll
        for (int tc = 0; tc < NTC; ++tc)
            acc = A::mma(HOIST ? ath[HOIST ? ti : 0][tc] : ag_a_theta<T, CI>(p.wth, ti, tc, lane), s[tc], acc);
        pre[ti] = acc;
    }
}

template <typename T, int CS, int CI>
__global__ __launch_bounds__(AG_THREADS) void ag_fwd_kernel(const AgParams p) {
    typedef AgT<T> A;
    typedef typename A::frag frag;
    constexpr int NTC = CS / 16, NTI = CI / 16;
    constexpr bool HOIST = NTC * NTI <= 8;
    __shared__ float red[AG_WAVES][CS][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane & 15, g = lane >> 4, n = blockIdx.y;
    frag ath[HOIST ? NTI : 1][NTC];
    if (HOIST) {
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
            for (int tc = 0; tc < NTC; ++tc) ath[HOIST ? ti : 0][tc] = ag_a_theta<T, CI>(p.wth, ti, tc, lane);
    }
    const float bpsi = p.bpsi[0];
    f32x4 s1[NTC], s2[NTC];
#pragma unroll
    for (int tc = 0; tc < NTC; ++tc) { s1[tc] = (f32x4){0.f, 0.f, 0.f, 0.f}; s2[tc] = s1[tc]; }
    for (int it = blockIdx.x; it < p.niter; it += gridDim.x) {
        const AgVox x = ag_locate(p, n, it * AG_WAVES + wave, v);
        frag s[NTC];
#pragma unroll
        for (int tc = 0; tc < NTC; ++tc) s[tc] = x.valid ? A::load((const T*)p.skip + x.vox * CS + 16 * tc + 4 * g) : A::zero();
        f32x4 pre[NTI];
        ag_preact<T, CS, CI, HOIST>(p, x, s, ath, lane, pre);
        float z = 0.f;
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti) {
            const f32x4 wp = ag_ld4(p.wpsi + 16 * ti + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) z += fmaxf(pre[ti][r], 0.f) * wp[r];
        }
        z = ag_sum_groups(z) + bpsi;
        const float hv = 1.f / (1.f + __expf(-z));
        if (x.valid) {
            if (g == 0) p.h_out[x.vox] = hv;
#pragma unroll
            for (int tc = 0; tc < NTC; ++tc) {
                const frag o = A::pack(A::unpack(s[tc]) * hv);
                A::store((T*)p.gated + x.vox * CS + 16 * tc + 4 * g, o);
                const f32x4 st = A::unpack(o);                         // the statistics are those of the STORED values
                s1[tc] += st; s2[tc] += st * st;
            }
        }
    }
    // per-(n, c) sums: over the wave's 16 voxel lanes, over the waves through LDS, one atomic per workgroup and entry
#pragma unroll
    for (int tc = 0; tc < NTC; ++tc)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = ag_sum16(s1[tc][r]), b = ag_sum16(s2[tc][r]);
            if (v == 0) { red[wave][16 * tc + 4 * g + r][0] = a; red[wave][16 * tc + 4 * g + r][1] = b; }
        }
    __syncthreads();
    const int stripe = blockIdx.x & (VG_STRIPES - 1);
    for (int i = threadIdx.x; i < CS * 2; i += AG_THREADS) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < AG_WAVES; ++w) a += red[w][i >> 1][i & 1];
        atomicAdd(p.sums + (((size_t)stripe * p.N + n) * CS + (i >> 1)) * 2 + (i & 1), a);
    }
}

template <typename T, int CS, int CI>
__global__ __launch_bounds__(AG_THREADS) void ag_bwd_kernel(const AgParams p) {
    typedef AgT<T> A;
    typedef typename A::frag frag;
    constexpr int NTC = CS / 16, NTI = CI / 16, NT = NTC * NTI, MYT = (NT + AG_WAVES - 1) / AG_WAVES;
    constexpr bool HOIST = NT <= 8;
    constexpr int NQ = A::NQ;
    constexpr int SV = (size_t)(CS + NQ * CI) * (A::SV + 4) * sizeof(T) > 65536 ? A::SV / 2 : A::SV;
    constexpr int LDW = SV + 4, WPR = SV / 16, ROUNDS = AG_WAVES / WPR;                 // LDS row: SV voxels + 4 (rows stay 8 / 16 B aligned)
    __shared__ __attribute__((aligned(16))) T tr[(CS + NQ * CI) * LDW];                 // [channel of skip ; channel of dq (hi ; lo)][voxel]
    T* const sT = tr;
    T* const qT = tr + CS * LDW;
    T* const qT2 = qT + CI * LDW;            // (NQ == 2) the low parts
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = lane & 15, g = lane >> 4, n = blockIdx.y;
    frag ath[HOIST ? NTI : 1][NTC], ads[HOIST ? NTC : 1][NTI];
    if (HOIST) {
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
            for (int tc = 0; tc < NTC; ++tc) {
                ath[HOIST ? ti : 0][tc] = ag_a_theta<T, CI>(p.wth, ti, tc, lane);
                ads[HOIST ? tc : 0][ti] = ag_a_dskip<T, CI>(p.wth, tc, ti, lane);
            }
    }
    f32x4 accw[MYT], dbt[NTI], dwp[NTI];
    float dbp = 0.f;
#pragma unroll
    for (int j = 0; j < MYT; ++j) accw[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) { dbt[ti] = (f32x4){0.f, 0.f, 0.f, 0.f}; dwp[ti] = dbt[ti]; }
    for (int it = blockIdx.x; it < p.niter; it += gridDim.x) {
        const AgVox x = ag_locate(p, n, it * AG_WAVES + wave, v);
        frag s[NTC], dgf[NTC];
#pragma unroll
        for (int tc = 0; tc < NTC; ++tc) {
            s[tc] = x.valid ? A::load((const T*)p.skip + x.vox * CS + 16 * tc + 4 * g) : A::zero();
            dgf[tc] = x.valid ? A::load((const T*)p.dg + x.vox * CS + 16 * tc + 4 * g) : A::zero();
        }
        const float hv = x.valid ? p.h_in[x.vox] : 0.f;
        f32x4 pre[NTI];
        ag_preact<T, CS, CI, HOIST>(p, x, s, ath, lane, pre);          // theta and q are recomputed, never stored
        float dh = 0.f;
#pragma unroll
        for (int tc = 0; tc < NTC; ++tc) {
            const f32x4 a = A::unpack(s[tc]), b = A::unpack(dgf[tc]);
            dh += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
        }
        dh = ag_sum_groups(dh);
        const float dz = dh * hv * (1.f - hv);
        if (g == 0) dbp += dz;
        frag dqf[NTI], dql[NQ == 2 ? NTI : 1];
        const bool low_writer = x.valid && (v & 7) == 0;
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti) {
            const f32x4 wp = ag_ld4(p.wpsi + 16 * ti + 4 * g);
            f32x4 dq, dlow;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float q = fmaxf(pre[ti][r], 0.f);
                dq[r] = q > 0.f ? dz * wp[r] : 0.f;
                dwp[ti][r] += dz * q;
                dlow[r] = ag_sum8(dq[r]);                               // the 8 children of the low-resolution voxel
            }
            dbt[ti] += dq;
            dqf[ti] = A::pack(dq);
            // a weight gradient is a sum over every voxel that may cancel to a small fraction of its terms: the 2^-9 rounding of a single
            // 16-bit operand would show in it at full size, so dW_theta takes dq as hi + lo (d_skip, a 16-bit tensor, takes hi alone)
            if (NQ == 2) dql[NQ == 2 ? ti : 0] = A::pack(dq - A::unpack(dqf[ti]));
            if (low_writer) A::store((T*)p.dphi + x.low * CI + 16 * ti + 4 * g, A::pack(dlow));
        }
        // d_skip = dG * h + dq . W_theta^T
#pragma unroll
        for (int tc = 0; tc < NTC; ++tc) {
            f32x4 acc = A::unpack(dgf[tc]) * hv;
#pragma unroll
            for (int ti = 0; ti < NTI; ++ti)
                acc = A::mma(HOIST ? ads[HOIST ? tc : 0][ti] : ag_a_dskip<T, CI>(p.wth, tc, ti, lane), dqf[ti], acc);
            if (x.valid) {
                T* const o = (T*)p.dskip + x.vox * CS + 16 * tc + 4 * g;
                if (p.acc_skip) acc += A::unpack(A::load(o));
                A::store(o, A::pack(acc));
            }
        }
        // dW_theta += skip^T . dq over the workgroup's 64 voxels: transpose through LDS, SV voxels per round
#pragma unroll
        for (int rd = 0; rd < ROUNDS; ++rd) {
            __syncthreads();
            if (wave / WPR == rd) {
                const int col = (wave % WPR) * 16 + v;
#pragma unroll
                for (int tc = 0; tc < NTC; ++tc)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sT[(16 * tc + 4 * g + r) * LDW + col] = s[tc][r];
#pragma unroll
                for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        qT[(16 * ti + 4 * g + r) * LDW + col] = dqf[ti][r];
                        if (NQ == 2) qT2[(16 * ti + 4 * g + r) * LDW + col] = dql[NQ == 2 ? ti : 0][r];
                    }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < MYT; ++j) {
                const int id = wave + AG_WAVES * j;
                if (id < NT) {
                    const int tc = id / NTI, ti = id - tc * NTI;
#pragma unroll
                    for (int ks = 0; ks < WPR; ++ks) {
                        const frag a = *(const frag*)(sT + (16 * tc + v) * LDW + 16 * ks + 4 * g);
                        const frag b = *(const frag*)(qT + (16 * ti + v) * LDW + 16 * ks + 4 * g);
                        accw[j] = A::mma(a, b, accw[j]);
                        if (NQ == 2) accw[j] = A::mma(a, *(const frag*)(qT2 + (16 * ti + v) * LDW + 16 * ks + 4 * g), accw[j]);
                    }
                }
            }
        }
    }
    // ---- parameter gradients: one atomic per workgroup and destination ----
#pragma unroll
    for (int j = 0; j < MYT; ++j) {
        const int id = wave + AG_WAVES * j;
        if (id < NT) {
            const int tc = id / NTI, ti = id - tc * NTI;
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(p.dwth + (size_t)(16 * tc + 4 * g + r) * CI + 16 * ti + v, accw[j][r]);
        }
    }
    __syncthreads();
    float* const red = (float*)tr;                  // [wave][2][CI] + [wave]: at most 4 * 513 floats <= the transpose image
    static_assert((size_t)(CS + NQ * CI) * LDW * sizeof(T) <= 65536 && (size_t)(CS + CI) * LDW * sizeof(T) >= (size_t)AG_WAVES * (2 * CI + 1) * sizeof(float), "reduction scratch");
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float a = ag_sum16(dbt[ti][r]), b = ag_sum16(dwp[ti][r]);
            if (v == 0) { red[(wave * 2) * CI + 16 * ti + 4 * g + r] = a; red[(wave * 2 + 1) * CI + 16 * ti + 4 * g + r] = b; }
        }
    dbp = wave_sum(dbp);
    if (lane == 0) red[AG_WAVES * 2 * CI + wave] = dbp;
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * CI; i += AG_THREADS) {
        const int k = i / CI, c = i - k * CI;
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < AG_WAVES; ++w) a += red[(w * 2 + k) * CI + c];
        atomicAdd((k ? p.dwpsi : p.dbth) + c, a);
    }
    if (threadIdx.x == 0) {
        float a = 0.f;
        for (int w = 0; w < AG_WAVES; ++w) a += red[AG_WAVES * 2 * CI + w];
        atomicAdd(p.dbpsi, a);
    }
}

static bool ag_shape_ok(int N, int D, int H, int W, int Cs, int Ci) {
    if (N < 1 || N > 65535 || D < 2 || H < 2 || W < 2 || (D | H | W) & 1) return false;
    if ((int64_t)N * D * H * W > ((int64_t)1 << 31)) return false;
    return Ci == 2 * Cs && (Cs == 16 || Cs == 32 || Cs == 64 || Cs == 128);
}
static void ag_geometry(AgParams& p, int N, int D, int H, int W) {
    p.N = N; p.D = D; p.H = H; p.W = W; p.LH = H / 2; p.LW = W / 2;
    p.nlow = (D / 2) * p.LH * p.LW;
    p.niter = (int)cdiv64(cdiv64(p.nlow, 2), AG_WAVES);
}
static bool ag_aligned(const void* q) { return q && !((uintptr_t)q & 15); }

template <typename T> static void ag_launch_fwd(const AgParams& p, int Cs, dim3 grid, hipStream_t s) {
    switch (Cs) {
        case 16: hipLaunchKernelGGL((ag_fwd_kernel<T, 16, 32>), grid, dim3(AG_THREADS), 0, s, p); break;
        case 32: hipLaunchKernelGGL((ag_fwd_kernel<T, 32, 64>), grid, dim3(AG_THREADS), 0, s, p); break;
        case 64: hipLaunchKernelGGL((ag_fwd_kernel<T, 64, 128>), grid, dim3(AG_THREADS), 0, s, p); break;
        default: hipLaunchKernelGGL((ag_fwd_kernel<T, 128, 256>), grid, dim3(AG_THREADS), 0, s, p); break;
    }
}
template <typename T> static void ag_launch_bwd(const AgParams& p, int Cs, dim3 grid, hipStream_t s) {
    switch (Cs) {
        case 16: hipLaunchKernelGGL((ag_bwd_kernel<T, 16, 32>), grid, dim3(AG_THREADS), 0, s, p); break;
        case 32: hipLaunchKernelGGL((ag_bwd_kernel<T, 32, 64>), grid, dim3(AG_THREADS), 0, s, p); break;
        case 64: hipLaunchKernelGGL((ag_bwd_kernel<T, 64, 128>), grid, dim3(AG_THREADS), 0, s, p); break;
        default: hipLaunchKernelGGL((ag_bwd_kernel<T, 128, 256>), grid, dim3(AG_THREADS), 0, s, p); break;
    }
}

extern "C" int vg_attn_gate_fwd(const void* skip, const void* phi, const float* w_theta, const float* b_theta, const float* w_psi,
                                const float* b_psi, int N, int D, int H, int W, int Cs, int Ci, int f32, void* gated, float* h, float* sums,
                                vg_stream_t stream) {
    vg_begin();
    if (!ag_shape_ok(N, D, H, W, Cs, Ci) || !ag_aligned(skip) || !ag_aligned(phi) || !w_theta || !b_theta
        || !w_psi || !b_psi || !ag_aligned(gated) || !h || !sums) return VG_EINVAL;
    AgParams p = {};
    ag_geometry(p, N, D, H, W);
    p.skip = skip; p.phi = phi; p.wth = w_theta; p.bth = b_theta; p.wpsi = w_psi; p.bpsi = b_psi;
    p.gated = gated; p.h_out = h; p.sums = sums;
    const dim3 grid(p.niter < 2048 ? p.niter : 2048, N);
    if (f32) ag_launch_fwd<float>(p, Cs, grid, (hipStream_t)stream);
    else ag_launch_fwd<bf16_t>(p, Cs, grid, (hipStream_t)stream);
    return vg_check_launch();
}

extern "C" int vg_attn_gate_bwd(const void* dg, const void* skip, const float* h, const void* phi, const float* w_theta,
                                const float* b_theta, const float* w_psi, int N, int D, int H, int W, int Cs, int Ci, int f32, void* dskip,
                                int accumulate, void* dphi, float* dw_theta, float* db_theta, float* dw_psi, float* db_psi,
                                vg_stream_t stream) {
    vg_begin();
    if (!ag_shape_ok(N, D, H, W, Cs, Ci) || !ag_aligned(dg) || !ag_aligned(skip) || !h || !ag_aligned(phi) || !w_theta
        || !b_theta || !w_psi || !ag_aligned(dskip) || !ag_aligned(dphi) || !dw_theta || !db_theta || !dw_psi
        || !db_psi) return VG_EINVAL;
    AgParams p = {};
    ag_geometry(p, N, D, H, W);
    p.dg = dg; p.skip = skip; p.h_in = h; p.phi = phi; p.wth = w_theta; p.bth = b_theta; p.wpsi = w_psi;
    p.dskip = dskip; p.acc_skip = accumulate ? 1 : 0; p.dphi = dphi;
    p.dwth = dw_theta; p.dbth = db_theta; p.dwpsi = dw_psi; p.dbpsi = db_psi;
    // every workgroup ends with Cs * Ci + 2 Ci + 1 float atomics: fewer, longer-running workgroups where the kernel is large
    int cap = (1 << 21) / (Cs * Ci);
    cap = cap < 64 ? 64 : (cap > 2048 ? 2048 : cap);
    const dim3 grid(p.niter < cap ? p.niter : cap, N);
    if (f32) ag_launch_bwd<float>(p, Cs, grid, (hipStream_t)stream);
    else ag_launch_bwd<bf16_t>(p, Cs, grid, (hipStream_t)stream);
    return vg_check_launch();
}
