// vg_specnorm.hip -- spectral normalisation of the discriminator's wrapped convolution kernels (get_discriminator(use_SN=True),
// discriminator.py:16,54-61,86,100; building_blocks.py:172-180): the power iteration of tfa.layers.SpectralNormalization
// (power_iterations = 1) on the fp32 master weights, multi-tensor -- one call serves every wrapped kernel of a network from a device
// table (vg_sn_item), as vg_adam_clip serves every tensor of its flat buffer.
//
// TP (TensorFlow Addons, restated): W in Keras layout viewed as [K = k^3 * Cin][Cout], u [1][Cout] stored,
//   l2n(x) = x * rsqrt(max(sum(x * x), 1e-12));  v = l2n(u W^T);  u' = l2n(v W);  sigma = (v W) u'^T;  u <- u';  W <- W / sigma.
//
// t = W u^T and s = t W are both linear in W, so ONE pass over a slab of rows gives t_k, sum t_k^2 and the un-normalised column sums
// sum_k t_k W[k][:] while the row is still in registers; v is never materialised: v W = s * rsqrt(max(|t|^2, 1e-12)).  Projection
// p > 0 of a call reads the ORIGINAL W with the row scale c = 1 / (sigma_1 ... sigma_p) (the earlier projections' W / sigma is not
// written), and the last pass writes W * c: n projections are n reads + one read-modify-write of W.
//
// Cross-workgroup phases are SEPARATE LAUNCHES (pass -> fold -> ... -> scale), and there is no floating-point atomic: a workgroup
// leaves its per-column partial sums in the caller's scratch, the fold adds them in block order.  Every sum has one fixed
// association, so the result is bit-identical from run to run and from rank to rank (data-parallel replicas never exchange W or u
// after the initial broadcast).
#include "vg_common.h"

#define SN_THREADS 1024
#define SN_WAVES (SN_THREADS / 64)
#define SN_CHUNK 256                  // floats one wave moves per instruction: 64 lanes x 16 B
#define SN_NCH 8                      // chunks a wave holds in registers at once (8 KiB in flight per wave)
#define SN_ROUNDS 2
#define SN_SLAB (SN_WAVES * SN_NCH * SN_ROUNDS * SN_CHUNK)      // 65536 floats (256 KiB) of W per workgroup
#define SN_PSTRIDE (VG_SN_MAX_COUT + 4)                          // scratch floats per workgroup: column partials, then sum t^2
#define SN_EPS 1e-12f
static_assert(SN_SLAB == VG_SN_SLAB, "include/vangan_hip.h: VG_SN_SLAB");

typedef const __attribute__((address_space(1))) f32x4* sn_gp4;

// the item whose workgroups [blk0, blk0 + nblk) hold blk (block-uniform; T <= VG_SN_MAX_ITEMS)
__device__ __forceinline__ int sn_find(const vg_sn_item* items, int T, int blk) {
    int i = 0;
    while (i + 1 < T && blk >= items[i].blk0 + items[i].nblk) ++i;
    return i;
}
__device__ __forceinline__ float sn_row_scale(const vg_sn_item& it, int first) { return first ? 1.f : it.state[VG_SN_STATE_CUM]; }

// One slab of rows of a [K][COUT] kernel.  A wave owns whole rows: a row is CPR chunks of 256 floats (COUT = 512) or a chunk holds RPC
// rows of LPR lanes each (COUT <= 256); lane l keeps the columns cp * 256 + (l % LPR) * 4 + {0..3} of its rows' running sums.
template <int COUT>
__device__ __forceinline__ void sn_pass_slab(const vg_sn_item& it, int slab, float rs, float* part, float* lds) {
    constexpr int LPR = COUT / 4 < 64 ? COUT / 4 : 64;
    constexpr int CPR = COUT > 256 ? COUT / 256 : 1;
    constexpr int RPC = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col0 = (lane % LPR) * 4;
    const int64_t total = (int64_t)it.K * COUT;
    f32x4 u[CPR], acc[CPR];
#pragma unroll
    for (int cp = 0; cp < CPR; ++cp) { u[cp] = *(const f32x4*)(it.u + cp * 256 + col0); acc[cp] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    float tt = 0.f;
#pragma unroll
    for (int r = 0; r < SN_ROUNDS; ++r) {
        const int64_t base = (int64_t)slab * SN_SLAB + (int64_t)((r * SN_WAVES + wave) * SN_NCH) * SN_CHUNK;
        f32x4 w[SN_NCH];
#pragma unroll
        for (int j = 0; j < SN_NCH; ++j) {           // K * COUT is a multiple of SN_CHUNK: a chunk is inside W or outside it
            const int64_t off = base + (int64_t)j * SN_CHUNK;
            w[j] = off < total ? *(sn_gp4)(uintptr_t)(it.w + off + lane * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int g = 0; g < SN_NCH / CPR; ++g) {
            float d = 0.f;
#pragma unroll
            for (int cp = 0; cp < CPR; ++cp)
#pragma unroll
                for (int e = 0; e < 4; ++e) d += w[g * CPR + cp][e] * u[cp][e];
#pragma unroll
            for (int o = LPR / 2; o > 0; o >>= 1) d += __shfl_xor(d, o);       // every lane of the row ends with the row's sum
            const float t = d * rs;
            tt += t * t;
#pragma unroll
            for (int cp = 0; cp < CPR; ++cp)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[cp][e] += t * w[g * CPR + cp][e];
        }
    }
    // fold over the workgroup in a fixed order: [wave][row group of the wave][column] in LDS, then one thread per column
    float* red = lds + SN_WAVES * RPC * COUT;
#pragma unroll
    for (int cp = 0; cp < CPR; ++cp) *(f32x4*)(lds + (wave * RPC + lane / LPR) * COUT + cp * 256 + col0) = acc[cp];
    tt = wave_sum((lane % LPR) == 0 ? tt : 0.f);
    if (lane == 0) red[wave] = tt;
    __syncthreads();
    for (int c = threadIdx.x; c < COUT; c += SN_THREADS) {
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < SN_WAVES * RPC; ++j) s += lds[j * COUT + c];
        part[c] = s;
    }
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int j = 0; j < SN_WAVES; ++j) s += red[j];
        part[VG_SN_MAX_COUT] = s;
    }
}

__global__ __launch_bounds__(SN_THREADS) void sn_pass_kernel(const vg_sn_item* items, int T, int total_blocks, int first, float* scratch) {
    __shared__ float lds[SN_WAVES * VG_SN_MAX_COUT + SN_WAVES];       // SN_WAVES * RPC * COUT <= SN_WAVES * 512 for every served COUT
    const int blk = blockIdx.x;
    if (blk >= total_blocks) return;
    const vg_sn_item it = items[sn_find(items, T, blk)];
    const int slab = blk - it.blk0;
    if (slab < 0 || slab >= it.nblk) return;
    const float rs = sn_row_scale(it, first);
    float* part = scratch + (int64_t)blk * SN_PSTRIDE;
    switch (it.Cout) {
        case 64: sn_pass_slab<64>(it, slab, rs, part, lds); break;
        case 128: sn_pass_slab<128>(it, slab, rs, part, lds); break;
        case 256: sn_pass_slab<256>(it, slab, rs, part, lds); break;
        case 512: sn_pass_slab<512>(it, slab, rs, part, lds); break;
        default: break;
    }
}

// One workgroup per item: column sums over the item's workgroups in block order, u' = l2n(v W), sigma, the cumulative 1 / sigma.
// sigma == 0 (an all-zero W or u: l2n's clamp keeps everything finite) leaves u and the cumulative scale as they are -- the
// projection is then the identity and nothing is divided by zero.
__global__ __launch_bounds__(SN_THREADS) void sn_fold_kernel(const vg_sn_item* items, int total_blocks, int p, const float* scratch) {
    __shared__ float cs[SN_THREADS];
    __shared__ float s_true[VG_SN_MAX_COUT];
    __shared__ float red[SN_WAVES];
    __shared__ float tt_s;
    const vg_sn_item it = items[blockIdx.x];
    const int C = it.Cout, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((C != 64 && C != 128 && C != 256 && C != 512) || it.blk0 < 0) return;
    const int nb = it.blk0 + it.nblk <= total_blocks ? it.nblk : 0;
    const float* part = scratch + (int64_t)it.blk0 * SN_PSTRIDE;
    const int H = SN_THREADS / C, c = tid % C, h = tid / C;      // H interleaved subsets of the partial rows per column
    float s = 0.f;
#pragma unroll 32                // the loads of a batch are in flight together
    for (int b = h; b < nb; b += H) s += part[(int64_t)b * SN_PSTRIDE + c];
    cs[tid] = s;
    if (wave == 0) {
        float t = 0.f;
        for (int b = lane; b < nb; b += 64) t += part[(int64_t)b * SN_PSTRIDE + VG_SN_MAX_COUT];
        t = wave_sum(t);
        if (lane == 0) tt_s = t;
    }
    __syncthreads();
    const float rs = sn_row_scale(it, p == 0);
    const float rn_t = rsqrtf(fmaxf(tt_s, SN_EPS));
    float x = 0.f;
    if (tid < C) {
        float a = 0.f;
        for (int j = 0; j < H; ++j) a += cs[j * C + tid];
        x = a * rs * rn_t;                                       // (v W)[c] with W = rs * the stored kernel
        s_true[tid] = x;
    }
    const float q = wave_sum(x * x);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    float nn = 0.f;
    for (int j = 0; j < SN_WAVES; ++j) nn += red[j];
    const float rn = rsqrtf(fmaxf(nn, SN_EPS));
    const float sigma = nn * rn;                                 // (v W) . u'
    const bool ok = sigma > 0.f && sigma < INFINITY;
    if (ok && tid < C) it.u[tid] = s_true[tid] * rn;
    if (tid == 0) {
        it.state[p] = ok ? sigma : 0.f;
        it.state[VG_SN_STATE_CUM] = ok ? rs / sigma : rs;
    }
}

__global__ __launch_bounds__(SN_THREADS) void sn_scale_kernel(const vg_sn_item* items, int T, int total_blocks) {
    const int blk = blockIdx.x;
    if (blk >= total_blocks) return;
    const vg_sn_item it = items[sn_find(items, T, blk)];
    const int slab = blk - it.blk0;
    if (slab < 0 || slab >= it.nblk) return;
    const float rs = it.state[VG_SN_STATE_CUM];
    if (rs == 1.f) return;                                       // every projection of the call was the identity
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t total = (int64_t)it.K * it.Cout;
    for (int r = 0; r < SN_ROUNDS; ++r) {
        const int64_t base = (int64_t)slab * SN_SLAB + (int64_t)((r * SN_WAVES + wave) * SN_NCH) * SN_CHUNK;
        float* p = it.w + base + lane * 4;
        const int nch = total - base >= SN_NCH * SN_CHUNK ? SN_NCH : (total > base ? (int)((total - base) / SN_CHUNK) : 0);     // wave-uniform
        f32x4 w[SN_NCH];
#pragma unroll
        for (int j = 0; j < SN_NCH; ++j) w[j] = j < nch ? *(sn_gp4)(uintptr_t)(p + j * SN_CHUNK) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < SN_NCH; ++j)
            if (j < nch) *(f32x4*)(p + j * SN_CHUNK) = w[j] * rs;
    }
}

extern "C" int vg_spectral_norm_blocks(int K, int Cout) {
    if (K < 1 || (Cout != 64 && Cout != 128 && Cout != 256 && Cout != 512)) return VG_EINVAL;
    const int64_t total = (int64_t)K * Cout;
    if (total % SN_CHUNK || total > ((int64_t)1 << 36)) return VG_EINVAL;
    return (int)cdiv64(total, SN_SLAB);
}
extern "C" int64_t vg_spectral_norm_scratch_bytes(int total_blocks) {
    if (total_blocks < 1) return VG_EINVAL;
    return (int64_t)total_blocks * SN_PSTRIDE * (int64_t)sizeof(float);
}
extern "C" int vg_spectral_norm(const vg_sn_item* items_dev, int T, int total_blocks, int n_proj, float* scratch, int64_t scratch_bytes,
                                vg_stream_t stream) {
    vg_begin();
    if (!items_dev || !scratch || T < 1 || T > VG_SN_MAX_ITEMS || total_blocks < T || n_proj < 1 || n_proj > VG_SN_MAX_PROJ
        || ((uintptr_t)scratch & 15) || scratch_bytes < vg_spectral_norm_scratch_bytes(total_blocks)) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    for (int p = 0; p < n_proj; ++p) {
        hipLaunchKernelGGL(sn_pass_kernel, dim3(total_blocks), dim3(SN_THREADS), 0, s, items_dev, T, total_blocks, p == 0 ? 1 : 0, scratch);
        hipLaunchKernelGGL(sn_fold_kernel, dim3(T), dim3(SN_THREADS), 0, s, items_dev, total_blocks, p, (const float*)scratch);
    }
    hipLaunchKernelGGL(sn_scale_kernel, dim3(total_blocks), dim3(SN_THREADS), 0, s, items_dev, T, total_blocks);
    return vg_check_launch();
}
