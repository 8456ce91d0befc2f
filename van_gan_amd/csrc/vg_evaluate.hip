// vg_evaluate.hip -- scoring a vessel mask against a ground truth (van_gan_amd/postprocess.py overlap_counts, mask_surface,
// euler_characteristic, betti_numbers, surface_distances, cldice_score, evaluate_segmentation; include/vangan_hip.h "Scoring a mask";
// DESIGN.md 3.20): the four overlap counts of two masks, the surface voxels of a mask, the cells of its cubical complex (the Euler
// characteristic), the labels that reach no face (the cavities), and count / maximum / sum / order statistics of a 32-bit array over the
// selected voxels.  Nothing here depends on the 16-bit storage format of the build.  256-thread workgroups (4 wave64) on a
// one-dimensional grid of at most VOL_MAX_BLOCKS workgroups; every loop is a grid stride over a count known at launch.  Only integer
// atomics, every one of them a sum: no result depends on their order.  The one floating-point sum goes through per-workgroup partials in
// the scratch that one workgroup adds in a fixed order (the scheme of vg_volume_moments).
#include "vg_volume.h"

typedef unsigned long long ev_u64;

// n = X * Y * Z where the shape is served (extents >= 1, n < 2^31), else 0
static inline int64_t ev_voxels(int X, int Y, int Z) {
    if (X < 1 || Y < 1 || Z < 1) return 0;
    if ((int64_t)X * Y >= ((int64_t)1 << 31)) return 0;                    // so that the product below cannot overflow
    const int64_t n = (int64_t)X * Y * Z;
    return n < ((int64_t)1 << 31) ? n : 0;
}
static inline bool ev_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }
static inline bool ev_overlap(const void* a, const void* b, int64_t bytes) {
    return (uintptr_t)a < (uintptr_t)b + (uintptr_t)bytes && (uintptr_t)b < (uintptr_t)a + (uintptr_t)bytes;
}

// 0x01 in every byte of x that is not 0
__device__ __forceinline__ unsigned ev_nonzero4(unsigned x) { return ((x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; }

__device__ __forceinline__ unsigned ev_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The K counters of every thread added over the workgroup: per wave by shuffles, the four waves through LDS; thread k < K returns the
// total of counter k, every other thread 0.  Called by all 256 threads.
template <int K>
__device__ __forceinline__ ev_u64 ev_block_sums(const unsigned (&c)[K], unsigned (*wsum)[K]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned s = ev_wave_sum(c[k]);
        if ((t & 63) == 0) wsum[t >> 6][k] = s;
    }
    __syncthreads();
    return t < K ? (ev_u64)wsum[0][t] + wsum[1][t] + wsum[2][t] + wsum[3][t] : 0ull;
}

// ------------------------------------------------------------------------------------------------ overlap counts
// Elements [head, head + 16 nv) go in 16-byte loads, sixteen voxels of each mask a lane; the head (what brings both pointers to a 16-byte
// boundary) and the tail go one voxel a lane.  A thread counts |a|, |b| and |a & b|; the four counters follow from them and n:
// counts[3] = n - |a| - |b| + |a & b|, which workgroup 0 starts with n and every workgroup lowers -- a sum of 64-bit integers modulo 2^64
// whose final value is the count.
__global__ __launch_bounds__(256) void ev_counts_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t n, int64_t head,
                                                        int64_t nv, ev_u64* __restrict__ counts) {
    __shared__ unsigned wsum[4][3];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    unsigned c[3] = {0u, 0u, 0u};                                   // |a & b|, |a|, |b|
    for (int64_t i = tid; i < nv; i += nthr) {
        const uint4 x = *(const uint4*)(a + head + i * 16), y = *(const uint4*)(b + head + i * 16);
        const unsigned xw[4] = {x.x, x.y, x.z, x.w}, yw[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned na = ev_nonzero4(xw[j]), nb = ev_nonzero4(yw[j]);
            c[0] += __popc(na & nb); c[1] += __popc(na); c[2] += __popc(nb);
        }
    }
    const int64_t rest = n - nv * 16;
    for (int64_t e = tid; e < rest; e += nthr) {
        const int64_t i = e < head ? e : e + nv * 16;
        const unsigned na = a[i] != 0, nb = b[i] != 0;
        c[0] += na & nb; c[1] += na; c[2] += nb;
    }
    const ev_u64 s = ev_block_sums<3>(c, wsum);
    const int t = threadIdx.x;
    if (t == 0) {
        const ev_u64 uni = (ev_u64)wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1] + wsum[0][2] + wsum[1][2] + wsum[2][2] + wsum[3][2] - s;   // |a or b|
        atomicAdd(&counts[0], s);
        atomicAdd(&counts[3], (blockIdx.x == 0 ? (ev_u64)n : 0ull) - uni);
    } else if (t < 3) {
        const ev_u64 both = (ev_u64)wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
        atomicAdd(&counts[t], s - both);                            // |a & !b|, |!a & b|
    }
}

extern "C" int vg_mask_counts(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* counts4, vg_stream_t stream) {
    vg_begin();
    if (!a || !b || !counts4 || !ev_n_ok(n) || (uintptr_t)counts4 % 8 != 0) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int64_t head = (int64_t)((16 - (uintptr_t)a % 16) % 16), nv = 0;
    if (((uintptr_t)b + (uintptr_t)head) % 16 == 0 && head < n) nv = (n - head) / 16;
    if (nv == 0) head = 0;
    if (hipMemsetAsync(counts4, 0, 32, s) != hipSuccess) return VG_ELAUNCH;
    hipLaunchKernelGGL(ev_counts_kernel, dim3(vol_blocks(nv + (n - nv * 16))), dim3(256), 0, s, a, b, n, head, nv, (ev_u64*)counts4);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ surface
// The wave scheme of sg_classify_kernel (vg_skelgraph.hip): a wave takes a piece of 62 lanes' worth of z of one row (x, y), lanes 0 and
// 63 the halo, and walks the pieces by a grid stride.  W = 4: a lane holds four consecutive voxels in one 32-bit word, a byte each (0 /
// 1), and the arithmetic stays packed; it needs Z % 4 == 0 and 4-byte aligned pointers, so that every word lies in one row.  W = 1: a
// byte per lane, any Z.  A voxel is interior when it and its six face neighbours are foreground; what lies outside the volume is not.
template <int W>
__device__ __forceinline__ unsigned ev_load_nz(const uint8_t* p) { return W == 4 ? ev_nonzero4(*(const unsigned*)p) : (unsigned)(*p != 0); }

template <int W>
__global__ __launch_bounds__(256) void ev_surface_kernel(const uint8_t* __restrict__ mask, int64_t pieces, int np, int X, int Y, int Z,
                                                         uint8_t* __restrict__ surf, uint8_t* __restrict__ nsurf, ev_u64* __restrict__ count) {
    __shared__ unsigned wsum[4][1];
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const unsigned ones = W == 4 ? 0x01010101u : 1u;
    unsigned c[1] = {0u};
    for (int64_t pi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); pi < pieces; pi += nw) {         // uniform over the wave
        const int64_t row = pi / np;
        const int x = (int)(row / Y), y = (int)(row - (int64_t)x * Y);
        const int z = ((int)(pi - row * np) * 62 - 1 + lane) * W;
        const bool inz = z >= 0 && z < Z;
        unsigned self = 0u, side = 0u;
        if (inz) {
            const uint8_t* p = mask + row * Z + z;
            self = ev_load_nz<W>(p);
            side = self;
            side &= x > 0 ? ev_load_nz<W>(p - (int64_t)Y * Z) : 0u;
            side &= x < X - 1 ? ev_load_nz<W>(p + (int64_t)Y * Z) : 0u;
            side &= y > 0 ? ev_load_nz<W>(p - Z) : 0u;
            side &= y < Y - 1 ? ev_load_nz<W>(p + Z) : 0u;
        }
        const unsigned below = __shfl_up(self, 1), above = __shfl_down(self, 1);
        if (lane >= 1 && lane <= 62 && inz) {
            const unsigned zm = W == 4 ? (self << 8) | (below >> 24) : below, zp = W == 4 ? (self >> 8) | (above << 24) : above;
            const unsigned sf = self & ~(side & zm & zp);
            const int64_t o = row * Z + z;
            if (W == 4) {
                if (surf) *(unsigned*)(surf + o) = sf;
                if (nsurf) *(unsigned*)(nsurf + o) = sf ^ ones;
            } else {
                if (surf) surf[o] = (uint8_t)sf;
                if (nsurf) nsurf[o] = (uint8_t)(sf ^ ones);
            }
            c[0] += __popc(sf);
        }
    }
    const ev_u64 s = ev_block_sums<1>(c, wsum);
    if (threadIdx.x == 0 && s) atomicAdd(count, s);
}

// pieces of `per` payload lanes that cover `lanes` lanes of each of `rows` rows
static inline int ev_pieces_per_row(int64_t lanes, int per) { return (int)((lanes + per - 1) / per); }
static inline int ev_piece_blocks(int64_t pieces) { return vol_blocks(pieces, 4); }

extern "C" int vg_mask_surface(const uint8_t* mask, int X, int Y, int Z, uint8_t* surf_or_null, uint8_t* not_surf_or_null, uint64_t* count,
                               vg_stream_t stream) {
    vg_begin();
    const int64_t n = ev_voxels(X, Y, Z);
    if (!mask || !count || n == 0 || (uintptr_t)count % 8 != 0) return VG_EINVAL;
    if ((surf_or_null && ev_overlap(surf_or_null, mask, n)) || (not_surf_or_null && ev_overlap(not_surf_or_null, mask, n))) return VG_EINVAL;
    if (surf_or_null && not_surf_or_null && ev_overlap(surf_or_null, not_surf_or_null, n)) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool wide = Z % 4 == 0 && (uintptr_t)mask % 4 == 0 && (uintptr_t)surf_or_null % 4 == 0 && (uintptr_t)not_surf_or_null % 4 == 0;
    const int np = ev_pieces_per_row(wide ? Z / 4 : Z, 62);
    const int64_t pieces = (int64_t)X * Y * np;
    if (hipMemsetAsync(count, 0, 8, s) != hipSuccess) return VG_ELAUNCH;
    if (wide) hipLaunchKernelGGL(ev_surface_kernel<4>, dim3(ev_piece_blocks(pieces)), dim3(256), 0, s, mask, pieces, np, X, Y, Z, surf_or_null, not_surf_or_null, (ev_u64*)count);
    else hipLaunchKernelGGL(ev_surface_kernel<1>, dim3(ev_piece_blocks(pieces)), dim3(256), 0, s, mask, pieces, np, X, Y, Z, surf_or_null, not_surf_or_null, (ev_u64*)count);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ Euler characteristic
// The cells of the closed cubical complex of the foreground, each counted by the thread at its low corner.  Positions run over
// [0, X] x [0, Y] x [0, Z], one more than the voxels on every axis, so that the cells on the high faces of the volume have an owner.  With
// m(i, j, k) = the voxel at (x - i, y - j, z - k), 0 outside the volume, position (x, y, z) owns: the cube m(0,0,0); the three faces
// through its vertex, each the OR of the two voxels on its sides; the three edges from its vertex towards +x, +y, +z, each the OR of the
// four voxels around it; the vertex, the OR of all eight.  The same wave scheme: a wave reads the rows (x, y), (x - 1, y), (x, y - 1),
// (x - 1, y - 1) at its z, and the voxels at z - 1 come from the lane below (lane 0 is the halo, 63 lanes of payload).  W = 4 as above;
// the row has Z / 4 + 1 words, the last of them past the end: it is never loaded and holds position Z alone.
template <int W>
__global__ __launch_bounds__(256) void ev_euler_kernel(const uint8_t* __restrict__ mask, int64_t pieces, int np, int X, int Y, int Z,
                                                       ev_u64* __restrict__ cells) {
    __shared__ unsigned wsum[4][4];
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * 4;
    const int Y1 = Y + 1;
    unsigned cnt[4] = {0u, 0u, 0u, 0u};                             // vertices, edges, faces, cubes
    for (int64_t pi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); pi < pieces; pi += nw) {         // uniform over the wave
        const int64_t row = pi / np;
        const int x = (int)(row / Y1), y = (int)(row - (int64_t)x * Y1);
        const int z = ((int)(pi - row * np) * 63 - 1 + lane) * W;
        unsigned a = 0u, b = 0u, c = 0u, d = 0u;
        if (z >= 0 && z < Z) {
            const uint8_t* p = mask + ((int64_t)x * Y + y) * Z + z;         // only dereferenced where (x, y) is a voxel's
            if (x < X && y < Y) a = ev_load_nz<W>(p);
            if (x > 0 && y < Y) b = ev_load_nz<W>(p - (int64_t)Y * Z);
            if (x < X && y > 0) c = ev_load_nz<W>(p - Z);
            if (x > 0 && y > 0) d = ev_load_nz<W>(p - (int64_t)Y * Z - Z);
        }
        const unsigned pa = __shfl_up(a, 1), pb = __shfl_up(b, 1), pc = __shfl_up(c, 1), pd = __shfl_up(d, 1);
        if (lane >= 1) {                                            // a position past Z sees no voxel and counts nothing
            const unsigned a1 = W == 4 ? (a << 8) | (pa >> 24) : pa, b1 = W == 4 ? (b << 8) | (pb >> 24) : pb;
            const unsigned c1 = W == 4 ? (c << 8) | (pc >> 24) : pc, d1 = W == 4 ? (d << 8) | (pd >> 24) : pd;
            const unsigned ab = a | b, ac = a | c, all = ab | c | d, ab1 = a1 | b1, ac1 = a1 | c1, all1 = ab1 | c1 | d1;
            cnt[3] += __popc(a);
            cnt[2] += __popc(ab) + __popc(ac) + __popc(a | a1);
            cnt[1] += __popc(ac | ac1) + __popc(ab | ab1) + __popc(all);
            cnt[0] += __popc(all | all1);
        }
    }
    const ev_u64 s = ev_block_sums<4>(cnt, wsum);
    const int t = threadIdx.x;
    if (t < 4 && s) atomicAdd(&cells[t], s);
    if (t == 4) {
        ev_u64 k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = (ev_u64)wsum[0][j] + wsum[1][j] + wsum[2][j] + wsum[3][j];
        const ev_u64 chi = k[0] - k[1] + k[2] - k[3];               // modulo 2^64: the sum over the workgroups is the signed value
        if (chi) atomicAdd(&cells[4], chi);
    }
}

extern "C" int vg_euler_characteristic(const uint8_t* mask, int X, int Y, int Z, int64_t* cells5, vg_stream_t stream) {
    vg_begin();
    const int64_t n = ev_voxels(X, Y, Z);
    if (!mask || !cells5 || n == 0 || (uintptr_t)cells5 % 8 != 0) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const bool wide = Z % 4 == 0 && (uintptr_t)mask % 4 == 0;
    const int np = ev_pieces_per_row(wide ? Z / 4 + 1 : (int64_t)Z + 1, 63);
    const int64_t pieces = ((int64_t)X + 1) * ((int64_t)Y + 1) * np;
    if (hipMemsetAsync(cells5, 0, 40, s) != hipSuccess) return VG_ELAUNCH;
    if (wide) hipLaunchKernelGGL(ev_euler_kernel<4>, dim3(ev_piece_blocks(pieces)), dim3(256), 0, s, mask, pieces, np, X, Y, Z, (ev_u64*)cells5);
    else hipLaunchKernelGGL(ev_euler_kernel<1>, dim3(ev_piece_blocks(pieces)), dim3(256), 0, s, mask, pieces, np, X, Y, Z, (ev_u64*)cells5);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ labels that reach no face
// flags: what vg_fill_holes_mark wrote, a byte per label.  K comes from result4[0] on the device and is capped by the labels the flags
// have room for, so no value of it makes a read leave the buffer.
__global__ __launch_bounds__(256) void ev_flags_count_kernel(const uint8_t* __restrict__ flags, const unsigned* __restrict__ result4, int64_t cap,
                                                             unsigned* __restrict__ out) {
    __shared__ unsigned wsum[4][1];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    int64_t K = (int64_t)result4[0];
    if (K > cap - 1) K = cap - 1;
    unsigned c[1] = {0u};
    for (int64_t l = 1 + tid; l <= K; l += nthr) c[0] += flags[l] == 0;
    const ev_u64 s = ev_block_sums<1>(c, wsum);
    if (threadIdx.x == 0 && s) atomicAdd(out, (unsigned)s);
}

extern "C" int vg_flags_count(const uint8_t* flags, const uint32_t* result4, int64_t n, uint32_t* out, vg_stream_t stream) {
    vg_begin();
    if (!flags || !result4 || !out || !ev_n_ok(n) || (uintptr_t)result4 % 4 != 0 || (uintptr_t)out % 4 != 0) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int64_t cap = n / 2 + 2;                                  // the bytes of flags
    if (hipMemsetAsync(out, 0, 4, s) != hipSuccess) return VG_ELAUNCH;
    hipLaunchKernelGGL(ev_flags_count_kernel, dim3(vol_blocks(cap)), dim3(256), 0, s, flags, result4, cap, out);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ statistics over the selected voxels
// scratch: psum[VOL_MAX_BLOCKS] fp64 | pcnt[VOL_MAX_BLOCKS] | pmax[VOL_MAX_BLOCKS] | the state of the radix select, in 32-bit words:
// hist[VG_EVAL_MAX_STATS][256] | prefix[VG_EVAL_MAX_STATS] (the key digits chosen so far) | rem[VG_EVAL_MAX_STATS] (the rank among the keys
// that share the prefix).  The select is that of vg_order_stats (vg_preproc.hip) on the raw bit patterns, restricted to sel != 0, with the
// ranks formed on the device from the selected count.  Kernel boundaries on the stream are the only synchronisation.
#define EV_HIST_WORDS (VG_EVAL_MAX_STATS * 256)
#define EV_STATE_WORDS (EV_HIST_WORDS + 2 * VG_EVAL_MAX_STATS)
#define EV_PART_BYTES ((int64_t)VOL_MAX_BLOCKS * 16)
struct ev_qs { double q[VG_EVAL_MAX_STATS]; };
struct ev_stats_out { ev_u64 m; unsigned max_key, pad; double sum; unsigned stat[VG_EVAL_MAX_STATS]; };      // VG_EVAL_STATS_BYTES
static_assert(sizeof(ev_stats_out) == VG_EVAL_STATS_BYTES, "the result block of vg_masked_stats");

template <int KIND>
__device__ __forceinline__ double ev_value(unsigned key) {
    return KIND == VG_EVAL_SQ_I32 ? __dsqrt_rn((double)key) : (double)__uint_as_float(key);
}

// Keys [head, head + 4 nv) go in 16-byte loads with a 32-bit load of their four selection bytes; head and tail one key a lane.  A thread
// adds its values in the order it meets them; the 256 threads are added by a fixed tree in LDS; the workgroup's sum, count and maximum go
// to slot blockIdx.x of the scratch.
template <int KIND>
__global__ __launch_bounds__(256) void ev_stats_reduce_kernel(const unsigned* __restrict__ keys, const uint8_t* __restrict__ sel, int64_t n, int64_t head,
                                                              int64_t nv, double* __restrict__ psum, unsigned* __restrict__ pcnt, unsigned* __restrict__ pmax) {
    __shared__ double rs[256];
    __shared__ unsigned rc[256], rm[256];
    const int t = threadIdx.x;
    const int64_t tid = (int64_t)blockIdx.x * 256 + t, nthr = (int64_t)gridDim.x * 256;
    double sum = 0.0;
    unsigned cnt = 0u, mx = 0u;
    for (int64_t i = tid; i < nv; i += nthr) {
        const uint4 k = *(const uint4*)(keys + head + i * 4);
        const unsigned sw = *(const unsigned*)(sel + head + i * 4);
        const unsigned kj[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((sw >> (8 * j)) & 0xffu) { ++cnt; mx = kj[j] > mx ? kj[j] : mx; sum += ev_value<KIND>(kj[j]); }
    }
    const int64_t rest = n - nv * 4;
    for (int64_t e = tid; e < rest; e += nthr) {
        const int64_t i = e < head ? e : e + nv * 4;
        if (sel[i]) { const unsigned k = keys[i]; ++cnt; mx = k > mx ? k : mx; sum += ev_value<KIND>(k); }
    }
    rs[t] = sum; rc[t] = cnt; rm[t] = mx;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { rs[t] += rs[t + o]; rc[t] += rc[t + o]; rm[t] = rm[t + o] > rm[t] ? rm[t + o] : rm[t]; }
        __syncthreads();
    }
    if (t == 0) { psum[blockIdx.x] = rs[0]; pcnt[blockIdx.x] = rc[0]; pmax[blockIdx.x] = rm[0]; }
}

// One workgroup: thread t adds the partials t, t + 256, ... in ascending order, then the same tree.  Writes m, the maximum and the sum,
// clears the histograms and sets rank r = max(ceil(q[r] m) - 1, 0), the product rounded once and the ceiling exact, both in fp64.
__global__ __launch_bounds__(256) void ev_stats_final_kernel(const double* __restrict__ psum, const unsigned* __restrict__ pcnt, const unsigned* __restrict__ pmax,
                                                             int nb, ev_qs qs, int R, unsigned* __restrict__ st, ev_stats_out* __restrict__ out) {
    __shared__ double rs[256];
    __shared__ ev_u64 rc[256];
    __shared__ unsigned rm[256];
    const int t = threadIdx.x;
    double sum = 0.0;
    ev_u64 cnt = 0ull;
    unsigned mx = 0u;
    for (int b = t; b < nb; b += 256) { sum += psum[b]; cnt += pcnt[b]; mx = pmax[b] > mx ? pmax[b] : mx; }
    rs[t] = sum; rc[t] = cnt; rm[t] = mx;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) { rs[t] += rs[t + o]; rc[t] += rc[t + o]; rm[t] = rm[t + o] > rm[t] ? rm[t + o] : rm[t]; }
        __syncthreads();
    }
    for (int i = t; i < EV_HIST_WORDS; i += 256) st[i] = 0u;
    const ev_u64 m = rc[0];
    if (t == 0) { out->m = m; out->max_key = rm[0]; out->pad = 0u; out->sum = rs[0]; }
    if (t < VG_EVAL_MAX_STATS) {
        ev_u64 rank = 0ull;
        if (t < R && m > 0ull) {
            const double c = ceil(__dmul_rn(qs.q[t], (double)m));   // 0 < q <= 1 and m < 2^31: 0 <= c <= m
            rank = c >= 1.0 ? (ev_u64)c - 1ull : 0ull;
            if (rank > m - 1ull) rank = m - 1ull;
        }
        st[EV_HIST_WORDS + t] = 0u;
        st[EV_HIST_WORDS + VG_EVAL_MAX_STATS + t] = (unsigned)rank;
        out->stat[t] = 0u;                                          // what m == 0 leaves: no pass finds a digit
    }
}

// Ranks whose prefixes are equal so far count the same keys: only the first of them (src[r] == r) is counted, the others read its row.
__device__ __forceinline__ void ev_load_state(const unsigned* __restrict__ st, int R, unsigned* pre, int* src) {
#pragma unroll
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r) {
        pre[r] = r < R ? st[EV_HIST_WORDS + r] : 0u;
        src[r] = r;
#pragma unroll
        for (int p = r - 1; p >= 0; --p) if (pre[p] == pre[r]) src[r] = p;
    }
}

__device__ __forceinline__ void ev_count(unsigned (*h)[256], unsigned key, int R, int shift, unsigned mask, const unsigned* pre, const int* src) {
    const unsigned d = (key >> shift) & 255u;
#pragma unroll
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r)
        if (r < R && src[r] == r && ((key ^ pre[r]) & mask) == 0u) atomicAdd(&h[r][d], 1u);
}

// Histogram of digit (key >> shift) & 255 over the selected keys whose higher digits equal the rank's prefix: LDS counters per workgroup,
// non-zero bins flushed with integer atomics (at most R * 256 per workgroup).
__global__ __launch_bounds__(256) void ev_hist_kernel(const unsigned* __restrict__ keys, const uint8_t* __restrict__ sel, int64_t n, int64_t head, int64_t nv,
                                                      int R, int shift, unsigned* __restrict__ st) {
    __shared__ unsigned h[VG_EVAL_MAX_STATS][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r) h[r][t] = 0u;
    unsigned pre[VG_EVAL_MAX_STATS]; int src[VG_EVAL_MAX_STATS];
    ev_load_state(st, R, pre, src);
    const unsigned mask = shift >= 24 ? 0u : 0xffffffffu << (shift + 8);
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * 256 + t, nthr = (int64_t)gridDim.x * 256;
    for (int64_t i = tid; i < nv; i += nthr) {
        const unsigned sw = *(const unsigned*)(sel + head + i * 4);
        if (sw == 0u) continue;
        const uint4 k = *(const uint4*)(keys + head + i * 4);
        const unsigned kj[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((sw >> (8 * j)) & 0xffu) ev_count(h, kj[j], R, shift, mask, pre, src);
    }
    const int64_t rest = n - nv * 4;
    for (int64_t e = tid; e < rest; e += nthr) {
        const int64_t i = e < head ? e : e + nv * 4;
        if (sel[i]) ev_count(h, keys[i], R, shift, mask, pre, src);
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) { const unsigned c = h[r][t]; if (c) atomicAdd(&st[r * 256 + t], c); }
}

// One workgroup, thread t = bin t.  Per rank: exclusive scan of the 256 counts; the one bin with excl <= rem < excl + count is the next
// digit.  Everything is read before anything is written (first barrier); the histogram is cleared for the next pass.  After the last
// digit (shift == 0) the prefix is the whole key of the selected value.
__global__ __launch_bounds__(256) void ev_scan_kernel(unsigned* __restrict__ st, int R, int shift, ev_stats_out* __restrict__ out) {
    __shared__ unsigned wsum[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    unsigned pre[VG_EVAL_MAX_STATS], rem[VG_EVAL_MAX_STATS], c[VG_EVAL_MAX_STATS]; int src[VG_EVAL_MAX_STATS];
    ev_load_state(st, R, pre, src);
#pragma unroll
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r) {
        rem[r] = r < R ? st[EV_HIST_WORDS + VG_EVAL_MAX_STATS + r] : 0u;
        c[r] = 0u;
    }
#pragma unroll
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r)
#pragma unroll
        for (int p = 0; p <= r; ++p) if (r < R && src[r] == p) c[r] = st[p * 256 + t];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r) st[r * 256 + t] = 0u;
#pragma unroll
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r) {
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
            st[EV_HIST_WORDS + r] = np;
            st[EV_HIST_WORDS + VG_EVAL_MAX_STATS + r] = rem[r] - excl;
            if (shift == 0) out->stat[r] = np;
        }
        __syncthreads();
    }
}

extern "C" int64_t vg_masked_stats_scratch_bytes(int64_t n, int R) {
    if (!ev_n_ok(n) || R < 1 || R > VG_EVAL_MAX_STATS) return VG_EINVAL;
    return EV_PART_BYTES + (int64_t)EV_STATE_WORDS * 4;
}

extern "C" int vg_masked_stats(const void* keys, const uint8_t* sel, int64_t n, int kind, const double* q_host, int R, void* out, void* scratch,
                               int64_t scratch_bytes, vg_stream_t stream) {
    vg_begin();
    if (!keys || !sel || !q_host || !out || !scratch || !ev_n_ok(n) || R < 1 || R > VG_EVAL_MAX_STATS) return VG_EINVAL;
    if (kind != VG_EVAL_SQ_I32 && kind != VG_EVAL_DIST_F32) return VG_EINVAL;
    if (scratch_bytes < vg_masked_stats_scratch_bytes(n, R) || (uintptr_t)scratch % 16 != 0 || (uintptr_t)keys % 4 != 0 || (uintptr_t)out % 8 != 0)
        return VG_EINVAL;
    ev_qs qs;
    for (int r = 0; r < VG_EVAL_MAX_STATS; ++r) {
        qs.q[r] = r < R ? q_host[r] : 1.0;
        if (!(qs.q[r] > 0.0 && qs.q[r] <= 1.0)) return VG_EINVAL;   // a NaN fails both
    }
    hipStream_t s = (hipStream_t)stream;
    int64_t head = (int64_t)((16 - (uintptr_t)keys % 16) % 16) / 4, nv = 0;
    if (((uintptr_t)sel + (uintptr_t)head) % 4 == 0 && head < n) nv = (n - head) / 4;
    if (nv == 0) head = 0;
    const unsigned* k = (const unsigned*)keys;
    double* psum = (double*)scratch;
    unsigned* pcnt = (unsigned*)((char*)scratch + (int64_t)VOL_MAX_BLOCKS * 8);
    unsigned* pmax = pcnt + VOL_MAX_BLOCKS;
    unsigned* st = (unsigned*)((char*)scratch + EV_PART_BYTES);
    ev_stats_out* o = (ev_stats_out*)out;
    const dim3 grid(vol_blocks(nv + (n - nv * 4))), block(256);
    if (kind == VG_EVAL_SQ_I32) hipLaunchKernelGGL(ev_stats_reduce_kernel<VG_EVAL_SQ_I32>, grid, block, 0, s, k, sel, n, head, nv, psum, pcnt, pmax);
    else hipLaunchKernelGGL(ev_stats_reduce_kernel<VG_EVAL_DIST_F32>, grid, block, 0, s, k, sel, n, head, nv, psum, pcnt, pmax);
    hipLaunchKernelGGL(ev_stats_final_kernel, dim3(1), block, 0, s, psum, pcnt, pmax, (int)grid.x, qs, R, st, o);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(ev_hist_kernel, grid, block, 0, s, k, sel, n, head, nv, R, shift, st);
        hipLaunchKernelGGL(ev_scan_kernel, dim3(1), block, 0, s, st, R, shift, o);
    }
    return vg_check_launch();
}
