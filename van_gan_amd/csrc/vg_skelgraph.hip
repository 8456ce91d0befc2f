// vg_skelgraph.hip -- the graph of a vessel skeleton (van_gan_amd/postprocess.py skeleton_graph, prune_spurs, network_summary,
// vessel_graph; include/vangan_hip.h "The vessel graph"): the voxels of a uint8 mask split by their 26-neighbour count
// into segment voxels (count 2) and node voxels (every other count), and -- once vg_cc_label (csrc/vg_components.hip) has numbered the
// 26-components of both classes -- the tables of the segments (voxels, half-steps per step class, the two attachments, length, chord,
// radius) and of the nodes (voxels, attachments, kind, centroid), and the removal of short terminal spurs.  Nothing here depends on the
// 16-bit storage format of the build.  256-thread workgroups (4 wave64) on a one-dimensional grid; no LDS, no workgroup barrier, no loop
// that waits on another thread.  Only integer atomics, every one of them a sum, a minimum or a maximum of integers: the tables do not
// depend on their order.  Every floating-point result is computed once, by one thread, from those integers, each operation rounded on
// its own: contraction into fused multiply-adds is switched off for the whole file, host and device.
#include "vg_volume.h"
#include <cmath>

#pragma clang fp contract(off)

typedef unsigned long long sg_u64;

static inline int64_t sg_al16(int64_t b) { return (b + 15) & ~(int64_t)15; }
// n = X * Y * Z where the shape is served (extents >= 1, n < 2^31), else 0
static inline int64_t sg_voxels(int X, int Y, int Z) {
    if (X < 1 || Y < 1 || Z < 1) return 0;
    if ((int64_t)X * Y >= ((int64_t)1 << 31)) return 0;                    // so that the product below cannot overflow
    const int64_t n = (int64_t)X * Y * Z;
    return n < ((int64_t)1 << 31) ? n : 0;
}
// 0 <= count <= n / 2 + 1: the labels vg_cc_label can hand out for a volume of n voxels
static inline bool sg_count_ok(int c, int64_t n) { return c >= 0 && (int64_t)c <= n / 2 + 1; }

// the lengths of the seven step classes c = 4 |dx| + 2 |dy| + |dz| - 1 and what the fixed point of the radius needs, from the shape and
// the sampling alone
struct sg_metric {
    double s[3];                            // the voxel spacing along X, Y, Z
    double l[7];                            // l[c] = sqrt((|dx| sx)^2 + (|dy| sy)^2 + (|dz| sz)^2)
    double D;                               // the diagonal of the volume: no radius is above it
    double scale, inv_scale;                // 2^k and 2^-k
};

static inline int sg_ceil_log2_i(int64_t n) {                               // n >= 1
    int b = 0;
    while (((int64_t)1 << b) < n) ++b;
    return b;
}
static inline int sg_ceil_log2_d(double d) {                                // d > 0, finite
    int e;
    const double m = frexp(d, &e);                                          // d = m 2^e, 0.5 <= m < 1
    return m > 0.5 ? e : e - 1;
}

static bool sg_metric_of(const double* sampling3_or_null, int X, int Y, int Z, sg_metric* m) {
    for (int a = 0; a < 3; ++a) {
        m->s[a] = sampling3_or_null ? sampling3_or_null[a] : 1.0;
        if (!(m->s[a] > 0.0) || !std::isfinite(m->s[a])) return false;
    }
    for (int c = 0; c < 7; ++c) {
        const double ax = ((c + 1) >> 2 & 1) * m->s[0], ay = ((c + 1) >> 1 & 1) * m->s[1], az = ((c + 1) & 1) * m->s[2];
        m->l[c] = sqrt(ax * ax + ay * ay + az * az);
    }
    const double ex = X * m->s[0], ey = Y * m->s[1], ez = Z * m->s[2];
    m->D = sqrt(ex * ex + ey * ey + ez * ez);
    if (!(m->D > 0.0) || !std::isfinite(m->D)) return false;
    const int k = 62 - sg_ceil_log2_i((int64_t)X * Y * Z) - sg_ceil_log2_d(m->D);
    if (k < -1000 || k > 1000) return false;
    m->scale = ldexp(1.0, k);
    m->inv_scale = ldexp(1.0, -k);
    return true;
}

// ------------------------------------------------------------------------------------------------ classify
// The wave scheme of sk_degree_kernel (vg_skeleton.hip): one wave per (row, piece of 62 lanes' worth of z), lanes 0 and 63 the halo;
// every lane sums the nine rows around at its z, the sums of z - 1 and z + 1 come from the neighbouring lanes.  W = 4: a lane holds four
// consecutive voxels in one 32-bit word, a byte each, and all the arithmetic stays packed (no byte ever exceeds 27); it needs Z % 4 == 0
// and 4-byte aligned pointers, so that every word lies in one row.  W = 1: a byte per lane, any Z.
__device__ __forceinline__ unsigned sg_nonzero4(unsigned x) { return ((x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u; }

template <int W>
__global__ __launch_bounds__(256) void sg_classify_kernel(const uint8_t* __restrict__ mask, int64_t pieces, int np, int X, int Y, int Z,
                                                          uint8_t* __restrict__ deg, uint8_t* __restrict__ bm, uint8_t* __restrict__ nm) {
    const int lane = threadIdx.x & 63;
    const int64_t pi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= pieces) return;                                       // the whole wave leaves
    const int64_t row = pi / np;
    const int x = (int)(row / Y), y = (int)(row - (int64_t)x * Y);
    const int z = ((int)(pi - row * np) * 62 - 1 + lane) * W;
    const bool inz = z >= 0 && z < Z;
    unsigned s = 0, self = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int xx = x + i / 3 - 1, yy = y + i % 3 - 1;
        if (inz && xx >= 0 && xx < X && yy >= 0 && yy < Y) {
            const uint8_t* p = mask + ((int64_t)xx * Y + yy) * Z + z;
            const unsigned v = W == 4 ? sg_nonzero4(*(const unsigned*)p) : (unsigned)(*p != 0);
            s += v;
            if (i == 4) self = v;
        }
    }
    const unsigned below = __shfl_up(s, 1), above = __shfl_down(s, 1);
    if (lane < 1 || lane > 62 || !inz) return;
    const int64_t o = row * Z + z;
    if (W == 4) {
        const unsigned tot = s + ((s << 8) | (below >> 24)) + ((s >> 8) | (above << 24));
        const unsigned d = (tot - self) & (self * 0xffu);
        const unsigned t = d ^ 0x02020202u;
        const unsigned b = (~(((t & 0x7f7f7f7fu) + 0x7f7f7f7fu) | t) >> 7) & 0x01010101u & self;      // the bytes of d that are 2
        *(unsigned*)(deg + o) = d;
        *(unsigned*)(bm + o) = b;
        *(unsigned*)(nm + o) = self ^ b;
    } else {
        const unsigned d = self ? s + below + above - 1 : 0u;
        const unsigned b = self && d == 2u;
        deg[o] = (uint8_t)d;
        bm[o] = (uint8_t)b;
        nm[o] = (uint8_t)(self ^ b);
    }
}

// ------------------------------------------------------------------------------------------------ accumulate
// What the per-voxel pass adds into, all in the scratch: E1 = E + 1 rows per segment array, V1 = V + 1 per node array, row 0 unused.
struct sg_acc {
    long long* half;                        // [E1][7]
    sg_u64* kmax;                           // [E1]  the largest attachment key (p << 32) | q
    long long* rsum;                        // [E1]  sum of llrint(r 2^k)
    sg_u64* csum;                           // [V1][3]  coordinate sums
    int* seg_vox;                           // [E1]
    unsigned* rmax;                         // [E1]  largest radius, as its bit pattern (radii are >= 0)
    int* node_vox;                          // [V1]
    int* node_deg;                          // [V1]  attachments
    unsigned* tips;                         // [V1]  voxels of degree 0, + 65536 per voxel of degree 1
    unsigned* bad;                          // [4]   (voxels with an unusable radius, labels out of range, 0, 0)
    sg_u64* kmin;                           // [E1]  the smallest attachment key; starts as all ones
    unsigned* rmin;                         // [E1]  smallest radius; starts as all ones
};

static inline int64_t sg_zero_bytes(int E, int V) { return sg_al16(80 * ((int64_t)E + 1) + 36 * ((int64_t)V + 1) + 16); }
static inline int64_t sg_ones_bytes(int E) { return sg_al16(12 * ((int64_t)E + 1)); }

static sg_acc sg_carve(void* scratch, int E, int V) {
    const int64_t E1 = (int64_t)E + 1, V1 = (int64_t)V + 1;
    sg_acc a;
    char* p = (char*)scratch;
    a.half = (long long*)p;      p += 56 * E1;
    a.kmax = (sg_u64*)p;         p += 8 * E1;
    a.rsum = (long long*)p;      p += 8 * E1;
    a.csum = (sg_u64*)p;         p += 24 * V1;
    a.seg_vox = (int*)p;         p += 4 * E1;
    a.rmax = (unsigned*)p;       p += 4 * E1;
    a.node_vox = (int*)p;        p += 4 * V1;
    a.node_deg = (int*)p;        p += 4 * V1;
    a.tips = (unsigned*)p;       p += 4 * V1;
    a.bad = (unsigned*)p;
    p = (char*)scratch + sg_zero_bytes(E, V);
    a.kmin = (sg_u64*)p;         p += 8 * E1;
    a.rmin = (unsigned*)p;
    return a;
}

__device__ __forceinline__ unsigned sg_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ sg_u64 sg_wave_sum64(sg_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned sg_wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned sg_wave_max(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor(v, o));
    return v;
}

// the seven 9-bit fields of a packed half-step count (a wave adds at most 64 voxels x 2 neighbours x 2 to a field)
__device__ __forceinline__ void sg_add_half(long long* row, sg_u64 packed) {
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const unsigned h = (unsigned)(packed >> (9 * c)) & 511u;
        if (h) atomicAdd((sg_u64*)(row + c), (sg_u64)h);
    }
}

// One thread per voxel; a wave without foreground leaves after its one load.  Lanes run along z: where every segment voxel of the wave
// lies in one segment (a vessel along z), the wave adds its lanes up first and one lane issues the atomics; likewise for the node
// voxels of a wave that lie in one node (a solid block).  Otherwise every lane issues its own.  A label outside 1 .. E (1 .. V) is
// counted in bad[1] and never used as an index.
__global__ __launch_bounds__(256) void sg_accumulate_kernel(const uint8_t* __restrict__ skel, const uint8_t* __restrict__ deg, const int* __restrict__ seg,
                                                            const int* __restrict__ node, const float* __restrict__ radius, int64_t n, int X, int Y, int Z,
                                                            int E, int V, double scale, double D, sg_acc a) {
    const int lane = threadIdx.x & 63;
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool fg = v < n && skel[v] != 0;
    if (__builtin_amdgcn_ballot_w64(fg) == 0ull) return;            // the whole wave leaves
    int e = 0, nd = 0, x = 0, y = 0, z = 0;
    unsigned wrong = 0;
    if (fg) {
        e = seg[v];
        if (e == 0) nd = node[v];
        if ((unsigned)e > (unsigned)E) { e = 0; ++wrong; }
        if ((unsigned)nd > (unsigned)V) { nd = 0; ++wrong; }
        const int64_t row = v / Z;
        z = (int)(v - row * Z);
        x = (int)(row / Y);
        y = (int)(row - (int64_t)x * Y);
    }
    // ---- a segment voxel: its half-steps, its attachments, its radius
    sg_u64 packed = 0;
    long long rq = 0;
    unsigned rbits_lo = 0xffffffffu, rbits_hi = 0u, rbad = 0;
    if (e) {
        for (int dx = -1; dx <= 1; ++dx) {
            if ((unsigned)(x + dx) >= (unsigned)X) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                if ((unsigned)(y + dy) >= (unsigned)Y) continue;
#pragma unroll
                for (int dz = -1; dz <= 1; ++dz) {
                    if ((unsigned)(z + dz) >= (unsigned)Z || (dx == 0 && dy == 0 && dz == 0)) continue;
                    const int64_t q = v + ((int64_t)dx * Y + dy) * Z + dz;
                    const int c = 4 * (dx != 0) + 2 * (dy != 0) + (dz != 0) - 1;
                    if (seg[q] != 0) {
                        packed += (sg_u64)1 << (9 * c);
                    } else {
                        const int nq = node[q];
                        if (nq == 0) continue;
                        packed += (sg_u64)2 << (9 * c);
                        const sg_u64 key = ((sg_u64)v << 32) | (sg_u64)q;
                        atomicMin(a.kmin + e, key);
                        atomicMax(a.kmax + e, key);
                        if ((unsigned)nq <= (unsigned)V) atomicAdd(a.node_deg + nq, 1);
                        else ++wrong;
                    }
                }
            }
        }
        if (radius) {
            float r = radius[v];
            if (r == 0.0f) r = 0.0f;                                // -0 is 0: the bit pattern below is that of a value >= 0
            if (r >= 0.0f && (double)r <= D) {                      // false for a NaN
                rq = llrint((double)r * scale);                     // exact product: fp32 times a power of two
                rbits_lo = rbits_hi = __float_as_uint(r);
            } else {
                rbad = 1;
            }
        }
    }
    const sg_u64 mB = __builtin_amdgcn_ballot_w64(e != 0);
    if (mB) {
        const int first = __builtin_ctzll(mB);
        const int e0 = __shfl(e, first);
        const bool one = __builtin_amdgcn_ballot_w64(e != 0 && e != e0) == 0ull && (mB & (mB - 1)) != 0ull;
        if (one) {
            const sg_u64 psum = sg_wave_sum64(packed);
            sg_u64 rs = 0;
            unsigned lo = 0xffffffffu, hi = 0u;
            if (radius) {
                rs = sg_wave_sum64((sg_u64)rq);
                lo = sg_wave_min(rbits_lo);
                hi = sg_wave_max(rbits_hi);
            }
            if (lane == first) {
                sg_add_half(a.half + (int64_t)e0 * 7, psum);
                atomicAdd(a.seg_vox + e0, __builtin_popcountll(mB));
                if (radius) {
                    if (rs) atomicAdd((sg_u64*)(a.rsum + e0), rs);
                    atomicMin(a.rmin + e0, lo);
                    atomicMax(a.rmax + e0, hi);
                }
            }
        } else if (e) {
            sg_add_half(a.half + (int64_t)e * 7, packed);
            atomicAdd(a.seg_vox + e, 1);
            if (radius) {
                if (rq) atomicAdd((sg_u64*)(a.rsum + e), (sg_u64)rq);
                atomicMin(a.rmin + e, rbits_lo);
                atomicMax(a.rmax + e, rbits_hi);
            }
        }
    }
    // ---- a node voxel: one voxel, its degree class, its coordinates
    const sg_u64 mN = __builtin_amdgcn_ballot_w64(nd != 0);
    if (mN) {
        const unsigned d = nd ? deg[v] : 0u;
        const unsigned tip = nd ? (d == 0u ? 1u : d == 1u ? 65536u : 0u) : 0u;
        const int first = __builtin_ctzll(mN);
        const int n0 = __shfl(nd, first);
        const bool one = __builtin_amdgcn_ballot_w64(nd != 0 && nd != n0) == 0ull && (mN & (mN - 1)) != 0ull;
        if (one) {
            const unsigned tsum = sg_wave_sum(tip);
            const sg_u64 sx = sg_wave_sum64(nd ? (sg_u64)x : 0ull), sy = sg_wave_sum64(nd ? (sg_u64)y : 0ull), sz = sg_wave_sum64(nd ? (sg_u64)z : 0ull);
            if (lane == first) {
                atomicAdd(a.node_vox + n0, __builtin_popcountll(mN));
                if (tsum) atomicAdd(a.tips + n0, tsum);
                atomicAdd(a.csum + (int64_t)n0 * 3, sx);
                atomicAdd(a.csum + (int64_t)n0 * 3 + 1, sy);
                atomicAdd(a.csum + (int64_t)n0 * 3 + 2, sz);
            }
        } else if (nd) {
            atomicAdd(a.node_vox + nd, 1);
            if (tip) atomicAdd(a.tips + nd, tip);
            atomicAdd(a.csum + (int64_t)nd * 3, (sg_u64)x);
            atomicAdd(a.csum + (int64_t)nd * 3 + 1, (sg_u64)y);
            atomicAdd(a.csum + (int64_t)nd * 3 + 2, (sg_u64)z);
        }
    }
    const unsigned nbad = sg_wave_sum(rbad), nwrong = sg_wave_sum(wrong);
    if (lane == 0) {
        if (nbad) atomicAdd(a.bad, nbad);
        if (nwrong) atomicAdd(a.bad + 1, nwrong);
    }
}

// ------------------------------------------------------------------------------------------------ finalise
struct sg_out {
    long long* half;                        // [E1][7]
    int* seg_vox;                           // [E1]
    long long* seg_ends;                    // [E1][2]
    int* seg_nodes;                         // [E1][2]
    double* seg_length;                     // [E1]
    double* seg_chord;                      // [E1]
    double* seg_rmean;                      // [E1] or NULL
    float* seg_rminmax;                     // [E1][2] or NULL
    int* node_vox;                          // [V1]
    int* node_deg;                          // [V1]
    uint8_t* node_kind;                     // [V1]
    double* node_centroid;                  // [V1][3]
    unsigned* bad2;
};

// (sum over c of half[c] l[c]) / 2, left to right, every operation rounded on its own
__device__ __forceinline__ double sg_length(const long long* h, const sg_metric& m) {
    double acc = (double)h[0] * m.l[0];
#pragma unroll
    for (int c = 1; c < 7; ++c) acc = acc + (double)h[c] * m.l[c];
    return acc / 2.0;
}

// thread t: the segment t for t <= E, the node t - E - 1 beyond; row 0 of every table is written as zeros
__global__ __launch_bounds__(256) void sg_finalise_kernel(const int* __restrict__ node, int64_t n, int Y, int Z, int E, int V, sg_metric m, sg_acc a, sg_out o) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) {
        o.bad2[0] = a.bad[0];
        o.bad2[1] = a.bad[1];
    }
    if (t <= E) {
        const int64_t e = t;
        long long h[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            h[c] = e ? a.half[e * 7 + c] : 0;
            o.half[e * 7 + c] = h[c];
        }
        const int vox = e ? a.seg_vox[e] : 0;
        o.seg_vox[e] = vox;
        const sg_u64 k0 = a.kmin[e], k1 = a.kmax[e];
        long long q0 = -1, q1 = -1;
        int n0 = 0, n1 = 0;
        double chord = 0.0;
        if (e == 0) {
            q0 = q1 = 0;
        } else if (k0 != ~0ull) {
            q0 = (long long)(k0 & 0xffffffffull);
            q1 = (long long)(k1 & 0xffffffffull);
            if (q0 < n && q1 < n) {
                n0 = node[q0];
                n1 = node[q1];
                if ((unsigned)n0 > (unsigned)V) n0 = 0;
                if ((unsigned)n1 > (unsigned)V) n1 = 0;
                const long long r0 = q0 / Z, r1 = q1 / Z;
                const double dx = (double)(r0 / Y - r1 / Y) * m.s[0], dy = (double)(r0 % Y - r1 % Y) * m.s[1], dz = (double)(q0 % Z - q1 % Z) * m.s[2];
                chord = sqrt(dx * dx + dy * dy + dz * dz);
            }
        }
        o.seg_ends[e * 2] = q0;
        o.seg_ends[e * 2 + 1] = q1;
        o.seg_nodes[e * 2] = n0;
        o.seg_nodes[e * 2 + 1] = n1;
        o.seg_length[e] = sg_length(h, m);
        o.seg_chord[e] = chord;
        if (o.seg_rmean) {
            const unsigned lo = a.rmin[e];
            const bool any = e != 0 && lo != 0xffffffffu && vox > 0;
            o.seg_rmean[e] = any ? (double)a.rsum[e] * m.inv_scale / (double)vox : 0.0;
            o.seg_rminmax[e * 2] = any ? __uint_as_float(lo) : 0.0f;
            o.seg_rminmax[e * 2 + 1] = any ? __uint_as_float(a.rmax[e]) : 0.0f;
        }
    } else if (t <= (int64_t)E + 1 + V) {
        const int64_t k = t - E - 1;
        const int vox = k ? a.node_vox[k] : 0;
        const unsigned tips = k ? a.tips[k] : 0u;
        o.node_vox[k] = vox;
        o.node_deg[k] = k ? a.node_deg[k] : 0;
        o.node_kind[k] = (uint8_t)(k == 0 ? 0 : vox == 1 ? ((tips & 0xffffu) ? 0 : (tips >> 16) ? 1 : 2) : 2);
#pragma unroll
        for (int c = 0; c < 3; ++c) o.node_centroid[k * 3 + c] = vox > 0 ? (double)a.csum[k * 3 + c] / (double)vox : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------ prune
// flags[e] = 1 where segment e is a spur: a path (two attachments) with exactly one of its two nodes an end point, shorter than
// min_length; counts[0] = the spurs
__global__ __launch_bounds__(256) void sg_flag_kernel(const long long* __restrict__ half, const int* __restrict__ seg_nodes, const uint8_t* __restrict__ kind,
                                                      int E, int V, double min_length, sg_metric m, uint8_t* __restrict__ flags, unsigned* counts) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e > E) return;
    bool spur = false;
    if (e > 0) {
        const int n0 = seg_nodes[e * 2], n1 = seg_nodes[e * 2 + 1];
        if (n0 >= 1 && n0 <= V && n1 >= 1 && n1 <= V) {
            long long h[7];
#pragma unroll
            for (int c = 0; c < 7; ++c) h[c] = half[e * 7 + c];
            spur = ((kind[n0] == 1) != (kind[n1] == 1)) && sg_length(h, m) < min_length;
        }
    }
    flags[e] = (uint8_t)spur;
    if (spur) atomicAdd(counts, 1u);
}

// out = the mask without the voxels of the flagged segments and without the end voxels they hang from; counts[1] = voxels deleted
__global__ __launch_bounds__(256) void sg_apply_kernel(const uint8_t* __restrict__ skel, const uint8_t* __restrict__ deg, const int* __restrict__ seg,
                                                       const int* __restrict__ node, const uint8_t* __restrict__ flags, int64_t n, int X, int Y, int Z, int E,
                                                       uint8_t* __restrict__ out, unsigned* counts) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool fg = v < n && skel[v] != 0;
    if (__builtin_amdgcn_ballot_w64(fg) == 0ull) {                  // the whole wave: background
        if (v < n) out[v] = 0;
        return;
    }
    bool del = false;
    if (fg) {
        const int e = seg[v];
        if (e != 0) {
            del = (unsigned)e <= (unsigned)E && flags[e] != 0;
        } else if (deg[v] == 1) {                                   // an end voxel: it goes with the spur that is its one neighbour
            const int64_t row = v / Z;
            const int z = (int)(v - row * Z), x = (int)(row / Y), y = (int)(row - (int64_t)x * Y);
            for (int dx = -1; dx <= 1; ++dx) {
                if ((unsigned)(x + dx) >= (unsigned)X) continue;
                for (int dy = -1; dy <= 1; ++dy) {
                    if ((unsigned)(y + dy) >= (unsigned)Y) continue;
#pragma unroll
                    for (int dz = -1; dz <= 1; ++dz) {
                        if ((unsigned)(z + dz) >= (unsigned)Z || (dx == 0 && dy == 0 && dz == 0)) continue;
                        const int eq = seg[v + ((int64_t)dx * Y + dy) * Z + dz];
                        if (eq != 0 && (unsigned)eq <= (unsigned)E && flags[eq] != 0) del = true;
                    }
                }
            }
        }
    }
    if (v < n) out[v] = (uint8_t)(fg && !del);
    const unsigned cnt = (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(del));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(counts + 1, cnt);
}

// ------------------------------------------------------------------------------------------------ entries
extern "C" int vg_skelgraph_classify(const uint8_t* skel, int X, int Y, int Z, uint8_t* degree, uint8_t* segment_mask, uint8_t* node_mask, vg_stream_t stream) {
    vg_begin();
    if (!skel || !degree || !segment_mask || !node_mask || !sg_voxels(X, Y, Z)) return VG_EINVAL;
    const bool wide = Z % 4 == 0 && ((uintptr_t)skel | (uintptr_t)degree | (uintptr_t)segment_mask | (uintptr_t)node_mask) % 4 == 0;
    const int per = wide ? 4 * 62 : 62;
    const int np = (Z + per - 1) / per;
    const int64_t pieces = (int64_t)X * Y * np;                     // <= n < 2^31
    const dim3 grid((unsigned)((pieces + 3) / 4));
    if (wide) hipLaunchKernelGGL(sg_classify_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, skel, pieces, np, X, Y, Z, degree, segment_mask, node_mask);
    else hipLaunchKernelGGL(sg_classify_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, skel, pieces, np, X, Y, Z, degree, segment_mask, node_mask);
    return vg_check_launch();
}

extern "C" int64_t vg_skelgraph_scratch_bytes(int E, int V) {
    if (E < 0 || V < 0 || E > (1 << 30) || V > (1 << 30)) return VG_EINVAL;
    return sg_zero_bytes(E, V) + sg_ones_bytes(E);
}

extern "C" int vg_skelgraph_tables(const uint8_t* skel, const uint8_t* degree, const int32_t* segment_labels, const int32_t* node_labels,
                                   const float* radius_or_null, int X, int Y, int Z, int E, int V, const double* sampling3_or_null,
                                   int64_t* seg_half_steps, int32_t* seg_voxels, int64_t* seg_ends, int32_t* seg_nodes, double* seg_length, double* seg_chord,
                                   double* seg_radius_mean_or_null, float* seg_radius_minmax_or_null, int32_t* node_voxels, int32_t* node_degree,
                                   uint8_t* node_kind, double* node_centroid, uint32_t* bad2, void* scratch, int64_t scratch_bytes, vg_stream_t stream) {
    vg_begin();
    const int64_t n = sg_voxels(X, Y, Z);
    if (!skel || !degree || !segment_labels || !node_labels || !n || !sg_count_ok(E, n) || !sg_count_ok(V, n)) return VG_EINVAL;
    if (!seg_half_steps || !seg_voxels || !seg_ends || !seg_nodes || !seg_length || !seg_chord || !node_voxels || !node_degree || !node_kind || !node_centroid ||
        !bad2 || !scratch)
        return VG_EINVAL;
    if ((radius_or_null != nullptr) != (seg_radius_mean_or_null != nullptr) || (radius_or_null != nullptr) != (seg_radius_minmax_or_null != nullptr)) return VG_EINVAL;
    if (((uintptr_t)seg_half_steps | (uintptr_t)seg_ends | (uintptr_t)seg_length | (uintptr_t)seg_chord | (uintptr_t)seg_radius_mean_or_null |
         (uintptr_t)node_centroid) % 8 != 0)
        return VG_EINVAL;
    if (((uintptr_t)segment_labels | (uintptr_t)node_labels | (uintptr_t)radius_or_null | (uintptr_t)seg_voxels | (uintptr_t)seg_nodes |
         (uintptr_t)seg_radius_minmax_or_null | (uintptr_t)node_voxels | (uintptr_t)node_degree | (uintptr_t)bad2) % 4 != 0)
        return VG_EINVAL;
    if ((uintptr_t)scratch % 16 != 0 || scratch_bytes < vg_skelgraph_scratch_bytes(E, V)) return VG_EINVAL;
    sg_metric m;
    if (!sg_metric_of(sampling3_or_null, X, Y, Z, &m)) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const sg_acc a = sg_carve(scratch, E, V);
    if (hipMemsetAsync(scratch, 0, (size_t)sg_zero_bytes(E, V), s) != hipSuccess) return VG_ELAUNCH;
    if (hipMemsetAsync((char*)scratch + sg_zero_bytes(E, V), 0xff, (size_t)sg_ones_bytes(E), s) != hipSuccess) return VG_ELAUNCH;
    hipLaunchKernelGGL(sg_accumulate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, skel, degree, (const int*)segment_labels, (const int*)node_labels,
                       radius_or_null, n, X, Y, Z, E, V, m.scale, m.D, a);
    sg_out o;
    o.half = (long long*)seg_half_steps;
    o.seg_vox = seg_voxels;
    o.seg_ends = (long long*)seg_ends;
    o.seg_nodes = seg_nodes;
    o.seg_length = seg_length;
    o.seg_chord = seg_chord;
    o.seg_rmean = seg_radius_mean_or_null;
    o.seg_rminmax = seg_radius_minmax_or_null;
    o.node_vox = node_voxels;
    o.node_deg = node_degree;
    o.node_kind = node_kind;
    o.node_centroid = node_centroid;
    o.bad2 = bad2;
    const int64_t rows = (int64_t)E + V + 2;
    hipLaunchKernelGGL(sg_finalise_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, (const int*)node_labels, n, Y, Z, E, V, m, a, o);
    return vg_check_launch();
}

extern "C" int vg_skelgraph_prune(const uint8_t* skel, const uint8_t* degree, const int32_t* segment_labels, const int32_t* node_labels, int X, int Y, int Z,
                                  int E, int V, const int64_t* seg_half_steps, const int32_t* seg_nodes, const uint8_t* node_kind, double min_length,
                                  const double* sampling3_or_null, uint8_t* flags, uint8_t* out, uint32_t* counts2, vg_stream_t stream) {
    vg_begin();
    const int64_t n = sg_voxels(X, Y, Z);
    if (!skel || !degree || !segment_labels || !node_labels || !n || !sg_count_ok(E, n) || !sg_count_ok(V, n)) return VG_EINVAL;
    if (!seg_half_steps || !seg_nodes || !node_kind || !flags || !out || !counts2 || min_length != min_length) return VG_EINVAL;
    if ((uintptr_t)seg_half_steps % 8 != 0 || ((uintptr_t)segment_labels | (uintptr_t)node_labels | (uintptr_t)seg_nodes | (uintptr_t)counts2) % 4 != 0)
        return VG_EINVAL;
    sg_metric m;
    if (!sg_metric_of(sampling3_or_null, X, Y, Z, &m)) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts2, 0, 8, s) != hipSuccess) return VG_ELAUNCH;
    hipLaunchKernelGGL(sg_flag_kernel, dim3((unsigned)(((int64_t)E + 256) / 256)), dim3(256), 0, s, (const long long*)seg_half_steps, (const int*)seg_nodes, node_kind, E,
                       V, min_length, m, flags, counts2);
    hipLaunchKernelGGL(sg_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, skel, degree, (const int*)segment_labels, (const int*)node_labels,
                       (const uint8_t*)flags, n, X, Y, Z, E, out, counts2);
    return vg_check_launch();
}
