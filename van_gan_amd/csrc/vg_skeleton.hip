// vg_skeleton.hip -- the centreline of a vessel mask (van_gan_amd/postprocess.py skeletonize, skeleton_nodes, vessel_centreline;
// include/vangan_hip.h "Prediction post-processing"): exact topological thinning of a uint8 mask by directional
// sub-iterations over eight parity subfields, and the 26-neighbour count of every foreground voxel.  Nothing here depends on the 16-bit
// storage format of the build.  256-thread workgroups (4 wave64) on a one-dimensional grid; no LDS, no workgroup barrier, no loop that
// waits on another thread: every loop is bounded by 64 bits of a word or by the 27 bits of a neighbourhood code.
//
// The thinning works on a bit-packed copy of the mask: word w of row (x, y) holds z = 64 w .. 64 w + 63, bit z & 63; nw = ceil(Z / 64)
// words per row, padding bits always 0, so "outside the volume is background" needs no test along z.  A second bit volume holds the
// marks of the current direction.
#include "vg_volume.h"

typedef unsigned long long sk_word;

static inline int64_t sk_al16(int64_t b) { return (b + 15) & ~(int64_t)15; }
static inline int sk_nw(int Z) { return (Z + 63) >> 6; }
// n = X * Y * Z where the shape is served (extents >= 1, n < 2^31), else 0
static inline int64_t sk_voxels(int X, int Y, int Z) {
    if (X < 1 || Y < 1 || Z < 1) return 0;
    if ((int64_t)X * Y >= ((int64_t)1 << 31)) return 0;                    // so that the product below cannot overflow
    const int64_t n = (int64_t)X * Y * Z;
    return n < ((int64_t)1 << 31) ? n : 0;
}
static inline int64_t sk_words(int X, int Y, int Z) { return (int64_t)X * Y * sk_nw(Z); }        // <= n < 2^31
static inline int64_t sk_vol_bytes(int X, int Y, int Z) { return sk_al16(sk_words(X, Y, Z) * 8); }

// ------------------------------------------------------------------------------------------------ the neighbourhood code
// bit 9 (dx + 1) + 3 (dy + 1) + (dz + 1) is the state of p + (dx, dy, dz); bit 13 (p) is 0.
#define SK_ALL 0x7ffffffu
#define SK_CENTRE (1u << 13)
#define SK_Z0 0x1249249u                    // the bits with dz = -1
#define SK_Z2 0x4924924u                    //               dz = +1
#define SK_Y0 0x01c0e07u                    //               dy = -1
#define SK_Y2 0x70381c0u                    //               dy = +1
#define SK_CORNERS ((1u << 0) | (1u << 2) | (1u << 6) | (1u << 8) | (1u << 18) | (1u << 20) | (1u << 24) | (1u << 26))
#define SK_N18 (SK_ALL & ~SK_CENTRE & ~SK_CORNERS)
#define SK_FACES ((1u << 4) | (1u << 22) | (1u << 10) | (1u << 16) | (1u << 12) | (1u << 14))

// The two adjacency tables of the flood fill, as their definition: sk_adj26(b) = the bits 26-adjacent to bit b among the 26 neighbours,
// sk_adj6(b) = the bits 6-adjacent to bit b inside the 18-neighbourhood.  A frontier grows by the OR of adj[b] over its bits b; that OR
// is a dilation of the 3x3x3 window, which three shifts with the masks above compute for the whole frontier at once (sk_grow26,
// sk_grow6) -- no table in memory, no indexed array.  The static_asserts below hold the two forms together, bit by bit.
constexpr int sk_abs(int v) { return v < 0 ? -v : v; }
constexpr unsigned sk_adj(int b, bool six) {
    unsigned m = 0;
    for (int c = 0; c < 27; ++c) {
        const int dx = sk_abs(b / 9 - c / 9), dy = sk_abs(b / 3 % 3 - c / 3 % 3), dz = sk_abs(b % 3 - c % 3);
        const bool adj = six ? dx + dy + dz == 1 : (dx <= 1 && dy <= 1 && dz <= 1 && c != b);
        if (adj && b != 13 && c != 13) m |= 1u << c;
    }
    return six ? (((SK_N18 >> b) & 1u) ? m & SK_N18 : 0u) : m;
}
__host__ __device__ constexpr unsigned sk_dil_z(unsigned f) { return f | ((f << 1) & SK_ALL & ~SK_Z0) | ((f >> 1) & ~SK_Z2); }
__host__ __device__ constexpr unsigned sk_dil_y(unsigned f) { return f | ((f << 3) & SK_ALL & ~SK_Y0) | ((f >> 3) & ~SK_Y2); }
__host__ __device__ constexpr unsigned sk_dil_x(unsigned f) { return f | (f << 9) | (f >> 9); }
// the frontier and everything adjacent to it (bits above 26 and the centre are for the caller's mask to drop)
__host__ __device__ constexpr unsigned sk_grow26(unsigned f) { return sk_dil_x(sk_dil_y(sk_dil_z(f))); }
__host__ __device__ constexpr unsigned sk_grow6(unsigned f) {
    return f | ((f << 1) & SK_ALL & ~SK_Z0) | ((f >> 1) & ~SK_Z2) | ((f << 3) & SK_ALL & ~SK_Y0) | ((f >> 3) & ~SK_Y2) | (f << 9) | (f >> 9);
}
constexpr bool sk_tables_agree() {
    for (int b = 0; b < 27; ++b) {
        if (b == 13) continue;
        if ((sk_grow26(1u << b) & SK_ALL & ~SK_CENTRE & ~(1u << b)) != sk_adj(b, false)) return false;
        if (((SK_N18 >> b) & 1u) && (sk_grow6(1u << b) & SK_N18 & ~(1u << b)) != sk_adj(b, true)) return false;
    }
    return true;
}
static_assert(sk_tables_agree(), "the shift form of the flood fill is the OR of the adjacency tables");
static_assert(sk_adj(0, false) == 0x161au && sk_adj(1, true) == 0x410u, "the tables of the restatement");

// p is simple: T26 = 1 (one fill from the lowest foreground bit covers the foreground) and T6bar = 1 (one fill from the lowest
// background face neighbour, inside background n 18-neighbourhood, covers every background face neighbour).  No foreground, or no
// background face neighbour: a count of 0, not simple.  Each loop adds at least one of 27 bits per round.
__device__ __forceinline__ bool sk_simple(unsigned code) {
    if (code == 0u) return false;
    const unsigned bg = ~code & SK_N18, faces = bg & SK_FACES;
    if (faces == 0u) return false;
    unsigned f = code & (0u - code);
    for (;;) {
        const unsigned g = sk_grow26(f) & code;
        if (g == f) break;
        f = g;
    }
    if (f != code) return false;
    f = faces & (0u - faces);
    for (;;) {
        const unsigned g = sk_grow6(f) & bg;
        if (g == f) break;
        f = g;
    }
    return (faces & ~f) == 0u;
}

// ------------------------------------------------------------------------------------------------ bytes <-> bits
// pack: one wave per word, lane = z & 63, a ballot of "foreground"; every access coalesced, padding bits 0.
__global__ __launch_bounds__(256) void sk_pack_kernel(const uint8_t* __restrict__ mask, int64_t words, int nw, int Z, sk_word* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int64_t wi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wi >= words) return;                                        // the whole wave leaves
    const int64_t row = wi / nw;
    const int z = (int)(wi - row * nw) * 64 + lane;
    const sk_word b = __builtin_amdgcn_ballot_w64(z < Z && mask[row * Z + z] != 0);
    if (lane == 0) bits[wi] = b;
}

// unpack: a thread per 16 consecutive voxels of the flat volume (they may span rows), one 16-byte store where V == 16, else bytes
template <int V>
__global__ __launch_bounds__(256) void sk_unpack_kernel(const sk_word* __restrict__ bits, int64_t n, int nw, int Z, uint8_t* __restrict__ out) {
    const int64_t v0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (v0 >= n) return;
    int64_t row = v0 / Z;
    int z = (int)(v0 - row * Z);
    int cw = z >> 6;
    sk_word word = bits[row * nw + cw];
    unsigned q[4] = {0u, 0u, 0u, 0u};
    const int cnt = n - v0 < 16 ? (int)(n - v0) : 16;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j < cnt) {
            if ((z >> 6) != cw) { cw = z >> 6; word = bits[row * nw + cw]; }
            q[j >> 2] |= (unsigned)((word >> (z & 63)) & 1ull) << (8 * (j & 3));
            if (++z == Z) {
                z = 0;
                ++row;
                cw = 0;
                if (j + 1 < cnt) word = bits[row * nw];
            }
        }
    }
    if (V == 16 && cnt == 16) {
        *(uint4*)(out + v0) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (j < cnt) out[v0 + j] = (uint8_t)((q[j >> 2] >> (8 * (j & 3))) & 0xffu);
    }
}

// ------------------------------------------------------------------------------------------------ one direction of a pass
// Every launch of a pass after the first of its call starts with one uniform load of the previous pass's count of deletions and leaves
// when that is 0: launches that came earlier on the stream wrote it.
// mark: cand = the foreground voxels whose neighbour in direction D is background; D = 0 .. 5: -x, +x, -y, +y, -z, +z.
template <int D>
__global__ __launch_bounds__(256) void sk_mark_kernel(const sk_word* __restrict__ bits, int64_t words, int X, int Y, int nw, const unsigned* prev,
                                                      sk_word* __restrict__ cand) {
    if (prev && *prev == 0u) return;
    const int64_t wi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (wi >= words) return;
    const int64_t row = wi / nw;
    const int w = (int)(wi - row * nw), x = (int)(row / Y), y = (int)(row - (int64_t)x * Y);
    const sk_word c = bits[wi];
    sk_word nb = 0;
    if (D == 0) { if (x > 0) nb = bits[wi - (int64_t)Y * nw]; }
    else if (D == 1) { if (x < X - 1) nb = bits[wi + (int64_t)Y * nw]; }
    else if (D == 2) { if (y > 0) nb = bits[wi - nw]; }
    else if (D == 3) { if (y < Y - 1) nb = bits[wi + nw]; }
    else if (D == 4) { nb = c << 1; if (w > 0) nb |= bits[wi - 1] >> 63; }
    else { nb = c >> 1; if (w < nw - 1) nb |= bits[wi + 1] << 63; }
    cand[wi] = c & ~nb;
}

// thin: sub-step (sx, sy, sz) of the direction whose marks are in cand.  One thread owns one word of a row with (x & 1, y & 1) =
// (sx, sy) and is the only one to write it in this launch; it looks at its marked bits of z parity sz that are still set.  What another
// thread reads of this word (the bit beside a word edge, from the same row; the rows around have another parity and are not written at
// all) differs, before or after the store, in bits of this subfield only, and those lie in no window that thread assembles: two voxels
// of a subfield are two apart on every axis on which they differ.  So a plain load and a plain store are enough.
__global__ __launch_bounds__(256) void sk_thin_kernel(sk_word* bits, const sk_word* __restrict__ cand, int X, int Y, int nw, int sx, int sy, int sz,
                                                      int nry, int64_t total, const unsigned* prev, unsigned* deleted) {
    if (prev && *prev == 0u) return;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    sk_word del = 0;
    if (t < total) {
        const int64_t r = t / nw;
        const int w = (int)(t - r * nw);
        const int xi = (int)(r / nry), x = 2 * xi + sx, y = 2 * (int)(r - (int64_t)xi * nry) + sy;
        const int64_t wi = ((int64_t)x * Y + y) * nw + w;
        const sk_word cur = bits[wi];
        sk_word todo = cand[wi] & cur & (sz ? 0xaaaaaaaaaaaaaaaaull : 0x5555555555555555ull);
        if (todo) {
            sk_word c[9];                                           // the nine rows of the window, this word of each
            unsigned lo[9], hi[9];                                  // z = 64 w - 1 and z = 64 w + 64 of each
            const bool edge_lo = (todo & 1ull) && w > 0, edge_hi = (todo >> 63) && w < nw - 1;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const int xx = x + i / 3 - 1, yy = y + i % 3 - 1;
                const bool in = xx >= 0 && xx < X && yy >= 0 && yy < Y;
                const int64_t a = in ? ((int64_t)xx * Y + yy) * nw + w : wi;       // a row outside the volume: a valid address, the value dropped
                const sk_word m = in ? ~0ull : 0ull;
                c[i] = bits[a] & m;
                lo[i] = edge_lo ? (unsigned)((bits[a - 1] & m) >> 63) : 0u;
                hi[i] = edge_hi ? (unsigned)(bits[a + 1] & m & 1ull) : 0u;
            }
            while (todo) {
                const int k = __builtin_ctzll(todo);
                todo &= todo - 1;
                unsigned code = 0;
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    unsigned u = k ? (unsigned)(c[i] >> (k - 1)) & 7u : ((unsigned)(c[i] << 1) & 6u) | lo[i];
                    if (k == 63) u |= hi[i] << 2;
                    code |= u << (3 * i);
                }
                code &= ~SK_CENTRE;
                if (__builtin_popcount(code) >= 2 && sk_simple(code)) del |= 1ull << k;      // not an end point, and simple
            }
            if (del) bits[wi] = cur & ~del;
        }
    }
    unsigned cnt = (unsigned)__builtin_popcountll(del);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(deleted, cnt);
}

// ------------------------------------------------------------------------------------------------ 26-neighbour count
// One wave per (row, piece of 62 voxels): lane l holds z = 62 piece - 1 + l, so lanes 0 and 63 are the halo.  Every lane sums the nine
// rows around at its z (nine coalesced byte loads), the sums of z - 1 and z + 1 come from the neighbouring lanes.  It reads the mask
// bytes, not packed bits: the entry takes any mask and has no scratch, and all that voxels share is along z, inside a wave.
__global__ __launch_bounds__(256) void sk_degree_kernel(const uint8_t* __restrict__ mask, int64_t pieces, int np, int X, int Y, int Z,
                                                        uint8_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t pi = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= pieces) return;                                       // the whole wave leaves
    const int64_t row = pi / np;
    const int x = (int)(row / Y), y = (int)(row - (int64_t)x * Y);
    const int z = (int)(pi - row * np) * 62 - 1 + lane;
    const bool inz = z >= 0 && z < Z;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int xx = x + i / 3 - 1, yy = y + i % 3 - 1;
        if (inz && xx >= 0 && xx < X && yy >= 0 && yy < Y) s += mask[((int64_t)xx * Y + yy) * Z + z] != 0;
    }
    const bool self = inz && mask[row * Z + z] != 0;
    const int below = __shfl_up(s, 1), above = __shfl_down(s, 1);
    if (lane >= 1 && lane <= 62 && inz) out[row * Z + z] = (uint8_t)(self ? s + below + above - 1 : 0);     // at most 26: never saturates
}

// ------------------------------------------------------------------------------------------------ entries
extern "C" int64_t vg_skeleton_scratch_bytes(int X, int Y, int Z, int n_passes) {
    if (!sk_voxels(X, Y, Z) || n_passes < 1 || n_passes > VG_SKELETON_MAX_PASSES) return VG_EINVAL;
    return 2 * sk_vol_bytes(X, Y, Z) + sk_al16((int64_t)n_passes * 4);
}

extern "C" int vg_skeleton_begin(const uint8_t* mask, int X, int Y, int Z, void* scratch, int64_t scratch_bytes, vg_stream_t stream) {
    vg_begin();
    if (!mask || !scratch || !sk_voxels(X, Y, Z)) return VG_EINVAL;
    if ((uintptr_t)scratch % 16 != 0 || scratch_bytes < vg_skeleton_scratch_bytes(X, Y, Z, 1)) return VG_EINVAL;
    const int64_t words = sk_words(X, Y, Z);
    hipLaunchKernelGGL(sk_pack_kernel, dim3((unsigned)((words + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mask, words, sk_nw(Z), Z, (sk_word*)scratch);
    return vg_check_launch();
}

template <int D>
static void sk_direction(sk_word* bits, sk_word* cand, int X, int Y, int nw, const unsigned* prev, unsigned* deleted, hipStream_t s) {
    const int64_t words = (int64_t)X * Y * nw;
    hipLaunchKernelGGL(sk_mark_kernel<D>, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, (const sk_word*)bits, words, X, Y, nw, prev, cand);
    for (int sub = 0; sub < 8; ++sub) {
        const int sx = sub >> 2, sy = (sub >> 1) & 1, sz = sub & 1;
        const int nrx = (X - sx + 1) / 2, nry = (Y - sy + 1) / 2;   // the rows with x & 1 == sx, y & 1 == sy
        const int64_t total = (int64_t)nrx * nry * nw;
        if (total == 0) continue;                                   // X == 1 or Y == 1 has no odd rows
        hipLaunchKernelGGL(sk_thin_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, bits, (const sk_word*)cand, X, Y, nw, sx, sy, sz, nry,
                           total, prev, deleted);
    }
}

extern "C" int vg_skeleton_passes(int X, int Y, int Z, int n_passes, void* scratch, int64_t scratch_bytes, uint32_t* deleted_out, vg_stream_t stream) {
    vg_begin();
    if (!scratch || !deleted_out || !sk_voxels(X, Y, Z) || n_passes < 1 || n_passes > VG_SKELETON_MAX_PASSES) return VG_EINVAL;
    if ((uintptr_t)scratch % 16 != 0 || (uintptr_t)deleted_out % 4 != 0 || scratch_bytes < vg_skeleton_scratch_bytes(X, Y, Z, n_passes)) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int nw = sk_nw(Z);
    sk_word* bits = (sk_word*)scratch;
    sk_word* cand = (sk_word*)((char*)scratch + sk_vol_bytes(X, Y, Z));
    if (hipMemsetAsync(deleted_out, 0, (size_t)n_passes * 4, s) != hipSuccess) return VG_ELAUNCH;
    for (int p = 0; p < n_passes; ++p) {
        const unsigned* prev = p ? deleted_out + p - 1 : nullptr;
        unsigned* del = deleted_out + p;
        sk_direction<0>(bits, cand, X, Y, nw, prev, del, s);
        sk_direction<1>(bits, cand, X, Y, nw, prev, del, s);
        sk_direction<2>(bits, cand, X, Y, nw, prev, del, s);
        sk_direction<3>(bits, cand, X, Y, nw, prev, del, s);
        sk_direction<4>(bits, cand, X, Y, nw, prev, del, s);
        sk_direction<5>(bits, cand, X, Y, nw, prev, del, s);
    }
    return vg_check_launch();
}

extern "C" int vg_skeleton_end(int X, int Y, int Z, const void* scratch, int64_t scratch_bytes, uint8_t* out, vg_stream_t stream) {
    vg_begin();
    const int64_t n = sk_voxels(X, Y, Z);
    if (!scratch || !out || !n) return VG_EINVAL;
    if ((uintptr_t)scratch % 16 != 0 || scratch_bytes < vg_skeleton_scratch_bytes(X, Y, Z, 1)) return VG_EINVAL;
    const dim3 grid((unsigned)((n + 4095) / 4096));
    if ((uintptr_t)out % 16 == 0) hipLaunchKernelGGL(sk_unpack_kernel<16>, grid, dim3(256), 0, (hipStream_t)stream, (const sk_word*)scratch, n, sk_nw(Z), Z, out);
    else hipLaunchKernelGGL(sk_unpack_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const sk_word*)scratch, n, sk_nw(Z), Z, out);
    return vg_check_launch();
}

extern "C" int vg_neighbour_count26(const uint8_t* mask, int X, int Y, int Z, uint8_t* out, vg_stream_t stream) {
    vg_begin();
    if (!mask || !out || !sk_voxels(X, Y, Z)) return VG_EINVAL;
    const int np = (Z + 61) / 62;
    const int64_t pieces = (int64_t)X * Y * np;                     // <= n < 2^31
    hipLaunchKernelGGL(sk_degree_kernel, dim3((unsigned)((pieces + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mask, pieces, np, X, Y, Z, out);
    return vg_check_launch();
}
