// vg_components.hip -- prediction post-processing (van_gan_amd/postprocess.py; include/vangan_hip.h "Prediction post-processing";
// DESIGN.md 3.16): 3-D connected-component labelling of a uint8 mask by union-find, the removal of small components, the 256-bin
// histogram of a prediction, Otsu's threshold and the thresholding pass.  Nothing here depends on the 16-bit storage format of the build.
// 256-thread workgroups (4 wave64) on a one-dimensional grid.  Only integer atomics.
//
// The union-find keeps ONE invariant: parent[v] <= v, because a link only ever goes to the smaller index (an atomic minimum can only
// lower a word, and every value offered to it is below the index of the word).  Hence every chain of parents strictly decreases: a find
// ends, and so does a unite, whatever mixture of old and new values its loads return -- a stale parent is still an ancestor.  No
// workgroup waits on another: there is no flag, no spin and no look-back; what needs the whole array settled runs in the next launch.
#include "vg_volume.h"

#define CC_TX VG_CC_TILE_X
#define CC_TY VG_CC_TILE_Y
#define CC_TZ VG_CC_TILE_Z
#define CC_TILE (CC_TX * CC_TY * CC_TZ)    // 4096 voxels: two int32 arrays of it are 32 KiB of LDS
#define CC_QUADS (CC_TILE / 4 / 256)       // quads per thread
#define CC_CHUNK 2048                      // voxels per workgroup of the flat passes: 8 consecutive ones per thread
#define CC_HDR_WORDS 16                    // scratch: this header, parent[n], count[n] (later: rank), total[n], roots per chunk
#define CC_FG 0
#define CC_STATUS 1
#define CC_ST_CAP 1u                       // a loop ran into its cap
#define CC_ST_ORDER 2u                     // a parent above its child (or a negative one) was read
#define CC_PLAIN (-1)                      // cc_find on an array nobody writes during the launch: plain loads

static inline bool cc_n_ok(int64_t n) { return n >= 1 && n < ((int64_t)1 << 31); }
static inline int64_t cc_al16(int64_t b) { return (b + 15) & ~(int64_t)15; }
static inline int64_t cc_chunks(int64_t n) { return (n + CC_CHUNK - 1) / CC_CHUNK; }

// The root of a.  parent[v] <= v (see the head of the file), so a strictly decreases until it meets a root: at most a + 1 <= cap loads.
// The decrease is checked, not assumed: a value that breaks it is reported and never followed, so no index leaves [0, a].
template <int SCOPE>
__device__ __forceinline__ int cc_find(const int* p, int a, int64_t cap, unsigned& st) {
    for (int64_t it = 0; it <= cap; ++it) {
        int q;
        if constexpr (SCOPE == CC_PLAIN) q = p[a];
        else q = __hip_atomic_load(p + a, __ATOMIC_RELAXED, SCOPE);
        if (q == a) return a;
        if (q < 0 || q > a) { st |= CC_ST_ORDER; return a; }
        a = q;
    }
    st |= CC_ST_CAP;
    return a;
}

// Joins the trees of a and b.  Every link is a returning atomic minimum on the larger of the two, and the retry is driven by the value it
// RETURNS: old == a means a was a root and now hangs below b; otherwise old < a is (or was) a's parent, a hangs below min(old, b), and
// what remains is to join old and b.  max(a, b) strictly decreases from one round to the next (old < a, parent[v] <= v), so there are at
// most cap = n rounds.
template <int SCOPE>
__device__ __forceinline__ void cc_unite(int* p, int a, int b, int64_t cap, unsigned& st) {
    a = cc_find<SCOPE>(p, a, cap, st);
    b = cc_find<SCOPE>(p, b, cap, st);
    for (int64_t it = 0; it <= cap; ++it) {
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        if (old < 0 || old > a) { st |= CC_ST_ORDER; return; }
        a = old;
    }
    st |= CC_ST_CAP;
}

// The forward half of the structuring element -- the offsets (dx, dy, dz) lexicographically above (0, 0, 0), which lead to a larger
// linear index; the other half is met from the other voxel -- is (0, 0, 1) and the three voxels dz = -1, 0, 1 of four neighbouring rows
// (dx, dy) = (0, 1), (1, -1), (1, 0), (1, 1).  An offset belongs to connectivity c when at most c of its components are non-zero.  Where
// the middle voxel (dx, dy, 0) of a row is foreground, its two neighbours along z hang on it by (0, 0, 1) links -- made in LDS or, across
// a tile face, by the border pass -- and (dx, dy, 0) belongs to every connectivity that (dx, dy, +-1) belongs to: joining the middle voxel
// alone joins the same components, so dz = +-1 are only looked at where the middle voxel is background.
__device__ __forceinline__ int cc_row_dx(int r) { return r == 0 ? 0 : 1; }
__device__ __forceinline__ int cc_row_dy(int r) { return r == 0 ? 1 : r - 2; }

struct cc_tile { int x0, y0, z0; };
__device__ __forceinline__ cc_tile cc_tile_of(int b, int nty, int ntz) {
    cc_tile t;
    t.z0 = (b % ntz) * CC_TZ;
    t.y0 = ((b / ntz) % nty) * CC_TY;
    t.x0 = (b / ntz / nty) * CC_TX;
    return t;
}

// ------------------------------------------------------------------------------------------------ 1: union-find inside a tile, in LDS
// A local index l = (lx * CC_TY + ly) * CC_TZ + lz orders the voxels of a tile as their linear indices do, so the smallest local index of a
// local component is its smallest linear index.  Writes for every voxel of the tile inside the volume: parent = the linear index of its
// local root (-1: background), count = the size of the local component at its root and 0 elsewhere, total = 0.
__global__ __launch_bounds__(256) void cc_local_kernel(const uint8_t* __restrict__ mask, int X, int Y, int Z, int nty, int ntz, int conn,
                                                       int* __restrict__ parent, int* __restrict__ count, int* __restrict__ total,
                                                       unsigned* __restrict__ hdr) {
    __shared__ int lp[CC_TILE], lc[CC_TILE];
    __shared__ unsigned wred[4];
    const int t = threadIdx.x;
    const cc_tile T = cc_tile_of(blockIdx.x, nty, ntz);
    unsigned bits[CC_QUADS], st = 0u, nfg = 0u;
#pragma unroll
    for (int k = 0; k < CC_QUADS; ++k) {
        const int l = (t + 256 * k) * 4, row = l / CC_TZ, lz = l % CC_TZ;
        const int x = T.x0 + row / CC_TY, y = T.y0 + row % CC_TY, z = T.z0 + lz;
        unsigned m = 0u;
        if (x < X && y < Y && z < Z) {
            const uint8_t* src = mask + ((int64_t)x * Y + y) * Z + z;
            if (z + 3 < Z && ((uintptr_t)src & 3) == 0) {
                const unsigned w = *(const unsigned*)src;
                m = ((w & 0xffu) ? 1u : 0u) | ((w & 0xff00u) ? 2u : 0u) | ((w & 0xff0000u) ? 4u : 0u) | ((w & 0xff000000u) ? 8u : 0u);
            } else {
                for (int j = 0; j < 4; ++j) if (z + j < Z && src[j]) m |= 1u << j;
            }
        }
        bits[k] = m;
        nfg += __popc(m);
        int run = -1;                                            // a run along z inside the quad starts out joined
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((m >> j) & 1u) { if (run < 0) run = l + j; } else run = -1;
            lp[l + j] = run;
            lc[l + j] = 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_QUADS; ++k) {
        const int l = (t + 256 * k) * 4, row = l / CC_TZ, lz0 = l % CC_TZ, lx = row / CC_TY, ly = row % CC_TY;
        for (int j = 0; j < 4; ++j) {
            if (!((bits[k] >> j) & 1u)) continue;
            const int lz = lz0 + j;
            if (j == 3 && lz + 1 < CC_TZ && lp[l + 4] >= 0)                           // (0, 0, 1): inside the quad it is joined above
                cc_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, l + 3, l + 4, CC_TILE, st);
            for (int r = 0; r < 4; ++r) {                                                // the four forward rows, see cc_row
                const int dx = cc_row_dx(r), dy = cc_row_dy(r);
                if ((dx != 0) + (dy != 0) > conn) continue;
                const int nx = lx + dx, ny = ly + dy;
                if (nx >= CC_TX || ny < 0 || ny >= CC_TY) continue;                      // across a face: the next launch
                const int nb = (nx * CC_TY + ny) * CC_TZ + lz;
                if (lp[nb] >= 0) { cc_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, l + j, nb, CC_TILE, st); continue; }     // the sign never changes
                if ((dx != 0) + (dy != 0) + 1 > conn) continue;
                if (lz > 0 && lp[nb - 1] >= 0) cc_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, l + j, nb - 1, CC_TILE, st);
                if (lz + 1 < CC_TZ && lp[nb + 1] >= 0) cc_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, l + j, nb + 1, CC_TILE, st);
            }
        }
    }
    __syncthreads();
    int root[CC_QUADS][4];
#pragma unroll
    for (int k = 0; k < CC_QUADS; ++k) {
        const int l = (t + 256 * k) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            root[k][j] = ((bits[k] >> j) & 1u) ? cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lp, l + j, CC_TILE, st) : -1;
    }
#pragma unroll
    for (int k = 0; k < CC_QUADS; ++k) {                             // one LDS atomic per run of equal roots
        int len = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = root[k][j];
            ++len;
            if (j == 3 || root[k][j < 3 ? j + 1 : 3] != r) {
                if (r >= 0) atomicAdd(&lc[r], len);
                len = 0;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < CC_QUADS; ++k) {
        const int l = (t + 256 * k) * 4, row = l / CC_TZ, lz = l % CC_TZ;
        const int x = T.x0 + row / CC_TY, y = T.y0 + row % CC_TY, z = T.z0 + lz;
        if (!(x < X && y < Y && z < Z)) continue;
        const int64_t g = ((int64_t)x * Y + y) * Z + z;
        int gr[4], gc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = root[k][j];
            gr[j] = -1;
            if (r >= 0) {
                const int rrow = r / CC_TZ;
                gr[j] = (int)(((int64_t)(T.x0 + rrow / CC_TY) * Y + (T.y0 + rrow % CC_TY)) * Z + (T.z0 + r % CC_TZ));
            }
            gc[j] = r == l + j ? lc[l + j] : 0;
        }
        if (z + 3 < Z && (g & 3) == 0) {                              // the three arrays are 16-byte aligned: one store each
            *(int4*)(parent + g) = make_int4(gr[0], gr[1], gr[2], gr[3]);
            *(int4*)(count + g) = make_int4(gc[0], gc[1], gc[2], gc[3]);
            *(int4*)(total + g) = make_int4(0, 0, 0, 0);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (z + j < Z) { parent[g + j] = gr[j]; count[g + j] = gc[j]; total[g + j] = 0; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nfg += __shfl_xor(nfg, o); st |= __shfl_xor(st, o); }
    if ((t & 63) == 0) wred[t >> 6] = nfg;
    __syncthreads();
    if (t == 0) {
        const unsigned tot = wred[0] + wred[1] + wred[2] + wred[3];
        if (tot) atomicAdd(hdr + CC_FG, tot);
    }
    if ((t & 63) == 0 && st) atomicOr(hdr + CC_STATUS, st);
}

// ------------------------------------------------------------------------------------------------ 2: links across tile faces
// Workgroups on different XCDs join the same trees here, so parent is touched by agent-scope atomics only: relaxed atomic loads in the
// finds, returning atomic minima for the links.  mask (which nobody writes) says what is foreground.
__global__ __launch_bounds__(256) void cc_border_kernel(const uint8_t* __restrict__ mask, int X, int Y, int Z, int nty, int ntz, int conn,
                                                        int* parent, int64_t n, unsigned* __restrict__ hdr) {
    const int t = threadIdx.x;
    const cc_tile T = cc_tile_of(blockIdx.x, nty, ntz);
    unsigned st = 0u;
    for (int k = 0; k < CC_QUADS; ++k) {
        const int l = (t + 256 * k) * 4, row = l / CC_TZ, lz0 = l % CC_TZ, lx = row / CC_TY, ly = row % CC_TY;
        const int x = T.x0 + lx, y = T.y0 + ly;
        if (!(x < X && y < Y)) continue;
        for (int j = 0; j < 4; ++j) {
            const int lz = lz0 + j, z = T.z0 + lz;
            if (z >= Z) break;
            if (lx < CC_TX - 1 && ly > 0 && ly < CC_TY - 1 && lz > 0 && lz < CC_TZ - 1) continue;      // no neighbour outside the tile
            const int64_t g = ((int64_t)x * Y + y) * Z + z;
            if (!mask[g]) continue;
            if (lz == CC_TZ - 1 && z + 1 < Z && mask[g + 1]) cc_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)g, (int)g + 1, n, st);     // (0, 0, 1)
            for (int r = 0; r < 4; ++r) {                                                // the four forward rows, see cc_row
                const int dx = cc_row_dx(r), dy = cc_row_dy(r);
                if ((dx != 0) + (dy != 0) > conn) continue;
                const int gx = x + dx, gy = y + dy;
                if (gx >= X || gy < 0 || gy >= Y) continue;
                const bool row_out = lx + dx >= CC_TX || ly + dy < 0 || ly + dy >= CC_TY;     // the whole row lies in another tile
                const int64_t gn = ((int64_t)gx * Y + gy) * Z + z;
                if (mask[gn]) { if (row_out) cc_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)g, (int)gn, n, st); continue; }
                if ((dx != 0) + (dy != 0) + 1 > conn) continue;
                if (z > 0 && (row_out || lz == 0) && mask[gn - 1]) cc_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)g, (int)gn - 1, n, st);
                if (z + 1 < Z && (row_out || lz == CC_TZ - 1) && mask[gn + 1]) cc_unite<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)g, (int)gn + 1, n, st);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) st |= __shfl_xor(st, o);
    if ((t & 63) == 0 && st) atomicOr(hdr + CC_STATUS, st);
}

// sum of c over the workgroup's threads with a lower index (exclusive), and the workgroup's sum
__device__ __forceinline__ int cc_block_scan(int c, int* wsum, int& block_total) {
    const int t = threadIdx.x, lane = t & 63;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) wsum[t >> 6] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < (t >> 6); ++w) before += wsum[w];
    block_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return before + inc - c;
}

// ------------------------------------------------------------------------------------------------ 3: roots, sizes, roots per chunk
// parent is settled (the launch before is over) and only read here: plain loads.  root[v] goes to its own array (labels), so nothing
// read in this launch is written in it.  The size of a component is the sum of its tile-local counts: one atomic per local component.
__global__ __launch_bounds__(256) void cc_flatten_kernel(const int* __restrict__ parent, const int* __restrict__ count, int* __restrict__ total,
                                                         int* __restrict__ root, int64_t n, int* __restrict__ chunk_roots,
                                                         unsigned* __restrict__ hdr) {
    __shared__ int wsum[4];
    const int64_t base = (int64_t)blockIdx.x * CC_CHUNK + threadIdx.x * 8;
    unsigned st = 0u;
    int c = 0;
    for (int j = 0; j < 8; ++j) {
        const int64_t v = base + j;
        if (v >= n) break;
        int r = -1;
        if (parent[v] >= 0) {
            r = cc_find<CC_PLAIN>(parent, (int)v, n, st);
            const int cv = count[v];
            if (cv) atomicAdd(total + r, cv);
            c += r == (int)v;
        }
        root[v] = r;
    }
    int tot;
    cc_block_scan(c, wsum, tot);
    if (threadIdx.x == 0) chunk_roots[blockIdx.x] = tot;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) st |= __shfl_xor(st, o);
    if ((threadIdx.x & 63) == 0 && st) atomicOr(hdr + CC_STATUS, st);
}

// ------------------------------------------------------------------------------------------------ 4: exclusive scan of the chunk counts
// One workgroup; a thread takes a contiguous piece.  Also writes result4 and sizes[0].
__global__ __launch_bounds__(256) void cc_scan_kernel(int* __restrict__ chunk_roots, int64_t nchunks, int64_t n, const unsigned* __restrict__ hdr,
                                                      unsigned* __restrict__ result4, unsigned* __restrict__ sizes) {
    __shared__ int part[256];
    const int t = threadIdx.x;
    const int64_t per = (nchunks + 255) / 256, lo = t * per, hi = lo + per < nchunks ? lo + per : nchunks;
    int s = 0;
    for (int64_t i = lo; i < hi; ++i) s += chunk_roots[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        result4[0] = (unsigned)run; result4[1] = hdr[CC_STATUS]; result4[2] = hdr[CC_FG]; result4[3] = 0u;
        sizes[0] = (unsigned)(n - (int64_t)hdr[CC_FG]);
    }
    __syncthreads();
    int run = part[t];
    for (int64_t i = lo; i < hi; ++i) { const int v = chunk_roots[i]; chunk_roots[i] = run; run += v; }
}

// ------------------------------------------------------------------------------------------------ 5: rank of every root = its label
__global__ __launch_bounds__(256) void cc_number_kernel(const int* __restrict__ root, const int* __restrict__ total, const int* __restrict__ chunk_roots,
                                                        int64_t n, int* __restrict__ rank, unsigned* __restrict__ sizes, unsigned* __restrict__ result4) {
    __shared__ int wsum[4];
    const int64_t base = (int64_t)blockIdx.x * CC_CHUNK + threadIdx.x * 8;
    unsigned is_root = 0u;
    for (int j = 0; j < 8; ++j) {
        const int64_t v = base + j;
        if (v < n && root[v] == (int)v) is_root |= 1u << j;
    }
    int tot;
    int k = chunk_roots[blockIdx.x] + cc_block_scan(__popc(is_root), wsum, tot);
    for (int j = 0; j < 8; ++j)
        if ((is_root >> j) & 1u) {
            ++k;                                                    // labels start at 1
            rank[base + j] = k;
            if (k <= n / 2 + 1) sizes[k] = (unsigned)total[base + j];     // the room sizes has; more roots than that cannot be
            else atomicOr(result4 + 1, CC_ST_CAP);
        }
}

// ------------------------------------------------------------------------------------------------ 6: labels, in place over the roots
__global__ __launch_bounds__(256) void cc_relabel_kernel(int* __restrict__ labels, const int* __restrict__ rank, int64_t n) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    for (int64_t v = tid; v < n; v += nthr) {
        const int r = labels[v];
        labels[v] = r >= 0 ? rank[r] : 0;
    }
}

extern "C" int64_t vg_cc_scratch_bytes(int64_t n) {
    if (!cc_n_ok(n)) return VG_EINVAL;
    return (int64_t)CC_HDR_WORDS * 4 + 3 * cc_al16(4 * n) + cc_al16(4 * cc_chunks(n));
}

extern "C" int vg_cc_label(const uint8_t* mask, int X, int Y, int Z, int connectivity, int32_t* labels, uint32_t* sizes, uint32_t* result4,
                           void* scratch, int64_t scratch_bytes, vg_stream_t stream) {
    vg_begin();
    if (!mask || !labels || !sizes || !result4 || !scratch || X < 1 || Y < 1 || Z < 1) return VG_EINVAL;
    if ((int64_t)X * Y >= ((int64_t)1 << 31)) return VG_EINVAL;             // so that the product below cannot overflow
    const int64_t n = (int64_t)X * Y * Z;
    if (!cc_n_ok(n) || connectivity < 1 || connectivity > 3) return VG_EINVAL;
    if ((uintptr_t)labels % 4 != 0 || (uintptr_t)sizes % 4 != 0 || (uintptr_t)result4 % 4 != 0) return VG_EINVAL;
    if (scratch_bytes < vg_cc_scratch_bytes(n) || (uintptr_t)scratch % 16 != 0) return VG_EINVAL;
    const int64_t ntx = (X + CC_TX - 1) / CC_TX, nty = (Y + CC_TY - 1) / CC_TY, ntz = (Z + CC_TZ - 1) / CC_TZ, tiles = ntx * nty * ntz;
    if (tiles * 256 > (int64_t)UINT32_MAX) return VG_EINVAL;                 // one workgroup per tile, and a grid holds fewer than 2^32 threads
    hipStream_t s = (hipStream_t)stream;
    unsigned* hdr = (unsigned*)scratch;
    int* parent = (int*)(hdr + CC_HDR_WORDS);
    int* count = (int*)((char*)parent + cc_al16(4 * n));
    int* total = (int*)((char*)count + cc_al16(4 * n));
    int* chunk_roots = (int*)((char*)total + cc_al16(4 * n));
    const int64_t nchunks = cc_chunks(n);
    const dim3 block(256);
    if (hipMemsetAsync(hdr, 0, CC_HDR_WORDS * 4, s) != hipSuccess) return VG_ELAUNCH;
    hipLaunchKernelGGL(cc_local_kernel, dim3((unsigned)tiles), block, 0, s, mask, X, Y, Z, (int)nty, (int)ntz, connectivity, parent, count, total, hdr);
    hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)tiles), block, 0, s, mask, X, Y, Z, (int)nty, (int)ntz, connectivity, parent, n, hdr);
    hipLaunchKernelGGL(cc_flatten_kernel, dim3((unsigned)nchunks), block, 0, s, parent, count, total, labels, n, chunk_roots, hdr);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), block, 0, s, chunk_roots, nchunks, n, hdr, result4, sizes);
    hipLaunchKernelGGL(cc_number_kernel, dim3((unsigned)nchunks), block, 0, s, labels, total, chunk_roots, n, count, sizes, result4);
    hipLaunchKernelGGL(cc_relabel_kernel, vol_grid(n, 0), block, 0, s, labels, count, n);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ removal of small components
// One workgroup walks sizes[1 .. K] in steps of 256: which components stay, their count, and (newid != nullptr) their new numbers in
// the same order.  Zeroes counts2[0] for the pass that follows.
__global__ __launch_bounds__(256) void cc_keep_kernel(const unsigned* __restrict__ sizes, const unsigned* __restrict__ result4, unsigned min_size,
                                                      int64_t cap, unsigned* __restrict__ counts2, unsigned* __restrict__ newid) {
    __shared__ int wsum[4];
    const int t = threadIdx.x;
    int64_t K = result4[0];
    if (K > cap) K = cap;                                           // never past the room sizes and newid have
    unsigned carry = 0u;
    if (t == 0 && newid) newid[0] = 0u;
    for (int64_t b = 1; b <= K; b += 256) {
        const int64_t k = b + t;
        const int keep = k <= K && sizes[k] >= min_size;
        int tot;
        const int before = cc_block_scan(keep, wsum, tot);
        if (newid && k <= K) newid[k] = keep ? carry + (unsigned)before + 1u : 0u;
        carry += (unsigned)tot;
        __syncthreads();                                            // wsum is written again in the next round
    }
    if (t == 0) { counts2[0] = 0u; counts2[1] = carry; }
}

template <int V>
__global__ __launch_bounds__(256) void cc_filter_kernel(const int* __restrict__ labels, int64_t n, const unsigned* __restrict__ sizes, unsigned min_size,
                                                        uint8_t* __restrict__ out, unsigned* __restrict__ counts2, const unsigned* __restrict__ newid,
                                                        int* __restrict__ relabel) {
    __shared__ unsigned wred[4];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = V == 4 ? n / 4 : 0;
    unsigned kept = 0u;
    for (int64_t i = tid; i < nv; i += nthr) {
        const int4 l = *(const int4*)(labels + i * 4);
        const int lj[4] = {l.x, l.y, l.z, l.w};
        unsigned word = 0u;
        int nl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned k = lj[j] != 0 && sizes[lj[j]] >= min_size;
            word |= k << (8 * j);
            kept += k;
            nl[j] = relabel ? (int)newid[lj[j]] : 0;
        }
        *(unsigned*)(out + i * 4) = word;
        if (relabel) *(int4*)(relabel + i * 4) = make_int4(nl[0], nl[1], nl[2], nl[3]);
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) {
        const int l = labels[e];
        const unsigned k = l != 0 && sizes[l] >= min_size;
        out[e] = (uint8_t)k;
        kept += k;
        if (relabel) relabel[e] = (int)newid[l];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = wred[0] + wred[1] + wred[2] + wred[3];
        if (tot) atomicAdd(counts2, tot);
    }
}

extern "C" int vg_cc_filter(const int32_t* labels, int64_t n, const uint32_t* sizes, const uint32_t* result4, uint32_t min_size, uint8_t* out,
                            uint32_t* counts2, uint32_t* newid_or_null, int32_t* relabel_or_null, vg_stream_t stream) {
    vg_begin();
    if (!labels || !sizes || !result4 || !out || !counts2 || !cc_n_ok(n) || (relabel_or_null && !newid_or_null)) return VG_EINVAL;
    if ((uintptr_t)labels % 4 != 0 || (uintptr_t)sizes % 4 != 0 || (uintptr_t)result4 % 4 != 0 || (uintptr_t)counts2 % 4 != 0 ||
        (uintptr_t)newid_or_null % 4 != 0 || (uintptr_t)relabel_or_null % 4 != 0)
        return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_keep_kernel, dim3(1), dim3(256), 0, s, sizes, result4, min_size, n / 2 + 1, counts2, newid_or_null);
    const int vec = (uintptr_t)labels % 16 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)relabel_or_null % 16 == 0;
    if (vec) hipLaunchKernelGGL(cc_filter_kernel<4>, vol_grid(n, 1), dim3(256), 0, s, labels, n, sizes, min_size, out, counts2, newid_or_null, relabel_or_null);
    else hipLaunchKernelGGL(cc_filter_kernel<1>, vol_grid(n, 0), dim3(256), 0, s, labels, n, sizes, min_size, out, counts2, newid_or_null, relabel_or_null);
    return vg_check_launch();
}

// ------------------------------------------------------------------------------------------------ histogram, Otsu, threshold
// (uint8)x by C truncation for x in [0, 256); finite values outside go to the nearest bin
__device__ __forceinline__ int cc_bin(float x) { return x < 0.f ? 0 : x >= 255.f ? 255 : (int)x; }

template <int V>
__global__ __launch_bounds__(256) void cc_hist_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ hist, unsigned* __restrict__ nonfinite) {
    __shared__ unsigned bins[256];
    __shared__ unsigned wred[4];
    const int t = threadIdx.x;
    bins[t] = 0u;
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * 256 + t, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = V == 4 ? n / 4 : 0;
    unsigned bad = 0u;
    for (int64_t i = tid; i < nv; i += nthr) {
        const f32x4 v = *(const f32x4*)(x + i * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (vol_nonfinite(v[j])) ++bad; else atomicAdd(&bins[cc_bin(v[j])], 1u);
        }
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) {
        const float v = x[e];
        if (vol_nonfinite(v)) ++bad; else atomicAdd(&bins[cc_bin(v)], 1u);
    }
    __syncthreads();
    if (bins[t]) atomicAdd(hist + t, bins[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((t & 63) == 0) wred[t >> 6] = bad;
    __syncthreads();
    if (t == 0) {
        const unsigned tot = wred[0] + wred[1] + wred[2] + wred[3];
        if (tot) atomicAdd(nonfinite, tot);
    }
}

extern "C" int vg_hist256(const float* pred, int64_t n, uint32_t* hist, uint32_t* nonfinite, vg_stream_t stream) {
    vg_begin();
    if (!pred || !hist || !nonfinite || !cc_n_ok(n)) return VG_EINVAL;
    if ((uintptr_t)pred % 4 != 0 || (uintptr_t)hist % 4 != 0 || (uintptr_t)nonfinite % 4 != 0) return VG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, 256 * 4, s) != hipSuccess) return VG_ELAUNCH;
    const dim3 grid(vol_blocks(n, 256 * 16));                       // at least 4096 voxels per flush of the LDS bins
    if ((uintptr_t)pred % 16 == 0) hipLaunchKernelGGL(cc_hist_kernel<4>, grid, dim3(256), 0, s, pred, n, hist, nonfinite);
    else hipLaunchKernelGGL(cc_hist_kernel<1>, grid, dim3(256), 0, s, pred, n, hist, nonfinite);
    return vg_check_launch();
}

// Otsu's threshold of a 256-bin histogram, one thread, fp64.  The cumulative sums are integers below 2^53 (n < 2^31, bins < 2^8), so
// they are exact in any order and kept as integers; the two divisions, the difference and the three products are rounded one by one
// (contraction is off in the function), in numpy's order: (weight1 * weight2) * (d * d).  256 steps: one thread is the right size.
__global__ void cc_otsu_kernel(const unsigned* __restrict__ hist, float* __restrict__ t_out) {
#pragma clang fp contract(off)             // every fp64 operation below is rounded on its own, as numpy rounds it
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    unsigned long long s0 = 0ull, s1 = 0ull;
    for (int b = 0; b < 256; ++b) { s0 += hist[b]; s1 += (unsigned long long)hist[b] * (unsigned)b; }
    unsigned long long w1 = 0ull, m1 = 0ull;
    double best = 0.0;
    int arg = 0;
    for (int i = 0; i < 255; ++i) {
        w1 += hist[i];
        m1 += (unsigned long long)hist[i] * (unsigned)i;
        const unsigned long long w2 = s0 - w1, m2 = s1 - m1;
        double var = 0.0;
        if (w1 != 0ull && w2 != 0ull) {
            const double mean1 = (double)m1 / (double)w1, mean2 = (double)m2 / (double)w2;
            const double d = mean1 - mean2;
            const double ww = (double)w1 * (double)w2, dd = d * d;
            var = ww * dd;
        }
        if (i == 0 || var > best) { best = var; arg = i; }          // the first maximum
    }
    *t_out = (float)arg;
}

template <int V>
__global__ __launch_bounds__(256) void cc_threshold_kernel(const float* __restrict__ x, int64_t n, int as_u8, float t_host, const float* __restrict__ t_dev,
                                                           uint8_t* __restrict__ mask, unsigned* __restrict__ nonfinite) {
    __shared__ unsigned wred[4];
    const float thr = t_dev ? *t_dev : t_host;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthr = (int64_t)gridDim.x * 256;
    const int64_t nv = V == 4 ? n / 4 : 0;
    unsigned bad = 0u;
    for (int64_t i = tid; i < nv; i += nthr) {
        const f32x4 v = *(const f32x4*)(x + i * 4);
        unsigned word = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned nf = vol_nonfinite(v[j]);
            const unsigned m = !nf && (as_u8 ? (float)cc_bin(v[j]) > thr : v[j] > thr);
            bad += nf;
            word |= m << (8 * j);
        }
        *(unsigned*)(mask + i * 4) = word;
    }
    for (int64_t e = nv * 4 + tid; e < n; e += nthr) {
        const float v = x[e];
        const unsigned nf = vol_nonfinite(v);
        bad += nf;
        mask[e] = (uint8_t)(!nf && (as_u8 ? (float)cc_bin(v) > thr : v > thr));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = wred[0] + wred[1] + wred[2] + wred[3];
        if (tot) atomicAdd(nonfinite, tot);
    }
}

extern "C" int vg_threshold_mask(const float* pred, int64_t n, int as_u8, float t, const float* t_dev_or_null, int otsu, const uint32_t* hist256_or_null,
                                 float* t_otsu_or_null, uint8_t* mask, uint32_t* nonfinite, vg_stream_t stream) {
    vg_begin();
    if (!pred || !mask || !nonfinite || !cc_n_ok(n) || (otsu != 0 && otsu != 1) || (otsu && (!hist256_or_null || !t_otsu_or_null))) return VG_EINVAL;
    if ((uintptr_t)pred % 4 != 0 || (uintptr_t)t_dev_or_null % 4 != 0 || (uintptr_t)hist256_or_null % 4 != 0 || (uintptr_t)t_otsu_or_null % 4 != 0 ||
        (uintptr_t)nonfinite % 4 != 0)
        return VG_EINVAL;
    if (!otsu && !t_dev_or_null && t != t) return VG_EINVAL;        // a NaN threshold
    hipStream_t s = (hipStream_t)stream;
    if (otsu) {
        hipLaunchKernelGGL(cc_otsu_kernel, dim3(1), dim3(64), 0, s, hist256_or_null, t_otsu_or_null);
        as_u8 = 1;
        t_dev_or_null = t_otsu_or_null;
    }
    if ((uintptr_t)pred % 16 == 0 && (uintptr_t)mask % 4 == 0)
        hipLaunchKernelGGL(cc_threshold_kernel<4>, vol_grid(n, 1), dim3(256), 0, s, pred, n, as_u8 ? 1 : 0, t, t_dev_or_null, mask, nonfinite);
    else
        hipLaunchKernelGGL(cc_threshold_kernel<1>, vol_grid(n, 0), dim3(256), 0, s, pred, n, as_u8 ? 1 : 0, t, t_dev_or_null, mask, nonfinite);
    return vg_check_launch();
}
