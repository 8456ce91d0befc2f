// vg_stitch.hip -- batched sliding-window gather / weighted overlap-add for the blended and flip-averaged inference modes
// (van_gan_amd/inference.py; beyond the reference's GanMonitor.stitch_subvolumes, off by default).  fp32 only: the same code in both
// storage builds.  One launch serves a whole batch of windows from a device-resident table of B rows (x0, y0, z0, flip); flip bit a
// mirrors axis a of the window (bit 0 = x, the first axis of the [X][Y][Z] volume).
//
// Shape of both kernels: a "row" is one (entry, i, j) line of the window along z.  `lpr` lanes (a power of two, 4..64, the smallest
// that covers the line or 64) walk one row, so a wave's accesses are 64 / lpr contiguous runs; the 64-bit div/mod that turns the row
// number into (entry, i, j) is done once per row, not per element.  Rows are grid-strided.  No LDS.
#include "vg_common.h"

static inline int sblocks(int64_t threads) { int64_t b = (threads + 255) / 256; return (int)(b > 4095 ? 4095 : (b < 1 ? 1 : b)); }   // odd cap, as vg_loss.hip
static inline int lanes_per_row(int n) { int l = 4; while (l < n && l < 64) l <<= 1; return l; }

struct stitch_row { int x0, y0, z0, flip; bool ok; };
// A row the host wrapper should have rejected (origin outside the volume, unknown flip bits) is skipped and never dereferenced.
__device__ __forceinline__ stitch_row load_row(const int* tab, int64_t b, int kx, int ky, int kz, int X, int Y, int Z) {
    stitch_row r;
    r.x0 = tab[b * 4]; r.y0 = tab[b * 4 + 1]; r.z0 = tab[b * 4 + 2]; r.flip = tab[b * 4 + 3];
    r.ok = r.x0 >= 0 && r.y0 >= 0 && r.z0 >= 0 && r.x0 <= X - kx && r.y0 <= Y - ky && r.z0 <= Z - kz && (unsigned)r.flip < 8u;
    return r;
}

// out[b][i][j][k] = vol[x0 + f_x(i)][y0 + f_y(j)][z0 + f_z(k)]
__global__ void window_gather_kernel(const float* __restrict__ vol, int X, int Y, int Z, const int* __restrict__ tab, int B, int kx, int ky, int kz,
                                     int lpr_log2, float* __restrict__ out) {
    const int lpr = 1 << lpr_log2;
    const int64_t rows = (int64_t)B * kx * ky;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const int lane = (int)(tid & (lpr - 1));
    for (int64_t row = tid >> lpr_log2; row < rows; row += nthr >> lpr_log2) {
        const int j = (int)(row % ky); const int64_t q = row / ky; const int i = (int)(q % kx); const int64_t b = q / kx;
        const stitch_row r = load_row(tab, b, kx, ky, kz, X, Y, Z);
        if (!r.ok) continue;
        const int si = (r.flip & 1) ? kx - 1 - i : i, sj = (r.flip & 2) ? ky - 1 - j : j;
        const float* src = vol + ((size_t)(r.x0 + si) * Y + (r.y0 + sj)) * Z + r.z0;
        float* dst = out + (size_t)row * kz;
        if (r.flip & 4) { for (int k = lane; k < kz; k += lpr) dst[k] = src[kz - 1 - k]; }
        else            { for (int k = lane; k < kz; k += lpr) dst[k] = src[k]; }
    }
}

// pred[x0+i][y0+j][z0+k] += w * win[b][f_x(i)][f_y(j)][f_z(k)], cnt[...] += w over the border-cropped box (i, j, k in volume orientation);
// w = (wx[i] * wy[j]) * wz[k], or 1 when the tables are NULL (then exactly what overlap_add_kernel adds).  Atomics: clamped trailing
// origins coincide, the windows of a batch overlap, and two inference lanes run concurrently.
__global__ void window_scatter_kernel(const float* __restrict__ win, const int* __restrict__ tab, int B, int kx, int ky, int kz, int px, int py, int pz,
                                      const float* __restrict__ wx, const float* __restrict__ wy, const float* __restrict__ wz, int X, int Y, int Z,
                                      int lpr_log2, float* pred, float* cnt) {
    const int lpr = 1 << lpr_log2;
    const int cx = kx - 2 * px, cy = ky - 2 * py;
    const int64_t rows = (int64_t)B * cx * cy;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const int lane = (int)(tid & (lpr - 1));
    for (int64_t row = tid >> lpr_log2; row < rows; row += nthr >> lpr_log2) {
        const int j = (int)(row % cy) + py; const int64_t q = row / cy; const int i = (int)(q % cx) + px; const int64_t b = q / cx;
        const stitch_row r = load_row(tab, b, kx, ky, kz, X, Y, Z);
        if (!r.ok) continue;
        const int si = (r.flip & 1) ? kx - 1 - i : i, sj = (r.flip & 2) ? ky - 1 - j : j;
        const float* src = win + (((size_t)b * kx + si) * ky + sj) * kz;
        const size_t o = ((size_t)(r.x0 + i) * Y + (r.y0 + j)) * Z + r.z0;
        const bool fz = (r.flip & 4) != 0;
        if (wx) {
            const float wxy = wx[i] * wy[j];
            for (int k = pz + lane; k < kz - pz; k += lpr) {
                const float w = wxy * wz[k];
                atomicAdd(&pred[o + k], w * src[fz ? kz - 1 - k : k]);
                atomicAdd(&cnt[o + k], w);
            }
        } else {
            for (int k = pz + lane; k < kz - pz; k += lpr) {
                atomicAdd(&pred[o + k], src[fz ? kz - 1 - k : k]);
                atomicAdd(&cnt[o + k], 1.f);
            }
        }
    }
}

extern "C" int vg_window_gather(const float* vol, int X, int Y, int Z, const int* tab, int B, int kx, int ky, int kz, float* out,
                                vg_stream_t stream) {
    vg_begin();
    if (!vol || !tab || !out || B < 1 || kx < 1 || ky < 1 || kz < 1 || kx > X || ky > Y || kz > Z) return VG_EINVAL;
    const int lpr = lanes_per_row(kz);
    hipLaunchKernelGGL(window_gather_kernel, dim3(sblocks((int64_t)B * kx * ky * lpr)), dim3(256), 0, (hipStream_t)stream, vol, X, Y, Z, tab,
                       B, kx, ky, kz, __builtin_ctz(lpr), out);
    return vg_check_launch();
}

extern "C" int vg_window_scatter(const float* win, const int* tab, int B, int kx, int ky, int kz, int px, int py, int pz, const float* wx,
                                 const float* wy, const float* wz, int X, int Y, int Z, float* pred, float* cnt, vg_stream_t stream) {
    vg_begin();
    if (!win || !tab || !pred || !cnt || B < 1 || kx < 1 || ky < 1 || kz < 1 || kx > X || ky > Y || kz > Z) return VG_EINVAL;
    if (px < 0 || py < 0 || pz < 0 || kx - 2 * px < 1 || ky - 2 * py < 1 || kz - 2 * pz < 1) return VG_EINVAL;
    if ((wx || wy || wz) && !(wx && wy && wz)) return VG_EINVAL;
    const int lpr = lanes_per_row(kz - 2 * pz);
    hipLaunchKernelGGL(window_scatter_kernel, dim3(sblocks((int64_t)B * (kx - 2 * px) * (ky - 2 * py) * lpr)), dim3(256), 0, (hipStream_t)stream,
                       win, tab, B, kx, ky, kz, px, py, pz, wx, wy, wz, X, Y, Z, __builtin_ctz(lpr), pred, cnt);
    return vg_check_launch();
}
