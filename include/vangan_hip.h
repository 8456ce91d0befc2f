/* vangan_hip.h -- C ABI of libvangan_hip.so (MI355X / gfx950 only).
 *
 * The reference (psweens/VAN-GAN) has NO native plugin/FFI interface: its hot path sits behind
 * the Python class VanGan (vangan.py:20-550) and executes inside TensorFlow.  These entry points
 * are what a ctypes binding on the reference side would call in place of the TensorFlow ops of
 * that path; each one cites the reference lines whose arithmetic it replaces.
 *
 * Rules of the boundary:
 *   - every pointer is a DEVICE pointer owned by the caller, valid on `stream` for the call;
 *   - the library never allocates/frees device memory and never synchronises: enqueue-only (launch plans that need
 *     device workspace take it from the caller: vg_conv_desc::scratch, the scratch argument of vg_conv3d_wgrad);
 *   - every entry returns 0 on success, <0 on error (vg_status_string); no exception or abort
 *     crosses the ABI;
 *   - activations are NDHWC (channel innermost). "bf16" buffers hold 16-bit brain floats.
 */
#ifndef VANGAN_HIP_H
#define VANGAN_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* vg_stream_t;          /* hipStream_t */

#define VG_OK 0
#define VG_EINVAL (-1)              /* bad argument / unsupported shape */
#define VG_ELDS (-2)                /* tile does not fit the 160 KiB LDS */
#define VG_ELAUNCH (-3)             /* HIP launch failure */

#define VG_ACT_NONE 0
#define VG_ACT_RELU 1
#define VG_ACT_LRELU 2              /* LeakyReLU(0.2), discriminator.py:75 */

#define VG_PAD_ZERO 0               /* Keras 'same' zero padding */
#define VG_PAD_REFLECT 1            /* ReflectionPadding3D, building_blocks.py:30-39 */

#define VG_MAX_TAPS 64

/* Per-(n,c) reduction buffers (InstanceNorm sums, backward reductions) are STRIPED: [VG_STRIPES][N][C][2]; a
 * workgroup adds into stripe (its index mod VG_STRIPES) so that float atomics from 10^4 workgroups do not serialise
 * on one 128-byte line; consumers sum the stripes. */
#define VG_STRIPES 8

const char* vg_status_string(int code);
/* diagnostic builds only: device buffer receiving s_memtime stamps of the conv kernel phases (NULL = off) */
int vg_set_stamp_buffer(void* dev_u64);
int vg_version(void);
/* The 16-bit storage format of THIS build: 0 = bfloat16 (libvangan_hip.so: training and inference), 1 = IEEE half precision
 * (libvangan_hip_h.so: the same sources compiled with -DVG_FP16 -- the fp16 sliding-window inference of BASELINE config 5,
 * post_training.py:38-39 / custom_callback.py:174-175).  Every "bf16" buffer of this header holds that format. */
int vg_storage16(void);
/* sizeof() of the descriptor structs as THIS library was compiled (which: 0 vg_conv_desc, 1 vg_actnorm_bwd_desc,
 * 2 vg_pack_item, 3 vg_fin_desc, 4 vg_sn_item; else VG_EINVAL): a binding that mirrors the structs by hand checks its layout at load time. */
int vg_abi_sizeof(int which);

/* ---------------------------------------------------------------------------------------------
 * Gather-convolution (implicit GEMM on bf16 MFMA).  One descriptor covers
 *   - Conv3D forward for every variant on the path (resunet_model.py:42-143,
 *     building_blocks.py:126-196, discriminator.py:50-117): k3/k1/k4, stride 1/2, reflect or zero
 *     padding folded into the index math, InstanceNorm-apply + ReLU/LeakyReLU (+ channel-dropout,
 *     + GaussianNoise) applied on read, nearest-2x upsample + concat read virtually
 *     (resunet_model.py:175-181), bias / residual-add / tanh / next-InstanceNorm statistics in
 *     the epilogue;
 *   - its data gradient (what tf.GradientTape computes for d/d input of Conv3D): the same kernel
 *     on dY with transposed packed weights, per output-parity class for stride 2.
 * out[n, o*ostr+ooff, co] (+)= sum_taps sum_ci f(src[n, bnd(o*istr + tap), ci]) * W[tap][ci][co]
 * --------------------------------------------------------------------------------------------- */
struct vg_actnorm_bwd_desc_s;
/* InstanceNorm finalisation of a convolution's OUTPUT by the launch that produces it (resunet_model.py:23-39 / building_blocks.py:190:
 * tfa InstanceNormalization = per-(n, c) mean and biased variance over the volume, y = (x - mean) * rsqrt(var + eps) * gamma + beta).
 * The producing kernel already accumulates (sum, sum of squares) of what it stores (out_sums); with a vg_fin_desc the workgroup that
 * finishes LAST (ticket) turns them into the on-read affine of up to two consuming norms -- scale = gamma * rstd (* mult),
 * shift = (beta - mean * gamma * rstd) (* mult), and mean / rstd for the backward pass -- instead of a vg_in_finalize launch
 * between producer and consumer (120 launches of a train step, each on a lane's dependent chain).  A tensor may feed two norms
 * (an encoder output: the next block's first norm and, as the skip half of a virtual concat, a decoder block's): job j writes
 * channels [c_off, c_off + Cout) of arrays with c_tot channels per sample.  Kernel families without the epilogue are followed by a
 * small kernel inside vg_conv3d: either way the arrays are complete, in stream order, when the call's launches have run. */
typedef struct {
    const float* gamma; const float* beta;    /* [c_tot] of the consuming norm (NULL: 1 / 0) */
    const float* mult;                        /* [N][c_tot] SpatialDropout3D multipliers folded into scale / shift, or NULL */
    float* scale; float* shift;               /* [N][c_tot] */
    float* mean; float* rstd;                 /* [N][c_tot] or NULL */
    int32_t c_off, c_tot;
} vg_fin_job;
typedef struct {
    uint32_t* ticket;                         /* one zeroed word per launch (left non-zero) */
    float count;                              /* voxels per (n, c) of the produced tensor */
    float eps;
    int32_t njobs;                            /* 1 or 2 */
    vg_fin_job job[2];
} vg_fin_desc;
typedef struct {
    /* input: virtual concat of src0 (c_src0 channels) and src1 (c_src1 channels, may be 0) */
    const void* src0;
    const void* src1;
    int32_t c_src0, c_src1;
    int32_t src0_shift;      /* 1: src0 is stored at half resolution, read at (d>>1,h>>1,w>>1) */
    int32_t src_f32;         /* 1: sources are float32 (only with a single input channel) */
    int32_t N, D, H, W;      /* logical input grid (full resolution) */
    const float* in_scale;   /* [N][Cin] on-read affine (InstanceNorm apply) or NULL */
    const float* in_shift;
    int32_t act;             /* VG_ACT_* applied after the affine */
    const void* noise;       /* bf16 [N][D+2np][H+2np][W+2np][Cin] added after act, or NULL */
    int32_t noise_pad;       /* np: 1 when the noise lives on the reflect-padded grid */
    /* geometry */
    int32_t istr;            /* input stride per output step */
    int32_t pad_mode;        /* VG_PAD_* for out-of-range input positions */
    int32_t ntaps;
    int8_t tap_d[VG_MAX_TAPS], tap_h[VG_MAX_TAPS], tap_w[VG_MAX_TAPS];  /* input offset of tap */
    int32_t OD, OH, OW;      /* iteration space: output positions per dim */
    int32_t ostr, ooff_d, ooff_h, ooff_w;   /* buffer position = o*ostr + ooff */
    int32_t BD, BH, BW;      /* output buffer grid */
    int32_t Cout;
    /* weights: bf16 [round_up(Cout,64)][Ktot], packed by vg_pack_weights with the same CK/taps */
    const void* wpacked;
    int32_t CK;              /* contraction channels staged per chunk (multiple of 16) */
    const float* bias;       /* [Cout] or NULL */
    /* epilogue */
    const void* res;         /* bf16 [N][BD][BH][BW][Cout] residual operand or NULL */
    const float* res_scale;  /* [N][Cout] affine on the residual (InstanceNorm of the shortcut) */
    const float* res_shift;
    int32_t tanh_out;        /* tanh after everything else; with accumulate: out = tanh(out + value) (last tap chunk of a 7^3 head) */
    void* out;               /* bf16 (or f32 when out_f32) [N][BD][BH][BW][Cout] */
    int32_t out_f32;
    int32_t accumulate;      /* out += value (data-gradient accumulation) */
    float* out_sums;         /* [VG_STRIPES][N][Cout][2] += (sum, sum of squares) of the stored values, or NULL */
    int32_t f32;             /* exact-parity mode: every "bf16" buffer of this call (multi-channel sources, res, out,
                                packed weights, and dy/dgrad operands) is float32 and the MFMA is the f32 16x16x4 form */
    /* Fused output-parity classes (data gradient of a strided Conv3D, vangan.py:426-438 via tf.GradientTape): with
       nclass > 1 ONE launch stages each dY halo tile once and produces the outputs of all classes.  Class c uses the
       taps tap_*[cls_tap0[c] .. cls_tap0[c+1]), its own packed weights cls_w[c] (packed with those taps and CK), the
       output offset cls_ooff[c] (replaces ooff_*) and cls_iters[c] outputs per axis (replaces OD/OH/OW, which must
       hold the per-axis maximum).  With one channel chunk (c_src0 + c_src1 <= CK, bf16, no noise) the classes share the
       staged tile; otherwise the launch is class-parallel (workgroup -> one class), any number of chunks, all classes
       packed with the same CK.  nclass 0 or 1: fields unused. */
    int32_t nclass;
    int32_t cls_tap0[9];
    const void* cls_w[8];
    int32_t cls_ooff[8][3];
    int32_t cls_iters[8][3];
    /* W-packed single-channel source (the Conv3D layers that read a 1-channel volume: resunet_model.py:44-60 stem,
       discriminator.py:50-60 first conv).  wpack = k > 1: the k taps along W become k pseudo-channels, the descriptor lists
       only the k*k (d, h) taps (tap_w = 0), wpack_wmin is the W offset of the first tap (-pad_before).  The packed weights
       are the same DHWIO kernel read as [k*k taps][k channels][Cout] (vg_pack_weights with ntaps = k*k, Cin = k), and
       vg_conv3d_wgrad returns dw in that layout, i.e. the unchanged DHWIO tensor (T_total = k*k).  0: off. */
    int32_t wpack;
    int32_t wpack_wmin;
    /* Optional (data-gradient launches): the STATISTICS pass of the IN backward that consumes this launch's output (g == out,
       bf16, one launch covering the whole grid, no accumulate).  The 16-channel specialist accumulates sum dn and sum dn*xhat
       in its epilogue -- the upstream gradient is not re-read from HBM -- other kernels are followed by vg_actnorm_bwd_stats.
       Either way the striped sums in red are complete when the call returns; the caller then runs vg_actnorm_bwd_apply (which adds
       the stripes up and produces dgamma / dbeta). */
    const struct vg_actnorm_bwd_desc_s* bstat;
    /* Optional caller-owned device workspace for launches on THIS stream (the library never allocates).  Bytes
       [0, VG_SCRATCH_CTR_BYTES) are arrival counters: zeroed ONCE by the caller when it allocates the buffer, left at zero by every
       launch.  The rest carries no state between launches (fp32 partial tiles of K-split launches, the materialised operand of the
       LDS-DMA convolution).  Two launches may share a scratch only if they are ordered (same stream).  NULL or too small: the
       library chooses launch plans that need none. */
    void* scratch;
    int64_t scratch_bytes;
    /* Layout of wpacked / cls_w: 0 = rows x Ktot (vg_pack_weights, the gather kernels); 64 / 128 = the block layout of the LDS-DMA
       convolution with that channel-panel width (vg_pack_weights_dma; the caller asks vg_conv3d_dma_bn which layers take it and needs
       a scratch big enough for the materialised operand).  A call whose weights are in the block layout is served by that kernel
       family or fails with VG_EINVAL -- never by a silent fallback. */
    int32_t wlayout;
    /* Optional (forward launches with out_sums): finalise the InstanceNorm statistics of this launch's output for its consumers
       (see vg_fin_desc). */
    const vg_fin_desc* fin;
    /* res_c1 != 0: `res` is a SINGLE-channel fp32 volume [N][BD][BH][BW] (same grid as the output, ostr == 1) whose value is broadcast
       over the output channels: out += res[v] * res_scale[n][c] + res_shift[n][c].  The stem's shortcut Conv3D(16, 1x1x1)(x) ->
       InstanceNorm (resunet_model.py:96-99) is an affine function of the input volume per channel, so the block's residual add reads
       the 4-byte volume instead of a stored 16-channel tensor (vg_stem_short_fwd produces the scale / shift).  Served by the 16-channel
       specialist and the generic kernel; other families return VG_EINVAL. */
    int32_t res_c1;
    /* Optional, forward launches whose src0 is the virtually upsampled half-resolution tensor (src0_shift != 0, c_src0 a multiple of 16,
       reflection pad, 3x3x3): the class panels of vg_pack_up_weights for the c_src0 / 16 upsampled channel chunks.  The 16-channel
       specialist then contracts those chunks over the half-resolution image with the D / H taps collapsed (12 instead of 27 taps per
       chunk; UpSampling3D + IN + ReLU + reflect pad + Conv3D of resunet_model.py:175-181 and :42-66 -- IN and ReLU commute with the
       upsampling, the reflection pad becomes edge replication at half resolution).  NULL: the plain 27-tap form. */
    const void* wpacked_up;
} vg_conv_desc;
#define VG_SCRATCH_CTR_BYTES 16384

int vg_conv3d(const vg_conv_desc* d, vg_stream_t stream);

/* bytes of dynamic LDS the chosen tile needs, or <0 */
int vg_conv3d_lds_bytes(const vg_conv_desc* d);
/* the launch plan vg_conv3d would use for this descriptor: plan[0] = channel panel BN, plan[1] = voxels per tile,
   plan[2] = LDS bytes, plan[3] = workgroups; lets the host compare channel-chunk sizes (CK) before packing weights */
int vg_conv3d_plan(const vg_conv_desc* d, int32_t* plan4);
/* Shape-only: 2 when the two-panel instance of the thin-channel specialist (3x3x3, stride 1, 16-channel chunks, 32 output channels
   per workgroup: the 32-channel layers at 64^3) would serve d -- the host then packs those weights with CK = 16; else 0.  d->CK is
   ignored.  (Replaces nothing in the reference: tile planning of resunet_model.py:36-43,82-95's Conv3D calls.) */
int vg_conv3d_thin_np(const vg_conv_desc* d);
/* Dry run of vg_conv3d: the whole dispatch runs, nothing is launched, and buf receives the name of the kernel variant the
   call would launch, e.g. "conv<bf16,16,8,n0,wl1,dma0,mc0,c10>|walk1|ch0" (template arguments, then walk = a workgroup
   visits more than one tile, ch = several channel chunks per tile) or "pw_cto1<bf16,2>".  The parity tests use it to prove
   that every variant the BASELINE configurations run is compared with the oracle (tests/test_variant_coverage.py). */
int vg_conv3d_variant(const vg_conv_desc* d, char* buf, int buflen);
/* Host-side heuristic switches (forced tile shapes, persistent grid sizes, ...): key without the VG_ prefix of the
   environment variable that sets the same switch, e.g. ("CONV_MSUB", 4).  reset != 0: back to environment / default.
   Testing and tuning aid; the defaults are what the benchmarks run. */
int vg_set_tuning(const char* key, int value, int reset);

/* Class panels of the collapsed upsampled chunks (vg_conv_desc::wpacked_up) from the fp32 DHWIO kernel w[3][3][3][Cin][Cout] of a decoder
 * block's first convolution whose first c_up input channels (a multiple of 16) are the upsampled tensor:
 *   out[chunk][class = pd*2 + ph][co][(td*2 + th)*3 + tw][16 channels of the chunk]   (16-bit storage format of the build), where for an
 *   output voxel of parity p along an axis the collapsed tap t = 0 sums the original taps {-1} (p = 0) or {-1, 0} (p = 1) and t = 1 sums
 *   {0, +1} (p = 0) or {+1} (p = 1); sums in fp32, one rounding. */
int vg_pack_up_weights(const float* w, int Cin, int Cout, int c_up, void* out, vg_stream_t stream);

/* Pack fp32 Keras DHWIO weights [T][Cin][Cout] to the bf16 layout vg_conv3d reads.
 * transpose=0: rows = Cout, contraction = Cin (forward); transpose=1: rows = Cin, contraction =
 * Cout (data gradient).  tap_idx[i] selects the source tap of packed tap i.  Returns Ktot>0. */
int vg_pack_weights(const float* w, int T, int Cin, int Cout, const int32_t* tap_idx_dev, int ntaps,
                    int transpose, int CK, void* out, int out_f32, vg_stream_t stream);
/* Table-driven repack of every packed operand of a network in ONE launch: items_dev is a device array of n
 * vg_pack_item (all pointers device pointers).  Item i is served by the nblk >= 1 blocks starting at blk0 of a 1-D grid of
 * total_blocks = sum(nblk) blocks (the caller sizes nblk in proportion to the operand, the ranges must tile the grid). */
typedef struct {
    const float* w; const int32_t* tap_idx; void* out;
    int32_t Cin, Cout, ntaps, transpose, CK, out_f32;
    int32_t blk0, nblk;
    int32_t bn;              /* > 0: the block layout of vg_pack_weights_dma with this panel width (CK / out_f32 unused) */
    int32_t pad_;
} vg_pack_item;
int vg_pack_weights_multi(const vg_pack_item* items_dev, int n, int total_blocks, vg_stream_t stream);
/* The LDS-DMA convolution (vg_conv_dma.hip: both MFMA operands staged by global_load_lds, the wide layers of discriminator.py:64-117
 * and resunet_model.py:103-143 and their data gradients).  vg_conv3d_dma_bn: shape-only query -- the channel-panel width (64 / 128)
 * with which vg_conv3d would serve this descriptor through that family, 0 if it would not; no pointer of d is looked at.
 * vg_pack_weights_dma: fp32 DHWIO [T][Cin][Cout] -> bf16 [rows / bn][contraction / 16][tap][8-channel half][bn rows][8], rows =
 * output channels (transpose 0) or input channels (transpose 1, data gradient); rows * contraction * ntaps elements. */
int vg_conv3d_dma_bn(const vg_conv_desc* d);
/* Bytes of vg_conv_desc::scratch with which a call whose weights are in the block layout (wlayout != 0) runs at its preferred plan:
 * counters + the materialised operand -- which grows with d->N, the one thing the shape-only query above cannot see -- + the partial
 * tiles of its K split.  A smaller scratch drops the K split first; one that cannot hold the operand makes vg_conv3d return VG_EINVAL
 * (block-layout weights have no other kernel).  0 for every other descriptor.  The caller sizes / grows its workspace with this. */
int64_t vg_conv3d_scratch_bytes(const vg_conv_desc* d);
int vg_pack_weights_dma(const float* w, int T, int Cin, int Cout, const int32_t* tap_idx_dev, int ntaps, int transpose, int bn,
                        void* out, vg_stream_t stream);
int vg_packed_ktot(int ntaps, int C, int CK);
int vg_packed_rows(int N);

/* ---------------------------------------------------------------------------------------------
 * Weight gradient of the same gather-convolution (tf.GradientTape d/dW of Conv3D, vangan.py:426-438):
 * dW[tap][ci][co] += sum_{n,o} f(src[n, bnd(o*istr+tap), ci]) * dY[n,o,co];  db[co] += sum dY.
 * Uses the input fields of vg_conv_desc (src*, transform, taps, OD/OH/OW); `dy` is bf16 (or f32 when
 * dy_f32) [N][OD][OH][OW][Cout]; dw is fp32 DHWIO [T_total][Cin][Cout] indexed by tap_idx_host[i].
 * --------------------------------------------------------------------------------------------- */
int vg_conv3d_wgrad(const vg_conv_desc* d, const void* dy, int dy_f32, const int32_t* tap_idx_host,
                    int T_total, float* dw, float* db, float* scratch, int64_t scratch_bytes, vg_stream_t stream);
/* dry run of vg_conv3d_wgrad (see vg_conv3d_variant): "wgrad<bf16,8,1,n0>|bm256|cib16|part1|walk1" */
int vg_conv3d_wgrad_variant(const vg_conv_desc* d, int dy_f32, const int32_t* tap_idx_host, int T_total,
                            int64_t scratch_bytes, char* buf, int buflen);
/* scratch (optional, device): when many workgroups share one dW element their slabs are stored to
 * scratch[workgroup column][T_total*Cin*Cout] and summed in a fixed order by a second kernel instead of float atomics. */

/* ---------------------------------------------------------------------------------------------
 * InstanceNorm helpers (tfa InstanceNormalization, resunet_model.py:36, building_blocks.py:190)
 * --------------------------------------------------------------------------------------------- */
/* scale/shift[n][c] for on-read normalisation from accumulated striped (sum,sumsq) [VG_STRIPES][N][c][2]; channels
 * [0,c0) come from sums0 (count0 voxels), [c0,c0+c1) from sums1.  mult[n][c] (SpatialDropout3D mask, >=0) optional.
 * Also writes mean/rstd [N][C] when non-NULL (needed by the backward). */
int vg_in_finalize(const float* sums0, int c0, float count0, const float* sums1, int c1, float count1,
                   const float* gamma, const float* beta, const float* mult, int N, float eps,
                   float* scale, float* shift, float* mean, float* rstd, vg_stream_t stream);

/* Backward of  a = mult * act(x*scale+shift)  [InstanceNorm -> activation -> dropout], with the
 * upstream gradient g read either plain ([N][D][H][W][C]) or folded from the reflect-padded grid
 * ([N][D+2][H+2][W+2][C], transpose of ReflectionPadding3D).
 * pass 1 (stats):  red[stripe][n][c][0] += sum dn,  red[stripe][n][c][1] += sum dn*xhat,   dn = g*mult*act'(.)   (striped partial
 *                  sums; the apply pass adds the stripes up and produces dgamma / dbeta)
 * pass 2 (apply):  dx (+)= gamma*rstd*(dn - mean(dn) - xhat*mean(dn*xhat))      (norm=1)
 *                  dx (+)= dn                                                     (norm=0)
 * x is bf16 (x_f32=0) ; g is bf16; dx is bf16 unless dx_f32. */
typedef struct vg_actnorm_bwd_desc_s {
    const void* g; int32_t g_padded;
    const void* x; int32_t x_f32;            /* forward input of the norm (channels [0,c_x0) when x1 is set) */
    const void* x1; int32_t c_x0; int32_t x0_shift;   /* virtual upsample+concat: x = [up(x), x1] */
    int32_t N, D, H, W, C;
    const float* scale; const float* shift;   /* on-read affine of the forward, [N][C], or NULL */
    const float* mult;                        /* [N][C] or NULL */
    int32_t act; int32_t norm;
    const float* gamma; const float* mean; const float* rstd;   /* norm=1 */
    float* red;                               /* [VG_STRIPES][N][C][2], zeroed by the caller */
    void* dx; int32_t dx_f32; int32_t accumulate;
    int32_t dx_cstride, dx_coff;              /* dx channel stride / offset (write into a slice) */
    int32_t f32;                              /* exact-parity mode: g, x, x1 and dx are float32 */
    float* dgamma;                            /* optional [C]: the APPLY pass adds d/d gamma and d/d beta of the InstanceNorm */
    float* dbeta;                             /* (summed over samples and stripes) instead of a separate vg_in_param_grads */
    int32_t* ticket;        /* unused (the stripes are added up by the apply pass); kept for layout stability */
    /* Several upstream gradients of ONE forward sample in one launch (the discriminator's two backward sweeps -- the critic loss over
       [real; fake] and the generator loss through the fake half, vangan.py:426-438 -- as one 3B-sample sweep): samples n >= alias_n0 of g /
       dx / red read x, x1 and every per-(sample, channel) array (scale, shift, mean, rstd, mult) of sample n - alias_shift.  0: off.
       pgrad_n > 0: only samples < pgrad_n add to dgamma / dbeta (the generator-loss gradient updates no discriminator parameter). */
    int32_t alias_n0, alias_shift, pgrad_n, pad_;
} vg_actnorm_bwd_desc;
int vg_actnorm_bwd_stats(const vg_actnorm_bwd_desc* d, vg_stream_t stream);
int vg_actnorm_bwd_apply(const vg_actnorm_bwd_desc* d, vg_stream_t stream);
/* the apply passes of two independent norms of one batch (same N; statistics of both complete) in one launch -- a residual block's shortcut
 * norm and the norm in front of its second convolution (resunet_model.py:103-143 under the tape); two launches where the pair does not share
 * a kernel instance */
int vg_actnorm_bwd_apply2(const vg_actnorm_bwd_desc* d1, const vg_actnorm_bwd_desc* d2, vg_stream_t stream);
/* both passes in one call (statistics only when d->norm) */
int vg_actnorm_bwd(const vg_actnorm_bwd_desc* d, vg_stream_t stream);
/* The stem's shortcut in the forward pass (resunet_model.py:96-99: Conv3D(C, 1x1x1)(x) -> InstanceNorm on the single-channel volume x [N][S],
 * fp32) WITHOUT materialising its output: w[c]*x + b[c] normalises to gamma[c]*w[c]*rs*(x - mean x) + beta[c] with
 * rs = (w[c]^2 var x + eps)^-1/2 (the convolution's bias cancels), i.e. the branch is  scale[n][c] * x + shift[n][c]  with
 *     scale = gamma*w*rs,   shift = beta - scale * mean x.
 * One launch: per-workgroup partial sums of x and x^2 in part[N][G][2] (doubles), fixed-order sum and the 2*N*C results by the
 * workgroup that draws the last of the N*G tickets (*ticket zero on entry, left at zero).  G = vg_stem_short_fwd_workgroups(N, S).
 * The consuming convolution adds the branch through vg_conv_desc::res_c1.  round16 as in vg_stem_short_bwd. */
int vg_stem_short_fwd_workgroups(int N, int64_t S);
int vg_stem_short_fwd(const float* x, int N, int64_t S, int C, const float* w, const float* gamma, const float* beta, float eps, int round16,
                      float* scale, float* shift, double* part, int G, unsigned* ticket, vg_stream_t stream);
/* The stem's shortcut in the backward pass (resunet_model.py:96-99: Conv3D(16, 1x1x1)(x) -> InstanceNorm, no activation; its input is the
 * single-channel volume, so no data gradient exists).  The branch's output w[c]*x + b[c] normalises to
 * xhat[c] = w[c]*rs[c]*(x - mean x), rs[c] = (w[c]^2 var x + eps)^-1/2: the loss sees w[c] only through eps, and with the two moments
 * R0 = sum_v g, T = sum_v g*x of the gradient g of the block output [N][S][C] (16-bit storage or fp32) against x [N][S] (fp32),
 *     dL/dw[c] += sum_n eps*gamma[c]*rs^3*(T - mean(x) R0),   dgamma[c] += sum_n w[c]*rs*(T - mean(x) R0),   dbeta[c] += sum_n R0,
 *     dL/db[c] = 0 identically
 * -- no apply pass, no gradient tensor, no weight-gradient launch, and no read of the stored branch output (whose 16-bit rounding the
 * 1/w of the older statistics-based form amplified to 6-13 % of this gradient).  Deterministic: part[N][G][2C+2] doubles receive one
 * partial sum per workgroup (fp32 inside a wave, double across waves), the workgroup drawing the last of the N*G tickets (*ticket zeroed by the caller) adds them in a fixed
 * order.  G = vg_stem_short_bwd_workgroups(N, S, C); C in {8, 16, 32, 64}.  w: the C kernel weights as the forward used them
 * (round16 != 0: rounded to the library's 16-bit storage format first). */
int vg_stem_short_bwd_workgroups(int N, int64_t S, int C);
int vg_stem_short_bwd(const void* g, int g_f32, const float* x, int N, int64_t S, int C, const float* w, const float* gamma, float eps,
                      int round16, float* dw, float* dgamma, float* dbeta, double* part, int G, unsigned* ticket, vg_stream_t stream);
/* dgamma[c] += sum_{stripes,n} red[.][n][c][1], dbeta[c] += sum red[.][n][c][0] */
int vg_in_param_grads(const float* red, int N, int C, float* dgamma, float* dbeta, vg_stream_t stream);

/* Backward of the virtual upsample+concat (resunet_model.py:175-181): g is bf16 [N][D][H][W][Cu+Cs];
 * dlow[N][D/2][H/2][W/2][Cu] (+)= sum of the 8 children, dskip[N][D][H][W][Cs] (+)= g[..., Cu:].
 * accumulate: bit 0 -- add to dlow (else overwrite), bit 1 -- add to dskip: the first writer of a gradient buffer overwrites,
 * so the buffers need no memset.  Cs == 0 (dskip ignored): the backward of a bare UpSampling3D (generator.py:58-66), a 2x2x2 sum-pool. */
int vg_concat_bwd(const void* g, int N, int D, int H, int W, int Cu, int Cs, void* dlow, void* dskip,
                  int f32, int accumulate, vg_stream_t stream);

/* The data gradient of a decoder block's 1x1x1 shortcut convolution (resunet_model.py:126-131 over the concat of :175-181) FUSED with
 * vg_concat_bwd: d is the descriptor of the accumulating data-gradient launch (src0 = gradient of the shortcut's output, out = the
 * gradient of the virtual concat [N][D][H][W][c_low + Cs] holding the convolution branch's part; it is only READ); the sums go to
 * dskip / (over every 2x2x2 block) dlow with vg_concat_bwd's accumulate bits -- the concat gradient is neither rewritten nor re-read
 * (804 -> 486 MB per application at 128^3).  Returns VG_OK when launched, 1 when the shape is not served (the caller then runs
 * vg_conv3d(d) + vg_concat_bwd), < 0 on error. */
int vg_shortcut_dgrad_concat(const vg_conv_desc* d, void* dlow, void* dskip, int c_low, int accumulate, vg_stream_t stream);
/* The same with the block's first convolution branch folded in: the concat gradient is never stored.  b describes the (InstanceNorm ->
 * act) backward of that convolution's input (g = its data gradient on the reflection-padded grid, x / x1 = the virtual concat's
 * sources, statistics already in b->red: vg_actnorm_bwd_stats or the data-gradient epilogue); the launch computes
 * dx = gamma * rstd * (dn - mean(dn) - xhat * mean(dn * xhat)) per voxel where vg_actnorm_bwd_apply would have written it, adds the
 * shortcut's data gradient, and writes dskip / dlow as above; d->out is not used; b->dgamma / b->dbeta are added as the apply pass does.
 * 838 -> 436 MB per application at 128^3.  Returns 1 when the shape is not served (caller: vg_actnorm_bwd_apply + the call above). */
int vg_shortcut_dgrad_concat_norm(const vg_conv_desc* d, const vg_actnorm_bwd_desc* b, void* dlow, void* dskip, int c_low,
                                  int accumulate, vg_stream_t stream);

/* out = act(a * a_scale + a_shift) + (b * b_scale + b_shift): layers.add([input_tensor, InstanceNorm(conv2)]) of the ResNet generator's
 * residual block (building_blocks.py:68-123; generator.py:52-56), both operands [N][S][C] bf16 (f32: float) with their pending on-read
 * affine [N][C] (NULL: none); a_act a VG_ACT_* applied to the first operand after its affine. */
int vg_affine_add(const void* a, const float* a_scale, const float* a_shift, int a_act, const void* b, const float* b_scale,
                  const float* b_shift, int N, int64_t S, int C, void* out, int f32, vg_stream_t stream);

/* db[c] += sum_rows dy[row][c]: the bias gradient of a layer from its output gradient dy [rows][C] (bf16, or float when f32).
 * Conv3D's comes out of vg_conv3d_wgrad; this entry serves the k2 s2 Conv3DTranspose of the 'deconv' decoder (resunet_model.py:168-174,
 * vnet_model.py:244-245), whose forward IS the strided data gradient of vg_conv3d (output-parity classes, one tap each, bias in the
 * epilogue), whose data gradient is the forward convolution with the same packed weights and whose kernel gradient is
 * vg_conv3d_wgrad with the roles of input and output gradient exchanged (van_gan_amd.ops.ConvTranspose3dK2S2 is the recipe). */
int vg_bias_grad(const void* dy, int f32, int64_t rows, int C, float* db, vg_stream_t stream);

/* Data gradient of a 4x4x4 stride-2 Conv3D over ReflectionPadding3D(1) of a SINGLE-channel volume (discriminator.py:50-60 under the tape,
 * vangan.py:433-438: the generator loss reaches the generators through it) as a stride-1 convolution over CELLS: cell c = the 2x2x2 block
 * of reflect-padded positions 2c + r, all of which draw from dY voxels c - 1 + n, n in {0,1} per axis, with tap r + 2 - 2n.
 * vg_pack_cell_weights: fp32 DHWIO kernel w [4][4][4][1][C] -> the packed operand (16-bit, [64][(C/16)*448]: rows 4rd+2rh+rw < 8, 27 taps
 * n - 1 in -1..1 of which the n = 2 ones are zero, CK = 16) of a vg_conv3d call with src0 = dY [N][D/2][H/2][W/2][C], zero padding,
 * OD/OH/OW = D/2+1 .., Cout = 16, out = cells.  vg_cells_fold: cells (16-bit [N][D/2+1][H/2+1][W/2+1][16]) -> dx fp32 [N][D][H][W]: depth to
 * space and the transpose of the reflection pad (positions 0 and n+1 fold onto 1 and n-2).  D, H, W even and >= 4. */
int vg_pack_cell_weights(const float* w, int C, void* out, vg_stream_t stream);
int vg_cells_fold(const void* cells, int N, int D, int H, int W, float* dx, vg_stream_t stream);

/* d_pre = dy * (1 - y*y)   (tanh output activation, resunet_model.py:245), all fp32 */
int vg_tanh_bwd(const float* dy, const float* y, float* dpre, int64_t n, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Loss kernels (fp32 single-channel volumes [B][S])
 * --------------------------------------------------------------------------------------------- */
/* mm[b] = (min, max, n_min, n_max) -- utils.py:27-48 */
int vg_minmax(const float* x, int B, int64_t S, float* mm4, vg_stream_t stream);
int vg_minmax_apply(const float* x, const float* mm4, int B, int64_t S, float* y, vg_stream_t stream);
/* dx = gy/(max-min) + [x==min] * sum(gy*(y-1))/(R n_min) - [x==max] * sum(gy*y)/(R n_max);
 * tmp2[b][2] is scratch (zeroed by the caller) */
int vg_minmax_bwd(const float* x, const float* y, const float* gy, const float* mm4, int B, int64_t S,
                  float* tmp2, float* dx, vg_stream_t stream);
/* BCE of loss_functions.py:185-190 on normalised volumes: acc[0] += sum bce; gp (+)= gscale*dbce/dp */
int vg_bce(const float* t, const float* p, int64_t n, float* acc, float gscale, float* gp, int accumulate,
           vg_stream_t stream);
/* acc[0] += sum (a-b)^2 ; gb (+)= gscale * 2 (b-a) -- loss_functions.py:56-68 */
int vg_mse(const float* a, const float* b, int64_t n, float* acc, float gscale, float* gb, int accumulate,
           vg_stream_t stream);
/* LSGAN terms on patch logits (loss_functions.py:273-274,306-308):
 * acc[0] += sum (target - x)^2 ; gx (+)= gscale * 2 (x - target); x bf16 or f32 */
int vg_mse_const(const void* x, int x_f32, float target, int64_t n, float* acc, float gscale, float* gx,
                 int accumulate, vg_stream_t stream);
/* Selectable cycle terms MAE / MSE / L4 (loss_functions.py:41-84,177-184), p in {1, 2, 4} (anything else: VG_EINVAL):
 * acc[0] += sum |b-a|^p ; gb (+)= gscale * p * |d|^(p-1) * sign(d), d = b-a, sign(0) = 0 (TP: tf.abs has gradient 0 at 0);
 * gb == NULL: forward only.  p = 2 gives vg_mse's values. */
int vg_lp_loss(const float* a, const float* b, int64_t n, int p, float* acc, float gscale, float* gb, int accumulate,
               vg_stream_t stream);
/* Selectable adversarial terms on patch logits (loss_functions.py:275-286,309-322 with from_logits=True); x bf16 or f32, target z in
 * {0, 1}, kind in {0, 1} (anything else: VG_EINVAL).  TP, restated from Keras 2.10:
 *   kind 0  BinaryCrossentropy(from_logits=True)      = max(x,0) - x z + log1p(exp(-|x|))
 *   kind 1  BinaryFocalCrossentropy(from_logits=True) = (1 - p_t)^2 * bce, p_t = z s + (1-z)(1-s), s = sigmoid(x)  (gamma 2, no balancing)
 * acc[0] += sum loss ; gx (+)= gscale * d loss / d x (closed forms, finite for every finite logit); gx == NULL: forward only. */
int vg_logit_loss(const void* x, int x_f32, float target, int kind, int64_t n, float* acc, float gscale, float* gx,
                  int accumulate, vg_stream_t stream);
/* SSIM (loss_functions.py:86-117): acc[0] += sum (1-ssim); part[3][B][S] = dL/d(mu_p, E[pp], E[tp]) */
int vg_ssim_fwd(const float* t, const float* p, int B, int D, int H, int W, float* acc, float* part,
                vg_stream_t stream);
int vg_ssim_bwd(const float* t, const float* p, const float* part, int B, int D, int H, int W, float gscale,
                float* gp, int accumulate, vg_stream_t stream);

/* clDice soft skeleton (clDice_func.py:8-80).  imgs: [iters+2][B][S] receives img_0..img_{iters+1}
 * (img_{j+1} = soft_erode(img_j)); skels: [iters+1][B][S] receives the skeleton after every step, the
 * last slab is soft_skel(img, iters).
 * aux == NULL (a skeleton that is not differentiated: the target's): the erosion chain runs two steps per launch on tiles held in LDS
 * with a 2-voxel halo, the skeleton recursion is one launch over the stored chain.
 * aux != NULL ((iters+1) * B*S * 6 bytes: [iters+1][B][S] float delta_j, then [iters+1][B][S] uint8 arg-max codes of the dilation in
 * delta_j = relu(img_j - dilate(img_{j+1})), then [iters+1][B][S] uint8 arg-min codes of the erosion img_{j+1} = erode(img_j); a code
 * is ((a+1)*3 + (b+1))*3 + (c+1) for the offset (a, b, c) along (D, H, W) of the FIRST extremum in TensorFlow's scan order, TP): the
 * forward pass files where every pooling gradient will go, and vg_soft_skel_bwd with the same aux routes by table lookup. */
int vg_soft_skel_fwd(const float* img, int B, int D, int H, int W, int iters, float* imgs, float* skels, void* aux,
                     vg_stream_t stream);
/* gimg += (d skel / d img)^T gskel.  aux != NULL (what vg_soft_skel_fwd filed): iters + 2 streaming launches, work = [4][B][S] scratch
 * (no initialisation needed); aux == NULL: two scan launches per step that recompute the arg-extrema from imgs, work = [3][B][S]. */
int vg_soft_skel_bwd(const float* imgs, const float* skels, const float* gskel, int B, int D, int H, int W,
                     int iters, float* work, float* gimg, const void* aux, vg_stream_t stream);
/* Dice + clDice combination (clDice_func.py:83-149, loss_functions.py:223-226) without a host sync.
 * sums7 = (sum skel_p*t, sum skel_p, sum t, sum skel_t*p, sum skel_t, sum p, sum t*p);
 * coef6: gskel_p = c0*t - c1;  gp += c2*t + c3 + c4*skel_t;  c5 = w*((1-alpha)*dice + alpha*clDice). */
int vg_cldice_coef(const float* sums7, float w, float alpha, float* coef6, vg_stream_t stream);
int vg_cldice_grads(const float* t, const float* skel_t, const float* coef6, int64_t n, float* gskel_p, float* gp,
                    int accumulate, vg_stream_t stream);
/* sums[k] += (sum a*b, sum a, sum b) over n elements */
int vg_dot_sums(const float* a, const float* b, int64_t n, float* sums3, vg_stream_t stream);
/* y (+)= alpha*a + beta*b (b may be NULL) */
int vg_axpby(const float* a, float alpha, const float* b, float beta, int64_t n, float* y, int accumulate,
             vg_stream_t stream);

/* Wasserstein mode -- what `wasserstein=True` of the reference trains once traced (its gradient penalty never reaches a weight: DESIGN.md
 * section 8): the discriminator's Flatten -> Dropout(0.2) -> Dense(1) head over the patch logits (discriminator.py:116-119),
 *   z[s] = b + sum_i w[i] * mask[s][i] * x[s][i]          (mask: dropout multipliers {0, 1/(1-rate)} or NULL),
 * its backward  dx[s][i] = gz[s] * mask[s][i] * w[i],  dw[i] += sum_s gz[s] * mask[s][i] * x[s][i],  db += sum_s gz[s]  (dx / dw / db
 * optional), and the loss terms of loss_functions.py:325-355 on z = [real (B); fake (B)]: acc2[0] += sum z_real, acc2[1] += sum z_fake,
 * gz_d[2B] = d(-reduce_mean(D(real) - D(fake)))/dz = (-inv ..., +inv ...), gz_g[B] = d(-reduce_mean(D(fake)))/dz_fake = -inv,
 * inv = 1 / (B * global batch size) (reduce_mean(axis=None) averages over the batch too, loss_functions.py:21-22). */
int vg_dense_head_fwd(const float* x, const float* mask, const float* w, const float* b, int N, int n, float* z, vg_stream_t stream);
int vg_dense_head_bwd(const float* x, const float* mask, const float* w, const float* gz, int N, int n, float* dx, float* dw, float* db,
                      vg_stream_t stream);
int vg_wasserstein_terms(const float* z, int B, float inv, float* acc2, float* gz_d, float* gz_g, vg_stream_t stream);

/* Sliding-window inference (GanMonitor.stitch_subvolumes, custom_callback.py:47-223): pred/cnt [X][Y][Z] fp32.
 * vg_overlap_add: pred[box] += window[crop], cnt[box] += 1 for the border-cropped box of one k^3 window at (x0,y0,z0)
 * (custom_callback.py:165-183); vg_divide_crop: out = pred/cnt on the un-padded sub-box (:192-200; 0/0 = NaN as numpy). */
int vg_overlap_add(const float* win, int kx, int ky, int kz, int px, int py, int pz, int x0, int y0, int z0,
                   int X, int Y, int Z, float* pred, float* cnt, vg_stream_t stream);
int vg_divide_crop(const float* pred, const float* cnt, int X, int Y, int Z, int sx, int sy, int sz, int ox, int oy,
                   int oz, float* out, vg_stream_t stream);
/* Batched forms for the blended / flip-averaged modes (beyond the reference; van_gan_amd/inference.py), fp32 in both storage builds.
 * tab: device table of B rows of four int32 (x0, y0, z0, flip); flip bit 0 mirrors x (the first axis of the [X][Y][Z] volume), bit 1 y,
 * bit 2 z:  f_a(i) = flip bit a ? k_a - 1 - i : i.  One launch per call, whatever B.
 * vg_window_gather:  out[b][i][j][k] = vol[x0 + f_x(i)][y0 + f_y(j)][z0 + f_z(k)],  out [B][kx][ky][kz]  (a copy: bit-exact).
 * vg_window_scatter: for every row b and every voxel px <= i < kx - px (likewise y, z; window coordinates in VOLUME orientation)
 *   v = win[b][f_x(i)][f_y(j)][f_z(k)]  (un-flips the prediction),  w = (wx[i] * wy[j]) * wz[k]  (fp32; per-axis tables of k_a floats),
 *   atomicAdd(pred[x0+i][y0+j][z0+k], w * v),  atomicAdd(cnt[...], w).  wx == wy == wz == NULL: w = 1, pred += v, what vg_overlap_add adds.
 *   vg_divide_crop then divides by the summed weights.  Float atomics: the sums depend on arrival order in their last bits.
 * VG_EINVAL (nothing launched): a NULL pointer, B < 1, k_a < 1, k_a > the volume extent, p_a < 0, k_a - 2 p_a < 1, one or two of the
 * three weight tables.  The table is on the device and is the caller's to validate (origins in [0, extent - k_a], flip in 0..7); a row
 * outside those ranges is skipped by the kernels and never dereferenced. */
int vg_window_gather(const float* vol, int X, int Y, int Z, const int* tab, int B, int kx, int ky, int kz, float* out,
                     vg_stream_t stream);
int vg_window_scatter(const float* win, const int* tab, int B, int kx, int ky, int kz, int px, int py, int pz, const float* wx,
                      const float* wy, const float* wz, int X, int Y, int Z, float* pred, float* cnt, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-tensor Adam with per-tensor clip-by-norm (tf.keras.optimizers.Adam(2e-4, 0.5, 0.9,
 * clipnorm=100), vangan.py:220-235, applied by optimizer.minimize at vangan.py:426-438).
 * w,g,m,v: flat fp32 buffers of `total` elements; seg_off[T+1] tensor boundaries (device int64);
 * norms[T + 2 * ceil(total / 4096)] scratch (T squared norms, then per-block partial sums: the norms
 * are added in a fixed order, so replicas holding the same reduced gradients apply bit-identical
 * updates).  grad_scale multiplies g before clipping (1/world for mean, 1 for the reference's SUM
 * all-reduce).
 * --------------------------------------------------------------------------------------------- */
int vg_adam_clip(float* w, const float* g, float* m, float* v, const int64_t* seg_off_dev, int T,
                 int64_t total, float* norms, float lr_t, float beta1, float beta2, float eps,
                 float clipnorm, float grad_scale, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Spectral normalisation of the discriminator's wrapped convolution kernels (get_discriminator(use_SN=True), discriminator.py:16,54-61,
 * 86,100; building_blocks.py:172-180 -- tfa.layers.SpectralNormalization with power_iterations = 1), multi-tensor: one call serves every
 * wrapped kernel of a network from a device table.  TP (TensorFlow Addons, restated): w is the fp32 master kernel in Keras layout viewed
 * as [K = k^3 * Cin][Cout], u [Cout] the stored power-iteration vector; one projection is
 *   l2n(x) = x * rsqrt(max(sum(x * x), 1e-12));  v = l2n(u w^T);  u' = l2n(v w);  sigma = (v w) . u';  u <- u';  w <- w / sigma   (in place).
 * n_proj (1 .. VG_SN_MAX_PROJ) projections are applied back to back (the reference calls a discriminator twice per training step); w is
 * read n_proj + 1 times and written once.  state[VG_SN_STATE]: [p] = sigma of projection p of this call, [VG_SN_STATE_CUM] = the factor
 * w was multiplied by, 1 / (sigma_0 ... sigma_{n_proj - 1}).  sigma = 0 (an all-zero w or u) makes that projection the identity: w and u
 * stay as they are, state[p] = 0, nothing is divided by zero and no NaN appears.
 * Served shapes: Cout in {64, 128, 256, 512}, K * Cout a multiple of 256, w and u 16-byte aligned (vg_spectral_norm_blocks returns
 * VG_EINVAL otherwise).  Item i owns the workgroups [blk0, blk0 + nblk), nblk = vg_spectral_norm_blocks(K, Cout) (VG_SN_SLAB weights
 * each); the ranges tile [0, total_blocks) in item order.  scratch: caller-owned, vg_spectral_norm_scratch_bytes(total_blocks) bytes,
 * 16-byte aligned; nothing is allocated and the call only enqueues.  No floating-point atomics: every sum has one fixed association,
 * so equal inputs give bit-identical w, u and sigma on every run and on every rank.
 * --------------------------------------------------------------------------------------------- */
#define VG_SN_MAX_ITEMS 8
#define VG_SN_MAX_PROJ 4
#define VG_SN_MAX_COUT 512
#define VG_SN_SLAB 65536
#define VG_SN_STATE 8
#define VG_SN_STATE_CUM 4
typedef struct {
    float* w; float* u; float* state;
    int32_t K, Cout;
    int32_t blk0, nblk;
} vg_sn_item;
int vg_spectral_norm_blocks(int K, int Cout);
int64_t vg_spectral_norm_scratch_bytes(int total_blocks);
int vg_spectral_norm(const vg_sn_item* items_dev, int T, int total_blocks, int n_proj, float* scratch, int64_t scratch_bytes,
                     vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention gate of the ResUNet decoder (ResUNet(use_attention_gate=True), resunet_model.py:178-179 / vnet_model.py:24-77), restated:
 *   q = relu(skip . w_theta + b_theta + phi[parent]);  h = sigmoid(q . w_psi + b_psi);  gated = skip * h.
 * skip / gated / dg / dskip [N][D][H][W][Cs], phi / dphi [N][D/2][H/2][W/2][Ci] (the 1x1x1 convolution of the low-resolution tensor, its
 * bias included: it commutes with UpSampling3D(2) and is read through the parent index), all in the build's 16-bit format or, f32 != 0,
 * float32 (exact-parity mode); h [N][D][H][W] float32; w_theta [Cs][Ci], b_theta [Ci], w_psi [Ci], b_psi [1] are the fp32 master
 * parameters in Keras layout (rounded to the storage format on the matrix pipe; 4-byte alignment suffices).
 * Served shapes: D, H, W even, (Cs, Ci) in {(16, 32), (32, 64), (64, 128), (128, 256)}; tensors 16-byte aligned; else VG_EINVAL.
 * vg_attn_gate_fwd also ADDS the per-(n, c) (sum, sum of squares) of the STORED gated values into sums [VG_STRIPES][N][Cs][2].
 * vg_attn_gate_bwd recomputes q, writes dskip = dg * h + dq . w_theta^T (accumulate != 0: adds to what dskip holds), dphi = the sum of
 * dq over the 8 children of each low-resolution voxel, and ADDS dw_theta, db_theta, dw_psi, db_psi (reduced per workgroup on chip, then
 * one float atomic per workgroup and destination: the sums' last bits may differ from run to run).
 * Neither call allocates or synchronises.
 * --------------------------------------------------------------------------------------------- */
int vg_attn_gate_fwd(const void* skip, const void* phi, const float* w_theta, const float* b_theta, const float* w_psi,
                     const float* b_psi, int N, int D, int H, int W, int Cs, int Ci, int f32, void* gated, float* h, float* sums,
                     vg_stream_t stream);
int vg_attn_gate_bwd(const void* dg, const void* skip, const float* h, const void* phi, const float* w_theta,
                     const float* b_theta, const float* w_psi, int N, int D, int H, int W, int Cs, int Ci, int f32, void* dskip,
                     int accumulate, void* dphi, float* dw_theta, float* db_theta, float* dw_psi, float* db_psi,
                     vg_stream_t stream);

/* The three entry points whose per-step host scalars change from step to step -- the Philox counter, the noise standard deviation
 * (GanMonitor decays it per epoch, custom_callback.py:413-424) and Adam's bias-corrected rate lr_t -- with those scalars read from
 * DEVICE memory: a HIP graph captured over one VanGan.train_step (vangan.py:380-440) is then replayable, the host refreshing a
 * 32-byte parameter block before each replay instead of re-enqueueing ~900 launches.  offset = *offset_dev + offset_add. */
int vg_randn_bf16_dev(void* out, int64_t n, const float* std_dev, uint64_t seed, const uint64_t* offset_dev, uint64_t offset_add,
                      vg_stream_t stream);
int vg_dropout_mask_dev(float* out, int64_t n, float rate, uint64_t seed, const uint64_t* offset_dev, uint64_t offset_add,
                        vg_stream_t stream);
int vg_adam_clip_dev(float* w, const float* g, float* m, float* v, const int64_t* seg_off_dev, int T, int64_t total, float* norms,
                     const float* lr_t_dev, float beta1, float beta2, float eps, float clipnorm, float grad_scale, vg_stream_t stream);

/* Writes that 32-byte parameter block: bytes [0, 8) the Philox counter base, [8, 12) the noise standard deviation, [16, 32) lr_t of
 * gen_IS, gen_SI, disc_I, disc_S (the reference's four optimizers, vangan.py:220-235).  The values travel as KERNEL ARGUMENTS, i.e. they
 * are bound at enqueue time: a host that enqueues step N+1 before step N has executed cannot disturb step N (block: 8-byte aligned). */
int vg_set_step_params(void* block, uint64_t offset, float std, float lr0, float lr1, float lr2, float lr3, vg_stream_t stream);

/* Stand-in for the RCCL SUM all-reduce of a gradient bucket (the implicit all-reduce of optimizer.minimize under MirroredStrategy,
 * vangan.py:426-438; main.py:22) on a box with ONE GPU, so that the data-parallel schedule -- communication stream, per-bucket
 * events, early suffix pieces, cross-step optimizer overlap -- can be timed without a second device: `workgroups` workgroups (RCCL
 * channels) move buf[0, n) to scratch and back (2 x 4n bytes read + written, buf ends bit-identical; n a multiple of 4, both
 * pointers 16-byte aligned) and then hold their CUs until min_us microseconds of wall clock have passed since they started (the
 * time a ring over xGMI would take for the message; 0: none).  Never part of a real multi-GPU run. */
int vg_local_exchange(float* buf, float* scratch, int64_t n, int workgroups, int min_us, vg_stream_t stream);

/* N(0,std) noise as bf16 and SpatialDropout3D channel masks {0,1/(1-rate)} (fp32), counter-based RNG */
int vg_randn_bf16(void* out, int64_t n, float std, uint64_t seed, uint64_t offset, vg_stream_t stream);
int vg_dropout_mask(float* out, int64_t n, float rate, uint64_t seed, uint64_t offset, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training data pipeline on resident volumes (DatasetGen.process_imaging_domain / process_seg_domain /
 * random_spatial_augmentation, dataset.py:205-251).  vol: fp32 [X][Y][Z][C]; out: fp32 [px][py][pz][C].
 * vg_crop_augment: out = rot90_k( flip_up_down?( flip_left_right?( vol[x0:x0+px, y0:y0+py, z0:z0+pz] ))) with the
 *   tf.image semantics the reference gets on 4-D tensors: X is a batch axis, "height" = Y, "width" = Z, i.e.
 *   flip_left_right reverses Z, flip_up_down reverses Y, rot90 turns the (Y,Z) plane counter-clockwise k times
 *   (k is taken modulo 4; odd k needs py == pz).  The random draws stay with the caller.
 * vg_crop_max: out[0] = max over the crop box (the seg-domain rejection test reduce_max(arr) < 0.8, dataset.py:242).
 * --------------------------------------------------------------------------------------------- */
int vg_crop_augment(const float* vol, int X, int Y, int Z, int C, int x0, int y0, int z0, int px, int py, int pz,
                    int flip_lr, int flip_ud, int rot_k, float* out, vg_stream_t stream);
int vg_crop_max(const float* vol, int X, int Y, int Z, int C, int x0, int y0, int z0, int px, int py, int pz,
                float* out, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Raw-volume preprocessing (preprocess_rsom_images, main.py:127-150, then min_max_norm and (x - 0.5) / 0.5 of process_tiff,
 * preprocessing.py:179-185), restated; van_gan_amd/preprocess.py, csrc/vg_preproc.hip, DESIGN.md section 3.12.  The same code in both
 * storage builds.  vol: [X][Y][Z] with Z innermost, nxy = X * Y, n = nxy * Z; dtype is one of VG_PP_U8 / VG_PP_U16 / VG_PP_F32 (a raw
 * 8- or 16-bit stack is read as it is).  Every entry only enqueues, allocates nothing and checks its arguments on the host before any
 * launch (VG_EINVAL, nothing launched): NULL pointers, nxy < 1 or >= 2^40, Z < 1 or > 2^20, an unknown dtype, a scratch smaller than
 * its query says, and what is listed per entry.  Only integer atomics: equal inputs give bit-identical results on every run.
 *
 * vg_slice_moments: mean_std[z] = (mean, population standard deviation) of vol[:, :, z], accumulated in fp64 as sums of (x - vol[0][0][z])
 *   and of its square -- the pivot keeps E[d^2] - E[d]^2 free of cancellation and makes a constant slice give exactly 0 -- per workgroup
 *   into the caller's scratch (vg_slice_moments_scratch_bytes(nxy, Z) bytes, 16-byte aligned), summed in a fixed order by a second
 *   kernel and rounded once to fp32.
 * vg_zscore_slices: out = s > 0 ? (x - m) / s : x - m in fp32 with (m, s) = mean_std[z]; ADDS the number of non-finite values written to
 *   *nonfinite (one integer atomic per workgroup; zeroed by the caller).
 * vg_order_stats: out[r] = sorted(x)[ranks[r]] for r < R (exact; -0.0 sorts before +0.0), x fp32 [n] of finite values (a NaN is ordered
 *   by its bit pattern: beyond the infinity of its sign).  ranks is a HOST array; 1 <= R <= VG_PP_MAX_RANKS, 1 <= n < 2^31,
 *   0 <= ranks[r] < n, duplicates allowed.  A most-significant-digit radix select, 8 bits per pass, on the order-preserving key of the
 *   float's bits: per pass a histogram kernel over the whole array and a one-workgroup kernel that picks the bin; 9 launches whatever the
 *   data, no host read-back.  scratch: vg_order_stats_scratch_bytes(n, R) bytes, 16-byte aligned, contents irrelevant on entry.
 * vg_clip_rescale: stats4 = the order statistics (a[i], a[i+1], a[j], a[j+1]) on the device; the limits are formed as
 *   scipy.stats.scoreatpercentile does, in fp64 with every operation rounded, lp = a[i] * (1 - f_lo) + a[i+1] * f_lo (up likewise from
 *   f_hi; 0 <= f <= 1), rounded once to fp32 and written to limits2.  c = z < lp ? lp : z > up ? up : z, and
 *   out = rescale ? ((c - lp) / (up - lp) - 0.5) / 0.5 : c in fp32, each operation rounded (rescale is 0 or 1).  out may be z itself.
 * --------------------------------------------------------------------------------------------- */
#define VG_PP_U8 0
#define VG_PP_U16 1
#define VG_PP_F32 2
#define VG_PP_MAX_RANKS 4
int64_t vg_slice_moments_scratch_bytes(int64_t nxy, int Z);
int vg_slice_moments(const void* vol, int dtype, int64_t nxy, int Z, float* mean_std, void* scratch, int64_t scratch_bytes,
                     vg_stream_t stream);
int vg_zscore_slices(const void* vol, int dtype, int64_t nxy, int Z, const float* mean_std, float* out, uint32_t* nonfinite,
                     vg_stream_t stream);
int64_t vg_order_stats_scratch_bytes(int64_t n, int R);
int vg_order_stats(const float* x, int64_t n, const int64_t* ranks_host, int R, float* out, void* scratch, int64_t scratch_bytes,
                   vg_stream_t stream);
int vg_clip_rescale(const float* z, int64_t n, const float* stats4, double f_lo, double f_hi, int rescale, float* limits2, float* out,
                    vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Volume resize (resize_volume, utils.py:224-255: cv2.resize(..., INTER_LANCZOS4) slice by slice), restated; van_gan_amd/preprocess.py
 * (lanczos4_table, resize_volume), csrc/vg_resample.hip, DESIGN.md section 3.13.  fp32, the same code in both storage builds.
 * TP, unverifiable here: the filter below restates OpenCV's float32 single-channel Lanczos-4 resize from its published source; OpenCV
 * itself was never run against this code.
 *
 * The filter of one axis, source length L -> target length T, built on the HOST (van_gan_amd.preprocess.lanczos4_table):
 *   scale = 1.0 / (T / L) in fp64; for dx = 0 .. T-1: fx = (float)((dx + 0.5) * scale - 0.5), sx = floor(fx), t = fx - (float)sx in fp32;
 *   first[dx] = sx - 3 (unclamped: -3 .. L + 3 occur); the 8 taps read source indices clamp(first[dx] + k, 0, L - 1), k = 0 .. 7 (OpenCV
 *   replicates the edge).  Coefficients of a phase t: t < FLT_EPSILON gives the unit tap at k = 3; else, in fp64, y_k = -(t + 3 - k) * pi / 4,
 *   c_k = (float)((-1)^k sin(y_k) / y_k^2) -- formed, as OpenCV forms it, from sin y_0, cos y_0 and the eighth-turn table
 *   {(1,0), (-s,-s), (0,1), (s,-s), (-1,0), (s,s), (0,-1), (-s,s)}, s = sqrt(1/2) -- S = c_0 + ... + c_7 in fp32 in that order and
 *   w_k = c_k * (float)(1 / S) in fp32: sinc(u) sinc(u / 4) at u = t + 3 - k, normalised to sum 1.
 * A volume [X][Y][Z] is resized by up to three passes with fp32 intermediates in the order Y, X, Z (OpenCV's 2-D resize runs columns, then
 * rows; the reference resizes every z-slice, then every x-slab); an axis whose lengths are equal is skipped by the host.
 *
 * vg_resample_axis: one pass.  The volume is viewed as [outer][L][inner] -> [outer][T][inner]:
 *   out[o][j][i] = sum_k w8[j][k] * x[o][clamp(first[j] + k, 0, L - 1)][i],  acc = w8[j][0] * x_0, then fmaf in tap order (fp32).
 *   The passes of [X][Y][Z] -> [T0][T1][T2] are (outer, L, inner) = (X, Y, Z), (1, X, T1 * Z), (T0 * T1, Z, 1).  first: int32 [T] and w8:
 *   fp32 [T][8] on the device; the clamp is applied by the kernel, so no table content can make a read leave its row.  inner >= 2 runs a
 *   kernel whose lanes take neighbouring i (16-byte accesses when inner % 4 == 0 and x, out are 16-byte aligned, else 4-byte); inner == 1
 *   stages whole rows in LDS (rows of more than 1023 floats are read from global memory directly).  Only enqueues, allocates nothing, keeps no
 *   state, no atomics: equal inputs give equal bits.  A tap of weight 0 contributes +-0, so an identity table copies every value bit for bit
 *   except that a -0.0 may come out as +0.0.  VG_EINVAL (nothing launched): a NULL pointer; outer, inner, L or T < 1; L or T > 2^20;
 *   outer * max(L, T) * inner >= 2^40; out == x; a pointer that is not 4-byte aligned.
 * --------------------------------------------------------------------------------------------- */
int vg_resample_axis(const float* x, int64_t outer, int L, int64_t inner, int T, const int32_t* first, const float* w8, float* out,
                     vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Label-volume preprocessing (the partition 'S' branch of process_tiff, preprocessing.py:173-189: min_max_norm, inversion when
 * scipy.stats.mode of the normalised stack is 1, (x - 0.5) / 0.5, binarise), restated; van_gan_amd/preprocess.py (value_mode,
 * prepare_segmentation), csrc/vg_labelprep.hip, DESIGN.md section 3.14.  fp32, the same code in both storage builds.  Every entry only
 * enqueues, allocates nothing, reads nothing back and checks its arguments on the host before any launch (VG_EINVAL, nothing launched):
 * a NULL pointer (mm4_or_null excepted), n < 1 or n >= 2^31, a pointer that is not 4-byte aligned, a scratch smaller than its query says
 * or not 16-byte aligned.  Only integer atomics, and every reduction is an integer sum or maximum: equal inputs give bit-identical
 * results on every run, whatever slot of the table a value lands in.  Every probe loop is bounded by the slot count of its table, and no
 * workgroup waits on another.
 *
 * vg_value_mode: the exact mode of the n values of x -- the most frequent value, and among equally frequent values the numerically
 *   smallest (scipy.stats.mode(x, axis=None)); -0.0 and +0.0 are one value, reported as +0.0.  mm4_or_null != NULL: the row
 *   (min, max, ., .) vg_minmax wrote, on the device; the values counted are then y = (x - min) / (max - min), formed on the fly in fp32
 *   with each of the three operations rounded (no reciprocal, no contraction) -- the normalisation is not injective in fp32, so the mode
 *   of y is not the image of the mode of x.  result4 (device): [0] the mode's fp32 bits, [1] its count, [2] status -- 0 ok, bit 0 the
 *   table overflowed (cannot happen with the scratch the query asks for), bit 1 max > min does not hold while normalising -- [3] the
 *   number of non-finite values met, which are counted here and never inserted; when no value is finite, [0] is a NaN and [1] is 0.
 *   n < 2^31: 32-bit counts cannot overflow.  scratch: vg_value_mode_scratch_bytes(n) bytes, 16-byte aligned, contents irrelevant on
 *   entry: a 64-byte header and an open-addressing table of 2^k >= 2 n slots of (32-bit key, 32-bit count), the empty key a NaN pattern.
 *   Four launches whatever the data: fill the table; count -- 0 and 1 in registers, one atomic each per workgroup; every other value
 *   through a combiner of VG_MODE_LDS_SLOTS slots in LDS that is flushed with one global insert per occupied slot, a value that finds
 *   the combiner full going to the table directly; 16-byte loads when x is 16-byte aligned --; a 64-bit integer maximum of
 *   (count << 32 | inverted order key) over the table; one thread that folds in the counts of 0 and 1 and writes result4.
 * vg_label_finish: y = (x - min) / (max - min) from mm4; when result4 says the mode is 1.0 with status 0, y = |y - 1|; z = (y - 0.5) / 0.5;
 *   out = z < 0 ? -1 : +1 -- fp32, each operation rounded.  Every thread reads the decision from result4 on the device.  out may be x.
 *   state: 8 words on the device; [0] is left alone (the caller's non-finite counter), [1] 1 when inverted else 0, [2], [3] the bits of
 *   (min, max), [4..7] a copy of result4 -- what one optional read-back needs.  When min == max the output is unspecified (the kernel still
 *   terminates and writes only inside out and state).
 * The clamp to [0, 255] the reference applies to a resized label stack is vg_clip_rescale with stats4 = (0, 0, 255, 255), fractions 0 and
 * rescale = 0.
 * --------------------------------------------------------------------------------------------- */
#define VG_MODE_LDS_SLOTS 1024
int64_t vg_value_mode_scratch_bytes(int64_t n);
int vg_value_mode(const float* x, int64_t n, const float* mm4_or_null, uint32_t* result4, void* scratch, int64_t scratch_bytes,
                  vg_stream_t stream);
int vg_label_finish(const float* x, int64_t n, const float* mm4, const uint32_t* result4, float* out, uint32_t* state,
                    vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Imaging filters (scipy.ndimage.median_filter and threshold_outliers, utils.py:108-133, both brought in by the reference's driver,
 * main.py:34-36), restated; van_gan_amd/preprocess.py (median_filter, volume_moments, outlier_limits, threshold_outliers),
 * csrc/vg_filters.hip (vg_volume_moments: csrc/vg_preproc.hip), DESIGN.md section 3.15.  The same code in both storage builds.  vol: [X][Y][Z] with Z innermost, n = X * Y * Z;
 * dtype is one of VG_PP_U8 / VG_PP_U16 / VG_PP_F32 and the values are converted to fp32 exactly.  Every entry only enqueues, allocates
 * nothing and checks its arguments on the host before any launch (VG_EINVAL, nothing launched): NULL pointers, an unknown dtype, a
 * pointer that is not aligned for its type, a scratch smaller than its query says, and what is listed per entry.  Only integer atomics:
 * equal inputs give bit-identical results on every run.  No result depends on what an output or scratch buffer held before, the
 * non-finite counters excepted, which are ADDED to and zeroed by the caller (as vg_zscore_slices' is).
 *
 * vg_median3: out[x][y][z] = the value of rank m / 2 (0-based) among the m = sx * sy * sz values of the window centred on the voxel;
 *   each of sx, sy, sz is 1 (no neighbours along that axis) or 3, anything else is VG_EINVAL.  (3,3,3) is the 3-D median, (3,3,1) the
 *   median of every z-slice.  The boundary is scipy's default mode='reflect': index -1 reads index 0 and index n reads index n - 1, so an
 *   axis of length 1 reads its only element three times.  The result is one of the inputs, hence exact.  *nonfinite has the number of
 *   non-finite voxels of vol ADDED to it (each counted once, at its own position); where a window holds a NaN the output value is
 *   unspecified (scipy's is order-dependent there).  X, Y >= 1, X * Y < 2^40, 1 <= Z <= 2^20; out (n floats) must not overlap vol.
 * vg_volume_moments: mean_std[0..1] = (mean, population standard deviation) of the n values, accumulated as vg_slice_moments does: fp64
 *   sums of (x - vol[0]) and of its square (a constant volume gives exactly 0) per workgroup into the caller's scratch
 *   (vg_volume_moments_scratch_bytes(n) bytes, 16-byte aligned), summed in a fixed order by a second kernel, rounded once to fp32.
 *   1 <= n < 2^60.
 * vg_outlier_limits: with (m, s) = mean_std read on the device, a voxel is kept when fabsf((x - m) / s) <= threshold in fp32, every
 *   operation rounded and the division correctly rounded; a NaN compares false, so a NaN voxel is never kept and no voxel is when s is 0
 *   or not finite.  stats4 = (lo, lo, hi, hi), lo / hi the smallest / largest kept value -- taken by integer atomic min / max on the
 *   order-preserving key of vg_order_stats, held in stats4 itself meanwhile, and converted by a last one-thread kernel -- laid out for
 *   vg_clip_rescale with fractions 0.  kept_nonfinite2[0] = the number of kept voxels, saturating at 2^32 - 1; kept_nonfinite2[1] has the
 *   number of non-finite voxels ADDED to it.  No kept voxel: stats4 = (+inf, +inf, -inf, -inf).  threshold must be finite and > 0;
 *   1 <= n < 2^60.  Three launches whatever the data.
 * --------------------------------------------------------------------------------------------- */
int vg_median3(const void* vol, int dtype, int X, int Y, int Z, int sx, int sy, int sz, float* out, uint32_t* nonfinite,
               vg_stream_t stream);
int64_t vg_volume_moments_scratch_bytes(int64_t n);
int vg_volume_moments(const void* vol, int dtype, int64_t n, float* mean_std, void* scratch, int64_t scratch_bytes, vg_stream_t stream);
int vg_outlier_limits(const void* vol, int dtype, int64_t n, const float* mean_std, float threshold, float* stats4,
                      uint32_t* kept_nonfinite2, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Prediction post-processing (what a user does with the stitched prediction, 255 * minmax(pred), that stitch_subvolumes returns where the
 * reference writes a TIFF, custom_callback.py:202-223): threshold, 3-D connected components, removal of small components;
 * van_gan_amd/postprocess.py (binarise_prediction, label_components, remove_small_objects, vessel_mask), csrc/vg_components.hip,
 * DESIGN.md section 3.16.  The same code in both storage builds.  Volumes are [X][Y][Z] with Z innermost, n = X * Y * Z, 1 <= n < 2^31;
 * masks are uint8 (0 is background, anything else foreground; the entries write 0 / 1), labels are int32.  Every entry only enqueues,
 * allocates nothing and checks its arguments on the host before any launch (VG_EINVAL, nothing launched): NULL pointers (those named
 * _or_null excepted), n out of range, a pointer that is not aligned for its type, a scratch smaller than its query says or not 16-byte
 * aligned, and what is listed per entry.  Only integer atomics, and every result is an integer that does not depend on their order:
 * equal inputs give bit-identical results on every run.  No workgroup waits on another, and every loop is bounded.
 *
 * vg_cc_label: labels[v] = 0 where mask[v] == 0, else the number 1 .. K of v's connected component under
 *   scipy.ndimage.generate_binary_structure(3, connectivity): connectivity 1 / 2 / 3 joins the 6 / 18 / 26 neighbours that differ by 1
 *   along at most 1 / 2 / 3 axes.  Components are numbered in raster order of their first voxel (ascending smallest linear index), which
 *   is scipy.ndimage.label's numbering.  sizes[k] = voxels of component k for k = 1 .. K and sizes[0] = background voxels; sizes has room
 *   for n / 2 + 2 words (no connectivity allows more than ceil(n / 2) components); entries beyond K are left alone.
 *   result4 = (K, status, foreground voxels, 0); status 0 is success, bit 0: a loop ran into its cap, bit 1: a parent above its child
 *   was read -- neither can happen on intact scratch; the kernels then leave the loop, and labels / sizes are unspecified but every write
 *   stays inside its buffer.  mask is only read.  scratch: vg_cc_scratch_bytes(n) bytes, contents irrelevant on entry.
 *   VG_EINVAL also when ceil(X / VG_CC_TILE_X) * ceil(Y / VG_CC_TILE_Y) * ceil(Z / VG_CC_TILE_Z) * 256 >= 2^32: one 256-thread workgroup
 *   runs per tile and a grid holds fewer than 2^32 threads, so a volume of more than 2^24 - 1 tiles -- (2^27, 1, 1), say -- is refused.
 *   Union-find with links to the smaller index only.  Six launches whatever the data: union-find in LDS over tiles of VG_CC_TILE_X x
 *   VG_CC_TILE_Y x VG_CC_TILE_Z voxels; links across tile faces by returning agent-scope atomic minima; roots and sizes (one atomic per
 *   tile-local component) with the count of roots per block of 2048 voxels; a one-workgroup scan of those counts; rank = label of every
 *   root, with its size; labels.
 * vg_cc_filter: out[v] = labels[v] != 0 && sizes[labels[v]] >= min_size (0 / 1).  K is read from result4[0] on the device.
 *   counts2 = (kept voxels, kept components K').  newid_or_null: room for n / 2 + 2 words; newid[k] = the number 1 .. K' of component k
 *   among the kept ones in the same order, 0 when it is dropped (newid[0] = 0); relabel_or_null (needs newid): relabel[v] =
 *   newid[labels[v]].  Two launches: one workgroup over sizes, one streaming pass (16-byte loads where labels, out and relabel allow).
 *   labels, out and relabel must not overlap; 0 <= min_size.
 * vg_hist256: hist[b] = number of finite voxels with (uint8)pred == b, the conversion being C truncation of the fp32 value -- the
 *   reference's pred.astype('uint8') (custom_callback.py:205) -- of a value in [0, 256); a finite value below 0 counts in bin 0 and one
 *   from 256 on in bin 255.  hist (256 words) is overwritten; *nonfinite has the number of non-finite voxels ADDED to it (zeroed by the
 *   caller).  Bins are kept per workgroup in LDS and reach hist as one atomic per occupied bin per workgroup.  1 <= n < 2^31.
 * vg_threshold_mask: mask[v] = as_u8 ? (uint8)pred[v] > t : pred[v] > t (0 / 1; the comparison in fp32, the conversion as above), where
 *   t = *t_dev_or_null when that is given, else the host value t.  A non-finite voxel is background and is ADDED to *nonfinite.
 *   otsu = 1: hist256 (the 256 words vg_hist256 wrote) must be given; one thread computes Otsu's threshold from it in fp64 -- with
 *   h = hist and b = 0 .. 255, weight1 = cumsum(h), weight2 = cumsum(h[::-1])[::-1], mean1 = cumsum(h b) / weight1, mean2 =
 *   (cumsum((h b)[::-1]) / weight2[::-1])[::-1], var12 = weight1[:-1] weight2[1:] (mean1[:-1] - mean2[1:])^2 evaluated left to right, every
 *   operation rounded on its own (the sums are integers below 2^53, hence exact), var12 = 0 where a weight is 0; t = the first index of
 *   the maximum of var12 -- writes it (as fp32) to *t_otsu, and the mask is (uint8)pred > t; as_u8, t and t_dev_or_null are ignored.
 *   An empty or one-bin histogram gives t = 0.
 *
 * Measuring the mask (csrc/vg_edt.hip; distance_transform_edt, fill_holes, vessel_radius):
 * vg_edt: the exact Euclidean distance of every voxel to the nearest background voxel (mask[v] == 0), 0 on the background, as
 *   scipy.ndimage.distance_transform_edt(mask, sampling).  Needs X^2 + Y^2 + Z^2 < 2^31 beside 1 <= n < 2^31 (VG_EINVAL otherwise), so
 *   that every squared distance in voxel units is an int32.  sampling3_or_null = NULL: integer form -- squared distances in int32 by
 *   three separable passes (along Z: (z - z')^2 to the nearest background voxel of the row; along Y, then X: min over p' of f(p') +
 *   (p - p')^2), the sentinel 2^31 - 1 standing for "no background voxel met" and never taking part in a sum.  out_kind
 *   VG_EDT_SQUARED_I32 writes them (int32[n]); VG_EDT_DIST_F32 writes float[n], the fp32 rounding of the fp64 square root.  A volume
 *   without any background voxel gives 2^31 - 1 / +inf everywhere (scipy's result is not meaningful there).  sampling3 = three doubles
 *   IN HOST MEMORY, read before the call returns: the voxel spacing along X, Y, Z, each finite and > 0; the same passes on fp64 costs
 *   f + s_a^2 (p - p')^2, every product and sum rounded on its own, sentinel +inf; VG_EDT_DIST_F32 only.  out is 4-byte aligned.
 *   scratch: vg_edt_scratch_bytes(X, Y, Z, weighted) bytes (two cost arrays: 8 bytes per voxel, 16 weighted), contents irrelevant.
 *   Three launches whatever the data; no atomics; bit-identical on every run.
 * vg_fill_holes_mark / vg_fill_holes_apply: scipy.ndimage.binary_fill_holes with its default structure, given labels = vg_cc_label of
 *   the INVERTED mask (1 where mask is 0) at connectivity 1.  mark: zeroes flags -- n / 2 + 2 BYTES, one per possible label -- and
 *   sets flags[l] = 1 for every label l >= 1 met on one of the six faces of the volume (plain stores of one value).  apply:
 *   out[v] = mask[v] != 0 || !flags[labels[v]] (0 / 1); a label outside [1, n / 2 + 2) is never used as an index.  out and mask must not overlap; 16-byte loads where labels, mask and out allow.
 *
 * The centreline (csrc/vg_skeleton.hip; skeletonize, skeleton_nodes, vessel_centreline): exact topological
 * thinning of the mask to a curve skeleton, one voxel wide, with the topology of the mask.  THE ALGORITHM.  Foreground is mask != 0 and
 * is 26-connected; everything outside the volume is background, which is 6-connected.  The neighbourhood of a voxel p is its 27-bit
 * code: bit 9 (dx + 1) + 3 (dy + 1) + (dz + 1) is the foreground state of p + (dx, dy, dz), bit 13 (p itself) taken as 0.  p is SIMPLE
 * when T26(p) = 1 and T6bar(p) = 1 (Malandain-Bertrand): T26 = the number of 26-connected components of the foreground among the 26
 * neighbours; T6bar = the number of 6-connected components of the background within the 18-neighbourhood (the 26 neighbours minus the 8
 * corners) that contain at least one of the six face neighbours.  p is an END POINT when fewer than two of its 26 neighbours are
 * foreground.  Directions d = 0 .. 5: (-1,0,0), (+1,0,0), (0,-1,0), (0,+1,0), (0,0,-1), (0,0,+1).  Subfields s = 0 .. 7:
 * s = 4 (x & 1) + 2 (y & 1) + (z & 1).  A PASS runs for d = 0 .. 5: (1) mark: C_d = the foreground voxels whose neighbour at p + d is
 * background, in the image as it is now; (2) for s = 0 .. 7 in order, delete simultaneously every p in C_d of subfield s that, in the
 * image as it is at the start of this sub-step, is still foreground, is not an end point and is simple.  Passes repeat until one
 * deletes nothing.  Two voxels of one subfield differ by an even amount on every axis, so neither lies in the other's 3x3x3 window,
 * which is all the two tests read: deleting a sub-step's voxels at once equals deleting them one by one in any order, every deletion
 * is of a simple point (the topology is kept), and the result is a function of the mask and this schedule alone -- bit-identical on
 * every run and equal to the numpy restatement (tests/skeleton_restate.py).
 * vg_skeleton_begin: packs the mask into the scratch as bits -- word w (uint64) of row (x, y) holds z = 64 w .. 64 w + 63, bit z & 63,
 *   ceil(Z / 64) words per row, padding bits 0.  One launch.  scratch: vg_skeleton_scratch_bytes(X, Y, Z, n_passes) bytes, 16-byte
 *   aligned: two bit volumes of al16(8 X Y ceil(Z / 64)) bytes each (the image, the marks of a direction), then al16(4 n_passes) bytes
 *   that the entries never touch by themselves -- room for deleted_out.  begin and end need the size for n_passes = 1.
 * vg_skeleton_passes: n_passes (1 .. VG_SKELETON_MAX_PASSES) passes on the packed image, in place; may be called again to go on
 *   thinning without repacking.  deleted_out: n_passes uint32 words ON THE DEVICE, 4-byte aligned, anywhere -- the tail of the scratch
 *   (offset 2 al16(8 X Y ceil(Z / 64))) or a buffer of the caller's beside it, not inside the two bit volumes; zeroed by the entry,
 *   then deleted_out[i] = voxels deleted by pass i.  A pass is 6 x (1 + 8) launches (fewer where X or Y is 1: a subfield without rows
 *   is not launched); every launch of pass i > 0 first reads deleted_out[i - 1] and leaves at once when it is 0, so the passes after
 *   convergence cost their launches only and leave deleted_out[i] = 0.  Pass 0 of a call always runs.  One integer atomic per wave
 *   (the count); the image is updated by plain stores of words that one thread owns.
 * vg_skeleton_end: unpacks the image to out (uint8[n], 0 / 1; 16-byte stores where out is 16-byte aligned).  One launch; the scratch
 *   is only read, so thinning may go on afterwards.
 * vg_neighbour_count26: out[v] (uint8) = the number of foreground voxels among the 26 neighbours of v where mask[v] != 0 (saturated at
 *   255, which 26 never reaches), 0 on the background.  On a skeleton: 1 = end point, 2 = segment, >= 3 = junction, 0 = isolated
 *   voxel.  One launch, no scratch; out and mask must not overlap.
 * --------------------------------------------------------------------------------------------- */
#define VG_EDT_SQUARED_I32 0
#define VG_EDT_DIST_F32 1
#define VG_SKELETON_MAX_PASSES 4096
#define VG_CC_TILE_X 8
#define VG_CC_TILE_Y 8
#define VG_CC_TILE_Z 64
int64_t vg_cc_scratch_bytes(int64_t n);
int vg_cc_label(const uint8_t* mask, int X, int Y, int Z, int connectivity, int32_t* labels, uint32_t* sizes, uint32_t* result4,
                void* scratch, int64_t scratch_bytes, vg_stream_t stream);
int vg_cc_filter(const int32_t* labels, int64_t n, const uint32_t* sizes, const uint32_t* result4, uint32_t min_size, uint8_t* out,
                 uint32_t* counts2, uint32_t* newid_or_null, int32_t* relabel_or_null, vg_stream_t stream);
int vg_hist256(const float* pred, int64_t n, uint32_t* hist, uint32_t* nonfinite, vg_stream_t stream);
int vg_threshold_mask(const float* pred, int64_t n, int as_u8, float t, const float* t_dev_or_null, int otsu, const uint32_t* hist256_or_null,
                      float* t_otsu_or_null, uint8_t* mask, uint32_t* nonfinite, vg_stream_t stream);
int64_t vg_edt_scratch_bytes(int X, int Y, int Z, int weighted);
int vg_edt(const uint8_t* mask, int X, int Y, int Z, const double* sampling3_or_null, void* out, int out_kind, void* scratch,
           int64_t scratch_bytes, vg_stream_t stream);
int vg_fill_holes_mark(const int32_t* labels, int X, int Y, int Z, uint8_t* flags, vg_stream_t stream);
int vg_fill_holes_apply(const uint8_t* mask, const int32_t* labels, const uint8_t* flags, int64_t n, uint8_t* out, vg_stream_t stream);
int64_t vg_skeleton_scratch_bytes(int X, int Y, int Z, int n_passes);
int vg_skeleton_begin(const uint8_t* mask, int X, int Y, int Z, void* scratch, int64_t scratch_bytes, vg_stream_t stream);
int vg_skeleton_passes(int X, int Y, int Z, int n_passes, void* scratch, int64_t scratch_bytes, uint32_t* deleted_out, vg_stream_t stream);
int vg_skeleton_end(int X, int Y, int Z, const void* scratch, int64_t scratch_bytes, uint8_t* out, vg_stream_t stream);
int vg_neighbour_count26(const uint8_t* mask, int X, int Y, int Z, uint8_t* out, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The vessel graph (csrc/vg_skelgraph.hip; van_gan_amd/postprocess.py skeleton_graph, prune_spurs,
 * network_summary, vessel_graph): the skeleton as segments and nodes with their measurements, and the removal of short terminal spurs.
 * The same code in both storage builds.  Every entry only enqueues, allocates nothing, checks its arguments on the host before any
 * launch (VG_EINVAL, nothing launched) and initialises its own outputs: no result depends on what a buffer held before.  Only integer
 * atomics -- no float atomic appears anywhere in the file: equal inputs give bit-identical results on every run.
 *
 * THE DEFINITIONS.  Input: skel, a uint8 volume [X][Y][Z] with Z innermost, 1 <= n = X Y Z < 2^31.  Foreground is S = {skel != 0},
 * 26-connected; outside the volume is background.  Any mask is legal, not only a skeleton.
 * Degree and classes: deg(p) is the number of p's 26 neighbours in S (what vg_neighbour_count26 returns).  Segment voxels are
 *   B = {p in S : deg(p) = 2}; node voxels are N = S \ B, that is deg 0, 1 or >= 3.
 * Segments are the 26-components of B, numbered 1 .. E; nodes are the 26-components of N, numbered 1 .. V.  A cluster of adjacent
 *   junction voxels is one node; an end voxel adjacent to a junction voxel belongs to that node.  Both are numbered as
 *   scipy.ndimage.label(., np.ones((3,3,3))) numbers them, by raster order of the first voxel: they are vg_cc_label at connectivity 3 of
 *   the two masks vg_skelgraph_classify writes.
 * Segment shape: every B voxel has exactly two S-neighbours, so a segment is a simple path or a simple closed cycle.  The number of
 *   (B voxel, N neighbour) pairs of a segment is 2 for a path and 0 for a cycle.  Two different nodes are never adjacent, so every
 *   connection between nodes runs through a segment.
 * Attachments: for a path, sort the two pairs (p, q) (p in the segment, q in N, 26-adjacent) by (linear index of p, linear index of q);
 *   end 0 is the smaller pair and end 1 the larger.  seg_ends[e] = (q0, q1) as linear indices, seg_nodes[e] = (node(q0), node(q1)).  A
 *   cycle has (-1, -1) and (0, 0).  A loop, with both ends at one node, is legal.  On the device this is a 64-bit integer atomic min
 *   and a 64-bit integer atomic max of the key (p << 32) | q per segment.
 * Length, exactly: the class of a step (dx, dy, dz) is c = 4 |dx| + 2 |dy| + |dz| - 1 in 0 .. 6.  seg_half_steps[e][c] (int64) sums,
 *   over p in the segment and over every S-neighbour q of p of class c, the value 1 if q is in B and 2 if q is in N.  Every row sum is
 *   even: 2 (voxels + 1) for a path, 2 voxels for a cycle.  With sampling = (sx, sy, sz), default 1, the step length is l_c =
 *   sqrt((|dx| sx)^2 + (|dy| sy)^2 + (|dz| sz)^2), computed in fp64 on the host, and seg_length[e] = (sum over c = 0 .. 6 of
 *   half[e][c] l_c) / 2 in fp64, the products and the sum evaluated left to right, each operation rounded, with no fused multiply-add.
 * Chord and tortuosity: seg_chord[e] is the fp64 Euclidean distance between q0 and q1 under sampling -- sqrt of the left-to-right sum
 *   of the squares of (difference of the coordinate) * spacing; 0 for a cycle or for q0 = q1.  Tortuosity is length / chord, taken in
 *   the host's summary only.
 * Radius (optional; an fp32 volume such as vg_edt writes): per segment, min and max over its voxels are exact (integer atomics on the
 *   bit pattern; the values are >= 0).  The mean is deterministic, through fixed point: with D = sqrt((X sx)^2 + (Y sy)^2 + (Z sz)^2),
 *   b = 62 - ceil(log2 n) and k = b - ceil(log2 D), both from the shape and the sampling alone, on the host, the kernel adds
 *   llrint(r 2^k) into an int64 per segment (the product is exact: fp32 -> fp64 times a power of two) and seg_radius_mean =
 *   sum / 2^k / voxels.  The quantisation is at most 2^-(k+1) absolute per voxel.  Voxels whose radius is negative, NaN, infinite or
 *   above D are skipped and counted in bad2[0].
 * Nodes: node_voxels and node_degree are int32; node_degree counts attachments, so a loop counts twice.  node_kind (uint8): 0 is
 *   isolated, one voxel of deg 0; 1 is end, one voxel of deg 1; 2 is every other node.  node_centroid is fp64 [V + 1][3], built from
 *   uint64 coordinate sums divided by the voxel count.
 * Spur: a path segment with exactly one of its two nodes of kind end and seg_length < min_length.  One pruning round deletes, from S,
 *   the voxels of every spur and the end voxel it hangs from; nothing else.  It is 26-neighbour local: a B voxel goes iff its segment
 *   is flagged; a node voxel with deg 1 goes iff its single neighbour is a B voxel of a flagged segment.  A path between two end nodes
 *   is kept, cycles are kept, nodes of kind 2 are never touched.  Each removal is a chain of simple-point deletions from the tip, so
 *   the 26-components and the Euler characteristic of S are unchanged.
 *
 * vg_skelgraph_classify: one pass over skel writes degree (as vg_neighbour_count26), segment_mask (1 on B) and node_mask (1 on N), each
 *   uint8[n]; none may overlap skel.  One launch; 32-bit loads and stores, four voxels a lane, where Z % 4 == 0 and the four pointers
 *   are 4-byte aligned, bytes otherwise.
 * vg_skelgraph_scratch_bytes(E, V): the scratch of vg_skelgraph_tables, al16(80 (E + 1) + 36 (V + 1) + 16) + al16(12 (E + 1)) bytes.
 * vg_skelgraph_tables: the tables above from skel, degree, and the two label volumes (int32[n]) with their counts E and V (each
 *   0 .. n / 2 + 1).  Every table has E + 1 (V + 1) rows, row 0 zeros: seg_half_steps int64 [E + 1][7], seg_voxels int32, seg_ends int64
 *   [E + 1][2], seg_nodes int32 [E + 1][2], seg_length and seg_chord fp64; with radius_or_null (then both or neither of) seg_radius_mean
 *   fp64 [E + 1] and seg_radius_minmax fp32 [E + 1][2]; node_voxels, node_degree int32, node_kind uint8, node_centroid fp64 [V + 1][3].
 *   bad2 = (voxels with a skipped radius, labels met outside 0 .. E / 0 .. V -- such a label is never used as an index).  sampling3 =
 *   three doubles IN HOST MEMORY, read before the call returns, each finite and > 0.  fp64 / int64 tables are 8-byte aligned, 32-bit
 *   ones 4-byte; scratch 16-byte aligned, contents irrelevant on entry.  Two memsets and two launches: one thread per voxel (a wave
 *   without foreground leaves after one load; a wave whose segment voxels lie in one segment, or whose node voxels lie in one node,
 *   adds its lanes up before one lane issues the atomics), then one thread per segment and per node.
 * vg_skelgraph_prune: out (uint8[n], 0 / 1) = S after one pruning round with min_length (not a NaN) under sampling3; reads the
 *   seg_half_steps, seg_nodes and node_kind that vg_skelgraph_tables wrote.  flags: E + 1 bytes of scratch (1 per spur).  counts2 =
 *   (spurs, voxels deleted).  out must not overlap an input.  One memset and two launches.
 * --------------------------------------------------------------------------------------------- */
int vg_skelgraph_classify(const uint8_t* skel, int X, int Y, int Z, uint8_t* degree, uint8_t* segment_mask, uint8_t* node_mask, vg_stream_t stream);
int64_t vg_skelgraph_scratch_bytes(int E, int V);
int vg_skelgraph_tables(const uint8_t* skel, const uint8_t* degree, const int32_t* segment_labels, const int32_t* node_labels,
                        const float* radius_or_null, int X, int Y, int Z, int E, int V, const double* sampling3_or_null,
                        int64_t* seg_half_steps, int32_t* seg_voxels, int64_t* seg_ends, int32_t* seg_nodes, double* seg_length, double* seg_chord,
                        double* seg_radius_mean_or_null, float* seg_radius_minmax_or_null, int32_t* node_voxels, int32_t* node_degree,
                        uint8_t* node_kind, double* node_centroid, uint32_t* bad2, void* scratch, int64_t scratch_bytes, vg_stream_t stream);
int vg_skelgraph_prune(const uint8_t* skel, const uint8_t* degree, const int32_t* segment_labels, const int32_t* node_labels, int X, int Y, int Z,
                       int E, int V, const int64_t* seg_half_steps, const int32_t* seg_nodes, const uint8_t* node_kind, double min_length,
                       const double* sampling3_or_null, uint8_t* flags, uint8_t* out, uint32_t* counts2, vg_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scoring a mask (csrc/vg_evaluate.hip; van_gan_amd/postprocess.py overlap_counts, mask_surface,
 * euler_characteristic, betti_numbers, surface_distances, cldice_score, evaluate_segmentation): what measures a segmentation against a
 * ground truth -- overlap, topology, surface distances.  The same code in both storage builds.  Volumes are [X][Y][Z] with Z innermost,
 * n = X * Y * Z, 1 <= n < 2^31; masks are uint8, foreground is != 0.  Every entry only enqueues, allocates nothing, checks its arguments
 * on the host before any launch (VG_EINVAL, nothing launched: NULL pointers, those named _or_null excepted; n or an extent out of range;
 * a pointer that is not aligned for its type; a scratch smaller than its query says or not 16-byte aligned; what is listed per entry)
 * and initialises its own outputs: no result depends on what a buffer held before.  Only integer atomics, each a sum -- no float atomic
 * appears in the file: equal inputs give bit-identical results on every run.  No workgroup waits on another, and every loop is a grid
 * stride over a count fixed at launch.
 *
 * vg_mask_counts: counts4 (uint64[4], 8-byte aligned) = (|a & b|, |a & !b|, |!a & b|, |!a & !b|) of the two masks of n voxels; with a the
 *   prediction and b the truth that is (tp, fp, fn, tn).  A memset and one launch: 16-byte loads where a and b are equally far from a
 *   16-byte boundary (the voxels before it and after the last whole vector go one a lane), single voxels otherwise; a sum per wave, then
 *   one atomic per workgroup and counter.
 * vg_mask_surface: surf[v] = mask[v] != 0 && (a face neighbour of v is 0 or lies outside the volume) (0 / 1) -- the mask without
 *   scipy.ndimage.binary_erosion(mask, generate_binary_structure(3, 1), border_value=0) -- and not_surf[v] = !surf[v], the mask whose
 *   vg_edt is the distance to the nearest surface voxel; either may be NULL.  *count (uint64, 8-byte aligned) = the surface voxels.
 *   A memset and one launch; 32-bit loads and stores, four voxels a lane in packed arithmetic, where Z % 4 == 0 and the three pointers
 *   are 4-byte aligned, bytes otherwise.  surf and not_surf must overlap neither mask nor each other.
 * vg_euler_characteristic: cells5 (int64[5], 8-byte aligned) = (V, E, F, C, V - E + F - C) of the closed cubical complex of the
 *   foreground: C the foreground voxels, and a face / edge / vertex of the voxel grid counted once when any of the 2 / 4 / 8 voxels that
 *   share it is foreground, voxels outside the volume being background.  V - E + F - C is the Euler characteristic of the foreground
 *   under 26-connectivity with a 6-connected background, the convention of vg_skeleton_*.  A memset and one launch over the
 *   (X + 1)(Y + 1)(Z + 1) corners, each thread counting the cells at the low corner of its voxel; the same two forms as vg_mask_surface.
 * vg_flags_count: out[0] (uint32) = the labels l in 1 .. K with flags[l] == 0, K = result4[0] read on the device and capped at n / 2 + 1,
 *   the last label the n / 2 + 2 bytes of flags have room for.  With labels = vg_cc_label of the INVERTED mask at connectivity 1, result4
 *   its result and flags from vg_fill_holes_mark, that is the number of enclosed cavities.  A memset and one launch.
 * vg_masked_stats: statistics of the 32-bit array keys[n] over the voxels with sel[v] != 0 (sel: uint8[n]).  kind VG_EVAL_SQ_I32: keys
 *   are non-negative int32 squared distances, value = sqrt((double)key), correctly rounded; VG_EVAL_DIST_F32: non-negative finite fp32,
 *   value = (double)key.  In both the order of the values is the order of the bit patterns as uint32, which is what is selected on.
 *   out: VG_EVAL_STATS_BYTES bytes on the device, 8-byte aligned: uint64 m, the selected count | uint32 the largest selected key |
 *   uint32 0 | fp64 sum of the values | uint32 stat[VG_EVAL_MAX_STATS]: stat[r], r < R, is the key of rank max(ceil(q[r] m) - 1, 0) among
 *   the selected keys in ascending order, product and ceiling in fp64 on the device from m (stat[r] = 0 for r >= R).  m == 0 gives
 *   maximum, sum and stats 0.  q_host: R doubles IN HOST MEMORY, read before the call returns, 0 < q <= 1; 1 <= R <= VG_EVAL_MAX_STATS.
 *   The sum: every thread adds its values in index order, a fixed tree of eight levels adds the 256 threads of a workgroup, the
 *   workgroup's partial goes to the scratch, and one workgroup adds the partials -- thread t those of workgroups t, t + 256, ... in
 *   ascending order, then the same tree.  The select: the most-significant-digit radix select of vg_order_stats, 8 bits a pass -- a
 *   histogram kernel over the selected keys that share the prefix, a one-workgroup pick -- without any read-back.  Ten launches
 *   whatever the data.  scratch: vg_masked_stats_scratch_bytes(n, R) bytes, 16-byte aligned, contents irrelevant on entry.  16-byte loads
 *   of the keys with 32-bit loads of sel where the two pointers allow, as vg_mask_counts.
 * --------------------------------------------------------------------------------------------- */
#define VG_EVAL_SQ_I32 0
#define VG_EVAL_DIST_F32 1
#define VG_EVAL_MAX_STATS 4
#define VG_EVAL_STATS_BYTES 40
int vg_mask_counts(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* counts4, vg_stream_t stream);
int vg_mask_surface(const uint8_t* mask, int X, int Y, int Z, uint8_t* surf_or_null, uint8_t* not_surf_or_null, uint64_t* count,
                    vg_stream_t stream);
int vg_euler_characteristic(const uint8_t* mask, int X, int Y, int Z, int64_t* cells5, vg_stream_t stream);
int vg_flags_count(const uint8_t* flags, const uint32_t* result4, int64_t n, uint32_t* out, vg_stream_t stream);
int64_t vg_masked_stats_scratch_bytes(int64_t n, int R);
int vg_masked_stats(const void* keys, const uint8_t* sel, int64_t n, int kind, const double* q_host, int R, void* out, void* scratch,
                    int64_t scratch_bytes, vg_stream_t stream);

/* Device memset-to-zero / device-to-device copy on an explicit stream (hipMemsetAsync / hipMemcpyAsync): what a recorded launch list
 * (van_gan_amd.VanGan.record_train_step) replays in place of torch's zero_() / copy_(), which would go to torch's current stream. */
int vg_memset_zero(void* p, int64_t nbytes, vg_stream_t stream);
int vg_copy_bytes(void* dst, const void* src, int64_t nbytes, vg_stream_t stream);

/* f32 <-> bf16 copies */
int vg_f32_to_bf16(const float* x, void* y, int64_t n, vg_stream_t stream);
int vg_bf16_to_f32(const void* x, float* y, int64_t n, vg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
