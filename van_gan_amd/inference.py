"""Sliding-window generator inference on MI355X: the counterpart of GanMonitor.stitch_subvolumes
(custom_callback.py:47-223) / run_mapping (:466-509) / post_training.epoch_sweep (post_training.py:22-39) without the
TIFF I/O.  Windows are batched through the HIP generator; overlap-add, coverage count, division, un-padding and the
final 255*min-max run on the GPU.

Beyond the reference, and off by default: centre-weighted (Gaussian) blending of the overlapping windows (blend='gaussian') and flip
test-time augmentation (tta='xz', ...).  Either one moves the gather and the overlap-add onto two batched kernels driven by a
device-resident window table (vg_window_gather / vg_window_scatter, csrc/vg_stitch.hip)."""
from __future__ import annotations

import math
from typing import Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import check, lib
from .ops import _p, stream


def window_origins(n: int, k: int, s: int):
    """The reference's loop (custom_callback.py:140-190): dim_out+1 iterations, start += stride, clamped to n-k (so the
    last windows may coincide - they are then counted twice, as in the reference)."""
    dim_out = int(math.floor((n - k) / s + 1))
    out, start = [], 0
    for _ in range(dim_out + 1):
        if start > n - k:
            start = n - k
        out.append(start)
        start += s
    return out


_AXIS_BIT = {'x': 1, 'y': 2, 'z': 4}
WEIGHT_FLOOR = 1e-12          # per-axis lower bound of the Gaussian tables: the product of three stays a normal fp32 number (1e-36)


def flip_masks(tta) -> list:
    """tta: a subset of the axes 'x', 'y', 'z' (a string such as 'xz', or an iterable of such letters) -> the 2^len(tta) flip masks
    over those axes in ascending order, the unflipped 0 first (bit 0 = x, bit 1 = y, bit 2 = z)."""
    axes = [] if tta is None else list(tta) if isinstance(tta, (str, list, tuple, set, frozenset)) else None
    if axes is None:
        raise ValueError("tta must be a string or an iterable of axes out of 'x', 'y', 'z', got %r" % (tta,))
    allowed = 0
    for a in axes:
        if not isinstance(a, str) or a not in _AXIS_BIT:
            raise ValueError("tta must name axes out of 'x', 'y', 'z', got %r" % (a,))
        if allowed & _AXIS_BIT[a]:
            raise ValueError('tta names axis %r twice' % a)
        allowed |= _AXIS_BIT[a]
    return [m for m in range(8) if not m & ~allowed]


def gaussian_weights(k: int, sigma_scale: float) -> np.ndarray:
    """Per-axis blending table: w[i] = float32(max(exp(-0.5 * ((i - (k-1)/2) / (sigma_scale * k))^2), WEIGHT_FLOOR)), evaluated in float64.
    The floor only matters for sigma_scale below ~0.07 (the default 0.125 gives exp(-8) = 3.4e-4 at the window's edge): without it a narrow
    Gaussian underflows to 0 at the edges and a voxel that only window edges cover would come out as 0/0."""
    i = np.arange(k, dtype=np.float64)
    return np.maximum(np.exp(-0.5 * ((i - (k - 1) / 2.0) / (float(sigma_scale) * k)) ** 2), WEIGHT_FLOOR).astype(np.float32)


def _blend_args(blend, sigma_scale, tta):
    """Validation of the blending / TTA keywords; touches no device."""
    if blend not in ('count', 'gaussian'):
        raise ValueError("blend must be 'count' or 'gaussian', got %r" % (blend,))
    try:
        sig = float(sigma_scale)
    except (TypeError, ValueError):
        raise ValueError('sigma_scale must be a positive finite number, got %r' % (sigma_scale,))
    if not math.isfinite(sig) or sig <= 0:
        raise ValueError('sigma_scale must be a positive finite number, got %r' % (sigma_scale,))
    return blend == 'gaussian', sig, flip_masks(tta)


def _check_table(tab, dims, k) -> np.ndarray:
    """Host-side validation of a window table (any [B,4] integer array-like; a device tensor is copied to the host): every origin in
    [0, extent - k_a], every flip in 0..7.  The kernels skip other rows, but a caller that builds one has a bug worth hearing about."""
    t = tab.detach().cpu().numpy() if isinstance(tab, torch.Tensor) else np.asarray(tab)
    if t.ndim != 2 or t.shape[1] != 4 or t.shape[0] < 1 or t.dtype.kind not in 'iu':
        raise ValueError('window table must be an integer array of shape [B, 4] with B >= 1')
    for a in range(3):
        if k[a] < 1 or k[a] > dims[a]:
            raise ValueError('window %s does not fit the volume %s' % (tuple(k), tuple(dims)))
        if t[:, a].min() < 0 or t[:, a].max() > dims[a] - k[a]:
            raise ValueError('window table: origin outside [0, %d] on axis %d' % (dims[a] - k[a], a))
    if t[:, 3].min() < 0 or t[:, 3].max() > 7:
        raise ValueError('window table: flip mask outside 0..7')
    return t


def _dev_f32(t, numel, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel):
        raise ValueError('%s must be a contiguous fp32 device tensor of %d elements' % (what, numel))
    return t


def _dev_tab(tab):
    if not (isinstance(tab, torch.Tensor) and tab.is_cuda and tab.dtype == torch.int32 and tab.is_contiguous()):
        raise ValueError('window table must be a contiguous int32 device tensor')
    return tab


def window_gather(vol: torch.Tensor, tab: torch.Tensor, k: Sequence[int], out: torch.Tensor) -> torch.Tensor:
    """out[b][i][j][l] = vol[x0 + f_x(i)][y0 + f_y(j)][z0 + f_z(l)] for the B rows (x0, y0, z0, flip) of the int32 device table `tab`
    (vg_window_gather, include/vangan_hip.h); vol [X,Y,Z] and out [B,kx,ky,kz] (a trailing channel of 1 is fine) fp32 on the device.
    The table is validated on a host copy (a synchronising read): this is the checked public form, the stitch loop calls the entry."""
    kx, ky, kz = (int(a) for a in k)
    if vol.dim() != 3:
        raise ValueError('vol must be [X,Y,Z]')
    X, Y, Z = vol.shape
    t = _check_table(_dev_tab(tab), (X, Y, Z), (kx, ky, kz))
    _dev_f32(vol, X * Y * Z, 'vol')
    _dev_f32(out, t.shape[0] * kx * ky * kz, 'out')
    check(lib.vg_window_gather(_p(vol), X, Y, Z, _p(tab), t.shape[0], kx, ky, kz, _p(out), stream()), 'vg_window_gather')
    return out


def window_scatter(win: torch.Tensor, tab: torch.Tensor, k: Sequence[int], p: Sequence[int], weights, pred: torch.Tensor,
                   cnt: torch.Tensor) -> None:
    """pred[x0+i][y0+j][z0+l] += w * win[b][f_x(i)][f_y(j)][f_z(l)], cnt[...] += w over the box cropped by p = (px,py,pz) on each side
    (vg_window_scatter).  weights: None (w = 1) or the three per-axis fp32 device tables (wx, wy, wz) of kx, ky, kz elements."""
    kx, ky, kz = (int(a) for a in k)
    px, py, pz = (int(a) for a in p)
    if pred.dim() != 3 or pred.shape != cnt.shape:
        raise ValueError('pred and cnt must be [X,Y,Z] and alike')
    X, Y, Z = pred.shape
    t = _check_table(_dev_tab(tab), (X, Y, Z), (kx, ky, kz))
    if min(px, py, pz) < 0 or kx - 2 * px < 1 or ky - 2 * py < 1 or kz - 2 * pz < 1:
        raise ValueError('crop %s leaves nothing of window %s' % ((px, py, pz), (kx, ky, kz)))
    _dev_f32(win, t.shape[0] * kx * ky * kz, 'win')
    _dev_f32(pred, X * Y * Z, 'pred')
    _dev_f32(cnt, X * Y * Z, 'cnt')
    if weights is None:
        wx = wy = wz = None
    else:
        wx, wy, wz = weights
        for w, n in ((wx, kx), (wy, ky), (wz, kz)):
            _dev_f32(w, n, 'a weight table')
    check(lib.vg_window_scatter(_p(win), _p(tab), t.shape[0], kx, ky, kz, px, py, pz, _p(wx), _p(wy), _p(wz), X, Y, Z, _p(pred), _p(cnt),
                                stream()), 'vg_window_scatter')


def stitch_subvolumes(engine, gen: str, img: torch.Tensor, subvol_size: Sequence[int], stride=(25, 25, 128), complete=True,
                      padFactor: float = 0.25, border_removal: bool = True, process_img: bool = False,
                      window_batch: int = 4, precision: str = None, *, blend: str = 'count', sigma_scale: float = 0.125,
                      tta=()) -> torch.Tensor:
    """img: [X,Y,Z,1] fp32 (host or device).  gen: 'gen_IS' or 'gen_SI'.  Returns 255*minmax(pred) as fp32 [X,Y,Z,1]
    on the device (custom_callback.py:202).  subvol_size is (kX,kY,kZ).
    precision: None = the engine's training precision (bf16 / fp32 storage); 'fp16' = IEEE half-precision storage with fp32
    accumulation (BASELINE config 5; the reference's inference runs whatever policy TF was given, post_training.py:38-39): the
    generator's forward runs in libvangan_hip_h.so (van_gan_amd.ops.Fp16) on weights repacked to fp16 at the start of the call.
    Beyond the reference (defaults = the reference's equal-weight stitch, on its own unchanged code path):
    blend: 'count' (every window counts equally) or 'gaussian' (a voxel at window position (i,j,l) weighs wx[i]*wy[j]*wz[l], per-axis
    Gaussians centred on the window with sigma = sigma_scale * k_a, floored at 1e-12 per axis so that no covered voxel ever divides 0 by 0;
    the border crop still applies).
    tta: flip test-time augmentation over a subset of 'x','y','z' ('xz', ('x','z'), ...): every window is predicted under all
    2^len(tta) mirror flips over those axes, un-flipped, and all predictions are accumulated (2^len(tta) times the forwards)."""
    import contextlib
    gaussian, sigma_scale, masks = _blend_args(blend, sigma_scale, tta)           # before any device access
    batched = gaussian or len(masks) > 1
    dev = engine.device
    ops.set_device(dev.index)
    if precision not in (None, 'fp16', engine.precision):
        raise ValueError("precision must be None, 'fp16' or the engine's own precision")
    half = precision == 'fp16'
    net = engine.fp16_generator(gen) if half else engine.nets[gen]
    kx, ky, kz = subvol_size
    if tuple(net.dims) != (kx, ky, kz):
        raise ValueError('generator was built for windows %s' % (net.dims,))
    v = img.to(dev, torch.float32)[..., 0]
    ox, oy, oz = v.shape
    sx = sy = sz = 0
    if complete:                       # np.pad(..., 'symmetric'): mirror INCLUDING the edge voxel (host-side indexing)
        sx, sy = int(padFactor * ox), int(padFactor * oy)
        sz = 0 if stride[2] == 1 else int(padFactor * oz)

        def sym(n, p):
            idx = torch.arange(-p, n + p, device=dev)
            idx = torch.where(idx < 0, -idx - 1, idx)
            return torch.where(idx >= n, 2 * n - 1 - idx, idx)
        v = v[sym(ox, sx)][:, sym(oy, sy)][:, :, sym(oz, sz)].contiguous()
    X, Y, Z = v.shape
    if not complete or not border_removal:
        px = py = pz = 0
    else:
        px, py, pz = int(0.1 * kx), int(0.1 * ky), int(0.1 * kz)
        if kz == Z:
            pz = 0
    pred = torch.zeros(X, Y, Z, device=dev)
    cnt = torch.zeros(X, Y, Z, device=dev)
    origins = [(a, b, c) for a in window_origins(X, kx, stride[0]) for b in window_origins(Y, ky, stride[1])
               for c in window_origins(Z, kz, stride[2])]
    S = kx * ky * kz
    if batched:
        # the whole call's window table, one upload: window order as above (x outer, z inner), flips innermost
        host_tab = _check_table(np.array([(a, b, c, m) for a, b, c in origins for m in masks], dtype=np.int32), (X, Y, Z), (kx, ky, kz))
        tab = torch.from_numpy(host_tab).to(dev)
        wts = [torch.from_numpy(gaussian_weights(n, sigma_scale)).to(dev) for n in (kx, ky, kz)] if gaussian else [None] * 3
        origins = host_tab                                   # the chunk loop below walks table entries: 16 bytes each on the device
    # two lanes: consecutive window batches alternate between two streams, each with its own workspace, so that the
    # low-occupancy deep layers of one batch overlap the full-resolution layers of the other
    main = torch.cuda.current_stream()
    lane_b = getattr(engine, '_lane_b', None)
    lanes = [(main, engine.arena)]
    if lane_b is not None and getattr(engine, 'arena_b', None) is not None:
        lane_b.wait_stream(main)                             # v, pred, cnt are ready
        lanes.append((lane_b, engine.arena_b))
    for bi, i0 in enumerate(range(0, len(origins), window_batch)):
        chunk = origins[i0:i0 + window_batch]
        B = len(chunk)
        strm, ar = lanes[bi % len(lanes)]
        with torch.cuda.stream(strm):
            ar.reset()
            xin = ar.alloc((B, kx, ky, kz, 1), torch.float32)
            yout = ar.alloc((B, kx, ky, kz, 1), torch.float32)
            if batched:
                check(lib.vg_window_gather(_p(v), X, Y, Z, tab.data_ptr() + 16 * i0, B, kx, ky, kz, _p(xin), stream()), 'vg_window_gather')
            else:
                for b, (a, bb, c) in enumerate(chunk):
                    xin[b, ..., 0].copy_(v[a:a + kx, bb:bb + ky, c:c + kz])
            if process_img:            # process_imaging_otf with axis=None (main.py:169-177): per-window min-max to [-1,1]
                mm = ar.alloc((B, 4), torch.float32)
                tmp = ar.alloc((B, kx, ky, kz, 1), torch.float32)
                ops.minmax(xin, B, S, mm)
                ops.minmax_apply(xin, mm, B, S, tmp)
                ones = ar.alloc((B, kx, ky, kz, 1), torch.float32)
                ones.fill_(1.0)                              # memset-style fill (plumbing)
                ops.axpby(tmp, 2.0, ones, -1.0, xin)         # 2*n - 1
            with (ops.Fp16() if half else contextlib.nullcontext()):
                net.forward(ar, xin, yout, save=False)
            if batched:
                check(lib.vg_window_scatter(_p(yout), tab.data_ptr() + 16 * i0, B, kx, ky, kz, px, py, pz, _p(wts[0]), _p(wts[1]), _p(wts[2]),
                                            X, Y, Z, _p(pred), _p(cnt), stream()), 'vg_window_scatter')
            else:
                for b, (a, bb, c) in enumerate(chunk):
                    check(lib.vg_overlap_add(_p(yout[b]), kx, ky, kz, px, py, pz, a, bb, c, X, Y, Z, _p(pred), _p(cnt), stream()),
                          'vg_overlap_add')
    if len(lanes) > 1:
        main.wait_stream(lane_b)
    out = torch.zeros(ox, oy, oz, device=dev)
    check(lib.vg_divide_crop(_p(pred), _p(cnt), X, Y, Z, sx, sy, sz, ox, oy, oz, _p(out), stream()), 'vg_divide_crop')
    mm = torch.zeros(1, 4, device=dev)
    nrm = torch.zeros_like(out)
    ops.minmax(out, 1, out.numel(), mm)
    ops.minmax_apply(out, mm, 1, out.numel(), nrm)
    res = torch.zeros_like(out)
    ops.axpby(nrm, 255.0, None, 0.0, res)
    return res[..., None]
