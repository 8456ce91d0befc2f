"""Prediction post-processing on MI355X: from the stitched prediction -- 255 * minmax(pred), fp32, what stitch_subvolumes returns where the
reference's GanMonitor.stitch_subvolumes writes a TIFF (custom_callback.py:202-223) -- to a binary vascular network without leaving the
device: a threshold (a number, or Otsu's from the 256-bin histogram of pred.astype('uint8')), 3-D connected components numbered as
scipy.ndimage.label numbers them, and the removal of components below a voxel count (skimage.morphology.remove_small_objects).  The
arithmetic runs in csrc/vg_components.hip (include/vangan_hip.h "Prediction post-processing"); this module owns
buffers and checks.  Then what measures that network, at the end of the file: the exact Euclidean distance transform
(scipy.ndimage.distance_transform_edt), hole filling (scipy.ndimage.binary_fill_holes) and the vessel radius, the two chained
(csrc/vg_edt.hip).  Then its centreline: exact topological thinning to a one-voxel-wide curve skeleton, the
degree of every skeleton voxel, and the radius along the centreline (csrc/vg_skeleton.hip).  Then the graph of
that centreline: segments and nodes with length, chord and radius per segment, the pruning of short spurs and a summary of the network
(csrc/vg_skelgraph.hip); skeleton_graph reads the two counts back once to size its tables.

A volume is [X,Y,Z] (or [X,Y,Z,1]) with Z innermost, a contiguous torch tensor ON THE DEVICE: a prediction is fp32, a mask uint8 or bool
(0 is background).  Arguments are checked before the device is touched (ValueError).  Every function only enqueues unless a read-back
is asked for (return_threshold, return_sizes, return_info); a read-back raises RuntimeError on a non-zero status word of vg_cc_label.
The one exception is thinning until nothing changes (skeletonize with max_passes=None and what builds on it), which reads the voxels
deleted by every four passes back to know when to stop; skeletonize(mask, max_passes=k) only enqueues."""
from __future__ import annotations

import ctypes
import math
import numbers
import operator
from typing import Tuple

import torch

from ._lib import check as _check, lib
from .ops import _p, stream
from .preprocess import _shape3

R_K, R_STATUS, R_FOREGROUND = 0, 1, 2      # the words of vg_cc_label's result4
OTSU = 'otsu'


TILE = (8, 8, 64)                          # VG_CC_TILE_X / _Y / _Z
MAX_TILES = (2 ** 32 - 1) // 256           # vg_cc_label runs one 256-thread workgroup per tile, and a grid holds fewer than 2^32 threads


def label_tiles(shape) -> int:
    """The tiles vg_cc_label cuts a volume of this shape into."""
    return math.prod(-(-s // t) for s, t in zip(shape, TILE))


def _on_device(x, what: str):
    if not x.is_cuda:
        raise ValueError('%s must be on the device, got a tensor on %s' % (what, x.device))


def _device_volume(x, dtypes, what: str, labelled: bool = False, check_device: bool = True) -> Tuple[torch.Tensor, Tuple[int, int, int]]:
    """x and its (X, Y, Z); everything a wrong argument can be is rejected here, on the host -- type, shape, dtype, layout and size first,
    none of which needs a device, then where the tensor lives.  labelled: the volume goes through vg_cc_label, which has a tile limit."""
    if not isinstance(x, torch.Tensor):
        raise ValueError('%s must be a torch tensor on the device, got %s' % (what, type(x).__name__))
    shape = _shape3(x.shape)
    if x.dtype not in dtypes:
        raise ValueError('%s must be %s, got %s' % (what, ' or '.join(str(d) for d in dtypes), x.dtype))
    if not x.is_contiguous():
        raise ValueError('%s must be contiguous' % what)
    if math.prod(shape) >= 2 ** 31:
        raise ValueError('%s has %d voxels; the post-processing serves fewer than 2^31' % (what, math.prod(shape)))
    if labelled and label_tiles(shape) > MAX_TILES:
        raise ValueError('%s of shape %s is %d tiles of %dx%dx%d voxels; the labelling serves at most %d (a very thin volume: reshape it)'
                         % ((what, shape, label_tiles(shape)) + TILE + (MAX_TILES,)))
    if check_device:
        _on_device(x, what)
    return x.detach(), shape


def _mask_volume(mask):
    """A mask that is going to be labelled."""
    m, shape = _device_volume(mask, (torch.uint8, torch.bool), 'mask', labelled=True)
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), shape


def _connectivity(connectivity) -> int:
    try:
        c = operator.index(connectivity)
    except TypeError:
        raise ValueError('connectivity is 1, 2 or 3, got %r' % (connectivity,)) from None
    if c not in (1, 2, 3):
        raise ValueError('connectivity is 1, 2 or 3 (6, 18 or 26 neighbours), got %r' % (connectivity,))
    return c


def _min_size(min_size) -> int:
    try:
        m = operator.index(min_size)
    except TypeError:
        raise ValueError('min_size is an integer >= 0, got %r' % (min_size,)) from None
    if m < 0:
        raise ValueError('min_size is an integer >= 0, got %r' % (min_size,))
    return min(m, 2 ** 32 - 1)                                      # no component has 2^31 voxels: every larger bound drops them all


def _threshold(threshold):
    """('otsu' | 'u8' | 'f32' | 'dev', value): an int compares uint8(pred) > t, a float pred > t (t rounded to fp32), a one-element fp32
    device tensor pred > t with t read on the device."""
    if isinstance(threshold, str):
        if threshold != OTSU:
            raise ValueError("threshold is a number, a one-element fp32 device tensor or 'otsu', got %r" % (threshold,))
        return OTSU, None
    if isinstance(threshold, torch.Tensor):
        if not (threshold.is_cuda and threshold.dtype == torch.float32 and threshold.numel() == 1):
            raise ValueError('a threshold tensor is one fp32 element on the device')
        return 'dev', threshold
    if isinstance(threshold, bool) or not isinstance(threshold, numbers.Real):
        raise ValueError("threshold is a number, a one-element fp32 device tensor or 'otsu', got %r" % (threshold,))
    if isinstance(threshold, numbers.Integral):
        return 'u8', float(int(threshold))
    if not math.isfinite(threshold):
        raise ValueError('threshold must be finite, got %r' % (threshold,))
    return 'f32', float(threshold)


def _scratch(query: str, *args, dev) -> Tuple[torch.Tensor, int]:
    """(buffer, bytes): the scratch an entry needs for these sizes, as its query tells (preprocess._scratch, on this module's handle)."""
    nbytes = int(getattr(lib, query)(*args))
    _check(nbytes, query)
    return torch.empty(nbytes, dtype=torch.uint8, device=dev), nbytes


def sizes_capacity(n: int) -> int:
    """Words of a sizes (or newid) buffer: no connectivity allows more than ceil(n / 2) components, and word 0 is the background's."""
    return n // 2 + 2


def histogram256(pred, return_count: bool = False):
    """np.bincount(pred.astype('uint8').ravel(), minlength=256) of the finite voxels as an int32 device tensor [256]; return_count: also
    the one-element int32 device tensor that counts the non-finite voxels.  Enqueue-only."""
    x, _ = _device_volume(pred, (torch.float32,), 'pred')
    with torch.cuda.device(x.device):
        hist = torch.empty(256, dtype=torch.int32, device=x.device)
        counter = torch.zeros(1, dtype=torch.int32, device=x.device)
        _check(lib.vg_hist256(_p(x), x.numel(), _p(hist), _p(counter), stream()), 'vg_hist256')
    return (hist, counter) if return_count else hist


def _binarise(x: torch.Tensor, shape, kind: str, value, counter: torch.Tensor):
    """(mask, threshold): the threshold as the host's float, or as a one-element fp32 device tensor where the device holds it (Otsu's is
    written there)."""
    dev, n = x.device, x.numel()
    mask = torch.empty(shape, dtype=torch.uint8, device=dev)
    if kind == OTSU:
        hist = torch.empty(256, dtype=torch.int32, device=dev)
        t = torch.empty(1, device=dev)
        skipped = torch.zeros(1, dtype=torch.int32, device=dev)          # vg_threshold_mask counts the same voxels again
        _check(lib.vg_hist256(_p(x), n, _p(hist), _p(skipped), stream()), 'vg_hist256')
        _check(lib.vg_threshold_mask(_p(x), n, 1, 0.0, None, 1, _p(hist), _p(t), _p(mask), _p(counter), stream()), 'vg_threshold_mask')
    elif kind == 'dev':
        t = value.reshape(1)
        _check(lib.vg_threshold_mask(_p(x), n, 0, 0.0, _p(t), 0, None, None, _p(mask), _p(counter), stream()), 'vg_threshold_mask')
    else:
        t = value
        _check(lib.vg_threshold_mask(_p(x), n, 1 if kind == 'u8' else 0, value, None, 0, None, None, _p(mask), _p(counter), stream()),
               'vg_threshold_mask')
    return mask, t


def _t_host(t) -> float:
    return float(t.cpu()[0]) if isinstance(t, torch.Tensor) else float(torch.tensor(t, dtype=torch.float32))


def binarise_prediction(pred, threshold=127.5, return_threshold: bool = False):
    """uint8 mask [X,Y,Z] (0 / 1) of the fp32 prediction pred ([X,Y,Z] or [X,Y,Z,1]).  threshold: a float -- pred > t; an int --
    pred.astype('uint8') > t, the comparison on what the reference writes to its TIFF; a one-element fp32 device tensor -- pred > t with
    t read on the device; 'otsu' -- Otsu's threshold of the 256-bin histogram of pred.astype('uint8'), computed on the device in fp64 (the
    first maximiser of the between-class variance; 0 for a one-bin histogram), then pred.astype('uint8') > t.  A non-finite voxel is
    background.  return_threshold=True: (mask, t) with t read back as a float (a synchronising copy); otherwise enqueue-only."""
    kind, value = _threshold(threshold)
    x, shape = _device_volume(pred, (torch.float32,), 'pred')
    with torch.cuda.device(x.device):
        mask, t = _binarise(x, shape, kind, value, torch.zeros(1, dtype=torch.int32, device=x.device))
        return (mask, _t_host(t)) if return_threshold else mask


def _label(m: torch.Tensor, shape, c: int):
    """(labels, sizes, result4) of the uint8 device mask m."""
    dev, n = m.device, m.numel()
    labels = torch.empty(shape, dtype=torch.int32, device=dev)
    sizes = torch.empty(sizes_capacity(n), dtype=torch.int32, device=dev)
    result = torch.empty(4, dtype=torch.int32, device=dev)
    scratch, nbytes = _scratch('vg_cc_scratch_bytes', n, dev=dev)
    _check(lib.vg_cc_label(_p(m), shape[0], shape[1], shape[2], c, _p(labels), _p(sizes), _p(result), _p(scratch), nbytes, stream()), 'vg_cc_label')
    return labels, sizes, result


def _read_result(result: torch.Tensor):
    host = [int(w) for w in result.cpu()]
    if host[R_STATUS] != 0:
        raise RuntimeError('vg_cc_label reported status %d' % host[R_STATUS])
    return host


def label_components(mask, connectivity=1, return_sizes: bool = False):
    """(labels, K): int32 [X,Y,Z] with 0 for background and 1 .. K for the connected components of mask under
    scipy.ndimage.generate_binary_structure(3, connectivity), numbered as scipy.ndimage.label numbers them (raster order of the first
    voxel), and K as a one-element int32 device tensor.  Enqueue-only.  return_sizes=True: (labels, K, sizes) with K an int and sizes the
    int32 device tensor [K + 1] of voxel counts, sizes[0] the background's; this reads K back and raises RuntimeError on a non-zero
    status.  Temporary device memory: 12 bytes per voxel of scratch and 2 for the sizes, beside the 4 of the labels."""
    c = _connectivity(connectivity)
    m, shape = _mask_volume(mask)
    with torch.cuda.device(m.device):
        labels, sizes, result = _label(m, shape, c)
        if not return_sizes:
            return labels, result[R_K:R_K + 1]
        K = _read_result(result)[R_K]
        return labels, K, sizes[:K + 1]


def _filter(labels: torch.Tensor, sizes: torch.Tensor, result: torch.Tensor, min_size: int, relabel: bool = False):
    dev, n = labels.device, labels.numel()
    out = torch.empty(labels.shape, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    newid = torch.empty(sizes_capacity(n), dtype=torch.int32, device=dev) if relabel else None
    renum = torch.empty(labels.shape, dtype=torch.int32, device=dev) if relabel else None
    _check(lib.vg_cc_filter(_p(labels), n, _p(sizes), _p(result), min_size, _p(out), _p(counts), None if newid is None else _p(newid),
                            None if renum is None else _p(renum), stream()), 'vg_cc_filter')
    return out, counts, renum


def remove_small_objects(mask, min_size=64, connectivity=1, return_labels: bool = False):
    """skimage.morphology.remove_small_objects(mask, min_size, connectivity) on the device: the uint8 mask (0 / 1) of the voxels whose
    component has at least min_size voxels.  min_size <= 1 drops nothing: the result is a copy of mask (as 0 / 1) and nothing is labelled,
    unless the labels are asked for.  return_labels=True: (mask, labels, K') with the kept components renumbered 1 .. K' in the same raster order and K' a
    one-element int32 device tensor.  Enqueue-only."""
    c = _connectivity(connectivity)
    msz = _min_size(min_size)
    m, shape = _mask_volume(mask)
    with torch.cuda.device(m.device):
        if msz <= 1 and not return_labels:
            return (m != 0).to(torch.uint8)
        labels, sizes, result = _label(m, shape, c)
        out, counts, renum = _filter(labels, sizes, result, msz, return_labels)
    return (out, renum, counts[1:2]) if return_labels else out


def vessel_mask(pred, threshold=127.5, min_size=64, connectivity=3, return_info: bool = False, fill_holes: bool = False, skeleton: bool = False):
    """binarise_prediction, label_components and remove_small_objects chained: the uint8 mask [X,Y,Z] of the vascular network in the
    prediction.  Enqueue-only; return_info=True: (mask, dict(threshold, components, kept, voxels, kept_voxels)) -- the threshold used, the
    components and the voxels above it, what is left of both -- read back in one synchronising step (RuntimeError on a non-zero status).
    fill_holes=True: the cavities of the kept components are closed afterwards (fill_holes below); the info counts what was there before.
    skeleton=True: skeletonize (below) of the mask that is returned comes as one more value at the end -- (mask, skeleton) or
    (mask, info, skeleton); it thins until nothing changes, which reads a few words back after every four passes."""
    if skeleton:
        got = vessel_mask(pred, threshold, min_size, connectivity, return_info, fill_holes)
        mask = got[0] if return_info else got
        with torch.cuda.device(mask.device):
            skel = _thin(mask, tuple(mask.shape), None)[0]
        return (got[0], got[1], skel) if return_info else (mask, skel)
    kind, value = _threshold(threshold)
    c = _connectivity(connectivity)
    msz = _min_size(min_size)
    x, shape = _device_volume(pred, (torch.float32,), 'pred', labelled=True)
    dev = x.device
    with torch.cuda.device(dev):
        mask, t = _binarise(x, shape, kind, value, torch.zeros(1, dtype=torch.int32, device=dev))
        if msz <= 1 and not return_info:
            return _fill(mask, shape) if fill_holes else mask
        labels, sizes, result = _label(mask, shape, c)
        out, counts, _ = _filter(labels, sizes, result, msz)
        if fill_holes:
            out = _fill(out, shape)
        if not return_info:
            return out
        host = _read_result(result)
        kept = [int(w) for w in counts.cpu()]
        info = dict(threshold=_t_host(t), components=host[R_K], kept=kept[1], voxels=host[R_FOREGROUND], kept_voxels=kept[0])
    return out, info


# ------------------------------------------------------------------------------------------------ measuring the mask (csrc/vg_edt.hip)
EDT_SQUARED_I32, EDT_DIST_F32 = 0, 1       # VG_EDT_SQUARED_I32, VG_EDT_DIST_F32
EDT_INF = 2 ** 31 - 1                      # the squared distance where the volume has no background voxel


def _sampling(sampling):
    """None, or the three voxel spacings (X, Y, Z) as floats; a single number stands for all three, as in scipy."""
    if sampling is None:
        return None
    if isinstance(sampling, numbers.Real) and not isinstance(sampling, bool):
        sampling = (sampling,) * 3
    try:
        s = tuple(float(v) for v in sampling)
    except (TypeError, ValueError):
        raise ValueError('sampling is None, a number or three numbers (the voxel spacing along X, Y, Z), got %r' % (sampling,)) from None
    if len(s) != 3 or not all(math.isfinite(v) and v > 0.0 for v in s):
        raise ValueError('sampling is None, a number or three numbers, each finite and > 0, got %r' % (sampling,))
    return s


def _edt_volume(mask, labelled: bool = False):
    """A mask whose distances are going to be taken: every squared distance in voxel units must be an int32."""
    m, shape = _device_volume(mask, (torch.uint8, torch.bool), 'mask', labelled=labelled, check_device=False)
    if sum(d * d for d in shape) >= 2 ** 31:
        raise ValueError('mask of shape %s: the distance transform serves X^2 + Y^2 + Z^2 < 2^31' % (shape,))
    _on_device(m, 'mask')
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), shape


def _edt(m: torch.Tensor, shape, s, squared: bool) -> torch.Tensor:
    dev = m.device
    out = torch.empty(shape, dtype=torch.int32 if squared else torch.float32, device=dev)
    scratch, nbytes = _scratch('vg_edt_scratch_bytes', shape[0], shape[1], shape[2], 0 if s is None else 1, dev=dev)
    s3 = None if s is None else (ctypes.c_double * 3)(*s)                  # host memory, read before the call returns
    _check(lib.vg_edt(_p(m), shape[0], shape[1], shape[2], s3, _p(out), EDT_SQUARED_I32 if squared else EDT_DIST_F32, _p(scratch), nbytes,
                      stream()), 'vg_edt')
    return out


def distance_transform_edt(mask, sampling=None, squared: bool = False):
    """scipy.ndimage.distance_transform_edt(mask, sampling) on the device: fp32 [X,Y,Z], the exact Euclidean distance of every foreground
    voxel to the nearest background voxel (0 on the background) -- the fp32 rounding of the fp64 square root of the exact squared
    distance.  sampling: None (voxel units; integer arithmetic), a number or three numbers, the voxel spacing along X, Y, Z (fp64
    arithmetic).  squared=True (sampling=None only): the int32 squared distances.  A volume WITHOUT any background voxel gives +inf
    everywhere (2^31 - 1 squared), where scipy returns numbers without meaning.  Needs X^2 + Y^2 + Z^2 < 2^31.  Enqueue-only; temporary
    device memory: 8 bytes per voxel, 16 with a sampling."""
    s = _sampling(sampling)
    if squared and s is not None:
        raise ValueError('squared=True returns the integer squared distances in voxel units: it takes no sampling')
    m, shape = _edt_volume(mask)
    with torch.cuda.device(m.device):
        return _edt(m, shape, s, bool(squared))


def _fill(m: torch.Tensor, shape) -> torch.Tensor:
    """The uint8 device mask m with its holes closed: the background components (connectivity 1) that reach no face become foreground."""
    dev, n = m.device, m.numel()
    labels, _, _ = _label((m == 0).view(torch.uint8), shape, 1)
    flags = torch.empty(sizes_capacity(n), dtype=torch.uint8, device=dev)
    out = torch.empty(shape, dtype=torch.uint8, device=dev)
    _check(lib.vg_fill_holes_mark(_p(labels), shape[0], shape[1], shape[2], _p(flags), stream()), 'vg_fill_holes_mark')
    _check(lib.vg_fill_holes_apply(_p(m), _p(labels), _p(flags), n, _p(out), stream()), 'vg_fill_holes_apply')
    return out


def fill_holes(mask):
    """scipy.ndimage.binary_fill_holes(mask) with its default structure, on the device: uint8 [X,Y,Z] (0 / 1), the mask with every
    background component that does not reach the border of the volume through face neighbours turned into foreground.  Enqueue-only;
    temporary device memory as label_components."""
    m, shape = _mask_volume(mask)
    with torch.cuda.device(m.device):
        return _fill(m, shape)


def vessel_radius(mask, sampling=None, fill: bool = True):
    """distance_transform_edt(fill_holes(mask) if fill else mask, sampling): the radius map of a vessel mask, fp32 [X,Y,Z].  fill=True
    closes hollow lumina first, so that a vessel is measured to its wall and not to its cavity.  Enqueue-only."""
    s = _sampling(sampling)
    if not fill:
        return distance_transform_edt(mask, s)
    m, shape = _edt_volume(mask, labelled=True)
    with torch.cuda.device(m.device):
        return _edt(_fill(m, shape), shape, s, False)


# ------------------------------------------------------------------------------------------------ the centreline (csrc/vg_skeleton.hip)
SKELETON_CHUNK = 4                         # passes enqueued between two read-backs when thinning until nothing changes
SKELETON_MAX_PASSES = 4096                 # VG_SKELETON_MAX_PASSES: the passes of one call of vg_skeleton_passes


def _max_passes(max_passes):
    if max_passes is None:
        return None
    try:
        k = operator.index(max_passes)
    except TypeError:
        raise ValueError('max_passes is None or an integer >= 1, got %r' % (max_passes,)) from None
    if isinstance(max_passes, bool) or k < 1:
        raise ValueError('max_passes is None or an integer >= 1, got %r' % (max_passes,))
    return k


def _skeleton_volume(mask):
    m, shape = _device_volume(mask, (torch.uint8, torch.bool), 'mask')
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), shape


def _thin(m: torch.Tensor, shape, max_passes, read: bool = False):
    """(skeleton, deleted): the uint8 device mask m thinned.  max_passes None: chunks of SKELETON_CHUNK passes, the counts of each read
    back, until a pass deleted nothing; deleted is the list of counts up to that 0.  An int: exactly that many passes, nothing read
    back unless read, deleted then the list of their counts, else None."""
    dev = m.device
    X, Y, Z = shape
    chunk = SKELETON_CHUNK if max_passes is None else min(max_passes, SKELETON_MAX_PASSES)
    scratch, nbytes = _scratch('vg_skeleton_scratch_bytes', X, Y, Z, chunk, dev=dev)
    counts = scratch[nbytes - (4 * chunk + 15) // 16 * 16:][:4 * chunk].view(torch.int32)      # the tail the query leaves for them
    _check(lib.vg_skeleton_begin(_p(m), X, Y, Z, _p(scratch), nbytes, stream()), 'vg_skeleton_begin')
    deleted, left = [], max_passes
    while True:
        k = chunk if left is None else min(left, chunk)
        _check(lib.vg_skeleton_passes(X, Y, Z, k, _p(scratch), nbytes, _p(counts), stream()), 'vg_skeleton_passes')
        if left is None or read:
            deleted += [int(c) for c in counts[:k].cpu()]
        if left is None:
            if 0 in deleted:
                deleted = deleted[:deleted.index(0) + 1]
                break
        else:
            left -= k
            if left == 0:
                break
    out = torch.empty(shape, dtype=torch.uint8, device=dev)
    _check(lib.vg_skeleton_end(X, Y, Z, _p(scratch), nbytes, _p(out), stream()), 'vg_skeleton_end')
    return out, (deleted if max_passes is None or read else None)


def skeletonize(mask, max_passes=None, return_info: bool = False):
    """The curve skeleton of mask on the device: uint8 [X,Y,Z] (0 / 1), a subset of the mask, one voxel wide, with the mask's topology
    -- the same 26-components of the foreground, 6-components of the background, tunnels and cavities -- and the end points of its
    branches kept.  Exact topological thinning by directional sub-iterations over eight parity subfields (include/vangan_hip.h has the
    algorithm): the result depends on the mask alone, bit for bit.  Foreground is 26-connected, the outside of the volume
    is background.  max_passes=None: thin until a pass deletes nothing -- passes are enqueued four at a time and their counts read back
    (a synchronising copy per chunk; a vessel of radius r needs about r + 1 passes, a solid block of side L about L / 2).  max_passes=k:
    exactly k passes, enqueue-only; the passes after one that deleted nothing do nothing.  return_info=True: (skeleton,
    dict(passes, deleted, converged)) -- the passes run, the voxels each deleted, and whether one of them deleted nothing; with
    max_passes=k this reads the k counts back.  A cavity stays enclosed by a closed surface of skeleton: fill_holes first where a
    hollow lumen is meant to be a vessel (vessel_centreline does).  Temporary device memory: a quarter of a byte per voxel."""
    k = _max_passes(max_passes)
    m, shape = _skeleton_volume(mask)
    with torch.cuda.device(m.device):
        out, deleted = _thin(m, shape, k, bool(return_info))
    if not return_info:
        return out
    return out, dict(passes=len(deleted), deleted=deleted, converged=0 in deleted)


def skeleton_nodes(skel):
    """uint8 [X,Y,Z]: for every foreground voxel of skel (a skeleton, or any mask) the number of its 26 neighbours that are
    foreground, 0 on the background.  On a skeleton 1 is an end point, 2 a voxel of a segment, 3 or more a junction (0: a voxel on its
    own).  Enqueue-only."""
    m, shape = _skeleton_volume(skel)
    with torch.cuda.device(m.device):
        out = torch.empty(shape, dtype=torch.uint8, device=m.device)
        _check(lib.vg_neighbour_count26(_p(m), shape[0], shape[1], shape[2], _p(out), stream()), 'vg_neighbour_count26')
    return out


def vessel_centreline(mask, sampling=None, fill: bool = True):
    """(skeleton, radius): skeletonize of the mask and vessel_radius(mask, sampling, fill) multiplied by it -- the radius of the vessel
    at every voxel of its centreline, 0 elsewhere (also where the radius is +inf: a volume without background); uint8 and fp32
    [X,Y,Z].  fill=True: both are taken of fill_holes(mask), so that a
    hollow lumen is measured to its wall and does not leave a shell of centreline around its cavity.  The thinning reads its counts
    back every four passes."""
    s = _sampling(sampling)
    m, shape = _edt_volume(mask, labelled=bool(fill))
    with torch.cuda.device(m.device):
        if fill:
            m = _fill(m, shape)
        skel = _thin(m, shape, None)[0]
        radius = _edt(m, shape, s, False)
        return skel, torch.where(skel != 0, radius, torch.zeros((), dtype=radius.dtype, device=radius.device))


# ------------------------------------------------------------------------------------------------ the vessel graph (csrc/vg_skelgraph.hip)
NODE_ISOLATED, NODE_END, NODE_OTHER = 0, 1, 2      # node_kind


class SkeletonGraph:
    """The graph of a skeleton as device tensors (include/vangan_hip.h "The vessel graph" has the definitions).  segment_labels and
    node_labels: int32 [X,Y,Z], 1 .. E on the voxels with two neighbours, 1 .. V on every other foreground voxel, numbered as
    scipy.ndimage.label numbers them; degree: uint8 [X,Y,Z], skeleton_nodes of the input.  E, V: ints.  Tables with E + 1 rows, row 0
    zeros: seg_voxels int32, seg_nodes int32 [.,2], seg_ends int64 [.,2] (linear indices, -1 for a cycle), seg_half_steps int64 [.,7],
    seg_length and seg_chord fp64; seg_radius_mean fp64, seg_radius_min / _max fp32 when a radius was given, else None.  Tables with
    V + 1 rows: node_voxels, node_degree int32, node_kind uint8 (NODE_ISOLATED, NODE_END, NODE_OTHER), node_centroid fp64 [.,3].
    shape, sampling: the (X, Y, Z) of the volume and the three spacings the lengths are in."""
    FIELDS = ('segment_labels', 'node_labels', 'degree', 'E', 'V', 'seg_voxels', 'seg_nodes', 'seg_ends', 'seg_half_steps', 'seg_length', 'seg_chord',
              'seg_radius_mean', 'seg_radius_min', 'seg_radius_max', 'node_voxels', 'node_degree', 'node_kind', 'node_centroid', 'shape', 'sampling')

    def __init__(self, **fields):
        assert set(fields) == set(self.FIELDS), sorted(set(fields) ^ set(self.FIELDS))
        self.__dict__.update(fields)

    def __repr__(self):
        return 'SkeletonGraph(E=%d, V=%d, shape=%s, sampling=%s)' % (self.E, self.V, self.shape, self.sampling)


def _graph_volume(skel):
    """A skeleton (or any mask) whose two classes of voxels are going to be labelled."""
    m, shape = _device_volume(skel, (torch.uint8, torch.bool), 'skel', labelled=True)
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), shape


def _s3(s):
    return None if s is None else (ctypes.c_double * 3)(*s)               # host memory, read before the call returns


def _graph(m: torch.Tensor, shape, radius, s) -> SkeletonGraph:
    dev = m.device
    X, Y, Z = shape
    deg, bm, nm = (torch.empty(shape, dtype=torch.uint8, device=dev) for _ in range(3))
    _check(lib.vg_skelgraph_classify(_p(m), X, Y, Z, _p(deg), _p(bm), _p(nm), stream()), 'vg_skelgraph_classify')
    seg_labels, _, res_b = _label(bm, shape, 3)
    node_labels, _, res_n = _label(nm, shape, 3)
    host = [int(w) for w in torch.cat([res_b, res_n]).cpu()]              # the one read-back that sizes the tables
    if host[R_STATUS] != 0 or host[4 + R_STATUS] != 0:
        raise RuntimeError('vg_cc_label reported status %d (segments), %d (nodes)' % (host[R_STATUS], host[4 + R_STATUS]))
    E, V = host[R_K], host[4 + R_K]

    def table(rows, dtype, *cols):
        return torch.empty((rows + 1,) + cols, dtype=dtype, device=dev)
    half, vox, ends, nodes = table(E, torch.int64, 7), table(E, torch.int32), table(E, torch.int64, 2), table(E, torch.int32, 2)
    length, chord = table(E, torch.float64), table(E, torch.float64)
    rmean = None if radius is None else table(E, torch.float64)
    rminmax = None if radius is None else table(E, torch.float32, 2)
    nvox, ndeg, kind, centroid = table(V, torch.int32), table(V, torch.int32), table(V, torch.uint8), table(V, torch.float64, 3)
    bad = torch.empty(2, dtype=torch.int32, device=dev)
    scratch, nbytes = _scratch('vg_skelgraph_scratch_bytes', E, V, dev=dev)
    _check(lib.vg_skelgraph_tables(_p(m), _p(deg), _p(seg_labels), _p(node_labels), None if radius is None else _p(radius), X, Y, Z, E, V, _s3(s),
                                   _p(half), _p(vox), _p(ends), _p(nodes), _p(length), _p(chord), None if rmean is None else _p(rmean),
                                   None if rminmax is None else _p(rminmax), _p(nvox), _p(ndeg), _p(kind), _p(centroid), _p(bad), _p(scratch), nbytes,
                                   stream()), 'vg_skelgraph_tables')
    if radius is not None:
        nbad = [int(w) for w in bad.cpu()]
        if nbad[0] or nbad[1]:
            raise RuntimeError('skeleton_graph: %d voxels of the skeleton have a radius that is negative, not finite or above the diagonal of the '
                               'volume (%d labels out of range)' % (nbad[0], nbad[1]))
    return SkeletonGraph(segment_labels=seg_labels, node_labels=node_labels, degree=deg, E=E, V=V, seg_voxels=vox, seg_nodes=nodes, seg_ends=ends,
                         seg_half_steps=half, seg_length=length, seg_chord=chord, seg_radius_mean=rmean,
                         seg_radius_min=None if rminmax is None else rminmax[:, 0], seg_radius_max=None if rminmax is None else rminmax[:, 1],
                         node_voxels=nvox, node_degree=ndeg, node_kind=kind, node_centroid=centroid, shape=tuple(shape),
                         sampling=(1.0, 1.0, 1.0) if s is None else s)


def skeleton_graph(skel, radius=None, sampling=None) -> SkeletonGraph:
    """The graph of a skeleton (uint8 / bool [X,Y,Z] on the device; any mask is legal) as a SkeletonGraph: the voxels with exactly two
    26-neighbours form the segments, every other voxel the nodes (a cluster of adjacent junction voxels is one node), both numbered as
    scipy.ndimage.label numbers them; per segment its voxels, its two end nodes and end voxels, its exact length under sampling (None,
    a number or three: the voxel spacing along X, Y, Z), the chord between its ends, and with radius (fp32 [X,Y,Z], such as vessel_radius
    or vessel_centreline returns) the mean, min and max radius along it; per node its voxels, attachments, kind and centroid.  Every
    number is a function of the input alone, bit for bit (integer atomics only).  Reads the two counts back once to size the tables
    (RuntimeError on a non-zero status of the labelling), and with a radius one more word: RuntimeError when a voxel of a segment has a
    radius that is negative, NaN, infinite or above the diagonal of the volume.  An empty mask gives E = V = 0 and tables of their zero
    row.  Temporary device memory: that of label_components, beside the two label volumes and three bytes per voxel."""
    s = _sampling(sampling)
    m, shape = _device_volume(skel, (torch.uint8, torch.bool), 'skel', labelled=True, check_device=False)
    r = None
    if radius is not None:
        r, rshape = _device_volume(radius, (torch.float32,), 'radius', check_device=False)
        if rshape != shape:
            raise ValueError('radius has shape %s, skel %s' % (rshape, shape))
    _on_device(m, 'skel')
    if r is not None:
        _on_device(r, 'radius')
        if r.device != m.device:
            raise ValueError('radius is on %s, skel on %s' % (r.device, m.device))
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    with torch.cuda.device(m.device):
        return _graph(m, shape, r, s)


def _min_length(min_length, what='min_length') -> float:
    if isinstance(min_length, bool) or not isinstance(min_length, numbers.Real) or math.isnan(min_length):
        raise ValueError('%s is a number (a length in the units of the sampling), got %r' % (what, min_length))
    return float(min_length)


def _rounds(rounds) -> int:
    try:
        k = operator.index(rounds)
    except TypeError:
        raise ValueError('rounds is an integer >= 1, got %r' % (rounds,)) from None
    if isinstance(rounds, bool) or k < 1:
        raise ValueError('rounds is an integer >= 1, got %r' % (rounds,))
    return k


def _prune_round(m: torch.Tensor, g: SkeletonGraph, min_length: float, s):
    """(mask, counts2) of one pruning round of the uint8 device mask m whose graph is g."""
    X, Y, Z = g.shape
    out = torch.empty(g.shape, dtype=torch.uint8, device=m.device)
    flags = torch.empty(g.E + 1, dtype=torch.uint8, device=m.device)
    counts = torch.empty(2, dtype=torch.int32, device=m.device)
    _check(lib.vg_skelgraph_prune(_p(m), _p(g.degree), _p(g.segment_labels), _p(g.node_labels), X, Y, Z, g.E, g.V, _p(g.seg_half_steps), _p(g.seg_nodes),
                                  _p(g.node_kind), min_length, _s3(s), _p(flags), _p(out), _p(counts), stream()), 'vg_skelgraph_prune')
    return out, counts


def prune_spurs(skel, min_length, sampling=None, rounds=1, return_info: bool = False):
    """skel (uint8 / bool [X,Y,Z] on the device) without its short spurs, uint8 (0 / 1): a spur is a segment between an end point and a
    node that is none, shorter than min_length (in the units of sampling); a round deletes the voxels of every spur and the end voxel
    it hangs from, and nothing else -- the connected components and the Euler characteristic stay, a segment between two end points
    and every cycle stay.  Each of up to `rounds` rounds is a skeleton_graph of what the round before left (removing a spur can turn
    its junction into a voxel of a longer segment, which the next round may find to be a spur) and one launch pair; with rounds > 1 or
    return_info the two counts of each round are read back and the rounds stop after one that removed nothing.  return_info=True:
    (mask, dict(rounds, spurs, voxels)) -- the rounds run and the spurs and voxels each removed.  min_length <= 0 returns a copy."""
    ml = _min_length(min_length)
    k = _rounds(rounds)
    s = _sampling(sampling)
    m, shape = _graph_volume(skel)
    info = dict(rounds=0, spurs=[], voxels=[])
    with torch.cuda.device(m.device):
        cur = m
        if ml > 0.0:
            for _ in range(k):
                cur, counts = _prune_round(cur, _graph(cur, shape, None, s), ml, s)
                info['rounds'] += 1
                if k > 1 or return_info:
                    c = [int(w) for w in counts.cpu()]
                    info['spurs'].append(c[0])
                    info['voxels'].append(c[1])
                    if c[1] == 0:
                        break
        out = (m != 0).to(torch.uint8) if cur is m else cur
    return (out, info) if return_info else out


def network_summary(graph: SkeletonGraph) -> dict:
    """Numbers about the network of a SkeletonGraph, as a dict on the host (one read-back of the tables): segments, cycles (closed
    segments without a node), loops (both ends at one node), nodes, end_points, junctions (the nodes of kind NODE_OTHER), isolated
    (voxels on their own), total_length, length_density (total length per unit volume, the volume being that of the whole array under
    the sampling), mean_radius (weighted by the voxels of the segments; None without a radius) and mean_tortuosity (the mean of
    length / chord over the segments with chord > 0; None where there is none)."""
    if not isinstance(graph, SkeletonGraph):
        raise ValueError('network_summary takes a SkeletonGraph, got %s' % type(graph).__name__)
    g = graph
    has_r = g.seg_radius_mean is not None
    cols = [g.seg_length, g.seg_chord, g.seg_voxels.double(), g.seg_nodes[:, 0].double(), g.seg_nodes[:, 1].double(), g.seg_ends[:, 0].double()]
    if has_r:
        cols.append(g.seg_radius_mean)
    host = torch.cat(cols + [g.node_kind.double()]).cpu().numpy()         # every integer here is below 2^31: exact in fp64
    E1 = g.E + 1
    length, chord, vox, n0, n1, e0 = (host[i * E1 + 1:(i + 1) * E1] for i in range(6))
    kind = host[len(cols) * E1 + 1:]
    total = float(length.sum())
    volume = math.prod(g.shape) * math.prod(g.sampling)
    curved = chord > 0
    return dict(segments=g.E, cycles=int((e0 < 0).sum()), loops=int(((n0 == n1) & (n0 > 0)).sum()), nodes=g.V,
                end_points=int((kind == NODE_END).sum()), junctions=int((kind == NODE_OTHER).sum()), isolated=int((kind == NODE_ISOLATED).sum()),
                total_length=total, length_density=total / volume,
                mean_radius=(float((host[6 * E1 + 1:7 * E1] * vox).sum() / vox.sum()) if has_r and vox.sum() > 0 else None),
                mean_tortuosity=float((length[curved] / chord[curved]).mean()) if curved.any() else None)


def vessel_graph(mask, sampling=None, fill: bool = True, min_spur=0.0):
    """(skeleton, graph): vessel_centreline(mask, sampling, fill), then prune_spurs(skeleton, min_spur, sampling) when min_spur > 0, then
    skeleton_graph of the skeleton with the radius map along it -- the network of a vessel mask with length and radius per vessel.
    A volume without any background voxel has an infinite radius, which skeleton_graph refuses."""
    s = _sampling(sampling)
    ms = _min_length(min_spur, 'min_spur')
    skel, radius = vessel_centreline(mask, s, fill)
    if ms > 0.0:
        skel = prune_spurs(skel, ms, s)
    return skel, skeleton_graph(skel, radius, s)
