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
(csrc/vg_skelgraph.hip); skeleton_graph reads the two counts back once to size its tables.  Last, what says how
good a mask is against a ground truth: overlap, clDice, Betti numbers and Euler characteristic, surface distances
(csrc/vg_evaluate.hip); evaluate_segmentation enqueues all of it and reads one small block back.

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
import struct
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


# ------------------------------------------------------------------------------------------------ scoring the mask (csrc/vg_evaluate.hip)
EVAL_SQ_I32, EVAL_DIST_F32 = 0, 1          # VG_EVAL_SQ_I32, VG_EVAL_DIST_F32
EVAL_MAX_STATS, EVAL_STATS_BYTES = 4, 40   # VG_EVAL_MAX_STATS, VG_EVAL_STATS_BYTES


class SegmentationScores:
    """What evaluate_segmentation returns, all on the host.  The integers: shape, voxels; tp, fp, fn, tn (pred & truth, pred & !truth,
    !pred & truth, neither).  From them, in fp64: dice = 2 tp / (2 tp + fp + fn), iou = tp / (tp + fp + fn), precision = tp / (tp + fp),
    recall = tp / (tp + fn), specificity = tn / (tn + fp), accuracy = (tp + tn) / voxels.  With cldice: skeleton_pred, skeleton_truth (the
    voxels of the two skeletons), skeleton_pred_in_truth, skeleton_truth_in_pred, tprec = skeleton_pred_in_truth / skeleton_pred, tsens =
    skeleton_truth_in_pred / skeleton_truth, cldice = 2 tprec tsens / (tprec + tsens).  With topology: betti_pred, betti_truth ((b0, b1,
    b2): 26-components, tunnels, cavities; b1 = b0 + b2 - euler), euler_pred, euler_truth, betti_error (the three absolute differences)
    and euler_error.  With surface: surface_pred, surface_truth (the surface voxels), pred_to_truth and truth_to_pred (dict(count,
    max_key, percentile_key, max, mean, percentile): over the surface voxels of the first mask, the distance to the surface of the
    second -- the two keys are the device's integers, a squared distance without sampling and the bits of an fp32 distance with it,
    and value(key) is sqrt(key) or that fp32 number; max = value(max_key), mean = sum / count, percentile = value(percentile_key), the key of
    rank max(ceil(percentile / 100 * count) - 1, 0)), hausdorff = max of the two max, hausdorff_percentile = max of the two percentile,
    assd = (sum + sum) / (count + count), and the percentile and sampling they were taken with.  A part that was not asked for is None.
    Both masks empty: dice = iou = precision = recall = cldice = tprec = tsens = 1 and every distance is 0.  Exactly one empty: those are 0
    and every distance is inf.  Any other ratio 0 / 0 -- specificity without a negative, cldice of two masks whose skeletons miss each other
    entirely -- is nan."""
    FIELDS = ('shape', 'voxels', 'tp', 'fp', 'fn', 'tn', 'dice', 'iou', 'precision', 'recall', 'specificity', 'accuracy',
              'skeleton_pred', 'skeleton_truth', 'skeleton_pred_in_truth', 'skeleton_truth_in_pred', 'tprec', 'tsens', 'cldice',
              'betti_pred', 'betti_truth', 'euler_pred', 'euler_truth', 'betti_error', 'euler_error',
              'surface_pred', 'surface_truth', 'pred_to_truth', 'truth_to_pred', 'hausdorff', 'hausdorff_percentile', 'assd', 'percentile', 'sampling')

    def __init__(self, **fields):
        assert set(fields) == set(self.FIELDS), sorted(set(fields) ^ set(self.FIELDS))
        self.__dict__.update(fields)

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f in self.FIELDS}

    def __repr__(self):
        return 'SegmentationScores(shape=%s, dice=%r, cldice=%r, hausdorff=%r)' % (self.shape, self.dice, self.cldice, self.hausdorff)


def _percentile(percentile) -> float:
    if isinstance(percentile, bool) or not isinstance(percentile, numbers.Real) or not (0.0 < percentile <= 100.0):
        raise ValueError('percentile is a number in (0, 100], got %r' % (percentile,))
    return float(percentile)


def _score_volume(mask, what: str, labelled: bool = False):
    m, shape = _device_volume(mask, (torch.uint8, torch.bool), what, labelled=labelled)
    return (m.view(torch.uint8) if m.dtype == torch.bool else m), shape


def _score_pair(pred, truth, labelled: bool = False, distances: bool = False):
    """(pred, truth, shape) as uint8 device volumes of one shape on one device."""
    p, shape = _device_volume(pred, (torch.uint8, torch.bool), 'pred', labelled=labelled, check_device=False)
    t, tshape = _device_volume(truth, (torch.uint8, torch.bool), 'truth', labelled=labelled, check_device=False)
    if tshape != shape:
        raise ValueError('truth has shape %s, pred %s' % (tshape, shape))
    if distances and sum(d * d for d in shape) >= 2 ** 31:
        raise ValueError('pred of shape %s: the distance transform serves X^2 + Y^2 + Z^2 < 2^31' % (shape,))
    _on_device(p, 'pred')
    _on_device(t, 'truth')
    if t.device != p.device:
        raise ValueError('truth is on %s, pred on %s' % (t.device, p.device))
    return (p.view(torch.uint8) if p.dtype == torch.bool else p), (t.view(torch.uint8) if t.dtype == torch.bool else t), shape


class _Block:
    """A small zeroed result block on the device, filled by the entries through pointers into it and read back in one copy."""

    def __init__(self, nbytes: int, dev):
        self.t = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self.host = None

    def at(self, off: int) -> int:
        return self.t.data_ptr() + off

    def put(self, off: int, words: torch.Tensor):
        """a device-to-device copy of a small tensor into the block (enqueue-only)"""
        raw = words.contiguous().view(torch.uint8).reshape(-1)
        self.t[off:off + raw.numel()].copy_(raw)

    def read(self):
        self.host = self.t.cpu().numpy()                             # the one synchronising read-back

    def get(self, off: int, dtype: str, count: int = 1):
        return [v.item() for v in self.host[off:off + count * int(dtype[1:])].view(dtype)]


def _enqueue_counts(a: torch.Tensor, b: torch.Tensor, blk: _Block, off: int):
    _check(lib.vg_mask_counts(_p(a), _p(b), a.numel(), blk.at(off), stream()), 'vg_mask_counts')


def _enqueue_surface(m: torch.Tensor, shape, blk: _Block, off: int, want_surf: bool = True, want_not: bool = True):
    """(surf, not_surf) of the uint8 device mask m, the count of surface voxels into the block."""
    surf = torch.empty(shape, dtype=torch.uint8, device=m.device) if want_surf else None
    nsurf = torch.empty(shape, dtype=torch.uint8, device=m.device) if want_not else None
    _check(lib.vg_mask_surface(_p(m), shape[0], shape[1], shape[2], _p(surf), _p(nsurf), blk.at(off), stream()), 'vg_mask_surface')
    return surf, nsurf


TOPOLOGY_BYTES = 80                        # cells5 (40) | result4 of the mask at connectivity 3 (16) | of its inverse at 1 (16) | cavities (4) | 0 (4)


def _enqueue_topology(m: torch.Tensor, shape, blk: _Block, off: int):
    dev, n = m.device, m.numel()
    _check(lib.vg_euler_characteristic(_p(m), shape[0], shape[1], shape[2], blk.at(off), stream()), 'vg_euler_characteristic')
    blk.put(off + 40, _label(m, shape, 3)[2])
    labels, _, result = _label((m == 0).view(torch.uint8), shape, 1)
    flags = torch.empty(sizes_capacity(n), dtype=torch.uint8, device=dev)
    _check(lib.vg_fill_holes_mark(_p(labels), shape[0], shape[1], shape[2], _p(flags), stream()), 'vg_fill_holes_mark')
    _check(lib.vg_flags_count(_p(flags), _p(result), n, blk.at(off + 72), stream()), 'vg_flags_count')
    blk.put(off + 56, result)


def _read_topology(blk: _Block, off: int):
    """((b0, b1, b2), euler) from the block after its read-back."""
    cells = blk.get(off, 'i8', 5)
    fg, bg, b2 = blk.get(off + 40, 'i4', 4), blk.get(off + 56, 'i4', 4), blk.get(off + 72, 'u4')[0]
    if fg[R_STATUS] != 0 or bg[R_STATUS] != 0:
        raise RuntimeError('vg_cc_label reported status %d (mask), %d (background)' % (fg[R_STATUS], bg[R_STATUS]))
    b0, chi = fg[R_K], cells[4]
    return (b0, b0 + b2 - chi, b2), chi


def _enqueue_distances(sel: torch.Tensor, nsurf_other: torch.Tensor, shape, s, q: float, blk: _Block, off: int):
    """Statistics, over the voxels of sel, of the distance to the nearest zero of nsurf_other."""
    dev, n = sel.device, sel.numel()
    keys = _edt(nsurf_other, shape, s, s is None)
    scratch, nbytes = _scratch('vg_masked_stats_scratch_bytes', n, 1, dev=dev)
    _check(lib.vg_masked_stats(_p(keys), _p(sel), n, EVAL_SQ_I32 if s is None else EVAL_DIST_F32, (ctypes.c_double * 1)(q), 1, blk.at(off), _p(scratch),
                               nbytes, stream()), 'vg_masked_stats')


def _key_value(key: int, weighted: bool) -> float:
    """the value of a key of vg_masked_stats: the fp32 number with these bits, or the square root of the integer"""
    return struct.unpack('<f', struct.pack('<I', key))[0] if weighted else math.sqrt(key)


def _read_distances(blk: _Block, off: int, weighted: bool):
    m, = blk.get(off, 'u8')
    kmax, = blk.get(off + 8, 'u4')
    total, = blk.get(off + 16, 'f8')
    kq, = blk.get(off + 24, 'u4')
    return dict(count=m, max_key=kmax, percentile_key=kq, max=_key_value(kmax, weighted), mean=total / m if m else 0.0,
                percentile=_key_value(kq, weighted)), total


def _surface_figures(pt, tp, sums) -> dict:
    """The two directions joined; an empty surface on exactly one side makes every distance infinite."""
    if (pt['count'] == 0) != (tp['count'] == 0):
        for d in (pt, tp):
            d.update(max=math.inf, mean=math.inf, percentile=math.inf)
        return dict(pred_to_truth=pt, truth_to_pred=tp, hausdorff=math.inf, hausdorff_percentile=math.inf, assd=math.inf)
    both = pt['count'] + tp['count']
    return dict(pred_to_truth=pt, truth_to_pred=tp, hausdorff=max(pt['max'], tp['max']), hausdorff_percentile=max(pt['percentile'], tp['percentile']),
                assd=(sums[0] + sums[1]) / both if both else 0.0)


def _ratio(a: int, b: int) -> float:
    return a / b if b else math.nan


def _overlap_figures(tp: int, fp: int, fn: int, tn: int) -> dict:
    if tp + fp == 0 or tp + fn == 0:                                 # a mask is empty: 1 when both are, else 0
        v = 1.0 if tp + fp + fn == 0 else 0.0
        dice = iou = precision = recall = v
    else:
        dice, iou, precision, recall = _ratio(2 * tp, 2 * tp + fp + fn), _ratio(tp, tp + fp + fn), _ratio(tp, tp + fp), _ratio(tp, tp + fn)
    return dict(tp=tp, fp=fp, fn=fn, tn=tn, dice=dice, iou=iou, precision=precision, recall=recall, specificity=_ratio(tn, tn + fp),
                accuracy=_ratio(tp + tn, tp + fp + fn + tn))


def _cldice_figures(sp_in_t: int, sp: int, st_in_p: int, st: int) -> dict:
    if sp == 0 or st == 0:                                           # a skeleton is empty exactly when its mask is
        tprec = tsens = cldice = 1.0 if sp + st == 0 else 0.0
    else:
        tprec, tsens = sp_in_t / sp, st_in_p / st
        cldice = 2.0 * tprec * tsens / (tprec + tsens) if tprec + tsens > 0.0 else math.nan
    return dict(skeleton_pred=sp, skeleton_truth=st, skeleton_pred_in_truth=sp_in_t, skeleton_truth_in_pred=st_in_p, tprec=tprec, tsens=tsens,
                cldice=cldice)


def overlap_counts(pred, truth) -> Tuple[int, int, int, int]:
    """(tp, fp, fn, tn) of two masks (uint8 / bool [X,Y,Z] on the device, one shape): the voxels in both, in pred alone, in truth alone,
    in neither, as Python ints.  One launch and one read-back of the four counters."""
    p, t, _ = _score_pair(pred, truth)
    with torch.cuda.device(p.device):
        blk = _Block(32, p.device)
        _enqueue_counts(p, t, blk, 0)
        blk.read()
    return tuple(blk.get(0, 'u8', 4))


def mask_surface(mask, return_count: bool = False):
    """uint8 [X,Y,Z] (0 / 1): the foreground voxels of mask with a face neighbour that is background or outside the volume -- mask &
    ~scipy.ndimage.binary_erosion(mask, generate_binary_structure(3, 1), border_value=0).  Enqueue-only; return_count=True: (surface,
    voxels) with the count read back."""
    m, shape = _score_volume(mask, 'mask')
    with torch.cuda.device(m.device):
        blk = _Block(8, m.device)
        surf, _ = _enqueue_surface(m, shape, blk, 0, want_not=False)
        if not return_count:
            return surf
        blk.read()
    return surf, blk.get(0, 'u8')[0]


def euler_characteristic(mask) -> int:
    """The Euler characteristic of the foreground of mask (26-connected, background 6-connected, outside the volume background): vertices
    - edges + faces - cubes of its closed cubical complex, counted on the device; one read-back."""
    m, shape = _score_volume(mask, 'mask')
    with torch.cuda.device(m.device):
        blk = _Block(40, m.device)
        _check(lib.vg_euler_characteristic(_p(m), shape[0], shape[1], shape[2], blk.at(0), stream()), 'vg_euler_characteristic')
        blk.read()
    return blk.get(0, 'i8', 5)[4]


def betti_numbers(mask) -> Tuple[int, int, int]:
    """(b0, b1, b2) of the foreground of mask under the convention of skeletonize: b0 its 26-components (label_components at connectivity
    3), b2 its cavities -- the 6-components of the background that reach no face of the volume -- and b1 = b0 + b2 - euler_characteristic,
    its tunnels.  One read-back (RuntimeError on a non-zero status of a labelling).  Temporary device memory as label_components."""
    m, shape = _score_volume(mask, 'mask', labelled=True)
    with torch.cuda.device(m.device):
        blk = _Block(TOPOLOGY_BYTES, m.device)
        _enqueue_topology(m, shape, blk, 0)
        blk.read()
    return _read_topology(blk, 0)[0]


def surface_distances(pred, truth, sampling=None, percentile=95.0) -> dict:
    """The distances between the surfaces (mask_surface) of two masks, as a dict on the host: surface_pred, surface_truth (voxels),
    pred_to_truth and truth_to_pred, hausdorff, hausdorff_percentile, assd, percentile, sampling -- the fields of SegmentationScores,
    defined there.  Without sampling the distances are exact: integer squared distances on the device, the square root of each in fp64;
    with sampling (a number or three, the voxel spacing) they are the fp32 distances of distance_transform_edt.  The sums are fp64, added
    in a fixed order: equal inputs give equal bits.  The percentile is the nearest-rank one of each direction.  One read-back; the two
    transforms are enqueued whatever the masks hold, and an empty surface is told from the counts afterwards."""
    s, q = _sampling(sampling), _percentile(percentile) / 100.0
    p, t, shape = _score_pair(pred, truth, distances=True)
    with torch.cuda.device(p.device):
        blk = _Block(16 + 2 * EVAL_STATS_BYTES, p.device)
        _enqueue_surfaces_and_distances(p, t, shape, s, q, blk, 0)
        blk.read()
    return _read_surfaces_and_distances(blk, 0, s, percentile)


def _enqueue_surfaces_and_distances(p, t, shape, s, q, blk: _Block, off: int):
    """block: surface voxels of pred (8) | of truth (8) | statistics pred -> truth | truth -> pred"""
    surf_p, nsurf_p = _enqueue_surface(p, shape, blk, off)
    surf_t, nsurf_t = _enqueue_surface(t, shape, blk, off + 8)
    _enqueue_distances(surf_p, nsurf_t, shape, s, q, blk, off + 16)
    _enqueue_distances(surf_t, nsurf_p, shape, s, q, blk, off + 16 + EVAL_STATS_BYTES)


def _read_surfaces_and_distances(blk: _Block, off: int, s, percentile) -> dict:
    pt, sum_pt = _read_distances(blk, off + 16, s is not None)
    tp, sum_tp = _read_distances(blk, off + 16 + EVAL_STATS_BYTES, s is not None)
    out = dict(surface_pred=blk.get(off, 'u8')[0], surface_truth=blk.get(off + 8, 'u8')[0])
    out.update(_surface_figures(pt, tp, (sum_pt, sum_tp)))
    out.update(percentile=float(percentile), sampling=(1.0, 1.0, 1.0) if s is None else s)
    return out


def _enqueue_cldice(p, t, shape, k, blk: _Block, off: int):
    """block: counts4 of (skeleton of pred, truth) | counts4 of (skeleton of truth, pred)"""
    _enqueue_counts(_thin(p, shape, k)[0], t, blk, off)
    _enqueue_counts(_thin(t, shape, k)[0], p, blk, off + 32)


def _read_cldice(blk: _Block, off: int) -> dict:
    a, b = blk.get(off, 'u8', 4), blk.get(off + 32, 'u8', 4)
    return _cldice_figures(a[0], a[0] + a[1], b[0], b[0] + b[1])


def cldice_score(pred, truth, max_passes=None) -> dict:
    """The hard clDice of two masks, as a dict on the host: with S = skeletonize of each mask as it is given (no hole filling), tprec =
    |S_pred & truth| / |S_pred|, tsens = |S_truth & pred| / |S_truth| and cldice = 2 tprec tsens / (tprec + tsens), beside the four
    integers (the fields of SegmentationScores).  max_passes=None thins until nothing changes, which reads a few words back every four
    passes, as skeletonize does; max_passes=k runs exactly k passes and is enqueue-only up to the one read-back of the counts."""
    k = _max_passes(max_passes)
    p, t, shape = _score_pair(pred, truth)
    with torch.cuda.device(p.device):
        blk = _Block(64, p.device)
        _enqueue_cldice(p, t, shape, k, blk, 0)
        blk.read()
    return _read_cldice(blk, 0)


def evaluate_segmentation(pred, truth, sampling=None, percentile=95.0, topology: bool = True, surface: bool = True, cldice: bool = True,
                          max_passes=None) -> SegmentationScores:
    """Score the mask pred against the ground truth (both uint8 / bool [X,Y,Z] on the device, one shape) without leaving the device:
    overlap (overlap_counts), and as asked for clDice (cldice_score), the Betti numbers and the Euler characteristic of both masks
    (betti_numbers) and the surface distances (surface_distances, under sampling and percentile).  Returns a SegmentationScores, where
    every formula and the degenerate cases are written down.  Every integer is counted on the device; the ratios are formed on the host
    in fp64 from the integers.  Everything is enqueued first and one small block is read back at the end -- the one synchronising
    step, except that cldice=True with max_passes=None thins until nothing changes, which reads its counts back every four passes
    (skeletonize); max_passes=k thins exactly k passes and keeps the call to the one read-back.  RuntimeError on a non-zero status of
    a labelling.  Needs X^2 + Y^2 + Z^2 < 2^31 with surface=True."""
    s, q = _sampling(sampling), _percentile(percentile) / 100.0
    k = _max_passes(max_passes)
    p, t, shape = _score_pair(pred, truth, labelled=bool(topology), distances=bool(surface))
    o_cl, o_top, o_surf = 32, 96, 96 + 2 * TOPOLOGY_BYTES
    with torch.cuda.device(p.device):
        blk = _Block(o_surf + 16 + 2 * EVAL_STATS_BYTES, p.device)
        _enqueue_counts(p, t, blk, 0)
        if cldice:
            _enqueue_cldice(p, t, shape, k, blk, o_cl)
        if topology:
            _enqueue_topology(p, shape, blk, o_top)
            _enqueue_topology(t, shape, blk, o_top + TOPOLOGY_BYTES)
        if surface:
            _enqueue_surfaces_and_distances(p, t, shape, s, q, blk, o_surf)
        blk.read()
    f = dict.fromkeys(SegmentationScores.FIELDS)
    f.update(shape=tuple(shape), voxels=math.prod(shape))
    f.update(_overlap_figures(*blk.get(0, 'u8', 4)))
    if cldice:
        f.update(_read_cldice(blk, o_cl))
    if topology:
        (bp, cp), (bt, ct) = _read_topology(blk, o_top), _read_topology(blk, o_top + TOPOLOGY_BYTES)
        f.update(betti_pred=bp, betti_truth=bt, euler_pred=cp, euler_truth=ct, betti_error=tuple(abs(a - b) for a, b in zip(bp, bt)),
                 euler_error=abs(cp - ct))
    if surface:
        f.update(_read_surfaces_and_distances(blk, o_surf, s, percentile))
    return SegmentationScores(**f)
