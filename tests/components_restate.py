"""numpy / scipy restatement of the prediction post-processing (van_gan_amd/postprocess.py, csrc/vg_components.hip): what the GPU suite
(tests/test_gpu_components.py) compares by equality, pinned on the CPU by tests/test_components_host.py.  Not a test module.

label: scipy.ndimage.label with generate_binary_structure(3, connectivity); it numbers components in raster order of their first voxel
(checked in test_components_host.py), which is the contract of vg_cc_label.  remove_small: skimage.morphology.remove_small_objects is
ndi.label + np.bincount + a comparison (skimage is not installed; that is its implementation).  otsu: skimage's threshold_otsu on 256
bins, restated: weight1 = cumsum(h), weight2 = cumsum(h[::-1])[::-1], the means likewise, var12 = weight1[:-1] * weight2[1:] *
(mean1[:-1] - mean2[1:]) ** 2 in float64, the first maximum; where a weight is 0 the mean is undefined and the split's variance is taken
as 0 (skimage never meets the case: it bins between the image's extremes)."""
import numpy as np
import scipy.ndimage as ndi


def structure(connectivity):
    return ndi.generate_binary_structure(3, connectivity)


def label(mask, connectivity):
    """(labels int32, K)"""
    lab, K = ndi.label(np.asarray(mask) != 0, structure=structure(connectivity))
    return lab.astype(np.int32), int(K)


def sizes(labels, K):
    """voxel counts [K + 1], [0] the background's"""
    return np.bincount(labels.ravel(), minlength=K + 1).astype(np.int64)


def remove_small(mask, min_size, connectivity):
    """uint8 0 / 1: the voxels of the components with at least min_size voxels"""
    lab, K = label(mask, connectivity)
    keep = sizes(lab, K) >= min_size
    keep[0] = False
    return keep[lab].astype(np.uint8)


def relabel_kept(mask, min_size, connectivity):
    """(labels of the kept components renumbered 1 .. K' in the same order, K')"""
    lab, K = label(mask, connectivity)
    keep = sizes(lab, K) >= min_size
    keep[0] = False
    newid = np.where(keep, np.cumsum(keep), 0).astype(np.int32)
    return newid[lab], int(keep.sum())


def as_u8(pred):
    """pred.astype('uint8') (custom_callback.py:205) for finite values in [0, 256): C truncation"""
    return np.asarray(pred, np.float32).astype(np.uint8)


def hist256(pred):
    p = np.asarray(pred, np.float32).ravel()
    return np.bincount(as_u8(p[np.isfinite(p)]), minlength=256).astype(np.int64)


def otsu_var12(hist):
    """float64 [255]: the between-class variance (times n^2) of the split after bin i"""
    h = np.asarray(hist).astype(np.float64)
    b = np.arange(256, dtype=np.float64)
    weight1 = np.cumsum(h)
    weight2 = np.cumsum(h[::-1])[::-1]
    with np.errstate(divide='ignore', invalid='ignore'):
        mean1 = np.cumsum(h * b) / weight1
        mean2 = (np.cumsum((h * b)[::-1]) / weight2[::-1])[::-1]
        var12 = weight1[:-1] * weight2[1:] * (mean1[:-1] - mean2[1:]) ** 2
    return np.where((weight1[:-1] == 0) | (weight2[1:] == 0), 0.0, var12)


def otsu(hist):
    return int(np.argmax(otsu_var12(hist)))                        # the first maximum


def binarise(pred, threshold):
    """threshold: 'otsu', an int (uint8(pred) > t) or a float (pred > t in fp32); non-finite voxels are background"""
    p = np.asarray(pred, np.float32)
    fin = np.isfinite(p)
    q = np.where(fin, p, np.float32(0))
    if isinstance(threshold, str):
        m = as_u8(q) > otsu(hist256(p))
    elif isinstance(threshold, (int, np.integer)):
        m = as_u8(q).astype(np.float32) > np.float32(threshold)
    else:
        m = q > np.float32(threshold)
    return (m & fin).astype(np.uint8)


def vessel_mask(pred, threshold=127.5, min_size=64, connectivity=3):
    pred = np.asarray(pred, np.float32)
    pred = pred[..., 0] if pred.ndim == 4 else pred
    return remove_small(binarise(pred, threshold), min_size, connectivity)


# ------------------------------------------------------------------------------------------------ masks that break a tiled union-find
def bernoulli(shape, p, seed=0):
    return (np.random.default_rng(seed + sum((i + 2) * s for i, s in enumerate(shape))).random(shape) < p).astype(np.uint8)


def checkerboard(shape):
    return (np.indices(shape).sum(0) % 2 == 0).astype(np.uint8)


def snake(shape):
    """A single 6-connected path, one voxel wide, with no shortcuts: plane x holds rows y = 0, 2, 4, ... filled along z and joined at
    alternating z ends; planes 0, 2, 4, ... hold such a layer, and a single voxel in the odd plane between two layers joins them at
    alternating ends of the layer's path."""
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8)
    ys = list(range(0, Y, 2))
    ends = []
    for xi, x in enumerate(range(0, X, 2)):
        for i, y in enumerate(ys):
            m[x, y, :] = 1
            if i + 1 < len(ys):
                m[x, y + 1, (Z - 1) if i % 2 == 0 else 0] = 1
        first = (ys[0], 0)
        last = (ys[-1], (Z - 1) if (len(ys) - 1) % 2 == 0 else 0)
        ends.append((first, last))
    for xi, x in enumerate(range(0, X - 2, 2)):                        # join layer x to layer x + 2 at the end where its path stops
        y, z = ends[xi][1] if xi % 2 == 0 else ends[xi][0]
        m[x + 1, y, z] = 1
    return m


def rods(shape, touch):
    """Two rods along z that cross the tile corner (8, 8, 64) and touch only by their edges ('edge': rows (7, 7) and (8, 8), all z) or only
    by one corner ('corner': (7, 7, z < 64) and (8, 8, z >= 64)): connectivity 1 sees two components in both, connectivity 2 joins the
    first pair only, connectivity 3 both."""
    m = np.zeros(shape, np.uint8)
    if touch == 'edge':
        m[7, 7, :] = 1
        m[8, 8, :] = 1
    else:
        m[7, 7, :64] = 1
        m[8, 8, 64:] = 1
    return m


def corner_chain(shape):
    """The diagonal (k, k, 56 + k), k = 0 .. 15: every link is a corner link, and the one from k = 7 to 8 crosses a tile boundary on all
    three axes at once -- one component at connectivity 3, sixteen below it."""
    m = np.zeros(shape, np.uint8)
    for k in range(16):
        m[k, k, 56 + k] = 1
    return m
