"""van_gan_amd -- MI355X-native engine for the VAN-GAN ``train_step`` hot path (psweens/VAN-GAN vangan.py).

The package directory is spelled with underscores (``van_gan_amd``) because a hyphen is not importable in
Python.  Importing it builds/loads ``libvangan_hip.so`` (hand-written gfx950 HIP kernels behind the C ABI of
``include/vangan_hip.h``); there is no CPU or eager-PyTorch fallback for the data path.
"""
from . import _lib  # noqa: F401  (fails loudly when the HIP library cannot be built/loaded)
from .vangan import NETS, RESULT_KEYS, VanGan  # noqa: F401
from .preprocess import (lanczos4_table, median_filter, order_stats, outlier_limits, percentiles, prepare_imaging,  # noqa: F401
                         prepare_segmentation, preprocess_rsom_images, resize_volume, slice_moments, threshold_outliers, value_mode,
                         volume_moments, zscore_slices)
from .postprocess import binarise_prediction, histogram256, label_components, remove_small_objects, vessel_mask  # noqa: F401
from .postprocess import distance_transform_edt, fill_holes, vessel_radius  # noqa: F401
from .postprocess import skeleton_nodes, skeletonize, vessel_centreline  # noqa: F401
from .postprocess import SkeletonGraph, network_summary, prune_spurs, skeleton_graph, vessel_graph  # noqa: F401
from .postprocess import (SegmentationScores, betti_numbers, cldice_score, euler_characteristic, evaluate_segmentation, mask_surface,  # noqa: F401
                          overlap_counts, surface_distances)
