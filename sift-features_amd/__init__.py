"""sift_features_amd -- MI355X-native SIFT hot path (gfx950 HIP kernels behind a
C ABI, include/sift_mi.h), a drop-in for tnibler/sift-features' `sift()`.

See sift.py for the reference API mirror and DESIGN.md for the design.
"""
from ._lib import SiftMiError, lib  # noqa: F401
from .sift import (  # noqa: F401
    DESCRIPTOR_SIZE, Context, ImageprocProcessing, KeyPoint, OpenCVProcessing, PrecomputedImages, Processing,
    ResultBuffers, Tracks, build_tracks_device, track_frames,
    pair_counters, propose_frames, propose_pairs_device,
    Selection, select_counters, select_frames, select_keypoints, select_spread_device,
    SiftResult, compute_descriptor, decode_jpeg, default_context, jpeg_dims, key_fields, match_descriptors,
    match_frames, match_frames_guided, match_guided, match_neighbors, match_pairs_device, match_pairs_guided_device,
    precompute_images, sift,
    sift_with_precomputed,
    sift_with_processing, stable_sort_xy_size, verify_frames, verify_matches, verify_pairs_device)

__version__ = "0.1.0"
