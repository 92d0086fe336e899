"""C-ABI boundary of the progressive verification calls that needs no GPU: the
four symbols are exported, null arguments are rejected before the context is
touched with nothing written (quality alone may be null), and the bindings
carry the new keywords."""
import ctypes
import inspect

import pytest

PAIR_CALLS = ("sift_mi_verify_pairs_progressive_device", "sift_mi_verify_pairs_epipolar_progressive_device")
ONE_PAIR_CALLS = ("sift_mi_verify_matches_progressive", "sift_mi_verify_matches_epipolar_progressive")


def test_progressive_symbols_exported(pkg):
    from sift_features_amd import _lib
    L = pkg.lib()
    for name in PAIR_CALLS + ONE_PAIR_CALLS:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
        assert getattr(L, name).argtypes is not None
    assert "0.5.0" in L.sift_mi_version().decode()


def test_progressive_null_arguments_rejected(pkg):
    from sift_features_amd import _lib
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 256)()
    offs = (ctypes.c_size_t * 3)(0, 1, 2)
    po = (ctypes.c_size_t * 2)(0, 1)
    prm = _lib.RansacParams(2.0, 64, 0, 0)
    fake = ctypes.c_void_p(16)  # a non-null "context": the null argument must be seen before it is touched
    for name in PAIR_CALLS:
        # ctx, d_kps, offsets, n_segs, pairs, n_pairs, matches, pair_offsets, quality (may be null), params, models, inliers
        args = [fake, buf, offs, 2, buf, 1, buf, po, None, ctypes.byref(prm), buf, buf]
        for i in (0, 1, 2, 4, 6, 7, 9, 10, 11):
            a = list(args)
            a[i] = None
            assert getattr(L, name)(*a) == -1, (name, i)
            assert b"null" in L.sift_mi_last_error()
    for name in ONE_PAIR_CALLS:
        # ctx, query_kps, nq, train_kps, nt, matches, n_matches, quality (may be null), params, model, inliers
        args = [fake, buf, 1, buf, 1, buf, 1, None, ctypes.byref(prm), buf, buf]
        for i in (0, 1, 3, 5, 8, 9, 10):
            a = list(args)
            a[i] = None
            assert getattr(L, name)(*a) == -1, (name, i)
            assert b"null" in L.sift_mi_last_error()
    assert not any(buf)  # nothing written


def test_progressive_binding_keywords(pkg):
    for name in ("verify_pairs_device", "verify_frames", "verify_matches"):
        for fn in (getattr(pkg, name), getattr(pkg.Context, name)):
            sig = inspect.signature(fn).parameters
            assert sig["sampling"].default == "uniform" and sig["quality"].default is None, name
    with pytest.raises(ValueError):
        pkg.Context._verify_model("homography", "prosac")
    with pytest.raises(ValueError):
        pkg.Context._quality_args("uniform", [[1.0]], [0, 1])
