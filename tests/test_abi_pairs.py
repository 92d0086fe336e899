"""C-ABI boundary of the frame-pair proposal that needs no GPU: both symbols
are exported and null arguments are rejected before the context is touched."""
import ctypes


def test_pair_symbols_exported(pkg):
    L = pkg.lib()
    for name in ("sift_mi_propose_pairs_device", "sift_mi_pair_counters"):
        assert hasattr(L, name), name


def test_pair_null_arguments_rejected(pkg):
    from sift_features_amd import _lib
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 256)()
    offs = (ctypes.c_size_t * 3)(0, 1, 2)
    n = ctypes.c_size_t(77)
    prm = _lib.PairParams(128, 0.8, 8, 0)
    fake = ctypes.c_void_p(16)  # a non-null "context": the null argument must be seen before it is touched
    # ctx, d_desc, d_kps, offsets, n_segs, params, scores (may be null), pairs, cap, n_pairs
    args = [fake, buf, buf, offs, 2, ctypes.byref(prm), None, buf, 1, ctypes.byref(n)]
    for i in (0, 1, 2, 3, 5, 7, 9):
        a = list(args)
        a[i] = None
        assert L.sift_mi_propose_pairs_device(*a) == -1, i
        assert b"null" in L.sift_mi_last_error()
    assert n.value == 77 and not any(buf)  # nothing written
    ms, tiles = ctypes.c_double(), ctypes.c_uint64()
    assert L.sift_mi_pair_counters(None, ctypes.byref(ms), ctypes.byref(tiles)) == -1
    assert L.sift_mi_pair_counters(fake, None, ctypes.byref(tiles)) == -1
    assert L.sift_mi_pair_counters(fake, ctypes.byref(ms), None) == -1


def test_pair_binding_mirrors(pkg):
    for name in ("propose_pairs_device", "propose_frames", "pair_counters"):
        assert callable(getattr(pkg, name)) and callable(getattr(pkg.Context, name)), name
