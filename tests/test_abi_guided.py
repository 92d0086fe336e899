"""C-ABI boundary of guided matching that needs no GPU: the three symbols are
exported and a null context / null params are rejected before any device
call."""
import ctypes


def test_guided_symbols_exported(pkg):
    L = pkg.lib()
    for name in ("sift_mi_match_pairs_guided_device", "sift_mi_match_guided", "sift_mi_guided_counters"):
        assert hasattr(L, name), name


def test_guided_null_arguments_rejected(pkg):
    from sift_features_amd import _lib
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 256)()
    model = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    offs = (ctypes.c_size_t * 2)(0, 1)
    n = ctypes.c_size_t()
    prm = _lib.GuidedParams(3.0, 0.0, 0.0, 1)
    fake = ctypes.c_void_p(16)  # a non-null "context": the null params must be seen before it is touched
    # null context
    assert L.sift_mi_match_pairs_guided_device(None, buf, buf, offs, 1, buf, 1, 0, model, ctypes.byref(prm), buf, 1,
                                               offs) == -1
    assert b"null" in L.sift_mi_last_error()
    assert L.sift_mi_match_guided(None, buf, buf, 1, buf, buf, 1, 0, model, ctypes.byref(prm), buf, 1,
                                  ctypes.byref(n)) == -1
    tiles, culled = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.sift_mi_guided_counters(None, ctypes.byref(tiles), ctypes.byref(culled)) == -1
    # null params
    assert L.sift_mi_match_pairs_guided_device(fake, buf, buf, offs, 1, buf, 1, 0, model, None, buf, 1, offs) == -1
    assert L.sift_mi_match_guided(fake, buf, buf, 1, buf, buf, 1, 0, model, None, buf, 1, ctypes.byref(n)) == -1
    assert L.sift_mi_set_path_option(None, 16, 0) == -1
