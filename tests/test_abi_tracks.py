"""C-ABI boundary of the feature tracks that needs no GPU: both symbols are
exported and a null context / null params are rejected before anything is
touched."""
import ctypes


def test_track_symbols_exported(pkg):
    L = pkg.lib()
    for name in ("sift_mi_build_tracks_device", "sift_mi_track_counters"):
        assert hasattr(L, name), name


def test_track_null_arguments_rejected(pkg):
    from sift_features_amd import _lib
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 256)()
    offs = (ctypes.c_size_t * 2)(0, 1)
    n = ctypes.c_uint32(77)
    prm = _lib.TrackParams(2, 0)
    fake = ctypes.c_void_p(16)  # a non-null "context": the null params must be seen before it is touched
    assert L.sift_mi_build_tracks_device(None, buf, offs, 1, buf, 1, buf, offs, None, ctypes.byref(prm), buf,
                                         ctypes.byref(n), buf, buf, buf) == -1
    assert b"null" in L.sift_mi_last_error()
    assert L.sift_mi_build_tracks_device(fake, buf, offs, 1, buf, 1, buf, offs, None, None, buf, ctypes.byref(n), buf,
                                         buf, buf) == -1
    assert b"null" in L.sift_mi_last_error()
    # every other pointer but keep
    args = [fake, buf, offs, 1, buf, 1, buf, offs, None, ctypes.byref(prm), buf, ctypes.byref(n), buf, buf, buf]
    for i in (1, 2, 4, 6, 7, 10, 11, 12, 13, 14):
        a = list(args)
        a[i] = None
        assert L.sift_mi_build_tracks_device(*a) == -1, i
    assert n.value == 77 and not any(buf)  # nothing written
    ms, edges = ctypes.c_double(), ctypes.c_uint64()
    assert L.sift_mi_track_counters(None, ctypes.byref(ms), ctypes.byref(edges)) == -1
    assert L.sift_mi_track_counters(fake, None, ctypes.byref(edges)) == -1
    assert L.sift_mi_track_counters(fake, ctypes.byref(ms), None) == -1
