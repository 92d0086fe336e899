"""C-ABI boundary of the spread-limited selection that needs no GPU: the four
symbols are exported and null arguments are rejected before the context is
touched, with nothing written."""
import ctypes

SYMBOLS = ("sift_mi_select_spread_device", "sift_mi_selected_results", "sift_mi_select_keypoints",
           "sift_mi_select_counters")


def test_select_symbols_exported(pkg):
    L = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name


def test_select_null_arguments_rejected(pkg):
    from sift_features_amd import _lib
    L = pkg.lib()
    buf = (ctypes.c_uint8 * 256)()
    offs = (ctypes.c_size_t * 3)(0, 1, 2)
    sel = (ctypes.c_size_t * 3)(7, 7, 7)
    n = ctypes.c_size_t(77)
    prm = _lib.SelectParams(100, 0.9)
    fake = ctypes.c_void_p(16)  # a non-null "context": the null argument must be seen before it is touched
    # ctx, d_kps, d_desc (may be null), offsets, n_segs, params, sel_offsets, rows, cap, radius2 (may be null)
    args = [fake, buf, None, offs, 2, ctypes.byref(prm), sel, buf, 2, None]
    for i in (0, 1, 3, 5, 6, 7):
        a = list(args)
        a[i] = None
        assert L.sift_mi_select_spread_device(*a) == -1, i
        assert b"null" in L.sift_mi_last_error()
    # ctx, kps, n, params, rows, cap, n_rows, radius2 (may be null)
    args = [fake, buf, 2, ctypes.byref(prm), buf, 2, ctypes.byref(n), None]
    for i in (0, 1, 3, 4, 6):
        a = list(args)
        a[i] = None
        assert L.sift_mi_select_keypoints(*a) == -1, i
        assert b"null" in L.sift_mi_last_error()
    kp, desc = ctypes.c_void_p(5), ctypes.c_void_p(5)
    args = [fake, ctypes.byref(kp), ctypes.byref(desc), ctypes.byref(n)]
    for i in range(4):
        a = list(args)
        a[i] = None
        assert L.sift_mi_selected_results(*a) == -1, i
    ms, tests = ctypes.c_double(), ctypes.c_uint64()
    assert L.sift_mi_select_counters(None, ctypes.byref(ms), ctypes.byref(tests)) == -1
    assert L.sift_mi_select_counters(fake, None, ctypes.byref(tests)) == -1
    assert L.sift_mi_select_counters(fake, ctypes.byref(ms), None) == -1
    # nothing written
    assert n.value == 77 and not any(buf) and list(sel) == [7, 7, 7] and kp.value == 5 and desc.value == 5


def test_select_binding_mirrors(pkg):
    for name in ("select_spread_device", "select_frames", "select_keypoints", "select_counters"):
        assert callable(getattr(pkg, name)) and callable(getattr(pkg.Context, name)), name
    sel = pkg.Selection([0, 2], [1, 3], None, 64, None)
    assert len(sel) == 2 and list(sel.segment_rows(0)) == [1, 3] and sel.d_desc_ptr is None
    from sift_features_amd import _lib
    assert ctypes.sizeof(_lib.SelectParams) == 8
