"""The JPEG step on the hand-built streams of tests/jpeg_streams.py:
sift_mi_decode_jpeg against the restatement (tests/golden/jpeg_decode.py with
zune-jpeg's arithmetic, then luma), bit for bit.  Exact equality only.

tests/test_jpeg_streams_cpu.py shows that the streams hold what the case
table says (against libjpeg and against the coefficients the writer was
given); here the kernels see the edges the PIL-encoded files of
tests/test_gpu_jpeg.py never reach: the DC-only and col0 shortcuts of
k_jpeg_idct, saturation in both directions, sample()'s clamps next to block
padding that differs from the picture, every clamp of k_jpeg_luma.
"""
import sys
import threading

import numpy as np
import pytest
from conftest import GOLDEN

import jpeg_streams as J

pytestmark = pytest.mark.gpu
sys.path.insert(0, GOLDEN)
ZUNE = dict(idct="zune", upsample="twopass", color="zune", edge="pad")
EINVAL, EUNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """name -> the restatement's luma, decoded once per case (NotImplementedError where it has no upsampler)."""
    import jpeg_decode
    d = tmp_path_factory.mktemp("streams")
    _REF = {}

    def get(name):
        if name not in _REF:
            s = J.spec(name)  # (the restatement's parse has no fill-byte loop: it reads the stream without them)
            data = J.write(J.without_fill(s))[0] if s.fill else J.stream(name)[0]
            f = d / (name + ".jpg")
            f.write_bytes(data)
            try:
                out = jpeg_decode.decode(str(f), **ZUNE)
                out = out if out.ndim == 2 else jpeg_decode.luma(out)
                out.setflags(write=False)  # shared among the tests
            except NotImplementedError as e:
                out = e
            _REF[name] = out
        return _REF[name]
    return get


@pytest.mark.parametrize("name", [n for n in J.CASES if n not in J.SAMPLING_CASES])
def test_stream_decodes_to_the_restatement(ctx, reference, name):
    s = J.spec(name)
    got = ctx.decode_jpeg(J.stream(name)[0])
    assert got.shape == (s.h, s.w)
    assert np.array_equal(got, reference(name))


def test_colour_sweep_closed_form(ctx):
    """Every block of the colour frame is flat, so the luma is the closed form of jpeg.hip's file comment on
    the known values: no entropy decoder of the tests' own in between."""
    got = ctx.decode_jpeg(J.stream("colour")[0])
    want = J.colour_luma(*J.colour_values()).astype(np.uint8)
    assert np.array_equal(got, np.kron(want, np.ones((8, 8), np.uint8)))


def test_sampling_combinations(pkg, ctx, reference):
    """All 64 combinations: the library equals the restatement or refuses with EUNSUPPORTED, and refuses
    where the restatement itself raises."""
    decoded, refused = [], []
    for name in J.SAMPLING_CASES:
        ref = reference(name)
        try:
            got = ctx.decode_jpeg(J.stream(name)[0])
        except pkg.SiftMiError as e:
            assert e.code == EUNSUPPORTED, (name, e)
            refused.append(name)
            continue
        assert not isinstance(ref, Exception), name  # the restatement raises: the library must refuse
        assert np.array_equal(got, ref), name
        decoded.append(name)
    print("decoded %d: %s\nrefused %d: %s" % (len(decoded), " ".join(decoded), len(refused), " ".join(refused)))
    assert {"samp_1x1_1x1_1x1", "samp_2x1_1x1_1x1", "samp_2x2_1x1_1x1"} <= set(decoded)
    assert len(decoded) + len(refused) == 64
    assert set(decoded) == {n for n, hv in J.SAMPLING_CASES.items() if J.sampling_supported(hv)}


@pytest.mark.parametrize("name", ["size_420_17x17", "size_422_31x9", "size_444_33x1", "size_gray_1x33",
                                  "restart_420_5"])
def test_decode_to_device_leaves_the_padding(ctx, reference, name):
    import torch
    s = J.spec(name)
    t = torch.full((s.h + 2, s.w + 5), 77, dtype=torch.uint8, device="cuda")
    ctx.decode_jpeg_device(J.stream(name)[0], t.data_ptr(), t.stride(0))
    torch.cuda.synchronize()
    out = t.cpu().numpy()
    assert np.array_equal(out[:s.h, :s.w], reference(name))
    assert np.all(out[:, s.w:] == 77) and np.all(out[s.h:] == 77)  # stride padding and the rows below: untouched


def _batch(ctx, datas, w, h, threads):
    import torch
    t = torch.full((len(datas), h, w + 8), 77, dtype=torch.uint8, device="cuda")
    ctx.decode_jpeg_batch_device(datas, t.data_ptr(), t.stride(0), t.stride(1), threads=threads)
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.mark.parametrize("threads", [1, 4, 64])
def test_batch_of_different_tables(ctx, reference, threads):
    """37 frames of one size, cycling through six sets of Huffman tables, quantisation tables and restart
    intervals: each equals its single-frame decode (and the restatement)."""
    names = [J.BATCH[i % len(J.BATCH)] for i in range(37)]
    s = J.spec(names[0])
    out = _batch(ctx, [J.stream(n)[0] for n in names], s.w, s.h, threads)
    single = {n: ctx.decode_jpeg(J.stream(n)[0]) for n in J.BATCH}
    for i, n in enumerate(names):
        assert np.array_equal(out[i, :, :s.w], single[n]), (i, n)
        assert np.array_equal(single[n], reference(n)), n
    assert np.all(out[:, :, s.w:] == 77)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("at", [0, 20, 36])
def test_batch_error_return(pkg, ctx, reference, at, threads):
    """One frame of 37 has a scan that runs past coefficient 63: the call returns that error (it does not hang:
    the call runs on a thread that is given 60 s), and the next batch on the same context is right.  An error
    return and nothing else: the failing chunk's kernels are never launched."""
    names = [J.BATCH[i % len(J.BATCH)] for i in range(37)]
    s = J.spec(names[0])
    datas = [J.stream(n)[0] for n in names]
    bad = list(datas)
    bad[at] = J.overrun_stream()
    assert pkg.jpeg_dims(bad[at]) == (s.w, s.h)
    result = []

    def call():
        try:
            _batch(ctx, bad, s.w, s.h, threads)
            result.append(None)
        except Exception as e:  # noqa: BLE001
            result.append(e)
    th = threading.Thread(target=call, daemon=True)
    th.start()
    th.join(60)
    assert not th.is_alive(), "sift_mi_decode_jpeg_batch did not return"
    err = result[0]
    assert isinstance(err, pkg.SiftMiError) and err.code == EINVAL, err
    assert "coefficient index out of range" in str(err)
    out = _batch(ctx, datas, s.w, s.h, threads)
    for i, n in enumerate(names):
        assert np.array_equal(out[i, :, :s.w], reference(n)), (i, n)


def test_oversized_frame_refused(pkg, ctx):
    """A 16385 x 1 header: the decode entry points refuse before sizing anything; jpeg_dims reports it."""
    s = J.gray_spec(8, 8, J.grid([J.zz_block(1)], 1))
    data, st = J.write(s)
    i = data.index(b"\xff\xc0") + 5
    data = data[:i] + (1).to_bytes(2, "big") + (16385).to_bytes(2, "big") + data[i + 4:st.scan_start]
    assert pkg.jpeg_dims(data) == (16385, 1)
    with pytest.raises(pkg.SiftMiError) as e:
        ctx.decode_jpeg(data)
    assert e.value.code == EINVAL and "16384" in str(e.value)
