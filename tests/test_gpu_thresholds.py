"""The pyramid and detection kernels at their dispatch thresholds
(tests/kernel_shapes.py), against the CPU oracle.

Every other GPU test uses frame shapes well inside the regions the kernel
families are chosen by; an off-by-one at a threshold -- a strip window that
needs exactly one reflection, an octave exactly one strip wide, the tail
kernel with its LDS full to the last float of slack -- gives wrong pixels in
a few columns or rows of one octave of some frame sizes, and none of those
shapes would show it.  The table's shapes sit on the thresholds; each entry
names the predicate it straddles (Case.target, Case.why) and the launch count
that proves on the device that the case took the dispatch it was written for.

  * test_pyramid: precompute_images of seeded u8 noise under the case's path
    options; every G_s and D_s of every octave np.array_equal to the
    oracle's, and stats()["pyramid_launches"] equal to the table's literal
    (primary options) or the mirror's count (the other option sets) -- which
    also pins the Python mirror to the library;
  * test_batch_path: sift() of the case's pattern images with the fused
    blur-5 + scan pass forced on (pair and one-column forms), off, and by
    default; the batch path's planes bit for bit, the keypoints within
    test_gpu_parity.assert_parity, the octaves that ran fused
    (stats()["pyramid_scan_bytes"]) the ones the mirror names, and the exact
    descriptor mode byte-identical;
  * test_tail_workgroups: three different frames of a capacity shape in one
    chunk (one tail workgroup per frame), every frame's planes and keypoints.

No tolerance of its own: bit equality or assert_parity.
"""
import contextlib

import numpy as np
import pytest

import kernel_shapes as K
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

_memo = {}


def _oracle_sift(oracle, case, iname, img, profile):
    """The oracle's keypoints of a pattern image: computed once, shared, read-only."""
    key = (case.name, iname, profile)
    if key not in _memo:
        r = oracle.sift(img, profile=profile, internal=True)
        for a in r:
            a.setflags(write=False)
        _memo[key] = r
    return _memo[key]


@contextlib.contextmanager
def _device(pkg, what):
    """A library error (a HIP error among them) ends the session: nothing more
    is started on a device that may have faulted."""
    try:
        yield
    except pkg.SiftMiError as e:
        pytest.exit(f"library error in {what}: {e}", returncode=3)


def _processing(pkg, profile):
    return pkg.OpenCVProcessing if profile == K.OPENCV else pkg.ImageprocProcessing


@pytest.fixture(scope="module")
def ctxs(pkg):
    c = {p: pkg.Context(0, _processing(pkg, p)) for p in K.PROFILES}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def exact_ctxs(pkg):
    c = {p: pkg.Context(0, _processing(pkg, p)) for p in K.PROFILES}
    for x in c.values():
        x.set_exact_descriptors(True)
    yield c
    for x in c.values():
        x.close()


def _same(got, want, what):
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} values differ, planes {sorted(set(bad[:, 0].tolist()))}, "
                             f"rows {bad[:, 1].min()}..{bad[:, 1].max()}, columns {bad[:, 2].min()}..{bad[:, 2].max()}, "
                             f"first (plane, y, x) {bad[:5].tolist()}")


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("profile", K.PROFILES)
@pytest.mark.parametrize("case", K.CASES, ids=_ids(K.CASES))
def test_pyramid(pkg, ctxs, oracle, case, profile):
    """Planes bit for bit and the launch count of the dispatch the case is
    written for (Case.target / Case.why name the predicate)."""
    c = ctxs[profile]
    img = K.noise(case.w, case.h)
    opy = oracle.Pyramid(img, profile)
    want = [(opy.scale_space(o), opy.dog(o)) for o in range(opy.n_octaves)]
    for name in K.pyramid_option_sets(case):
        opts = K.OPTION_SETS[name]
        with _device(pkg, f"{case.name} {name}"), c.path_options(**opts):
            c.reset_stats()
            pre = c.precompute_images(img)
            launches = c.stats()["pyramid_launches"]
            assert pre.n_octaves == opy.n_octaves
            got = [(pre.dims(o), pre.scale_space_octave(o), pre.dog_octave(o)) for o in range(pre.n_octaves)]
        for o, ((go, do), (dims, g, d)) in enumerate(zip(want, got)):
            assert dims == opy.dims(o)
            _same(g, go, f"{case.name} {name} G octave {o} {dims}")
            _same(d, do, f"{case.name} {name} D octave {o} {dims}")
        o_tail, count = K.dispatch(case.w, case.h, profile, opts)
        if name == case.opts:
            assert (o_tail, count) == (case.tail[profile], case.launches[profile])
        assert launches == count, (name, launches, count, case.target)


DETECT = [c for c in K.CASES if c.detect]


@pytest.mark.parametrize("profile", K.PROFILES)
@pytest.mark.parametrize("case", DETECT, ids=_ids(DETECT))
def test_batch_path(pkg, ctxs, exact_ctxs, oracle, case, profile):
    """sift() on the blocks and squares patterns: the batch path's own planes,
    the keypoints, which octaves ran the fused pass, exact descriptors."""
    c = ctxs[profile]
    for iname, img in K.pattern_images(case).items():
        kp_o, desc_o, ext_o = _oracle_sift(oracle, case, iname, img, profile)
        opy = oracle.Pyramid(img, profile)
        sizes = K.octave_sizes(case.w, case.h)
        planes = [opy.scale_space(o) for o in range(opy.n_octaves)]
        for mode in K.detect_modes(case):
            opts = K.DETECT_MODES[mode]
            with _device(pkg, f"{case.name} {iname} {mode}"), c.path_options(**opts):
                c.reset_stats()
                res = c.sift(img)
                st = c.stats()
                got = [c.read_batch_scale_space(0, o, sizes[o]) for o in range(len(planes))]
            for o, (g, go) in enumerate(zip(got, planes)):
                _same(g, go, f"{case.name} {iname} {mode} G octave {o} {sizes[o]}")
            try:
                assert_parity(pkg, res, kp_o, desc_o, ext_o)
            except AssertionError as e:
                raise AssertionError(f"{case.name} {iname} {mode}: {e}") from e
            fused = K.fused_octaves(case.w, case.h, profile, opts)
            assert st["pyramid_scan_bytes"] == 20 * sum(sizes[o][0] * sizes[o][1] for o in fused), (iname, mode, fused)
        with _device(pkg, f"{case.name} {iname} exact"):
            res = exact_ctxs[profile].sift(img)
        assert len(res) == len(kp_o), (iname, "exact", len(res), len(kp_o))
        assert np.array_equal(res.descriptors, desc_o), (iname, "exact", int((res.descriptors != desc_o).sum()))


TAIL_BATCH = {K.OPENCV: ["capacity_48x50", "capacity_32x243", "capacity_473x16"],
              K.IMAGEPROC: ["capacity_25x100", "capacity_75x141", "capacity_327x31"]}


@pytest.mark.parametrize("profile,name", [(p, n) for p in K.PROFILES for n in TAIL_BATCH[p]])
def test_tail_workgroups(pkg, oracle, profile, name):
    """k_octave_tail at its LDS capacity with more than one workgroup: three
    different frames in one chunk, each frame's planes and keypoints."""
    case = K.BY_NAME[name]
    assert case.cap == profile
    ims = K.pattern_images(case)
    frames = np.stack([ims["blocks4"], K.noise(case.w, case.h), ims["squares12"]])
    sizes = K.octave_sizes(case.w, case.h)
    c = pkg.Context(0, _processing(pkg, profile))
    with _device(pkg, name):
        c.set_chunk(3)
        got = c.sift_batch(frames)
        planes = [[c.read_batch_scale_space(i, o, sizes[o]) for o in range(len(sizes))] for i in range(len(frames))]
    c.close()
    for i, f in enumerate(frames):
        opy = oracle.Pyramid(f, profile)
        assert opy.n_octaves == len(sizes)
        for o in range(opy.n_octaves):
            _same(planes[i][o], opy.scale_space(o), f"{name} frame {i} G octave {o}")
        kp_o, desc_o, ext_o = oracle.sift(f, profile=profile, internal=True)
        assert_parity(pkg, got[i], kp_o, desc_o, ext_o)
