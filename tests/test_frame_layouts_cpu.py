"""CPU guards of tests/test_gpu_frame_layouts.py: from the oracle alone, the images of tests/frame_layouts.py would expose a kernel that
reads W * H * 4 where the frame stride belongs, or that rounds a frame's base address down to 16 bytes.  For every layout but the control
and every batch the GPU module binds: slicing at (lead, stride) gives the frames back, and every frame that such a reader would fetch from
another address comes out with another white balance, another histogram, another level-0 gray plane — and, per batch, other raw hits, and
per stream another first track() call.  Conditions on the inputs, asserted here so that a later edit of the generators cannot empty the GPU
tests."""
import numpy as np
import pytest

import cs_cases as cc
import frame_layouts as fl
from oracle import ht_oracle as ho

NOT_CONTROL = [name for name in fl.LAYOUTS if name != fl.CONTROL]
BATCHES = [("detect", w, h, 0) for w, h in fl.DETECT_SIZES] + [("camshift", w, h, k) for w, h in fl.CS_SIZES for k in range(fl.CS_STEPS + 1)]


def _batch(kind, w, h, k):
    return fl.detect_frames(w, h) if kind == "detect" else fl.cs_batch(w, h, k)


def _image(name, kind, w, h, k):
    lead, stride = fl.layout(name, w, h)
    frames = _batch(kind, w, h, k)
    return frames, lead, stride, fl.lay_out(frames, lead, stride, fl.layout_seed(name, w, h, k))


def test_layouts_are_what_their_names_promise():
    assert list(fl.LAYOUTS) == ["packed16", "lead4", "pad4", "lead12_rowpad", "double"] and fl.NFRAMES == 5
    for w, h in fl.DETECT_SIZES + fl.CS_SIZES:
        fb = w * h * 4
        assert {n: fl.layout(n, w, h) for n in fl.LAYOUTS} == {"packed16": (0, fb), "lead4": (4, fb), "pad4": (0, fb + 4),
                                                                "lead12_rowpad": (12, fb + 4 * (w + 5)), "double": (8, 2 * fb + 8)}
        for name in fl.LAYOUTS:
            lead, stride = fl.layout(name, w, h)
            assert lead % 4 == 0 and stride % 4 == 0 and stride >= fb  # what the C ABI accepts
            for how in fl.HOWS:
                assert (fl.affected(lead, stride, fl.NFRAMES, w, h, how) == []) == (name == fl.CONTROL and fb % 16 == 0 or
                                                                                   how == "packed" and stride == fb), (name, w, h, how)
    # the sizes: 16-byte groups and a packed frame of whole groups, resp. neither
    assert [(w % 4, w * h * 4 % 16) for w, h in fl.DETECT_SIZES] == [(0, 0), (1, 4)]
    assert [(w % 4, w * h * 4 % 16) for w, h in fl.CS_SIZES] == [(0, 0), (1, 4)]
    # pad4 on whole-group frames: frame f starts at 4 f mod 16 — every alignment class, and the wrap
    w, h = fl.DETECT_SIZES[0]
    lead, stride = fl.layout("pad4", w, h)
    assert [o % 16 for o in fl.true_offsets(lead, stride, fl.NFRAMES)] == [0, 4, 8, 12, 0]
    # every non-control layout puts at least one frame of every geometry on a base that is not 16-byte aligned
    for name in NOT_CONTROL:
        for w, h in fl.DETECT_SIZES + fl.CS_SIZES:
            assert any(o % 16 for o in fl.true_offsets(*fl.layout(name, w, h), fl.NFRAMES)), (name, w, h)


def test_gaps_are_seeded_noise_not_a_constant():
    w, h = fl.DETECT_SIZES[0]
    frames, lead, stride, img = _image("double", "detect", w, h, 0)
    gap = img[lead + w * h * 4 : lead + stride]
    assert len(gap) == w * h * 4 + 8 and len(np.unique(gap)) == 256 and abs(float(gap.mean()) - 127.5) < 2
    assert len(img) == lead + fl.NFRAMES * stride + fl.TAIL
    again = fl.lay_out(frames, lead, stride, fl.layout_seed("double", w, h, 0))
    assert np.array_equal(img, again) and not np.array_equal(img, fl.lay_out(frames, lead, stride, 1))


@pytest.mark.parametrize("batch", BATCHES, ids=lambda b: f"{b[0]}-{b[1]}x{b[2]}-{b[3]}")
@pytest.mark.parametrize("name", NOT_CONTROL)
def test_round_trip_and_visible_misreads(name, batch, cascade):
    kind, w, h, k = batch
    frames, lead, stride, img = _image(name, kind, w, h, k)
    n = len(frames)
    assert n == fl.NFRAMES
    assert np.array_equal(fl.read_at(img, fl.true_offsets(lead, stride, n), w, h), frames)  # round trip
    seen = 0
    for how in fl.HOWS:
        hit = fl.affected(lead, stride, n, w, h, how)
        wrong = fl.misread(img, lead, stride, n, w, h, how)
        for f in range(n):
            if f not in hit:
                assert np.array_equal(wrong[f], frames[f])
                continue
            seen += 1
            where = (name, kind, w, h, k, how, f)
            assert ho.whitebalance(wrong[f]) != ho.whitebalance(frames[f]), where
            assert not np.array_equal(cc.frame_histogram(wrong[f]), cc.frame_histogram(frames[f])), where
            for gray_in_r in (False, True):
                assert not np.array_equal(fl.gray_plane(wrong[f], gray_in_r), fl.gray_plane(frames[f], gray_in_r)), where + (gray_in_r,)
        if kind == "detect" and hit:
            differ = [f for f in hit if ho.detect_raw(wrong[f], cascade.blob).tobytes() != ho.detect_raw(frames[f], cascade.blob).tobytes()]
            assert differ, (name, w, h, how)
            assert any(len(ho.detect_raw(frames[f], cascade.blob)) > 0 for f in differ)  # ... and not only by hits that appear in noise
    assert seen > 0  # every non-control layout is misread by at least one of the two readers


@pytest.mark.parametrize("w,h", fl.CS_SIZES)
@pytest.mark.parametrize("name", NOT_CONTROL)
def test_misread_frames_move_every_affected_tracker(name, w, h):
    """the oracle's first track() of every stream on its misread frame differs from the truth in an integer field of the track object or
    the search window (the tracker initialised on the true frame: the track kernels alone are on trial), and so does the model
    histogram of initTracker on the misread frame, for the stream's own rect and for the short and tall rects of the init test"""
    seqs = fl.cs_streams(w, h)
    lead, stride = fl.layout(name, w, h)
    img0 = fl.lay_out(fl.cs_batch(w, h, 0), lead, stride, fl.layout_seed(name, w, h, 0))
    img1 = fl.lay_out(fl.cs_batch(w, h, 1), lead, stride, fl.layout_seed(name, w, h, 1))
    seen = 0
    for how in fl.HOWS:
        hit = fl.affected(lead, stride, fl.NFRAMES, w, h, how)
        wrong0 = fl.misread(img0, lead, stride, fl.NFRAMES, w, h, how)
        wrong1 = fl.misread(img1, lead, stride, fl.NFRAMES, w, h, how)
        for f in hit:
            seen += 1
            assert fl.oracle_first_track(seqs[f], wrong1[f]) != fl.oracle_first_track(seqs[f], seqs[f].frames[1]), (name, w, h, how, f)
            for rect in (seqs[f].rect, fl.cs_init_rects(w, h, "short")[f], fl.cs_init_rects(w, h, "tall")[f]):
                assert not np.array_equal(cc.model_histogram(wrong0[f], rect), cc.model_histogram(seqs[f].frames[0], rect)), (name, w, h, how, f, rect)
    assert seen > 0


@pytest.mark.parametrize("w,h", fl.CS_SIZES)
def test_camshift_streams_keep_their_object_and_the_init_rects_choose_both_kernels(w, h):
    seqs = fl.cs_streams(w, h)
    assert len(seqs) == fl.NFRAMES and len({s.name for s in seqs}) == fl.NFRAMES
    for s in seqs:
        assert (s.w, s.h, s.ncalls) == (w, h, fl.CS_STEPS)
        for k, (_b, sw, to) in enumerate(s.oracle_calls()):
            assert to["width"] > 0 and to["height"] > 0 and sw[2] > 0 and sw[3] > 0, (s.name, k, to, sw)
    short, tall = fl.cs_init_rects(w, h, "short"), fl.cs_init_rects(w, h, "tall")
    # ht_camshift_init_batch: the row-split kernel for n < 64 with (tallest rect + 15) / 16 >= 2
    assert (max(r[3] for r in short) + 15) // 16 == 1 and (max(r[3] for r in tall) + 15) // 16 >= 2
    for x, y, rw, rh in short + tall + [s.rect for s in seqs]:
        assert 0 <= x and x + rw <= w and 0 <= y and y + rh <= h and rw > 0 and rh > 0
    # the pairs name frames out of order, one of them twice, and never stream s on frame s
    assert [f for _s, f in fl.PAIRS].count(3) == 2 and all(s != f for s, f in fl.PAIRS) and [f for _s, f in fl.PAIRS] != sorted(f for _s, f in fl.PAIRS)
