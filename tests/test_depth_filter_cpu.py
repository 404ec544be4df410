"""The depth filter's host statement (synthetic.depth_filter_numpy) and what DepthFilter / filter_depth refuse.  No GPU."""
import itertools

import numpy as np
import pytest

import vlfm_amd.synthetic as S
from vlfm_amd.synthetic import DepthFilter, depth_filter_numpy

f32 = np.float32
NAN = float("nan")
FRAME = np.array([[.5, 0, 0, 0, .9],
                  [0, 0, .2, 0, 0],
                  [.3, 0, 0, 0, NAN],
                  [0, 0, 0, 0, 0]], f32)


def loop_statement(frame, flt):
    """The rule, pixel by pixel: for every hole walk outwards in the four directions until a source or the frame's edge."""
    d = np.asarray(frame, f32)
    H, W = d.shape
    clip = f32(flt.clip_far_thresh)
    pos = lambda v: bool(v > 0)                                                     # noqa: E731
    src = lambda v: pos(v) and not (flt.clip_far_thresh > 0 and bool(v > clip))     # noqa: E731
    keep = pos if flt.recover_nonzero else src
    out, filled, left = d.copy(), 0, 0
    for r in range(H):
        for c in range(W):
            if keep(d[r, c]):
                continue
            cands = []
            for dr, dc in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                rr, cc, steps = r + dr, c + dc, 1
                while 0 <= rr < H and 0 <= cc < W and (flt.reach_px is None or steps <= flt.reach_px):
                    if src(d[rr, cc]):
                        cands.append(d[rr, cc])
                        break
                    rr, cc, steps = rr + dr, cc + dc, steps + 1
            if cands:
                out[r, c] = max(cands) if flt.fill == "far" else min(cands)
                filled += 1
            else:
                out[r, c] = f32(0.0) if flt.set_black_value is None else f32(flt.set_black_value)
                left += 1
    return out, filled, left


def test_the_hand_derived_frame():
    """FRAME, rows 0..3 and columns 0..4; sources are .5 (0,0), .9 (0,4), .2 (1,2), .3 (2,0); (2,4) is NaN: a hole, no source.

    DepthFilter() -- far, no limit.  Row 0: (0,1..3) see .5 to the left and .9 to the right; (0,2) also .2 below: max .9.
    Row 1: (1,0) sees .5 above, .3 below, .2 right: .5; (1,1) sees only .2 to its right (column 1 holds no source): .2;
    (1,3) only .2 to its left: .2; (1,4) .9 above, .2 left: .9.  Row 2: (2,1) sees .3 left: .3; (2,2) .3 left, .2 above: .3;
    (2,3) .3 left (column 3 is empty): .3; (2,4), the NaN, .3 left and .9 above: .9.  Row 3: (3,0) .3 above (the nearest, not
    .5): .3; (3,1) row 3 and column 1 hold no source: left; (3,2) .2 above: .2; (3,3) nothing: left; (3,4) .9 above: .9.
    16 holes, 2 left.

    reach_px=1 -- only the four neighbours.  (0,1) .5; (0,2) .2 (below); (0,3) .9; (1,0) max(.5, .3) = .5; (1,1) .2; (1,3) .2;
    (1,4) .9; (2,1) .3; (2,2) .2 (above); (3,0) .3: 10 filled.  (2,3), (2,4), (3,1), (3,2), (3,3), (3,4) have no source next to
    them: 6 left.

    reach_px=2, clip_far_thresh=.8 -- .9 is no source any more but, recovered, keeps its value.  (0,1) .5 at 1; (0,2) .5 at 2 and .2
    at 1: .5; (0,3) .5 is 3 away, .9 no source, column 3 empty: left; (1,0) .5; (1,1) .2; (1,3) .2; (1,4) .2 at 2; (2,1) .3;
    (2,2) max(.3 at 2, .2 at 1) = .3; (2,3) .3 is 3 away: left; (2,4) left; (3,0) .3; (3,1) left; (3,2) .2 at 2; (3,3), (3,4)
    left: 10 filled, 6 left.  With recover_nonzero=False (0,4) is a hole as well, with nothing within 2: 0, and 7 left."""
    cases = [
        (DepthFilter(), [[.5, .9, .9, .9, .9], [.5, .2, .2, .2, .9], [.3, .3, .3, .3, .9], [.3, 0, .2, 0, .9]], (14, 2)),
        (DepthFilter(reach_px=1), [[.5, .5, .2, .9, .9], [.5, .2, .2, .2, .9], [.3, .3, .2, 0, 0], [.3, 0, 0, 0, 0]], (10, 6)),
        (DepthFilter(reach_px=2, clip_far_thresh=.8),
         [[.5, .5, .5, 0, .9], [.5, .2, .2, .2, .2], [.3, .3, .3, 0, 0], [.3, 0, .2, 0, 0]], (10, 6)),
        (DepthFilter(reach_px=2, clip_far_thresh=.8, recover_nonzero=False),
         [[.5, .5, .5, 0, 0], [.5, .2, .2, .2, .2], [.3, .3, .3, 0, 0], [.3, 0, .2, 0, 0]], (10, 7)),
    ]
    for flt, want, counts in cases:
        out, filled, left = depth_filter_numpy(FRAME, flt)
        assert out.dtype == np.float32 and out.tobytes() == np.array(want, f32).tobytes(), flt
        assert (filled, left) == counts, flt
        assert loop_statement(FRAME, flt)[1:] == counts


def random_frame(rng, H, W, holes=0.3):
    d = rng.uniform(0.05, 1.0, (H, W)).astype(f32)
    kind = rng.uniform(size=(H, W))
    d[kind < holes] = 0.0
    d[kind < holes * 0.15] = NAN
    d[(kind >= holes * 0.15) & (kind < holes * 0.3)] = -0.5
    d[(kind >= holes * 0.3) & (kind < holes * 0.4)] = -0.0
    return d


@pytest.mark.parametrize("shape", [(18, 9), (7, 260)])
def test_the_statement_is_the_loop(shape):
    rng = np.random.Generator(np.random.PCG64(shape[1]))
    d = random_frame(rng, *shape)
    n = 0
    for fill, reach, clip, recover, black in itertools.product(("far", "near"), (1, 3, None), (0.0, 0.7), (True, False),
                                                                (None, -1.0)):
        flt = DepthFilter(fill, reach, clip, recover, black)
        got, want = depth_filter_numpy(d, flt), loop_statement(d, flt)
        assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:], flt
        n += got[2] > 0
    assert n > 0                                 # some case leaves holes


def test_a_frame_without_holes_is_its_input():
    d = np.array([[1.0, np.inf, np.finfo(f32).smallest_subnormal], [0.25, 3e38, 1e-30]], f32)
    for flt in (DepthFilter(), DepthFilter("near", 1, set_black_value=7.0)):
        out, filled, left = depth_filter_numpy(d, flt)
        assert out.tobytes() == d.tobytes() and (filled, left) == (0, 0)


def test_nan_negative_zero_and_negatives_are_holes():
    d = np.array([[.5, NAN, .5], [.5, -0.0, .5], [.5, -2.0, .5], [.5, -np.inf, .5]], f32)
    out, filled, left = depth_filter_numpy(d, DepthFilter())
    assert out.tobytes() == np.full((4, 3), .5, f32).tobytes() and (filled, left) == (4, 0)
    # ... and no sources: between them nothing is filled
    d = np.array([[NAN, 0.0, -1.0, -0.0]], f32)
    out, filled, left = depth_filter_numpy(d, DepthFilter())
    assert out.tobytes() == np.zeros((1, 4), f32).tobytes() and (filled, left) == (0, 4)


def test_a_pixel_equal_to_the_clip_threshold_is_a_source():
    t = f32(0.7)
    d = np.array([[t, 0.0, np.nextafter(t, f32(1))]], f32)
    out, filled, left = depth_filter_numpy(d, DepthFilter(clip_far_thresh=float(t)))
    assert out.tobytes() == np.array([[t, t, d[0, 2]]], f32).tobytes() and (filled, left) == (1, 0)
    out, filled, left = depth_filter_numpy(d[:, ::-1], DepthFilter(clip_far_thresh=float(t), recover_nonzero=False))
    assert out.tobytes() == np.array([[t, t, t]], f32).tobytes() and (filled, left) == (2, 0)
    # just below the threshold nothing is a source
    out, filled, left = depth_filter_numpy(d, DepthFilter(clip_far_thresh=float(np.nextafter(t, f32(0)))))
    assert out.tobytes() == d.tobytes() and (filled, left) == (0, 1)


def test_an_all_hole_frame_stays():
    d = np.zeros((5, 7), f32)
    out, filled, left = depth_filter_numpy(d, DepthFilter())
    assert out.tobytes() == d.tobytes() and (filled, left) == (0, 35)
    out, filled, left = depth_filter_numpy(d, DepthFilter(set_black_value=2.5))
    assert out.tobytes() == np.full((5, 7), 2.5, f32).tobytes() and (filled, left) == (0, 35)


@pytest.mark.parametrize("reach", [1, 3])
@pytest.mark.parametrize("vertical", [False, True])
def test_runs_of_reach_and_twice_reach_plus_one(reach, vertical):
    turn = (lambda a: np.ascontiguousarray(a.T)) if vertical else (lambda a: a)
    run = np.array([[.4] + [0.0] * reach + [.6]], f32)                      # the other axis offers nothing: one row
    out, filled, left = depth_filter_numpy(turn(run), DepthFilter(reach_px=reach))
    assert np.all(out > 0) and (filled, left) == (reach, 0)
    run = np.array([[.4] + [0.0] * (2 * reach + 1) + [.6]], f32)
    out, filled, left = depth_filter_numpy(turn(run), DepthFilter(reach_px=reach))
    want = np.array([[.4] * (reach + 1) + [0.0] + [.6] * (reach + 1)], f32)
    assert out.tobytes() == turn(want).tobytes() and (filled, left) == (2 * reach, 1)


def test_a_filled_value_never_feeds_a_fill():
    out, filled, left = depth_filter_numpy(np.array([[.5, 0, 0]], f32), DepthFilter(reach_px=1))
    assert out.tobytes() == np.array([[.5, .5, 0]], f32).tobytes() and (filled, left) == (1, 1)


def test_fill_modes_differ_only_in_the_choice():
    d = np.array([[.2, 0.0, .8]], f32)
    assert depth_filter_numpy(d, DepthFilter("far"))[0][0, 1] == f32(.8)
    assert depth_filter_numpy(d, DepthFilter("near"))[0][0, 1] == f32(.2)


@pytest.mark.parametrize("kw", [dict(fill="nearest"), dict(fill=0), dict(reach_px=0), dict(reach_px=65536), dict(reach_px=1.5),
                                dict(reach_px=True), dict(clip_far_thresh=-0.1), dict(clip_far_thresh=NAN),
                                dict(clip_far_thresh=float("inf")), dict(clip_far_thresh=1e39), dict(clip_far_thresh="1"),
                                dict(set_black_value=NAN), dict(set_black_value=float("inf")), dict(set_black_value=-1e39),
                                dict(set_black_value="0"), dict(recover_nonzero=1)])
def test_what_the_filter_refuses(kw):
    with pytest.raises(ValueError, match="DepthFilter"):
        DepthFilter(**kw)


def test_what_the_filter_accepts():
    DepthFilter(reach_px=np.int64(65535), clip_far_thresh=np.float32(3.0), set_black_value=-0.0, recover_nonzero=np.bool_(False))
    assert DepthFilter() == DepthFilter("far", None, 0.0, True, None) and S.DEPTH_FILTER_MAX_REACH == 65535
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        depth_filter_numpy(np.zeros((2, 2, 2), f32), DepthFilter())
    with pytest.raises(ValueError, match="DepthFilter"):
        depth_filter_numpy(np.zeros((2, 2), f32), None)


def test_filter_depth_refuses_blurring_and_bad_filters_without_a_device():
    from vlfm_amd.utils.depth_filter import filter_depth, filter_depth_batch

    d = np.zeros((4, 4), f32)
    for blur in ("gaussian", "closing", ""):
        with pytest.raises(NotImplementedError, match="blurring is not built"):
            filter_depth(d, blur_type=blur)
    with pytest.raises(ValueError, match="DepthFilter"):
        filter_depth(d, clip_far_thresh=-1.0)
    with pytest.raises(ValueError, match="DepthFilter"):
        filter_depth(d, reach_px=0)
    with pytest.raises(ValueError, match=r"\[H,W\]"):
        filter_depth(np.zeros((4, 4, 3), f32))
    import torch

    with pytest.raises(ValueError, match="HIP device"):
        filter_depth_batch(torch.zeros((1, 4, 4)))
    with pytest.raises(ValueError, match="DepthFilter"):
        filter_depth_batch(torch.zeros((1, 4, 4)), flt="far")
