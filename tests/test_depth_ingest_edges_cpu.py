"""The inputs of tests/test_depth_ingest_edges_gpu.py are worth their name, and the reference is stable on them (no device needed).

For EVERY input of every group: the host statement of tests/ingest_cases.py (the kernel's left-to-right arithmetic, elementwise NumPy)
and the oracle (whose transform is a BLAS ``np.dot``) set the same cells, or both raise IndexError.  That is a condition on the inputs --
a case that fails it gets another seed -- and it is what lets the GPU tests compare with the oracle alone.  The other assertions are the
coverage conditions: enough in-band texels, in-band texels at the top and the bottom of the image, a case most of whose rows cannot
reach the band, real island frames, exact band edges, exact rounding ties, cells exactly on the wrap / error boundaries."""
import numpy as np
import pytest

import ingest_cases as ic


def _assert_agrees(case):
    a, b = ic.statement_or_error(case), ic.oracle_or_error(case)
    if isinstance(a, str) or isinstance(b, str):
        assert isinstance(a, str) and isinstance(b, str), f"{case.name}: IndexError in only one of statement / oracle"
    else:
        assert np.array_equal(a, b), f"{case.name}: host statement and oracle differ in {(a != b).sum()} cells -- change the seed"


# ------------------------------------------------------------------------------------------------ group A
@pytest.fixture(scope="module")
def a_stats():
    """{(name, H): (in-band texels, island texels, image rows that hold in-band texels)}, computed once."""
    out = {}
    for name in ic.A_NAMES:
        for shape in ic.A_SHAPES:
            frame = ic.a_frame(name, shape)
            rows = np.flatnonzero(frame["clean"].statement(place=False).inband.any(axis=1))
            out[(name, shape[0])] = ic.a_frame_counts(frame) + (rows,)
    return out


@pytest.mark.parametrize("name", ic.A_NAMES)
def test_tilted_cases_meet_their_conditions(name, a_stats):
    """Per FRAME: statement == oracle in the three hole modes, nothing off the map, >= 200 in-band texels, >= 20 in-band valid texels
    inside the island frame's ring.  Only the 48x64 frames of the five cameras of ic.A_UPWARD are held to lower floors."""
    for shape in ic.A_SHAPES:
        frame = ic.a_frame(name, shape)
        for c in frame.values():
            assert c.depth.shape == shape
            _assert_agrees(c)
            assert not isinstance(ic.oracle_or_error(c), str), f"{c.name}: off the map"
        assert not (frame["clean"].depth == 0).any() and (frame["minus1"].depth == 0).any() and (frame["island"].depth == 0).any()
        n, isl, _ = a_stats[(name, shape[0])]
        excepted = name in ic.A_UPWARD and shape[0] == 48
        assert ic.a_minimum(name, shape[0]) == ((ic.A_UPWARD_MIN_INBAND, ic.A_UPWARD_MIN_ISLAND) if excepted else (200, 20))
        assert n >= ic.a_minimum(name, shape[0])[0] and isl >= ic.a_minimum(name, shape[0])[1], (name, shape, n, isl)
        tf = frame["clean"].tf
        assert 0.3 <= tf[2, 3] <= 1.5 and np.abs(tf[:2, 3]).max() <= 3.0


def test_tilted_set_covers_the_image_and_has_rows_to_skip(a_stats):
    top = [k for k, s in a_stats.items() if (s[2] < k[1] // 4).any()]
    bottom = [k for k, s in a_stats.items() if (s[2] >= k[1] - k[1] // 4).any()]
    sparse = [k for k, s in a_stats.items() if s[0] >= 200 and len(s[2]) < k[1] / 4]
    assert top and bottom, (top, bottom)
    assert sparse, "no frame leaves row_may_hit three quarters of the rows to skip"
    # the exception list is exactly the cameras pitched up by more than 1 rad, and only their 48x64 frames fall short
    pitch = {a[0]: a[1] for a in ic.A_ANGLES}
    assert sorted(ic.A_UPWARD) == sorted(n for n in ic.A_NAMES if pitch[n] < -1.0) and len(ic.A_UPWARD) == 5
    short = sorted(k for k, s in a_stats.items() if s[0] < 200 or s[1] < 20)
    assert short == sorted((n, 48) for n in ic.A_UPWARD), short
    kinds = [ic.a_kind(n) for n in ic.A_NAMES]
    assert abs(kinds.count("noise") - kinds.count("profile")) <= 1                     # half noise, half depth_frame
    t9 = [abs(ic.a_case(n)["clean"][0].tf[2, 1]) for n in ic.A_ROLLED]
    assert len(ic.A_ROLLED) >= 8 and min(t9) > 0.15           # the rolled cases: the column term of the filters is far from zero
    down = ic.a_case("pitch+90")["clean"][0].tf
    assert down[2, 0] == -1.0 and abs(down[2, 2]) < 1e-15
    side = ic.a_case("roll+90")["clean"][0].tf
    assert side[2, 1] == 1.0 and abs(side[2, 2]) < 1e-15


def test_pitched_trajectory_is_stable_and_rarely_a_tie():
    from oracle.ref_obstacle_map import RefObstacleMap
    from test_obstacle_map_gpu import _extreme_angle_tie

    ref = RefObstacleMap(size=ic.SIDE, **ic.OM_KW)
    skipped = 0
    for c in ic.a_trajectory():
        _assert_agrees(c)
        ref.update_map(c.depth.copy(), c.tf, c.lo, c.hi, c.fx, c.fx, 1.0, explore=False)
        skipped += bool(_extreme_angle_tie(ref, c.tf))
    assert skipped <= 2, skipped
    assert ref._map.sum() > 200


# ------------------------------------------------------------------------------------------------ group B
@pytest.mark.parametrize("shape", ic.B_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shape_cases_are_stable(shape):
    H, W = shape
    zero_past_31 = False
    for th in ic.B_THRESH:
        for cam in ic.b_cameras_of(H, W, th):
            for c in ic.b_frames(H, W, cam, th):
                _assert_agrees(c)
                assert not isinstance(ic.oracle_or_error(c), str), c.name
                assert (c.depth == 0).any(), c.name
                zero_past_31 |= bool((c.depth[:, W - 1] == 0).any())
    assert zero_past_31
    if H >= 15:      # the ring really is an island in "all" mode and is left alone in "some" mode
        c = [c for c in ic.b_frames(H, W, ic.b_cameras_of(H, W, "all")[0], "all") if c.name.endswith("combined")][0]
        assert (ic.filled_texels(c.depth, ic.B_THRESH["all"]) & (c.depth != 0)).any()
        assert not (ic.filled_texels(c.depth, ic.B_THRESH["some"]) & (c.depth != 0)).any()
        assert ic.filled_texels(c.depth, ic.B_THRESH["some"]).any()


@pytest.mark.parametrize("thresh", [ic.FILL_ALL, -1])
def test_batch_cases_are_stable(thresh):
    cases = ic.b_batch_cases(thresh)
    assert len(cases) == ic.BATCH_DISTINCT
    for c in cases:
        _assert_agrees(c)
        assert not isinstance(ic.oracle_or_error(c), str), c.name
    assert [ic.launch_bands(n, *ic.BATCH_SHAPE) for n in ic.BATCH_SIZES] == [3, 3, 1]


def test_colmax_frames_and_key_decoding():
    d = ic.colmax_frames(7, 36, 4)
    assert (d[0] > 0).all() and (d[1] < 0).all() and (d[2] > 0).any() and (d[2] < 0).any()
    assert np.isfinite(d).all() and (d != 0).all()
    # the key restated: monotone in the float, and decode_keys inverts it
    f = np.sort(d.reshape(-1))
    b = f.view(np.uint32)
    keys = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    assert (np.diff(keys.astype(np.int64)) >= 0).all()
    assert np.array_equal(ic.decode_keys(keys).view(np.uint32), b)


# ------------------------------------------------------------------------------------------------ group C
def test_band_edges_are_exact_and_inclusive():
    from oracle.ref_geometry import apply_tf, unproject
    from oracle.ref_obstacle_map import keep_height_band

    c = ic.c_band_cases(ic.C_BAND)["all"]
    z = c.depth * (c.hi - c.lo) + c.lo
    world = apply_tf(c.tf, unproject(z, z < c.hi, c.fx, c.fx))
    v = np.repeat(np.arange(40), 64)
    assert np.array_equal(world[:, 2], 1.0 - (v - 20) / 32.0)                        # Z = 1 - (v - 20)/32, exactly
    assert len(keep_height_band(world, *ic.C_BAND)) == 13 * 64                        # rows 24 .. 36, both edges included
    assert len(keep_height_band(world, *ic.C_BAND_INSIDE)) == 11 * 64                 # rows 25 .. 35
    for band, placed in ((ic.C_BAND, True), (ic.C_BAND_INSIDE, False)):
        cases = ic.c_band_cases(band)
        for name, case in cases.items():
            _assert_agrees(case)
        for v_edge in ic.C_EDGE_ROWS:
            plane = cases[f"row{v_edge}"].oracle()
            assert bool(plane.any()) == placed, (band, v_edge)
            if placed:
                assert np.array_equal(plane, cases["all"].oracle())


def test_rounding_ties_are_exact():
    pos = neg = 0
    for name in ic.C_TIE_TFS:
        c = ic.c_tie_case(name)
        _assert_agrees(c)
        p, n = ic.exact_ties(c)
        pos, neg = pos + (p if name in ("pos", "neg") else 0), neg + (n if name in ("pos", "neg") else 0)
        assert p + n == c.statement().inband.sum() == 40 * 64, name                   # every texel of the frame is a tie
        st = c.statement()
        arg = st.x20 if not name.startswith("col") else st.y20
        k = np.floor(arg).astype(np.int64)
        assert (k % 2 == 0).any() and (k % 2 == 1).any(), name                         # both parities: half-to-even goes both ways
    assert pos >= 16 and neg >= 16, (pos, neg)
    assert ic.exact_ties(ic.c_tie_case("pos"))[1] == 0 and ic.exact_ties(ic.c_tie_case("neg"))[0] == 0


def test_wrap_and_error_cells_sit_on_the_boundaries():
    S = ic.C_SIDE
    for axis in (0, 1):
        for target, t in ic.C_TARGETS.items():
            for path in ic.C_PATHS:
                c = ic.c_wrap_case(axis, target, path)
                _assert_agrees(c)
                got = ic.oracle_or_error(c)
                if target in ic.C_RAISES:
                    assert isinstance(got, str), c.name
                    continue
                cell = [10, 10]
                cell[axis] = t % S
                assert np.argwhere(got).tolist() == [cell], (c.name, np.argwhere(got).tolist())
                st = c.statement(place=False)
                assert set((st.rows if axis == 0 else st.cols).tolist()) == {t}
                zeros = c.depth == 0
                island = ic.filled_texels(c.depth, c.hole_thresh) & ~zeros
                assert bool(zeros.any()) == (path != "clean") and bool(island.any()) == (path == "island"), c.name
                if path == "island":
                    clean_inband = ic.c_wrap_case(axis, target, "clean").statement(place=False).inband
                    assert (island & clean_inband).sum() >= 5 and st.inband.sum() >= 20      # texels dropped, texels that survive
    _assert_agrees(ic.c_ordinary_case())
    assert ic.c_ordinary_case().oracle().sum() > 100


# ------------------------------------------------------------------------------------------------ groups D, E, F
@pytest.mark.parametrize("cam", list(ic.B_CAMERAS))
def test_depth_value_cases(cam):
    for mode in ic.D_MODES:
        c = ic.d_case(cam, mode)
        _assert_agrees(c)
        bits = c.depth.view(np.uint32)
        for value in ic.D_SPECIALS:
            assert (bits == value.view(np.uint32)).sum() >= 6, (c.name, value)
        # what the values mean to the reference: 1.0 is masked, the float below it is kept, a subnormal is no hole, both zeros are
        z = c.depth * np.float32(c.hi - c.lo) + np.float32(c.lo)
        assert not (z[c.depth == np.float32(1.0)] < c.hi).any()
        assert (z[bits == ic.D_SPECIALS[1].view(np.uint32)] < c.hi).all()
        assert (c.depth[bits == ic.D_SPECIALS[2].view(np.uint32)] != 0).all()
        assert (c.depth[bits == ic.D_SPECIALS[4].view(np.uint32)] == 0).all()
        assert c.statement().inband.sum() >= 200


def test_tilted_rig_has_undo_steps():
    steps = ic.e_steps()
    assert len(steps) == ic.E_STEPS and all(len(obs) == ic.E_SLOTS * len(ic.E_CAMERAS) for obs, _ in steps)
    for obs, _ in steps:
        for _, c in obs:
            _assert_agrees(c)
            assert not isinstance(ic.oracle_or_error(c), str), c.name
    assert ic.e_undo_steps(steps) >= 2


def test_refusal_cases():
    first, odd, last = ic.f_cases()
    assert odd.depth.shape == (48, 62) and first.depth.shape == last.depth.shape == (48, 64)
    for c in (first, last):
        _assert_agrees(c)
        assert c.oracle().sum() > 50
    assert (ic.filled_texels(last.depth, last.hole_thresh) & (last.depth != 0)).any()
