"""The host statement of the world's colours (synthetic.render_rgb_numpy): the rule pinned by a hand-computed frame, and its
relation to the depth and id planes.  No GPU."""
import numpy as np
import pytest

from vlfm_amd import synthetic as S
from world_object_cases import EDGES
from world_rgb_cases import ENV_OF, PALETTE, SIZES, SIZE_IDS, WORLD_OF, _args, colours, kinds, objects, reference, worlds


def _pack(r, g, b):
    return (r << 16) | (g << 8) | b


def test_palette_and_object_colours():
    assert S.WORLD_PALETTE.shape == (12,) and S.WORLD_PALETTE.dtype == np.int32 and S.WORLD_PALETTE[11] == 0
    assert ((S.WORLD_PALETTE >= 0) & (S.WORLD_PALETTE <= 0xFFFFFF)).all() and len(set(S.WORLD_PALETTE[:11].tolist())) == 11
    assert list(S.OBJECT_COLOURS) == list(S.OBJECT_SIZES) and len(set(S.OBJECT_COLOURS.values())) == len(S.OBJECT_SIZES)
    assert all(0 <= c <= 0xFFFFFF for c in S.OBJECT_COLOURS.values())


def test_hand_computed_frame():
    """One wall box, one object, H = W = 4, every byte worked out by hand.

    Camera at (0, 0.125) looking along +x, 0.5 m up, fx = 8, range [0, 8]: m = .25, .125, 0, -.125, dx = 1, dy = m (1e-12 in
    column 2).  The wall (4, -0.25)-(5, 10) is hit on its x-face at t_w = 4 in columns 0-2 -- q = y + 4 dy = 1.125, .625, .125,
    floor(2q) = 2, 1, 0: column 1 is an odd panel -- and missed by column 3 (q = -.375): void.  Depth .5, cue g = 64: x 192 >> 8.
      wall (200,160,80)            -> (150,120,60)                       columns 0 and 2
      odd panel: -= ch >> 3 -> (175,140,70) -> (131,105,52)              column 1
    floor_d of row rr = 1 is .5 * 8 / 1 = 4, NOT < t_w: the wall reaches the bottom row, where r_sk = ceil(.38 * 8 / 4) = 1:
      column 1: (175,140,70) >> 1 = (87,70,35) -> (65,52,26);  column 2: (100,80,40) -> (75,60,30)
    Column 3, rr = 1: floor at (4, .125 - .5 = -.375): floor(8) + floor(-.75) = 7, odd -> palette[9] = (90,60,33) -> (67,45,24);
    above it the void palette[10] = (10,20,30) with no cue.
    The object (1, .625)-(3, 2), z 0-.75, colour (255,100,9): column 0 enters through its y-face (ty0 = .5 / .25 = 2 > tx0 = 1) at
    t = 2, covers rr = ceil(-.25 * 8 / 2) = -1 .. floor(.5 * 8 / 2) = 2, depth .25, g = 32: (255,100,9) -= ch >> 2 ->
    (192,75,7) x 224 >> 8 -> (168,65,6).  Column 1 misses it (ty0 = 4 > tx1 = 3)."""
    k = S._mix32(0, 0, 31) % 8
    assert k == 2
    pal = np.zeros(12, np.int32)
    pal[k], pal[8], pal[9], pal[10], pal[11] = _pack(200, 160, 80), _pack(1, 2, 3), _pack(90, 60, 33), _pack(10, 20, 30), 0xFFFFFF
    depth, ids, rgb = S.render_rgb_numpy(0.0, 0.125, 1.0, 0.0, 0.5, 8.0, 0.0, 8.0, 4, 4, [(1.0, 0.625, 3.0, 2.0, 0.0, 0.75)],
                                         [_pack(255, 100, 9)], boxes=[(4.0, -0.25, 5.0, 10.0)], palette=pal)
    assert depth.dtype == np.float32 and ids.dtype == np.uint8 and rgb.dtype == np.uint8 and rgb.shape == (4, 4, 3)
    assert depth.tolist() == [[.5, .5, .5, 1.], [.25, .5, .5, 1.], [.25, .5, .5, 1.], [.25, .5, .5, .5]]
    assert ids.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0]]
    assert rgb.tolist() == [[[150, 120, 60], [131, 105, 52], [150, 120, 60], [10, 20, 30]],
                            [[168, 65, 6], [131, 105, 52], [150, 120, 60], [10, 20, 30]],
                            [[168, 65, 6], [131, 105, 52], [150, 120, 60], [10, 20, 30]],
                            [[168, 65, 6], [65, 52, 26], [75, 60, 30], [67, 45, 24]]]


@pytest.mark.parametrize("H,W", SIZES, ids=SIZE_IDS)
def test_depth_and_ids_are_the_object_renderer_s(H, W):
    depth, ids, _, rgb = reference(H, W)
    w = worlds()[0]
    for i in range(7):
        d, k = S.render_objects_numpy(*_args(i, H, W), boxes=w[WORLD_OF[i]])
        assert np.array_equal(depth[i].view(np.int32), d.view(np.int32)) and np.array_equal(ids[i], k)
    assert rgb.shape == (7, H, W, 3) and rgb.dtype == np.uint8


@pytest.mark.parametrize("H,W", SIZES, ids=SIZE_IDS)
def test_every_kind_of_pixel_is_in_the_reference(H, W):
    kind, skirting, odd, yface = kinds(H, W)
    assert all((kind == k).any() for k in range(4)) and skirting.any()
    wall, obj = kind == 1, kind == 3
    assert (wall & odd).any() and (wall & ~odd).any() and (wall & yface).any() and (wall & ~yface).any()
    assert (obj & yface).any() and (obj & ~yface).any()
    if (H, W) == (48, 64):
        assert [int((kind == k).sum()) for k in range(4)] == [4355, 8886, 5887, 2376] and int(skirting.sum()) == 242
    # the kinds are what the colours say: void pixels are the void colour, skirting halves the wall above it
    rgb = reference(H, W)[3]
    void = np.array([(PALETTE[10] >> 16) & 255, (PALETTE[10] >> 8) & 255, PALETTE[10] & 255])
    assert (rgb[kind == 0] == void).all()


def test_no_object_pixel_where_the_id_plane_has_none():
    """Black world, white objects: what is not black is an object of the id plane -- also beyond the range, where both clamp."""
    black = np.zeros(12, np.int32)
    scenes = [(p, b) for p, b in EDGES.values()] + [((0.0, 0.0, 0), objects()[1])]
    seen = 0
    for (x, y, k), boxes6 in scenes:
        c, s = S.HEADINGS[k]
        _, ids, rgb = S.render_rgb_numpy(x, y, c, s, S.CAMERA_HEIGHT, S.camera_intrinsics(64)[0], S.MIN_DEPTH, S.MAX_DEPTH, 48, 64,
                                         boxes6, [0xFFFFFF] * len(boxes6), palette=black)
        lit = rgb.any(axis=2)
        assert np.array_equal(lit, ids > 0)
        seen += int(lit.sum())
    assert seen > 1000
    (x, y, k), far = EDGES["beyond_range"]
    c, s = S.HEADINGS[k]
    assert not S.render_rgb_numpy(x, y, c, s, S.CAMERA_HEIGHT, S.camera_intrinsics(64)[0], S.MIN_DEPTH, S.MAX_DEPTH, 48, 64, far,
                                  [0xFFFFFF], palette=black)[2].any()


def test_wall_colour_follows_the_index_inside_the_world():
    """The same wall as box 0 and as box 1 of its world (behind a box no ray meets) wears palette[mix32(0)] / palette[mix32(1)]."""
    assert S._mix32(0, 0, 31) % 8 != S._mix32(1, 0, 31) % 8
    wall, unseen = (4.0, -10.0, 5.0, 10.0), (-9.0, -9.0, -8.0, -8.0)
    args = (0.0, 0.125, 1.0, 0.0, 0.5, 8.0, 0.0, 8.0, 4, 4, [], [])
    a = S.render_rgb_numpy(*args, boxes=[wall], palette=PALETTE)
    b = S.render_rgb_numpy(*args, boxes=[unseen, wall], palette=PALETTE)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])
    swapped = PALETTE.copy()
    i, j = S._mix32(0, 0, 31) % 8, S._mix32(1, 0, 31) % 8
    swapped[[i, j]] = PALETTE[[j, i]]
    assert np.array_equal(S.render_rgb_numpy(*args, boxes=[unseen, wall], palette=swapped)[2], a[2])


def test_colours_and_palette_are_checked():
    args = (0.0, 0.0, 1.0, 0.0, 0.88, 8.0, 0.5, 5.0, 4, 4)
    with pytest.raises(ValueError):
        S.render_rgb_numpy(*args, [(1.0, -0.2, 1.4, 0.2, 0.0, 1.0)], [])
    with pytest.raises(ValueError):
        S.render_rgb_numpy(*args, [], [], palette=np.zeros(11, np.int32))


def test_render_rgb_is_refused_before_the_device_is_touched():
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig

    with pytest.raises(ValueError, match="closed_loop"):
        BatchedEpisodes(2, use_blip2=False, select_frontiers=True, render_rgb=True)
    with pytest.raises(ValueError, match="rig"):
        BatchedEpisodes(2, use_blip2=False, select_frontiers=True, closed_loop=True, render_rgb=True, rig=CameraRig([Camera()]))


def test_case_colours_are_distinct():
    c = colours()
    assert c.shape == (3, 8) and len(set(c.reshape(-1).tolist())) == 24 and ((c > 0) & (c <= 0xFFFFFF)).all()
    assert len(ENV_OF) == len(WORLD_OF) == 7
