"""-m gpu: csrc/depth_ingest.hip + csrc/depth_holes.hip and their callers in vlfm_amd/mapping/obstacle_map.py where the rest of the
suite never takes them: tilted cameras (the f32 pre-filters' column and pitch terms), image shapes that are no multiple of 32 / 128
columns or 16 rows, texels exactly on the band edges, on rounding ties and on the wrap / IndexError boundaries of the map, special
depth values, a tilted camera rig, and a refused frame.  Reference: the oracle (oracle/ref_obstacle_map.py, oracle/ref_geometry.py),
bit for bit, no tolerance: the obstacle and the navigable plane after EVERY frame, the filled-texel plane of fill_small_holes, the
column maxima.  tests/test_depth_ingest_edges_cpu.py proves on the host that every input used here is one on which the oracle does
not depend on its BLAS (tests/ingest_cases.py states why and how).  Every case prints a line (``-s`` shows them:
profiles/depth_ingest_edges.txt)."""
import functools

import numpy as np
import pytest

import ingest_cases as ic
from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

pytestmark = pytest.mark.gpu
FOV = camera_intrinsics(640)[2]


def _pair(gpu_device, case):
    from oracle.ref_obstacle_map import RefObstacleMap
    from vlfm_amd.mapping import ObstacleMap

    kw = dict(case.om_kw, hole_area_thresh=case.hole_thresh, size=case.size)
    return ObstacleMap(device=gpu_device, **kw), RefObstacleMap(**kw)


def _update(m, case):
    m.update_map(case.depth.copy(), case.tf, case.lo, case.hi, case.fx, case.fx, FOV, explore=False)


def _filled_words(ours):
    return ours._batch._filled_bits[0].cpu().numpy().view(np.uint32)


def _same_planes(ours, ref, where):
    got, want = ours._map, ref._map.astype(bool)
    assert np.array_equal(got, want), f"{where}: obstacle plane differs in {(got != want).sum()} cells: {np.argwhere(got != want)[:6].tolist()}"
    got, want = ours._navigable_map != 0, np.asarray(ref._navigable_map) != 0
    assert np.array_equal(got, want), f"{where}: navigable plane differs in {(got != want).sum()} cells"


def _same_filled(ours, case):
    """The filled-texel plane against fill_small_holes (read as test_fill_small_holes_parity reads it), and no bit at or beyond
    column W."""
    H, W = case.depth.shape
    words = _filled_words(ours)
    assert words.shape == (H, (W + 31) // 32)
    got = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(H, -1).astype(bool)
    assert not got[:, W:].any(), f"{case.name}: filled bits at or beyond column {W}"
    want = ic.filled_texels(case.depth, case.hole_thresh)
    assert np.array_equal(got[:, :W], want), f"{case.name}: filled plane differs in {(got[:, :W] != want).sum()} texels"


def _report(group, case, ref, ours=None, bands=None):
    line = f"edges {group} {case.name}: inband={int(case.statement(place=False).inband.sum())} cells={int(ref._map.sum())}"
    if (case.depth == 0).any():
        if case.hole_thresh != -1 and ours is not None:
            c = ours._batch._hole_counts[0].cpu().numpy()
            line += f" contours={int(c[0])} filled={int(c[1])} island={bool(c[3] & 2)}"
        else:
            line += " zeros->1.0"
    if bands is not None:
        line += f" bands={bands}"
    print(line)


def _step(group, ours, ref, case, bands=None):
    """One frame into both maps; planes (and the filled plane, where fill_small_holes ran on a frame with zeros) compared."""
    _update(ours, case)
    _update(ref, case)
    _report(group, case, ref, ours, bands)
    _same_planes(ours, ref, case.name)
    if case.hole_thresh != -1 and (case.depth == 0).any():
        _same_filled(ours, case)
        c = ours._batch._hole_counts[0].cpu().numpy()
        island = bool((ic.filled_texels(case.depth, case.hole_thresh) & (case.depth != 0)).any())
        assert c[2] == 0 and bool(c[3] & 2) == island, (case.name, c.tolist(), island)     # the island path ran exactly when it should


# ------------------------------------------------------------------------------------------------ group A: tilted cameras
@pytest.mark.parametrize("name", ic.A_NAMES)
def test_tilted_cameras(gpu_device, name):
    """One camera (fixed pitch, fixed roll or a random combination), a 48x64 and a 240x424 frame, three hole modes: no zero texel;
    hole_area_thresh = -1 with zero rectangles; the default threshold with rectangles and a ring around the in-band centroid (an
    island frame: journal undo, second placement).  With a level camera t8 = t9 = 0 and the column term gx of candidate_fast, the
    column hull of row_may_hit and most of the margin vanish: here they decide which texels reach the exact f64 placement."""
    cases = ic.a_case(name)
    for mode in ic.A_MODES:
        ours, ref = _pair(gpu_device, cases[mode][0])
        for case in cases[mode]:
            _step("A", ours, ref, case)


def test_pitched_trajectory_with_exploration(gpu_device):
    """A camera pitched 30 degrees down walks 24 steps; obstacles first, then the reveal as its own call unless the pose is an
    extreme-angle tie of the reference (test_obstacle_map_gpu._extreme_angle_tie: at most 2 steps, the CPU test asserts it for the
    seed); every plane and the frontiers after every step."""
    from test_obstacle_map_gpu import _extreme_angle_tie, _same

    steps = ic.a_trajectory()
    ours, ref = _pair(gpu_device, steps[0])
    skipped = 0
    for k, case in enumerate(steps):
        _update(ours, case)
        _update(ref, case)
        _same_planes(ours, ref, f"trajectory step {k}")
        if _extreme_angle_tie(ref, case.tf):
            skipped += 1
            continue
        for m in (ours, ref):
            m.update_map(None, case.tf, case.lo, case.hi, case.fx, case.fx, FOV, update_obstacles=False)
        _same(ours, ref, k)
    print(f"edges A trajectory: steps={len(steps)} skipped={skipped} cells={int(ref._map.sum())} explored={int(ref.explored_area.sum())}")
    assert skipped <= 2 and ref._map.sum() > 200 and ref.explored_area.sum() > 500


# ------------------------------------------------------------------------------------------------ group B: image shapes
@pytest.mark.parametrize("thresh_name", list(ic.B_THRESH))
@pytest.mark.parametrize("shape", ic.B_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_shapes(gpu_device, shape, thresh_name):
    """Widths that end in a partial 32-bit word of the hole / filled planes and in a partial 128-column workgroup, heights that end
    in a partial 16-row group, odd heights, fewer row groups than the unrolled band loop covers; zero blobs on the right border, across
    the 31|32 seam, in the last column, in the last row, a ring with an island; a threshold that fills everything / some / -1."""
    H, W = shape
    bands = ic.launch_bands(1, H, W)
    for cam in ic.b_cameras_of(H, W, thresh_name):
        frames = ic.b_frames(H, W, cam, thresh_name)
        ours, ref = _pair(gpu_device, frames[0])
        for case in frames:
            _step("B", ours, ref, case, bands)


@functools.lru_cache(maxsize=None)
def _batch_oracle(thresh):
    """(obstacle, navigable) planes of the 50 distinct batch cases, each in an empty map: computed once per threshold."""
    from oracle.ref_obstacle_map import RefObstacleMap

    out = []
    for case in ic.b_batch_cases(thresh):
        ref = RefObstacleMap(hole_area_thresh=thresh, size=ic.SIDE, **ic.OM_KW)
        _update(ref, case)
        out.append((ref._map.astype(bool), np.asarray(ref._navigable_map) != 0))
    return out


@pytest.mark.parametrize("thresh", [ic.FILL_ALL, -1])
@pytest.mark.parametrize("n", ic.BATCH_SIZES)
def test_batch_sizes_and_row_bands(gpu_device, n, thresh):
    """33x260 through ObstacleMapBatch, one slot per observation: n = 1 and 5 launch three interleaved row bands, n = 700 one band
    (every column maximum has a single owner).  The same pass also reduces the column maxima (the harness's combined form)."""
    import torch

    from vlfm_amd.mapping import ObstacleMapBatch

    H, W = ic.BATCH_SHAPE
    assert [ic.launch_bands(m, H, W) for m in ic.BATCH_SIZES] == [3, 3, 1]
    cases, want = ic.b_batch_cases(thresh), _batch_oracle(thresh)
    pick = [i % ic.BATCH_DISTINCT for i in range(n)]
    depth = np.stack([cases[j].depth for j in pick])
    tfs = np.stack([cases[j].tf for j in pick])
    fx = cases[0].fx
    batch = ObstacleMapBatch(n, hole_area_thresh=thresh, size=ic.SIDE, device=gpu_device, **ic.OM_KW)
    keys = batch.ingest(torch.from_numpy(depth).to(gpu_device), tfs, MIN_DEPTH, MAX_DEPTH, fx, fx, want_colmax=True)
    batch.check_status()
    batch.update_after_ingest(tfs, MAX_DEPTH, FOV, explore=False)
    obst = batch._unpack(batch.obstacle_bits).cpu().numpy().astype(bool)
    nav = batch._unpack(batch.navigable_bits).cpu().numpy().astype(bool)
    for i, j in enumerate(pick):
        assert np.array_equal(obst[i], want[j][0]), f"slot {i} ({cases[j].name}): {(obst[i] != want[j][0]).sum()} obstacle cells differ"
        assert np.array_equal(nav[i], want[j][1]), f"slot {i} ({cases[j].name}): navigable plane differs"
    got = ic.decode_keys(keys[:n].cpu().numpy())
    assert np.array_equal(got.view(np.uint32), depth.max(axis=1).view(np.uint32)), "column maxima differ"
    counts = batch._hole_counts[:n].cpu().numpy() if thresh != -1 else np.zeros((n, 4), np.int64)
    print(f"edges B batch-33x260-n{n}-thresh{thresh}: bands={ic.launch_bands(n, H, W)} inband="
          f"{sum(int(cases[j].statement(place=False).inband.sum()) for j in pick)} cells={int(obst.sum())} contours={int(counts[:, 0].sum())} "
          f"filled={int(counts[:, 1].sum())} island_frames={int((counts[:, 3] & 2).astype(bool).sum())}")


def _column_maxima(gpu_device, depth):
    import torch

    from vlfm_amd.mapping import ObstacleMapBatch

    n, H, W = depth.shape
    batch = ObstacleMapBatch(n, size=ic.SIDE, device=gpu_device, **ic.OM_KW)
    tfs = np.tile(np.eye(4), (n, 1, 1))
    fx = camera_intrinsics(W)[0]
    keys = batch.ingest(torch.from_numpy(depth).to(gpu_device), tfs, MIN_DEPTH, MAX_DEPTH, fx, fx, want_colmax=True,
                        update_obstacles=False)
    got = ic.decode_keys(keys[:n].cpu().numpy())
    want = np.max(depth, axis=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f"{n}x{H}x{W}: {(got.view(np.uint32) != want.view(np.uint32)).sum()} column maxima differ"
    assert not batch.obstacle_bits.any()
    print(f"edges B colmax-{H}x{W}-n{n}: bands={ic.launch_bands(n, H, W)} columns={n * W} negative_maxima={int((want < 0).sum())}")


@pytest.mark.parametrize("shape", ic.B_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_column_maxima_of_every_shape(gpu_device, shape):
    """The streaming-only pass: keys decoded by the inverse of the order-preserving key equal np.max(depth, axis=0) bit for bit, for a
    positive frame, an entirely negative one, mixed signs and a wide dynamic range."""
    _column_maxima(gpu_device, ic.colmax_frames(*shape, 4))


@pytest.mark.parametrize("n", ic.BATCH_SIZES)
def test_column_maxima_of_every_batch_size(gpu_device, n):
    frames = ic.colmax_frames(*ic.BATCH_SHAPE, min(n, 8))
    _column_maxima(gpu_device, np.ascontiguousarray(frames[np.arange(n) % len(frames)]))


# ------------------------------------------------------------------------------------------------ group C: exact boundaries
@pytest.mark.parametrize("inside", [False, True], ids=["band", "band_shrunk_by_an_ulp"])
def test_height_band_edges(gpu_device, inside):
    """Z = 1 - (v - 20)/32 exactly: rows 24 and 36 lie ON the band (0.5, 0.875) and are placed (the widened f32 band lets them
    through, the f64 test is inclusive); with the band shrunk by one ulp on each side they are not."""
    for name, case in ic.c_band_cases(ic.C_BAND_INSIDE if inside else ic.C_BAND).items():
        ours, ref = _pair(gpu_device, case)
        _step("C", ours, ref, case)
        if name != "all":
            assert bool(ours._map.any()) == (not inside), name
        else:
            assert ours._map.sum() == 40


@pytest.mark.parametrize("name", list(ic.C_TIE_TFS))
def test_rounding_ties(gpu_device, name):
    """Every texel's row (or column) argument of rint is exactly k + 0.5, k of both parities, positive and negative."""
    case = ic.c_tie_case(name)
    ours, ref = _pair(gpu_device, case)
    _step("C", ours, ref, case)


@pytest.mark.parametrize("path", ic.C_PATHS)
@pytest.mark.parametrize("axis", [0, 1], ids=["row", "col"])
def test_wrap_and_index_error(gpu_device, axis, path):
    """One cell exactly at -1, -S (wrap like NumPy's negative indices), S - 1 (the last cell), -S - 1 and S (IndexError), in a
    frame without zeros (the speculative pass's note is promoted), with a solid zero block (promoted by the fill kernel) and as an
    island frame (the hole scatter places the survivors and raises).  After the error: reset(), and an ordinary frame is right."""
    for target in ic.C_TARGETS:
        case = ic.c_wrap_case(axis, target, path)
        ours, ref = _pair(gpu_device, case)
        if target not in ic.C_RAISES:
            _step("C", ours, ref, case)
            assert ours._map.sum() == 1
            continue
        with pytest.raises(IndexError):
            _update(ref, case)
        with pytest.raises(IndexError):
            _update(ours, case)
        print(f"edges C {case.name}: IndexError in both")
        ours.reset()
        ref.reset()
        _step("C", ours, ref, ic.c_ordinary_case())


# ------------------------------------------------------------------------------------------------ group D: depth values
@pytest.mark.parametrize("mode", ic.D_MODES)
@pytest.mark.parametrize("cam", list(ic.B_CAMERAS))
def test_special_depth_values(gpu_device, cam, mode):
    """1.0 is masked (z < max_depth is false), the float below 1.0 is kept, 2^-149 is no hole, +0.0 and -0.0 both are."""
    case = ic.d_case(cam, mode)
    ours, ref = _pair(gpu_device, case)
    _step("D", ours, ref, case)


# ------------------------------------------------------------------------------------------------ group E: a tilted rig
def test_tilted_rig(gpu_device):
    """ingest_cameras: 2 slots x 3 cameras (level, pitched 30 degrees down, rolled 90 degrees), 6 steps of clean / rectangle / island
    frames, against the oracle updated camera by camera in call order; planes after every step.  In at least 2 steps an island
    frame's undo would take a bit a sibling placed (the CPU test asserts it): the per-slot "undone" path."""
    from oracle.ref_obstacle_map import RefObstacleMap
    from vlfm_amd.mapping import ObstacleMapBatch

    steps = ic.e_steps()
    om = ObstacleMapBatch(ic.E_SLOTS, hole_area_thresh=ic.FILL_ALL, size=ic.SIDE, device=gpu_device, **ic.OM_KW)
    refs = [RefObstacleMap(hole_area_thresh=ic.FILL_ALL, size=ic.SIDE, **ic.OM_KW) for _ in range(ic.E_SLOTS)]
    undone_steps = 0
    for k, (obs, reveal) in enumerate(steps):
        slot = np.array([s for s, _ in obs])
        fx = obs[0][1].fx
        om.ingest_cameras(np.stack([c.depth for _, c in obs]), np.stack([c.tf for _, c in obs]), MIN_DEPTH, MAX_DEPTH, fx, fx, slot)
        slots = sorted(reveal)
        om.update_after_ingest(np.stack([reveal[s] for s in slots]), MAX_DEPTH, FOV, env_ids=slots, explore=False, update_obstacles=True)
        om.check_status()
        for s, c in obs:
            _update(refs[s], c)
        obst = om._unpack(om.obstacle_bits).cpu().numpy().astype(bool)
        nav = om._unpack(om.navigable_bits).cpu().numpy().astype(bool)
        undone = om._slot_undone.cpu().numpy()
        counts = om._hole_counts[:len(obs)].cpu().numpy()
        undone_steps += bool(undone.any())
        print(f"edges E step{k}: inband={sum(int(c.statement(place=False).inband.sum()) for _, c in obs)} "
              f"cells={[int(r._map.sum()) for r in refs]} contours={int(counts[:, 0].sum())} filled={int(counts[:, 1].sum())} "
              f"island_frames={int((counts[:, 3] & 2).astype(bool).sum())} slots_undone={undone.tolist()}")
        for s in range(ic.E_SLOTS):
            assert np.array_equal(obst[s], refs[s]._map.astype(bool)), f"step {k} slot {s}: {(obst[s] != refs[s]._map).sum()} cells differ"
            assert np.array_equal(nav[s], np.asarray(refs[s]._navigable_map) != 0), f"step {k} slot {s}: navigable differs"
    assert undone_steps >= 2


# ------------------------------------------------------------------------------------------------ group F: refusal
def test_refused_width_changes_nothing(gpu_device):
    """A 48x62 frame (width no multiple of 4) raises what _lib.check raises for VLFM_ERR_INVALID, the planes stay as they were, and
    the next island frame is right: the journal the refused step left marked dirty undoes nothing."""
    from vlfm_amd import _lib

    with pytest.raises(Exception) as refused:
        _lib.check(_lib.VLFM_ERR_INVALID, "probe")
    first, odd, last = ic.f_cases()
    ours, ref = _pair(gpu_device, first)
    _step("F", ours, ref, first)
    before = (ours._map.copy(), ours._navigable_map.copy())
    with pytest.raises(refused.type, match="multiple of 4"):
        _update(ours, odd)
    assert np.array_equal(ours._map, before[0]) and np.array_equal(ours._navigable_map, before[1])
    print(f"edges F {odd.name}: {refused.type.__name__}, planes unchanged")
    _step("F", ours, ref, last)
