"""-m gpu: the camera-rig entry points -- several cameras per environment slot in ONE call -- against (1) the same
observations fed one camera per call through `update` / `ingest` (which are pinned to the reference), (2) the oracle, camera
by camera in the reference's order, and (3) the committed reference fixtures.  Every comparison is exact equality."""
import os
import sys

import numpy as np
import pytest

from rig_cases import MODELS_1000, ValueRig, columns, explored_plane, pack_plane
from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics, depth_frame, pose_to_tf

pytestmark = pytest.mark.gpu
MODES = [("default", False), ("default", True), ("replace", False), ("equal_weighting", False)]
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits_equal(a, b):
    """Bitwise equality of two device tensors (an f64 -0.0 differs from +0.0: the explored clear multiplies by zero)."""
    import torch

    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    elif a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return bool(torch.equal(a, b))


def _cells(size, ppm, tf):
    """(row, col) map cells of camera positions [n,4,4] (value_map.py:164-167's convention)."""
    px = (-tf[:, 0, 3] * ppm).astype(np.int64) + size // 2
    py = (-tf[:, 1, 3] * ppm).astype(np.int64) + size // 2
    return np.stack([size - px, py], axis=1)


class _Explored:
    """What RefValueMap reads of an attached obstacle map."""
    pixels_per_meter = 20

    def __init__(self, size):
        self.size = size
        self.explored_area = np.zeros((size, size), bool)


def _run_rig_vs_sequential(device, seed, size, models, width, fusion, use_max, channels, sync, steps=20, extent=20.0):
    import torch

    from vlfm_amd.mapping import ValueMapBatch

    rng = np.random.default_rng(seed)
    n_envs, K = int(rng.integers(1, 17)), int(rng.integers(2, 7))
    rig = ValueRig(seed + 1, range(n_envs), K, channels=channels, width=width, models=models, extent=extent)
    kw = dict(size=size, use_max_confidence=use_max, fusion_type=fusion, device=device)
    a, b = ValueMapBatch(n_envs, channels, **kw), ValueMapBatch(n_envs, channels, **kw)
    fused_cells = 0
    for step in range(steps):
        obs = rig.step()
        if n_envs > 1 and step % 3 == 1:      # not every slot reports every step
            keep = set(rng.choice(n_envs, size=int(rng.integers(1, n_envs + 1)), replace=False).tolist())
            obs = [o for o in obs if o[0] in keep]
        slot, depth, tf, lo, hi, fov, vals = columns(obs)
        if sync:
            planes = np.stack([explored_plane(rng, size, _cells(size, 20, tf[slot == e]), int(rng.integers(30, 90)))
                               if (slot == e).any() else np.zeros((size, size), bool) for e in range(n_envs)])
            ex = torch.from_numpy(pack_plane(planes)).to(device)
            a.explored_bits = b.explored_bits = ex
        a.update_cameras(vals, depth, tf, lo, hi, fov, slot)
        for i in range(len(obs)):
            b.update(vals[i:i + 1], depth[i:i + 1], tf[i:i + 1], float(lo[i]), float(hi[i]), float(fov[i]), env_ids=[int(slot[i])])
        assert _bits_equal(a.conf, b.conf), (seed, step, "conf")
        assert _bits_equal(a.value, b.value), (seed, step, "value")
        assert np.array_equal(a.n_updates, b.n_updates)
        if sync:
            assert _bits_equal(a._written, b._written), (seed, step, "written")
        wps = np.concatenate([tf[:, :2, 3] + rng.uniform(-1.5, 1.5, (len(obs), 2))])
        half = size / 40.0 - 0.1
        wps = np.clip(wps, -half, half)
        va, vb = a.waypoint_values(wps, slot, 0.5), b.waypoint_values(wps, slot, 0.5)
        assert np.array_equal(va, vb), (seed, step, "sort_waypoints values")
        assert np.array_equal(np.argsort(-va.max(axis=1), kind="stable"), np.argsort(-vb.max(axis=1), kind="stable"))
        fused_cells = int((b.conf > 0).sum())
    assert fused_cells > 500 * n_envs // 2, "the generator no longer fuses anything"
    assert int(a._counters.abs().sum()) == 0 and int(a._colmax.abs().sum()) == 0, "keys / counters were not handed back zeroed"


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("fusion,use_max", MODES)
def test_update_cameras_equals_one_camera_per_call(gpu_device, fusion, use_max, channels, sync):
    """Random rigs (K = 2..6 cameras, 1..16 slots interleaved in the call, mixed camera models), 20 steps: one `update_cameras`
    per step on one batch, the same observations through `update` one camera per call on another.  conf, value, `written`,
    sort_waypoints values and permutation equal after EVERY step, in all four fusion modes, C = 1 and 2, with and without
    the explored-synchronised mode."""
    seed = 900 + 8 * MODES.index((fusion, use_max)) + 2 * channels + int(sync)
    _run_rig_vs_sequential(gpu_device, seed, 1000, MODELS_1000, 640, fusion, use_max, channels, sync)


@pytest.mark.parametrize("sync", [False, True])
@pytest.mark.parametrize("size,hfov_deg,max_depth,width", [(500, 60.0, 3.5, 320), (700, 90.0, 8.0, 640)])
def test_update_cameras_other_map_sizes_and_camera_models(gpu_device, size, hfov_deg, max_depth, width, sync):
    """The map sizes / camera models of test_other_map_sizes_and_camera_models (tail words of the bit planes, T = 141 and 321 --
    the latter reads the confidence quadrant through the caches and overflows the cell list), windows clipped at the map edge."""
    models = [(float(np.deg2rad(hfov_deg)), max_depth), (float(np.deg2rad(hfov_deg)) * 0.8, max_depth * 0.5)]
    _run_rig_vs_sequential(gpu_device, size + int(sync), size, models, width, "default", False, 1, sync, extent=size / 40.0 - 1.0)


@pytest.mark.parametrize("sync", [False, True])
def test_update_cameras_against_the_oracle(gpu_device, sync):
    """A 16-slot rig batch, three cameras with mixed optics per slot: slots 0, 8 and 15 equal RefValueMap fed camera by camera
    in the reference's order (weighted mode: f32 -> f64 promotion included)."""
    import torch

    from oracle.ref_value_map import RefValueMap
    from vlfm_amd.mapping import ValueMap, ValueMapBatch

    rng = np.random.default_rng(77 + int(sync))
    rig = ValueRig(78 + int(sync), range(16), 3, models=MODELS_1000)
    vb = ValueMapBatch(16, 1, use_max_confidence=False, device=gpu_device)
    watch = (0, 8, 15)
    stubs = {e: _Explored(1000) for e in watch}
    refs = {e: RefValueMap(1, use_max_confidence=False, obstacle_map=stubs[e] if sync else None) for e in watch}
    for step in range(6):
        obs = rig.step()
        slot, depth, tf, lo, hi, fov, vals = columns(obs)
        if sync:
            planes = np.stack([explored_plane(rng, 1000, _cells(1000, 20, tf[slot == e]), 70) for e in range(16)])
            vb.explored_bits = torch.from_numpy(pack_plane(planes)).to(gpu_device)
            for e in watch:
                stubs[e].explored_area = planes[e]
        vb.update_cameras(vals, depth, tf, lo, hi, fov, slot)
        for o in obs:
            if o[0] in watch:
                refs[o[0]].update_map(o[6], o[1].copy(), o[2], o[3], o[4], o[5])
        for e in watch:
            view = ValueMap(1, use_max_confidence=False, _batch=vb, _slot=e)
            assert np.array_equal(view._map, refs[e]._map), (step, e)
            assert view._value_map.dtype == refs[e]._value_map.dtype
            assert np.array_equal(view._value_map, refs[e]._value_map), (step, e)
            assert (refs[e]._map > 0).sum() > 300


def test_two_camera_fixture_through_one_rig_call_per_step(gpu_device):
    """tests/golden/vm_two_cameras.npz (the REFERENCE's map after two cameras with different fov and range per step): both
    optics in ONE update_cameras call per step."""
    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import make_golden as mg
    from golden_util import dense, load, sha
    from vlfm_amd.mapping import ValueMapBatch

    g = load("vm_two_cameras")
    vb = ValueMapBatch(1, 1, use_max_confidence=False, device=gpu_device)
    k = 0
    for cams in mg.two_camera_script(int(g["seed"]), int(g["steps"])):
        for depth, *_ in cams:
            assert sha(depth) == str(g["depth_sha256"][k]), "synthetic depth differs from the fixture's input"
            k += 1
        depth, tf, lo, hi, fov, vals = (np.stack([c[i] for c in cams]) for i in range(6))
        vb.update_cameras(vals, depth, tf, lo, hi, fov, [0, 0])
    assert np.array_equal(vb.conf[0].cpu().numpy(), dense(g["conf_idx"], g["conf_val"], (1000, 1000), np.float32))
    assert sha(vb.value[0].cpu().numpy().reshape(1000, 1000)) == str(g["value_sha"])


def order_cases():
    """12 one-slot rigs of three overlapping cameras, two steps each (weighted mode)."""
    for case in range(12):
        rig = ValueRig(5000 + case, [0], 3)
        yield case, [rig.step() for _ in range(2)]


def oracle_forward_and_reversed(steps):
    from oracle.ref_value_map import RefValueMap

    fwd, rev = RefValueMap(1, use_max_confidence=False), RefValueMap(1, use_max_confidence=False)
    for obs in steps:
        for m, seq in ((fwd, obs), (rev, obs[::-1])):
            for o in seq:
                m.update_map(o[6], o[1].copy(), o[2], o[3], o[4], o[5])
    return fwd, rev


def test_order_within_a_slot_is_honoured(gpu_device):
    """Condition on the generator first: in weighted mode EVERY case gives a different map under the oracle when the cameras of a
    step are applied in reverse -- so a device that fused them in another order could not pass.  Then the device equals the
    forward order."""
    from vlfm_amd.mapping import ValueMapBatch

    for case, steps in order_cases():
        fwd, rev = oracle_forward_and_reversed(steps)
        differ = int((np.asarray(fwd._value_map) != np.asarray(rev._value_map)).sum())
        assert differ > 100, f"case {case}: the reversed camera order changes only {differ} cells -- order is not exercised"
        vb = ValueMapBatch(1, 1, use_max_confidence=False, device=gpu_device)
        for obs in steps:
            slot, depth, tf, lo, hi, fov, vals = columns(obs)
            vb.update_cameras(vals, depth, tf, lo, hi, fov, slot)
        assert np.array_equal(vb.conf[0].cpu().numpy(), fwd._map), case
        assert np.array_equal(vb.value[0].cpu().numpy(), np.asarray(fwd._value_map, np.float64)), case


def test_update_cameras_error_paths(gpu_device):
    """Same exception types as `update`: a camera window whose cell is outside the map and a slot out of range are
    AssertionErrors raised before anything is launched (keys handed in are zeroed, the maps are untouched); frames of different
    shapes are a ValueError."""
    import torch

    from vlfm_amd.mapping import ValueMapBatch

    vb = ValueMapBatch(2, 1, device=gpu_device)
    rng = np.random.default_rng(3)
    d = np.stack([depth_frame(rng) for _ in range(2)])
    fov = camera_intrinsics(640)[2]
    tfs = np.stack([pose_to_tf(0, 0, 0), pose_to_tf(0, 0, 1)])
    with pytest.raises(AssertionError, match="out of range"):
        vb.update_cameras(np.array([[0.3], [0.4]]), d, tfs, MIN_DEPTH, MAX_DEPTH, fov, [1, 2])
    keys = torch.full((2, 640), 7, dtype=torch.int32, device=gpu_device)
    with pytest.raises(AssertionError):
        vb.update_cameras(np.array([[0.3], [0.4]]), d, np.stack([tfs[0], pose_to_tf(80.0, 0, 0)]), MIN_DEPTH, MAX_DEPTH, fov,
                          [1, 1], colmax=keys)
    assert int(keys.abs().sum()) == 0
    with pytest.raises(ValueError, match="share the image shape"):
        vb.update_cameras(np.array([[0.3], [0.4]]), [d[0], d[1][:, :320]], tfs, MIN_DEPTH, MAX_DEPTH, fov, [1, 1])
    assert int((vb.conf != 0).sum()) == 0 and vb.n_updates.sum() == 0
    vb.update_cameras(np.array([[0.3], [0.4]]), [d[0], d[1]], tfs, MIN_DEPTH, [MAX_DEPTH, 2.5], fov, [1, 1])   # and it still works
    assert int((vb.conf[1] != 0).sum()) > 500 and int((vb.conf[0] != 0).sum()) == 0 and list(vb.n_updates) == [0, 2]


@pytest.mark.parametrize("workgroups", [1, 2])
def test_rig_with_one_and_two_workgroups_per_slot(gpu_device, workgroups):
    """The value tests above run with 7 workgroups per slot (few slots on a 256-CU device).  At >= 256 slots a slot has ONE
    workgroup, at 128 two: VLFM_VM_TARGET_WGS (read once per process) stands in for the CU count, so a child process repeats
    the value-map tests of this file with the launch shape of a large batch."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VLFM_VM_TARGET_WGS=str(workgroups))
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(root, "tests", "test_rig_gpu.py"), "-k", "update_cameras or order_within or two_camera_fixture"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------------------------------ obstacle map
OM_KW = dict(min_height=0.61, max_height=0.88, agent_radius=0.18, area_thresh=1.5)


def _planes(om):
    return om.obstacle_bits, om.navigable_bits, om.explored_bits


def _sequential_step(om, obs, reveal, fx, fy, fov, max_depth=MAX_DEPTH):
    """The reference's call pattern on the single-camera entry points: per camera an ingest + navigable recompute
    (explore=False), then one reveal-only call per slot."""
    import torch

    for slot, depth, tf in obs:
        d = torch.from_numpy(depth[None]).to(om.device)
        om.ingest(d, tf[None], MIN_DEPTH, max_depth, fx, fy, env_ids=[slot])
        om.update_after_ingest(tf[None], max_depth, fov, env_ids=[slot], explore=False)
    slots = sorted(reveal)
    om.update_after_ingest(np.stack([reveal[s] for s in slots]), max_depth, fov, env_ids=slots, explore=True,
                           update_obstacles=False)
    om.check_status()


def _rig_step(om, obs, reveal, fx, fy, fov, max_depth=MAX_DEPTH):
    slot = np.array([o[0] for o in obs])
    om.ingest_cameras(np.stack([o[1] for o in obs]), np.stack([o[2] for o in obs]), MIN_DEPTH, max_depth, fx, fy, slot)
    slots = sorted(reveal)
    om.update_after_ingest(np.stack([reveal[s] for s in slots]), max_depth, fov, env_ids=slots, explore=True,
                           update_obstacles=True)
    om.check_status()


def _assert_same_maps(a, b, where):
    import torch

    for name, x, y in zip(("obstacle", "navigable", "explored"), _planes(a), _planes(b)):
        assert torch.equal(x, y), (where, name, int((x != y).sum()))
    fa, fb = a.frontiers_px(), b.frontiers_px()
    for e in range(a.n_envs):
        assert np.array_equal(fa[e], fb[e]), (where, "frontiers", e)


@pytest.mark.parametrize("hole_thresh", [None, -1])
def test_ingest_cameras_equals_one_camera_per_call(gpu_device, hole_thresh):
    """Random rigs (one slot with 6 cameras, 16 slots with 5, a random 2..16 slots with 2..6; slots interleaved in the call and
    dropping out of steps; clean / holed / island frames), 20 steps each: one `ingest_cameras` + one `update_after_ingest` per step vs the K + 1 single-camera calls of the reference's pattern; obstacle / navigable / explored
    planes and frontiers equal after every step, with the dirty windows and with full-plane kernels."""
    from rig_cases import HOLE_THRESH, ObstacleRig
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    fx, fy, fov = camera_intrinsics(640)
    thresh = HOLE_THRESH if hole_thresh is None else hole_thresh
    for case in range(3):
        rng = np.random.default_rng(300 + case + (10 if thresh == -1 else 0))
        n_envs, K = (1, 6) if case == 0 else (16, 5) if case == 1 else (int(rng.integers(2, 17)), int(rng.integers(2, 7)))
        steps = 20
        rig = ObstacleRig(400 + case, range(n_envs), K)
        a, b, c = (ObstacleMapBatch(n_envs, hole_area_thresh=thresh, device=gpu_device, **OM_KW) for _ in range(3))
        c.full_planes = True
        for step in range(steps):
            obs, reveal = rig.step()
            if n_envs > 2 and step % 3 == 1:
                keep = set(rng.choice(n_envs, size=int(rng.integers(1, n_envs)), replace=False).tolist())
                obs = [o for o in obs if o[0] in keep]
                reveal = {s: reveal[s] for s in keep}
            _rig_step(a, obs, reveal, fx, fy, fov)
            _sequential_step(b, obs, reveal, fx, fy, fov)
            _rig_step(c, obs, reveal, fx, fy, fov)
            _assert_same_maps(a, b, (case, step, "rig vs sequential"))
            _assert_same_maps(a, c, (case, step, "windowed vs full planes"))
        assert int((a.obstacle_bits != 0).sum()) > 20 * n_envs


def _island_pairs():
    """Two cameras of one slot at the SAME pose, so their obstacle cells coincide: (island frame, hole-free frame), the reverse, two
    island frames, and a rig without a zero texel at all (the simulator's case)."""
    from rig_cases import ring, wall_frame

    tf = pose_to_tf(0.4, -0.3, 0.7)
    # a wall 3 m away: its in-band image rows (240..275) all cross the ring, so the ring's columns lose EVERY in-band texel and the
    # island frame alone leaves 9 obstacle cells out that the hole-free frame sets
    clean = wall_frame(3.0).copy()
    isl_a = ring(wall_frame(3.0).copy(), 320, 258, 30, 14)
    isl_b = ring(ring(wall_frame(3.0).copy(), 200, 258, 36, 20), 470, 258, 22, 9)
    return {"island_then_clean": [(0, isl_a, tf), (0, clean, tf)], "clean_then_island": [(0, clean, tf), (0, isl_a, tf)],
            "both_islands": [(0, isl_a, tf), (0, isl_b, tf)], "no_zero_texel": [(0, clean, tf), (0, wall_frame(2.4).copy(), tf)]}, tf


@pytest.mark.parametrize("name", ["island_then_clean", "clean_then_island", "both_islands", "no_zero_texel"])
def test_island_frames_in_a_rig(gpu_device, name):
    """The undo journal records a new bit for the frame that set it first.  An island frame whose bits are taken back must not
    take a sibling's legitimate bits with it: the result equals the sequential path and RefObstacleMap.  The island frame
    really is one (the reference drops cells that the speculative pass had placed), so the undo path is exercised."""
    from oracle.ref_obstacle_map import RefObstacleMap
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    fx, fy, fov = camera_intrinsics(640)
    cases, tf = _island_pairs()
    obs = cases[name]
    a, b = (ObstacleMapBatch(1, device=gpu_device, **OM_KW) for _ in range(2))
    ref = RefObstacleMap(**OM_KW)
    for rep in range(2):   # the second round meets the first round's bits already set (nothing to journal)
        _rig_step(a, obs, {0: tf}, fx, fy, fov)
        _sequential_step(b, obs, {0: tf}, fx, fy, fov)
        for _, depth, t in obs:
            ref.update_map(depth.copy(), t, MIN_DEPTH, MAX_DEPTH, fx, fy, fov, explore=False)
        ref.update_map(None, tf, MIN_DEPTH, MAX_DEPTH, fx, fy, fov, explore=True, update_obstacles=False)
        _assert_same_maps(a, b, (name, rep))
        # the device saw an island frame in the slot (and re-placed the siblings' texels) exactly in the island cases
        assert int(a._slot_undone[0]) == int(name != "no_zero_texel"), (name, rep)
        got = a._unpack(a.obstacle_bits)[0].cpu().numpy().astype(bool)
        assert np.array_equal(got, ref._map.astype(bool)), (name, rep)
        assert np.array_equal(a.explored[0].cpu().numpy().astype(bool), ref.explored_area.astype(bool)), (name, rep)
        assert np.array_equal(a.frontiers_px()[0], np.asarray(ref._frontiers_px, np.float64).reshape(-1, 2)), (name, rep)
    assert ref._map.sum() > 20
    if name != "no_zero_texel":
        # the island frame ALONE leaves cells out that its sibling sets: the sibling's bits are what the undo must not take
        alone = RefObstacleMap(**OM_KW)
        alone.update_map(cases["island_then_clean"][0][1].copy(), tf, MIN_DEPTH, MAX_DEPTH, fx, fy, fov, explore=False)
        assert (ref._map.astype(bool) & ~alone._map.astype(bool)).sum() > 0


def test_ingest_cameras_against_the_oracle(gpu_device):
    """Slots 0 / 8 / 15 of a 16-slot rig batch vs RefObstacleMap fed camera by camera (explore=False) + the reveal."""
    from oracle.ref_obstacle_map import RefObstacleMap
    from rig_cases import HOLE_THRESH, ObstacleRig
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    fx, fy, fov = camera_intrinsics(640)
    rig = ObstacleRig(61, range(16), 3)
    a = ObstacleMapBatch(16, hole_area_thresh=HOLE_THRESH, device=gpu_device, **OM_KW)
    watch = (0, 8, 15)
    refs = {e: RefObstacleMap(hole_area_thresh=HOLE_THRESH, **OM_KW) for e in watch}
    for step in range(5):
        obs, reveal = rig.step()
        _rig_step(a, obs, reveal, fx, fy, fov)
        for slot, depth, tf in obs:
            if slot in watch:
                refs[slot].update_map(depth.copy(), tf, MIN_DEPTH, MAX_DEPTH, fx, fy, fov, explore=False)
        planes = [a._unpack(p).cpu().numpy().astype(bool) for p in _planes(a)]
        fr = a.frontiers_px()
        for e in watch:
            refs[e].update_map(None, reveal[e], MIN_DEPTH, MAX_DEPTH, fx, fy, fov, explore=True, update_obstacles=False)
            assert np.array_equal(planes[0][e], refs[e]._map.astype(bool)), (step, e)
            assert np.array_equal(planes[1][e], refs[e]._navigable_map.astype(bool)), (step, e)
            assert np.array_equal(planes[2][e], refs[e].explored_area.astype(bool)), (step, e)
            assert np.array_equal(fr[e], np.asarray(refs[e]._frontiers_px, np.float64).reshape(-1, 2)), (step, e)


def test_multicam_fixture_through_one_rig_ingest_per_step(gpu_device):
    """tests/golden/om_multicam.npz (the REFERENCE's planes and frontiers for the robot's call pattern): the K cameras of a step in
    ONE ingest_cameras, then one update_after_ingest from the robot pose."""
    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import make_golden as mg
    from golden_util import load, sha, unpack_plane
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    g = load("om_multicam")
    om = ObstacleMapBatch(1, hole_area_thresh=100000, min_height=0.1, max_height=1.5, agent_radius=0.2, area_thresh=1.5,
                          device=gpu_device)
    offs = np.concatenate([[0], np.cumsum(g["frontier_counts"])])
    k = 0
    for step, (cams, tf_robot, fx, fy, fov) in enumerate(mg.multicam_script(int(g["seed"]), int(g["steps"]))):
        for depth, _ in cams:
            assert sha(depth) == str(g["depth_sha256"][k]), "synthetic depth differs from the fixture's input"
            k += 1
        om.ingest_cameras(np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams]), 0.5, 2.5, fx, fy, [0] * len(cams))
        om.update_after_ingest(tf_robot[None], 2.5, 2 * fov, env_ids=[0], explore=True, update_obstacles=True)
        om.check_status()
        got = om.px_to_xy(om.frontiers_px()[0]) if len(om.frontiers_px()[0]) else np.zeros((0, 2))
        assert np.array_equal(np.asarray(got, np.float64).reshape(-1, 2), g["frontiers_xy"][offs[step]:offs[step + 1]]), step
    for name, plane in zip(("obstacle_bits", "navigable_bits", "explored_bits"), _planes(om)):
        assert np.array_equal(om._unpack(plane)[0].cpu().numpy().astype(bool), unpack_plane(g[name])), name


def test_ingest_cameras_error_paths(gpu_device):
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    fx, fy, fov = camera_intrinsics(640)
    om = ObstacleMapBatch(2, device=gpu_device, **OM_KW)
    d = np.stack([depth_frame(np.random.default_rng(1)) for _ in range(2)])
    tfs = np.stack([pose_to_tf(0, 0, 0), pose_to_tf(0, 0, 1)])
    with pytest.raises(AssertionError, match="out of range"):
        om.ingest_cameras(d, tfs, MIN_DEPTH, MAX_DEPTH, fx, fy, [1, 2])
    with pytest.raises(ValueError, match="share the image shape"):
        om.ingest_cameras([d[0], d[1][:, :320]], tfs, MIN_DEPTH, MAX_DEPTH, fx, fy, [1, 1])
    om.ingest_cameras(d, np.stack([tfs[0], pose_to_tf(30.0, 0, 0)]), MIN_DEPTH, MAX_DEPTH, fx, fy, [1, 1])   # points off the map
    with pytest.raises(IndexError):
        om.check_status()


# ------------------------------------------------------------------------------------------------ batched rig step
def test_batched_rig_step_equals_sequential_drop_in_maps(gpu_device):
    """BatchedEpisodes(n_envs=8, rig=three cameras: two feed both maps with different optics, one the obstacle map only), stub
    cosines, 40 steps: slots 0 / 3 / 7 equal the drop-in ObstacleMap / ValueMap fed the downloaded frames camera by camera in
    the order of ITMPolicyV2Step.step_cameras (obstacle cameras with explore=False, the reveal from the robot pose, then the
    value cameras)."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig
    from vlfm_amd.mapping import ObstacleMap, ValueMap

    rig = CameraRig([Camera(yaw=0.5, max_depth=3.5), Camera(yaw=-0.5, forward=0.1, hfov=float(np.deg2rad(60.0))),
                     Camera(yaw=np.pi, left=0.1, value=False, max_depth=2.5)])
    sim = BatchedEpisodes(8, device=gpu_device, use_blip2=False, rig=rig, episode_len=500)
    fov0 = camera_intrinsics(640)[2]
    hfov = [fov0 if c.hfov is None else c.hfov for c in rig.cameras]
    fx = [640 / (2 * np.tan(h / 2)) for h in hfov]
    watch = (0, 3, 7)
    oms = {e: ObstacleMap(device=gpu_device, **OM_KW) for e in watch}
    vms = {e: ValueMap(1, use_max_confidence=False, device=gpu_device) for e in watch}
    for step in range(40):
        t = sim.t % 500
        sim.step()
        torch.cuda.synchronize()
        depth, tf, slot, cam = sim.last_rig
        depth, cos = depth.cpu().numpy(), sim.last_cosines.double().cpu().numpy().reshape(-1)
        v_rows = [i for i in range(len(slot)) if rig.cameras[cam[i]].value]
        assert len(cos) == len(v_rows) == 16
        for e in watch:
            mine = [i for i in range(len(slot)) if slot[i] == e]
            assert [cam[i] for i in mine] == [0, 1, 2]
            for i in mine:
                c = rig.cameras[cam[i]]
                if c.obstacle:
                    oms[e].update_map(depth[i], tf[i], c.min_depth, c.max_depth, fx[cam[i]], fx[cam[i]], hfov[cam[i]], explore=False)
            oms[e].update_map(None, sim.tf_table[t][e], MIN_DEPTH, 5.0, fx[0], fx[0], max(hfov), explore=True, update_obstacles=False)
            for i in mine:
                c = rig.cameras[cam[i]]
                if c.value:
                    vms[e].update_map(cos[v_rows.index(i):v_rows.index(i) + 1], depth[i], tf[i], c.min_depth, c.max_depth, hfov[cam[i]])
            for name, got, want in zip(("obstacle", "navigable", "explored"), _planes(sim.obstacles), _planes(oms[e]._batch)):
                assert torch.equal(got[e], want[0]), (step, e, name)
            assert np.array_equal(sim.obstacles.frontiers_px()[e], np.asarray(oms[e]._frontiers_px, np.float64).reshape(-1, 2)), (step, e)
            assert _bits_equal(sim.values.conf[e], vms[e]._batch.conf[0]), (step, e, "conf")
            assert _bits_equal(sim.values.value[e], vms[e]._batch.value[0]), (step, e, "value")
    sim.check()
    assert int((sim.values.conf[0] > 0).sum()) > 2000 and list(sim.values.n_updates) == [80] * 8


def test_rig_of_one_camera_at_the_robot_pose_equals_no_rig(gpu_device):
    """rig=None is the step as it always was (tests/test_harness_gpu.py holds it to the oracle); a rig of ONE camera at the robot
    pose goes through ingest_cameras / update_cameras instead and must give the same maps, frontiers and frontier values."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig

    a = BatchedEpisodes(4, device=gpu_device, use_blip2=False, episode_len=500)
    b = BatchedEpisodes(4, device=gpu_device, use_blip2=False, episode_len=500, rig=CameraRig([Camera()]))
    for step in range(30):
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert torch.equal(a.rooms.frame((a.t - 1) % 500), b.last_rig[0]), step
        for name, x, y in zip(("obstacle", "navigable", "explored"), _planes(a.obstacles), _planes(b.obstacles)):
            assert torch.equal(x, y), (step, name)
        assert _bits_equal(a.values.conf, b.values.conf) and _bits_equal(a.values.value, b.values.value), step
        fa, fb = a.last_frontier_values, b.last_frontier_values
        assert (fa is None) == (fb is None) and (fa is None or np.array_equal(fa, fb)), step
    a.check()
    b.check()


def test_rig_detector_stage_uses_the_designated_camera(gpu_device):
    """With a rig the detector / segmenter / object-map stage keeps ONE camera per environment (object_map_rgbd on the robot):
    the designated one.  A rig whose designated camera sits at the robot pose, between two other cameras, must build the same
    object clouds, detections and object-goal decisions as the harness without a rig (whose single camera is that pose), on
    the scripted sightings; the scripted objects are painted into the designated camera's depth frame."""
    import torch

    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig, ScriptedSightings

    def make(**kw):
        return BatchedEpisodes(4, device=gpu_device, use_blip2=False, episode_len=500, object_maps=True, select_frontiers=True,
                               sightings=ScriptedSightings(search_min=3, search_span=4, nav_steps=12), **kw)

    rig = CameraRig([Camera(yaw=0.6, max_depth=3.5), Camera(), Camera(yaw=-0.6, value=False)], designated=1)
    a, b = make(), make(rig=rig)
    navigated = 0
    for step in range(60):
        t = a.t % 500
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert torch.equal(a.rooms.frame(t), b.last_rig[0][1::3]), (step, "designated frames = the robot camera's, objects painted")
        for e in range(4):
            da, db = a.last_detections[e], b.last_detections[e]
            assert torch.equal(da.boxes, db.boxes) and list(da.phrases) == list(db.phrases), (step, e)
            ca, cb = a.object_maps[e].clouds, b.object_maps[e].clouds
            assert sorted(ca) == sorted(cb), (step, e)
            for name in ca:
                assert np.array_equal(np.asarray(ca[name]), np.asarray(cb[name])), (step, e, name)
        nav_a = [m == "navigate" for m in a.last_modes]
        assert nav_a == [m == "navigate" for m in b.last_modes], step
        assert np.array_equal(a.last_goals[nav_a], b.last_goals[nav_a]), step
        assert np.array_equal(a.last_episode_end, b.last_episode_end)
        navigated += sum(nav_a)
    for k in ("detections", "masks", "cloud_updates"):
        assert a.object_stats[k] == b.object_stats[k], k
    assert b.object_stats["cloud_updates"] > 5 and navigated > 5, (b.object_stats, navigated)
    with pytest.raises(ValueError, match="designated camera"):
        make(rig=CameraRig([Camera(max_depth=3.5), Camera()], designated=0))


def test_no_rig_maps_are_what_they_were(gpu_device):
    """BatchedEpisodes() without a rig is the step as it always was: the digest of its maps after 30 stub-cosine steps of 4
    environments, recorded from the commit before camera rigs existed (the renderer's ray cast was refactored for them)."""
    import hashlib

    import torch

    from vlfm_amd.harness import BatchedEpisodes

    sim = BatchedEpisodes(4, device=gpu_device, use_blip2=False, episode_len=500)
    for _ in range(30):
        sim.step()
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in (sim.values.conf, sim.values.value, sim.obstacles.obstacle_bits, sim.obstacles.navigable_bits, sim.obstacles.explored_bits):
        h.update(t.cpu().numpy().tobytes())
    assert h.hexdigest() == "0dd79ea6165fe7077ced42947dd8dc0b4916ad4aad30ee8d6e9a28c9803648c1"
