"""-m gpu: the object-map update with several jobs per call (object_point_cloud_map.update_maps_batch, csrc/object_cloud.hip): all
detections of a step through erosion, back-projection, sub-sampling and DBSCAN together.  Clouds, goals and every draw of every
NumPy generator must be BIT-IDENTICAL to the reference's own class (tests/golden/object_map_rand*.npz), to the oracle restatement
(oracle/ref_object_map.py) and to the same detections sent as batches of one job (ObjectPointCloudMap.update_map,
_extract_object_cloud): a job's result must not depend on what else is in its batch."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

from golden_util import load
from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

FULL_JOB = 5000 * 79 * 8 + 16 * 5000 + 192        # DBSCAN scratch of one 5000-point job: a budget of this is one job per chunk


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _same(a, b) -> bool:
    """Bit for bit, shape and dtype included."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _state_equal(a, b) -> bool:
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---------------------------------------------------------------------------------------------- 1. the reference's sessions
@functools.lru_cache(maxsize=None)
def _random_sessions():
    from make_golden import object_map_random_script

    return [object_map_random_script(seed) for seed in (0, 1, 2)]


@pytest.mark.parametrize("budget", [None, FULL_JOB], ids=["default-budget", "one-job-per-chunk"])
def test_three_reference_sessions_in_lockstep(gpu_device, budget):
    """The three random sessions recorded from the reference's ObjectPointCloudMap (tests/test_object_map_gpu.py replays them one
    by one) as three maps of erosion 3 / 5 / 2: every `update` index is ONE update_maps_batch of three jobs."""
    from vlfm_amd.mapping.object_point_cloud_map import ObjectPointCloudMap, update_maps_batch

    sessions = _random_sessions()
    golden = [load(f"object_map_rand{seed}") for seed in (0, 1, 2)]
    assert len({len(s) for s in sessions}) == 1 and all(len({s[i][0] for s in sessions}) == 1 for i in range(len(sessions[0])))
    fx, fy, fov = camera_intrinsics(640)
    maps = [ObjectPointCloudMap(erosion_size=(3, 5, 2)[seed], device=gpu_device, rng=np.random.RandomState(4321 + seed))
            for seed in (0, 1, 2)]
    kw = {} if budget is None else {"scratch_budget_bytes": budget}
    n_best = 0
    for i in range(len(sessions[0])):
        ops = [s[i] for s in sessions]
        if ops[0][0] == "update":
            update_maps_batch(maps, [op[1] for op in ops], np.stack([op[2] for op in ops]), [0, 1, 2],
                              np.stack([op[3] for op in ops]), [op[4] for op in ops], MIN_DEPTH, MAX_DEPTH, fx, fy, **kw)
        for m, op, g in zip(maps, ops, golden):
            if op[0] == "best":
                assert [int(m.has_object(n)) for n in ("chair", "bed", "tv")] == list(g[f"has_{i}"]), i
                if m.has_object(op[1]):
                    assert np.array_equal(np.asarray(m.get_best_object(op[1], op[2]), np.float64), g[f"best_{i}"]), i
                    n_best += 1
            elif op[0] == "explored":
                m.update_explored(op[1], MAX_DEPTH, fov)
            for name in ("chair", "bed", "tv"):
                assert (name in m.clouds) == (f"sig_{i}_{name}" in g), (i, name)
                if name in m.clouds:
                    c = np.asarray(m.clouds[name], np.float64)
                    assert [str(c.shape[0]), _sha(c)] == list(g[f"sig_{i}_{name}"]), (i, name, c.shape)
    assert n_best >= 15
    for m, g in zip(maps, golden):
        for name in ("chair", "bed", "tv"):
            if f"final_{name}" in g:
                assert np.array_equal(np.asarray(m.clouds[name], np.float64), g[f"final_{name}"])


# ---------------------------------------------------------------------------------------------- 2. draws of a shared generator
@functools.lru_cache(maxsize=None)
def _script_updates():
    from make_golden import object_map_script

    return [op for op in object_map_script() if op[0] == "update"]


@pytest.mark.parametrize("shared", ["RandomState", "global"])
def test_draw_order_with_a_shared_generator(gpu_device, shared):
    """object_map_script()'s six updates as calls of 1, 2 and 3 jobs on ONE map, so that every job of a call shares the map's
    generator.  With erosion 5 the masks keep 6483, 8689, 3109, 3217, 29821 and 5 points: the big blob (index 4) needs a
    `choice` and is the second job of its call, behind a job whose `rand` has to be drawn first."""
    from vlfm_amd.mapping.object_point_cloud_map import ObjectPointCloudMap, update_maps_batch

    ups = _script_updates()
    assert len(ups) == 6
    calls = [[0], [1, 2], [3, 4, 5]]
    fx, fy, _ = camera_intrinsics(640)

    def run(batched):
        if shared == "global":
            np.random.seed(7)
            m = ObjectPointCloudMap(erosion_size=5, device=gpu_device)
        else:
            m = ObjectPointCloudMap(erosion_size=5, device=gpu_device, rng=np.random.RandomState(7))
        after = []
        for call in calls:
            if batched:
                update_maps_batch([m] * len(call), [ups[k][1] for k in call], np.stack([ups[k][2] for k in call]),
                                  list(range(len(call))), np.stack([ups[k][3] for k in call]), [ups[k][4] for k in call],
                                  MIN_DEPTH, MAX_DEPTH, fx, fy)
            else:
                for k in call:
                    m.update_map(ups[k][1], ups[k][2], ups[k][3], ups[k][4], MIN_DEPTH, MAX_DEPTH, fx, fy)
            after.append({name: c.copy() for name, c in m.clouds.items()})
        return after, (np.random.get_state() if shared == "global" else m._rng.get_state())

    one_by_one, state_a = run(False)
    together, state_b = run(True)
    assert any(len(c) for c in one_by_one[-1].values())
    for a, b in zip(one_by_one, together):
        assert a.keys() == b.keys()
        for name in a:
            assert _same(a[name], b[name]), (name, a[name].shape, b[name].shape)
    assert _state_equal(state_a, state_b)


# ---------------------------------------------------------------------------------------------- 3. small shapes
SH, SW = 50, 70            # W is no multiple of 32: three words per row, the last with 6 live bits


def _block(n, y0, x0, wide=12):
    """The first n pixels, row-major, of a `wide`-column block at (y0, x0): a compact blob of exactly n points."""
    m = np.zeros((SH, SW), np.uint8)
    for k in range(n):
        m[y0 + k // wide, x0 + k % wide] = 1
    return m


@functools.lru_cache(maxsize=None)
def _small():
    """(depth frames [3][SH][SW], specs): spec = (what, mask, frame, erosion).  Frame 0: a near surface (0.95 m: 0.2 m is 9 pixels,
    blobs of >= 100 points are clusters); frame 1: the same with holes (depth 0 -> the far plane); frame 2: the far plane (5 m:
    0.2 m is under 2 pixels, every point is noise)."""
    rng = np.random.default_rng(11)
    near = (0.1 + 0.004 * rng.random((SH, SW))).astype(np.float32)
    holes = near.copy()
    holes[18:24, 20:27] = 0.0
    far = np.ones((SH, SW), np.float32)
    thin = np.zeros((SH, SW), np.uint8)
    thin[10:14, 5:60] = 1
    pixel = np.zeros((SH, SW), np.uint8)
    pixel[49, 69] = 1
    cross = np.zeros((SH, SW), np.uint8)
    cross[20:31, :] = 1
    cross[:, 30:41] = 1
    holed = np.zeros((SH, SW), np.uint8)
    holed[10:32, 12:36] = 1
    big = np.zeros((SH, SW), np.uint8)
    big[8:42, 33:69] = 1
    specs = [("erodes to nothing", thin, 0, 3), ("one pixel", pixel, 0, 0), ("63 points", _block(63, 3, 2), 0, 0),
             ("64 points", _block(64, 30, 50), 0, 0), ("65 points", _block(65, 20, 29), 1, 0),
             ("129 points", _block(129, 35, 1), 0, 0), ("touches all four borders", cross, 0, 1),
             ("holes inside", holed, 1, 1), ("erosion 3", big, 0, 3), ("all noise", _block(400, 5, 10, wide=20), 2, 0),
             ("empty mask", np.zeros((SH, SW), np.uint8), 2, 1)]
    return np.stack([near, holes, far]), specs


@functools.lru_cache(maxsize=None)
def _small_oracle(use_dbscan):
    from oracle.ref_object_map import extract_object_cloud

    depth, specs = _small()
    fx, fy, _ = camera_intrinsics(SW)
    return [extract_object_cloud(depth[f], m, it, MIN_DEPTH, MAX_DEPTH, fx, fy, use_dbscan=use_dbscan) for _, m, f, it in specs]


def _maps(device, use_dbscan, rng=None):
    from vlfm_amd.mapping.object_point_cloud_map import ObjectPointCloudMap

    maps = {}
    for it in (0, 1, 3):
        maps[it] = ObjectPointCloudMap(erosion_size=it, device=device, rng=rng)
        maps[it].use_dbscan = use_dbscan
    return maps


@pytest.mark.parametrize("use_dbscan", [False, True], ids=["no-dbscan", "dbscan"])
@pytest.mark.parametrize("D", [1, 3, 11, 67])
def test_small_shapes_against_oracle_and_single_path(gpu_device, D, use_dbscan):
    """D = 11 is every case once; 67 cycles through them (more jobs than a wavefront has lanes); 1 and 3 start at the 129-point blob
    so that the smallest batches hold a cluster."""
    from vlfm_amd.mapping.object_point_cloud_map import extract_object_clouds_batch, too_offset

    depth, specs = _small()
    fx, fy, _ = camera_intrinsics(SW)
    want = _small_oracle(use_dbscan)
    maps = _maps(gpu_device, use_dbscan)
    pick = [(5 + j) % len(specs) for j in range(D)] if D < len(specs) else [j % len(specs) for j in range(D)]
    got = list(extract_object_clouds_batch([maps[specs[s][3]] for s in pick], depth, [specs[s][2] for s in pick],
                                           np.stack([specs[s][1] for s in pick]), MIN_DEPTH, MAX_DEPTH, fx, fy))
    assert [g[0] for g in got] == list(range(D))
    single = {}
    for j, s in enumerate(pick):
        what, mask, frame, it = specs[s]
        if s not in single:
            single[s] = maps[it]._extract_object_cloud(depth[frame], mask, MIN_DEPTH, MAX_DEPTH, fx, fy)
        cloud = got[j][1]
        assert _same(cloud, want[s]), (what, j, cloud.shape, want[s].shape)
        assert _same(cloud, single[s]), (what, j, cloud.shape, single[s].shape)
        assert got[j][2] == too_offset(mask), (what, j)
    if use_dbscan:
        by = {specs[s][0]: got[j][1] for j, s in enumerate(pick)}
        assert len(by["129 points"]) > 0
        if D >= len(specs):
            assert by["all noise"].shape == (0,) and by["erodes to nothing"].shape == (0,) and by["empty mask"].shape == (0,)
            assert len(by["touches all four borders"]) > 0 and len(by["holes inside"]) > 0


def test_point_counts_and_column_extents(gpu_device):
    import torch

    from vlfm_amd.mapping.object_point_cloud_map import mask_stats_batch
    from oracle.ref_object_map import erode3x3

    _, specs = _small()
    masks = np.stack([m for _, m, _, _ in specs])
    _, st = mask_stats_batch(torch.from_numpy(masks).to(gpu_device), [it for _, _, _, it in specs], gpu_device)
    for (what, m, _, it), row in zip(specs, st):
        cols = np.flatnonzero(m.any(0))
        assert int(row[0]) == int((erode3x3(m, it) > 0).sum()), what
        assert (int(row[1]), int(row[2])) == ((int(cols[0]), int(cols[-1])) if len(cols) else (-1, -1)), what


def test_more_than_5000_points_behind_a_small_job(gpu_device):
    """96 x 80 frames; job 0 a small blob, job 1 an all-ones mask (the border does not erode: 7680 points), 5000 of them drawn by
    the map's generator."""
    from oracle.ref_object_map import extract_object_cloud
    from vlfm_amd.mapping.object_point_cloud_map import ObjectPointCloudMap, extract_object_clouds_batch

    H, W = 80, 96
    rng = np.random.default_rng(12)
    depth = (0.1 + 0.004 * rng.random((1, H, W))).astype(np.float32)
    depth[0, 30:34, 40:50] = 0.0
    small = np.zeros((H, W), np.uint8)
    small[5:16, 5:17] = 1
    small[5, 5:8] = 0
    masks = np.stack([small, np.ones((H, W), np.uint8)])
    fx, fy, _ = camera_intrinsics(W)
    for use_dbscan in (False, True):
        np.random.seed(99)
        want = [extract_object_cloud(depth[0], m, 1, MIN_DEPTH, MAX_DEPTH, fx, fy, use_dbscan=use_dbscan) for m in masks]
        state = np.random.get_state()
        clouds = {}
        for path in ("batch", "single"):
            om = ObjectPointCloudMap(erosion_size=1, device=gpu_device, rng=np.random.RandomState(99))
            om.use_dbscan = use_dbscan
            if path == "batch":
                clouds[path] = [c for _, c, _ in extract_object_clouds_batch([om, om], depth, [0, 0], masks, MIN_DEPTH,
                                                                             MAX_DEPTH, fx, fy)]
            else:
                clouds[path] = [om._extract_object_cloud(depth[0], m, MIN_DEPTH, MAX_DEPTH, fx, fy) for m in masks]
            assert _state_equal(om._rng.get_state(), state)
        for j in range(2):
            assert _same(clouds["batch"][j], want[j]), (use_dbscan, j, clouds["batch"][j].shape, want[j].shape)
            assert _same(clouds["batch"][j], clouds["single"][j]), (use_dbscan, j)
        assert len(clouds["batch"][1]) == 5000 if not use_dbscan else len(clouds["batch"][1]) > 0


# ---------------------------------------------------------------------------------------------- 4. the harness
def test_harness_batched_equals_one_by_one(gpu_device):
    """Two closed-loop ObjectNav harnesses of 8 environments, one with batch_object_maps=False.  Environment 0 starts with its chair
    2.25 m ahead and environment 1 with its bed 1.2 m ahead (tests/test_objectnav_closed_loop_gpu.py: the chair is reached after
    19 steps), everybody else, and every later episode, draws the default layout."""
    import torch

    from vlfm_amd import synthetic as S
    from vlfm_amd.harness import BatchedEpisodes, WorldObjects
    from world_object_cases import A

    bed = (2.95, 1.42, 3.95, 2.32, 0.0, 0.7)

    def layout(env_id, episode, robot_xy):
        if episode == 0 and env_id in (0, 1):
            return [("chair", A)] if env_id == 0 else [("bed", bed)]
        return S.object_layout(env_id, episode, robot_xy)

    sims = [BatchedEpisodes(8, device=gpu_device, use_blip2=False, select_frontiers=True, episode_len=500, closed_loop=True,
                            world_objects=WorldObjects(layout=layout, max_episode_steps=100), object_maps=True,
                            batch_object_maps=batched) for batched in (False, True)]
    assert sims[1].batch_object_maps and not sims[0].batch_object_maps
    together = 0
    for t in range(20):
        for s in sims:
            s.step()
        a, b = sims
        assert np.array_equal(a.last_goals, b.last_goals, equal_nan=True), t
        assert a.last_modes == b.last_modes, t
        assert np.array_equal(a.last_world_actions, b.last_world_actions), t
        assert (a.last_masks is None) == (b.last_masks is None), t
        if a.last_masks is not None:
            assert a.last_masks[0] == b.last_masks[0], t
            together += len(set(a.last_masks[0])) >= 2
        for ma, mb in zip(a.object_maps, b.object_maps):
            assert ma.clouds.keys() == mb.clouds.keys(), t
            for name in ma.clouds:
                assert _same(ma.clouds[name], mb.clouds[name]), (t, name)
            assert _state_equal(ma._rng.get_state(), mb._rng.get_state()), t
    torch.cuda.synchronize()
    a, b = sims
    assert together >= 1                                          # a step with detections in two or more environments
    assert int(a.live.objectnav_stats["episodes"].sum()) >= 1          # an episode ended
    assert a.object_stats["cloud_updates"] > 0
    assert a.object_stats.keys() == b.object_stats.keys()
    for key in a.object_stats:
        assert np.array_equal(np.asarray(a.object_stats[key]), np.asarray(b.object_stats[key])), key
    assert a.live.objectnav_stats.keys() == b.live.objectnav_stats.keys()
    for key in a.live.objectnav_stats:
        assert np.array_equal(np.asarray(a.live.objectnav_stats[key]), np.asarray(b.live.objectnav_stats[key])), key


# ---------------------------------------------------------------------------------------------- 5. launches and read-backs
def test_launches_and_syncs_do_not_grow_with_the_jobs(gpu_device):
    from vlfm_amd import _lib
    from vlfm_amd.mapping import object_point_cloud_map as opm

    L = _lib.lib()
    depth, specs = _small()
    fx, fy, _ = camera_intrinsics(SW)
    cost = {}
    for D in (2, 16):
        maps = [opm.ObjectPointCloudMap(erosion_size=(3, 1)[j % 2], device=gpu_device, rng=np.random.RandomState(j))
                for j in range(D)]
        pick = [(8, 7)[j % 2] for j in range(D)]                  # "erosion 3" and "holes inside": every job reaches the DBSCAN
        launches, syncs = L.vlfm_object_cloud_launch_count(), opm.SYNCS[0]
        out = list(opm.extract_object_clouds_batch(maps, depth, [specs[s][2] for s in pick], np.stack([specs[s][1] for s in pick]),
                                                   MIN_DEPTH, MAX_DEPTH, fx, fy))
        cost[D] = (L.vlfm_object_cloud_launch_count() - launches, opm.SYNCS[0] - syncs)
        assert len(out) == D and all(len(c) > 0 for _, c, _ in out)
    # pack + 3 erosions + statistics; expansion; adjacency + clusters.  One read-back for the counts, one for the chunk
    assert cost[2] == cost[16] == (8, 2), cost
    # one detection alone ("erosion 3") is a batch of one job and costs exactly what every batch costs
    m = opm.ObjectPointCloudMap(erosion_size=3, device=gpu_device)
    launches, syncs = L.vlfm_object_cloud_launch_count(), opm.SYNCS[0]
    assert len(m._extract_object_cloud(depth[0], specs[8][1], MIN_DEPTH, MAX_DEPTH, fx, fy)) > 0
    assert (L.vlfm_object_cloud_launch_count() - launches, opm.SYNCS[0] - syncs) == (8, 2) == cost[2] == cost[16]
