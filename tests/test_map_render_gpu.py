"""The device renderer (csrc/map_render.hip) bit-equal to the NumPy renderer of tests/map_render_ref.py, which
tests/test_map_render_cpu.py pins to the reference's own visualize() on the same seeded states: batched value and obstacle
renders over several slots and slot subsets, the drop-in visualize() along mapped sessions, incremental trajectories,
slot independence and reset."""
import numpy as np
import pytest

import map_render_ref as R

pytestmark = pytest.mark.gpu


def _pack(planes: np.ndarray):
    """[n,S,S] bool -> [n,S,ceil(S/32)] int32 bit-planes (bit x of a row in word x >> 5) on cuda:0."""
    import torch

    n, S, _ = planes.shape
    W = (S + 31) // 32
    pad = np.zeros((n, S, W * 32), np.uint8)
    pad[:, :, :S] = planes
    words = np.packbits(pad.reshape(n, S, W, 32), axis=-1, bitorder="little").view("<u4").reshape(n, S, W)
    return torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")


def _markers_rows(slot, markers):
    return [[slot, x, y, r, t, *c] for x, y, r, t, c in markers]


@pytest.mark.parametrize("seed", range(16))
def test_value_batch_render_equals_numpy_renderer(gpu_device, seed):
    import torch

    from vlfm_amd.mapping.value_map import ValueMapBatch

    st = R.random_value_state(seed)
    S, C, f32 = st["size"], st["channels"], st["value"].dtype == np.float32
    b = ValueMapBatch(3, C, S, use_max_confidence=f32, device=gpu_device)
    b.n_updates[:] = 1
    rng = np.random.default_rng(seed)
    values, explored, rows, want = [], [], [], {}
    for slot in range(3):
        v = st["value"] if slot == 1 else (st["value"] * (slot + 1)).astype(st["value"].dtype)
        values.append(v.astype(np.float64))
        ex = st["explored"] if st["explored"] is not None else np.ones((S, S), bool)
        if slot == 2:
            ex = rng.uniform(0, 1, (S, S)) < 0.5
        explored.append(ex)
        pos = [p + slot * 0.7 for p in st["positions"]] if slot != 0 else st["positions"][:2]
        if pos:
            b.update_agent_traj([slot] * len(pos), pos, [st["yaw"]] * len(pos))
        mk = R.pixel_markers(st["markers"], S)
        mk = mk[slot:] if slot else mk
        rows += _markers_rows(slot, mk)
        want[slot] = R.render_value(st["reduce_fn"](v), ex, pos, st["yaw"], mk)
    b.value.copy_(torch.from_numpy(np.stack(values)).to(gpu_device))
    b.explored_bits = _pack(np.stack(explored))
    reduce = ("explore", st["thresh"]) if C == 2 else "max"
    got = b.render([2, 1], reduce=reduce, markers=np.array(rows).reshape(-1, 8)).cpu().numpy()
    assert np.array_equal(got[0], want[2]) and np.array_equal(got[1], want[1]), seed
    rgb = b.render([0], reduce=reduce, markers=np.array(rows).reshape(-1, 8), rgb=True).cpu().numpy()[0]
    assert np.array_equal(rgb, want[0][..., ::-1])
    # a host-reduced plane (any other reduce_fn) in the reference array's dtype
    plane = np.stack([(R.max_reduce(v) - 0.25).astype(st["value"].dtype) for v in values[1:]])
    got = b.render([1, 2], reduce=plane, markers=np.array(rows).reshape(-1, 8), explored=None).cpu().numpy()
    for k, slot in enumerate((1, 2)):
        pos = [p + slot * 0.7 for p in st["positions"]]
        mk = R.pixel_markers(st["markers"], S)[slot:]
        assert np.array_equal(got[k], R.render_value(plane[k], None, pos, st["yaw"], mk)), (seed, slot)


@pytest.mark.parametrize("seed", range(8))
def test_obstacle_batch_render_equals_numpy_renderer(gpu_device, seed):
    from vlfm_amd.mapping.obstacle_map import ObstacleMapBatch

    st = R.random_obstacle_state(seed)
    S = st["size"]
    b = ObstacleMapBatch(2, 0.61, 0.88, 0.18, size=S, device=gpu_device)
    planes = {"obstacle": [], "navigable": [], "explored": []}
    want = []
    for slot in range(2):
        for k in planes:
            planes[k].append(st[k] if slot == 0 else st[k][::-1, ::-1].copy())
        fr = st["frontiers"] if slot == 0 else st["frontiers"][:2]
        pos = st["positions"] if slot == 0 else [p[::-1] for p in st["positions"]]
        if pos:
            b.update_agent_traj([slot] * len(pos), pos, [st["yaw"]] * len(pos))
        want.append(R.render_obstacle(planes["obstacle"][slot], planes["navigable"][slot], planes["explored"][slot], fr,
                                      pos, st["yaw"]))
    b.obstacle_bits.copy_(_pack(np.stack(planes["obstacle"])))
    b.navigable_bits.copy_(_pack(np.stack(planes["navigable"])))
    b.explored_bits.copy_(_pack(np.stack(planes["explored"])))
    got = b.render([1, 0], [st["frontiers"][:2], st["frontiers"]]).cpu().numpy()
    assert np.array_equal(got[0], want[1]) and np.array_equal(got[1], want[0]), seed
    b.reset([0])   # reset clears the slot's planes and its trajectory, the other slot keeps both
    b.obstacle_bits[1:].copy_(_pack(np.stack(planes["obstacle"][1:])))
    got = b.render([0, 1], [np.zeros((0, 2)), st["frontiers"][:2]]).cpu().numpy()
    z = np.zeros((S, S), bool)
    assert np.array_equal(got[0], R.render_obstacle(z, z, z, np.zeros((0, 2))))
    assert np.array_equal(got[1], want[1])


def _session(vm, om, steps, on_step=None, seed=3):
    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, SyntheticEnv, camera_intrinsics

    fx, fy, fov = camera_intrinsics(640)
    env = SyntheticEnv(seed)
    for k in range(steps):
        depth, tf, values = env.observe()
        om.update_map(depth, tf, MIN_DEPTH, MAX_DEPTH, fx, fy, fov)
        vm.update_map(values, depth, tf, MIN_DEPTH, MAX_DEPTH, fov)
        xy, yaw = tf[:2, 3].copy(), float(np.arctan2(tf[1, 0], tf[0, 0]))
        vm.update_agent_traj(xy, yaw)
        om.update_agent_traj(xy, yaw)
        if on_step is not None:
            on_step(k)


def _expected(vm, om, markers):
    S = vm.size
    value = R.render_value(np.max(vm._value_map, axis=-1), om.explored_area, vm._camera_positions, vm._last_camera_yaw,
                           R.pixel_markers(markers, S))
    obst = R.render_obstacle(om._map, om._navigable_map, om.explored_area, om._frontiers_px, om._camera_positions,
                             om._last_camera_yaw)
    return value, obst


@pytest.mark.parametrize("use_max_confidence", [False, True])
def test_dropin_visualize_along_a_session_incremental_and_reset(gpu_device, use_max_confidence):
    from vlfm_amd.mapping import ObstacleMap, ValueMap

    kw = dict(min_height=0.61, max_height=0.88, agent_radius=0.18, area_thresh=1.5)
    vm, om = ValueMap(1, use_max_confidence=use_max_confidence, device=gpu_device), ObstacleMap(device=gpu_device, **kw)
    vm2, om2 = ValueMap(1, use_max_confidence=use_max_confidence, device=gpu_device), ObstacleMap(device=gpu_device, **kw)

    def markers():
        mk = [(f[:2], {"radius": 5, "thickness": 2, "color": (0, 0, 255)}) for f in np.asarray(om.frontiers).reshape(-1, 2)]
        if len(mk):
            mk.append((mk[0][0], {"radius": 5, "thickness": 2, "color": (0, 255, 255)}))
        return mk

    def every_step(k):
        mk = markers()
        want_v, want_o = _expected(vm, om, mk)
        assert np.array_equal(vm.visualize(mk, obstacle_map=om), want_v), k
        assert np.array_equal(om.visualize(), want_o), k

    for episode in range(2):
        _session(vm, om, 6, every_step, seed=3 + episode)
        _session(vm2, om2, 6, seed=3 + episode)   # visualised once, at the end: same images
        mk = markers()
        assert np.array_equal(vm2.visualize(mk, obstacle_map=om2), vm.visualize(mk, obstacle_map=om))
        assert np.array_equal(om2.visualize(), om.visualize())
        # a host reduce_fn (uploaded plane) equals the device reducer's image when it computes the same plane
        assert np.array_equal(vm.visualize(mk, reduce_fn=lambda a: np.max(a, axis=-1) + 0, obstacle_map=om),
                              vm.visualize(mk, obstacle_map=om))
        for m in (vm, om, vm2, om2):
            m.reset()
        blank = vm.visualize()
        assert (blank == 255).all()             # reset cleared map and trajectory: an all-white image


@pytest.mark.parametrize("use_max_confidence", [False, True])
def test_dropin_visualize_equals_recorded_reference_session(gpu_device, use_max_confidence):
    """End to end against the reference: the drop-in ValueMap / ObstacleMap through the seeded session of
    map_render_ref.run_session (mapping, trajectory, reset between episodes), every step's visualize() equal to the
    digest of the image the reference's own classes produced (tests/golden/ref_map_render_session_*.json.gz)."""
    from golden_util import ReferenceRecord
    from vlfm_amd.mapping import ObstacleMap, ValueMap

    rec = ReferenceRecord(f"map_render_session_{int(use_max_confidence)}")
    rec.live = False                                  # replay the recorded images (the GPU test never reads the reference)
    vm = ValueMap(1, use_max_confidence=use_max_confidence, device=gpu_device)
    om = ObstacleMap(device=gpu_device, **R.SESSION_KW)

    def step(k):
        mk = R.frontier_markers(om.frontiers)
        want_v, want_o = rec(lambda: None)
        assert want_v.matches(vm.visualize(mk, obstacle_map=om)), ("value map", k)
        assert want_o.matches(om.visualize()), ("obstacle map", k)

    R.run_session(vm, om, step)
    rec.close()


@pytest.mark.parametrize("name", ["policy_hm3d_chair", "policy_mp3d_table", "policy_hm3d_explore"])
def test_policy_maps_along_a_policy_episode(gpu_device, name):
    """ITMPolicyV2Step.policy_maps() after a scripted episode of the reference's ITMPolicyV2 (decisions checked step by step
    by golden_util.replay_policy_episode): the RGB images _get_policy_info builds, frontier and goal markers included."""
    from golden_util import replay_policy_episode
    from vlfm_amd.policy_step import ITMPolicyV2Step
    from vlfm_amd.vlm.detections import ObjectDetections

    def make(vlm, **kw):
        return ITMPolicyV2Step(itm=vlm.itm, coco_detector=vlm.coco, detector=vlm.gdino, sam=vlm.sam, **kw)

    pol, _ = replay_policy_episode(name, make, ObjectDetections, tol=0.0)
    maps = pol.policy_maps()
    om, vm, _ = pol.maps()
    fr = np.asarray(pol._last_frontiers).reshape(-1, 2)
    mk = [(f[:2], {"radius": 5, "thickness": 2, "color": (0, 0, 255)}) for f in fr]
    goal = pol.last_goal
    if not np.array_equal(goal, np.zeros(2)):
        color = (0, 255, 255) if any(np.array_equal(goal, f) for f in fr) else (0, 255, 0)
        mk.append((goal, {"radius": 5, "thickness": 2, "color": color}))
    want_v = R.render_value(np.max(vm._value_map, axis=-1), None, vm._camera_positions, vm._last_camera_yaw,
                            R.pixel_markers(mk, vm.size))
    want_o = R.render_obstacle(om._map, om._navigable_map, om.explored_area, om._frontiers_px, om._camera_positions,
                               om._last_camera_yaw)
    assert np.array_equal(maps["value_map"], want_v[..., ::-1])
    assert np.array_equal(maps["obstacle_map"], want_o[..., ::-1])


def test_v3_policy_maps_use_the_exploration_reducer_on_the_device(gpu_device):
    from vlfm_amd.mapping.value_map import ValueMap, explore_reduce_fn

    st = R.random_value_state(6)             # two channels, f32
    S = st["size"]
    vm = ValueMap(2, size=S, use_max_confidence=True, device=gpu_device)
    import torch

    vm._batch.value[0].copy_(torch.from_numpy(st["value"].astype(np.float64)).to(gpu_device))
    for p in st["positions"]:
        vm.update_agent_traj(p, st["yaw"])
    fn = explore_reduce_fn(st["thresh"])
    got = vm.visualize(st["markers"], reduce_fn=fn)
    want = R.render_value(st["reduce_fn"](st["value"]), None, st["positions"], st["yaw"], R.pixel_markers(st["markers"], S))
    assert np.array_equal(got, want)
    assert np.array_equal(fn(st["value"]), st["reduce_fn"](st["value"]))   # the host callable computes the same plane


def test_harness_render_opt_in(gpu_device):
    from vlfm_amd.harness import BatchedEpisodes

    sim = BatchedEpisodes(3, device=gpu_device, use_blip2=False, world="rooms", episode_len=500, render_trajectories=True)
    for _ in range(6):
        sim.step()
    frames = sim.render([2, 0])
    torch_sync = __import__("torch").cuda.synchronize
    torch_sync()
    S = sim.S
    vals = sim.values.value.cpu().numpy()
    ob = sim.obstacles
    planes = [ob._unpack(t).cpu().numpy().astype(bool) for t in (ob.obstacle_bits, ob.navigable_bits, ob.explored_bits)]
    fr = ob.frontiers_px()
    for k, e in enumerate((2, 0)):
        pos = [sim.pose_table[t][e, :2] for t in range(6)]
        yaw = sim.pose_table[5][e, 2]
        want_v = R.render_value(np.max(vals[e].astype(sim.values.value_dtype(e)), axis=-1), None, pos, yaw)
        want_o = R.render_obstacle(planes[0][e], planes[1][e], planes[2][e], fr[e], pos, yaw)
        assert frames["value_map"][k].shape == (S, S, 3)
        assert np.array_equal(frames["value_map"][k].cpu().numpy(), want_v[..., ::-1]), e
        assert np.array_equal(frames["obstacle_map"][k].cpu().numpy(), want_o[..., ::-1]), e
