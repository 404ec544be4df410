"""-m gpu: multi-prompt BLIP-2 scoring and ITMPolicyV3 in the batched harness.

1. the T-prompt ITC head against the single head (bit for bit) and an f64 restatement;
2. ``cosine_prompts_batch``: one vision forward, columns equal to ``cosine_batch`` per prompt, graph replay;
3. ``ITMPolicyV3Step`` with the in-process client (one forward per camera and step) against a twin whose client only has
   ``cosine`` (two forwards);
4. the batched V3 step (stub / eager BLIP-2 / graphed BLIP-2) against the oracle: two-channel maps, [M, 2] frontier
   medians, goals, with both branches of the reducer taken;
5. the same through a camera rig;  6. ``render()`` with V3's visual reducer;  7. the default path, untouched;
8. the reference's own ITMPolicyV3 episode (tests/golden/policy_hm3d_v3.npz) through ``ITMPolicyV3Step``."""
import copy
import ctypes
import sys

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR, dense, replay_policy_episode, sha, unpack_plane
from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

if GOLDEN_DIR not in sys.path:
    sys.path.insert(0, GOLDEN_DIR)

pytestmark = pytest.mark.gpu

V3_PROMPT = "Seems like there is a target_object ahead.|There is a lot of area to explore ahead."
# Chosen by running THE ORACLE alone (RefObstacleMap + RefValueMap(2) on the stub harness's frames and U(0.15, 0.45)
# cosines, slots 0 / 7 / 15, steps 150-209): the best target-channel median of a step lies in 0.378 .. 0.428 there, so the
# stub range's midpoint 0.30 never takes the exploration branch (0 / 180); 0.40 takes it in 99 and the target branch in 81
# of the 180 environment-steps.
THRESH = 0.40
E = 16
SLOTS = (0, 7, 15)
KW = dict(min_height=0.61, max_height=0.88, agent_radius=0.18, area_thresh=1.5)


@pytest.fixture(scope="module")
def blip2(gpu_device):
    """The in-process client's model (random-init ViT-g + Q-Former), shared by every test of this file."""
    from vlfm_amd.vlm.blip2itm import BLIP2ITMClient

    torch.manual_seed(0)
    return BLIP2ITMClient(device=gpu_device, allow_random_init=True)._model


class _CountForwards:
    """Counts the calls of ``model.vision_tokens`` while active."""

    def __init__(self, blip2):
        self.model, self.n = blip2.model, 0

    def __enter__(self):
        inner = self.model.vision_tokens

        def counted(*a, **k):
            self.n += 1
            return inner(*a, **k)

        self.model.vision_tokens = counted
        return self

    def __exit__(self, *exc):
        del self.model.vision_tokens      # (the instance attribute: the class's method is back)


def _reduce(values, thresh):
    """Test-local restatement of ITMPolicyV3._reduce_values (itm_policy.py:296-316) on an [M, 2] array -> ([M], channel)."""
    values = np.asarray(values, np.float64).reshape(-1, 2)
    use = 1 if values[:, 0].max() < thresh else 0
    return values[:, use], use


def _choose(selector, pts, values, thresh, robot_xy):
    reduced, use = _reduce(values, thresh)
    order = np.argsort([-v for v in reduced])                    # value_map.py:183
    goal, _ = selector.choose(pts[order], [float(v) for v in reduced[order]], pts, robot_xy)
    return goal, use


def _oracle_values(vm, pts):
    """The [M, 2] disc medians the oracle's sort_waypoints hands to its reduce_fn."""
    rec = []
    vm.sort_waypoints(pts, 0.5, reduce_fn=lambda v: (rec.append(np.asarray(v, np.float64).reshape(-1, 2)), [x[0] for x in v])[1])
    return rec[0]


# ------------------------------------------------------------------------------------------------ 1. the head kernel
@pytest.mark.parametrize("B", [1, 8, 256])
def test_itc_head_multi_equals_single_head_bit_for_bit(gpu_device, B):
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(100 + B)
    NQ, H, P = 32, 768, 256
    q = torch.randn(B, NQ, H, generator=g)
    w = torch.randn(P, H, generator=g) * 0.05
    b = torch.randn(P, generator=g) * 0.1
    d = lambda t: t.contiguous().to(gpu_device)   # noqa: E731
    qd, wd, bd = d(q), d(w.t()), d(b)
    proj64 = q.double().numpy() @ w.double().numpy().T + b.double().numpy()
    for T in (1, 2, 5):
        for U in (1, 3, 11):
            table = torch.nn.functional.normalize(torch.randn(U, P, generator=g), dim=-1)
            idx = torch.randint(0, U, (B, T), generator=g)
            idx[0] = torch.arange(T) % U                      # repeated (T > U) and, below, permuted rows
            if B > 1:
                idx[1] = (U - 1 - torch.arange(T)) % U
            index = ops.itc_text_index(idx.tolist(), U, gpu_device)
            got = ops.itc_head_multi(qd, wd, bd, d(table), index)
            assert got.shape == (B, T) and got.dtype == torch.float32
            for t in range(T):
                single = ops.itc_head(qd, wd, bd, d(table[idx[:, t]]))
                assert torch.equal(got[:, t], single), (B, T, U, t, float((got[:, t] - single).abs().max()))
            # f64 NumPy restatement, the bound test_itc_head_vs_fp32_reference grants the single head
            text = table.double().numpy()[idx.numpy()]                                      # [B,T,P]
            nrm = np.maximum(np.linalg.norm(proj64, axis=-1, keepdims=True), 1e-12)
            want = np.einsum("bqp,btp->btq", proj64 / nrm, text).max(-1)
            assert np.abs(got.cpu().numpy() - want).max() <= 2e-5, (B, T, U, np.abs(got.cpu().numpy() - want).max())


def test_itc_head_multi_zero_row_and_refused_arguments(gpu_device):
    from vlfm_amd import _lib
    from vlfm_amd.vlm import ops

    g = torch.Generator().manual_seed(7)
    B, NQ, H, P, U, T = 3, 32, 768, 256, 4, 2
    q = torch.randn(B, NQ, H, generator=g)
    q[1] = 0.0                                       # with a zero bias: all-zero projected rows -> the 1e-12 clamp
    w = (torch.randn(P, H, generator=g) * 0.05).t().contiguous().to(gpu_device)
    bias = torch.zeros(P, device=gpu_device)
    table = torch.nn.functional.normalize(torch.randn(U, P, generator=g), dim=-1).to(gpu_device)
    index = ops.itc_text_index([[0, 1], [2, 3], [3, 0]], U, gpu_device)
    got = ops.itc_head_multi(q.to(gpu_device), w, bias, table, index)
    assert torch.equal(got[1], torch.zeros(T, device=gpu_device)) and torch.isfinite(got).all()
    for t in range(T):
        assert torch.equal(got[:, t], ops.itc_head(q.to(gpu_device), w, bias, table[index[:, t].long()].contiguous()))
    # an out-of-range index is refused by the wrapper that builds the index tensor, before any launch
    for rows in ([[0, U]], [[-1, 0]]):
        with pytest.raises(ValueError):
            ops.itc_text_index(rows, U, gpu_device)
    # what the C entry point refuses comes back as its error code, an exception through _lib.check
    L = _lib.lib()
    proj = torch.zeros(B, NQ, P, device=gpu_device)
    wide = torch.zeros(B, 65, P, device=gpu_device)
    out = torch.zeros(B, 9, device=gpu_device)
    idx9 = torch.zeros(B, 9, dtype=torch.int32, device=gpu_device)
    ok = (proj.data_ptr(), B, NQ, P, table.data_ptr(), U, idx9.data_ptr(), T, out.data_ptr(), None)
    bad = {"T = 0": {7: 0}, "T above the bound": {7: ops.ITC_MAX_PROMPTS + 1}, "NQ > 64": {0: wide.data_ptr(), 2: 65},
           "U = 0": {5: 0}, "null proj": {0: None}, "null table": {4: None}, "null index": {6: None}, "null out": {8: None}}
    for what, change in bad.items():
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        rc = L.vlfm_itc_head_multi(*args)
        assert rc == _lib.VLFM_ERR_INVALID, what
        with pytest.raises(RuntimeError, match="itc_head_multi"):
            _lib.check(rc, "itc_head_multi")
    assert L.vlfm_itc_head_multi(*ok) == 0
    torch.cuda.synchronize()
    assert ctypes.c_int(ops.ITC_MAX_PROMPTS).value == 8


# ------------------------------------------------------------------------------------------------ 2. one forward
@pytest.mark.parametrize("B", [1, 8, 64])
def test_cosine_prompts_batch_is_one_forward_and_equals_cosine_batch(gpu_device, blip2, B):
    g = torch.Generator().manual_seed(B)
    images = torch.randint(0, 256, (B, 480, 640, 3), generator=g, dtype=torch.uint8).to(gpu_device)
    targets = ["chair", "bed", "potted plant", "toilet", "tv", "couch"]
    p0 = [f"Seems like there is a {targets[i % 6]} ahead." for i in range(B)]
    p1 = ["There is a lot of area to explore ahead."] * B
    a, b = blip2.cosine_batch(images, p0).clone(), blip2.cosine_batch(images, p0).clone()
    d0 = float((a - b).abs().max())
    print(f"\nrun-to-run difference of cosine_batch at batch {B}: d0 = {d0!r}")
    with _CountForwards(blip2) as one:
        blip2.cosine_batch(images, p0)
    with _CountForwards(blip2) as multi:
        got = blip2.cosine_prompts_batch(images, [[x, y] for x, y in zip(p0, p1)]).clone()
    assert multi.n == one.n >= 1, (multi.n, one.n)
    assert got.shape == (B, 2) and got.dtype == torch.float32 and got.is_cuda
    for t, per in enumerate((p0, p1)):
        want = blip2.cosine_batch(images, per)
        if d0 == 0.0:
            assert torch.equal(got[:, t], want), (B, t, float((got[:, t] - want).abs().max()))
        else:
            assert float((got[:, t] - want).abs().max()) <= d0, (B, t, float((got[:, t] - want).abs().max()), d0)
    # one list shared by all images
    shared = blip2.cosine_prompts_batch(images, [p0[0], p1[0]])
    want = blip2.cosine_batch(images, [p0[0]])
    assert shared.shape == (B, 2)
    assert torch.equal(shared[:, 0], want) if d0 == 0.0 else float((shared[:, 0] - want).abs().max()) <= d0
    # steady state uploads nothing: the table and the index of a prompt structure are built once
    per = [[x, y] for x, y in zip(p0, p1)]
    assert blip2._prompt_tensors(per, B)[1] is blip2._prompt_tensors([list(p) for p in per], B)[1]
    # graph replay against eager: the 5e-3 test_harness_gpu.py grants graph against eager
    graphed = blip2.cosine_prompts_batch_graphed(images, per).clone()
    again = blip2.cosine_prompts_batch_graphed(images, per)
    assert float((graphed - got).abs().max()) <= 5e-3 and float((again - got).abs().max()) <= 5e-3
    assert torch.isfinite(got).all()


# ------------------------------------------------------------------------------------------------ 3. single environment
def test_v3_step_one_forward_per_camera_against_a_cosine_only_twin(gpu_device, blip2):
    import make_golden_v3 as mg3
    import policy_script as ps
    from golden_util import load
    from vlfm_amd.policy_step import ITMPolicyV3Step
    from vlfm_amd.vlm.blip2itm import BLIP2ITMClient
    from vlfm_amd.vlm.detections import ObjectDetections

    mg3.register()
    g = load(mg3.NAME)
    client = BLIP2ITMClient(device=gpu_device, allow_random_init=True)
    assert client._model is blip2

    class CosineOnly:
        def cosine(self, image, txt):
            return client.cosine(image, txt)

    image = np.random.Generator(np.random.PCG64(3)).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    d0 = abs(client.cosine(image, "a") - client.cosine(image, "a"))

    def make(itm):
        vlm = ps.ScriptedVLM(mg3.NAME, ObjectDetections)
        pol = ITMPolicyV3Step(THRESH, camera_height=0.88, min_depth=0.5, max_depth=5.0, camera_fov=79.0, image_width=ps.W,
                              text_prompt=V3_PROMPT, itm=itm, coco_detector=vlm.coco, detector=vlm.gdino, sam=vlm.sam)
        pol.reset("toilet")
        return pol

    one, twin = make(client), make(CosineOnly())
    worlds = [ps.ScriptedWorld(mg3.NAME, recorded=(g["pose"], g["wall"])) for _ in range(2)]
    goals = 0
    for k in range(30):
        results = []
        for pol, world, forwards in ((one, worlds[0], 1), (twin, worlds[1], 2)):
            _, rgb, depth, x, y, yaw = world.observe()
            with _CountForwards(blip2) as n:
                results.append(pol.step(rgb, depth, x, y, yaw))
            assert n.n == forwards, (k, n.n, forwards)
            world.advance(results[-1].mode, results[-1].rho, results[-1].theta)
        a, b = results
        assert a.mode == b.mode and np.array_equal(a.frontiers, b.frontiers), k
        assert (a.goal is None) == (b.goal is None) and (a.goal is None or np.array_equal(a.goal, b.goal)), (k, d0)
        goals += a.goal is not None
        va, vb = one.maps()[1], twin.maps()[1]
        assert np.array_equal(va._map, vb._map), k
        if d0 == 0.0:
            assert np.array_equal(va._value_map, vb._value_map), (k, np.abs(va._value_map - vb._value_map).max())
        else:
            assert np.abs(va._value_map - vb._value_map).max() <= d0, (k, d0)
    assert goals >= 10 and one.maps()[1]._value_map.shape[-1] == 2


# ------------------------------------------------------------------------------------------------ 4. batched V3, oracle
class _Follower:
    """The oracle side of one harness: reference obstacle maps (shared: every harness sees the same frames), reference
    two-channel value maps and frontier selectors for the watched slots, and the count of reducer branches."""

    def __init__(self, oms, vms):
        from vlfm_amd.policy_step import FrontierSelector

        self.oms, self.vms = oms, vms
        self.selectors = {e: FrontierSelector() for e in SLOTS}
        self.branches = [0, 0]

    def step_values(self, depth, cos, tf, fov):
        for e in SLOTS:
            self.vms[e].update_map(cos[e], depth[e].copy(), tf[e], MIN_DEPTH, MAX_DEPTH, fov)

    def compare(self, sim, where, poses=None):
        conf, value = sim.values.conf.cpu().numpy(), sim.values.value.cpu().numpy()
        wps, env_of = sim.obstacles.frontier_list()
        fr = sim.obstacles.frontiers_px()
        assert value.shape[-1] == 2 and value.dtype == np.float64 and conf.dtype == np.float32
        for e in SLOTS:
            om, vm = self.oms[e], self.vms[e]
            want_px = np.asarray(om._frontiers_px, np.float64).reshape(-1, 2)
            assert np.array_equal(fr[e].reshape(-1, 2), want_px), (where, e, "frontier pixels")
            assert np.array_equal(conf[e], vm._map), (where, e, "confidence map", np.abs(conf[e] - vm._map).max())
            assert np.array_equal(value[e], vm._value_map), (where, e, "value map", np.abs(value[e] - vm._value_map).max())
            if not len(want_px):
                continue
            got = np.asarray(sim.last_frontier_values, np.float64)
            assert got.ndim == 2 and got.shape[1] == 2, (where, got.shape)
            pts = wps[env_of == e]
            assert np.array_equal(pts, np.asarray(om.frontiers, np.float64).reshape(-1, 2)), (where, e)
            want = _oracle_values(vm, pts)
            assert np.array_equal(got[env_of == e], want), (where, e, "frontier medians [M, 2]")
            if poses is not None:      # a deciding step (explore mode for every environment: episode step >= 12, no object maps)
                assert sim.last_modes[e] == "explore", (where, e)
                goal, use = _choose(self.selectors[e], pts, want, THRESH, poses[e, :2])
                self.branches[use] += 1
                assert np.array_equal(sim.last_goals[e], goal), (where, e, "goal", sim.last_goals[e], goal, use)


def test_batched_v3_step_against_the_oracle(gpu_device, blip2):
    from oracle.ref_obstacle_map import RefObstacleMap
    from oracle.ref_value_map import RefValueMap
    from vlfm_amd.harness import BatchedEpisodes

    fx, fy, fov = camera_intrinsics(640)
    FF, STEPS = 150, 60
    common = dict(device=gpu_device, world="rooms", episode_len=500, overlap=True, select_frontiers=True,
                  text_prompt=V3_PROMPT, exploration_thresh=THRESH)
    sims = {
        "stub cosines": BatchedEpisodes(E, use_blip2=False, **common),
        "BLIP-2 cosine_prompts_batch": BatchedEpisodes(E, blip2=blip2, graph_blip2=False, **common),
        "BLIP-2 from a HIP graph": BatchedEpisodes(E, blip2=blip2, graph_blip2=True, **common),
    }
    names = list(sims)
    for sim in sims.values():
        assert sim.C == 2 and sim.values.channels == 2 and len(sim.prompts) == E and len(sim.prompts[0]) == 2
    oms = {e: RefObstacleMap(**KW) for e in SLOTS}
    stub = _Follower(oms, {e: RefValueMap(2, use_max_confidence=False) for e in SLOTS})
    followers = {}

    def advance(fast: bool, where: str):
        t = sims[names[0]].t % 500
        depth = sims[names[0]].rooms.frame(t).cpu().numpy()
        tf = sims[names[0]].tf_table[t]
        for e in SLOTS:
            oms[e].update_map(depth[e].copy(), tf[e], MIN_DEPTH, MAX_DEPTH, fx, fy, fov)
        fed = set()
        for n in names:
            sim = sims[n]
            assert sim.t % 500 == t and torch.equal(sim.rooms.frame(t), sims[names[0]].rooms.frame(t))
            if fast:
                sim.fast_forward(1)
            else:
                sim.step()
            torch.cuda.synchronize()
            assert tuple(sim.last_cosines.shape) == (E, 2), (where, n, tuple(sim.last_cosines.shape))
            cos = sim.last_cosines.double().cpu().numpy()
            f = followers.get(n, stub)
            if id(f) not in fed:
                f.step_values(depth, cos, tf, fov)
                f.last_cos = cos
                fed.add(id(f))
            assert np.array_equal(cos, f.last_cos), (where, n, "harnesses sharing a follower must feed the same cosines")
        return t

    for i in range(FF):
        advance(True, f"fast-forward step {i}")
        if i % 25 == 24 or i == FF - 1:
            for n in names:
                stub.compare(sims[n], f"{n}: fast-forward step {i}")
    for n in names[1:]:
        followers[n] = _Follower(oms, {e: copy.deepcopy(stub.vms[e]) for e in SLOTS})
    for i in range(STEPS):          # no step is excluded
        t = advance(False, f"step {FF + i}")
        for n in names:
            followers.get(n, stub).compare(sims[n], f"{n}: step {FF + i} (episode step {t})", sims[n].pose_table[t])
    for n in names:
        sims[n].check()
    # both branches of the reducer, counted from THE ORACLE's values over the stub harness's explore-mode environment-steps
    target, explore = stub.branches
    total = target + explore
    assert total == STEPS * len(SLOTS), (target, explore)
    assert min(target, explore) >= 0.1 * total, \
        f"reducer branches over {total} explore-mode environment-steps: target channel {target}, exploration channel {explore}"
    print(f"\nreducer branches (stub harness, oracle's values): target {target}, exploration {explore}; "
          f"BLIP-2 eager {followers[names[1]].branches}, graphed {followers[names[2]].branches}")
    real, g = followers[names[1]].last_cos, followers[names[2]].last_cos
    assert np.isfinite(real).all() and not np.array_equal(real, stub.last_cos)
    assert np.abs(g - real).max() <= 5e-3, np.abs(g - real).max()


# ------------------------------------------------------------------------------------------------ 5. rig
def test_batched_v3_rig_step_against_the_camera_by_camera_oracle(gpu_device):
    from oracle.ref_value_map import RefValueMap
    from vlfm_amd.harness import BatchedEpisodes, Camera, CameraRig
    from vlfm_amd.mapping import ObstacleMap
    from vlfm_amd.policy_step import FrontierSelector

    rig = CameraRig([Camera(yaw=0.5, max_depth=3.5), Camera(yaw=-0.5, forward=0.1, hfov=float(np.deg2rad(60.0))),
                     Camera(yaw=np.pi, left=0.1, value=False, max_depth=2.5)])
    sim = BatchedEpisodes(8, device=gpu_device, use_blip2=False, rig=rig, episode_len=500, select_frontiers=True,
                          text_prompt=V3_PROMPT, exploration_thresh=THRESH)
    fov0 = camera_intrinsics(640)[2]
    hfov = [fov0 if c.hfov is None else c.hfov for c in rig.cameras]
    fx = [640 / (2 * np.tan(h / 2)) for h in hfov]
    watch = (0, 3, 7)
    oms = {e: ObstacleMap(device=gpu_device, **KW) for e in watch}     # (the drop-in map: pinned to the reference elsewhere)
    vms = {e: RefValueMap(2, use_max_confidence=False) for e in watch}
    selectors = {e: FrontierSelector() for e in watch}
    decided, branches = 0, [0, 0]
    for step in range(40):
        t = sim.t % 500
        sim.step()
        torch.cuda.synchronize()
        depth, tf, slot, cam = sim.last_rig
        depth, cos = depth.cpu().numpy(), sim.last_cosines.double().cpu().numpy()
        v_rows = [i for i in range(len(slot)) if rig.cameras[cam[i]].value]
        assert cos.shape == (len(v_rows), 2) == (16, 2)
        conf, value = sim.values.conf.cpu().numpy(), sim.values.value.cpu().numpy()
        wps, env_of = sim.obstacles.frontier_list()
        for e in watch:
            mine = [i for i in range(len(slot)) if slot[i] == e]
            for i in mine:
                c = rig.cameras[cam[i]]
                if c.obstacle:
                    oms[e].update_map(depth[i], tf[i], c.min_depth, c.max_depth, fx[cam[i]], fx[cam[i]], hfov[cam[i]], explore=False)
            oms[e].update_map(None, sim.tf_table[t][e], MIN_DEPTH, 5.0, fx[0], fx[0], max(hfov), explore=True, update_obstacles=False)
            for i in mine:
                c = rig.cameras[cam[i]]
                if c.value:
                    vms[e].update_map(cos[v_rows.index(i)], depth[i].copy(), tf[i], c.min_depth, c.max_depth, hfov[cam[i]])
            assert np.array_equal(conf[e], vms[e]._map), (step, e, "conf")
            assert np.array_equal(value[e], vms[e]._value_map), (step, e, "value", np.abs(value[e] - vms[e]._value_map).max())
            pts = np.asarray(oms[e].frontiers, np.float64).reshape(-1, 2)
            if sim.last_modes[e] == "explore" and len(pts) and not np.array_equal(pts, np.zeros((1, 2))):
                assert np.array_equal(wps[env_of == e], pts), (step, e)
                want = _oracle_values(vms[e], pts)
                assert np.array_equal(np.asarray(sim.last_frontier_values)[env_of == e], want), (step, e, "medians")
                goal, use = _choose(selectors[e], pts, want, THRESH, sim.pose_table[t][e, :2])
                assert np.array_equal(sim.last_goals[e], goal), (step, e, "goal")
                decided += 1
                branches[use] += 1
    sim.check()
    # (the goals above were checked on BOTH branches of the reducer, not on one only)
    assert decided >= 30 and min(branches) >= 1, f"decided {decided}: target channel {branches[0]}, exploration channel {branches[1]}"


# ------------------------------------------------------------------------------------------------ 6. render
def test_harness_render_uses_the_explore_reducer(gpu_device):
    import map_render_ref as R
    from vlfm_amd.harness import BatchedEpisodes

    thresh = 0.3
    sim = BatchedEpisodes(3, device=gpu_device, use_blip2=False, world="rooms", episode_len=500, render_trajectories=True,
                          text_prompt=V3_PROMPT, exploration_thresh=thresh)
    for _ in range(6):
        sim.step()
    frames = sim.render([2, 0])
    torch.cuda.synchronize()
    vals = sim.values.value.cpu().numpy()
    assert vals.shape[-1] == 2
    above = 0
    for k, e in enumerate((2, 0)):
        pos = [sim.pose_table[t][e, :2] for t in range(6)]
        yaw = sim.pose_table[5][e, 2]
        v = vals[e].astype(sim.values.value_dtype(e))
        above += int((v[:, :, 0] > thresh).sum())
        want = R.render_value(R.explore_reduce(thresh)(v), None, pos, yaw)
        assert np.array_equal(frames["value_map"][k].cpu().numpy(), want[..., ::-1]), e
    assert above > 0


# ------------------------------------------------------------------------------------------------ 7. default path
def test_default_harness_is_untouched_by_the_new_arguments(gpu_device):
    from vlfm_amd.harness import PROMPT, BatchedEpisodes

    a = BatchedEpisodes(4, device=gpu_device, use_blip2=False, episode_len=500, select_frontiers=True)
    b = BatchedEpisodes(4, device=gpu_device, use_blip2=False, episode_len=500, select_frontiers=True, text_prompt=PROMPT)
    for sim in (a, b):
        assert sim.C == 1 and sim.exploration_thresh is None and sim.values.channels == 1
        assert sim.prompts == [f"Seems like there is a {t} ahead." for t in ("chair", "bed", "potted plant", "toilet")]
    for step in range(20):
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert tuple(a.last_cosines.shape) == (4,) and torch.equal(a.last_cosines, b.last_cosines), step
        assert torch.equal(a.values.conf, b.values.conf) and torch.equal(a.values.value, b.values.value), step
        assert np.array_equal(a.last_frontier_values, b.last_frontier_values), step
        assert np.array_equal(a.last_goals, b.last_goals, equal_nan=True), step
    assert a.values.value.shape[-1] == 1


# ------------------------------------------------------------------------------------------------ 8. the V3 fixture
def test_v3_episode_matches_the_references_itm_policy_v3(gpu_device, monkeypatch):
    import make_golden_v3 as mg3
    import policy_script as ps
    from vlfm_amd.policy_step import ITMPolicyV3Step
    from vlfm_amd.vlm.detections import ObjectDetections

    mg3.register()
    monkeypatch.setattr(ps, "ScriptedVLM", mg3.ScriptedVLMV3)      # cosines keyed on (step, prompt), a ``cosine``-only client

    def make(vlm, **kw):
        return ITMPolicyV3Step(mg3.EXPLORATION_THRESH, itm=vlm.itm, coco_detector=vlm.coco, detector=vlm.gdino, sam=vlm.sam,
                               text_prompt=mg3.TEXT_PROMPT, **kw)

    pol, g = replay_policy_episode(mg3.NAME, make, ObjectDetections, tol=0.0)
    obstacle, value, _ = pol.maps()
    conf = dense(g["conf_idx"], g["conf_val"], (1000, 1000), np.float32)
    assert np.array_equal(value._map, conf), np.abs(value._map - conf).max()
    val = np.zeros((10 ** 6, 2), np.float32)
    val[g["conf_idx"]] = g["v3_value_val"]                      # the fixture keeps the f64 map rounded to f32
    got = np.asarray(value._value_map)
    assert got.shape == (1000, 1000, 2)
    assert np.array_equal(got.astype(np.float32).reshape(-1, 2), val), np.abs(got.reshape(-1, 2) - val).max()
    assert sha(np.asarray(got, np.float64)) == str(g["v3_value_sha"])      # ... and the exact f64 map, by its digest
    assert np.array_equal(obstacle.explored_area.astype(bool), unpack_plane(g["explored"]))
    assert np.array_equal(obstacle._map.astype(bool), unpack_plane(g["obstacles"]))
