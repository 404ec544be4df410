"""Shared loader/replayer for the golden fixtures under tests/golden/ (generated from the reference's own source by
tests/golden/make_golden.py).  A replayer regenerates the synthetic depth frames from the stored seed and proves, via
the stored SHA-256 digests, that it feeds byte-identical inputs."""
import hashlib
import os

import numpy as np

from vlfm_amd.synthetic import SyntheticEnv

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VM_CASES = ["vm_default_c1", "vm_maxconf_c1", "vm_default_c2", "vm_replace_c1", "vm_equal_c1", "vm_default_hd"]
OM_CASES = ["om_traj", "om_holes_fill", "om_holes_all", "om_reality"]


def load(name):
    with np.load(os.path.join(GOLDEN_DIR, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dense(idx, val, shape, dtype):
    out = np.zeros(int(np.prod(shape)), dtype)
    out[idx] = val
    return out.reshape(shape)


def frames(g, channels=1, holes=False, height=480, width=640):
    """Yield (depth, tf, values) of a fixture, checking input identity."""
    env = SyntheticEnv(int(g["seed"]), height, width, holes=holes, channels=channels)
    for k in range(int(g["steps"])):
        depth, tf, values = env.observe()
        assert sha(depth) == str(g["depth_sha256"][k]), "synthetic depth differs from the fixture's input"
        assert np.array_equal(tf, g["tf"][k])
        if "values" in g:
            assert np.array_equal(values, g["values"][k])
        yield depth, tf, values


def split_frontiers(g):
    counts = g["frontier_counts"]
    offs = np.concatenate([[0], np.cumsum(counts)])
    return [g["frontiers_px"][offs[i]:offs[i + 1]] for i in range(len(counts))], \
           [g["frontiers_xy"][offs[i]:offs[i + 1]] for i in range(len(counts))]


def unpack_plane(bits, size=1000):
    return np.unpackbits(bits)[: size * size].reshape(size, size).astype(bool)


# ---------------------------------------------------------------------------------------------- policy episodes
POLICY_CASES = ["policy_hm3d_chair", "policy_mp3d_table", "policy_mp3d_cabinet", "policy_hm3d_explore", "policy_hm3d_explore_long"]


def replay_policy_episode(name, make_step, make_detections, tol=1e-4):
    """Drive a ``vlfm_amd.policy_step.ITMPolicyV2Step`` (built by ``make_step(vlm, **kwargs)``) through the scripted episode
    ``name`` and compare every step with what THE REFERENCE'S ``ITMPolicyV2`` did (tests/golden/<name>.npz).  Returns the
    step object so that the caller can compare final maps."""
    import sys

    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import policy_script as ps

    g = load(name)
    seed, steps, dataset, goal_name, caption = ps.EPISODES[name]
    vlm = ps.ScriptedVLM(name, make_detections)
    world = ps.ScriptedWorld(name, recorded=(g["pose"], g["wall"]))
    np.random.seed(777)  # ObjectPointCloudMap draws from NumPy's global RNG, as the reference does
    pol = make_step(vlm, camera_height=0.88, min_depth=0.5, max_depth=5.0, camera_fov=79.0, image_width=ps.W,
                    dataset_type=dataset, non_coco_caption=caption if dataset == "mp3d" else "")
    pol.reset(goal_name)
    offs = np.concatenate([[0], np.cumsum(g["frontier_counts"])])
    resets = 1  # the reference's counter includes the reset() of the episode start
    for k in range(steps):
        _, rgb, depth, x, y, yaw = world.observe()
        r = pol.step(rgb, depth, x, y, yaw)
        where = f"{name} step {k}"
        assert r.mode == str(g["mode"][k]), where
        assert np.array_equal(r.frontiers, g["frontiers"][offs[k]:offs[k + 1]]), where  # bit-exact frontier list
        assert np.array_equal(np.asarray(pol.last_goal, np.float64), g["nav_goal"][k]), where
        want_rt = g["rho_theta"][k]
        if np.isnan(want_rt[0]):
            assert np.isnan(r.rho), where
        else:
            assert abs(r.rho - want_rt[0]) <= 1e-9 and abs(r.theta - want_rt[1]) <= 1e-9, where
        assert pol.called_stop == bool(g["stop"][k]), where
        if np.isfinite(g["best_value"][k]):
            assert abs(r.best_value - g["best_value"][k]) <= tol, where
        else:
            assert r.best_value == g["best_value"][k], where
        assert int(pol.object_masks.sum()) == int(g["mask_px"][k]), where
        resets += int(r.pointnav_reset)
        assert resets == int(g["pointnav_resets"][k]), where
        world.advance(r.mode, r.rho, r.theta)
    assert vlm.prompts == [str(p) for p in g["prompts"]]
    assert [f"{k}:{w}" for k, w in vlm.calls] == [str(c) for c in g["calls"]]  # which model was asked, in which order
    assert (vlm.captions or [""]) == [str(c) for c in g["captions"]]
    cloud = pol.maps()[2].clouds.get(goal_name, np.zeros((0, 4)))
    assert len(cloud) == int(g["cloud_sig"][0])
    return pol, g


def replay_multicam(make_map):
    """Drive an ObstacleMap through the multi-camera script of make_golden.py (explore=False per body camera, then a reveal
    without depth) and compare with the fixture the reference produced.  Returns nothing; asserts."""
    import sys

    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import make_golden as mg

    g = load("om_multicam")
    om = make_map(hole_area_thresh=100000, min_height=0.1, max_height=1.5, agent_radius=0.2, area_thresh=1.5)
    offs = np.concatenate([[0], np.cumsum(g["frontier_counts"])])
    k = 0
    for step, (cams, tf_robot, fx, fy, fov) in enumerate(mg.multicam_script(int(g["seed"]), int(g["steps"]))):
        for depth, tf in cams:
            assert sha(depth) == str(g["depth_sha256"][k]), "synthetic depth differs from the fixture's input"
            k += 1
            om.update_map(depth, tf, 0.5, 2.5, fx, fy, fov, explore=False)
        om.update_map(None, tf_robot, 0.5, 2.5, fx, fy, 2 * fov, explore=True, update_obstacles=False)
        got = np.asarray(om.frontiers, np.float64).reshape(-1, 2)
        assert np.array_equal(got, g["frontiers_xy"][offs[step]:offs[step + 1]]), f"step {step}"
    assert np.array_equal(np.asarray(om._map).astype(bool), unpack_plane(g["obstacle_bits"]))
    assert np.array_equal(np.asarray(om._navigable_map).astype(bool), unpack_plane(g["navigable_bits"]))
    assert np.array_equal(np.asarray(om.explored_area).astype(bool), unpack_plane(g["explored_bits"]))


def replay_islands(make_map):
    """Obstacle map over make_golden.island_script(): valid texels enclosed by small depth holes are dropped together with
    the hole (fill_small_holes draws the contour filled); per-step obstacle planes, frontiers and final planes bit-exact."""
    import sys

    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import make_golden as mg
    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

    g = load("om_islands")
    fx, fy, fov = camera_intrinsics(640)
    om = make_map(hole_area_thresh=100000, **mg.OBSTACLE_KW)
    offs = np.concatenate([[0], np.cumsum(g["frontier_counts"])])
    for k, (depth, tf) in enumerate(mg.island_script()):
        assert sha(depth) == str(g["depth_sha256"][k]), "synthetic depth differs from the fixture's input"
        om.update_map(depth, tf, MIN_DEPTH, MAX_DEPTH, fx, fy, fov)
        assert np.array_equal(np.asarray(om._map).astype(bool), unpack_plane(g["obstacle_bits_per_step"][k])), f"step {k}"
        got = np.asarray(om.frontiers, np.float64).reshape(-1, 2)
        assert np.array_equal(got, g["frontiers_xy"][offs[k]:offs[k + 1]]), f"step {k}"
    assert np.array_equal(np.asarray(om._navigable_map).astype(bool), unpack_plane(g["navigable_bits"]))
    assert np.array_equal(np.asarray(om.explored_area).astype(bool), unpack_plane(g["explored_bits"]))


def replay_episode500(make_om, make_vm, steps: int = 500, on_step=None):
    """The full-length episode of tests/golden/world500.py against what THE REFERENCE'S ObstacleMap + ValueMap produced
    (tests/golden/ep500.npz), exact for the oracle and for the HIP path alike.  Every step: frontier pixels and world
    coordinates, sort_waypoints values AND permutation (value_map.py:183) bit-exact.  Steps 100 / 250 / 500: obstacle /
    navigable / explored planes bit-exact, SHA-256 of the f32 confidence map and of the f64 value map equal to the
    digests of the reference's arrays."""
    import sys

    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import make_golden as mg
    import world500 as w5
    from vlfm_amd.synthetic import MAX_DEPTH, MIN_DEPTH, camera_intrinsics

    g = load("ep500")
    fx, fy, fov = camera_intrinsics(w5.W)
    om = make_om(**mg.OBSTACLE_KW)
    vm = make_vm(1, use_max_confidence=False)
    offs = np.concatenate([[0], np.cumsum(g["frontier_counts"])])
    for i, depth, tf, values in w5.episode(g["actions"][:steps]):
        digest = np.frombuffer(hashlib.sha256(depth.tobytes()).digest()[:8], np.uint64)[0]
        assert digest == g["depth_digest"][i], "regenerated depth frame differs from the fixture's input"
        om.update_map(depth, tf, MIN_DEPTH, MAX_DEPTH, fx, fy, fov)
        vm.update_map(values, depth, tf, MIN_DEPTH, MAX_DEPTH, fov)
        want_px = g["frontiers_px"][offs[i]:offs[i + 1]]
        got_px = np.asarray(om._frontiers_px, np.float64).reshape(-1, 2)
        assert np.array_equal(got_px, want_px), f"frontier pixels differ at step {i}"
        if len(want_px):
            want_xy = np.asarray(om.frontiers, np.float64).reshape(-1, 2)
            q = want_px.copy()
            q[:, 0] = 1000 - q[:, 0]
            assert np.array_equal(want_xy, ((q - 500) / 20)[:, ::-1]), f"step {i}"  # base_map.py:48-60
            s_wp, s_val = vm.sort_waypoints(om.frontiers, 0.5)
            ref_val = g["sorted_values"][offs[i]:offs[i + 1]]
            ref_wp = want_xy[g["sorted_idx"][offs[i]:offs[i + 1]]]
            s_wp, s_val = np.asarray(s_wp), np.asarray(s_val, np.float64)
            assert np.array_equal(s_val, ref_val), (f"sort_waypoints values at step {i}", np.abs(s_val - ref_val).max())
            assert np.array_equal(s_wp, ref_wp), f"sort_waypoints permutation at step {i}"
        if on_step is not None:
            on_step(i, om, vm)
        step = i + 1
        if step in g["snapshots"]:
            for name, plane in (("obstacle", om._map), ("navigable", om._navigable_map), ("explored", om.explored_area)):
                assert np.array_equal(np.asarray(plane).astype(bool), unpack_plane(g[f"s{step}_{name}"])), \
                    f"{name} plane at step {step}"
            conf, val = np.asarray(vm._map), np.asarray(vm._value_map)
            assert conf.dtype == np.float32 and str(val.dtype) == str(g["value_dtype"])
            support = unpack_plane(g[f"s{step}_support"])
            assert np.array_equal(conf > 0, support), f"confidence support at step {step}"
            val = val.reshape(1000, 1000)
            ec = np.abs(conf[support] - g[f"s{step}_conf_q"] / 65535.0).max()   # u16-quantised copies: a readable
            ev = np.abs(val[support] - g[f"s{step}_value_q"] / 65535.0).max()   # distance should the digests differ
            assert sha(conf) == str(g[f"s{step}_conf_sha"]), (step, "confidence map digest", ec)
            assert sha(val) == str(g[f"s{step}_value_sha"]), (step, "value map digest", ev)


def replay_two_cameras(make_map):
    """One value map fed by two cameras with different (fov, max_depth) per step (make_golden.two_camera_script); exact."""
    import sys

    if GOLDEN_DIR not in sys.path:
        sys.path.insert(0, GOLDEN_DIR)
    import make_golden as mg

    g = load("vm_two_cameras")
    vm = make_map(1, use_max_confidence=False)
    k = 0
    for cams in mg.two_camera_script(int(g["seed"]), int(g["steps"])):
        for depth, tf, lo, hi, fov, values in cams:
            assert sha(depth) == str(g["depth_sha256"][k]), "synthetic depth differs from the fixture's input"
            k += 1
            vm.update_map(values, depth, tf, lo, hi, fov)
    conf = dense(g["conf_idx"], g["conf_val"], (1000, 1000), np.float32)
    assert np.array_equal(vm._map, conf)
    assert sha(np.asarray(vm._value_map, np.float64)) == str(g["value_sha"])


# ---------------------------------------------------------------------------------------------- recorded reference outputs
RECORD_ENV = "VLFM_RECORD_REFERENCE"   # =1: the differential tests write tests/golden/ref_<name>.json.gz from the live reference
_DIGEST_MIN = 4096                     # arrays with at least this many elements are stored as SHA-256 digests


def reference_present() -> bool:
    from oracle.ref_shim import REFERENCE_ROOT

    return os.path.isdir(os.path.join(REFERENCE_ROOT, "vlfm"))


class Digest:
    """A large array of the reference, as (dtype, shape, SHA-256 of its bytes)."""

    def __init__(self, dtype, shape, digest):
        self.dtype, self.shape, self.digest = np.dtype(dtype), tuple(shape), digest

    def matches(self, a) -> bool:
        a = np.asarray(a)
        return a.dtype == self.dtype and a.shape == self.shape and sha(a) == self.digest


def _encode(v, digests: bool = True):
    import torch

    if isinstance(v, torch.Tensor):
        return {"pt": _encode(v.detach().cpu().numpy(), digests)}
    if isinstance(v, Digest):
        return {"sha": v.digest, "dtype": v.dtype.str, "shape": list(v.shape)}
    if isinstance(v, np.ndarray):
        if digests and v.size >= _DIGEST_MIN:
            return {"sha": sha(v), "dtype": v.dtype.str, "shape": list(v.shape)}
        flat = v.reshape(-1)
        data = [str(x) for x in flat] if v.dtype.kind in "US" else (flat.astype(np.float64).tolist() if v.dtype.kind == "f"
                                                                     else flat.tolist())
        return {"nd": data, "dtype": v.dtype.str, "shape": list(v.shape)}
    if isinstance(v, np.generic):
        return {"np": _encode(np.asarray(v), digests)}
    if isinstance(v, (list, tuple)):
        return {"seq": [_encode(x, digests) for x in v], "tuple": isinstance(v, tuple)}
    if isinstance(v, dict):
        return {"map": [[k, _encode(x, digests)] for k, x in v.items()]}
    if isinstance(v, float):
        return {"f": repr(v)}                      # exact: float(repr(x)) == x, inf / nan included
    if v is None or isinstance(v, (bool, int, str)):
        return v
    raise TypeError(f"cannot record {type(v).__name__}")


def _decode(o):
    import torch

    if not isinstance(o, dict):
        return o
    if "pt" in o:
        a = _decode(o["pt"])
        return a if isinstance(a, Digest) else torch.from_numpy(a)
    if "sha" in o:
        return Digest(o["dtype"], o["shape"], o["sha"])
    if "nd" in o:
        dt = np.dtype(o["dtype"])
        return np.asarray(o["nd"], dtype=np.float64 if dt.kind == "f" else None).astype(dt).reshape(o["shape"])
    if "np" in o:
        return _decode(o["np"])[()]
    if "seq" in o:
        seq = [_decode(x) for x in o["seq"]]
        return tuple(seq) if o["tuple"] else seq
    if "map" in o:
        return {k: _decode(x) for k, x in o["map"]}
    if "f" in o:
        return float(o["f"])
    raise ValueError(o)


def same(want, got) -> bool:
    """Exact equality of a reference output (live, or replayed: arrays, Digests, scalars, nested sequences) and ours."""
    import torch

    if isinstance(want, Digest):
        return want.matches(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got)
    if isinstance(want, (list, tuple)) and isinstance(got, (list, tuple)):
        return len(want) == len(got) and all(same(a, b) for a, b in zip(want, got))
    if isinstance(want, (np.ndarray, torch.Tensor)) or isinstance(got, (np.ndarray, torch.Tensor)):
        a = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
        b = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
        return a.shape == b.shape and np.array_equal(a, b)
    return want == got


class ReferenceRecord:
    """The reference's side of a differential test, live or replayed.  ``rec(fn)`` returns ``fn()`` -- a call into the reference --
    where the reference tree exists, and the value that call returned when the record was made everywhere else, in call order.
    Live runs check every value against the committed record (large arrays by SHA-256), so the record cannot drift from the
    reference; ``VLFM_RECORD_REFERENCE=1`` (re)writes tests/golden/ref_<name>.json.gz instead."""

    def __init__(self, name: str):
        import gzip
        import json

        self.path = os.path.join(GOLDEN_DIR, f"ref_{name}.json.gz")
        self.live = reference_present()
        self.recording = self.live and os.environ.get(RECORD_ENV) == "1"
        self.values = []
        self.k = 0
        if not self.recording:
            if not os.path.isfile(self.path):
                raise FileNotFoundError(f"{self.path}: recorded reference outputs missing (make them with {RECORD_ENV}=1 "
                                        "where the reference tree exists)")
            with gzip.open(self.path, "rt") as f:
                self.values = json.load(f)

    def __call__(self, fn, digest: bool = True):
        """``digest=False`` stores every element (for values compared within a tolerance)."""
        if not self.live:
            assert self.k < len(self.values), f"{self.path}: more reference calls than recorded"
            v = _decode(self.values[self.k])
            self.k += 1
            return v
        v = fn()
        if self.recording:
            self.values.append(_encode(v, digest))
        else:
            assert self.k < len(self.values), f"{self.path}: more reference calls than recorded"
            rec = _decode(self.values[self.k])
            self.k += 1
            assert same(rec, v), f"{self.path}: value {self.k - 1} differs from the live reference"
        return v

    def close(self) -> None:
        import gzip
        import json

        if self.recording:
            with gzip.open(self.path, "wt") as f:
                json.dump(self.values, f, separators=(",", ":"))
        else:
            assert self.k == len(self.values), f"{self.path}: {len(self.values) - self.k} recorded reference calls left over"
