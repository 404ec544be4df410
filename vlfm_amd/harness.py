"""Batched-episode harness: E independent synthetic ObjectNav episodes resident on ONE GPU, stepped together.

Replaces the reference's single-env Habitat eval loop (vlfm/utils/vlfm_trainer.py:164-174, which raises when
distributed, :65-66) for throughput measurement.  One `step()` performs, for every resident environment, the
per-step hot path of ITMPolicyV2 (vlfm/policy/itm_policy.py:251-261):

    _cache_observations -> ObstacleMap.update_map      (habitat_policies.py:193-201)      [depth ingest + obstacle kernels]
    _update_value_map   -> BLIP2ITMClient.cosine        (itm_policy.py:191-203)            [batched in-process BLIP-2 ITC]
                        -> ValueMap.update_map          (itm_policy.py:204-206)            [one launch for all envs]
    _explore            -> ValueMap.sort_waypoints      (itm_policy.py:263-267)            [disc medians per frontier]

and, with a detector / segmenter / ``object_maps=True`` (the configs[2] "full" step, base_objectnav_policy.py:106-150,285-356):

    _update_object_map  -> detector.predict (YOLOv7 | GroundingDINO), class + confidence filters   (:221-241)
                        -> MobileSAM.segment_bbox per surviving box                               (:311-321)
                        -> ObjectPointCloudMap.update_map per mask, update_explored per step      (:337-350)
    act                 -> initialise (12 x TURN_LEFT) | explore (best frontier) | navigate (object goal, stop rule)
                        -> PointNav controller on the chosen goal                                  (:126-135,243-283)

Episodes are independent, so multi-GPU scaling is pure sharding (contiguous blocks: env e -> rank e // envs_per_rank,
vlfm_amd/distributed.py); the only collective is the metric all-reduce in bench.py.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .mapping.base_map import require_gpu
from .mapping.value_map import ValueMapBatch
from .synthetic import MAX_DEPTH, MIN_DEPTH, BangBangController, ReplayController, Trajectory, camera_intrinsics, depth_frame, \
    ProceduralWorlds, pose_to_tf, rgb_frame, PLAN_INVALID, PLAN_OK, PLAN_TOO_LONG, PLAN_UNREACHABLE, GridWorlds, _mix32, DepthSensor, DepthFilter  # noqa: F401
from .worlds import GeodesicFields, LatticeFields, LiveWorld, RoomsRenderer, WorldObjects, WorldTable, check_geodesic_backend, \
    objectnav_outcome, sightings_from_stats  # noqa: F401  (the worlds' names stay importable from here)

PROMPT = "Seems like there is a target_object ahead."  # vlfm/policy/base_objectnav_policy.py:377
TARGETS = ["chair", "bed", "potted plant", "toilet", "tv", "couch"]  # HM3D ObjectNav categories
OBSTACLE_HOLE_AREA_THRESH = 100000   # the harness's obstacle maps fill small depth holes (the reference's default); -1: they would not


class ScriptedSightings:
    """A deterministic detector HEAD and episode script for networks without pretrained weights: which (environment, step) pairs
    carry a detection, of what, how confident, where in the image and how far away -- a pure function of (env_id, step), so that
    the workload of the stages behind the detector (MobileSAM, ObjectPointCloudMap) is STATED instead of being decided by random
    logits.  An environment lives through ObjectNav episodes shaped like the reference's: 12 initialisation turns, a SEARCH phase of
    ``search_min + (hash mod search_span)`` steps in which only distractors show up (``distractor_rate`` of the steps: a wrong class
    or a low-confidence target, which the filters of base_objectnav_policy.py:231-233 must drop before SAM), then the target IN VIEW
    for ``nav_steps`` steps (``in_view_rate`` of them carry a confidence-0.9 detection: survives both the 0.8 YOLOv7 and the 0.4
    GroundingDINO threshold) while the policy navigates to it; after the last of these the robot "arrives": the episode ends like
    the reference's does on STOP, and the environment starts the next one in place (maps, object map, selector and controller
    reset).  ``desync``: environment e starts ``hash(e)`` steps into its first episode, so a batch is spread over all phases.
    The object is an ellipse painted into the depth frame (nearer surfaces win), so the object cloud is an object, not a wall."""

    def __init__(self, in_view_rate: float = 0.8, distractor_rate: float = 0.0625, search_min: int = 60, search_span: int = 120,
                 nav_steps: int = 30, height: int = 480, width: int = 640, desync: bool = True) -> None:
        self.in_view_rate, self.distractor_rate = in_view_rate, distractor_rate
        self.search_min, self.search_span, self.nav_steps = search_min, search_span, nav_steps
        self.H, self.W, self.desync = height, width, desync

    def episode_length(self, env_id: int, k: int) -> int:
        return 12 + self.search_min + _mix32(env_id, k, 3) % max(self.search_span, 1) + self.nav_steps

    def locate(self, env_id: int, step: int):
        """(episode index, step inside the episode, episode length) of environment ``env_id`` at harness step ``step``."""
        g = step + (_mix32(env_id, 0, 9) % self.episode_length(env_id, 0) if self.desync else 0)
        k = 0
        while g >= self.episode_length(env_id, k):
            g -= self.episode_length(env_id, k)
            k += 1
        return k, g, self.episode_length(env_id, k)

    def episode_ends(self, env_id: int, step: int) -> bool:
        _, s_, n = self.locate(env_id, step)
        return s_ == n - 1

    def mean_detections_per_env_step(self) -> float:
        return self.in_view_rate * self.nav_steps / (12 + self.search_min + (self.search_span - 1) / 2.0 + self.nav_steps)

    def at(self, env_id: int, step: int, target: str):
        """[(phrase, confidence, (cx, cy, ax, ay) pixels, normalised depth)] for one environment-step."""
        _, s_, n = self.locate(env_id, step)
        if s_ < 12:
            return []
        in_view = s_ >= n - self.nav_steps
        u = _mix32(env_id, step, 1) / 2.0 ** 32
        if u >= (self.in_view_rate if in_view else self.distractor_rate):
            return []
        g = _mix32(env_id, step, 2)
        cx = int(self.W * (0.2 + 0.6 * ((g & 0xFF) / 255.0)))
        cy = int(self.H * (0.45 + 0.15 * (((g >> 8) & 0xFF) / 255.0)))
        ax, ay = 40 + ((g >> 16) & 0x1F), 50 + ((g >> 21) & 0x1F)
        depth = 0.3 + 0.3 * (((g >> 26) & 0x3F) / 63.0)
        if in_view:
            return [(target, 0.9, (cx, cy, ax, ay), depth)]
        wrong = "tv" if target != "tv" else "chair"
        return [(wrong, 0.93, (cx, cy, ax, ay), depth)] if (g & 1) else [(target, 0.35, (cx, cy, ax, ay), depth)]


SAM_BATCH_BUCKETS = (1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256)


def sam_batch_bucket(n: int) -> int:
    """The batch size the segmenter runs ``n`` boxes at: the next of a fixed set of sizes (<= 25 % padding from 4 boxes on)."""
    for b in SAM_BATCH_BUCKETS:
        if b >= n:
            return b
    return -(-n // 64) * 64


def ellipse_masks(ellipses, height: int, width: int, device) -> torch.Tensor:
    """[n,H,W] bool: (x - cx)^2 / max(ax, 1)^2 + (y - cy)^2 / max(ay, 1)^2 <= 1 in f64 for ``ellipses`` [n,4] = (cx, cy, ax, ay)."""
    e = torch.as_tensor(np.asarray(ellipses, np.float64).reshape(-1, 4), device=device)
    yy = torch.arange(height, device=device, dtype=torch.float64)[None, :, None]
    xx = torch.arange(width, device=device, dtype=torch.float64)[None, None, :]
    cx, cy = e[:, 0, None, None], e[:, 1, None, None]
    ax, ay = e[:, 2, None, None].clamp(min=1.0), e[:, 3, None, None].clamp(min=1.0)
    return (xx - cx) ** 2 / ax ** 2 + (yy - cy) ** 2 / ay ** 2 <= 1


@dataclass(frozen=True)
class Camera:
    """One camera of a rig, mounted relative to the robot pose: yawed ``yaw`` radians to the left and moved ``forward`` /
    ``left`` / ``up`` metres in the robot frame.  ``hfov`` (radians; None = the harness's 79 degrees) and the depth range are
    the camera's own (reality/objectnav_env.py:184-228 hands min_depth / max_depth / fov per camera); ``obstacle`` / ``value``
    say which map the camera feeds (the robot: several depth cameras for obstacles, one RGB-D camera for values)."""
    yaw: float = 0.0
    forward: float = 0.0
    left: float = 0.0
    up: float = 0.0
    hfov: Optional[float] = None
    min_depth: float = MIN_DEPTH
    max_depth: float = MAX_DEPTH
    obstacle: bool = True
    value: bool = True

    def offset_tf(self) -> np.ndarray:
        """xyz_yaw_to_tf_matrix (geometry_utils.py:162-180) of the mounting offset."""
        c, s = np.cos(self.yaw), np.sin(self.yaw)
        return np.array([[c, -s, 0.0, self.forward], [s, c, 0.0, self.left], [0.0, 0.0, 1.0, self.up], [0.0, 0.0, 0.0, 1.0]])


class CameraRig:
    """The cameras every environment of a ``BatchedEpisodes(rig=...)`` carries, in the order they are applied to the maps
    (the reference loops over its cameras sequentially and the value fuse does not commute).  ``designated`` is the camera whose
    frames the single-camera stages use: the detector / segmenter / object maps (its RGB frame, depth frame and pose, like
    object_map_rgbd on the robot; it keeps the harness's default optics) and the PointNav depth.  The reveal uses the robot pose."""

    def __init__(self, cameras: Sequence[Camera], designated: int = 0) -> None:
        self.cameras = list(cameras)
        if any(not (c.obstacle or c.value) for c in self.cameras):
            raise ValueError("a rig camera must feed the obstacle map, the value map or both")
        self.obstacle_ids = [i for i, c in enumerate(self.cameras) if c.obstacle]
        self.value_ids = [i for i, c in enumerate(self.cameras) if c.value]
        if not self.obstacle_ids or not self.value_ids:
            raise ValueError("a rig needs at least one obstacle camera and one value camera")
        if not 0 <= designated < len(self.cameras):
            raise ValueError("designated camera out of range")
        self.designated = designated
        self.offsets = np.stack([c.offset_tf() for c in self.cameras])          # [K,4,4]

    def __len__(self) -> int:
        return len(self.cameras)

    def camera_tfs(self, robot_tf: np.ndarray) -> np.ndarray:
        """camera -> episodic transforms [..., K, 4, 4] for robot -> episodic transforms [..., 4, 4]: robot_tf @ offset."""
        robot_tf = np.asarray(robot_tf, np.float64)
        return np.matmul(robot_tf[..., None, :, :], self.offsets)


def episode_prompts(text_prompt: str, exploration_thresh: Optional[float], targets: Sequence[str]) -> List[List[str]]:
    """The prompts BLIP-2 sees for each environment's target: ``text_prompt`` split at "|" and checked against the policy
    (policy_step.split_text_prompt: several prompts need ``exploration_thresh``, a threshold needs two), ``target_object``
    substituted as itm_policy.py:197 does.  Needs no device."""
    from .policy_step import split_text_prompt, substitute_target

    base = split_text_prompt(text_prompt, exploration_thresh)
    return [substitute_target(base, t) for t in targets]


class BatchedEpisodes:
    def __init__(self, n_envs: int, device=None, height: int = 480, width: int = 640, env_offset: int = 0,
                 blip2=None, use_blip2: bool = True, frame_pool: int = 4, map_size: int = 1000,
                 n_frontiers: int = 8, sync_explored: bool = False, obstacle: bool = True,
                 episode_len: int = 500, overlap: bool = True, detector=None, sam=None, sam_every: int = 4,
                 graph_blip2: Optional[bool] = None, host_inputs: bool = False, select_frontiers: bool = False,
                 pointnav=None, world: str = "rooms", object_maps: bool = False,
                 sightings: Optional["ScriptedSightings"] = None, scripted_masks: bool = False,
                 coco_threshold: float = 0.8, non_coco_threshold: float = 0.4, pointnav_stop_radius: float = 0.9,
                 object_map_erosion_size: float = 5, concurrent_vlm_max_envs: int = 0,
                 render_trajectories: bool = False, emulate_jpeg: bool = False, rig: Optional[CameraRig] = None,
                 text_prompt: str = PROMPT, exploration_thresh: Optional[float] = None, closed_loop: bool = False,
                 controller=None, world_objects: Optional[WorldObjects] = None, batch_object_maps: bool = True,
                 device_object_clouds: bool = True, objectnav_metrics: bool = False,
                 worlds: Optional[Union[ProceduralWorlds, GridWorlds]] = None, render_rgb: bool = False,
                 geodesic: str = "graph", depth_sensor: Optional[DepthSensor] = None,
                 depth_filter: Optional[DepthFilter] = None) -> None:
        # text_prompt: "|"-separated prompts, one value-map channel each (itm_policy.py:50-54); exploration_thresh: ITMPolicyV3's
        # frontier rule over the two channels "target | exploration" (itm_policy.py:270-317).  Checked before the device is.
        self.env_ids = [env_offset + e for e in range(n_envs)]
        self.targets = [TARGETS[i % len(TARGETS)] for i in self.env_ids]
        self.prompt_lists = episode_prompts(text_prompt, exploration_thresh, self.targets)
        self.C = len(self.prompt_lists[0]) if self.prompt_lists else len(text_prompt.split("|"))
        self.exploration_thresh = exploration_thresh
        # closed_loop: the actions MOVE the robots (synthetic.step_poses) and every step observes from where they now are
        # (RoomsRenderer.cast_cameras) instead of from the next pose of the planned tour; the actions are the PointNav
        # controller's when it has the discrete head, else ``controller``'s: any object with
        # act(modes, rho_theta [E,2], stops [E], collided [E]) -> int64 [E] action ids (default: BangBangController)
        self.closed_loop = bool(closed_loop)
        # batch_object_maps: all detections of a step go through the object-cloud kernels together (update_maps_batch); False =
        # one ObjectPointCloudMap.update_map per detection, each a batch of one job -- same clouds, same random draws, more launches
        # and read-backs, kept for comparison
        self.batch_object_maps = bool(batch_object_maps)
        # device_object_clouds: update_explored and the object goals of all environments are asked of device mirrors of the clouds,
        # one launch and one read-back each per step (update_explored_batch, get_best_objects_batch); False = one NumPy pass per
        # environment over its accumulated clouds -- same clouds, same goals, kept for comparison
        self.device_object_clouds = bool(device_object_clouds)
        self.last_explored_drops = None         # device_object_clouds: per environment with clouds, did this step drop a far tag
        if self.closed_loop:
            if world != "rooms" or host_inputs:
                raise ValueError("closed_loop needs the rooms world rendered on the device (world='rooms', host_inputs=False)")
            if not obstacle or not select_frontiers:
                raise ValueError("closed_loop needs the obstacle map and the frontier selection (obstacle=True, "
                                 "select_frontiers=True): without a goal there is nothing to act on")
            if pointnav is not None and not getattr(pointnav, "discrete", False):
                raise ValueError("closed_loop needs discrete action ids: a PointNav policy with the continuous head cannot "
                                 "drive the 30 degree / 0.25 m world")
        elif controller is not None:
            raise ValueError("a controller acts only in a closed_loop harness")
        self.controller = (controller if controller is not None else BangBangController()) if self.closed_loop else None
        # world_objects: objects stand in the rooms world, the detector head reports what the ray caster saw of them, and the
        # environments run scored ObjectNav episodes (WorldObjects); None = every step is the step it always was
        self.world_objects = world_objects
        if world_objects is not None:
            if not self.closed_loop:
                raise ValueError("world_objects needs closed_loop=True: the objects are seen from where the robot is")
            if sightings is not None:
                raise ValueError("world_objects replaces the scripted sightings: give one of the two")
            if rig is not None:
                raise ValueError("world_objects renders the robot's own camera: it cannot be combined with a camera rig")
        # objectnav_metrics: the episodes are also scored by SPL, SoftSPL and the geodesic distance_to_goal (geodesic fields on
        # the device: one launch when episodes start, one query launch and read-back per step); nothing reads them back into the
        # policy, the controller or the world.  Off: every step and every key of objectnav_stats is what it always was
        self.objectnav_metrics = bool(objectnav_metrics)
        if self.objectnav_metrics and world_objects is None:
            raise ValueError("objectnav_metrics scores ObjectNav episodes: it needs world_objects")
        # worlds: environment e lives in its OWN floor plan, worlds.world(env_ids[e], episode) -- its robot starts at that world's
        # start pose, its depth is ray-cast against that world's walls (RoomsRenderer.cast_worlds, still one launch per step), its
        # moves are refused by them, and with world_objects every episode end draws the NEXT world (layouts from the world's own
        # spots, geodesics over its own walls); without world_objects it stays in episode 0's.  None: the one rooms world.
        # synthetic.GridWorlds: the worlds are occupancy grids (a top-down map someone already has) -- the same code, the world
        # table carries the grids beside the boxes
        self.worlds = worlds
        if worlds is not None:
            if not self.closed_loop:
                raise ValueError("worlds needs closed_loop=True: the open-loop tour is planned through the rooms world")
            if rig is not None:
                raise ValueError("worlds renders the robot's own camera: it cannot be combined with a camera rig")
            if sightings is not None:
                raise ValueError("worlds cannot be combined with the scripted sightings, which are painted along the rooms tour")
            # grid worlds (synthetic.GridWorlds: ``worlds.max_grid``): floor plans as occupancy grids, through the same code
            if getattr(worlds, "max_grid", None) is not None:
                if render_rgb:
                    raise ValueError("grid worlds cannot be combined with render_rgb: wall colours are defined by box and face")
        # geodesic: what the metrics measure path lengths with -- "graph": the visibility graph over the inflated rectangles (at
        # most 141 of them: no grid worlds); "lattice": the 16-connected metric lattice with integer costs, for every kind of world
        # (csrc/lattice_geodesic.hip; within [0.9838, 1.05] of the graph's lengths in the rooms world).  Same keys either way
        check_geodesic_backend(geodesic, self.objectnav_metrics, worlds)
        self.geodesic_backend = geodesic
        # render_rgb: the step's RGB frames are the camera's view of the world the depth frame shows (RoomsRenderer.cast_worlds_rgb /
        # cast_cameras_rgb: depth, ids, stats and colours from ONE launch) instead of the pool's noise -- what the transport hop,
        # BLIP-2, the detector and the segmenter then see; they stay readable as ``live.rgb``.  Off: every step is the step it was
        self.render_rgb = bool(render_rgb)
        if self.render_rgb:
            if not self.closed_loop:
                raise ValueError("render_rgb needs closed_loop=True: the frames are rendered from where the robot is")
            if rig is not None:
                raise ValueError("render_rgb renders the robot's own camera: it cannot be combined with a camera rig")
        # depth_sensor: a synthetic.DepthSensor between the ray caster and everything that reads the step's depth frames (both
        # maps, the object clouds, PointNav, the planner): noise, quantisation and holes, one more launch per step
        # (RoomsRenderer.sense_depth); ``live.clean_frames`` keeps the exact ranges.  Off: every step is the step it was
        # depth_filter: a synthetic.DepthFilter after the sensor (without one: after the ray caster) and before every reader: the
        # holes are filled from the nearest valid pixels of their row and column, two more launches per step
        # (RoomsRenderer.filter_depth); ``live.sensed_frames`` keeps what went in.  Off: every step is the step it was
        self.depth_filter = depth_filter
        if depth_filter is not None:
            if not isinstance(depth_filter, DepthFilter):
                raise ValueError("depth_filter must be a synthetic.DepthFilter")
            if not self.closed_loop:
                raise ValueError("depth_filter needs closed_loop=True: it filters the frames rendered from where the robot is")
            if rig is not None:
                raise ValueError("depth_filter filters the robot's own camera: it cannot be combined with a camera rig")
        self.depth_sensor = depth_sensor
        if depth_sensor is not None:
            if not isinstance(depth_sensor, DepthSensor):
                raise ValueError("depth_sensor must be a synthetic.DepthSensor")
            if not self.closed_loop:
                raise ValueError("depth_sensor needs closed_loop=True: it senses the frames rendered from where the robot is")
            if rig is not None:
                raise ValueError("depth_sensor senses the robot's own camera: it cannot be combined with a camera rig")
            from .mapping.obstacle_map import ObstacleMapBatch

            # isolated invalid pixels are one contour each for fill_small_holes, whose scratch holds HOLE_CAP_CONTOURS of them
            bound = ObstacleMapBatch.HOLE_CAP_CONTOURS / 2
            if depth_filter is not None:
                # a hole the filter leaves has no source within reach in any direction, so (reach_px >= 1) its four neighbours
                # inside the frame are holes too: dropout alone leaves at most the pixels dropped together with all four
                left = depth_sensor.dropout ** 5 * height * width
                if OBSTACLE_HOLE_AREA_THRESH != -1 and left > bound:
                    raise ValueError(f"depth_sensor with depth_filter: dropout**5 * height * width = {left:.0f} (the pixels dropped "
                                     f"together with their four neighbours, all the filter can leave) exceeds "
                                     f"ObstacleMapBatch.HOLE_CAP_CONTOURS / 2 = {bound:.0f} contours of the obstacle map's hole "
                                     f"filling: at {width} x {height} dropout <= {(bound / (height * width)) ** 0.2:.3f}")
            elif OBSTACLE_HOLE_AREA_THRESH != -1 and depth_sensor.dropout * height * width > bound:
                raise ValueError(f"depth_sensor: dropout * height * width = {depth_sensor.dropout * height * width:.0f} exceeds "
                                 f"ObstacleMapBatch.HOLE_CAP_CONTOURS / 2 = {bound:.0f} contours of the obstacle map's hole filling: "
                                 f"at {width} x {height} dropout <= {bound / (height * width):.3f}")
        self.device = require_gpu(device)
        # rig: K cameras per environment (CameraRig) fused into the environment's maps by ONE ingest_cameras / update_cameras per
        # step (step() -> _step_rig()); None = one camera at the robot pose, the step as it always was
        self.rig = rig
        if rig is not None:
            if world != "rooms" or host_inputs or not obstacle:
                raise ValueError("a camera rig needs the rooms world rendered on the device and the obstacle map")
            dc = rig.cameras[rig.designated]
            if (detector is not None or sam is not None or object_maps) and not (
                    dc.hfov in (None, camera_intrinsics(width)[2]) and dc.min_depth == MIN_DEPTH and dc.max_depth == MAX_DEPTH):
                raise ValueError("the designated camera feeds the detector / object-map stage, which runs with the harness's "
                                 "own optics: give it the default hfov and depth range")
        # a rank waiting for its GPU must not hold a host core (bench.py `host`).  Effective only before the device's first
        # stream exists (bench.py sets it first thing); here it is best effort: a warning on failure, VLFM_HOST_WAIT=spin opts out
        _lib.try_host_wait_blocking(self.device)
        self.E, self.H, self.W, self.S = n_envs, height, width, map_size
        # opt-in: record every step's pose in the maps' trajectory planes for render() (one small launch per map and step)
        self.render_trajectories = render_trajectories
        # opt-in: the reference's q90 JPEG client -> server hop (server_wrapper.py:57-68) on the step's RGB frames, on the
        # device (transport.jpeg_roundtrip_batch): BLIP-2, the detector and MobileSAM then see what the reference's models see
        self.emulate_jpeg = emulate_jpeg
        self.jpeg_frames = self.jpeg_scratch = None
        if emulate_jpeg:
            from .vlm.transport import jpeg_roundtrip_scratch

            self.jpeg_frames = torch.empty((n_envs, height, width, 3), dtype=torch.uint8, device=self.device)
            self.jpeg_scratch = jpeg_roundtrip_scratch(n_envs, height, width, self.device)
        self.fx, self.fy, self.fov = camera_intrinsics(width)
        self.episode_len = episode_len
        # one prompt: the environments' prompts as strings (what cosine_batch takes); several: per-environment lists
        self.prompts = [p[0] for p in self.prompt_lists] if self.C == 1 else self.prompt_lists
        self.values = ValueMapBatch(n_envs, self.C, map_size, use_max_confidence=False, device=self.device)
        self.n_frontiers = n_frontiers
        self.t = 0
        self.episodes_done = 0
        # synthetic observations live in HBM before the timed region starts (bench contract): a small pool of
        # distinct frames per env, cycled; the scripted poses of a whole episode are tabulated up front as well
        rng = np.random.Generator(np.random.PCG64(99991 + env_offset))
        # world "rooms": every environment walks the consistent rooms-and-pillars world (frames ray-cast on the device,
        # RoomsRenderer); world "random": SURVEY 8d's per-frame random wall profiles on scripted random-walk poses
        assert world in ("rooms", "random")
        self.rooms = RoomsRenderer(self.env_ids, episode_len, height, width, self.device) \
            if world == "rooms" and not host_inputs else None
        depth_pool = torch.from_numpy(np.stack([
            np.stack([depth_frame(rng, height, width) for _ in range(n_envs)])
            for _ in range(1 if self.rooms is not None else frame_pool)]))
        rgb_pool = torch.from_numpy(np.stack([
            np.stack([rgb_frame(rng, height, width) for _ in range(n_envs)]) for _ in range(frame_pool)]))
        # host_inputs: the simulator hands over HOST buffers every step (what the reference's API receives); the frames
        # then cross PCIe inside the step -- the "PCIe-inclusive" rate of DESIGN.md, never the headline value
        self.host_inputs = host_inputs
        if host_inputs:
            self.depth_pool, self.rgb_pool = depth_pool.pin_memory(), rgb_pool.pin_memory()
            self.depth_dev = torch.empty(depth_pool.shape[1:], dtype=depth_pool.dtype, device=self.device)
            self.rgb_dev = torch.empty(rgb_pool.shape[1:], dtype=rgb_pool.dtype, device=self.device)
        else:
            self.depth_pool, self.rgb_pool = depth_pool.to(self.device), rgb_pool.to(self.device)
        if self.rooms is not None:
            self.pose_table, self.tf_table = self.rooms.pose_table, self.rooms.tf_table
        else:
            trajs = [Trajectory(i) for i in self.env_ids]
            self.pose_table = np.array([[tr.step() for tr in trajs] for _ in range(episode_len)])  # [L,E,3]
            self.tf_table = np.stack([np.stack([pose_to_tf(x, y, yaw) for (x, y, yaw) in row]) for row in self.pose_table])
        # closed loop: the simulator -- where the robots are, their worlds, objects and episodes (worlds.LiveWorld); else None
        self.live = LiveWorld(self.rooms, self.env_ids, self.targets, world_objects, worlds, objectnav_metrics,
                              render_rgb, geodesic, depth_sensor, depth_filter) if self.closed_loop else None
        self.last_poses = self.last_world_actions = None     # closed loop: the poses the last step observed from, its actions
        # of a controller with act_on_map (MapPlannerController): plans = ok + unreachable + too_long + invalid (off the map)
        self.planner_stats = {k: np.zeros(n_envs, np.int64) for k in ("plans", "ok", "unreachable", "too_long", "invalid")}
        self.blip2 = blip2
        if use_blip2 and blip2 is None:
            from .vlm.blip2itm import BLIP2ITM

            self.blip2 = BLIP2ITM(device=self.device, allow_random_init=True)  # synthetic-episode harness: throughput only
        # small batches are launch-bound: replay the BLIP-2 forward from a captured HIP graph
        self.graph_blip2 = (n_envs <= 4) if graph_blip2 is None else graph_blip2  # measured: +43 % at 1 env, none at 8
        self.stub_rng = np.random.Generator(np.random.PCG64(7 + env_offset))
        self.obstacles = None
        if obstacle:
            from .mapping.obstacle_map import ObstacleMapBatch

            self.obstacles = ObstacleMapBatch(n_envs, min_height=0.61, max_height=0.88, agent_radius=0.18,
                                              area_thresh=1.5, hole_area_thresh=OBSTACLE_HOLE_AREA_THRESH, size=map_size,
                                              device=self.device)
            if sync_explored:
                self.values.explored_bits = self.obstacles.explored_bits
        # The obstacle pipeline is a handful of latency-bound workgroups per environment: it runs on its own HIP
        # stream beside the BLIP-2 GEMMs (which fill the chip) instead of in front of them.
        # "full" ITMPolicyV2 step (configs[2]): object detector on every frame (YOLOv7 for the COCO targets of HM3D,
        # base_objectnav_policy.py:221-233) and MobileSAM on the boxes that survive (:311-321).  With random-init networks
        # detections carry no meaning, so SAM is exercised on one synthetic box for every ``sam_every``-th environment-step.
        self.detector, self.sam, self.sam_every = detector, sam, sam_every
        self.detector_is_prompted = detector is not None and "caption" in getattr(detector, "__dict__", {})
        self.gdino_caption = " . ".join(TARGETS) + " ."
        self.last_detections = None
        self.last_masks = None
        # the stage BEHIND the detector (base_objectnav_policy.py:311-350): one ObjectPointCloudMap per environment, each with
        # its own NumPy stream (the reference draws from the global generator; E interleaved episodes need E streams)
        self.object_maps = None
        if object_maps:
            from .mapping.object_point_cloud_map import ObjectPointCloudMap

            self.object_maps = [ObjectPointCloudMap(object_map_erosion_size, device=self.device,
                                                    rng=np.random.RandomState(1000 + i)) for i in self.env_ids]
        self.sightings, self.scripted_masks = sightings, scripted_masks
        self.scripted_through_nms = True    # YOLOv7: the scripted head's candidates go through the detector's real post-processing
        self._sight_cache: Dict[int, List] = {}
        self._sched_cache: Dict[int, tuple] = {}
        if sightings is not None and self.rooms is not None:
            self.rooms.painter = self._paint_sightings
        self.det_threshold = non_coco_threshold if self.detector_is_prompted else coco_threshold   # :231-233
        self.stop_radius = pointnav_stop_radius
        self.last_modes: List[str] = []
        self.last_episode_end = np.zeros(n_envs, bool)
        self.last_stops = np.zeros(n_envs, bool)
        self.last_resets = np.zeros(n_envs, bool)
        self.last_rho_theta = np.full((n_envs, 2), np.nan)
        self.object_stats = {"detections": 0, "masks": 0, "cloud_updates": 0, "env_steps": 0,
                             "modes": {"initialize": 0, "explore": 0, "navigate": 0}}
        # SAM + ObjectPointCloudMap updates (a chain of small kernels and host read-backs) run beside the BLIP-2 forward (step()).
        # In the full step from 128 environments on, their stream and the map stream are HIGH-PRIORITY queues: beside a forward whose GEMMs hold every CU for a millisecond
        # at a time, the chain's small kernels otherwise wait their turn and the step ends when THEY do -- measured on one box, three
        # runs each (profiles/r05_side_stream_priority.txt): 726-738 env-steps/s at priority 0 (other boxes: 845-849, i.e. the slow
        # mode is box- or run-dependent) against 819-828 at priority -1; at 64 environments the priority costs 7 % (746-767 -> 702-715:
        # there the forward is the shorter part and is the one being pushed aside), so it is not set below 128.
        full_step = detector is not None and object_maps
        prio = -1 if n_envs >= 128 and full_step else 0
        self.map_stream = torch.cuda.Stream(self.device, priority=prio) if overlap else None
        self.obj_stream = torch.cuda.Stream(self.device, priority=prio) if overlap else None
        # (the object stream alone at priority -1: 790-796; both: 819-828; the headline -- no detector -- keeps priority 0: -0.3 % with it)
        # Optional (concurrent_vlm_max_envs > 0): at small batches neither the detector (a HIP graph of ~1 700 short
        # kernels for GroundingDINO) nor the BLIP-2 forward of 8 frames fills the chip, so the BLIP-2 forward can be enqueued FIRST,
        # on its own stream, with the detector beside it.  Measured in round 5 (profiles/r05_full_step_ab.txt): 323.6 -> 323.5
        # env-steps/s at 8 environments (YOLOv7-E6E), 184 -> 185 with GroundingDINO, 783 -> 672 at 64: no gain -- the 8-environment
        # step is bound by the host's launch rate and its read-backs, not by GPU occupancy -- so it is OFF by default; the
        # equivalence test (tests/test_full_step_gpu.py) keeps the path honest.
        self.vlm_stream = torch.cuda.Stream(self.device) if overlap and n_envs <= concurrent_vlm_max_envs else None
        self.last_cosines: Optional[torch.Tensor] = None
        self.last_frontier_values: Optional[np.ndarray] = None
        self.last_frontier_envs: Optional[np.ndarray] = None      # environment slot of each row of last_frontier_values
        # frontier selection of ITMPolicyV2 (stick-to-last rule, itm_policy.py:76-152), one selector per environment
        self.selectors = None
        if select_frontiers:
            from .policy_step import FrontierSelector

            self.selectors = [FrontierSelector() for _ in range(n_envs)]
        self.last_goals: Optional[np.ndarray] = None
        # PointNav controller (vlfm_amd.pointnav.WrappedPointNavResNetPolicy built for n_envs): the action towards the
        # selected frontier, one batched forward (base_objectnav_policy.py:243-283)
        self.pointnav = pointnav
        self.prev_goals = np.zeros((n_envs, 2))
        self.last_actions = None
        self.last_rig = None          # (frames, camera transforms, slots, camera indices) of the last rig step
        self._rig_keys = None
        self.timers: Dict[str, List] = {}

    def reset(self) -> None:
        self.t = 0
        self._reset_envs()
        if self.live is not None:
            self.live.reset()

    def _reset_envs(self, envs: Optional[List[int]] = None) -> None:
        """What an episode must not inherit, of the environments ``envs`` (None: all, each store as a whole): maps, object map,
        selector, previous goal, PointNav state and -- unless a SCRIPTED episode ends in place -- the controller's."""
        from .policy_step import FrontierSelector

        self.values.reset(envs)
        if self.obstacles is not None:
            self.obstacles.reset(envs)
        for e in range(self.E) if envs is None else envs:
            if self.object_maps is not None:
                self.object_maps[e].reset()
            if self.selectors is not None:
                self.selectors[e] = FrontierSelector()
        self.prev_goals[slice(None) if envs is None else envs] = 0.0
        if self.pointnav is not None:
            self.pointnav.reset(envs)
        if (envs is None or self.world_objects is not None) and hasattr(self.controller, "reset"):
            self.controller.reset() if envs is None else self.controller.reset(envs)

    # ------------------------------------------------------------------------------------------ scripted detector head
    def _sightings_at(self, t_ep: int) -> List:
        """[(env slot, phrase, confidence, (cx, cy, ax, ay), depth)] of episode step ``t_ep`` (memoised: the painter asks when
        the frame is rendered, the step asks again when it runs)."""
        if self.world_objects is not None:
            return self.live.sightings          # what the ray caster saw of the objects in this step's frames
        if t_ep not in self._sight_cache:
            if len(self._sight_cache) > 4096:
                self._sight_cache.clear()
            self._sight_cache[t_ep] = [(e, *sg) for e, i in enumerate(self.env_ids)
                                       for sg in self.sightings.at(i, t_ep, self.targets[e])]
        return self._sight_cache[t_ep]

    def _paint_sightings(self, t_ep: int, frames: torch.Tensor) -> torch.Tensor:
        """The scripted objects of step ``t_ep`` into the rendered depth frames: an ellipse at the object's depth wherever it is
        nearer than the wall / floor behind it (so both maps and the object cloud see one consistent scene)."""
        sg = self._sightings_at(t_ep)
        self._schedule(t_ep)
        if not sg:
            return frames
        idx = torch.tensor([s_[0] for s_ in sg], device=frames.device)
        m = ellipse_masks([s_[3] for s_ in sg], self.H, self.W, frames.device)
        d = torch.tensor([s_[4] for s_ in sg], dtype=frames.dtype, device=frames.device)[:, None, None]
        cur = frames[idx]
        frames[idx] = torch.where(m, torch.minimum(cur, d), cur)   # (an environment has at most one sighting per step)
        return frames

    CANDIDATES_PER_SIGHTING = 24

    def _inject_candidates(self, pred: torch.Tensor, in_hw, t_ep: int) -> torch.Tensor:
        """Write the scripted head's candidates into the detector's raw prediction [E, N, 5 + classes] (xywh in network-input pixels,
        objectness, class scores): per sighting a cluster of CANDIDATES_PER_SIGHTING boxes -- the scripted box with the scripted
        confidence and jittered, slightly less confident copies that the NMS has to suppress -- in the first rows of its frame;
        every other row keeps the network's own output (random weights: nothing passes the objectness gate)."""
        from .vlm.coco_classes import COCO_CLASSES

        sg = self._sightings_at(t_ep)
        if not sg:
            return pred
        K = self.CANDIDATES_PER_SIGHTING
        # the inverse of scale_coords (yolov7 [ext], as yolov7.py:99 calls it: one gain + centring pads, although the frame was
        # resized anisotropically -- the reference's quirk is kept): a box given in frame pixels comes back as itself, rounded
        gain = min(in_hw[0] / self.H, in_hw[1] / self.W)
        padx, pady = (in_hw[1] - self.W * gain) / 2, (in_hw[0] - self.H * gain) / 2
        rows = np.zeros((len(sg), K, pred.shape[2]), np.float32)
        # jitter of the suppressed copies: at most +-2 network pixels, scaled down for small boxes so that every copy keeps an IoU
        # above the NMS threshold (0.45) with the scripted box -- a copy that drifted below it would survive as a second detection
        jit = np.random.Generator(np.random.PCG64(4242 + t_ep)).uniform(-1.0, 1.0, size=(len(sg), K, 4)).astype(np.float32)
        jit[:, 0] = 0.0
        used = {}
        dst_e, dst_r = [], []
        for n, (e, phrase, conf, (cx, cy, ax, ay), _) in enumerate(sg):
            cls = COCO_CLASSES.index(phrase)
            amp = min(2.0, 0.05 * 2 * min(ax, ay) * gain)          # 5 % of the smaller side: IoU of a jittered copy >= ~0.8
            rows[n, :, 0] = cx * gain + padx + amp * jit[n, :, 0]
            rows[n, :, 1] = cy * gain + pady + amp * jit[n, :, 1]
            rows[n, :, 2] = 2 * ax * gain + amp * jit[n, :, 2]
            rows[n, :, 3] = 2 * ay * gain + amp * jit[n, :, 3]
            rows[n, :, 4] = 1.0
            rows[n, :, 5 + cls] = conf * np.concatenate([[1.0], np.linspace(0.97, 0.75, K - 1)])   # conf = objectness x class score
            base = used.get(e, 0)
            used[e] = base + K
            dst_e += [e] * K
            dst_r += list(range(base, base + K))
        # (written in place: the prediction is the detector's own scratch output of this step, produced under inference_mode)
        pred[torch.tensor(dst_e, device=pred.device), torch.tensor(dst_r, device=pred.device)] = \
            torch.from_numpy(rows.reshape(-1, rows.shape[2])).to(pred.device, pred.dtype)
        return pred

    def _scripted_detections(self, t_ep: int):
        """What the scripted head reports for every environment at this step, as the detector clients' ``ObjectDetections``
        (normalised xyxy boxes, f32, like yolov7.py:99-110 / grounding_dino.py:60-66)."""
        from .vlm.detections import ObjectDetections

        per = [[] for _ in range(self.E)]
        for (e, phrase, conf, (cx, cy, ax, ay), _) in self._sightings_at(t_ep):
            per[e].append(([(cx - ax) / self.W, (cy - ay) / self.H, (cx + ax) / self.W, (cy + ay) / self.H], conf, phrase))
        none = (torch.zeros((0, 4), dtype=torch.float32), torch.zeros(0, dtype=torch.float32))    # most environments, most steps
        return [ObjectDetections(none[0], none[1], [], image_source=None, fmt="xyxy") if not rows else
                ObjectDetections(torch.tensor([r[0] for r in rows], dtype=torch.float32).reshape(-1, 4),
                                 torch.tensor([r[1] for r in rows], dtype=torch.float32), [r[2] for r in rows],
                                 image_source=None, fmt="xyxy") for rows in per]

    # ------------------------------------------------------------------------------------------ object maps
    def _update_object_maps(self, dets, rgb: torch.Tensor, depth: torch.Tensor, tf: np.ndarray) -> None:
        """BaseObjectNavPolicy._update_object_map for every environment (base_objectnav_policy.py:285-352): class + confidence
        filters, ONE MobileSAM call for all surviving boxes of the batch (the reference re-encodes the frame per box too),
        the reference's ObjectPointCloudMap.update_map per mask (csrc/object_cloud.hip: erosion, back-projection, DBSCAN) -- all
        masks of the step as the jobs of one update_maps_batch, or with batch_object_maps=False one job per call -- update_explored
        per environment and step (one
        update_explored_batch over the environments that have clouds unless device_object_clouds=False)."""
        jobs = []
        for e, det in enumerate(dets):
            det.filter_by_class(self.targets[e].split("|"))
            det.filter_by_conf(self.det_threshold)
            # the reference multiplies the f32 row by an int64 ndarray: NumPy promotes to f64 first (:312)
            jobs += [(e, det.boxes[i].detach().cpu().numpy().astype(np.float64) * np.array([self.W, self.H, self.W, self.H]))
                     for i in range(len(det.logits))]
        self.object_stats["detections"] += len(jobs)
        self.last_masks = None
        if jobs:
            envs = [j[0] for j in jobs]
            boxes = np.stack([j[1] for j in jobs])
            masks = None
            if self.sam is not None:
                # the number of surviving boxes changes from step to step; MIOpen / hipBLASLt look every NEW batch size up (5 ms per
                # convolution the first time): the segmenter runs on a few fixed batch sizes, the tail padded with repeats
                n_pad = sam_batch_bucket(len(envs))
                pe = envs + [envs[-1]] * (n_pad - len(envs))
                pb = np.concatenate([boxes, np.repeat(boxes[-1:], n_pad - len(envs), axis=0)], axis=0)
                masks = self.sam.segment_bboxes(rgb[pe], torch.from_numpy(pb).to(torch.float32)[:, None, :])[:len(envs), 0]
            if (masks is None or self.scripted_masks) and self.world_objects is not None:
                # the instance's own pixels: the id plane of the frame the box was reported from
                masks = torch.stack([self.live.ids[e] == self.live.instance_of(e, boxes[j]) + 1 for j, e in enumerate(envs)])
            elif masks is None or self.scripted_masks:
                # without pretrained weights the segmenter's logits mean nothing: the mask handed on is the box's inscribed ellipse
                # (the MobileSAM forward above still ran and is timed); also the stand-in when no segmenter is attached
                masks = ellipse_masks(np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2,
                                                (boxes[:, 2] - boxes[:, 0]) / 2, (boxes[:, 3] - boxes[:, 1]) / 2], axis=1),
                                      self.H, self.W, self.device)
            self.last_masks = (envs, masks)
            self.object_stats["masks"] += len(jobs)
            if self.batch_object_maps:
                from .mapping.object_point_cloud_map import update_maps_batch

                # depth frame of job j = environment envs[j]; counted per job like the loop below
                self.object_stats["cloud_updates"] += sum(update_maps_batch(
                    [self.object_maps[e] for e in envs], [self.targets[e] for e in envs], depth, envs, masks, tf[envs],
                    MIN_DEPTH, MAX_DEPTH, self.fx, self.fy))
            else:
                for j, e in enumerate(envs):
                    om = self.object_maps[e]
                    before = len(om.clouds.get(self.targets[e], ()))
                    om.update_map(self.targets[e], depth[e], masks[j], tf[e], MIN_DEPTH, MAX_DEPTH, self.fx, self.fy)
                    self.object_stats["cloud_updates"] += int(len(om.clouds.get(self.targets[e], ())) != before)
        have = [e for e, om in enumerate(self.object_maps) if om.clouds]
        if self.device_object_clouds:
            from .mapping.object_point_cloud_map import update_explored_batch

            self.last_explored_drops = dict(zip(have, update_explored_batch(
                [self.object_maps[e] for e in have], [tf[e] for e in have], MAX_DEPTH, self.fov)))
        else:
            for e in have:
                self.object_maps[e].update_explored(tf[e], MAX_DEPTH, self.fov)     # cone_fov = get_fov(fx, width) (:349)

    # ------------------------------------------------------------------------------------------ act
    def _episode_steps(self, t_ep: int) -> np.ndarray:
        """Steps since each environment's last episode start (the policy's ``_num_steps``): the harness step for everybody
        without a script, the script's per-environment episode clock with one."""
        if self.live is not None and self.live.ep_clock is not None:
            return self.live.ep_clock               # per environment: an episode ends when ITS robot stops or gives up
        if self.sightings is None:
            return np.full(self.E, t_ep, np.int64)
        return self._schedule(t_ep)[0]

    def _schedule(self, t_ep: int):
        """(steps into the episode [E], episode ends with this step [E]) of the script at harness step ``t_ep``, memoised (the
        painter computes it when a frame is pre-rendered, outside a timed region)."""
        hit = self._sched_cache.get(t_ep)
        if hit is None:
            if len(self._sched_cache) > 4096:
                self._sched_cache.clear()
            loc = [self.sightings.locate(i, t_ep) for i in self.env_ids]
            hit = self._sched_cache[t_ep] = (np.array([l[1] for l in loc], np.int64),
                                            np.array([l[1] == l[2] - 1 for l in loc], bool))
        return hit

    def _end_episodes(self, t_ep: int) -> None:
        """Environments whose scripted episode ends with this step (the robot "arrived": the reference's episode ends on STOP):
        their maps, object map, selector and controller state are reset for the next episode, which starts in place."""
        self.last_episode_end = np.zeros(self.E, bool)
        if self.world_objects is not None:       # decided after ``_navigate``: the world says whose episode ends, and scores it
            done = self.live.end_episodes(self.last_modes, self.last_stops)
        elif self.sightings is None:
            return
        else:
            done = np.flatnonzero(self._schedule(t_ep)[1]).tolist()
        if not done:
            return
        self.last_episode_end[done] = True
        self._reset_envs(done)
        self.object_stats["episodes_ended"] = self.object_stats.get("episodes_ended", 0) + len(done)
        if self.world_objects is not None:       # the next episode: a new layout around the robot (with ``worlds``: a new world)
            self.live.start_episodes(done)

    def _decide(self, wps: np.ndarray, env_of: np.ndarray, vals, poses: np.ndarray, t_ep: int):
        """BaseObjectNavPolicy.act's three modes for every environment (base_objectnav_policy.py:126-135): 12 initialisation
        turns, then the object goal if the object map has the target, else the best frontier (itm_policy.py:64-152).  Returns
        (modes, goals [E,2] (nan = none), stop_no_frontier [E])."""
        goals = np.full((self.E, 2), np.nan)
        modes, halt = [], np.zeros(self.E, bool)
        thresh = self.exploration_thresh
        if thresh is None:
            vals = np.asarray(vals, np.float64).reshape(-1) if vals is not None else np.zeros(0)
        else:
            from .policy_step import explore_reduce_values

            vals = np.asarray(vals, np.float64).reshape(-1, self.C) if vals is not None else np.zeros((0, self.C))
        bounds = np.searchsorted(env_of, np.arange(self.E + 1))
        ep_steps = self._episode_steps(t_ep)
        object_goals = None
        if self.object_maps is not None and self.device_object_clouds:
            from .mapping.object_point_cloud_map import get_best_objects_batch

            object_goals = get_best_objects_batch(self.object_maps, self.targets, [poses[e, :2] for e in range(self.E)])
        for e in range(self.E):
            target, robot_xy = self.targets[e], poses[e, :2]
            obj = None
            if object_goals is not None:
                obj = object_goals[e]
            elif self.object_maps is not None and self.object_maps[e].has_object(target):
                obj = self.object_maps[e].get_best_object(target, robot_xy)        # every step, like the reference (:123)
            if ep_steps[e] < 12:     # _done_initializing flips after the 12th call (habitat_policies.py:150-153)
                modes.append("initialize")
            elif obj is None:
                modes.append("explore")
                lo, hi = bounds[e], bounds[e + 1]
                if hi <= lo:
                    halt[e] = True          # "No frontiers found during exploration, stopping." itm_policy.py:64-67
                    continue
                v = vals[lo:hi]
                if thresh is not None:    # ITMPolicyV3._reduce_values over this environment's frontiers (through lists: the ONE
                    # function the single-environment policy uses, which takes the reference's list of tuples)
                    v = np.array(explore_reduce_values(v.tolist(), thresh), np.float64)
                order = np.argsort(-v)       # sort_waypoints' descending order (value_map.py:183-186)
                pts = wps[lo:hi]
                goals[e], _ = self.selectors[e].choose(pts[order], [float(x) for x in v[order]], pts, robot_xy)
            else:
                modes.append("navigate")
                goals[e] = obj[:2]
        return modes, goals, halt

    def _navigate(self, depth: torch.Tensor, modes: List[str], goals: np.ndarray, halt: np.ndarray, poses: np.ndarray):
        """BaseObjectNavPolicy._pointnav for every environment with a goal (base_objectnav_policy.py:243-283): a goal that moved
        by more than 0.1 m resets the controller, (rho, theta) in the robot frame (geometry_utils.py:9-34), STOP within
        ``pointnav_stop_radius`` of an OBJECT goal; ONE batched controller forward.  Environments that do not consult the
        controller this step (initialising, stopping, no frontier) keep its recurrent state and previous action untouched, as in
        the single-environment policy.  Returns the [E] action ids (TURN_LEFT while initialising, STOP where issued)."""
        from .policy_step import ACTION_STOP, ACTION_TURN_LEFT

        E = self.E
        have = ~np.isnan(goals[:, 0])
        moved = np.zeros(E, bool)
        moved[have] = np.linalg.norm(goals[have] - self.prev_goals[have], axis=1) > 0.1
        self.prev_goals[have] = goals[have]
        d = np.where(have[:, None], goals - poses[:, :2], 0.0)
        c, s = np.cos(-poses[:, 2]), np.sin(-poses[:, 2])
        lx, ly = c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]
        rho, theta = np.hypot(lx, ly), np.arctan2(ly, lx)
        navigate = np.array([m == "navigate" for m in modes], bool)
        stop = halt | (have & navigate & (rho < self.stop_radius))
        run = have & ~stop
        self.last_stops, self.last_resets = stop, moved & have
        self.last_rho_theta = np.where(have[:, None], np.stack([rho, theta], axis=1), np.nan)
        if self.pointnav is None:
            return None
        pn = self.pointnav
        if moved.any():
            pn.reset(np.flatnonzero(moved))                     # (before the stop check, like the reference)
        keep = torch.from_numpy(~run).to(self.device)
        h0, a0 = pn.pointnav_test_recurrent_hidden_states.clone(), pn.pointnav_prev_actions.clone()
        rt = torch.from_numpy(np.stack([rho, theta], axis=1).astype(np.float32))
        acts = pn.act_on_depth(depth, rt, torch.from_numpy(~moved))
        pn.pointnav_test_recurrent_hidden_states[keep] = h0[keep]
        pn.pointnav_prev_actions[keep] = a0[keep]
        if not pn.discrete:
            return acts
        override = np.full(E, -1, np.int64)
        override[[m == "initialize" for m in modes]] = ACTION_TURN_LEFT
        override[stop] = ACTION_STOP
        ov = torch.from_numpy(override).to(self.device)
        return torch.where(ov >= 0, ov, acts.reshape(E).to(torch.int64))

    def warm_up_segmenter(self, max_boxes: Optional[int] = None) -> None:
        """Run the segmenter once at every batch size it can meet (``sam_batch_bucket``), outside any timed region: the library
        kernels' per-shape lookups happen here instead of in the first step that sees a size."""
        if self.sam is None:
            return
        top = sam_batch_bucket(max_boxes if max_boxes is not None else max(1, self.E // 2))
        rgb = self.rgb_pool[0]
        # on the stream the segmenter will run on (step()): MIOpen keeps its handle -- and with it the per-shape lookups -- per stream
        # (a first call on a fresh stream cost 9 ms per convolution)
        stream = self.obj_stream if (self.obj_stream is not None and self.detector is not None and self.object_maps is not None) \
            else torch.cuda.current_stream(self.device)
        torch.cuda.synchronize(self.device)
        with torch.cuda.stream(stream):
            for b in [b for b in SAM_BATCH_BUCKETS if b <= top]:
                idx = [i % self.E for i in range(b)]
                box = torch.tensor([[[0.3 * self.W, 0.3 * self.H, 0.7 * self.W, 0.8 * self.H]]] * b)
                self.sam.segment_bboxes(rgb[idx], box)
        torch.cuda.synchronize(self.device)

    def prepare(self, n_steps: int) -> None:
        """Render the depth frames of the next ``n_steps`` steps now (rooms world), so that a timed region that follows
        finds its inputs resident in HBM, as the benchmark contract asks."""
        if self.closed_loop:
            return      # nothing to pre-render: the poses of the coming steps depend on the actions still to be taken
        if self.rooms is not None:
            self.rooms.prepare(self.t % self.episode_len, n_steps)

    def current_depth(self, n: int) -> torch.Tensor:
        """The depth frames of the first ``n`` environments at the current step (diagnostics: bench.count_stored_cells)."""
        if self.closed_loop:
            return self.live.observe(self.rooms.painter, self.t % self.episode_len, fresh=True)[:n]
        if self.rooms is not None:
            return self.rooms.frame(self.t % self.episode_len)[:n]
        return self.depth_pool[self.t % self.depth_pool.shape[0]][:n].to(self.device)

    def fast_forward(self, n_steps: int) -> None:
        """Advance every episode by ``n_steps`` MAP-ONLY steps (stub cosines instead of the BLIP-2 forward, no detector /
        segmenter / controller): brings explored area, obstacle planes and contour lengths to a mid-episode state cheaply
        before a measurement, instead of timing the empty world of an episode's first steps."""
        saved = (self.blip2, self.detector, self.sam, self.selectors, self.pointnav, self.object_maps)
        self.blip2 = self.detector = self.sam = self.selectors = self.pointnav = self.object_maps = None
        if self.closed_loop:
            # the decision is host logic and stays (only the models are stubbed): without it the robots would stand still.  The
            # actions come from ``controller`` for these steps
            self.selectors = saved[3]
        try:
            for _ in range(n_steps):
                self.step()
        finally:
            self.blip2, self.detector, self.sam, self.selectors, self.pointnav, self.object_maps = saved

    def render(self, env_ids: Optional[Sequence[int]] = None, rgb: bool = True) -> Dict[str, "torch.Tensor"]:
        """The value and obstacle map frames of the chosen environments (all by default) as ValueMap.visualize /
        ObstacleMap.visualize draw them: device uint8 [n, S, S, 3] tensors, RGB by default (BGR with ``rgb=False``).  The
        agent's path and marker are drawn when the harness was built with ``render_trajectories=True``; the obstacle
        frames carry the current frontier circles.  Not part of the timed step."""
        env = list(range(self.E)) if env_ids is None else [int(e) for e in env_ids]
        main = torch.cuda.current_stream(self.device)
        if self.map_stream is not None:
            main.wait_stream(self.map_stream)   # obstacle planes and trajectories are written on the map stream
        if self.exploration_thresh is None:
            out = {"value_map": self.values.render(env, rgb=rgb)}
        else:     # the visual reducer ITMPolicyV3.__init__ installs (itm_policy.py:275-287)
            out = {"value_map": self.values.render(env, reduce=("explore", float(self.exploration_thresh)), rgb=rgb)}
        if self.obstacles is not None:
            out["obstacle_map"] = self.obstacles.render(env, rgb=rgb)
        return out

    def render_jpeg(self, env_ids: Optional[Sequence[int]] = None, quality: int = 90) -> Dict[str, List[bytes]]:
        """``render()`` as JPEG files: for each map the frames of the chosen environments (all by default), every one the
        bytes ``Image.fromarray(frame).save(format="JPEG", quality=quality, subsampling="4:2:0")`` writes for the RGB frame
        ``render()`` returns, encoded on the device (transport.jpeg_encode_batch_bytes) so that only the files cross to
        the host.  Not part of the timed step."""
        from .vlm.transport import jpeg_encode_batch_bytes

        return {name: jpeg_encode_batch_bytes(frames.contiguous(), quality, "rgb") for name, frames in self.render(env_ids).items()}

    def frontier_stats(self):
        """(mean, max) number of frontiers per environment at the last step (what the obstacle pipeline is working on)."""
        if self.obstacles is None or not self.obstacles.frontiers_ready:
            return None
        n = self.obstacles._h_counts.numpy()[:, 0]
        return [round(float(n.mean()), 2), int(n.max())]

    def check(self) -> None:
        """Raise what the reference would have raised inside the steps since the last check: IndexError for an obstacle
        point off the map (obstacle_map.py:101; the policy turns it into STOP, base_objectnav_policy.py:157-162), RuntimeError
        for an exhausted scratch capacity (never a silent wrong map).  Frontier-pipeline overflows already raise on the
        per-step frontier read-back; this adds the sticky flags of the depth passes.  One small D2H copy + sync: called
        at every episode end by step() and by the benchmark after its timed region, not per step."""
        if self.obstacles is not None:
            self.obstacles.check_status()
        if self.blip2 is not None and hasattr(self.blip2, "check_numerics"):
            self.blip2.check_numerics()
        if self.sam is not None and hasattr(self.sam, "check_numerics"):
            self.sam.check_numerics()

    def _log_finished_episodes(self) -> None:
        """One JSON file per finished episode in the reference's log format (vlfm/utils/log_saver.py:9-22) when
        ZSOS_LOG_DIR is set: what the reference's eval loop writes through episode_stats_logger.log_episode_stats."""
        if "ZSOS_LOG_DIR" not in os.environ:
            return
        from .utils.log_saver import is_evaluated, log_episode

        n_fr = self.obstacles.frontiers_px() if self.obstacles is not None and self.obstacles.frontiers_ready else None
        best = [None] * self.E
        if self.last_frontier_values is not None and len(self.last_frontier_values):
            if self.exploration_thresh is None:      # (single prompt: the batch-wide maximum, as it always was)
                best = [float(np.max(self.last_frontier_values))] * self.E
            else:     # V3's rule is per environment: the best value of ITS frontiers after ITS reduction
                from .policy_step import explore_reduce_values

                v, env_of = np.asarray(self.last_frontier_values).reshape(-1, self.C), np.asarray(self.last_frontier_envs)
                for e in range(self.E):
                    mine = v[env_of == e]
                    if len(mine):
                        best[e] = float(max(explore_reduce_values(mine.tolist(), self.exploration_thresh)))
        # closed loop: where the robot ended up, not where the plan would have had it
        final = self._poses_tf(0)[0] if self.closed_loop else self.pose_table[(self.t - 1) % self.episode_len]
        for e, env_id in enumerate(self.env_ids):
            episode_id = self.episodes_done * len(self.env_ids) + e
            scene = f"synthetic{env_id:04d}"
            if is_evaluated(episode_id, scene):
                continue
            log_episode(episode_id, scene, {
                "target_object": self.targets[e], "num_steps": int(self.episode_len),
                "final_pose": [float(v) for v in final[e]],
                "num_frontiers": int(len(n_fr[e])) if n_fr is not None else 0,
                "best_frontier_value_last_step": best[e]})

    def _detect(self, rgb: torch.Tensor, t_ep: int):
        """The detector on the frames ``rgb`` [E,H,W,3] of episode step ``t_ep`` (one frame per environment) -> per-environment
        ObjectDetections, or None without a detector and without a scripted head."""
        # YOLOv7 takes the frames alone; GroundingDINO is prompted (MP3D-style caption, habitat_policies.py:139-141)
        scripted = (self.sightings is not None or self.world_objects is not None) and \
            (self.detector is not None or self.object_maps is not None)
        if self.detector is None:
            d = None
        elif self.detector_is_prompted:
            d = self.detector.predict_batch(rgb, [self.gdino_caption])
        elif scripted and self.scripted_through_nms and hasattr(self.detector, "in_hw"):
            # the scripted head speaks THROUGH the detector's own post-processing: its candidates (a cluster of jittered boxes
            # per sighting, the scripted confidence on the best one) are written into the network's raw prediction, and
            # non_max_suppression / scale_coords / the rounding and normalisation of yolov7.py:91-110 produce the detections
            d = self.detector.predict_batch(rgb, pred_hook=lambda pred, in_hw: self._inject_candidates(pred, in_hw, t_ep))
            want = [0] * self.E
            for sg in self._sightings_at(t_ep):
                want[sg[0]] += 1
            self.object_stats["head_mismatch"] = self.object_stats.get("head_mismatch", 0) + sum(
                int(det.num_detections != w) for det, w in zip(d, want))
            return d
        else:
            d = self.detector.predict_batch(rgb)
        if scripted:
            d = self._scripted_detections(t_ep)     # the scripted HEAD: the network above ran (and is timed), its random logits are not used
        return d

    def rig_observations(self, t_ep: int):
        """The rig's observations of episode step ``t_ep``: (frames [E*K,H,W] device f32, camera transforms [E*K,4,4], slot of
        each frame [E*K], camera index of each frame [E*K]) -- environment-major, cameras in rig order."""
        K = len(self.rig)
        tf = self.rig.camera_tfs(self._poses_tf(t_ep)[1]).reshape(self.E * K, 4, 4)
        cam = np.tile(np.arange(K), self.E)
        hf = np.array([self.fov if c.hfov is None else c.hfov for c in self.rig.cameras])[cam]
        lo, hi = (np.array([getattr(c, a) for c in self.rig.cameras], np.float64)[cam] for a in ("min_depth", "max_depth"))
        frames = self.rooms.cast_cameras(tf, hf, lo, hi)
        if self.rooms.painter is not None:     # scripted objects: in front of the DESIGNATED camera (the detector stage's frame)
            d_idx = torch.from_numpy(np.arange(self.E) * K + self.rig.designated).to(self.device)
            frames[d_idx] = self.rooms.painter(t_ep, frames[d_idx])
        return frames, tf, np.repeat(np.arange(self.E), K), cam

    # ---- closed loop: the live poses, the frames seen from them, the world's answer to the step's actions
    def _poses_tf(self, t_ep: int):
        """(poses [E,3] = x, y, yaw; robot -> episodic transforms [E,4,4]) of this step: the planned tour's at episode step
        ``t_ep``, or, closed-loop, where the robots are."""
        return (self.pose_table[t_ep], self.tf_table[t_ep]) if self.live is None else self.live.poses_tf()

    def _advance_world(self, poses: np.ndarray) -> None:
        """Closed loop, after the policy acted: the step's actions -- PointNav's discrete ids with the policy's TURN_LEFT / STOP
        overrides, else ``controller``'s -- move the robots (LiveWorld.advance); ``poses``: where the step observed from."""
        controller, collided = self.controller, self.live.collided
        if self.pointnav is not None and self.last_actions is not None:
            acts = self.last_actions.detach().reshape(self.E).cpu().numpy().astype(np.int64)
        elif hasattr(controller, "act_on_map"):
            # a controller that plans over the navigable planes (synthetic.MapPlannerController): on the main stream, which
            # joined the map stream before the value update; an object goal may be entered up to the stop radius
            navigate = np.array([m == "navigate" for m in self.last_modes], bool)
            goal_free = [self.stop_radius if nav else None for nav in navigate]
            acts = controller.act_on_map(self.obstacles, poses, self.last_goals, goal_free, self.last_modes, self.last_rho_theta,
                                         self.last_stops, collided)
            status = np.asarray(controller.last_status)
            ps = self.planner_stats
            ps["plans"] += status >= 0
            ps["ok"] += status == PLAN_OK
            ps["unreachable"] += status == PLAN_UNREACHABLE
            ps["too_long"] += status == PLAN_TOO_LONG
            ps["invalid"] += status == PLAN_INVALID
        else:
            acts = controller.act(self.last_modes, self.last_rho_theta, self.last_stops, collided)
        self.last_poses, self.last_world_actions = np.array(poses, np.float64), self.live.advance(acts, self.last_episode_end)

    # ---- the pieces step() and _step_rig() share; each enqueues on the stream that is current when it is called
    def _transported(self, rgb: torch.Tensor) -> torch.Tensor:
        """The step's RGB frames after the JPEG transport hop, when it is emulated (main stream: every reader of the previous
        step's transported frames ran on it or was joined back into it)."""
        if not self.emulate_jpeg:
            return rgb
        from .vlm.transport import jpeg_roundtrip_batch

        return jpeg_roundtrip_batch(rgb, 90, out=self.jpeg_frames, scratch=self.jpeg_scratch)

    def _open_step(self, poses):
        """(main, side) streams of a step, the side stream joined to the main one (the previous step's value update consumed
        the column-max keys), after BaseMap.update_agent_traj of both maps (base_objectnav_policy / itm_policy)."""
        main = torch.cuda.current_stream(self.device)
        side = self.map_stream if self.map_stream is not None else main
        if self.render_trajectories:      # one pose per slot and step: the robot's
            self.values.update_agent_traj(range(self.E), poses[:, :2], poses[:, 2])
        side.wait_stream(main)
        if self.render_trajectories and self.obstacles is not None:
            with torch.cuda.stream(side):
                self.obstacles.update_agent_traj(range(self.E), poses[:, :2], poses[:, 2])
        return main, side

    def _cosines(self, rgb: torch.Tensor, prompts, graphed: bool = False) -> torch.Tensor:
        """One batched BLIP-2 ITC forward: [n] cosines for one prompt per frame, [n, C] for C prompts per frame (every prompt
        of every frame from one vision forward); ``graphed``: replayed from a captured graph."""
        if self.C == 1:
            return self.blip2.cosine_batch_graphed(rgb, prompts) if graphed else self.blip2.cosine_batch(rgb, prompts)
        return (self.blip2.cosine_prompts_batch_graphed(rgb, prompts) if graphed
                else self.blip2.cosine_prompts_batch(rgb, prompts))

    def _stub_cosines(self, n: int) -> torch.Tensor:
        """What stands in for the cosines of ``n`` frames without a model."""
        return torch.from_numpy(self.stub_rng.uniform(0.15, 0.45, size=n if self.C == 1 else (n, self.C))).to(self.device)

    def _fixed_box_sam(self, rgb: torch.Tensor) -> None:
        """(legacy leg without object maps: MobileSAM on one fixed box for every ``sam_every``-th environment-step)"""
        sel = [e for e in range(self.E) if (self.t + e) % self.sam_every == 0]
        if sel:
            box = torch.tensor([[[0.3 * self.W, 0.3 * self.H, 0.7 * self.W, 0.8 * self.H]]] * len(sel))
            self.last_masks = self.sam.segment_bboxes(rgb[sel], box)

    def _score_and_act(self, wps, env_of, poses, t_ep: int, nav_depth) -> None:
        """After the value update: frontier scoring (ITMPolicyV2._sort_frontiers_by_value, radius 0.5 m), the policy's decision,
        navigation on the frames ``nav_depth()`` [E,H,W], the end of the episodes; the step is over."""
        self.last_frontier_values, self.last_frontier_envs = None, env_of
        if len(wps):
            self.last_frontier_values = self.values.waypoint_values(wps, env_of, 0.5)  # D2H sync: the policy needs it
        if self.selectors is not None:
            modes, goals, halt = self._decide(wps, env_of, self.last_frontier_values, poses, t_ep)
            self.last_modes, self.last_goals = modes, goals
            self.last_actions = self._navigate(nav_depth(), modes, goals, halt, poses)
            self.object_stats["env_steps"] += self.E
            for m in modes:
                self.object_stats["modes"][m] += 1
        self._end_episodes(t_ep)
        self.t += 1

    def _step_rig(self) -> None:
        """step() for a camera rig: K * E frames rendered, ONE depth pass over the obstacle cameras' frames (which also reduces
        the column maxima of the value cameras among them), one obstacle pipeline call per slot from the robot pose, one BLIP-2
        batch over the K_v * E value frames, ONE value-map launch in which each slot fuses its cameras in rig order."""
        t_ep = self.t % self.episode_len
        rig, E = self.rig, self.E
        cams = rig.cameras
        poses, tf_robot = self._poses_tf(t_ep)
        depth, tf, slot, cam = self.rig_observations(t_ep)
        per = lambda f: np.array([f(c) for c in cams])[cam]   # noqa: E731
        lo, hi = per(lambda c: c.min_depth), per(lambda c: c.max_depth)
        hfov = per(lambda c: self.fov if c.hfov is None else c.hfov)
        fx = self.W / (2 * np.tan(hfov / 2))
        is_o, is_v = per(lambda c: c.obstacle), per(lambda c: c.value)
        o_idx, v_idx = np.flatnonzero(is_o), np.flatnonzero(is_v)
        v_only = np.flatnonzero(is_v & ~is_o)
        self.last_rig = (depth, tf, slot, cam)
        main, side = self._open_step(poses)
        with torch.cuda.stream(side):
            d_o = depth if len(o_idx) == len(slot) else depth[torch.from_numpy(o_idx).to(self.device)]
            keys_o = self.obstacles.ingest_cameras(d_o, tf[o_idx], lo[o_idx], hi[o_idx], fx[o_idx], fx[o_idx], slot[o_idx],
                                                   want_colmax=True)
            # the reveal: the robot pose, the widest obstacle camera's range and field of view
            self.obstacles.update_after_ingest(tf_robot, float(hi[o_idx].max()), float(hfov[o_idx].max()))
            # key rows in value-camera order: rows of the shared pass for cameras that feed both maps, a column-max-only pass
            # for the value-only ones; both key buffers are handed back zeroed, as a value update would
            if self._rig_keys is None:
                self._rig_keys = torch.zeros((len(v_idx), self.W), dtype=torch.int32, device=self.device)
                row_o, row_v = {int(i): r for r, i in enumerate(o_idx)}, {int(i): r for r, i in enumerate(v_only)}
                pick = lambda rows: [torch.tensor(x, dtype=torch.int64, device=self.device) for x in   # noqa: E731
                                     ([r for r, i in enumerate(v_idx) if int(i) in rows],
                                      [rows[int(i)] for i in v_idx if int(i) in rows])]
                self._rig_gather = (pick(row_o), pick(row_v))
            (dst_o, src_o), (dst_v, src_v) = self._rig_gather
            if len(dst_o):
                self._rig_keys[dst_o] = keys_o[src_o]
            keys_o.zero_()
            if len(v_only):
                keys_v = self.values.column_max(depth[torch.from_numpy(v_only).to(self.device)])
                self._rig_keys[dst_v] = keys_v[src_v]
                keys_v.zero_()
        # ---- the transport hop on the pool frames: every camera's frame is one of them (the synthetic RGB pool has one frame
        # per environment: the designated camera of environment e sees pool frame e, camera k pool frame (e + k - designated) mod E)
        n_v = len(v_idx)
        pool = self._transported(self.rgb_pool[self.t % self.rgb_pool.shape[0]])
        # ---- detector / segmenter / object maps: ONE designated camera per environment, as object_map_rgbd on the robot
        # (reality_policies.py:103-111) -- the single-camera stage on that camera's RGB frame, depth frame and pose
        d_rows = np.arange(E) * len(rig) + rig.designated
        dets = self._detect(pool, t_ep)
        self.last_detections = dets
        if self.object_maps is not None and dets is not None:
            self._update_object_maps(dets, pool, depth[torch.from_numpy(d_rows).to(self.device)], tf[d_rows])
        elif self.sam is not None:
            self._fixed_box_sam(pool)
        # ---- perception: one batch over the value cameras' frames
        if self.blip2 is not None:
            rgb = pool[torch.from_numpy((slot[v_idx] + cam[v_idx] - rig.designated) % E).to(self.device)]
            cos = self._cosines(rgb, [self.prompts[e] for e in slot[v_idx]])
        else:
            cos = self._stub_cosines(n_v)
        self.last_cosines = cos
        with torch.cuda.stream(side):
            wps, env_of = self.obstacles.frontier_list()
        main.wait_stream(side)
        self.values.update_cameras(cos.reshape(n_v, self.C), None, tf[v_idx], lo[v_idx], hi[v_idx], hfov[v_idx], slot[v_idx],
                                   colmax=self._rig_keys)
        self._score_and_act(wps, env_of, poses, t_ep, lambda: depth[torch.from_numpy(d_rows).to(self.device)])
        if self.closed_loop:
            self._advance_world(poses)

    def step(self) -> None:
        if self.t and self.t % self.episode_len == 0:
            self.check()
            self._log_finished_episodes()
            self.episodes_done += 1
            self.reset()
        if self.rig is not None:
            return self._step_rig()
        k = self.t % self.depth_pool.shape[0]
        kr = self.t % self.rgb_pool.shape[0]
        if self.host_inputs:
            depth = self.depth_dev.copy_(self.depth_pool[k], non_blocking=True)
            rgb = self.rgb_dev.copy_(self.rgb_pool[kr], non_blocking=True)
        elif self.closed_loop:
            depth, rgb = None, self.rgb_pool[kr]       # rendered below, from the live poses
        elif self.rooms is not None:
            depth, rgb = self.rooms.frame(self.t % self.episode_len), self.rgb_pool[kr]
        else:
            depth, rgb = self.depth_pool[k], self.rgb_pool[kr]
        if not self.render_rgb:
            rgb = self._transported(rgb)
        t_ep = self.t % self.episode_len
        poses, tf = self._poses_tf(t_ep)
        if self.closed_loop:
            depth = self.live.observe(self.rooms.painter, t_ep, tf=tf)
            if self.render_rgb:                        # the frames of the launch that gave the depth, then the transport hop
                rgb = self._transported(self.live.rgb)
        # ---- mapping, part 1 (side stream): one depth pass feeds both maps, then the obstacle/frontier pipeline
        main, side = self._open_step(poses)
        with torch.cuda.stream(side):
            if self.obstacles is not None:
                colmax = self.obstacles.ingest(depth, tf, MIN_DEPTH, MAX_DEPTH, self.fx, self.fy, want_colmax=True)
                self.obstacles.update_after_ingest(tf, MAX_DEPTH, self.fov)
            else:
                colmax = self.values.column_max(depth)
        # ---- detector (main stream).  With the object maps switched on it goes FIRST: its read-back is the step's first host
        # synchronisation anyway, and what follows it -- MobileSAM on the surviving boxes and one ObjectPointCloudMap.update_map per
        # mask, each a few small kernels and two host read-backs -- then runs on its own stream WHILE the BLIP-2 forward occupies the
        # GPU (17 ms of mostly idle GPU per 128-environment step before).  No result depends on the order: BLIP-2 sees the frames only.
        detector_first = self.detector is not None and self.object_maps is not None and self.obj_stream is not None
        dets = cos = None
        vlm_beside = detector_first and self.vlm_stream is not None and self.blip2 is not None
        if vlm_beside:
            self.vlm_stream.wait_stream(main)          # (the frames of this step are complete on the main stream)
            with torch.cuda.stream(self.vlm_stream):
                cos = self._cosines(rgb, self.prompts, self.graph_blip2)
        if detector_first:
            dets = self._detect(rgb, t_ep)
        # ---- perception (main stream): one batched BLIP-2 ITC forward for all resident envs
        if cos is None:
            cos = self._cosines(rgb, self.prompts, self.graph_blip2) if self.blip2 is not None else self._stub_cosines(self.E)
        self.last_cosines = cos
        if not detector_first:
            dets = self._detect(rgb, t_ep)
        self.last_detections = dets
        if self.object_maps is not None and dets is not None:
            if detector_first:
                # (the frames were complete when the detector's read-back returned; nothing else on the main stream is an input)
                with torch.cuda.stream(self.obj_stream):
                    self._update_object_maps(dets, rgb, depth, tf)
                main.wait_stream(self.obj_stream)   # the next step may not repaint the frames under the segmenter
            else:
                self._update_object_maps(dets, rgb, depth, tf)
        elif self.sam is not None:
            self._fixed_box_sam(rgb)
        # ---- frontiers back to the host (the policy needs them); waits for the side stream only, so the host-side
        # prologue of the value update overlaps the GPU's BLIP-2 work
        if self.obstacles is not None and self.obstacles.frontiers_ready:
            with torch.cuda.stream(side):
                wps, env_of = self.obstacles.frontier_list()
        else:
            ang = np.linspace(0, 2 * np.pi, self.n_frontiers, endpoint=False)
            wps = (poses[:, None, :2] + 1.5 * np.stack([np.cos(ang[None, :] + poses[:, 2:3]),
                                                        np.sin(ang[None, :] + poses[:, 2:3])], axis=2)).reshape(-1, 2)
            env_of = np.repeat(np.arange(self.E), self.n_frontiers)
        # ---- mapping, part 2 (main stream): value-map fusion needs the cosines and the column maxima
        main.wait_stream(side)
        if vlm_beside:
            main.wait_stream(self.vlm_stream)          # the cosines; and the next step may not repaint the frames under the ViT
            cos.record_stream(main)
        self.values.update(cos.reshape(self.E, self.C), None, tf, MIN_DEPTH, MAX_DEPTH, self.fov, colmax=colmax)
        self._score_and_act(wps, env_of, poses, t_ep, lambda: depth)
        if self.closed_loop:
            self._advance_world(poses)
