"""vlfm.mapping.object_point_cloud_map.ObjectPointCloudMap, MI355X-native
(reference: /root/reference/vlfm/mapping/object_point_cloud_map.py:17-297).

The heavy lifting of a detection -- mask erosion, masked back-projection, DBSCAN + largest-cluster selection
(``_extract_object_cloud``, :150-170) -- runs in HIP kernels (csrc/object_cloud.hip) that take all detections of a step at once
(``extract_object_clouds_batch`` / ``update_maps_batch``); ``update_map`` is a batch of one job.  The bookkeeping around it (range
ids, closest point, ``get_best_object`` hysteresis, ``update_explored``) is O(points kept) NumPy on the host exactly as in the
reference, INCLUDING its draws from NumPy's global RNG (``np.random.choice`` for the 5000-point subsample,
``np.random.rand`` for the out-of-range ids), so that a seeded run reproduces the reference's clouds.

The two questions asked of the ACCUMULATED clouds in every step -- which far tags are now in view (``update_explored``) and where
the closest point is (``get_best_object``) -- can also be asked of many maps at once: every map keeps a device mirror of its
clouds (``CloudMirror``), and ``update_explored_batch`` / ``get_best_objects_batch`` (csrc/cloud_query.hip) answer them with one
launch and one read-back per call.  The host arrays stay the source of truth, and what changes them stays host code."""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from .. import _lib
from .base_map import require_gpu
from .value_map import _stream_ptr


def extract_yaw(matrix: np.ndarray) -> float:
    return float(np.arctan2(matrix[1, 0], matrix[0, 0]))  # geometry_utils.py:145-159


def transform_points(transformation_matrix: np.ndarray, points: np.ndarray) -> np.ndarray:
    """geometry_utils.py:205-213."""
    h = np.hstack((points, np.ones((points.shape[0], 1))))
    t = np.dot(transformation_matrix, h.T).T
    return t[:, :3] / t[:, 3:]


def within_fov_cone(cone_origin, cone_angle, cone_fov, cone_range, points) -> np.ndarray:
    """geometry_utils.py:91-116."""
    directions = points[:, :3] - cone_origin
    dists = np.linalg.norm(directions, axis=1)
    angles = np.arctan2(directions[:, 1], directions[:, 0])
    angle_diffs = np.mod(angles - cone_angle + np.pi, 2 * np.pi) - np.pi
    mask = np.logical_and(dists <= cone_range, np.abs(angle_diffs) <= cone_fov / 2)
    return points[mask]


def too_offset(mask) -> bool:
    """Does the detection hug the left or right image border (object_point_cloud_map.py:272-297)?  A mask whose column
    extent lies wholly in the outer third of the image AND reaches within 5 % of that border is "too offset": its
    points get an out-of-range tag because the object is probably cut off by the image edge.  ``mask``: (H,W) ndarray."""
    width = mask.shape[1]
    occupied = np.flatnonzero(np.asarray(mask).any(axis=0))           # cv2.boundingRect's x-extent
    left, right = (int(occupied[0]), int(occupied[-1]) + 1) if len(occupied) else (0, 0)
    return extent_too_offset(left, right, width)


def extent_too_offset(left: int, right: int, width: int) -> bool:
    """``too_offset`` from the mask's column extent [left, right) -- (0, 0) for an empty mask."""
    band = width // 3
    if right <= band:
        return left <= int(0.05 * width)
    if left >= 2 * band:
        return right >= int(0.95 * width)
    return False


SUBSAMPLE = 5000                   # get_random_subarray's size (:165)
DBSCAN_EPS, DBSCAN_MIN_POINTS = 0.2, 100
DEFAULT_SCRATCH_BUDGET = 256 << 20
SYNCS = [0]                        # host read-backs made by this module so far (tools/world_objects_probe.py)
UPLOADED_BYTES = [0]               # bytes of cloud rows and slots copied to device mirrors so far
BAND_POINTS = [0]                  # points update_explored_batch re-evaluated on the host (slots the device left uncertain)
CONE_BAND = 1e-9                   # rad: csrc/cloud_query.hip's CQ_BAND
MIRROR_MIN_ROWS = 1024


class CloudMirror:
    """What one map knows about the cloud stored under one class name beyond the host array itself: one i32 SLOT per point (-1 for
    tag 1.0, else the index of the tag in ``table``, the distinct other tags in order of first appearance) and a device copy of
    the first ``on_device`` rows and slots.  Valid only for the very array ``key`` = (id, rows) names; ``array`` holds that array
    so that its id cannot be handed to another one meanwhile."""

    __slots__ = ("key", "array", "slots", "table", "index", "rows_d", "slots_d", "on_device")

    def __init__(self, array: np.ndarray, slots: np.ndarray, table: List[float]) -> None:
        self.key, self.array = (id(array), len(array)), array
        self.slots, self.table = slots, list(table)
        self.index = {t: i for i, t in enumerate(self.table)}
        self.rows_d = self.slots_d = None
        self.on_device = 0

    def rebind(self, array: np.ndarray, slots: np.ndarray) -> None:
        self.key, self.array, self.slots = (id(array), len(array)), array, slots

    def slot_of(self, tag: float) -> int:
        if tag not in self.index:
            self.index[tag] = len(self.table)
            self.table.append(tag)
        return self.index[tag]


def block_slots(tags: np.ndarray, slot_of) -> np.ndarray:
    """Slots of one committed block, whose tags are 1.0 and / or ONE other value: ``slot_of(value)`` names that value's slot."""
    far = tags != 1
    slots = np.full(len(tags), -1, np.int32)
    if far.any():
        slots[far] = slot_of(float(tags[np.argmax(far)]))
    return slots


def slots_of_array(tags: np.ndarray) -> Tuple[np.ndarray, List[float]]:
    """(slots, table) of an array nothing is known about: -1 for tag 1.0, the other values numbered by first appearance."""
    slots = np.full(len(tags), -1, np.int32)
    far = np.flatnonzero(tags != 1)
    if len(far) == 0:
        return slots, []
    values, first, inverse = np.unique(tags[far], return_index=True, return_inverse=True)
    rank = np.empty(len(values), np.int32)
    order = np.argsort(first, kind="stable")
    rank[order] = np.arange(len(values), dtype=np.int32)
    slots[far] = rank[inverse.reshape(-1)]
    return slots, [float(v) for v in values[order]]


def merge_cone_flags(inside: np.ndarray, uncertain: np.ndarray, decide) -> List[int]:
    """The slots to drop: those the device saw inside the cone, and of those it left uncertain (and did not also see inside) the
    ones for which ``decide(slot)`` -- the host's own evaluation of the slot's points -- says so.  Ascending."""
    inside, uncertain = np.asarray(inside) != 0, np.asarray(uncertain) != 0
    if inside.shape != uncertain.shape:
        raise ValueError("merge_cone_flags: one flag of each kind per slot")
    seen = set(np.flatnonzero(inside).tolist())
    seen.update(int(s) for s in np.flatnonzero(uncertain & ~inside) if decide(int(s)))
    return sorted(seen)


def apply_hysteresis(previous: Union[np.ndarray, None], candidate: np.ndarray, curr_position: np.ndarray) -> Tuple[np.ndarray, bool]:
    """get_best_object's rule (:82-100): (goal, whether the goal is the NEW candidate).  The previous goal is kept when the closest
    point moved < 0.1 m, or < 0.5 m while the robot is still more than 2 m away."""
    if previous is not None:
        moved = np.linalg.norm(candidate - previous)
        if moved < 0.1 or (moved < 0.5 and np.linalg.norm(curr_position - candidate) > 2.0):
            return previous, False
    return candidate, True


def get_random_subarray(points, size: int, rng=np.random):
    """At most ``size`` rows, chosen by NumPy's GLOBAL generator like the reference (:253-269), so a seeded session
    reproduces its clouds."""
    n = len(points)
    return points if n <= size else points[rng.choice(n, size, replace=False)]


class ObjectPointCloudMap:
    """Per object class: an (N, 4) cloud of episodic-frame points whose 4th column is a TAG -- 1.0 for points seen within
    95 % of the depth range, otherwise one random number per observation (so that all far points of an observation can be
    dropped together once the robot looks there from nearby, ``update_explored``)."""

    clouds: Dict[str, np.ndarray] = {}
    use_dbscan: bool = True

    def __init__(self, erosion_size: float, device=None, rng=None) -> None:
        """``rng``: where the two random draws come from.  Default = NumPy's GLOBAL generator, like the reference; the batched
        harness gives every environment its own ``np.random.RandomState(seed)`` (same stream as ``np.random.seed(seed)``
        followed by the global calls), so that E interleaved episodes each reproduce their single-environment run."""
        self._erosion_size = erosion_size
        self._rng = rng if rng is not None else np.random
        self.last_target_coord: Union[np.ndarray, None] = None
        self.device = require_gpu(device)
        _lib.lib()
        self.clouds = {}
        self._bufs = None
        self._near_only: Dict[str, tuple] = {}     # name -> (id(cloud array), rows): every tag of that array is 1.0
        self._mirrors: Dict[str, CloudMirror] = {}  # name -> slots and device copy of the array stored under that name

    def reset(self) -> None:
        self.clouds, self.last_target_coord = {}, None
        self._near_only = {}
        self._mirrors = {}

    def _all_near(self, name: str) -> bool:
        """True when the cloud stored under ``name`` is known to hold only trusted (tag 1.0) points -- bookkeeping of update_map /
        update_explored, valid only for the very array it was recorded for (``clouds`` is a public dict)."""
        cloud = self.clouds.get(name)
        return cloud is not None and self._near_only.get(name) == (id(cloud), len(cloud))

    def has_object(self, target_class: str) -> bool:
        return len(self.clouds.get(target_class, ())) > 0

    def update_map(self, object_name: str, depth_img: np.ndarray, object_mask: np.ndarray,
                   tf_camera_to_episodic: np.ndarray, min_depth: float, max_depth: float, fx: float, fy: float) -> None:
        """object_point_cloud_map.py:29-75: ``update_maps_batch`` with this detection as its one job."""
        update_maps_batch([self], [object_name], *_one_job(depth_img, object_mask), [tf_camera_to_episodic], min_depth, max_depth,
                          fx, fy)

    def _commit(self, object_name: str, camera_frame: np.ndarray, is_too_offset, tf_camera_to_episodic: np.ndarray,
                max_depth: float) -> None:
        """Everything of ``update_map`` after the camera-frame cloud is on the host (:40-75).  ``is_too_offset``: called (once) only
        for a non-empty cloud."""
        if len(camera_frame) == 0:
            return
        # exactly ONE draw from the global generator per non-empty observation, whichever branch is taken (the reference
        # evaluates np.random.rand() on both paths); the "near" path keeps its tags in f32 like the reference's astype
        tag = self._rng.rand()
        if is_too_offset():
            tags = np.full(len(camera_frame), tag, dtype=camera_frame.dtype)
        else:
            near = camera_frame[:, 0] <= max_depth * 0.95
            tags = np.where(near, np.float32(1.0), np.float32(tag)).astype(np.float32)
        tagged = np.concatenate((transform_points(tf_camera_to_episodic, camera_frame), tags[:, None]), axis=1)
        here = tf_camera_to_episodic[:3, 3]
        if np.linalg.norm(self._get_closest_point(tagged, here)[:3] - here) < 1.0:
            return  # closer than 1 m: depth this near is not trusted (:63-67)
        known = self.clouds.get(object_name)
        near_only = (known is None or self._all_near(object_name)) and bool(np.all(tags == 1))
        self.clouds[object_name] = tagged if known is None else np.concatenate((known, tagged), axis=0)
        self._mirror_commit(object_name, known, tagged)
        if near_only:
            self._near_only[object_name] = (id(self.clouds[object_name]), len(self.clouds[object_name]))
        else:
            self._near_only.pop(object_name, None)

    def get_best_object(self, target_class: str, curr_position: np.ndarray) -> np.ndarray:
        """Goal point with hysteresis (:77-101): keep the previous goal when the new closest point moved < 0.1 m, or
        < 0.5 m while the robot is still more than 2 m away."""
        # (a cloud of trusted points only IS its target cloud: no copy, no mask -- the harness asks this for every environment
        # and step, on clouds of 10^5 points)
        cloud = self.clouds[target_class] if self._all_near(target_class) else self.get_target_cloud(target_class)
        return self._goal_with_hysteresis(self._get_closest_point(cloud, curr_position)[:2], curr_position)

    def _goal_with_hysteresis(self, candidate: np.ndarray, curr_position: np.ndarray) -> np.ndarray:
        goal, is_new = apply_hysteresis(self.last_target_coord, candidate, curr_position)
        if is_new:
            self.last_target_coord = candidate
        return goal

    def update_explored(self, tf_camera_to_episodic: np.ndarray, max_depth: float, cone_fov: float) -> None:
        """Forget far-tagged observations the robot is now looking at from within half the depth range (:103-135): every
        tag other than 1 that shows up inside the view cone is removed from the cloud as a whole."""
        origin, heading = tf_camera_to_episodic[:3, 3], extract_yaw(tf_camera_to_episodic)
        for name, cloud in list(self.clouds.items()):
            if self._all_near(name):
                continue       # only tags other than 1 can be dropped (`- {1}` below): nothing to do, same result
            self._explore_cloud(name, cloud, origin, heading, max_depth, cone_fov)

    def _explore_cloud(self, name: str, cloud: np.ndarray, origin: np.ndarray, heading: float, max_depth: float,
                       cone_fov: float) -> bool:
        """``update_explored`` for one cloud on the host; whether a tag was dropped."""
        seen_tags = set(within_fov_cone(origin, heading, cone_fov, max_depth * 0.5, cloud)[..., -1].tolist()) - {1}
        self._drop_tags(name, cloud, seen_tags)
        return bool(seen_tags)

    def _drop_tags(self, name: str, cloud: np.ndarray, seen_tags) -> None:
        """Remove every point of ``cloud`` (the array stored under ``name``) that carries one of ``seen_tags`` (:127-132), and keep
        the mirror's slots in step with the same masks; the device copy is stale afterwards and is uploaded again in full."""
        mirror = self._mirror_for(name, cloud)
        slots = mirror.slots if mirror is not None else None
        for t in seen_tags:
            keep = cloud[..., -1] != t
            cloud = cloud[keep]
            if slots is not None:
                slots = slots[keep]
        self.clouds[name] = cloud
        if mirror is not None and seen_tags:
            mirror.rebind(cloud, slots)
            mirror.on_device = 0
        elif mirror is None:
            self._mirrors.pop(name, None)

    # ------------------------------------------------------------------------------------------ device mirror
    def _mirror_for(self, name: str, cloud: np.ndarray) -> Optional[CloudMirror]:
        """The mirror of ``name`` if it describes exactly ``cloud``, else None."""
        mirror = self._mirrors.get(name)
        return mirror if mirror is not None and mirror.key == (id(cloud), len(cloud)) else None

    def _mirror_commit(self, name: str, known: Union[np.ndarray, None], tagged: np.ndarray) -> None:
        """``clouds[name]`` has just become ``known`` + ``tagged``: record that, and the block's slots.  No device work here -- the
        next batched query uploads the appended rows."""
        cloud, tags = self.clouds[name], tagged[:, -1]
        if known is None:
            mirror = CloudMirror(cloud, np.zeros(0, np.int32), [])
            mirror.rebind(cloud, block_slots(tags, mirror.slot_of))
            self._mirrors[name] = mirror
            return
        mirror = self._mirror_for(name, known)
        if mirror is None:
            self._mirrors.pop(name, None)      # an array this map did not build: looked at as a whole by the next query
            return
        mirror.rebind(cloud, np.concatenate((mirror.slots, block_slots(tags, mirror.slot_of))))

    def _mirror_sync(self, name: str) -> Optional[CloudMirror]:
        """Bring the device copy of ``clouds[name]`` up to date on the current stream and return its mirror -- None when the array
        cannot be mirrored (not an (N, 4) C-contiguous f64 array, or one holding a non-finite value): its queries take the host path."""
        import torch

        cloud = self.clouds[name]
        mirror = self._mirror_for(name, cloud)
        if mirror is None:
            self._mirrors.pop(name, None)
            if not (isinstance(cloud, np.ndarray) and cloud.dtype == np.float64 and cloud.ndim == 2 and cloud.shape[1] == 4
                    and cloud.flags.c_contiguous and bool(np.isfinite(cloud).all())):
                return None
            mirror = self._mirrors[name] = CloudMirror(cloud, *slots_of_array(cloud[:, -1]))
        n = len(cloud)
        if mirror.on_device == n and mirror.rows_d is not None:
            return mirror
        if mirror.rows_d is None or mirror.rows_d.shape[0] < n:
            rows = max(MIRROR_MIN_ROWS, 2 * mirror.rows_d.shape[0] if mirror.rows_d is not None else 0)
            while rows < n:
                rows *= 2
            old_rows, old_slots = mirror.rows_d, mirror.slots_d
            mirror.rows_d = torch.empty((rows, 4), dtype=torch.float64, device=self.device)
            mirror.slots_d = torch.empty(rows, dtype=torch.int32, device=self.device)
            if old_rows is not None and mirror.on_device:
                mirror.rows_d[:mirror.on_device].copy_(old_rows[:mirror.on_device])
                mirror.slots_d[:mirror.on_device].copy_(old_slots[:mirror.on_device])
                # the old blocks go back to the allocator with this stream's copies still queued
                old_rows.record_stream(torch.cuda.current_stream(self.device))
                old_slots.record_stream(torch.cuda.current_stream(self.device))
        lo = mirror.on_device
        mirror.rows_d[lo:n].copy_(torch.from_numpy(cloud[lo:n]))
        mirror.slots_d[lo:n].copy_(torch.from_numpy(mirror.slots[lo:n]))
        UPLOADED_BYTES[0] += (n - lo) * (32 + 4)
        mirror.on_device = n
        return mirror

    def get_target_cloud(self, target_class: str) -> np.ndarray:
        """The trusted (tag 1) points when there are any, else everything (:137-144)."""
        cloud = self.clouds[target_class].copy()
        trusted = cloud[:, -1] == 1
        return cloud[trusted] if np.any(trusted) else cloud

    # ------------------------------------------------------------------------------------------ :150-170 on the GPU
    def _extract_object_cloud(self, depth: np.ndarray, object_mask: np.ndarray, min_depth: float, max_depth: float,
                              fx: float, fy: float) -> np.ndarray:
        """The camera-frame cloud of one detection: ``extract_object_clouds_batch`` with one job.  ``depth``: H x W values (leading
        unit axes allowed), ``object_mask``: (H, W), non-zero = object; NumPy arrays or device tensors."""
        (_, cloud, _), = extract_object_clouds_batch([self], *_one_job(depth, object_mask), min_depth, max_depth, fx, fy)
        return cloud

    # ------------------------------------------------------------------------------------------ :172-183
    def _get_closest_point(self, cloud: np.ndarray, curr_position: np.ndarray) -> np.ndarray:
        """With DBSCAN-cleaned clouds: the nearest point.  Without: the median of the nearest quarter, measured from the
        position lifted to 0.5 m when it is 2-D (outlier-tolerant)."""
        k = curr_position.shape[0]
        if self.use_dbscan:
            return cloud[np.argmin(np.linalg.norm(cloud[:, :k] - curr_position, axis=1))]
        anchor = curr_position if k != 2 else np.concatenate((curr_position, np.array([0.5])))
        order = np.argsort(np.linalg.norm(cloud[:, :3] - anchor, axis=1))
        nearest_quarter = order[: int(0.25 * len(cloud))]
        pick = nearest_quarter[int(len(nearest_quarter) / 2)] if len(nearest_quarter) else 0
        return cloud[pick]


# ---------------------------------------------------------------------------------------------- all detections of a step
def _one_job(depth, mask):
    """(depth_frames, frame_index, masks) of the batch that holds one detection: the depth as one H x W frame, H and W being the
    mask's."""
    import torch

    H, W = mask.shape
    if not torch.is_tensor(mask):
        mask = np.asarray(mask) != 0
    if not torch.is_tensor(depth):
        depth = np.asarray(depth)
    return depth.reshape(1, H, W), [0], mask[None]


def plan_waves(generators: Sequence[int], needs_choice: Sequence[bool]) -> List[List[int]]:
    """Split jobs 0..D-1, in order, into waves whose random draws can be made as "all ``choice``s of the wave in job order, then
    all ``rand``s in job order" and still leave every generator with the draws of the reference's ``update_map`` calls made one
    after the other (per job: ``choice`` if the mask has more than 5000 points, then ``rand`` if the final cloud is not empty).
    ``generators``: one key per job, equal for jobs that share a generator (``id(rng)``).  A new wave starts at a job that needs
    a ``choice`` and whose generator already has an earlier job in the current wave -- that job's ``rand`` has to come first."""
    if len(generators) != len(needs_choice):
        raise ValueError("plan_waves: one generator key and one flag per job")
    waves: List[List[int]] = []
    seen: set = set()
    for j, (g, c) in enumerate(zip(generators, needs_choice)):
        if not waves or (c and g in seen):
            waves.append([])
            seen = set()
        waves[-1].append(j)
        seen.add(g)
    return waves


def dbscan_job_bytes(n: int) -> int:
    """vlfm_dbscan_batch_scratch_bytes: adjacency bit matrix + four [n] i32 arrays, rounded up to 256 bytes."""
    return 0 if n <= 0 else (n * ((n + 63) // 64) * 8 + 16 * n + 255) & ~255


def plan_chunks(job_bytes: Sequence[int], budget: int) -> List[List[int]]:
    """Consecutive runs of jobs whose DBSCAN scratch fits ``budget`` bytes together."""
    if budget < dbscan_job_bytes(SUBSAMPLE):
        raise ValueError(f"scratch_budget_bytes = {budget} is below the {dbscan_job_bytes(SUBSAMPLE)} bytes that one job of "
                         f"{SUBSAMPLE} points needs")
    chunks: List[List[int]] = []
    used = 0
    for j, b in enumerate(job_bytes):
        if b > budget:
            raise ValueError(f"job {j} needs {b} bytes of DBSCAN scratch, the budget is {budget}")
        if not chunks or used + b > budget:
            chunks.append([])
            used = 0
        chunks[-1].append(j)
        used += b
    return chunks


def _check_batch(maps, frame_index, masks, depth_frames, scratch_budget_bytes, *per_job) -> Tuple[int, int, int, int]:
    """Refusals that need no device: (D, F, H, W)."""
    D = len(maps)
    if len(frame_index) != D or len(masks) != D or any(len(x) != D for x in per_job):
        raise ValueError("update_maps_batch: maps, object_names, frame_index, masks and tfs must have one entry per job")
    plan_chunks([], int(scratch_budget_bytes))
    shape = tuple(depth_frames.shape)
    if len(shape) < 3:
        raise ValueError("update_maps_batch: depth_frames is [F][H][W]")
    F, H, W = int(shape[0]), int(shape[-2]), int(shape[-1])
    if F * H * W != int(np.prod(shape)):
        raise ValueError(f"update_maps_batch: depth_frames {shape} is not F frames of H x W")
    if D and tuple(masks.shape) != (D, H, W):
        raise ValueError(f"update_maps_batch: masks {tuple(masks.shape)} is not {(D, H, W)}")
    bad = [int(f) for f in frame_index if not 0 <= int(f) < F]
    if bad:
        raise ValueError(f"update_maps_batch: frame index {bad[0]} is outside the {F} depth frames")
    return D, F, H, W


def mask_stats_batch(masks_u8, erosion: Sequence[float], device):
    """Stage 1 for D masks ([D][H][W] u8 device tensor) at once: pack, erode (per-job iteration counts) and count.  Returns the
    device scratch that the expansion reads and the [D][4] host array (points of the eroded mask, first and last occupied column
    of the un-eroded mask or -1 -1, 0) -- the one read-back that does not depend on anything random."""
    import torch

    L = _lib.lib()
    D, H, W = masks_u8.shape
    iterations = [max(int(e), 0) for e in erosion]
    with torch.cuda.device(device):
        scratch = torch.empty(L.vlfm_object_cloud_batch_scratch_bytes(D, H, W), dtype=torch.uint8, device=device)
        ero = torch.tensor(iterations, dtype=torch.int32).to(device)
        stats = torch.empty((D, 4), dtype=torch.int32, device=device)
        _lib.check(L.vlfm_object_cloud_batch_stats(masks_u8.data_ptr(), ero.data_ptr(), D, max(iterations), H, W,
                                                   scratch.data_ptr(), stats.data_ptr(), _stream_ptr()), "object_cloud_batch_stats")
        SYNCS[0] += 1
        return scratch, stats.cpu().numpy()


def extract_object_clouds_batch(maps: Sequence[ObjectPointCloudMap], depth_frames, frame_index: Sequence[int], masks,
                                min_depth: float, max_depth: float, fx: float, fy: float,
                                scratch_budget_bytes: int = DEFAULT_SCRATCH_BUDGET) -> Iterator[Tuple[int, np.ndarray, bool]]:
    """The reference's ``_extract_object_cloud`` (:150-170) of ``depth_frames[frame_index[j]]`` under ``masks[j]`` with the erosion
    size, ``use_dbscan`` and generator of ``maps[j]``, for every job j, all jobs going through the kernels together; yields
    ``(j, cloud, too_offset(masks[j]))`` in job order.  A job's cloud and draws do not depend on what else is in the batch.  A
    generator, because the random draws have to interleave with the caller's: the ``choice``s of a wave (``plan_waves``) are drawn
    when its first job is asked for, and whoever consumes a job makes that job's other draws before asking for the next one.

    Launches and host synchronisations: one synchronisation for the point counts of all jobs, then one per (wave, scratch chunk);
    pack, max(erosion) erosions and the statistics kernel for the counts, then expansion, adjacency and clustering per chunk.
    Device memory: 2 bit planes per job, at most 5000 points per job twice, and at most ``scratch_budget_bytes`` of adjacency
    scratch."""
    import torch

    D, F, H, W = _check_batch(maps, frame_index, masks, depth_frames, scratch_budget_bytes)
    if D == 0:
        return
    L = _lib.lib()
    dev = maps[0].device
    if any(m.device != dev for m in maps):
        raise ValueError("update_maps_batch: all maps must live on one device")
    d = depth_frames if torch.is_tensor(depth_frames) else torch.from_numpy(np.ascontiguousarray(depth_frames, np.float32))
    d = d.to(device=dev, dtype=torch.float32).reshape(F, H, W).contiguous()
    m = masks if torch.is_tensor(masks) else torch.from_numpy(np.ascontiguousarray(masks))
    m = m.to(dev)
    m = (m.contiguous().view(torch.uint8) if m.dtype == torch.bool else (m != 0).to(torch.uint8).contiguous())
    with torch.cuda.device(dev):
        stream = _stream_ptr()
        scratch, st = mask_stats_batch(m, [mp._erosion_size for mp in maps], dev)
        counts = [int(c) for c in st[:, 0]]
        offset = [extent_too_offset(int(a), int(b) + 1, W) if a >= 0 else extent_too_offset(0, 0, W) for a, b in st[:, 1:3]]
        for wave in plan_waves([id(mp._rng) for mp in maps], [c > SUBSAMPLE for c in counts]):
            ranks = {j: maps[j]._rng.choice(counts[j], SUBSAMPLE, replace=False) for j in wave if counts[j] > SUBSAMPLE}
            n_out = {j: min(counts[j], SUBSAMPLE) for j in wave}
            cluster = {j: bool(maps[j].use_dbscan) and n_out[j] > 0 for j in wave}
            need = [dbscan_job_bytes(n_out[j]) if cluster[j] else 0 for j in wave]
            for chunk in plan_chunks(need, int(scratch_budget_bytes)):
                jobs = [wave[i] for i in chunk]
                first = np.concatenate(([0], np.cumsum([n_out[j] for j in jobs]))).astype(np.int64)
                total = int(first[-1])
                out: Dict[int, np.ndarray] = {}
                if total:
                    rank_first, rank_list = {}, []
                    for j in jobs:
                        if j in ranks:
                            rank_first[j] = sum(len(r) for r in rank_list)
                            rank_list.append(ranks[j].astype(np.int32))
                    ex = np.array([(j, int(frame_index[j]), n_out[j], first[i], rank_first.get(j, -1), 0)
                                   for i, j in enumerate(jobs)], np.int32)
                    ex_d = torch.from_numpy(ex).to(dev)
                    rk_d = torch.from_numpy(np.concatenate(rank_list)).to(dev) if rank_list else None
                    points = torch.empty((total, 3), dtype=torch.float64, device=dev)
                    _lib.check(L.vlfm_object_cloud_batch_expand(
                        d.data_ptr(), F, H, W, float(min_depth), float(max_depth), float(fx), float(fy), scratch.data_ptr(), D,
                        ex_d.data_ptr(), len(jobs), max(n_out[j] for j in jobs), rk_d.data_ptr() if rk_d is not None else None,
                        rk_d.numel() if rk_d is not None else 0, points.data_ptr(), total, stream), "object_cloud_batch_expand")
                    db = [(i, j) for i, j in enumerate(jobs) if cluster[j]]
                    if db:
                        sc_first = np.concatenate(([0], np.cumsum([dbscan_job_bytes(n_out[j]) for _, j in db]))).astype(np.int64)
                        dj = np.array([(n_out[j], first[i], sc_first[k]) for k, (i, j) in enumerate(db)], np.int64)
                        dj_d = torch.from_numpy(dj).to(dev)
                        sc = torch.empty(int(sc_first[-1]), dtype=torch.uint8, device=dev)
                        # ONE buffer comes back: the kept counts ([len(db)] i32, padded to whole f64 words), then the kept points
                        head = (len(db) + 1) // 2
                        back = torch.empty(head + total * 3, dtype=torch.float64, device=dev)
                        _lib.check(L.vlfm_dbscan_largest_cluster_batch(
                            points.data_ptr(), total, dj_d.data_ptr(), len(db), max(n_out[j] for _, j in db), DBSCAN_EPS,
                            DBSCAN_MIN_POINTS, sc.data_ptr(), sc.numel(), back[head:].data_ptr(), back.data_ptr(), stream),
                            "dbscan_batch")
                        SYNCS[0] += 1
                        host = back.cpu().numpy()
                        kept, num = host[head:].reshape(total, 3), host[:head].view(np.int32)
                        for k, (i, j) in enumerate(db):
                            out[j] = kept[first[i]:first[i] + int(num[k])] if num[k] else np.array([])
                    if not all(maps[j].use_dbscan for j in jobs):    # maps without DBSCAN take the (sub-sampled) cloud as it is
                        SYNCS[0] += 1
                        host = points.cpu().numpy()
                        for i, j in enumerate(jobs):
                            if not maps[j].use_dbscan:
                                out[j] = host[first[i]:first[i + 1]]
                for j in jobs:
                    if j not in out:   # no point left: (0, 3) without DBSCAN, open3d_dbscan_filtering's np.array([]) with it
                        out[j] = np.array([]) if maps[j].use_dbscan else np.zeros((0, 3), np.float64)
                    yield j, out[j], offset[j]


def update_maps_batch(maps: Sequence[ObjectPointCloudMap], object_names: Sequence[str], depth_frames, frame_index: Sequence[int],
                      masks, tfs: Sequence[np.ndarray], min_depth: float, max_depth: float, fx: float, fy: float,
                      scratch_budget_bytes: int = DEFAULT_SCRATCH_BUDGET) -> List[bool]:
    """The reference's ``update_map`` (:29-75) of ``depth_frames[frame_index[j]]`` under ``masks[j]`` into class
    ``object_names[j]`` of ``maps[j]``, for j = 0..D-1 in order, with all D detections going through erosion, back-projection,
    sub-sampling and DBSCAN together (``extract_object_clouds_batch``).  ``maps[j]`` may repeat, several jobs may share a depth
    frame, maps may differ in erosion size and share generators: clouds and every draw of every generator are those of D calls
    of one job each.  Returns, per job, whether it changed the number of points its map holds for its class."""
    _check_batch(maps, frame_index, masks, depth_frames, scratch_budget_bytes, object_names, tfs)
    changed = []
    for j, cloud, off in extract_object_clouds_batch(maps, depth_frames, frame_index, masks, min_depth, max_depth, fx, fy,
                                                     scratch_budget_bytes):
        before = len(maps[j].clouds.get(object_names[j], ()))
        maps[j]._commit(object_names[j], cloud, lambda off=off: off, tfs[j], max_depth)
        changed.append(len(maps[j].clouds.get(object_names[j], ())) != before)
    return changed


# ---------------------------------------------------------------------------------------------- queries over device mirrors
QUERY_DTYPE = np.dtype([("d_rows", "<u8"), ("d_slots", "<u8"), ("p", "<f8", (3,)), ("heading", "<f8"), ("half_fov", "<f8"),
                        ("range", "<f8"), ("n", "<i4"), ("k", "<i4"), ("flag_offset", "<i4"), ("n_slots", "<i4")])
assert QUERY_DTYPE.itemsize == 80      # vlfm_cloud_query


def _check_queries(what: str, maps, *per_map) -> int:
    """Refusals that need no device: the number of maps."""
    E = len(maps)
    if any(len(x) != E for x in per_map):
        raise ValueError(f"{what}: one entry per map in every argument")
    if E and any(m.device != maps[0].device for m in maps):
        raise ValueError(f"{what}: all maps must live on one device")
    return E


def _query_row(q, mirror: CloudMirror, n: int, p, k: int) -> None:
    q["d_rows"], q["d_slots"], q["n"], q["k"] = mirror.rows_d.data_ptr(), mirror.slots_d.data_ptr(), n, k
    q["p"][:k] = p


def update_explored_batch(maps: Sequence[ObjectPointCloudMap], tfs: Sequence[np.ndarray], max_depth: float,
                          cone_fov: float) -> List[bool]:
    """``maps[i].update_explored(tfs[i], max_depth, cone_fov)`` for every i, over every class of every map, with ONE launch over
    the device mirrors of the clouds and ONE read-back, whatever the number of maps; returns, per map, whether anything was
    dropped.  The device says, per far-tag slot of a cloud, whether a point of it lies inside the cone; the removal is the host's
    own ``cloud[cloud[..., -1] != t]``, so the clouds are those of the per-map method bit for bit.  A point whose angle lies
    within ``CONE_BAND`` of the cone's edge is decided by ``within_fov_cone`` on the host (``BAND_POINTS``); clouds that cannot be
    mirrored, and every cloud when the band would reach the wrap at +-pi, take the per-map path."""
    import torch

    E = _check_queries("update_explored_batch", maps, tfs)
    dropped = [False] * E
    if E == 0:
        return dropped
    half, cone_range = cone_fov / 2, max_depth * 0.5
    device_ok = bool(np.isfinite(half) and np.isfinite(cone_range) and half + CONE_BAND < np.pi)
    dev = maps[0].device
    asked = []                                 # (map, name, mirror, origin, heading, first flag, slots)
    total = 0
    with torch.cuda.device(dev):
        for i, m in enumerate(maps):
            origin, heading = np.asarray(tfs[i])[:3, 3], extract_yaw(tfs[i])
            on_device = device_ok and bool(np.isfinite(origin).all() and np.isfinite(heading))
            for name, cloud in list(m.clouds.items()):
                if m._all_near(name):
                    continue
                mirror = m._mirror_sync(name) if on_device and len(cloud) else None
                if mirror is None:
                    dropped[i] |= m._explore_cloud(name, m.clouds[name], origin, heading, max_depth, cone_fov)
                elif mirror.table:             # (no far tag: nothing can be dropped)
                    asked.append((i, name, mirror, origin, heading, total, len(mirror.table)))
                    total += 2 * len(mirror.table)
        if not asked:
            return dropped
        q = np.zeros(len(asked), QUERY_DTYPE)
        for row, (i, name, mirror, origin, heading, first, n_slots) in zip(q, asked):
            _query_row(row, mirror, mirror.on_device, origin, 3)
            row["heading"], row["half_fov"], row["range"], row["flag_offset"], row["n_slots"] = heading, half, cone_range, first, n_slots
        q_d = torch.from_numpy(q.view(np.uint8)).to(dev)
        flags = torch.zeros(total, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().vlfm_cloud_cone_flags(q_d.data_ptr(), len(asked), int(q["n"].max()), flags.data_ptr(), _stream_ptr()),
                   "cloud_cone_flags")
        SYNCS[0] += 1
        host = flags.cpu().numpy()
    for i, name, mirror, origin, heading, first, n_slots in asked:
        m = maps[i]

        def decide(slot: int) -> bool:
            points = m.clouds[name][mirror.slots == slot]
            BAND_POINTS[0] += len(points)
            return len(within_fov_cone(origin, heading, cone_fov, cone_range, points)) > 0

        slots = merge_cone_flags(host[first:first + n_slots], host[first + n_slots:first + 2 * n_slots], decide)
        if slots:
            m._drop_tags(name, m.clouds[name], [mirror.table[s] for s in slots])
            dropped[i] = True
    return dropped


def get_best_objects_batch(maps: Sequence[ObjectPointCloudMap], target_classes: Sequence[str],
                           positions: Sequence[np.ndarray]) -> List[Optional[np.ndarray]]:
    """``maps[i].get_best_object(target_classes[i], positions[i]) if maps[i].has_object(target_classes[i]) else None`` for every
    i, in order (a map may repeat: its hysteresis sees the calls one after the other), with one launch sequence over the device
    mirrors and one read-back.  The device returns, per cloud, the number of trusted points and np.argmin's index of the closest
    trusted point and of the closest point; the host reads the candidate from its own array and applies the hysteresis.  Maps
    with ``use_dbscan=False`` and clouds that cannot be mirrored take the per-map path."""
    import torch

    E = _check_queries("get_best_objects_batch", maps, target_classes, positions)
    if E == 0:
        return []
    dev = maps[0].device
    asked: Dict[int, int] = {}                 # map index -> query
    rows = []
    with torch.cuda.device(dev):
        for i, m in enumerate(maps):
            name, p = target_classes[i], np.asarray(positions[i])
            if not m.has_object(name) or not m.use_dbscan or p.shape not in ((2,), (3,)) or not np.isfinite(p).all():
                continue
            mirror = m._mirror_sync(name)
            if mirror is not None:
                asked[i] = len(rows)
                rows.append((mirror, mirror.on_device, p.astype(np.float64)))
        if rows:
            L = _lib.lib()
            q = np.zeros(len(rows), QUERY_DTYPE)
            for row, (mirror, n, p) in zip(q, rows):
                _query_row(row, mirror, n, p, len(p))
            longest = int(q["n"].max())
            q_d = torch.from_numpy(q.view(np.uint8)).to(dev)
            need = L.vlfm_cloud_closest_scratch_bytes(len(rows), longest)
            scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
            result = torch.empty((len(rows), 4), dtype=torch.int32, device=dev)
            _lib.check(L.vlfm_cloud_closest(q_d.data_ptr(), len(rows), longest, scratch.data_ptr(), need, result.data_ptr(),
                                            _stream_ptr()), "cloud_closest")
            SYNCS[0] += 1
            found = result.cpu().numpy()
    out: List[Optional[np.ndarray]] = [None] * E
    for i, m in enumerate(maps):
        name = target_classes[i]
        if i in asked:
            trusted, first_trusted, first = (int(v) for v in found[asked[i]][:3])
            pick = first_trusted if trusted else first
            out[i] = m._goal_with_hysteresis(rows[asked[i]][0].array[pick][:2].copy(), positions[i])
        elif m.has_object(name):
            out[i] = m.get_best_object(name, positions[i])
    return out
