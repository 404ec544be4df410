"""vlfm.mapping.object_point_cloud_map.ObjectPointCloudMap, MI355X-native
(reference: /root/reference/vlfm/mapping/object_point_cloud_map.py:17-297).

The per-detection heavy lifting -- mask erosion, masked back-projection, DBSCAN + largest-cluster selection
(``_extract_object_cloud``, :150-170) -- runs in HIP kernels (csrc/object_cloud.hip); the bookkeeping around it (range ids,
closest point, ``get_best_object`` hysteresis, ``update_explored``) is O(points kept) NumPy on the host exactly as in the
reference, INCLUDING its draws from NumPy's global RNG (``np.random.choice`` for the 5000-point subsample,
``np.random.rand`` for the out-of-range ids), so that a seeded run reproduces the reference's clouds."""
from __future__ import annotations

from typing import Dict, Iterator, List, Sequence, Tuple, Union

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
    points get an out-of-range tag because the object is probably cut off by the image edge.  ``mask``: (H,W) ndarray, or a
    device tensor (the column occupancy is reduced on the device; W bytes cross to the host)."""
    width = mask.shape[1]
    if hasattr(mask, "is_cuda"):
        SYNCS[0] += 1
        occupied = np.flatnonzero((mask != 0).any(dim=0).cpu().numpy())
    else:
        occupied = np.flatnonzero(np.asarray(mask).any(axis=0))       # cv2.boundingRect's x-extent
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

    def reset(self) -> None:
        self.clouds, self.last_target_coord = {}, None
        self._near_only = {}

    def _all_near(self, name: str) -> bool:
        """True when the cloud stored under ``name`` is known to hold only trusted (tag 1.0) points -- bookkeeping of update_map /
        update_explored, valid only for the very array it was recorded for (``clouds`` is a public dict)."""
        cloud = self.clouds.get(name)
        return cloud is not None and self._near_only.get(name) == (id(cloud), len(cloud))

    def has_object(self, target_class: str) -> bool:
        return len(self.clouds.get(target_class, ())) > 0

    def update_map(self, object_name: str, depth_img: np.ndarray, object_mask: np.ndarray,
                   tf_camera_to_episodic: np.ndarray, min_depth: float, max_depth: float, fx: float, fy: float) -> None:
        """object_point_cloud_map.py:29-75."""
        camera_frame = self._extract_object_cloud(depth_img, object_mask, min_depth, max_depth, fx, fy)
        self._commit(object_name, camera_frame, lambda: too_offset(object_mask), tf_camera_to_episodic, max_depth)

    def _commit(self, object_name: str, camera_frame: np.ndarray, is_too_offset, tf_camera_to_episodic: np.ndarray,
                max_depth: float) -> None:
        """Everything of ``update_map`` after the camera-frame cloud is on the host (:40-75) -- shared by the per-detection and the
        batched path.  ``is_too_offset``: called (once) only for a non-empty cloud."""
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
        candidate = self._get_closest_point(cloud, curr_position)[:2]
        previous = self.last_target_coord
        if previous is not None:
            moved = np.linalg.norm(candidate - previous)
            if moved < 0.1 or (moved < 0.5 and np.linalg.norm(curr_position - candidate) > 2.0):
                return previous
        self.last_target_coord = candidate
        return candidate

    def update_explored(self, tf_camera_to_episodic: np.ndarray, max_depth: float, cone_fov: float) -> None:
        """Forget far-tagged observations the robot is now looking at from within half the depth range (:103-135): every
        tag other than 1 that shows up inside the view cone is removed from the cloud as a whole."""
        origin, heading = tf_camera_to_episodic[:3, 3], extract_yaw(tf_camera_to_episodic)
        for name, cloud in list(self.clouds.items()):
            if self._all_near(name):
                continue       # only tags other than 1 can be dropped (`- {1}` below): nothing to do, same result
            seen_tags = set(within_fov_cone(origin, heading, cone_fov, max_depth * 0.5, cloud)[..., -1].tolist()) - {1}
            for t in seen_tags:
                cloud = cloud[cloud[..., -1] != t]
            self.clouds[name] = cloud

    def get_target_cloud(self, target_class: str) -> np.ndarray:
        """The trusted (tag 1) points when there are any, else everything (:137-144)."""
        cloud = self.clouds[target_class].copy()
        trusted = cloud[:, -1] == 1
        return cloud[trusted] if np.any(trusted) else cloud

    # ------------------------------------------------------------------------------------------ :150-170 on the GPU
    def _extract_object_cloud(self, depth: np.ndarray, object_mask: np.ndarray, min_depth: float, max_depth: float,
                              fx: float, fy: float) -> np.ndarray:
        import torch

        L = _lib.lib()
        dev = self.device
        d = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(dev) if not torch.is_tensor(depth) else depth
        d = d.reshape(d.shape[-2], d.shape[-1]).contiguous()
        H, W = d.shape
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(object_mask) != 0).astype(np.uint8)).to(dev) \
            if not torch.is_tensor(object_mask) else (object_mask != 0).to(torch.uint8).contiguous()
        cap = H * W
        scratch = torch.empty(L.vlfm_object_cloud_scratch_bytes(H, W), dtype=torch.uint8, device=dev)
        cloud = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(L.vlfm_object_cloud_extract(d.data_ptr(), m.data_ptr(), H, W, int(self._erosion_size),
                                                   float(min_depth), float(max_depth), float(fx), float(fy),
                                                   scratch.data_ptr(), cloud.data_ptr(), cap, count.data_ptr(),
                                                   _stream_ptr()), "object_cloud_extract")
            SYNCS[0] += 1
            n = int(count.item())
            cloud = cloud[:n]
            if n > 5000:  # get_random_subarray: NumPy's global RNG picks, the device gathers
                idx = self._rng.choice(n, 5000, replace=False)
                cloud = cloud[torch.from_numpy(idx).to(dev)].contiguous()
                n = 5000
            if not self.use_dbscan:
                SYNCS[0] += 1
                return cloud.cpu().numpy()
            if n == 0:
                return np.array([])  # open3d_dbscan_filtering of an empty cloud: no non-noise label (:200-201), shape (0,) like the reference
            sc = torch.empty(L.vlfm_dbscan_scratch_bytes(n), dtype=torch.uint8, device=dev)
            labels = torch.empty(n, dtype=torch.int32, device=dev)
            keep = torch.empty(n, dtype=torch.int32, device=dev)
            num = torch.zeros(1, dtype=torch.int32, device=dev)
            _lib.check(L.vlfm_dbscan_largest_cluster(cloud.data_ptr(), n, 0.2, 100, sc.data_ptr(), sc.numel(),
                                                     labels.data_ptr(), keep.data_ptr(), num.data_ptr(), _stream_ptr()),
                       "dbscan")
            SYNCS[0] += 1
            k = int(num.item())
            if k == 0:
                return np.array([])  # only noise was detected (:200-201)
            SYNCS[0] += 1
            return cloud[keep[:k].to(torch.int64)].cpu().numpy()

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
def plan_waves(generators: Sequence[int], needs_choice: Sequence[bool]) -> List[List[int]]:
    """Split jobs 0..D-1, in order, into waves whose random draws can be made as "all ``choice``s of the wave in job order, then
    all ``rand``s in job order" and still leave every generator with the draws of the per-detection path in the same order
    (per job: ``choice`` if the mask has more than 5000 points, then ``rand`` if the final cloud is not empty).  ``generators``:
    one key per job, equal for jobs that share a generator (``id(rng)``).  A new wave starts at a job that needs a ``choice``
    and whose generator already has an earlier job in the current wave -- that job's ``rand`` has to come first."""
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
    """``maps[j]._extract_object_cloud(depth_frames[frame_index[j]], masks[j], ...)`` for every job j, all jobs going through the
    kernels together; yields ``(j, cloud, too_offset(masks[j]))`` in job order, with bit-identical clouds.  A generator, because
    the random draws have to interleave with the caller's: the ``choice``s of a wave (``plan_waves``) are drawn when its first job
    is asked for, and whoever consumes a job makes that job's other draws before asking for the next one.

    Launches and host synchronisations: one synchronisation for the point counts of all jobs, then one per (wave, scratch chunk);
    pack, max(erosion) erosions and the statistics kernel for the counts, then expansion, adjacency and clustering per chunk.  Device memory: 2 bit planes per job, at most 5000 points per job
    twice, and at most ``scratch_budget_bytes`` of adjacency scratch."""
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
    """``maps[j].update_map(object_names[j], depth_frames[frame_index[j]], masks[j], tfs[j], ...)`` for j = 0..D-1 with all D
    detections going through erosion, back-projection, sub-sampling and DBSCAN together (``extract_object_clouds_batch``).
    ``maps[j]`` may repeat, several jobs may share a depth frame, maps may differ in erosion size and share generators: clouds and
    every draw of every generator are those of the D calls made one after the other.  Returns, per job, whether it changed the
    number of points its map holds for its class."""
    _check_batch(maps, frame_index, masks, depth_frames, scratch_budget_bytes, object_names, tfs)
    changed = []
    for j, cloud, off in extract_object_clouds_batch(maps, depth_frames, frame_index, masks, min_depth, max_depth, fx, fy,
                                                     scratch_budget_bytes):
        before = len(maps[j].clouds.get(object_names[j], ()))
        maps[j]._commit(object_names[j], cloud, lambda off=off: off, tfs[j], max_depth)
        changed.append(len(maps[j].clouds.get(object_names[j], ())) != before)
    return changed
