"""vlfm.mapping.value_map.ValueMap, MI355X-native (reference: /root/reference/vlfm/mapping/value_map.py).

Two layers:

* :class:`ValueMapBatch` -- ``n_envs`` value maps resident in HBM on one GPU, updated by ONE kernel launch per step
  for all environments (depth ingest -> profile polygon -> LDS coverage -> rotate/place/fuse).  This is what the
  batched-episode harness drives.
* :class:`ValueMap` -- the reference's class signature (value_map.py:44-51, :100-108, :146-148) as a drop-in for
  ``BaseITMPolicy`` (itm_policy.py:48-54, :191-211, :263-267); a thin single-slot view of a ValueMapBatch.

PyTorch is used for device memory and streams only; every per-pixel operation is a hand-written gfx950 kernel in
``vlfm_amd/csrc`` reached through the C ABI of ``include/vlfm_amd.h``.  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from .. import _lib
from . import render as _render
from .base_map import BaseMap, require_gpu


def _stream_ptr() -> int:
    import torch

    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())   # (see vlm/ops.py:_stream)


_WAIT_EVENTS: Dict[int, Any] = {}


def wait_stream() -> None:
    """Wait for the current stream on a reusable event.  Whether the wait spins or sleeps is the DEVICE's schedule flag
    (hipDeviceScheduleBlockingSync, set by _lib.host_wait_blocking / vlfm_host_wait_mode): measured on MI355X
    (tools/host_wait_probe.py) hipEventBlockingSync on the event alone still holds a core for the whole wait, the device
    flag brings the waiting thread to 0.00 cores.  The per-step read-backs sit behind ~100 ms of queued perception
    work, so a spinning rank costs a full host core (`host` block of bench.py)."""
    import torch

    dev = torch.cuda.current_device()
    ev = _WAIT_EVENTS.get(dev)
    if ev is None:
        ev = _WAIT_EVENTS[dev] = torch.cuda.Event(blocking=True)
    ev.record()
    ev.synchronize()


def _bytes_to_device(buf, device):
    """Upload a ctypes array / bytes object as a uint8 tensor (8-byte aligned by the caching allocator)."""
    import torch

    host = torch.frombuffer(bytearray(bytes(buf)), dtype=torch.uint8)
    return host.to(device, non_blocking=False)


class UploadRing:
    """Small per-step parameter blocks (poses, ingest parameters) go to HBM through a ring of pinned host buffers with
    asynchronous copies on the compute stream, so a step never blocks on a pageable H2D copy.  A slot is reused only
    after the copy that last read it has completed (event check).  A ring belongs to ONE stream: the device buffer of a
    slot is handed to kernels launched on the stream that was current at upload(); with ``slots`` uploads in flight on
    a second stream the oldest kernel could still be reading the buffer being overwritten.  The map classes keep one ring
    per purpose and are driven from one stream each (harness: obstacle rings on the side stream, value rings on main).  The host-side fill is a plain single-threaded
    NumPy memcpy into the pinned buffer: a torch CPU copy of >= 32 K elements would fan out over the OpenMP pool, whose
    spinning workers can exhaust a container's CPU quota and stall the whole process until the next scheduler period."""

    def __init__(self, device, nbytes: int, slots: int = 4) -> None:
        import torch

        self.device, self.nbytes = device, nbytes
        self.host = [torch.empty(nbytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.host_np = [h.numpy() for h in self.host]
        self.dev = [torch.empty(nbytes, dtype=torch.uint8, device=device) for _ in range(slots)]
        self.done = [None] * slots
        self.events = [None] * slots   # one interrupt-driven event per slot, reused
        self.k = 0

    def upload(self, buf):
        import torch

        if isinstance(buf, np.ndarray):
            src = np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
        else:
            src = np.frombuffer(buf, dtype=np.uint8)  # ctypes arrays / bytes expose the buffer protocol
        n = src.size
        assert n <= self.nbytes
        i = self.k
        self.k = (self.k + 1) % len(self.host)
        if self.done[i] is not None:
            self.done[i].synchronize()
        self.host_np[i][:n] = src
        self.dev[i][:n].copy_(self.host[i][:n], non_blocking=True)
        if self.events[i] is None:
            self.events[i] = torch.cuda.Event(blocking=True)
        self.events[i].record()
        self.done[i] = self.events[i]
        return self.dev[i]


# NumPy views of the C structs of include/vlfm_amd.h (filled by the library's host functions or by array ops)
VM_POSE_DTYPE = np.dtype([("inv_affine", "<f8", (6,)), ("row0", "<i4"), ("col0", "<i4"), ("env", "<i4"),
                          ("reserved", "<i4")])
INGEST_DTYPE = np.dtype([("tf", "<f8", (12,)), ("depth_scale", "<f4"), ("depth_offset", "<f4"), ("depth_max", "<f4"),
                         ("reserved0", "<f4"), ("fx", "<f8"), ("fy", "<f8"), ("min_height", "<f8"),
                         ("max_height", "<f8"), ("env", "<i4"), ("scatter", "<i4")])
assert VM_POSE_DTYPE.itemsize == 64 and INGEST_DTYPE.itemsize == 152
VM_OPTICS_DTYPE = np.dtype([("d_template", "<u8"), ("d_template_bits", "<u8"), ("d_conf_quadrant", "<u8"), ("d_tan", "<u8"),
                            ("depth_scale", "<f4"), ("depth_offset", "<f4"), ("template_size", "<i4"), ("reserved", "<i4")])
assert VM_OPTICS_DTYPE.itemsize == 48


class _ConeTemplates:
    """Per-device cache of masked confidence templates, keyed like ValueMap._confidence_masks (value_map.py:37)."""

    def __init__(self) -> None:
        self._tmpl: Dict[Tuple[Any, ...], Any] = {}
        self._quad: Dict[Tuple[Any, ...], Any] = {}
        self._tan: Dict[Tuple[Any, ...], Any] = {}
        self._disc: Dict[Tuple[Any, ...], Any] = {}

    def template(self, device, fov: float, max_depth: float, ppm: int, min_conf: float):
        import torch

        key = (str(device), float(fov), float(max_depth), int(ppm), float(min_conf))
        if key not in self._tmpl:
            L = _lib.lib()
            size = int(max_depth * ppm)
            T = 2 * size + 1
            conf = np.zeros(T * T, np.float32)
            poly = np.zeros(2 * 512, np.int64)
            n_poly = ctypes.c_int(0)
            rc = L.vlfm_cone_template_host(float(fov), float(max_depth), int(ppm), float(min_conf),
                                           conf.ctypes.data, conf.size, poly.ctypes.data, 512, ctypes.byref(n_poly))
            _lib.check(rc, "cone_template_host")
            assert rc == T
            conf = _confidence_table_numpy(T, fov, min_conf)
            tab = conf.reshape(T, T)
            assert np.array_equal(tab, tab[::-1]) and np.array_equal(tab, tab[:, ::-1])  # |row - c|, |col - c| only
            self._quad[key] = torch.from_numpy(np.ascontiguousarray(tab[T // 2:, T // 2:])).to(device)
            d_conf = torch.from_numpy(conf).to(device)
            d_poly = torch.from_numpy(poly).to(device)
            d_tmpl = torch.empty(T * T, dtype=torch.float32, device=device)
            d_bits = torch.empty(T * ((T + 31) // 32), dtype=torch.int32, device=device)
            with torch.cuda.device(device):
                _lib.check(L.vlfm_cone_template_build(d_conf.data_ptr(), d_poly.data_ptr(), n_poly.value, T,
                                                      d_tmpl.data_ptr(), d_bits.data_ptr(), _stream_ptr()),
                           "cone_template_build")
                torch.cuda.current_stream().synchronize()
            self._tmpl[key] = (d_tmpl, d_bits, T)
        return self._tmpl[key]

    def quadrant(self, device, fov: float, max_depth: float, ppm: int, min_conf: float):
        """[(T/2+1)^2] f32: the unmasked confidence table's quadrant for the single-launch update's LDS taps."""
        self.template(device, fov, max_depth, ppm, min_conf)
        return self._quad[(str(device), float(fov), float(max_depth), int(ppm), float(min_conf))]

    def tan_table(self, device, fov: float, width: int):
        import torch

        key = (str(device), float(fov), int(width))
        if key not in self._tan:
            tab = np.zeros(width, np.float64)
            _lib.check(_lib.lib().vlfm_tan_table_host(float(fov), int(width), tab.ctypes.data), "tan_table_host")
            self._tan[key] = torch.from_numpy(tab).to(device)
        return self._tan[key]

    def disc(self, device, radius: int):
        import torch

        key = (str(device), int(radius))
        if key not in self._disc:
            hw = np.zeros(2 * radius + 1, np.int32)
            _lib.check(_lib.lib().vlfm_disc_rows_host(int(radius), hw.ctypes.data), "disc_rows_host")
            self._disc[key] = torch.from_numpy(hw).to(device)
        return self._disc[key]


_TEMPLATES = _ConeTemplates()


def _confidence_table_numpy(T: int, fov: float, min_conf: float) -> np.ndarray:
    """Unmasked confidence of value_map.py:343-351 evaluated with the reference's own math library (NumPy ufuncs for
    arctan2/cos, libm pow for the scalar ``** 2``), vectorised over the template; replaces the libm-only table of
    vlfm_cone_template_host when the host is Python so that the f64 intermediates are NumPy's to the last bit."""
    import math

    off = np.abs(np.arange(T) - T // 2)
    theta = np.arctan2(off[None, :].repeat(T, 0), off[:, None].repeat(T, 1))
    theta = (theta - 0) * (np.pi / 2 - 0) / (fov / 2 - 0) + 0
    cos = np.cos(theta)
    sq = np.array([math.pow(c, 2.0) for c in cos.reshape(-1)])
    conf = (sq - 0) * (1 - min_conf) / (1 - 0) + min_conf
    return np.ascontiguousarray(conf.astype(np.float32))


def pose_params(tf: np.ndarray, env_ids: Optional[Sequence[int]], size: int, ppm: int, T: int) -> np.ndarray:
    """Host prologue of ValueMap._localize_new_data for n observations -> structured array of vlfm_vm_pose."""
    tf = np.ascontiguousarray(np.asarray(tf, np.float64).reshape(-1, 16))
    n = tf.shape[0]
    out = np.zeros(n, VM_POSE_DTYPE)
    env = None
    if env_ids is not None:
        env = np.ascontiguousarray(np.asarray(env_ids, np.int32))
        assert env.shape == (n,)
    bad = ctypes.c_int(-1)
    # extract_yaw with the reference's own function: numpy.arctan2 (geometry_utils.py:157)
    yaw = np.ascontiguousarray(np.arctan2(tf[:, 4], tf[:, 0]))
    rc = _lib.lib().vlfm_value_map_pose_params(tf.ctypes.data, yaw.ctypes.data,
                                               env.ctypes.data if env is not None else None, n, size,
                                               ppm, T, out.ctypes.data, ctypes.byref(bad))
    _lib.check(rc, "value_map_pose_params")
    return out


def group_rig(env_ids: Sequence[int], n_envs: int) -> Tuple[np.ndarray, np.ndarray]:
    """Host grouping of a camera-rig call: ``env_ids`` [n] may repeat and interleave slots.  Returns ``order`` [n] -- the
    observations sorted by slot, the observations of one slot in the order they were listed (the reference applies its
    cameras sequentially) -- and ``slots`` [n_slots, 2] int32 = (first, count) into that order, one row per slot present."""
    env = np.asarray(env_ids, np.int64).reshape(-1)
    assert env.size > 0, "a rig call needs at least one observation"
    assert int(env.max()) < n_envs and int(env.min()) >= 0, "environment slot out of range"
    order = np.argsort(env, kind="stable")
    _, first, count = np.unique(env[order], return_index=True, return_counts=True)
    return order, np.ascontiguousarray(np.stack([first, count], axis=1).astype(np.int32))


def per_observation(x, n: int, dtype=np.float64) -> np.ndarray:
    """A scalar or a length-n sequence -> [n] array (the per-camera min_depth / max_depth / fov / fx / fy of a rig call)."""
    a = np.asarray(x, dtype)
    if a.ndim == 0:
        return np.full(n, a, dtype)
    assert a.shape == (n,), f"expected a scalar or {n} values, got shape {a.shape}"
    return np.ascontiguousarray(a)


def rig_optics(min_depth, max_depth, fov, n: int, lookup: Callable) -> np.ndarray:
    """vlfm_vm_optics records [n] (caller's order).  ``lookup(fov, max_depth)`` -> (template, template bits, quadrant, tangent
    table, T): device addresses of that camera model's cached tables and its template size."""
    lo, hi, fv = per_observation(min_depth, n), per_observation(max_depth, n), per_observation(fov, n)
    out = np.zeros(n, VM_OPTICS_DTYPE)
    out["depth_scale"] = (hi - lo).astype(np.float32)     # f32(max_depth - min_depth), the difference taken in f64
    out["depth_offset"] = lo.astype(np.float32)
    # one lookup per camera model, array ops over the observations (a 256-slot rig has a thousand of them per step)
    models, inv = np.unique(fv + 1j * hi, return_inverse=True)      # (fov, max_depth) pairs as complex numbers: a 1-D sort
    tab = np.array([lookup(float(m.real), float(m.imag)) for m in models], np.int64).reshape(len(models), 5)[inv.reshape(-1)]
    out["d_template"], out["d_template_bits"], out["d_conf_quadrant"], out["d_tan"] = tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3]
    out["template_size"] = tab[:, 4]
    return out


def stack_rig_frames(depth):
    """The frames of one rig call as [n,H,W]: a tensor / array passes through; a list of frames must share one shape (the
    tangent table and the key rows are per image width; cameras with other image sizes go into a call of their own)."""
    if not isinstance(depth, (list, tuple)):
        return depth
    shapes = {tuple(d.shape[-2:]) for d in depth}
    if len(shapes) != 1:
        raise ValueError(f"the cameras of one rig call must share the image shape, got {sorted(shapes)}: "
                         "use one call per image size")
    import torch

    if any(torch.is_tensor(d) for d in depth):
        return torch.stack([d.reshape(d.shape[-2], d.shape[-1]) if torch.is_tensor(d) else
                            torch.from_numpy(np.ascontiguousarray(d, np.float32)).to(depth[0].device) for d in depth])
    return np.stack([np.asarray(d, np.float32).reshape(d.shape[-2], d.shape[-1]) for d in depth])


class ValueMapBatch:
    """``n_envs`` value maps (+ confidence maps) resident in HBM, updated together."""

    _min_confidence: float = 0.25  # value_map.py:40

    def __init__(self, n_envs: int, value_channels: int, size: int = 1000, use_max_confidence: bool = True,
                 fusion_type: str = "default", pixels_per_meter: int = 20, device=None,
                 explored_bits: Optional[Any] = None) -> None:
        import torch

        self.device = require_gpu(device)
        _lib.lib()
        self.n_envs, self.channels, self.size, self.pixels_per_meter = n_envs, value_channels, size, pixels_per_meter
        self.use_max_confidence = bool(use_max_confidence)
        self.fusion_type = fusion_type
        if os.environ.get("MAP_FUSION_TYPE", "") != "":  # value_map.py:74-75
            self.fusion_type = os.environ["MAP_FUSION_TYPE"]
        assert self.fusion_type in _lib.FUSION_TYPES, f"Unknown fusion type {self.fusion_type}"
        self.conf = torch.zeros((n_envs, size, size), dtype=torch.float32, device=self.device)
        # f64: the reference's `_value_map` IS f64 after the first weighted fuse (value_map.py:423: `values` is an f64
        # ndarray and the attribute is re-bound to the f64 result); where the reference keeps it f32 (max-confidence :406,
        # "replace" :381-384) the kernel stores f32-representable doubles.  Either way: bit-equal to the reference.
        self.value = torch.zeros((n_envs, size, size, value_channels), dtype=torch.float64, device=self.device)
        self.n_updates = np.zeros(n_envs, np.int64)   # update_map calls per slot since construction (dtype rule below)
        # bit-packed ObstacleMap.explored_area of the same slots ([n_envs,S,ceil(S/32)] int32) when the value map is
        # synchronised with an obstacle map (value_map.py:369-375); None = Habitat default
        self.explored_bits = explored_bits
        self._colmax = None
        self._status = None
        self._ring = None
        self._written = None   # [n_envs,S,ceil(S/32)] cells that ever received a confidence (explored-synchronised mode)
        self._written_stale = False  # an update ran without the explored plane since `_written` was last complete
        self._counters = None
        self._rig_plans: Dict[Any, Dict[str, Any]] = {}   # update_cameras: per (env_ids, optics, width), see _rig_plan
        self._wp_out = self._wp_host = self._wp_cells = None
        self.traj = _render.TrajectoryPlanes(self.device, n_envs, size, pixels_per_meter)
        self._render_ring = _render.PackedRing(self.device)
        self._render_scratch = None
        self._render_plane_ring = None

    @property
    def value_is_f32(self) -> bool:
        """True when the reference's `_value_map` array never leaves f32 in this map's mode: masked assignment of
        `values` (use_max_confidence, value_map.py:406) or the "replace" ablation (:381-384, which returns before the
        weighted path).  Otherwise the first weighted fuse promotes it to f64 for good (:423)."""
        return self.fusion_type == "replace" or self.use_max_confidence

    def value_dtype(self, slot: int):
        """dtype of the reference's `_value_map` for this slot right now (f32 until the first weighted fuse; reset() keeps
        the dtype, value_map.py:96-98)."""
        return np.float32 if (self.value_is_f32 or self.n_updates[slot] == 0) else np.float64

    # ------------------------------------------------------------------------------------------ helpers
    def reset(self, env_ids: Optional[Sequence[int]] = None) -> None:
        if env_ids is None:
            self.conf.zero_()
            self.value.zero_()
            if self._written is not None:
                self._written.zero_()
        else:
            idx = list(env_ids)
            self.conf[idx] = 0
            self.value[idx] = 0
            if self._written is not None:
                self._written[idx] = 0
        self.traj.reset(env_ids)

    def _rings(self, n: int):
        if self._ring is None or self._ring.nbytes < max(n, self.n_envs) * 256:
            self._ring = UploadRing(self.device, max(n, self.n_envs) * 256, slots=8)
        return self._ring

    def _scratch(self, n: int, width: int):
        import torch

        if self._colmax is None or self._colmax.shape[0] < n or self._colmax.shape[1] != width:
            # order-preserving u32 keys, zero = "-inf"; produced by depth ingest, consumed + re-zeroed by the update
            self._colmax = torch.zeros((max(n, self.n_envs), width), dtype=torch.int32, device=self.device)
            self._status = torch.zeros((max(n, self.n_envs), 2), dtype=torch.int32, device=self.device)
        return self._colmax, self._status

    def column_max(self, depth) -> Any:
        """np.max(depth, axis=0) for a [n,H,W] device tensor via the depth-ingest kernel (no obstacle scatter).
        Returns the column-max KEY buffer that update() consumes."""
        import torch

        n, H, W = depth.shape
        colmax, status = self._scratch(n, W)
        prm = np.zeros(n, INGEST_DTYPE)
        with torch.cuda.device(self.device):
            d_prm = self._rings(n).upload(prm)
            _lib.check(_lib.lib().vlfm_depth_ingest_batched(depth.data_ptr(), n, H, W, d_prm.data_ptr(),
                                                           colmax.data_ptr(), None, self.size, self.pixels_per_meter,
                                                           status.data_ptr(), None, None, None, _stream_ptr()),
                       "depth_ingest")
        return colmax[:n]

    # ------------------------------------------------------------------------------------------ update
    def _device_values(self, values):
        """values -> device f64 [n, C] (device-resident scores straight from the ITC head make no host round trip)."""
        import torch

        if torch.is_tensor(values):
            return values.to(device=self.device, dtype=torch.float64).reshape(-1, self.channels).contiguous()
        return torch.from_numpy(
            np.ascontiguousarray(np.asarray(values, np.float64).reshape(-1, self.channels))).to(self.device)

    def _keys_from_depth(self, depth, n: int):
        """The column-max keys of [n,H,W] depth frames (device tensor, or host array that is uploaded), when no shared depth
        ingest handed them in."""
        import torch

        if not torch.is_tensor(depth):
            depth = torch.from_numpy(np.ascontiguousarray(depth, np.float32)).to(self.device)
        depth = depth.reshape(n, depth.shape[-2], depth.shape[-1]).contiguous()
        assert depth.dtype == torch.float32
        return self.column_max(depth)

    def _explored_and_written(self):
        """(explored, written) plane pointers of an update, (None, None) without an obstacle map attached."""
        import torch

        if self.explored_bits is None:
            self._written_stale = True   # cells fused from here on are not recorded in the plane
            return None, None
        ex = self.explored_bits
        assert ex.dtype == torch.int32 and ex.is_contiguous() and ex.shape[-2] == self.size
        if self._written is None or self._written_stale:
            # conf may already hold values (an obstacle map attached mid-episode, or detached for a while and
            # attached again): (re)start from conf != 0
            if self._written is None:
                self._written = torch.zeros((self.n_envs, self.size, (self.size + 31) // 32),
                                            dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().vlfm_bits_pack((self.conf != 0).to(torch.uint8).contiguous().data_ptr(),
                                                 self._written.data_ptr(), self.n_envs, self.size, self.size,
                                                 _stream_ptr()), "bits_pack")
            self._written_stale = False
        return ex.data_ptr(), self._written.data_ptr()

    def _counters_ptr(self, n: int):
        """Per-observation completion counters of the key hand-back: zero between launches."""
        import torch

        if self._counters is None or self._counters.numel() < n:
            self._counters = torch.zeros(max(n, self.n_envs), dtype=torch.int32, device=self.device)
        return self._counters.data_ptr()

    def update(self, values, depth, tf_camera_to_episodic, min_depth: float, max_depth: float, fov: float,
               env_ids: Optional[Sequence[int]] = None, colmax=None) -> None:
        """ValueMap.update_map for n observations at once (value_map.py:100-128).

        values [n,C] f64 host array or device tensor; depth [n,H,W] f32 (device tensor, or host array that is
        uploaded); tf [n,4,4] f64 host; ``colmax`` = column-max keys [n,W] on device (from a shared depth ingest).
        """
        import torch

        d_vals = self._device_values(values)
        n = d_vals.shape[0]
        # Host prologue FIRST: a camera outside the map (AssertionError, img_utils.py:43) or a bad slot list must fail before
        # any column maximum is reduced into the key buffer -- keys are only re-zeroed by a completed update, and stale keys
        # would max-merge this frame's depth profile into the next one.  Keys handed in by a shared depth ingest are
        # zeroed on that error path for the same reason.
        try:
            W = colmax.shape[-1] if colmax is not None else int(depth.shape[-1])
            d_tmpl, d_bits, T = _TEMPLATES.template(self.device, fov, max_depth, self.pixels_per_meter,
                                                    self._min_confidence)
            d_tan = _TEMPLATES.tan_table(self.device, fov, W)
            pose = pose_params(tf_camera_to_episodic, env_ids, self.size, self.pixels_per_meter, T)
            # one launch fuses every observation concurrently: two observations of the SAME slot (the reference's
            # multi-camera loop, reality_policies.py:113-141, is sequential) must go through separate calls
            assert len(np.unique(pose["env"])) == len(pose), "one observation per environment slot and call"
            assert int(pose["env"].max()) < self.n_envs and int(pose["env"].min()) >= 0, "environment slot out of range"
            self.n_updates[pose["env"]] += 1
        except Exception:
            if colmax is not None:
                colmax.zero_()
            raise
        if colmax is None:
            colmax = self._keys_from_depth(depth, n)
        with torch.cuda.device(self.device):
            d_pose = self._rings(n).upload(pose)
            explored_ptr, written_ptr = self._explored_and_written()
            _lib.check(_lib.lib().vlfm_value_map_update_fused_batched(
                colmax.data_ptr(), W, d_tan.data_ptr(), d_tmpl.data_ptr(), d_bits.data_ptr(), T, d_pose.data_ptr(),
                d_vals.data_ptr(), n, self.conf.data_ptr(), self.value.data_ptr(), self.size, self.channels,
                self.pixels_per_meter, float(min_depth), float(max_depth), int(self.use_max_confidence),
                _lib.FUSION_TYPES[self.fusion_type], explored_ptr, written_ptr, self._counters_ptr(n),
                _TEMPLATES.quadrant(self.device, fov, max_depth, self.pixels_per_meter,
                                    self._min_confidence).data_ptr(), _stream_ptr()), "value_map_update_fused")

    def update_cameras(self, values, depth, tf_camera_to_episodic, min_depth, max_depth, fov, env_ids: Sequence[int],
                       colmax=None) -> None:
        """ValueMap.update_map for the cameras of a rig in ONE launch (csrc/value_map.hip: value_map_update_rig_kernel).

        n observations; ``env_ids`` [n] may repeat and interleave slots.  The observations of one slot are fused in the
        order they are listed -- the reference loops over its cameras sequentially (itm_policy.py:191-211) and the weighted
        fuse does not commute -- different slots run concurrently; the maps equal n single-camera ``update`` calls bit for
        bit.  ``min_depth`` / ``max_depth`` / ``fov``: scalars or length-n arrays (each camera its own optics, as in
        reality/objectnav_env.py:184-228).  ``depth`` [n,H,W] (or a list of frames of ONE shape: mixed image sizes raise
        ValueError); ``colmax`` = the key rows [n,W] of a shared depth ingest, row i for observation i.

        Errors as in ``update``: a camera outside the map or a slot out of range is an AssertionError raised before
        anything is launched (``colmax`` keys handed in are zeroed); the maps are then unchanged, ``n_updates`` too."""
        import torch

        d_vals = self._device_values(values)
        n = d_vals.shape[0]
        try:
            if colmax is None:
                depth = stack_rig_frames(depth)
            W = colmax.shape[-1] if colmax is not None else int(depth.shape[-1])
            plan = self._rig_plan(env_ids, min_depth, max_depth, fov, n, W)
            tf = np.asarray(tf_camera_to_episodic, np.float64).reshape(n, 4, 4)[plan["order"]]
            if len(plan["groups"]) == 1:
                pose = pose_params(tf, plan["env"], self.size, self.pixels_per_meter, plan["groups"][0][0])
            else:                                               # the camera cell's window depends on the template size
                pose = np.zeros(n, VM_POSE_DTYPE)
                for T, idx in plan["groups"]:
                    pose[idx] = pose_params(tf[idx], plan["env"][idx], self.size, self.pixels_per_meter, T)
            pose["reserved"] = plan["order"]                    # row of the observation's keys / values / counter
        except Exception:
            if colmax is not None:
                colmax.zero_()
            raise
        self.n_updates += plan["counts"]
        if colmax is None:
            colmax = self._keys_from_depth(depth, n)
        with torch.cuda.device(self.device):
            d_pose = self._rings(n).upload(pose)
            explored_ptr, written_ptr = self._explored_and_written()
            static = plan["d_static"].data_ptr()
            _lib.check(_lib.lib().vlfm_value_map_update_rig_batched(
                colmax.data_ptr(), W, d_pose.data_ptr(), static, static + n * VM_OPTICS_DTYPE.itemsize, plan["n_slots"], n,
                plan["T_max"], d_vals.data_ptr(), self.conf.data_ptr(), self.value.data_ptr(),
                self.size, self.channels, self.pixels_per_meter, int(self.use_max_confidence),
                _lib.FUSION_TYPES[self.fusion_type], explored_ptr, written_ptr, self._counters_ptr(n),
                _stream_ptr()), "value_map_update_rig")

    def _rig_plan(self, env_ids, min_depth, max_depth, fov, n: int, W: int) -> Dict[str, Any]:
        """Everything of a rig call that does not depend on the poses: grouping by slot, the slot table and the optics records
        (already on the device, behind one another in ``d_static``).  A rig has the same slots and optics step after step, so
        the plan is kept per (env_ids, optics, width) and a step only builds and uploads its pose records."""
        env = np.ascontiguousarray(np.asarray(env_ids, np.int32).reshape(-1))
        assert env.shape == (n,), "one slot id per observation"
        lo, hi, fv = per_observation(min_depth, n), per_observation(max_depth, n), per_observation(fov, n)
        key = (n, W, env.tobytes(), lo.tobytes(), hi.tobytes(), fv.tobytes())
        plan = self._rig_plans.get(key)
        if plan is not None:
            return plan
        order, slots = group_rig(env, self.n_envs)

        def lookup(fov_, max_depth_):
            d_tmpl, d_bits, T = _TEMPLATES.template(self.device, fov_, max_depth_, self.pixels_per_meter, self._min_confidence)
            d_quad = _TEMPLATES.quadrant(self.device, fov_, max_depth_, self.pixels_per_meter, self._min_confidence)
            return (d_tmpl.data_ptr(), d_bits.data_ptr(), d_quad.data_ptr(),
                    _TEMPLATES.tan_table(self.device, fov_, W).data_ptr(), T)

        optics = rig_optics(lo, hi, fv, n, lookup)[order]
        sizes = optics["template_size"]
        static = np.concatenate([optics.view(np.uint8).reshape(-1), slots.view(np.uint8).reshape(-1)])
        plan = dict(order=order.astype(np.int32), env=np.ascontiguousarray(env[order]), n_slots=len(slots),
                    counts=np.bincount(env, minlength=self.n_envs), T_max=int(sizes.max()),
                    groups=[(int(T), np.nonzero(sizes == T)[0]) for T in np.unique(sizes)],
                    d_static=_bytes_to_device(static.tobytes(), self.device))
        if len(self._rig_plans) >= 16:
            self._rig_plans.clear()
        self._rig_plans[key] = plan
        return plan

    # ------------------------------------------------------------------------------------------ frontier scoring
    def waypoint_values(self, waypoints_xy: np.ndarray, env_of_waypoint: Sequence[int], radius: float) -> np.ndarray:
        """Disc medians for m waypoints -> [m, C] f64 (value_map.py:161-176, img_utils.py:213-266): np.median's result in
        the dtype of the reference's array (f64 in the weighted mode, f32 -- widened exactly -- otherwise)."""
        import torch

        wp = np.asarray(waypoints_xy, np.float64).reshape(-1, 2)
        m = wp.shape[0]
        if m == 0:
            return np.zeros((0, self.channels), np.float64)
        radius_px = int(radius * self.pixels_per_meter)
        # int() truncates toward zero (value_map.py:165-166) == ndarray.astype(int64) for finite values
        px = (-wp[:, 0] * self.pixels_per_meter).astype(np.int64) + self.size // 2
        py = (-wp[:, 1] * self.pixels_per_meter).astype(np.int64) + self.size // 2
        row, col = self.size - px, py
        assert ((row >= 0) & (row < self.size) & (col >= 0) & (col < self.size)).all(), \
            "Pixel location is outside the image."
        cells = np.stack([np.asarray(env_of_waypoint, np.int64), row, col], axis=1).astype(np.int32)
        d_disc = _TEMPLATES.disc(self.device, radius_px)
        if self._wp_out is None or self._wp_out.shape[0] < m:
            cap = max(64, 1 << (m - 1).bit_length())
            self._wp_out = torch.empty((cap, self.channels), dtype=torch.float64, device=self.device)
            self._wp_host = torch.empty((cap, self.channels), dtype=torch.float64).pin_memory()
            self._wp_cells = UploadRing(self.device, cap * 12, slots=4)
        with torch.cuda.device(self.device):
            d_cells = self._wp_cells.upload(cells)
            _lib.check(_lib.lib().vlfm_value_map_sort_waypoints_batched(self.value.data_ptr(), self.size,
                                                                       self.channels, d_cells.data_ptr(), m,
                                                                       radius_px, d_disc.data_ptr(),
                                                                       int(self.value_is_f32), self._wp_out.data_ptr(),
                                                                       _stream_ptr()),
                       "sort_waypoints")
            self._wp_host[:m].copy_(self._wp_out[:m], non_blocking=True)
            wait_stream()
        return self._wp_host[:m].numpy().copy()

    # ------------------------------------------------------------------------------------------ rendering
    def update_agent_traj(self, env_ids: Sequence[int], xy, yaw) -> None:
        """BaseMap.update_agent_traj for n slots: xy [n,2] metres, yaw [n]; a slot may repeat (positions in order).  Only
        the new path segments are rasterised (csrc/map_render.hip: traj_append_kernel)."""
        self.traj.append(env_ids, xy, yaw)

    def render(self, env_ids: Sequence[int], reduce: Any = "max", markers=None, explored: Any = "auto", out=None,
               rgb: bool = False):
        """ValueMap.visualize (value_map.py:189-219) for the slots ``env_ids`` -> uint8 [n,S,S,3] device tensor, BGR (RGB
        with ``rgb``).

        reduce: "max" (the default reduce_fn), ("explore", t) (ITMPolicyV3's visual reducer), or a reduced plane [n,S,S]
            (host array or device tensor, f32 or f64: the dtype the normalisation runs in) for any other reduce_fn.
        markers: rows (env slot, x, y, radius, thickness, b, g, r) drawn with cv2.circle after the trajectory, in order;
            like the reference, a slot without trajectory positions draws none.
        explored: "auto" = the synchronised obstacle map's plane (``explored_bits``) if any; None = no mask; or a
            bit-packed plane tensor [n_envs or 1, S, ceil(S/32)] (cells outside it become 0, value_map.py:198-199)."""
        import torch

        env = [int(e) for e in env_ids]
        n, S = len(env), self.size
        if any(not 0 <= e < self.n_envs for e in env):
            raise IndexError("environment slot out of range")
        out = _render.output(self.device, n, S, out)
        if n == 0:
            return out
        plane_ptr, thresh, mode = None, 0.0, _render.REDUCE_MAX
        f32 = [int(self.value_dtype(e) == np.float32) for e in env]
        keep = []
        if isinstance(reduce, str) and reduce == "max":
            pass
        elif isinstance(reduce, tuple) and len(reduce) == 2 and reduce[0] == "explore":
            mode, thresh = _render.REDUCE_EXPLORE, float(reduce[1])
        else:
            mode = _render.REDUCE_PLANE
            is_t = torch.is_tensor(reduce)
            dt = reduce.dtype if is_t else np.asarray(reduce).dtype
            if dt not in (np.float32, np.float64, torch.float32, torch.float64):
                raise TypeError(f"a reduced plane must be float32 or float64 (got {dt}): the normalisation runs in its dtype")
            f32 = [int(dt in (np.float32, torch.float32))] * n
            plane = (reduce.to(device=self.device, dtype=torch.float64) if is_t else
                     torch.from_numpy(np.ascontiguousarray(np.asarray(reduce), np.float64)).to(self.device))
            if tuple(plane.shape) != (n, S, S) and tuple(plane.shape) != (S, S) or (n != 1 and plane.dim() == 2):
                raise ValueError(f"a reduced plane must be [{n}, {S}, {S}] (got {tuple(plane.shape)})")
            plane = plane.reshape(n, S, S).contiguous()
            keep.append(plane)
            plane_ptr = plane.data_ptr()
        if isinstance(explored, str) and explored == "auto":
            explored = self.explored_bits
        ex_ptr, ex_idx = None, [-1] * n
        if explored is not None:
            _render.check_planes(explored, self.device, self.n_envs, S, "explored")
            ex_ptr = explored.data_ptr()
            ex_idx = [0] * n if explored.shape[0] == 1 else env
        frames = np.array([[e, f, x, 0] for e, f, x in zip(env, f32, ex_idx)], np.int32)
        by_slot = _render.marker_prims(markers)
        prims = []
        for e in env:
            p = self.traj.agent_prims(e)
            if self.traj.count[e] > 0:   # value_map.py:206-217: markers only with a trajectory
                p += by_slot.get(e, [])
            prims.append(p)
        buf, o_prims, o_vtx, any_prims = _render.pack(frames, prims)
        need = _lib.lib().vlfm_value_render_scratch_bytes(n, S)
        if self._render_scratch is None or self._render_scratch.numel() < need:
            self._render_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        path = self.traj.plane
        with torch.cuda.device(self.device):
            d = self._render_ring.upload(buf)
            base = d.data_ptr()
            _lib.check(_lib.lib().vlfm_value_map_render(
                self.value.data_ptr(), self.n_envs, S, self.channels, base, n, mode, thresh, plane_ptr, ex_ptr,
                path.data_ptr() if path is not None else None, base + 16 * n, base + o_prims if any_prims else None,
                base + o_vtx, int(bool(rgb)), self._render_scratch.data_ptr(), self._render_scratch.numel(),
                out.data_ptr(), _stream_ptr()), "value_map_render")
        return out


def _explored_bits_of(obstacle_map, device):
    """Bit-packed explored area [1,S,ceil(S/32)] of an attached obstacle map: ours hands over its HBM plane; any other
    object exposing the reference attribute ``explored_area`` (S,S bool) is uploaded and packed on the device."""
    import torch

    if hasattr(obstacle_map, "explored_bits_device"):
        return obstacle_map.explored_bits_device()
    area = np.ascontiguousarray(np.asarray(obstacle_map.explored_area).astype(np.uint8))
    S = area.shape[0]
    src = torch.from_numpy(area).to(device)
    dst = torch.empty((1, S, (S + 31) // 32), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().vlfm_bits_pack(src.data_ptr(), dst.data_ptr(), 1, S, S, _stream_ptr()), "bits_pack")
    return dst


# value_map.py:26-30 -- the reference's record/replay switches and on-disk format (8-bit depth PNGs + data.json + kwargs.json)
RECORDING = os.environ.get("RECORD_VALUE_MAP", "0") == "1"
PLAYING = os.environ.get("PLAY_VALUE_MAP", "0") == "1"
RECORDING_DIR = "value_map_recordings"
JSON_PATH = os.path.join(RECORDING_DIR, "data.json")
KWARGS_JSON = os.path.join(RECORDING_DIR, "kwargs.json")


def _default_reduce_fn(i):
    return np.max(i, axis=-1)


def explore_reduce_fn(thresh: float) -> Callable:
    """ITMPolicyV3's visual reducer (itm_policy.py:275-287) as a host callable that ValueMap.visualize runs on the device."""
    def visualize_value_map(arr: np.ndarray) -> np.ndarray:
        first_channel = arr[:, :, 0]
        return np.where(first_channel > thresh, first_channel, np.max(arr, axis=2))

    visualize_value_map.device_reduce = ("explore", float(thresh))
    return visualize_value_map


class ValueMap(BaseMap):
    """Drop-in for vlfm.mapping.value_map.ValueMap (same constructor and method signatures)."""

    _confidence_masks: Dict[Tuple[float, float], np.ndarray] = {}
    _min_confidence: float = 0.25
    _decision_threshold: float = 0.35

    def __init__(self, value_channels: int, size: int = 1000, use_max_confidence: bool = True,
                 fusion_type: str = "default", obstacle_map: Optional["ObstacleMap"] = None,  # noqa: F821
                 device=None, _batch: Optional[ValueMapBatch] = None, _slot: int = 0) -> None:
        super().__init__(size)
        self._value_channels = value_channels
        self._use_max_confidence = use_max_confidence
        self._obstacle_map = obstacle_map
        if obstacle_map is not None:
            assert obstacle_map.pixels_per_meter == self.pixels_per_meter  # value_map.py:71-73
            assert obstacle_map.size == self.size
        if _batch is None:
            _batch = ValueMapBatch(1, value_channels, size, use_max_confidence, fusion_type, self.pixels_per_meter,
                                   device)
            _slot = 0
        self._batch, self._slot = _batch, _slot
        self._fusion_type = _batch.fusion_type
        if RECORDING:  # value_map.py:77-94
            import json
            import shutil
            import warnings

            if os.path.isdir(RECORDING_DIR):
                warnings.warn(f"Recording directory {RECORDING_DIR} already exists. Deleting it.")
                shutil.rmtree(RECORDING_DIR)
            os.mkdir(RECORDING_DIR)
            with open(KWARGS_JSON, "w") as f:
                json.dump({"value_channels": value_channels, "size": size, "use_max_confidence": use_max_confidence}, f)
            with open(JSON_PATH, "w") as f:
                f.write("{}")

    # maps are HBM-resident; these attributes are host snapshots for the callers that read them (visualisation)
    @property
    def _map(self) -> np.ndarray:
        return self._batch.conf[self._slot].cpu().numpy()

    @property
    def _value_map(self) -> np.ndarray:
        # the reference's array is f32 until the first weighted fuse and f64 from then on (value_map.py:423); in the modes
        # that assign `values` into it (max-confidence, "replace") it stays f32.  The stored doubles are exact either way.
        return self._batch.value[self._slot].cpu().numpy().astype(self._batch.value_dtype(self._slot), copy=False)

    def reset(self) -> None:
        super().reset()
        self._batch.reset([self._slot])

    def update_map(self, values: np.ndarray, depth: np.ndarray, tf_camera_to_episodic: np.ndarray,
                   min_depth: float, max_depth: float, fov: float) -> None:
        assert len(values) == self._value_channels, \
            f"Incorrect number of values given ({len(values)}). Expected {self._value_channels}."
        import torch

        if not torch.is_tensor(depth):
            depth = np.asarray(depth, np.float32)
            if depth.ndim == 3:
                depth = depth.squeeze(2)  # value_map.py:231-232
            depth = depth[None]
        else:
            depth = depth.reshape(1, depth.shape[0], depth.shape[1])
        if self._obstacle_map is not None:
            self._batch.explored_bits = _explored_bits_of(self._obstacle_map, self._batch.device)
        self._batch.update(np.asarray(values, np.float64)[None], depth, np.asarray(tf_camera_to_episodic)[None],
                           min_depth, max_depth, fov, env_ids=[self._slot])
        if RECORDING:  # value_map.py:130-144 (cv2.imwrite of a single-channel u8 image == an 8-bit greyscale PNG)
            import glob
            import json

            from PIL import Image

            d = depth.cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
            idx = len(glob.glob(os.path.join(RECORDING_DIR, "*.png")))
            img_path = os.path.join(RECORDING_DIR, f"{idx:04d}.png")
            Image.fromarray((d.reshape(d.shape[-2], d.shape[-1]) * 255).astype(np.uint8)).save(img_path)
            with open(JSON_PATH, "r") as f:
                data = json.load(f)
            data[img_path] = {"values": np.asarray(values).tolist(),
                              "tf_camera_to_episodic": np.asarray(tf_camera_to_episodic).tolist(),
                              "min_depth": min_depth, "max_depth": max_depth, "fov": fov}
            with open(JSON_PATH, "w") as f:
                json.dump(data, f)

    def sort_waypoints(self, waypoints: np.ndarray, radius: float,
                       reduce_fn: Optional[Callable] = None) -> Tuple[np.ndarray, List[float]]:
        vals = self._batch.waypoint_values(waypoints, [self._slot] * len(waypoints), radius)
        if self._value_channels == 1:
            values: List[Any] = [float(v) if v != -1 else -1 for v in vals[:, 0]]
        else:
            values = [tuple(float(c) for c in v) for v in vals]
            assert reduce_fn is not None, "Must provide a reduction function when using multiple value channels."
            values = reduce_fn(values)
        order = np.argsort([-v for v in values])  # the reference's own ordering call (value_map.py:183)
        return np.array([waypoints[i] for i in order]), [values[i] for i in order]

    def visualize(self, markers: Optional[List[Tuple[np.ndarray, Dict[str, Any]]]] = None,
                  reduce_fn: Callable = _default_reduce_fn, obstacle_map=None) -> np.ndarray:
        """The reference's image (value_map.py:189-219), rendered on the device: the default reduce_fn (and a reducer
        made by ``explore_reduce_fn``) runs there, any other callable is applied to ``_value_map`` on the host and its
        plane uploaded."""
        return self.render_image(markers, reduce_fn, obstacle_map)

    def render_image(self, markers=None, reduce_fn: Callable = _default_reduce_fn, obstacle_map=None, rgb: bool = False,
                     host: bool = True):
        """visualize() with the kernel's RGB switch (``rgb``) and, with ``host=False``, the device [S,S,3] tensor."""
        self._push_trajectory(self._batch, self._slot)
        reduce: Any = "max"
        if getattr(reduce_fn, "device_reduce", None) is not None:
            reduce = reduce_fn.device_reduce
        elif reduce_fn is not _default_reduce_fn:
            reduce = np.asarray(reduce_fn(self._value_map)).copy()
        explored = None if obstacle_map is None else _explored_bits_of(obstacle_map, self._batch.device)
        rows = []
        for pos, kw in markers or []:
            extra = set(kw) - {"radius", "color", "thickness"}
            if extra:
                raise TypeError(f"marker keywords {sorted(extra)} are not supported by the device renderer")
            px = _render.metric_to_pixel(pos, self.pixels_per_meter, self._episode_pixel_origin)
            rows.append([self._slot, int(px[1]), int(px[0]), int(kw["radius"]), int(kw.get("thickness", 1)),
                         *[int(c) for c in kw["color"]]])
        img = self._batch.render([self._slot], reduce=reduce, markers=np.array(rows, np.int64).reshape(-1, 8),
                                 explored=explored, rgb=rgb)[0]
        return img.cpu().numpy() if host else img


def replay_from_dir(recording_dir: str = RECORDING_DIR, device=None) -> ValueMap:
    """value_map.py:448-475 without the interactive window: rebuilds a ValueMap from a recording made by the reference
    (or by this class) and returns it.  ``PLAY_VALUE_MAP=1 python -m vlfm_amd.mapping.value_map`` mirrors the reference's
    entry point and writes ``value_map_replay.png``."""
    import json

    from PIL import Image

    with open(os.path.join(recording_dir, "kwargs.json"), "r") as f:
        kwargs = json.load(f)
    with open(os.path.join(recording_dir, "data.json"), "r") as f:
        data = json.load(f)
    v = ValueMap(device=device, **kwargs)
    for img_path in sorted(data.keys()):
        rec = data[img_path]
        path = img_path if os.path.exists(img_path) else os.path.join(recording_dir, os.path.basename(img_path))
        depth = np.asarray(Image.open(path).convert("L")).astype(np.float32) / 255.0
        v.update_map(np.array(rec["values"]), depth, np.array(rec["tf_camera_to_episodic"]), float(rec["min_depth"]),
                     float(rec["max_depth"]), float(rec["fov"]))
    return v


if __name__ == "__main__":
    if PLAYING:
        from PIL import Image

        Image.fromarray(replay_from_dir().visualize()).save("value_map_replay.png")
        print("wrote value_map_replay.png")
