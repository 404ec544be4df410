"""Device rendering of the map classes' ``visualize()`` images (csrc/map_render.hip, DESIGN.md section 4, "Map renderer").

Host side only: the per-slot trajectory bookkeeping of the reference's TrajectoryVisualizer (traj_visualizer.py) and the
packing of one upload per render call -- frame headers, the primitives every frame draws in order (frontier circles,
agent disc, heading line, markers) and the 16.16 outline vertices of thick circles.  The pixels are the kernels'.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from .. import _lib

PRIM_DTYPE = np.dtype([("frame", "<i4"), ("kind", "<i4"), ("flags", "<i4"), ("thickness", "<i4"), ("x0", "<i4"),
                       ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("vtx_off", "<i4"), ("n_vtx", "<i4"),
                       ("bgr", "u1", (4,)), ("reserved", "<i4")])
assert PRIM_DTYPE.itemsize == 48

PRIM_CIRCLE_FILL, PRIM_CIRCLE, PRIM_LINE, PRIM_POLYLINE = 0, 1, 2, 3
FLIP_ROWS, UNDER_PATH = 1, 2
REDUCE_MAX, REDUCE_EXPLORE, REDUCE_PLANE = 0, 1, 2

# TrajectoryVisualizer's constants (traj_visualizer.py:10-18), scale_factor 1.0
PATH_THICKNESS = 3
AGENT_RADIUS = 8
AGENT_COLOR = (255, 192, 15)
AGENT_LINE_LENGTH = 10
AGENT_LINE_THICKNESS = 3

# marker rows of the batched render calls: (env slot, x, y, radius, thickness, b, g, r), x = column, y = row of the image
MARKER_COLUMNS = 8


def metric_to_pixel(pt, pixels_per_meter, origin) -> np.ndarray:
    """TrajectoryVisualizer._metric_to_pixel (traj_visualizer.py:99-105): (row, col) int32, truncated."""
    px = pt * pixels_per_meter * np.array([-1, -1]) + origin
    return px.astype(np.int32)


def circle_prim(x: int, y: int, radius: int, thickness: int, bgr, flags: int = 0) -> dict:
    """cv2.circle(img, (x, y), radius, bgr, thickness) as one primitive (outline vertices are added at packing)."""
    if radius < 0:
        raise ValueError("cv2.circle: radius must be >= 0")
    kind = PRIM_CIRCLE_FILL if thickness < 0 else (PRIM_CIRCLE if thickness <= 1 else PRIM_POLYLINE)
    return dict(kind=kind, flags=flags, thickness=int(thickness), x0=int(x), y0=int(y), x1=int(radius), y1=0,
                bgr=tuple(int(c) for c in bgr))


def line_prim(p0, p1, thickness: int, bgr, flags: int = 0) -> dict:
    if thickness < 2:
        raise ValueError("map rendering draws lines of thickness >= 2 only")
    return dict(kind=PRIM_LINE, flags=flags, thickness=int(thickness), x0=int(p0[0]), y0=int(p0[1]), x1=int(p1[0]),
                y1=int(p1[1]), bgr=tuple(int(c) for c in bgr))


def marker_prims(markers) -> Dict[int, List[dict]]:
    """Rows of a packed (env, x, y, radius, thickness, b, g, r) array as primitives per slot, in row order."""
    out: Dict[int, List[dict]] = {}
    if markers is None:
        return out
    for r in np.asarray(markers).reshape(-1, MARKER_COLUMNS).tolist():
        out.setdefault(int(r[0]), []).append(
            circle_prim(int(r[1]), int(r[2]), int(r[3]), int(r[4]), (int(r[5]), int(r[6]), int(r[7]))))
    return out


def pack(frames: np.ndarray, prims_per_frame: Sequence[List[dict]]):
    """One byte buffer: frame headers [n][4] i32 | prim_off [n+1] i32 | (16-aligned) prims | int64 vertices.
    Returns (buffer, offset of prims, offset of vertices, any primitive at all)."""
    n = len(prims_per_frame)
    flat = [(k, p) for k, ps in enumerate(prims_per_frame) for p in ps]
    circles = np.array([[p["x0"], p["y0"], p["x1"]] for _, p in flat if p["kind"] == PRIM_POLYLINE], np.int32)
    vtx = np.zeros((0, 2), np.int64)
    offs = np.zeros(1, np.int32)
    if len(circles):
        cap = 80 * len(circles)
        vtx = np.zeros((cap, 2), np.int64)
        offs = np.zeros(len(circles) + 1, np.int32)
        rc = _lib.lib().vlfm_circle_polygon_host(np.ascontiguousarray(circles).ctypes.data, len(circles),
                                                 vtx.ctypes.data, offs.ctypes.data, cap)
        _lib.check(rc, "circle_polygon_host")
        vtx = vtx[:rc]
    rows, c = [], 0
    for k, p in flat:
        off = nv = 0
        if p["kind"] == PRIM_POLYLINE:
            off, nv = int(offs[c]), int(offs[c + 1] - offs[c])
            c += 1
        rows.append((k, p["kind"], p["flags"], p["thickness"], p["x0"], p["y0"], p["x1"], p["y1"], off, nv,
                     (*p["bgr"], 0), 0))
    prims = np.array(rows, PRIM_DTYPE)
    prim_off = np.zeros(n + 1, np.int32)
    prim_off[1:] = np.cumsum([len(ps) for ps in prims_per_frame])
    head = np.concatenate([np.ascontiguousarray(frames, np.int32).reshape(-1), prim_off]).view(np.uint8)
    o_prims = (len(head) + 15) // 16 * 16
    o_vtx = o_prims + prims.nbytes
    buf = np.zeros(o_vtx + vtx.nbytes, np.uint8)
    buf[:len(head)] = head
    buf[o_prims:o_vtx] = prims.view(np.uint8)
    buf[o_vtx:] = np.ascontiguousarray(vtx).view(np.uint8).reshape(-1)
    return buf, o_prims, o_vtx, len(flat) > 0


class TrajectoryPlanes:
    """The TrajectoryVisualizer state of every slot of a batched map: a path bit-plane [n_envs, S, ceil(S/32)] in HBM (in
    image coordinates, i.e. after the flip), grown by one launch per update that rasterises only the new segments
    (== the reference's `_cached_path_mask` / `_num_drawn_points`: the union of idempotent segment paints), plus the
    last pixel position and heading per slot on the host for the agent marker."""

    def __init__(self, device, n_envs: int, size: int, pixels_per_meter: int) -> None:
        self.device, self.n_envs, self.size, self.ppm = device, n_envs, size, pixels_per_meter
        self.origin = np.array([size // 2, size // 2])
        self.count = np.zeros(n_envs, np.int64)
        self.last_px: List[Optional[np.ndarray]] = [None] * n_envs
        self.yaw: List[Any] = [0.0] * n_envs
        self.plane = None
        self._ring = None

    def reset(self, env_ids: Optional[Sequence[int]] = None) -> None:
        idx = list(range(self.n_envs)) if env_ids is None else list(env_ids)
        for e in idx:
            self.count[e], self.last_px[e], self.yaw[e] = 0, None, 0.0
        if self.plane is not None:
            self.plane[idx] = 0

    def append(self, env_ids: Sequence[int], xy, yaw) -> None:
        """Appends one position per entry (repeated slots are taken in order); yaw[k] becomes the slot's heading."""
        import torch

        from .value_map import UploadRing, _stream_ptr

        segs = []
        for e, p, y in zip(env_ids, xy, yaw):
            e = int(e)
            if not 0 <= e < self.n_envs:
                raise IndexError(f"environment slot {e} out of range")
            px = metric_to_pixel(np.asarray(p), self.ppm, self.origin)
            last = self.last_px[e]
            if last is not None and not np.array_equal(last, px):   # traj_visualizer.py:67-68
                segs.append((e, int(last[1]), int(last[0]), int(px[1]), int(px[0])))
            self.last_px[e], self.yaw[e] = px, y
            self.count[e] += 1
        if not segs:
            return
        if self.plane is None:
            self.plane = torch.zeros((self.n_envs, self.size, (self.size + 31) // 32), dtype=torch.int32,
                                     device=self.device)
        buf = np.ascontiguousarray(np.array(segs, np.int64).astype(np.int32))
        if self._ring is None or self._ring.nbytes < buf.nbytes:
            self._ring = UploadRing(self.device, max(buf.nbytes, 4096), slots=4)
        with torch.cuda.device(self.device):
            d = self._ring.upload(buf)
            _lib.check(_lib.lib().vlfm_traj_append(self.plane.data_ptr(), self.n_envs, self.size, d.data_ptr(),
                                                   len(segs), PATH_THICKNESS, _stream_ptr()), "traj_append")

    def agent_prims(self, e: int) -> List[dict]:
        """traj_visualizer.py:82-97: the filled agent disc and the heading line, when the slot has a position."""
        if self.count[e] == 0:
            return []
        px = self.last_px[e]
        yaw = self.yaw[e]
        end = (int(px[0] - AGENT_LINE_LENGTH * 1.0 * np.cos(yaw)), int(px[1] - AGENT_LINE_LENGTH * 1.0 * np.sin(yaw)))
        return [circle_prim(int(px[1]), int(px[0]), AGENT_RADIUS, -1, AGENT_COLOR),
                line_prim((int(px[1]), int(px[0])), (end[1], end[0]), AGENT_LINE_THICKNESS, (0, 0, 0))]


class PackedRing:
    """Growable UploadRing for the per-call primitive buffer."""

    def __init__(self, device) -> None:
        self.device, self.ring = device, None

    def upload(self, buf: np.ndarray):
        from .value_map import UploadRing

        if self.ring is None or self.ring.nbytes < buf.nbytes:
            self.ring = UploadRing(self.device, max(4096, 1 << (int(buf.nbytes) - 1).bit_length()), slots=4)
        return self.ring.upload(buf)


def output(device, n: int, size: int, out=None):
    import torch

    if out is None:
        return torch.empty((n, size, size, 3), dtype=torch.uint8, device=device)
    if (not torch.is_tensor(out) or out.device != torch.device(device) or out.dtype != torch.uint8
            or not out.is_contiguous() or tuple(out.shape) != (n, size, size, 3)):
        raise ValueError(f"out must be a contiguous uint8 [{n}, {size}, {size}, 3] tensor on {device}")
    return out


def check_planes(planes, device, n_envs: int, size: int, what: str):
    """A caller's bit-plane tensor: int32 [1 or n_envs, S, ceil(S/32)], contiguous, on the map's device."""
    import torch

    W = (size + 31) // 32
    if (not torch.is_tensor(planes) or planes.device != torch.device(device) or planes.dtype != torch.int32
            or not planes.is_contiguous() or planes.dim() != 3 or planes.shape[0] not in (1, n_envs)
            or tuple(planes.shape[1:]) != (size, W)):
        raise ValueError(f"{what} must be a contiguous int32 [1 or {n_envs}, {size}, {W}] bit-plane tensor on {device}")
    return planes
