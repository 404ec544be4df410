"""The synthetic worlds behind the batched harness (vlfm_amd/harness.py holds the policy step that acts in them).  The device
side: floor-plan tables (WorldTable), the ray caster and the geodesic fields (RoomsRenderer, GeodesicFields).  The closed-loop
simulator on top (LiveWorld): the robots' poses, floor plans, objects (WorldObjects), sightings, ObjectNav episodes and scores."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .synthetic import ACTION_FORWARD, ACTION_STOP, ACTION_TURN_LEFT, ACTION_TURN_RIGHT, BOXES, MAX_DEPTH, MIN_DEPTH, YAWS, \
    camera_intrinsics, integrate, GEODESIC_MAX_SOURCES, STEP_MARGIN, WORLD_MAX_BOXES, WORLD_MAX_OBJECTS, goal_viewpoints, \
    inflated_rects, object_layout, plan_actions, rect_distance, soft_spl, spl, step_poses, tf_of, OBJECT_COLOURS, WORLD_PALETTE, \
    GRID_MAX_CELLS, GridPlan, LATTICE_MAX_COST, lattice_extent, lattice_sources, DepthSensor, DepthFilter


@dataclass(frozen=True)
class WorldObjects:
    """``BatchedEpisodes(world_objects=WorldObjects(...))``: target and distractor objects stand IN the rooms world
    (synthetic.object_layout), the ray caster renders them with occlusion and reports what is in view, and the environments
    run ObjectNav episodes that end on the policy's STOP (success within ``success_distance`` metres of the target's
    footprint), on "no frontier" or after ``max_episode_steps`` steps.  An object with at least ``min_pixels`` visible pixels
    is a sighting of its class at ``confidence``; from a quarter of that on, at ``faint_confidence`` (which the confidence filter
    has to drop).  ``layout``: any callable (env_id, episode, robot_xy) -> [(class, box6)], at most 8 objects."""
    min_pixels: int = 200
    confidence: float = 0.9
    faint_confidence: float = 0.35
    success_distance: float = 1.0
    max_episode_steps: int = 500
    layout: Callable = object_layout


def sightings_from_stats(stats, classes, min_pixels: int, confidence: float, faint_confidence: float):
    """The scripted detector head of a world with objects: ``stats`` [E,8,5] (visible pixels, first / last column, first / last
    row per object slot, as the ray caster returns them) and ``classes`` (per environment the class names of its slots) ->
    [(env slot, class, confidence, (cx, cy, ax, ay), object slot)] in the format of ``_sightings_at``: the VISIBLE bounding box
    as centre and half-extents.  ``count >= min_pixels``: confident; ``min_pixels / 4 <= count < min_pixels``: faint; less:
    not seen.  Pure host function."""
    out = []
    for e, names in enumerate(classes):
        for k, name in enumerate(names):
            count, cmin, cmax, rmin, rmax = (int(v) for v in stats[e][k])
            if 4 * count < min_pixels:
                continue
            box = ((cmin + cmax + 1) / 2, (rmin + rmax + 1) / 2, (cmax - cmin + 1) / 2, (rmax - rmin + 1) / 2)
            out.append((e, name, confidence if count >= min_pixels else faint_confidence, box, k))
    return out


def objectnav_outcome(stopped: bool, navigating: bool, no_frontier: bool, steps_done: int, max_steps: int, robot_xy, target_box,
                      success_distance: float) -> Optional[str]:
    """How an ObjectNav episode ends with this step, or None if it goes on: a STOP issued while navigating to an object goal is
    a "success" when the robot is within ``success_distance`` of the target's footprint rectangle (``target_box``; None = the
    layout has no target) and a "wrong_stop" otherwise; a stop for want of frontiers is "no_frontier"; ``steps_done`` steps
    (this one included) reaching ``max_steps`` is a "timeout".  Pure host function."""
    if stopped and navigating:
        near = target_box is not None and rect_distance(robot_xy, target_box) <= success_distance
        return "success" if near else "wrong_stop"
    if no_frontier:
        return "no_frontier"
    return "timeout" if steps_done >= max_steps else None


@dataclass
class GeodesicFields:
    """Device handle of ``n`` geodesic fields (RoomsRenderer.geodesic_fields): the tables vlfm_geodesic_fields wrote and the
    source lists it read, all f64 / int32 device tensors with the strides of include/vlfm_amd.h (R = walls + 8 rectangles, 4R
    nodes per field).  ``has_target`` [n] bool on the host: False for a field built without a target (no source)."""
    n: int
    max_sources: int
    rects: torch.Tensor          # [n,R,4]
    nodes: torch.Tensor          # [n,4R,2]
    dist: torch.Tensor           # [n,4R]
    counts: torch.Tensor         # [n,2] int32: rectangles, nodes
    sources: torch.Tensor        # [n,max_sources,2]
    source_counts: torch.Tensor  # [n] int32
    has_target: np.ndarray

    def assign(self, rows, other: "GeodesicFields") -> None:
        """Overwrite the fields ``rows`` of this handle with the fields of ``other`` (len(rows) == other.n), on the device."""
        rows = np.asarray(rows, np.int64).reshape(-1)
        if len(rows) != other.n or other.max_sources != self.max_sources or other.rects.shape[1:] != self.rects.shape[1:]:
            raise ValueError("GeodesicFields.assign: the other handle must hold one field of the same shape per row")
        if np.any((rows < 0) | (rows >= self.n)):
            raise ValueError("GeodesicFields.assign: row out of range")
        if not len(rows):
            return
        idx = torch.from_numpy(rows).to(self.rects.device)
        for name in ("rects", "nodes", "dist", "counts", "sources", "source_counts"):
            getattr(self, name).index_copy_(0, idx, getattr(other, name))
        self.has_target[rows] = other.has_target


@dataclass
class LatticeFields:
    """Device handle of ``n`` lattice geodesic fields (RoomsRenderer.lattice_fields_worlds) of ``cells_per_metre`` nodes per
    metre, with the strides of include/vlfm_amd.h ("Lattice geodesic"): every plane holds max_nb x max_na nodes, field i uses
    the ``dims[i]`` = (a0, b0, na, nb) of them.  ``dims_host``: the same on the host; ``has_target`` [n] bool on the host:
    False for a field built without a target (no source).  ``residence``: where the last launch kept its bit planes
    (_lib.LATTICE_IN_LDS / LATTICE_IN_SCRATCH / LATTICE_ALL_IN_SCRATCH; None: nothing was launched)."""
    n: int
    cells_per_metre: int
    bits: torch.Tensor           # [n,max_nb,ceil(max_na / 32)] int32: the free planes
    dist: torch.Tensor           # [n,max_nb,max_na] int16 holding the uint16 costs, 0xFFFF for none (``costs``)
    dims: torch.Tensor           # [n,4] int32
    dims_host: np.ndarray        # [n,4] int32
    has_target: np.ndarray
    residence: Optional[int] = None

    def costs(self, i: int) -> np.ndarray:
        """uint16 [nb, na] on the host: the field ``i`` within its dims (a read-back)."""
        _, _, na, nb = (int(v) for v in self.dims_host[i])
        return self.dist[i, :nb, :na].contiguous().cpu().numpy().view(np.uint16)

    def free(self, i: int) -> np.ndarray:
        """bool [nb, na] on the host: the free nodes of field ``i`` within its dims (a read-back)."""
        _, _, na, nb = (int(v) for v in self.dims_host[i])
        words = self.bits[i, :nb].cpu().numpy().view(np.uint32)
        return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :na].astype(bool)

    def assign(self, rows, other: "LatticeFields") -> None:
        """Overwrite the fields ``rows`` of this handle with the fields of ``other`` (len(rows) == other.n), on the device.
        The planes of this handle grow to ``other``'s strides where those are larger."""
        rows = np.asarray(rows, np.int64).reshape(-1)
        if len(rows) != other.n or other.cells_per_metre != self.cells_per_metre:
            raise ValueError("LatticeFields.assign: the other handle must hold one field of the same spacing per row")
        if np.any((rows < 0) | (rows >= self.n)):
            raise ValueError("LatticeFields.assign: row out of range")
        if not len(rows):
            return
        for name in ("bits", "dist"):
            mine, theirs = getattr(self, name), getattr(other, name)
            if theirs.shape[1] > mine.shape[1] or theirs.shape[2] > mine.shape[2]:
                grown = torch.full((self.n, max(mine.shape[1], theirs.shape[1]), max(mine.shape[2], theirs.shape[2])),
                                   -1 if name == "dist" else 0, dtype=mine.dtype, device=mine.device)   # (0xFFFF: no cost)
                grown[:, :mine.shape[1], :mine.shape[2]] = mine
                setattr(self, name, grown)
                mine = grown
            idx = torch.from_numpy(rows).to(mine.device)
            mine[idx, :theirs.shape[1], :theirs.shape[2]] = theirs
        self.dims.index_copy_(0, torch.from_numpy(rows).to(self.dims.device), other.dims)
        self.dims_host[rows] = other.dims_host
        self.has_target[rows] = other.has_target


class WorldTable:
    """A table of ``n_worlds`` floor plans for the per-world entries (RoomsRenderer.cast_worlds / geodesic_fields_worlds): the
    host mirror -- ``boxes`` [n_worlds,max_boxes,4] f64, NaN beyond each world's ``counts`` [n_worlds] int32 (what
    synthetic.step_poses takes as ``boxes``) -- and its copy on ``device`` (``d_boxes``, ``d_counts``).  Every world starts
    empty.  ``max_grid`` = (ny, nx): every world may also hold an occupancy grid of up to that many cells (synthetic.GridPlan)
    whose occupied cells are walls as well: ``grids`` [n_worlds] on the host (a plan or None: what step_poses takes as
    ``grids``) and on the device bit-packed rows ``d_grid_bits`` int32 [n_worlds, ny, ceil(nx / 32)], edges ``d_grid_edges`` f64
    [n_worlds, nx + 1 + ny + 1] (xs, then ys from index nx + 1) and ``d_grid_dims`` int32 [n_worlds, 2] = (ny, nx) of each
    world, (0, 0) for none (include/vlfm_amd.h: grid worlds)."""

    def __init__(self, n_worlds: int, device, max_boxes: int = WORLD_MAX_BOXES, max_grid=None) -> None:
        if n_worlds < 0 or max_boxes < 0:
            raise ValueError("WorldTable: n_worlds and max_boxes must not be negative")
        self.n_worlds, self.max_boxes, self.device = int(n_worlds), int(max_boxes), torch.device(device)
        self.max_grid = None
        self.grids: List[Optional[GridPlan]] = [None] * self.n_worlds
        if max_grid is not None:
            ny, nx = (int(v) for v in max_grid)
            if not (1 <= ny <= GRID_MAX_CELLS and 1 <= nx <= GRID_MAX_CELLS):
                raise ValueError(f"WorldTable: max_grid = (ny, nx), each in [1, {GRID_MAX_CELLS}]")
            self.max_grid, self.grid_words = (ny, nx), (nx + 31) // 32
            self.d_grid_bits = torch.zeros((self.n_worlds, ny, self.grid_words), dtype=torch.int32, device=self.device)
            self.d_grid_edges = torch.zeros((self.n_worlds, nx + ny + 2), dtype=torch.float64, device=self.device)
            self.d_grid_dims = torch.zeros((self.n_worlds, 2), dtype=torch.int32, device=self.device)
        self.boxes = np.full((self.n_worlds, self.max_boxes, 4), np.nan)
        self.counts = np.zeros(self.n_worlds, np.int32)
        self.d_boxes = torch.full((self.n_worlds, self.max_boxes, 4), float("nan"), dtype=torch.float64, device=self.device)
        self.d_counts = torch.zeros((self.n_worlds,), dtype=torch.int32, device=self.device)

    def world(self, row: int) -> np.ndarray:
        """[count,4] f64: the boxes of world ``row`` (a copy of the host mirror's)."""
        return self.boxes[row, :self.counts[row]].copy()

    def assign(self, rows, list_of_boxes, grids=None) -> None:
        """World ``rows[i]`` becomes the boxes ``list_of_boxes[i]`` [B_i,4] (finite, B_i <= max_boxes) and, in a table with
        ``max_grid``, the grid ``grids[i]`` (a GridPlan within max_grid, or None; ``grids=None``: none of these rows has one).
        Only these rows cross, in ONE host-to-device copy (boxes, counts, row indices, grid dims, edges and bits in one buffer),
        and are scattered into the table on the device, on the current stream."""
        rows = np.asarray(rows, np.int64).reshape(-1)
        worlds = [np.asarray(b, np.float64).reshape(-1, 4) for b in list_of_boxes]
        if len(rows) != len(worlds):
            raise ValueError("WorldTable.assign: one list of boxes per row")
        grids = [None] * len(rows) if grids is None else list(grids)
        if len(grids) != len(rows):
            raise ValueError("WorldTable.assign: one grid (or None) per row")
        for g in grids:
            if g is None:
                continue
            if not isinstance(g, GridPlan):
                raise ValueError("WorldTable.assign: a grid must be a synthetic.GridPlan")
            if self.max_grid is None or g.ny > self.max_grid[0] or g.nx > self.max_grid[1]:
                raise ValueError(f"WorldTable.assign: a grid of {g.ny} x {g.nx} cells, the table holds max_grid = {self.max_grid}")
        if np.any((rows < 0) | (rows >= self.n_worlds)) or len(np.unique(rows)) != len(rows):
            raise ValueError("WorldTable.assign: rows must be distinct rows of the table")
        for b in worlds:
            if len(b) > self.max_boxes:
                raise ValueError(f"WorldTable.assign: a world of {len(b)} boxes, the table holds {self.max_boxes} per world")
            if not np.all(np.isfinite(b)):
                raise ValueError("WorldTable.assign: boxes must be finite")
        if not len(rows):
            return
        nb = 4 * self.max_boxes
        ne = nw = 0                                  # doubles of a row's grid edges / of its bit rows (two words each)
        if self.max_grid is not None:
            ny, nx = self.max_grid
            ne, nw = nx + ny + 2, (ny * self.grid_words + 1) // 2
        blob = np.full((len(rows), nb + 4 + ne + nw), np.nan)
        blob[:, nb + 2:] = 0.0
        for i, (b, g) in enumerate(zip(worlds, grids)):
            blob[i, :4 * len(b)] = b.reshape(-1)
            blob[i, nb:nb + 2] = len(b), rows[i]
            if g is not None:
                blob[i, nb + 2:nb + 4] = g.ny, g.nx
                blob[i, nb + 4:nb + 4 + g.nx + 1] = g.xs
                blob[i, nb + 4 + nx + 1:nb + 4 + nx + 1 + g.ny + 1] = g.ys
                words = blob[i, nb + 4 + ne:].view(np.uint32)[:ny * self.grid_words].reshape(ny, self.grid_words)
                words[:g.ny] = g.packed_rows(self.grid_words)
            self.grids[rows[i]] = g
        self.boxes[rows] = blob[:, :nb].reshape(len(rows), self.max_boxes, 4)
        self.counts[rows] = [len(b) for b in worlds]
        d_blob = torch.from_numpy(blob).to(self.device)
        idx = d_blob[:, nb + 1].long()
        self.d_boxes.index_copy_(0, idx, d_blob[:, :nb].reshape(len(rows), self.max_boxes, 4))
        self.d_counts.index_copy_(0, idx, d_blob[:, nb].to(torch.int32))
        if self.max_grid is not None:
            self.d_grid_dims.index_copy_(0, idx, d_blob[:, nb + 2:nb + 4].to(torch.int32))
            self.d_grid_edges.index_copy_(0, idx, d_blob[:, nb + 4:nb + 4 + ne])
            bits = d_blob[:, nb + 4 + ne:].contiguous().view(torch.int32)[:, :ny * self.grid_words]
            self.d_grid_bits.index_copy_(0, idx, bits.reshape(len(rows), ny, self.grid_words))


class RoomsRenderer:
    """Depth frames of the consistent rooms-and-pillars world (vlfm_amd/synthetic.py) for E environments at once, ray-cast ON
    THE DEVICE by one kernel (csrc/world_render.hip; f64, bit for bit synthetic.render_objects_numpy, and for the table's
    headings depth_from_profile(wall_profile(...))): environment e walks the planned tour starting ``37 * env_id mod L`` steps
    in, so the batch sees rooms, doorways, pillars and a dozen or more simultaneous frontiers instead of the per-frame random
    walls of depth_frame().  ``prepare(t0, n)`` renders a window of steps ahead of a timed region (inputs resident in HBM
    before the clock starts); other steps render on the fly."""

    def __init__(self, env_ids, episode_len: int, height: int, width: int, device) -> None:
        self.L, self.H, self.W = episode_len, height, width
        self.device = torch.empty(0, device=device).device           # with its index, as a tensor on it reports it
        poses = integrate(plan_actions(2 * episode_len))            # two laps of the tour: no wrap inside an episode
        offs = [(37 * int(i)) % episode_len for i in env_ids]
        at = [[poses[o + t] for o in offs] for t in range(episode_len)]
        self.pose_table = np.array([[(x, y, YAWS[k]) for (x, y, k) in row] for row in at])       # [L,E,3]
        self.tf_table = np.stack([np.stack([tf_of(x, y, k) for (x, y, k) in row]) for row in at])  # [L,E,4,4]
        self.k_table = np.array([[k for (_, _, k) in row] for row in at], np.int64)               # [L,E] heading indices
        self.window = None
        self.window_t0 = 0
        self.painter = None      # optional (t, frames [E,H,W]) -> frames: scripted objects in front of the walls
        self.table = WorldTable(1, self.device, len(BOXES))     # the rooms world for the kernels: a world table of one row
        self.table.assign([0], [BOXES])

    @torch.no_grad()
    def render(self, t: int) -> torch.Tensor:
        """[E,H,W] f32 normalised depth of episode step t."""
        d = self.cast_cameras(self.tf_table[t])
        return self.painter(t, d) if self.painter is not None else d

    @torch.no_grad()
    def _raycast(self, who: str, tf: np.ndarray, table: WorldTable, world_of, objects=None, env_of=None, hfov=None,
                 min_depth=None, max_depth=None, out=None, rgb: bool = False, colours=None, palette=None, rgb_out=None):
        """What every ``cast_*`` method does (vlfm_worlds_raycast, one launch on the current stream): camera i stands in world
        ``world_of[i]`` of ``table``.  ``objects=None``: walls only; ``rgb``: the colour plane as well.  Returns (depth, ids,
        stats, rgb), None for what was not asked for.  A table with ``max_grid`` brings its grid arrays (vlfm_worlds_raycast_grids:
        the occupied cells of a world's grid are walls as well); with ``rgb`` that is refused.  The camera records (x, y, cos, sin, height, fx, lo, hi) are built on the
        host; they, the object records and the int32 lists (world_of, env_of, colours, palette) cross in ONE host buffer and one
        copy (all 8-byte aligned pieces).  ``who`` names the caller in error messages."""
        tf = np.asarray(tf, np.float64).reshape(-1, 4, 4)
        n = len(tf)
        dev = self.device
        if table.device != dev:
            raise ValueError(f"{who}: the world table must live on {dev}")
        world_of = self._checked_world_of(who, table, world_of, n, "camera")
        ints = [world_of]
        with_grids = table.max_grid is not None
        if with_grids and rgb:
            raise ValueError(f"{who}: a table with grids has no colour view (wall colours are defined by box and face)")
        if objects is None and rgb:                 # a world without objects: one row of empty slots, ids of zeros
            if env_of is not None or colours is not None:
                raise ValueError(f"{who}: env_of and colours belong to objects")
            objects, env_of = np.zeros((1, WORLD_MAX_OBJECTS, 8)), np.zeros(n, np.int32)
        if objects is None:
            objects = np.zeros((0, WORLD_MAX_OBJECTS, 8))
        else:
            objects = np.ascontiguousarray(objects, np.float64)
            if objects.ndim != 3 or objects.shape[0] < 1 or objects.shape[1:] != (WORLD_MAX_OBJECTS, 8):
                raise ValueError(f"{who}: objects must be [n_envs >= 1, {WORLD_MAX_OBJECTS}, 8]")
            env_of = np.ascontiguousarray(np.asarray(env_of).reshape(-1), np.int32)
            if len(env_of) != n or np.any((env_of < 0) | (env_of >= len(objects))):
                raise ValueError(f"{who}: env_of must name one row of objects per camera")
            ints.append(env_of)
        with_objects = len(objects) > 0
        if rgb:
            colours = np.zeros((len(objects), WORLD_MAX_OBJECTS), np.int32) if colours is None else np.asarray(colours)
            if colours.shape != (len(objects), WORLD_MAX_OBJECTS) or colours.dtype.kind not in "iu":
                raise ValueError(f"{who}: colours must be integers [{len(objects)}, {WORLD_MAX_OBJECTS}], one per object slot")
            palette = np.asarray(WORLD_PALETTE if palette is None else palette)
            if palette.shape != (12,) or palette.dtype.kind not in "iu":
                raise ValueError(f"{who}: palette must be 12 integers")
            ints += [(colours.astype(np.int64) & 0xFFFFFF).astype(np.int32).reshape(-1),
                     (palette.astype(np.int64) & 0xFFFFFF).astype(np.int32)]
        rec = np.empty((n, 8), np.float64)
        rec[:, 0:2], rec[:, 2:4], rec[:, 4] = tf[:, :2, 3], tf[:, :2, 0], tf[:, 2, 3]
        rec[:, 5] = camera_intrinsics(self.W)[0] if hfov is None else self.W / (2 * np.tan(np.asarray(hfov, np.float64) / 2))
        rec[:, 6] = MIN_DEPTH if min_depth is None else np.asarray(min_depth, np.float64)
        rec[:, 7] = MAX_DEPTH if max_depth is None else np.asarray(max_depth, np.float64)
        if not np.all(rec[:, 7] > rec[:, 6]):
            raise ValueError(f"{who}: every camera needs max_depth > min_depth")

        def plane(given, name, shape, dtype):
            if given is None:
                return torch.empty(shape, dtype=dtype, device=dev)
            if given.shape != shape or given.dtype != dtype or not given.is_contiguous() or given.device != dev:
                kind = "f32" if dtype == torch.float32 else "u8"
                raise ValueError(f"{who}: {name} must be a contiguous {kind} [{','.join(map(str, shape))}] tensor on {dev}")
            return given

        out = plane(out, "out", (n, self.H, self.W), torch.float32)
        rgb_out = plane(rgb_out, "rgb_out", (n, self.H, self.W, 3), torch.uint8) if rgb else None
        ids = stats = None
        if with_objects:
            ids = torch.empty((n, self.H, self.W), dtype=torch.uint8, device=dev)
            stats = torch.empty((n, WORLD_MAX_OBJECTS, 5), dtype=torch.int32, device=dev)
        if n > 0:
            with torch.cuda.device(dev):
                ints = np.concatenate(ints)
                blob = np.concatenate([rec.reshape(-1), objects.reshape(-1), np.zeros((len(ints) + 1) // 2, np.float64)])
                blob[rec.size + objects.size:].view(np.int32)[:len(ints)] = ints
                d_blob = torch.from_numpy(blob).to(dev)
                p = d_blob.data_ptr()
                p_ints = p + 8 * (rec.size + objects.size)          # world_of [n], env_of [n], colours, palette
                g_bits, g_edges, g_dims, g_nx, g_ny = self._grid_pointers(table)
                _lib.check(_lib.lib().vlfm_worlds_raycast_grids(
                    p, n, table.d_boxes.data_ptr(), table.d_counts.data_ptr(), table.n_worlds, table.max_boxes, p_ints,
                    p + 8 * rec.size if with_objects else None, p_ints + 4 * n if with_objects else None, len(objects),
                    self.H, self.W, out.data_ptr(), ids.data_ptr() if with_objects else None, stats.data_ptr() if with_objects else None,
                    p_ints + 8 * n if rgb else None, p_ints + 8 * n + 4 * WORLD_MAX_OBJECTS * len(objects) if rgb else None,
                    rgb_out.data_ptr() if rgb else None, g_bits, g_edges, g_dims, g_nx, g_ny,
                    torch.cuda.current_stream().cuda_stream), "worlds_raycast")
        return out, ids, stats, rgb_out

    @staticmethod
    def _checked_world_of(who: str, table: WorldTable, world_of, n: int, per: str) -> np.ndarray:
        """int32 [n]: ``world_of`` as the library takes it, one world of ``table`` per ``per`` ("camera", "field")."""
        world_of = np.ascontiguousarray(np.asarray(world_of).reshape(-1), np.int32)
        if len(world_of) != n or np.any((world_of < 0) | (world_of >= table.n_worlds)):
            raise ValueError(f"{who}: world_of must name one world of the table per {per}")
        return world_of

    @staticmethod
    def _grid_pointers(table: WorldTable):
        """(d_grid_bits, d_grid_edges, d_grid_dims, max_nx, max_ny) as the library's grid arguments: NULLs and zeros for a
        table without grids."""
        if table.max_grid is None:
            return None, None, None, 0, 0
        g_ny, g_nx = table.max_grid
        return table.d_grid_bits.data_ptr(), table.d_grid_edges.data_ptr(), table.d_grid_dims.data_ptr(), g_nx, g_ny

    def _points_and_fields(self, who: str, handle, field_of, xy):
        """(m, out, d_blob) of a ``*_distances`` call: the number of points ``xy`` [m,2], the empty f64 [m] answer on the device,
        and -- for m > 0 -- the points followed by their int32 ``field_of`` (one field of ``handle``, or -1, each), sent in ONE
        copy: the points at the buffer's address, field_of 16 * m bytes behind it."""
        xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
        m = len(xy)
        field_of = np.ascontiguousarray(np.asarray(field_of).reshape(-1), np.int32)
        if len(field_of) != m or np.any((field_of < -1) | (field_of >= handle.n)):
            raise ValueError(f"{who}: field_of must name one field of the handle (or -1) per point")
        out = torch.empty((m,), dtype=torch.float64, device=self.device)
        if m == 0:
            return m, out, None
        with torch.cuda.device(self.device):
            blob = np.concatenate([xy.reshape(-1), np.zeros((m + 1) // 2, np.float64)])
            blob[2 * m:].view(np.int32)[:m] = field_of
            return m, out, torch.from_numpy(blob).to(self.device)

    def _rooms_world_of(self, tf) -> np.ndarray:
        """The rooms world: every camera of ``tf`` stands in row 0 of the renderer's own table."""
        return np.zeros(np.size(tf) // 16, np.int32)

    def cast_cameras(self, tf: np.ndarray, hfov: Optional[np.ndarray] = None, min_depth=None, max_depth=None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[n,H,W] f32 normalised depth seen from n camera -> episodic transforms [n,4,4] (yaw about z; a camera is just another
        pose for the ray caster), ONE kernel launch on the current stream: position tf[:, :2, 3], heading (cos, sin) =
        tf[:, :2, 0], height tf[:, 2, 3]; ``hfov`` [n] per camera (None = the renderer's); ``min_depth`` / ``max_depth`` [n]: each
        camera's own range, which its frame is normalised to (None = 0.5 / 5 m), so that a short-range camera sees a far wall as
        "beyond range", not nearer.  Walls only (the painter of scripted objects belongs to ``render``), bit for bit
        synthetic.render_objects_numpy(x, y, c, s, height, fx, lo, hi, H, W, [])[0].  ``out``: a contiguous f32 [n,H,W] device
        tensor to render into."""
        return self._raycast("cast_cameras", tf, self.table, self._rooms_world_of(tf), None, None, hfov, min_depth, max_depth,
                             out)[0]

    def cast_cameras_objects(self, tf: np.ndarray, objects: np.ndarray, env_of, hfov: Optional[np.ndarray] = None,
                             min_depth=None, max_depth=None, out: Optional[torch.Tensor] = None):
        """``cast_cameras`` with the objects of the cameras' environments standing in the world: ``objects`` [n_envs,8,8] f64 on
        the host -- x0, y0, x1, y1, z0, z1, valid, pad per slot -- and ``env_of`` [n], the row of ``objects`` each camera looks
        at.  Returns (depth f32 [n,H,W], ids u8 [n,H,W]: 0 = wall / floor, k + 1 = object slot k, stats int32 [n,8,5]: visible
        pixels, first / last column, first / last row of each slot; (0, W, -1, H, -1) for none), all on the device, bit for bit
        synthetic.render_objects_numpy / object_stats_numpy.  ``out``: the depth buffer, as in ``cast_cameras``."""
        return self._raycast("cast_cameras_objects", tf, self.table, self._rooms_world_of(tf), np.asarray(objects, np.float64),
                             env_of, hfov, min_depth, max_depth, out)[:3]

    def cast_worlds(self, tf: np.ndarray, table: WorldTable, world_of, objects: Optional[np.ndarray] = None, env_of=None,
                    hfov: Optional[np.ndarray] = None, min_depth=None, max_depth=None, out: Optional[torch.Tensor] = None):
        """``cast_cameras_objects`` with a floor plan per camera: camera i stands in world ``world_of[i]`` of ``table`` and sees
        the objects ``objects[env_of[i]]``.  Returns (depth, ids, stats) as ``cast_cameras_objects`` does, bit for bit
        synthetic.render_objects_numpy(..., boxes=table.world(world_of[i])); with ``objects=None`` the walls-only frames, as
        ``cast_cameras`` returns them."""
        res = self._raycast("cast_worlds", tf, table, world_of, objects, env_of, hfov, min_depth, max_depth, out)
        return res[0] if objects is None else res[:3]

    def cast_worlds_rgb(self, tf: np.ndarray, table: WorldTable, world_of, objects: Optional[np.ndarray] = None, env_of=None,
                        colours=None, palette=None, hfov: Optional[np.ndarray] = None, min_depth=None, max_depth=None,
                        out: Optional[torch.Tensor] = None, rgb_out: Optional[torch.Tensor] = None):
        """``cast_worlds`` and the cameras' RGB view of the same worlds from the same launch.  Returns (depth, ids, stats, rgb u8
        [n,H,W,3]) -- always all four; ``objects=None`` is a world without objects: ids of zeros -- with (depth, ids, stats) bit
        for bit ``cast_worlds``' and rgb every byte synthetic.render_rgb_numpy's.  ``colours`` int [n_envs,8]: packed 0x00RRGGBB
        of each slot of ``objects`` (None: zeros); ``palette`` int [12] (None: synthetic.WORLD_PALETTE).  ``rgb_out``: a
        contiguous u8 [n,H,W,3] device tensor to render into."""
        return self._raycast("cast_worlds_rgb", tf, table, world_of, objects, env_of, hfov, min_depth, max_depth, out, True,
                             colours, palette, rgb_out)

    def cast_cameras_rgb(self, tf: np.ndarray, objects: Optional[np.ndarray] = None, env_of=None, colours=None, palette=None,
                         hfov: Optional[np.ndarray] = None, min_depth=None, max_depth=None, out: Optional[torch.Tensor] = None,
                         rgb_out: Optional[torch.Tensor] = None):
        """``cast_worlds_rgb`` for the rooms world.  (depth, ids, stats) are bit for bit ``cast_cameras_objects``'."""
        return self._raycast("cast_cameras_rgb", tf, self.table, self._rooms_world_of(tf), objects, env_of, hfov, min_depth,
                             max_depth, out, True, colours, palette, rgb_out)

    @torch.no_grad()
    def sense_depth(self, clean: torch.Tensor, sensor: DepthSensor, env_ids, clocks, min_depth=None, max_depth=None,
                    out: Optional[torch.Tensor] = None, invalid_out: Optional[torch.Tensor] = None, band_rows: int = 0):
        """What the depth camera ``sensor`` makes of the clean frames ``clean`` (contiguous f32 [n,H,W] on the renderer's device,
        as the ``cast_*`` methods write them): frame i belongs to environment ``env_ids[i]`` at sensor clock ``clocks[i]`` and to
        a camera of the range ``min_depth[i]`` .. ``max_depth[i]`` (None = 0.5 / 5 m).  ONE launch on the current stream
        (vlfm_depth_sensor), bit for bit synthetic.depth_sensor_numpy per frame; the frames' keys and ranges cross in one small
        host-to-device copy.  Returns (frames f32 [n,H,W], invalid int32 [n]: the invalid pixels of each frame), both on the
        device.  ``out`` / ``invalid_out``: tensors to write into; ``out`` must not share storage with ``clean`` (the edge stage
        reads clean neighbours).  ``band_rows``: rows per workgroup (0: planned).  Everything is checked before the launch."""
        dev = self.device
        if not isinstance(sensor, DepthSensor):
            raise ValueError("sense_depth: sensor must be a synthetic.DepthSensor")
        if not isinstance(clean, torch.Tensor) or clean.dtype != torch.float32 or clean.dim() != 3 or \
                tuple(clean.shape[1:]) != (self.H, self.W) or not clean.is_contiguous() or clean.device != dev:
            raise ValueError(f"sense_depth: clean must be a contiguous f32 [n,{self.H},{self.W}] tensor on {dev}")
        n = clean.shape[0]
        if n > 65535:
            raise ValueError("sense_depth: at most 65535 frames per call")
        env_ids, clocks = np.asarray(env_ids).reshape(-1), np.asarray(clocks).reshape(-1)
        if len(env_ids) != n or len(clocks) != n or (n > 0 and (env_ids.dtype.kind not in "iu" or clocks.dtype.kind not in "iu")):
            raise ValueError("sense_depth: env_ids and clocks must hold one integer per frame")
        rng = np.empty((n, 2), np.float32)
        rng[:, 0] = MIN_DEPTH if min_depth is None else np.asarray(min_depth, np.float64)
        rng[:, 1] = MAX_DEPTH if max_depth is None else np.asarray(max_depth, np.float64)
        if not np.all(rng[:, 1] > rng[:, 0]):
            raise ValueError("sense_depth: every camera needs max_depth > min_depth")
        band_rows = int(band_rows)
        if band_rows < 0:
            raise ValueError("sense_depth: band_rows must not be negative")
        if out is None:
            out = torch.empty_like(clean)
        elif not isinstance(out, torch.Tensor) or out.shape != clean.shape or out.dtype != torch.float32 or \
                not out.is_contiguous() or out.device != dev:
            raise ValueError(f"sense_depth: out must be a contiguous f32 [{n},{self.H},{self.W}] tensor on {dev}")
        elif out is clean or (n > 0 and out.untyped_storage().data_ptr() == clean.untyped_storage().data_ptr()):
            raise ValueError("sense_depth: out must not share storage with clean (the edge stage reads clean neighbours)")
        if invalid_out is None:
            invalid_out = torch.empty((n,), dtype=torch.int32, device=dev)
        elif not isinstance(invalid_out, torch.Tensor) or tuple(invalid_out.shape) != (n,) or invalid_out.dtype != torch.int32 or \
                not invalid_out.is_contiguous() or invalid_out.device != dev:
            raise ValueError(f"sense_depth: invalid_out must be a contiguous int32 [{n}] tensor on {dev}")
        if n == 0:
            return out, invalid_out
        t_drop, t_patch = sensor.thresholds()
        blob = np.concatenate([sensor.frame_keys(env_ids, clocks), rng.reshape(-1).view(np.uint32)]).view(np.int32)      # keys [n], ranges [n][2]
        with torch.cuda.device(dev):
            d_blob = torch.from_numpy(blob).to(dev)
            p = d_blob.data_ptr()
            _lib.check(_lib.lib().vlfm_depth_sensor(
                clean.data_ptr(), out.data_ptr(), n, self.H, self.W, p, p + 4 * n, sensor.sigma0_m, sensor.sigma2_per_m,
                sensor.disparity_k, t_drop, t_patch, sensor.edge_m, sensor.min_range_m, sensor.max_range_m,
                invalid_out.data_ptr(), band_rows, torch.cuda.current_stream().cuda_stream), "depth_sensor")
        return out, invalid_out

    def filter_depth(self, frames: torch.Tensor, flt: DepthFilter, out: Optional[torch.Tensor] = None,
                     counts_out: Optional[torch.Tensor] = None):
        """The holes of ``frames`` (contiguous f32 [n,H,W] on the renderer's device) filled by ``flt``, a synthetic.DepthFilter:
        utils.depth_filter.filter_depth_batch (vlfm_depth_filter: two launches on the current stream, nothing read back, bit for
        bit synthetic.depth_filter_numpy per frame).  Returns (frames, counts int32 [n,2]: filled, left), both on the device."""
        from .utils.depth_filter import filter_depth_batch

        if not isinstance(frames, torch.Tensor) or frames.device != self.device or tuple(frames.shape[1:]) != (self.H, self.W):
            raise ValueError(f"filter_depth: frames must be a contiguous f32 [n,{self.H},{self.W}] tensor on {self.device}")
        return filter_depth_batch(frames, flt, out=out, counts_out=counts_out)

    def geodesic_fields(self, objects: np.ndarray, targets_boxes, success_distance: float,
                        max_sources: int = GEODESIC_MAX_SOURCES) -> GeodesicFields:
        """``geodesic_fields_worlds`` for the rooms world: every field stands in the renderer's own table."""
        return self.geodesic_fields_worlds(self.table, np.zeros(len(objects), np.int32), objects, targets_boxes, success_distance,
                                           max_sources)

    @torch.no_grad()
    def geodesic_fields_worlds(self, table: WorldTable, world_of, objects: np.ndarray, targets_boxes, success_distance: float,
                               max_sources: int = GEODESIC_MAX_SOURCES) -> GeodesicFields:
        """The geodesic fields of n environments in ONE launch on the current stream (vlfm_geodesic_fields, bit for bit
        synthetic.geodesic_field_numpy): ``objects`` [n,8,8] f64 on the host, the ray caster's records; the obstacles of field
        i are the walls of world ``world_of[i]`` of ``table`` and the valid footprints of ``objects[i]``, inflated by
        STEP_MARGIN, i.e. synthetic.inflated_rects(objects[i], STEP_MARGIN, table.world(world_of[i])).  ``targets_boxes``
        [n,>=4]: the footprint each environment has to reach within ``success_distance`` (a NaN row: no target, every distance
        in that field is inf).  The view points (synthetic.goal_viewpoints) are worked out on the host; they, their counts and
        world_of cross in one small copy, the records in another.  The handle is strided by R = table.max_boxes + 8;
        ``geodesic_distances`` and ``GeodesicFields.assign`` take it as they take any other."""
        objects = np.ascontiguousarray(objects, np.float64)
        if objects.ndim != 3 or objects.shape[1:] != (WORLD_MAX_OBJECTS, 8):
            raise ValueError(f"geodesic_fields_worlds: objects must be [n, {WORLD_MAX_OBJECTS}, 8]")
        n = len(objects)
        dev = self.device
        if table.device != dev:
            raise ValueError(f"geodesic_fields_worlds: the world table must live on {dev}")
        world_of = self._checked_world_of("geodesic_fields_worlds", table, world_of, n, "field")
        boxes = np.asarray(targets_boxes, np.float64).reshape(n, -1)[:, :4] if n else np.zeros((0, 4))
        # sources, their counts and world_of in one host buffer: [n][max_sources][2] doubles, then two int32 lists
        pad = (n + 1) // 2
        blob = np.zeros(n * max_sources * 2 + 2 * pad)
        src = blob[:n * max_sources * 2].reshape(n, max_sources, 2)
        cnt = blob[n * max_sources * 2:].view(np.int32)[:n]
        blob[n * max_sources * 2 + pad:].view(np.int32)[:n] = world_of
        has = np.zeros(n, bool)
        for e in range(n):
            if np.all(np.isfinite(boxes[e])):
                pts = goal_viewpoints(boxes[e], inflated_rects(objects[e], STEP_MARGIN, table.world(world_of[e])),
                                      success_distance, max_sources)
                src[e, :len(pts)], cnt[e], has[e] = pts, len(pts), True
        R = table.max_boxes + WORLD_MAX_OBJECTS
        f64 = dict(dtype=torch.float64, device=dev)
        h = GeodesicFields(n, max_sources, torch.empty((n, R, 4), **f64), torch.empty((n, 4 * R, 2), **f64),
                           torch.empty((n, 4 * R), **f64), torch.empty((n, 2), dtype=torch.int32, device=dev),
                           torch.empty((n, max_sources, 2), **f64), torch.empty((n,), dtype=torch.int32, device=dev), has)
        if n == 0:
            return h
        with torch.cuda.device(dev):
            d_obj = torch.from_numpy(objects).to(dev)
            d_blob = torch.from_numpy(blob).to(dev)
            h.sources.copy_(d_blob[:n * max_sources * 2].view(n, max_sources, 2))
            h.source_counts.copy_(d_blob[n * max_sources * 2:].view(torch.int32)[:n])
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(_lib.lib().vlfm_geodesic_fields(
                table.d_boxes.data_ptr(), table.d_counts.data_ptr(), table.n_worlds, table.max_boxes,
                d_blob.data_ptr() + 8 * (n * max_sources * 2 + pad), STEP_MARGIN, d_obj.data_ptr(), h.sources.data_ptr(),
                h.source_counts.data_ptr(), n, max_sources, h.rects.data_ptr(), h.nodes.data_ptr(), h.dist.data_ptr(),
                h.counts.data_ptr(), stream), "geodesic_fields")
        return h

    @torch.no_grad()
    def geodesic_distances(self, handle: GeodesicFields, field_of, xy) -> torch.Tensor:
        """f64 [m] on the device: the geodesic distance to the goal of the points ``xy`` [m,2], point i in the field
        ``field_of[i]`` of ``handle`` (-1: no field, the answer is NaN), ONE launch on the current stream
        (vlfm_geodesic_query, bit for bit synthetic.geodesic_query_numpy).  inf: no way to the goal."""
        m, out, d_blob = self._points_and_fields("geodesic_distances", handle, field_of, xy)
        if m == 0:
            return out
        with torch.cuda.device(self.device):
            p = d_blob.data_ptr()
            stream = torch.cuda.current_stream().cuda_stream
            n_boxes = handle.rects.shape[1] - WORLD_MAX_OBJECTS     # the stride the handle was built with (walls + 8)
            _lib.check(_lib.lib().vlfm_geodesic_query(p, p + 16 * m, m, handle.n, n_boxes, handle.rects.data_ptr(),
                                                      handle.nodes.data_ptr(), handle.dist.data_ptr(), handle.counts.data_ptr(),
                                                      handle.sources.data_ptr(), handle.source_counts.data_ptr(),
                                                      handle.max_sources, out.data_ptr(), stream), "geodesic_query")
        return out

    @torch.no_grad()
    def lattice_fields_worlds(self, table: WorldTable, world_of, objects: np.ndarray, targets_boxes, success_distance: float,
                              cells_per_metre: int = 20, pad_m: float = 1.0, max_cost: int = LATTICE_MAX_COST,
                              max_sources: int = GEODESIC_MAX_SOURCES) -> LatticeFields:
        """``geodesic_fields_worlds`` on the metric lattice (synthetic.py, "Lattice geodesic"), for worlds of any number of
        boxes and for grid worlds: TWO launches on the current stream -- vlfm_lattice_free builds the bit-packed free plane of
        every field from the table's rows (boxes and grids) and the records ``objects`` [n,8,8], bit for bit
        synthetic.lattice_free_numpy; vlfm_lattice_fields grows the uint16 cost fields from the view points, bit for bit
        synthetic.lattice_field_numpy.  Extents (synthetic.lattice_extent) and view points (synthetic.goal_viewpoints, the
        table's grid included) are worked out on the host; the source nodes, their counts, the dims and world_of cross in one
        copy, the records in another.  A field wider than 1024 nodes, or more than ``max_sources`` view points: ValueError
        before anything is launched."""
        objects = np.ascontiguousarray(objects, np.float64)
        if objects.ndim != 3 or objects.shape[1:] != (WORLD_MAX_OBJECTS, 8):
            raise ValueError(f"lattice_fields_worlds: objects must be [n, {WORLD_MAX_OBJECTS}, 8]")
        n, cpm, max_cost = len(objects), int(cells_per_metre), int(max_cost)
        dev = self.device
        if table.device != dev:
            raise ValueError(f"lattice_fields_worlds: the world table must live on {dev}")
        if not 0 <= max_cost <= LATTICE_MAX_COST:
            raise ValueError(f"lattice_fields_worlds: max_cost in [0, {LATTICE_MAX_COST}]")
        world_of = self._checked_world_of("lattice_fields_worlds", table, world_of, n, "field")
        boxes = np.asarray(targets_boxes, np.float64).reshape(n, -1)[:, :4] if n else np.zeros((0, 4))
        # source nodes [n][max_sources][2], counts [n], dims [n][4], world_of [n]: one int32 buffer
        blob = np.zeros(n * (2 * max_sources + 6), np.int32)
        src = blob[:2 * n * max_sources].reshape(n, max_sources, 2)
        cnt = blob[2 * n * max_sources:][:n]
        dims = blob[2 * n * max_sources + n:][:4 * n].reshape(n, 4)
        blob[2 * n * max_sources + 5 * n:] = world_of
        has = np.zeros(n, bool)
        lattice_extent(np.zeros((0, 4)), None, None, cpm, pad_m)            # (the spacing and the pad, checked even for n == 0)
        for e in range(n):
            walls, grid = table.world(world_of[e]), table.grids[world_of[e]]
            dims[e] = lattice_extent(walls, grid, objects[e], cpm, pad_m)
            if np.all(np.isfinite(boxes[e])):
                pts = goal_viewpoints(boxes[e], inflated_rects(objects[e], STEP_MARGIN, walls), success_distance, max_sources,
                                      grid=grid)
                src[e, :len(pts)], cnt[e], has[e] = lattice_sources(pts, cpm), len(pts), True
        max_na, max_nb = (int(dims[:, 2].max()), int(dims[:, 3].max())) if n else (1, 1)
        h = LatticeFields(n, cpm, torch.empty((n, max_nb, (max_na + 31) // 32), dtype=torch.int32, device=dev),
                          torch.empty((n, max_nb, max_na), dtype=torch.int16, device=dev),
                          torch.empty((n, 4), dtype=torch.int32, device=dev), dims.copy(), has)
        if n == 0:
            return h
        with torch.cuda.device(dev):
            L = _lib.lib()
            d_obj = torch.from_numpy(objects).to(dev)
            d_blob = torch.from_numpy(blob).to(dev)
            p = d_blob.data_ptr()
            p_cnt, p_dims, p_world = p + 8 * n * max_sources, p + 8 * n * max_sources + 4 * n, p + 8 * n * max_sources + 20 * n
            h.dims.copy_(d_blob[2 * n * max_sources + n:][:4 * n].view(n, 4))
            g_bits, g_edges, g_dims, g_nx, g_ny = self._grid_pointers(table)
            stream = torch.cuda.current_stream().cuda_stream
            _lib.check(L.vlfm_lattice_free(table.d_boxes.data_ptr(), table.d_counts.data_ptr(), table.n_worlds, table.max_boxes,
                                           g_bits, g_edges, g_dims, g_nx, g_ny, p_world, STEP_MARGIN, d_obj.data_ptr(), p_dims, n,
                                           cpm, max_nb, max_na, h.bits.data_ptr(), stream), "lattice_free")
            h.residence = self._launch_lattice_fields(h, p, p_cnt, max_sources, max_cost)
        return h

    def _launch_lattice_fields(self, h: LatticeFields, d_sources: int, d_source_counts: int, max_sources: int,
                             max_cost: int = LATTICE_MAX_COST) -> int:
        """vlfm_lattice_fields over the free planes ``h.bits`` and ``h.dims`` as they stand -- whatever wrote them --, into
        ``h.dist``, on the current stream: ``d_sources`` / ``d_source_counts`` are device addresses of int32 [n][max_sources][2]
        global nodes and [n] counts.  Returns where the bit planes lived (_lib.LATTICE_IN_LDS / LATTICE_IN_SCRATCH / LATTICE_ALL_IN_SCRATCH)."""
        L = _lib.lib()
        max_nb, max_na = h.dist.shape[1:]
        need = L.vlfm_lattice_scratch_bytes(h.n, max_nb, max_na)
        scratch = torch.empty((need,), dtype=torch.uint8, device=self.device) if need else None
        return _lib.check(L.vlfm_lattice_fields(h.bits.data_ptr(), h.dims.data_ptr(), h.n, max_nb, max_na, d_sources,
                                                d_source_counts, max_sources, max_cost, h.dist.data_ptr(),
                                                scratch.data_ptr() if need else None, need,
                                                torch.cuda.current_stream().cuda_stream), "lattice_fields")

    @torch.no_grad()
    def lattice_distances(self, handle: LatticeFields, field_of, xy) -> torch.Tensor:
        """f64 [m] on the device: the lattice geodesic distance to the goal of the points ``xy`` [m,2], point i in the field
        ``field_of[i]`` of ``handle`` (-1: no field, the answer is NaN), ONE launch on the current stream (vlfm_lattice_query,
        bit for bit synthetic.lattice_query_numpy).  inf: no way to the goal."""
        m, out, d_blob = self._points_and_fields("lattice_distances", handle, field_of, xy)
        if m == 0:
            return out
        with torch.cuda.device(self.device):
            p = d_blob.data_ptr()
            max_nb, max_na = handle.dist.shape[1:]
            _lib.check(_lib.lib().vlfm_lattice_query(p, p + 16 * m, m, handle.n, handle.dist.data_ptr(), handle.dims.data_ptr(),
                                                     max_nb, max_na, handle.cells_per_metre, out.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "lattice_query")
        return out

    def prepare(self, t0: int, n: int) -> None:
        self.window = torch.stack([self.render((t0 + i) % self.L) for i in range(n)])
        self.window_t0 = t0

    def frame(self, t: int) -> torch.Tensor:
        if self.window is not None and 0 <= t - self.window_t0 < self.window.shape[0]:
            return self.window[t - self.window_t0]
        return self.render(t)


def check_geodesic_backend(geodesic, objectnav_metrics: bool, worlds) -> None:
    """What ``LiveWorld`` and ``BatchedEpisodes`` refuse about ``geodesic`` before any device is touched: a name that is neither
    backend, "lattice" without the metrics it serves, and grid worlds scored by the visibility graph."""
    if geodesic not in ("graph", "lattice"):
        raise ValueError(f'geodesic must be "graph" or "lattice", not {geodesic!r}')
    if geodesic == "lattice" and not objectnav_metrics:
        raise ValueError('geodesic="lattice" is a backend of objectnav_metrics: it needs objectnav_metrics=True')
    if objectnav_metrics and geodesic == "graph" and getattr(worlds, "max_grid", None) is not None:
        raise ValueError('grid worlds cannot be combined with objectnav_metrics over the visibility graph: the geodesic fields '
                         'hold at most 141 rectangles; geodesic="lattice" scores them')


class LiveWorld:
    """The closed-loop world of ``BatchedEpisodes(closed_loop=True)`` (its ``live``): E robots that stand where their actions
    took them.  ``observe()`` ray-casts what they see -- one launch of ``renderer`` (a RoomsRenderer) -- and ``advance()``
    moves them (synthetic.step_poses).  ``worlds``: every environment in its own floor plan, a row of ``table`` each, else all
    in the renderer's rooms world; ``world_objects``: objects stand in the worlds and the environments run ObjectNav episodes
    (``start_episodes`` / ``end_episodes``, scored in ``objectnav_stats``; ``objectnav_metrics``: also SPL, SoftSPL, geodesic
    distance -- ``geodesic``: "graph", the visibility graph over at most 141 rectangles (GeodesicFields), or "lattice", the
    metric lattice that also holds grid worlds (LatticeFields)); ``render_rgb``: the colour view too.  Every attribute exists
    in every mode; what a mode does not use is None.  ``depth_sensor``: a synthetic.DepthSensor between the ray caster and every
    reader of ``frames`` (``clean_frames`` keeps the exact ranges).  ``depth_filter``: a synthetic.DepthFilter after the sensor (or,
    without one, after the ray caster): ``frames`` is then the filter's output and ``sensed_frames`` its input."""

    def __init__(self, renderer, env_ids, targets, world_objects: Optional[WorldObjects] = None, worlds=None,
                 objectnav_metrics: bool = False, render_rgb: bool = False, geodesic: str = "graph",
                 depth_sensor: Optional[DepthSensor] = None, depth_filter: Optional[DepthFilter] = None) -> None:
        self.renderer, self.env_ids, self.targets = renderer, list(env_ids), list(targets)
        if depth_sensor is not None and not isinstance(depth_sensor, DepthSensor):
            raise ValueError("depth_sensor must be a synthetic.DepthSensor")
        if depth_filter is not None and not isinstance(depth_filter, DepthFilter):
            raise ValueError("depth_filter must be a synthetic.DepthFilter")
        self.world_objects, self.worlds = world_objects, worlds
        self.objectnav_metrics, self.render_rgb = bool(objectnav_metrics), bool(render_rgb)
        check_geodesic_backend(geodesic, self.objectnav_metrics, worlds)
        self.geodesic_backend = geodesic
        E = self.E = len(self.env_ids)
        z = lambda dt: np.zeros(E, dt)   # noqa: E731
        # an episode starts at the environment's open-loop start pose (diverse, in free space), with ``worlds`` at its world's
        self.start_xy, self.start_k = renderer.pose_table[0][:, :2].copy(), renderer.k_table[0].copy()
        self.xy, self.k, self.collided = self.start_xy.copy(), self.start_k.copy(), z(bool)
        # where each robot's walls are: a row per environment with ``worlds``, else the renderer's one row for everybody
        self.table, self.world_of, self.world_episode = renderer.table, z(np.int32), None
        if worlds is not None:
            self.table = WorldTable(E, renderer.device, max_grid=getattr(worlds, "max_grid", None))
            self.world_of, self.world_episode = np.arange(E, dtype=np.int32), np.full(E, -1, np.int64)    # (its world's episode)
        self.stats = {"path_length": z(np.float64), "collisions": z(np.int64), "forward_steps": z(np.int64),
                      "turn_steps": z(np.int64), "stops": z(np.int64)}
        # the last observe(): depth, with objects the id plane, the per-slot statistics (host) and the sightings, the colours;
        # world_objects: the ray caster's records [E,8,8], the class names of the slots, the slot of the target (-1: none)
        self.frames = self.ids = self.seen_stats = self.sightings = self.rgb = self.objects = self.object_classes = self.target_slot = None
        self.ep_index = self.ep_clock = self.ep_path = self.ep_first = self.objectnav_stats = None
        self.distance_to_goal = self.ep_geodesic = self.geodesic = None   # objectnav_metrics: now; at the episode's start; the fields
        # depth_sensor: ``frames`` is what the depth camera makes of ``clean_frames``, the ray caster's (and painter's) output;
        # ``sensor_clock`` [E]: the noted observations of each environment so far; ``sensor_invalid``: the last counts (device)
        self.depth_sensor, self.clean_frames, self.sensor_invalid = depth_sensor, None, None
        self.sensor_clock = None if depth_sensor is None else z(np.int64)
        # depth_filter: ``frames`` is what the filter makes of ``sensed_frames`` -- the sensor's output, or without a sensor the
        # ray caster's (and painter's) --, a buffer the world keeps; ``filter_counts`` [E,2]: the last filled / left counts (device)
        self.depth_filter, self.sensed_frames, self.filter_counts = depth_filter, None, None
        if world_objects is not None:
            self.objects, self.sightings = np.zeros((E, WORLD_MAX_OBJECTS, 8)), []
            self.object_classes: List[List[str]] = [[] for _ in range(E)]
            self.target_slot = np.full(E, -1, np.int64)
            self.ep_index, self.ep_clock, self.ep_path, self.ep_first = z(np.int64), z(np.int64), z(np.float64), z(np.int64) - 1
            self.objectnav_stats = {"episodes": z(np.int64), "successes": z(np.int64), "wrong_stops": z(np.int64),
                                    "no_frontier_stops": z(np.int64), "timeouts": z(np.int64), "episode_env": [], "episode_outcome": [],
                                    "episode_steps": [], "episode_path_length": [], "episode_first_sighting": []}
            if self.objectnav_metrics:
                self.objectnav_stats.update({"episode_geodesic": [], "episode_distance_to_goal": [], "episode_spl": [],
                                             "episode_soft_spl": []})
                self.distance_to_goal, self.ep_geodesic = np.full(E, np.nan), np.full(E, np.nan)
        self.start_episodes(range(E))

    def poses_tf(self):
        """(poses [E,3] = x, y, yaw; robot -> episodic transforms [E,4,4]) of where the robots are."""
        yaw = np.array(YAWS)[self.k]
        return (np.concatenate([self.xy, yaw[:, None]], axis=1), np.stack([tf_of(x, y, k) for (x, y), k in zip(self.xy, self.k)]))

    def observe(self, painter=None, t_ep: int = 0, fresh: bool = False, tf=None) -> torch.Tensor:
        """The robots' own depth frames [E,H,W], ONE kernel launch, into ``frames``, a buffer the world keeps (every reader of the
        previous step's frames was joined back into the main stream); ``render_rgb``: also ``rgb`` (objects in OBJECT_COLOURS of
        their classes, else mid grey).  ``tf``: what ``poses_tf()`` returns for the CURRENT poses, from a caller that already holds
        it (nothing checks that; None: computed here).  With objects it notes what the ray caster saw (``ids``, ``seen_stats``,
        ``sightings``: the one extra D2H copy of that mode); without, ``painter(t_ep, frames)`` paints scripted ones in.
        ``fresh``: new buffers, nothing noted, no colours.  ``depth_sensor``: the ray caster (and the painter) write
        ``clean_frames`` and the sensor -- one more launch -- writes ``frames``, which is what is returned; ids, statistics and
        colours stay what the ray caster saw.  A noted observation advances ``sensor_clock``; a ``fresh`` one is sensed with the
        clock the next noted one will use.  ``depth_filter``: last of all the filter -- two more launches -- fills the holes of
        ``sensed_frames`` (the sensor's output, else the ray caster's and painter's) into ``frames``; ``fresh``: into new buffers."""
        r, wo = self.renderer, self.world_objects
        tf = self.poses_tf()[1] if tf is None else tf
        if self.frames is None and not fresh:
            self.frames = torch.empty((self.E, r.H, r.W), dtype=torch.float32, device=r.device)
        sensor, flt = self.depth_sensor, self.depth_filter
        if sensor is not None and self.clean_frames is None and not fresh:
            self.clean_frames = torch.empty((self.E, r.H, r.W), dtype=torch.float32, device=r.device)
        if flt is not None and self.sensed_frames is None and not fresh:
            self.sensed_frames = torch.empty((self.E, r.H, r.W), dtype=torch.float32, device=r.device)
        out = None if fresh else (self.frames if sensor is None else self.clean_frames)
        if flt is not None and sensor is None and not fresh:
            out = self.sensed_frames
        objects, env_of = (None, None) if wo is None else (self.objects, np.arange(self.E))
        if self.render_rgb and not fresh:
            if self.rgb is None:
                self.rgb = torch.empty((self.E, r.H, r.W, 3), dtype=torch.uint8, device=r.device)
            colours = None
            if wo is not None:
                colours = np.zeros((self.E, WORLD_MAX_OBJECTS), np.int32)
                for e, classes in enumerate(self.object_classes):
                    colours[e, :len(classes)] = [OBJECT_COLOURS.get(c, 0x808080) for c in classes]
            d, ids, stats, _ = r.cast_worlds_rgb(tf, self.table, self.world_of, objects, env_of, colours, out=out, rgb_out=self.rgb)
        else:
            seen = r.cast_worlds(tf, self.table, self.world_of, objects, env_of, out=out)
            d, ids, stats = (seen, None, None) if wo is None else seen
        if wo is None:
            d = painter(t_ep, d) if painter is not None else d
        elif not fresh:
            self.ids, self.seen_stats = ids, stats.cpu().numpy()
            self.sightings = sightings_from_stats(self.seen_stats, self.object_classes, wo.min_pixels, wo.confidence,
                                                  wo.faint_confidence)
            for (e, _, conf, _, k) in self.sightings:
                if k == self.target_slot[e] and conf == wo.confidence and self.ep_first[e] < 0:
                    self.ep_first[e] = self.ep_clock[e]
        d = d if sensor is None else self._sense(d, fresh)
        return d if flt is None else self._filter(d, fresh)

    def _sense(self, clean: torch.Tensor, fresh: bool) -> torch.Tensor:
        """The depth camera's view of the ``clean`` frames of this observation (RoomsRenderer.sense_depth: one launch, nothing
        read back): into ``frames`` (with a ``depth_filter``: ``sensed_frames``) and noted, or ``fresh``: new buffers at the clock
        the next noted observation will use."""
        keep = self.frames if self.depth_filter is None else self.sensed_frames
        sensed, invalid = self.renderer.sense_depth(clean, self.depth_sensor, self.env_ids, self.sensor_clock,
                                                    out=None if fresh else keep)
        if not fresh:
            self.clean_frames, self.sensor_invalid = clean, invalid
            self.sensor_clock += 1
        return sensed

    def _filter(self, sensed: torch.Tensor, fresh: bool) -> torch.Tensor:
        """The holes of this observation's ``sensed`` frames filled (RoomsRenderer.filter_depth: two launches, nothing read back):
        into ``frames`` and noted, or ``fresh``: new buffers, nothing noted."""
        filled, counts = self.renderer.filter_depth(sensed, self.depth_filter, out=None if fresh else self.frames)
        if not fresh:
            self.sensed_frames, self.filter_counts = sensed, counts
        return filled

    def advance(self, actions, ended) -> np.ndarray:
        """The step's ``actions`` [E] move the robots (synthetic.step_poses: refused by their worlds' walls and the objects'
        footprints); with objects, an episode that ``ended`` [E] with this step takes STOP.  Returns the actions taken."""
        acts, extra = np.asarray(actions, np.int64).reshape(self.E), None
        if self.world_objects is not None:
            acts = np.where(ended, ACTION_STOP, acts)
            extra = np.where(self.objects[:, :, 6:7] != 0.0, self.objects[:, :, :4], np.nan)
        grid_worlds = self.worlds is not None and self.table.max_grid is not None
        self.xy, self.k, self.collided = step_poses(self.xy, self.k, acts, extra, None if self.worlds is None else self.table.boxes,
                                                    self.table.grids if grid_worlds else None)
        st, fwd = self.stats, acts == ACTION_FORWARD
        st["forward_steps"] += fwd
        st["collisions"] += self.collided
        st["turn_steps"] += (acts == ACTION_TURN_LEFT) | (acts == ACTION_TURN_RIGHT)
        st["stops"] += acts == ACTION_STOP
        st["path_length"] += 0.25 * (fwd & ~self.collided)
        if self.world_objects is not None:
            self.ep_path += 0.25 * (fwd & ~self.collided)
        return acts

    def start_episodes(self, envs) -> None:
        """The environments ``envs`` start an episode.  ``worlds``: they move into their episodes' worlds (without objects: episode
        0's) -- the table rows cross in one copy -- and stand at those worlds' start poses, nothing refused yet.  Objects: layouts
        are drawn around where the robots stand (``objects``, ``object_classes``, ``target_slot``), the episode counters start over.
        objectnav_metrics: their geodesic fields, ONE launch, and ``ep_geodesic`` -- the distance to the goal from where each robot
        stands (nan: the layout has no target; inf: no way to it)."""
        envs, wo = list(envs), self.world_objects
        if self.worlds is not None:
            episodes = self.ep_index[envs] if wo is not None else np.zeros(len(envs), np.int64)
            made = [self.worlds.world(self.env_ids[e], int(k)) for e, k in zip(envs, episodes)]
            self.table.assign(envs, [w.boxes for w in made], [w.grid for w in made])
            for e, k, w in zip(envs, episodes, made):
                self.start_xy[e], self.start_k[e] = w.start_xy, w.start_k
                self.xy[e], self.k[e] = w.start_xy, w.start_k
                self.collided[e] = False
                self.world_episode[e] = int(k)
        if wo is None:
            return
        layout = self.worlds.layout if self.worlds is not None and wo.layout is object_layout else wo.layout
        for e in envs:
            lay = list(layout(self.env_ids[e], int(self.ep_index[e]), self.xy[e].copy()))
            if len(lay) > WORLD_MAX_OBJECTS:
                raise ValueError(f"a layout may hold at most {WORLD_MAX_OBJECTS} objects")
            self.objects[e] = 0.0
            for k, (_, box) in enumerate(lay):
                self.objects[e, k, :6], self.objects[e, k, 6] = np.asarray(box, np.float64), 1.0
            self.object_classes[e] = [cls for cls, _ in lay]
            self.target_slot[e] = next((k for k, (cls, _) in enumerate(lay) if cls == self.targets[e]), -1)
            self.ep_clock[e], self.ep_path[e], self.ep_first[e] = 0, 0.0, -1
        if not self.objectnav_metrics or not envs:
            return
        envs = np.array(envs, np.int64)
        slots = self.target_slot[envs]
        boxes = np.where((slots >= 0)[:, None], self.objects[envs, np.maximum(slots, 0), :4], np.nan)
        fields = self.renderer.lattice_fields_worlds if self.geodesic_backend == "lattice" else self.renderer.geodesic_fields_worlds
        fresh = fields(self.table, self.world_of[envs], self.objects[envs], boxes, wo.success_distance)
        if self.geodesic is None:               # (the first call starts every environment's episode)
            assert len(envs) == self.E and np.array_equal(envs, np.arange(self.E))
            self.geodesic = fresh
        else:
            self.geodesic.assign(envs, fresh)
        field_of = np.where(fresh.has_target, np.arange(len(envs)), -1)
        self.ep_geodesic[envs] = self._distances(fresh, field_of, self.xy[envs])
        self.distance_to_goal[envs] = self.ep_geodesic[envs]

    def _distances(self, fields, field_of, xy) -> np.ndarray:
        """f64 on the host: the distance to the goal of each point in its field, by the backend's query: one launch, one read-back."""
        r = self.renderer
        ask = r.lattice_distances if self.geodesic_backend == "lattice" else r.geodesic_distances
        return ask(fields, field_of, xy).cpu().numpy()

    def _score(self, e: int, outcome: str) -> None:
        st = self.objectnav_stats
        st["episodes"][e] += 1
        st[{"success": "successes", "wrong_stop": "wrong_stops", "no_frontier": "no_frontier_stops",
            "timeout": "timeouts"}[outcome]][e] += 1
        st["episode_env"].append(e)
        st["episode_outcome"].append(outcome)
        st["episode_steps"].append(int(self.ep_clock[e]))
        st["episode_path_length"].append(float(self.ep_path[e]))
        st["episode_first_sighting"].append(int(self.ep_first[e]))
        if self.objectnav_metrics:
            l, d_end, p = float(self.ep_geodesic[e]), float(self.distance_to_goal[e]), float(self.ep_path[e])
            st["episode_geodesic"].append(l)
            st["episode_distance_to_goal"].append(d_end)
            st["episode_spl"].append(spl(outcome == "success", l, p))
            st["episode_soft_spl"].append(soft_spl(d_end, l, p))

    def end_episodes(self, modes, stops) -> List[int]:
        """Objects, after the policy decided (``modes``, ``stops`` [E]): the environments whose episode ends with this step
        (objectnav_outcome), scored.  objectnav_metrics: one launch, one read-back judge where the robots are."""
        wo, done = self.world_objects, []
        self.ep_clock += 1                          # this step is taken
        if self.objectnav_metrics:
            field_of = np.where(self.geodesic.has_target, np.arange(self.E), -1)
            self.distance_to_goal = self._distances(self.geodesic, field_of, self.xy)
        for e in range(self.E):
            navigating = bool(modes) and modes[e] == "navigate"
            exploring = bool(modes) and modes[e] == "explore"
            k = int(self.target_slot[e])
            out = objectnav_outcome(bool(stops[e]), navigating, bool(stops[e]) and exploring, int(self.ep_clock[e]),
                                    wo.max_episode_steps, self.xy[e], self.objects[e, k, :4] if k >= 0 else None,
                                    wo.success_distance)
            if out is not None:
                self._score(e, out)
                done.append(e)
        self.ep_index[done] += 1                    # the episodes they start next
        return done

    def reset(self) -> None:
        """The robots return to their start poses; objects: running episodes end as timeouts, everybody starts the next."""
        self.xy, self.k = self.start_xy.copy(), self.start_k.copy()
        self.collided[:] = False
        if self.sensor_clock is not None:
            self.sensor_clock[:] = 0
        if self.world_objects is not None:
            running = np.flatnonzero(self.ep_clock > 0)
            for e in running:
                self._score(int(e), "timeout")
            self.ep_index[running] += 1
            self.start_episodes(range(self.E))

    def instance_of(self, e: int, box_px: np.ndarray) -> int:
        """The object slot behind a detection of environment ``e``'s target class with the pixel box ``box_px`` (xyxy): the
        sighting of that class whose visible bounding box is nearest."""
        best, slot = None, -1
        for (se, phrase, _, (cx, cy, ax, ay), k) in self.sightings:
            if se == e and phrase == self.targets[e]:
                d = float(np.abs(np.array([cx - ax, cy - ay, cx + ax, cy + ay]) - box_px).sum())
                if best is None or d < best:
                    best, slot = d, k
        return slot

    def objectnav_summary(self) -> Dict:
        """The ObjectNav table of the episodes scored so far: ``episodes``, ``success_rate`` and, with objectnav_metrics,
        Habitat's ``spl``, ``soft_spl`` and mean final ``distance_to_goal`` over the episodes that have a finite geodesic
        start distance; the others are counted in ``excluded_no_target`` / ``excluded_unreachable`` and in no mean."""
        st = self.objectnav_stats
        n = len(st["episode_outcome"])
        success = np.array([o == "success" for o in st["episode_outcome"]], bool)
        if not self.objectnav_metrics:
            return {"episodes": n, "success_rate": float(success.mean()) if n else float("nan")}
        l = np.asarray(st["episode_geodesic"], np.float64)
        ok = np.isfinite(l)
        mean = lambda v: float(np.asarray(v, np.float64)[ok].mean()) if ok.any() else float("nan")   # noqa: E731
        return {"episodes": n, "scored": int(ok.sum()), "excluded_no_target": int(np.isnan(l).sum()),
                "excluded_unreachable": int(np.isinf(l).sum()), "success_rate": mean(success), "spl": mean(st["episode_spl"]),
                "soft_spl": mean(st["episode_soft_spl"]), "distance_to_goal": mean(st["episode_distance_to_goal"])}
