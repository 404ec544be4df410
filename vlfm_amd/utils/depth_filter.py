"""The depth filter: holes (zeros, NaN, negatives) filled from the nearest valid pixels of their row and column, on the device
(csrc/depth_filter.hip: vlfm_depth_filter), bit for bit ``synthetic.depth_filter_numpy``.

``filter_depth`` has the call shape of ``depth_camera_filtering.filter_depth``, which the reference runs first on every depth
frame (vlfm/policy/habitat_policies.py:185, vlfm/reality/objectnav_env.py:155,182), so a VLFM checkout can swap the import.  The
RULE is this project's own (synthetic.DepthFilter): it follows that library's contract -- zero pixels are filled from valid
neighbours, originally non-zero pixels are optionally restored -- and claims no arithmetic parity with it; the library's source
is pinned nowhere.  ``filter_depth_batch`` is the batched form the closed loop uses."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _lib
from ..synthetic import DepthFilter


@torch.no_grad()
def filter_depth_batch(frames: torch.Tensor, flt: DepthFilter = DepthFilter(), out: Optional[torch.Tensor] = None,
                       counts_out: Optional[torch.Tensor] = None, band_rows: int = 0):
    """What ``flt`` makes of the frames ``frames`` (contiguous f32 [n,H,W] on a HIP device): two launches and one memset on the
    current stream, nothing read back.  Returns (frames f32 [n,H,W], counts int32 [n,2]: per frame the holes that were filled and
    the holes that were left), both on the device.  ``out`` / ``counts_out``: tensors to write into; ``out`` must not share
    storage with ``frames`` (the candidates are input pixels).  ``band_rows``: rows per workgroup of the column pass (0: planned;
    the result does not depend on it).  Everything is checked before the first launch."""
    if not isinstance(flt, DepthFilter):
        raise ValueError("filter_depth_batch: flt must be a synthetic.DepthFilter")
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32 or frames.dim() != 3 or not frames.is_cuda or \
            not frames.is_contiguous() or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("filter_depth_batch: frames must be a contiguous f32 [n,H,W] tensor on a HIP device, H, W >= 1")
    dev = frames.device
    n, H, W = frames.shape
    if n > 65535:
        raise ValueError("filter_depth_batch: at most 65535 frames per call")
    if H * W >= 2 ** 31:
        raise ValueError("filter_depth_batch: a frame holds fewer than 2**31 pixels")
    if isinstance(band_rows, bool) or not isinstance(band_rows, (int, np.integer)) or band_rows < 0:
        raise ValueError("filter_depth_batch: band_rows must be an integer and not negative")
    if out is None:
        out = torch.empty_like(frames)
    elif not isinstance(out, torch.Tensor) or out.shape != frames.shape or out.dtype != torch.float32 or \
            not out.is_contiguous() or out.device != dev:
        raise ValueError(f"filter_depth_batch: out must be a contiguous f32 [{n},{H},{W}] tensor on {dev}")
    elif out is frames or (n > 0 and out.untyped_storage().data_ptr() == frames.untyped_storage().data_ptr()):
        raise ValueError("filter_depth_batch: out must not share storage with frames (the candidates are input pixels)")
    if counts_out is None:
        counts_out = torch.empty((n, 2), dtype=torch.int32, device=dev)
    elif not isinstance(counts_out, torch.Tensor) or tuple(counts_out.shape) != (n, 2) or counts_out.dtype != torch.int32 or \
            not counts_out.is_contiguous() or counts_out.device != dev:
        raise ValueError(f"filter_depth_batch: counts_out must be a contiguous int32 [{n},2] tensor on {dev}")
    if n == 0:
        return out, counts_out
    black = flt.set_black_value
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().vlfm_depth_filter(
            frames.data_ptr(), out.data_ptr(), n, H, W, 0 if flt.fill == "far" else 1, 0 if flt.reach_px is None else int(flt.reach_px),
            float(flt.clip_far_thresh), int(bool(flt.recover_nonzero)), int(black is not None), 0.0 if black is None else float(black),
            counts_out.data_ptr(), int(band_rows), torch.cuda.current_stream().cuda_stream), "depth_filter")
    return out, counts_out


def filter_depth(depth_img: np.ndarray, clip_far_thresh: float = 0.0, set_black_value: Optional[float] = None,
                 blur_type: Optional[str] = None, recover_nonzero: bool = True, fill: str = "far",
                 reach_px: Optional[int] = None) -> np.ndarray:
    """One host frame [H,W] (or [H,W,1]) through the device filter; returns an f32 array of the input's shape.  The call shape of
    ``depth_camera_filtering.filter_depth`` -- the rule is synthetic.DepthFilter's, not that library's arithmetic (see the
    module's docstring).  ``blur_type`` other than None is refused: blurring is not built (the reference only ever passes
    None).  ``fill`` and ``reach_px`` are this project's additions."""
    if blur_type is not None:
        raise NotImplementedError(f"filter_depth: blur_type={blur_type!r}: blurring is not built; the reference passes None")
    flt = DepthFilter(fill=fill, reach_px=reach_px, clip_far_thresh=clip_far_thresh, recover_nonzero=recover_nonzero,
                      set_black_value=set_black_value)
    img = np.asarray(depth_img)
    plane = img[..., 0] if img.ndim == 3 and img.shape[2] == 1 else img
    if plane.ndim != 2 or plane.shape[0] < 1 or plane.shape[1] < 1:
        raise ValueError("filter_depth: depth_img must be [H,W] or [H,W,1]")
    if not torch.cuda.is_available():
        raise RuntimeError("filter_depth: no HIP device (vlfm_amd has no CPU fallback; the host statement of the rule is "
                           "synthetic.depth_filter_numpy)")
    frames = torch.from_numpy(np.array(plane, np.float32)[None]).cuda()           # (a copy: the caller's array may be read-only)
    out, _ = filter_depth_batch(frames, flt)
    return out[0].cpu().numpy().reshape(img.shape)
