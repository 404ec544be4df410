"""The reference's client -> server image transport, as an opt-in emulation.

Every ``*Client`` of the reference ships its frame as a quality-90 JPEG (vlfm/vlm/server_wrapper.py:57-61 ``image_to_str``,
:126 ``payload[k] = image_to_str(v, quality=kwargs.get("quality", 90))``) and the server decodes it again (:64-68
``str_to_image``), so the reference's models never see the raw frame.  The in-process clients of this package skip the hop;
``emulate_jpeg=True`` on a client reproduces it for A/B fidelity checks.

OpenCV is absent here, so the codec is Pillow's libjpeg binding: same baseline JPEG, same quality scaling of the standard
tables, 4:2:0 chroma subsampling in both.  ``cv2.imencode`` treats the array it is given as BGR; the reference hands it an RGB
frame, so the luma / chroma conversion sees the channels swapped -- reproduced here by swapping around the round trip.
"""
from __future__ import annotations

import io

import numpy as np


def jpeg_roundtrip(image: np.ndarray, quality: int = 90) -> np.ndarray:
    """``str_to_image(image_to_str(image, quality))`` of server_wrapper.py:57-68 for an (H,W,3) u8 frame."""
    from PIL import Image

    img = np.ascontiguousarray(image)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, "expects an (H,W,3) uint8 frame"
    buf = io.BytesIO()
    Image.fromarray(img[..., ::-1].copy()).save(buf, format="JPEG", quality=int(quality), subsampling="4:2:0")
    back = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    return np.ascontiguousarray(back[..., ::-1])


_tables_cache: dict = {}


def jpeg_quant_tables(quality: int) -> np.ndarray:
    """The [2,64] uint16 luma / chroma quantisation tables libjpeg derives for ``quality`` (jcparam.c jpeg_set_quality)."""
    from .. import _lib

    q = int(quality)
    if q not in _tables_cache:
        t = np.zeros(128, np.uint16)
        _lib.check(_lib.lib().vlfm_jpeg_quant_tables_host(q, t.ctypes.data), "jpeg_quant_tables_host")
        _tables_cache[q] = t
    return _tables_cache[q]


JPEG_MAX_DIMENSION = 65500   # libjpeg's limit on a frame side (csrc/jpeg_common.h: kMaxDim)


def _buffer(name: str, t, dtype, shape, device, where: str):
    """``t`` if it is a contiguous tensor of ``dtype`` and ``shape`` on ``device``; a new one for None."""
    import torch

    shape = tuple(int(d) for d in shape)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if (not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape or t.device != device
            or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[-1]} tensor of shape {shape} on {where}")
    return t


def _scratch(scratch, need: int, device):
    import torch

    if scratch is None:
        return torch.empty(need, dtype=torch.uint8, device=device)   # (the caching allocator: no device allocation)
    if (not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.uint8 or scratch.device != device
            or not scratch.is_contiguous() or scratch.numel() < need or scratch.data_ptr() % 16):
        raise ValueError(f"scratch must be a contiguous, 16-byte aligned uint8 device tensor of at least {need} bytes")
    return scratch


def _overlap(a, b) -> bool:
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _no_overlap(bufs) -> None:
    """``bufs``: (name, tensor) pairs, no two of which may share a byte."""
    for i, (na, a) in enumerate(bufs):
        for nb, b in bufs[i + 1:]:
            if _overlap(a, b):
                raise ValueError(f"{nb} must not overlap {na}")


def jpeg_roundtrip_scratch(n: int, height: int, width: int, device) -> "torch.Tensor":
    """A device buffer that ``jpeg_roundtrip_batch(..., scratch=)`` accepts for n frames of height x width."""
    import torch

    from .. import _lib

    return torch.empty(int(_lib.lib().vlfm_jpeg_scratch_bytes(n, height, width)), dtype=torch.uint8, device=device)


def jpeg_roundtrip_batch(images_u8, quality: int = 90, out=None, scratch=None):
    """``jpeg_roundtrip`` for a whole batch on the GPU: a contiguous [n,H,W,3] uint8 device tensor through a quality-q
    baseline 4:2:0 JPEG encode + decode, every frame bit-identical to ``jpeg_roundtrip(frame, quality)`` (csrc/jpeg_codec.hip).

    Runs on the current stream, with no synchronisation and no host copy.  Returns a new tensor, or ``out`` (a contiguous
    uint8 tensor of the same shape on the same device).  ``out`` may be ``images_u8`` itself: the kernels read the whole
    input before they write any output.  ``scratch`` (``jpeg_roundtrip_scratch``) is the decoded-plane buffer; without it one is
    taken from PyTorch's caching allocator per call.  Raises ValueError for a wrong dtype, rank, channel count or device, a non-contiguous
    tensor, a quality outside 1..100, or an ``out`` / ``scratch`` that does not fit."""
    import torch

    from .. import _lib
    from .ops import _stream

    x = images_u8
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError("jpeg_roundtrip_batch expects a [n,H,W,3] uint8 tensor")
    if x.device.type != "cuda":
        raise ValueError("jpeg_roundtrip_batch expects a tensor on a GPU")
    if not x.is_contiguous():
        raise ValueError("jpeg_roundtrip_batch expects a contiguous tensor")
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be an integer in 1..100, got {quality!r}")
    n, h, w, _ = x.shape
    if n == 0 or h == 0 or w == 0:
        raise ValueError(f"jpeg_roundtrip_batch expects a non-empty batch, got shape {tuple(x.shape)}")
    if h > 65500 or w > 65500:
        raise ValueError("JPEG frames are at most 65500 pixels on a side")
    if out is None:
        out = torch.empty_like(x)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != x.shape or out.device != x.device
          or not out.is_contiguous()):
        raise ValueError("out must be a contiguous uint8 tensor of the input's shape on the input's device")
    need = int(_lib.lib().vlfm_jpeg_scratch_bytes(n, h, w))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=x.device)   # (the caching allocator: no device allocation)
    elif (not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.uint8 or scratch.device != x.device
          or not scratch.is_contiguous() or scratch.numel() < need or scratch.data_ptr() % 16):
        raise ValueError(f"scratch must be a contiguous, 16-byte aligned uint8 device tensor of at least {need} bytes")
    else:
        s0, s1 = scratch.data_ptr(), scratch.data_ptr() + scratch.numel()
        for t in (x, out):
            if s0 < t.data_ptr() + t.numel() and t.data_ptr() < s1:
                raise ValueError("scratch must not overlap the input or the output")
    tables = jpeg_quant_tables(int(quality))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vlfm_jpeg_roundtrip_batched(x.data_ptr(), out.data_ptr(), n, h, w, tables.ctypes.data,
                                                          scratch.data_ptr(), scratch.numel(), _stream()),
                   "jpeg_roundtrip_batched")
    return out


JPEG_HEADER_BYTES = 623


def jpeg_header(quality: int, height: int, width: int) -> bytes:
    """The 623 bytes in front of the scan of every quality-q height x width file ``jpeg_encode_batch`` writes."""
    from .. import _lib

    import ctypes

    buf, n = np.zeros(JPEG_HEADER_BYTES, np.uint8), ctypes.c_size_t(0)
    _lib.check(_lib.lib().vlfm_jpeg_header_host(int(quality), int(height), int(width), buf.ctypes.data, buf.size,
                                                ctypes.byref(n)), "jpeg_header_host")
    return buf[:n.value].tobytes()


def jpeg_encode_bound(height: int, width: int) -> int:
    """A per-frame capacity that no height x width frame exceeds, whatever its content (0: not a size the encoder takes)."""
    from .. import _lib

    return int(_lib.lib().vlfm_jpeg_encode_bound(int(height), int(width)))


def jpeg_encode_scratch(n: int, height: int, width: int, device) -> "torch.Tensor":
    """A device buffer that ``jpeg_encode_batch(..., scratch=)`` accepts for n frames of height x width."""
    import torch

    from .. import _lib

    return torch.empty(int(_lib.lib().vlfm_jpeg_encode_scratch_bytes(n, height, width)), dtype=torch.uint8, device=device)


def jpeg_encode_batch(images_u8, quality: int = 90, channel_order: str = "bgr", capacity=None, out=None, lengths=None,
                      scratch=None):
    """Baseline 4:2:0 JPEG files of a whole batch on the GPU: a contiguous [n,H,W,3] uint8 device tensor to
    ``(out [n, capacity] uint8, lengths [n] int32)``, both on the device.  ``out[i, :lengths[i]]`` is, byte for byte, the
    file Pillow's ``save(format="JPEG", quality=q, subsampling="4:2:0")`` writes for frame i (csrc/jpeg_entropy.hip).

    ``channel_order="bgr"`` reads slot 2 of a pixel as R: what ``cv2.imencode`` does with the RGB frame the reference hands
    it (server_wrapper.py:57-61) and the convention of ``jpeg_roundtrip_batch``; ``"rgb"`` reads slot 0 as R
    (``Image.fromarray(rgb).save``).  ``capacity`` is the bytes per frame slot, by default ``jpeg_encode_bound(H, W)``, which
    no frame exceeds.  With a smaller one, a frame that does not fit is cut at ``capacity`` and its ``lengths[i]`` (the full
    length) says so; the other frames are complete.  Bytes of a slot behind the file's end are not written.

    Runs on the current stream, with no synchronisation and no host copy.  ``out`` (contiguous uint8 [n, capacity]),
    ``lengths`` (contiguous int32 [n]) and ``scratch`` (``jpeg_encode_scratch``) may be passed in; otherwise they come from
    PyTorch's caching allocator.  Raises ValueError for a wrong dtype, rank, channel count or device, a non-contiguous
    tensor, a quality outside 1..100, an unknown channel order, a capacity below 1, a frame the encoder does not take
    (larger than 65500 on a side, or than about 10 000 x 10 000 pixels), or an ``out`` / ``lengths`` / ``scratch`` that does
    not fit."""
    import torch

    from .. import _lib
    from .ops import _stream

    x = images_u8
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError("jpeg_encode_batch expects a [n,H,W,3] uint8 tensor")
    if x.device.type != "cuda":
        raise ValueError("jpeg_encode_batch expects a tensor on a GPU")
    if not x.is_contiguous():
        raise ValueError("jpeg_encode_batch expects a contiguous tensor")
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be an integer in 1..100, got {quality!r}")
    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    n, h, w, _ = x.shape
    if n == 0 or h == 0 or w == 0:
        raise ValueError(f"jpeg_encode_batch expects a non-empty batch, got shape {tuple(x.shape)}")
    if h > JPEG_MAX_DIMENSION or w > JPEG_MAX_DIMENSION:
        raise ValueError(f"JPEG frames are at most {JPEG_MAX_DIMENSION} pixels on a side")
    bound = jpeg_encode_bound(h, w)
    if bound == 0:
        raise ValueError(f"a {h} x {w} frame is too large for the encoder's 32-bit bit offsets")
    if capacity is None:
        capacity = bound if out is None else (out.shape[1] if isinstance(out, torch.Tensor) and out.dim() == 2 else bound)
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or int(capacity) < 1:
        raise ValueError(f"capacity must be a positive integer, got {capacity!r}")
    capacity = int(capacity)
    out = _buffer("out", out, torch.uint8, (n, capacity), x.device, "the input's device")
    lengths = _buffer("lengths", lengths, torch.int32, (n,), x.device, "the input's device")
    scratch = _scratch(scratch, int(_lib.lib().vlfm_jpeg_encode_scratch_bytes(n, h, w)), x.device)
    _no_overlap([("the input", x), ("out", out), ("lengths", lengths), ("scratch", scratch)])
    tables = jpeg_quant_tables(int(quality))
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().vlfm_jpeg_encode_batched(x.data_ptr(), n, h, w, int(channel_order == "rgb"),
                                                       tables.ctypes.data, out.data_ptr(), capacity, lengths.data_ptr(),
                                                       scratch.data_ptr(), scratch.numel(), _stream()),
                   "jpeg_encode_batched")
    return out, lengths


def jpeg_encode_batch_bytes(images_u8, quality: int = 90, channel_order: str = "bgr", capacity=None, out=None,
                            lengths=None, scratch=None):
    """``jpeg_encode_batch`` brought to the host as one ``bytes`` per frame.  One synchronisation: the lengths come first,
    then only the used prefix of every slot is copied.  Raises ValueError naming the frames that did not fit ``capacity``."""
    import torch

    dev_out, dev_len = jpeg_encode_batch(images_u8, quality, channel_order, capacity, out, lengths, scratch)
    lens = dev_len.cpu().numpy().astype(np.int64)           # (waits for the encoder)
    cap = dev_out.shape[1]
    over = [i for i in range(lens.size) if lens[i] > cap]
    if over:
        raise ValueError(f"frames {over} did not fit the capacity of {cap} bytes (they take "
                         f"{[int(lens[i]) for i in over]})")
    # one gather of the used prefixes, one copy
    starts = np.concatenate([[0], np.cumsum(lens)])
    idx = torch.from_numpy(np.concatenate([np.arange(l, dtype=np.int64) + i * cap for i, l in enumerate(lens)]))
    flat = dev_out.view(-1)[idx.to(dev_out.device)].cpu().numpy().tobytes()
    return [flat[starts[i]:starts[i + 1]] for i in range(lens.size)]


def image_to_str_batch(images_u8, quality: int = 90):
    """``image_to_str(frame, quality)`` of server_wrapper.py:57-61 for every frame of a [n,H,W,3] uint8 device tensor: the
    base64 text of ``cv2.imencode(".jpg", frame, [IMWRITE_JPEG_QUALITY, quality])``, which reads the frame as BGR."""
    import base64

    return [base64.b64encode(b).decode() for b in jpeg_encode_batch_bytes(images_u8, quality, "bgr")]


# ---------------------------------------------------------------------------------------------------------------- decoder
JPEG_FRAME_DTYPE = np.dtype([("height", "<i4"), ("width", "<i4"), ("restart_interval", "<i4"), ("scan_offset", "<i4"),
                             ("table_set", "<i4"), ("reserved", "<i4", (3,))])
JPEG_HUFF_DTYPE = np.dtype([("limit", "<u4", (16,)), ("delta", "<i4", (16,)), ("vals", "u1", (256,))])
JPEG_TABLE_SET_DTYPE = np.dtype([("quant", "<u2", (3, 64)), ("dc", JPEG_HUFF_DTYPE, (3,)), ("ac", JPEG_HUFF_DTYPE, (3,))])
assert JPEG_FRAME_DTYPE.itemsize == 32 and JPEG_TABLE_SET_DTYPE.itemsize == 2688
JPEG_STATUS = {1: "the file does not start with the given header", 2: "the file ends before its scan starts",
               3: "no EOI behind the scan", 4: "restart markers out of order or miscounted", 5: "invalid Huffman code",
               6: "coefficient size out of range", 7: "zigzag index past 63", 8: "a segment ran out of bits"}


def _jpeg_parse_raw(data, what: str):
    import ctypes

    from .. import _lib

    buf = np.frombuffer(data, np.uint8)
    frame, tset = np.zeros(1, JPEG_FRAME_DTYPE), np.zeros(1, JPEG_TABLE_SET_DTYPE)
    keep = np.ascontiguousarray(buf) if buf.size else np.zeros(1, np.uint8)
    rc = _lib.lib().vlfm_jpeg_parse_host(keep.ctypes.data, ctypes.c_size_t(buf.size), frame.ctypes.data, tset.ctypes.data)
    if rc > 0:
        raise ValueError(f"{what}: {_lib.lib().vlfm_jpeg_parse_reason(rc).decode()}")
    _lib.check(rc, "jpeg_parse_host")
    return frame, tset


def jpeg_parse(file) -> dict:
    """What stands in front of the scan of a baseline 4:2:0 JPEG file (bytes-like): ``height``, ``width``,
    ``restart_interval`` (0: none), ``scan_offset`` (the scan's first byte), ``quant`` ([3,64] uint16, natural order, per
    component) and ``dc`` / ``ac`` (per component the Huffman table in the form the kernel reads: ``limit``, ``delta``,
    ``vals``).  Raises ValueError with the reason for a file ``jpeg_decode_batch`` does not take."""
    frame, tset = _jpeg_parse_raw(file, "jpeg_parse")
    out = {k: int(frame[k][0]) for k in ("height", "width", "restart_interval", "scan_offset")}
    out["quant"] = tset["quant"][0].copy()
    for kind in ("dc", "ac"):
        out[kind] = [{k: tset[kind][0][c][k].copy() for k in ("limit", "delta", "vals")} for c in range(3)]
    return out


def jpeg_decode_scratch(n: int, height: int, width: int, max_file_bytes: int, device) -> "torch.Tensor":
    """A device buffer that ``jpeg_decode_batch(..., scratch=)`` accepts for n files of height x width, none longer than
    ``max_file_bytes`` (device form: the capacity of a slot).  After a call its first n * MCUs * 768 bytes hold the scan's
    coefficients in the encoder's layout (int16 [n, 6 * MCUs, 64], zigzag order, absolute DC values)."""
    import torch

    from .. import _lib

    return torch.empty(int(_lib.lib().vlfm_jpeg_decode_scratch_bytes(n, height, width, max_file_bytes)), dtype=torch.uint8,
                       device=device)


def jpeg_decode_batch(files, lengths=None, header=None, channel_order: str = "bgr", out=None, status=None, scratch=None,
                      device=None):
    """Baseline 4:2:0 JPEG files of one size to ``(out [n,H,W,3] uint8, status [n] int32)``, both on the device; every frame
    whose status is 0 is bit-equal to ``PIL.Image.open(file).convert("RGB")`` (csrc/jpeg_decode.hip), in slot order B, G, R for
    ``channel_order="bgr"`` (what ``cv2.imdecode`` returns, the convention of ``jpeg_roundtrip_batch``) or R, G, B for ``"rgb"``.

    Host form: ``files`` is a sequence of bytes-like objects; they are parsed on the host (ValueError naming the frame and the
    reason for a file the decoder does not take, or whose size differs from the first one's) and uploaded in one copy to
    ``device`` (default: the current one).  Every file may have its own tables and restart interval.

    Device form: ``files`` is the ``[n, capacity] uint8`` device tensor and ``lengths`` the ``int32 [n]`` device tensor that
    ``jpeg_encode_batch`` returns, and ``header`` the bytes every file starts with (``jpeg_header(q, H, W)`` for this
    package's files).  The device compares them; no byte of the files crosses to the host.

    A non-zero status (``JPEG_STATUS``) marks a frame whose stream is damaged: its pixels are unspecified, the other frames
    are complete.  Runs on the current stream, with no synchronisation.  ``out``, ``status`` and ``scratch``
    (``jpeg_decode_scratch``) may be passed in.  Raises ValueError for a wrong dtype, shape, device or contiguity, buffers that
    overlap, an unknown channel order or an empty batch."""
    import torch

    from .. import _lib
    from .ops import _stream

    if channel_order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', got {channel_order!r}")
    device_form = isinstance(files, torch.Tensor)
    if device_form:
        x = files
        if x.dtype != torch.uint8 or x.dim() != 2 or x.device.type != "cuda" or not x.is_contiguous():
            raise ValueError("the device form expects a contiguous [n, capacity] uint8 tensor on a GPU")
        n, cap = x.shape
        if n == 0 or cap == 0:
            raise ValueError("jpeg_decode_batch expects a non-empty batch")
        if (not isinstance(lengths, torch.Tensor) or lengths.dtype != torch.int32 or tuple(lengths.shape) != (n,)
                or lengths.device != x.device or not lengths.is_contiguous()):
            raise ValueError(f"lengths must be a contiguous int32 tensor of shape ({n},) on the files' device")
        if not isinstance(header, (bytes, bytearray, memoryview)) or len(header) == 0:
            raise ValueError("the device form needs header= (bytes): what every file starts with")
        if len(header) > cap:
            raise ValueError("the header is longer than a file slot")
        frame, tset = _jpeg_parse_raw(header, "header")
        if int(frame["scan_offset"][0]) != len(header):
            raise ValueError("header must end with the SOS segment")
        frames, sets, dev, max_file = np.repeat(frame, n), tset, x.device, cap
        blob_parts = [frames.tobytes(), sets.tobytes(), bytes(header)]
    else:
        if lengths is not None or header is not None:
            raise ValueError("lengths= and header= belong to the device form")
        try:
            views = [np.frombuffer(f, np.uint8) for f in files]
        except TypeError as exc:
            raise ValueError(f"files must be bytes-like objects: {exc}") from None
        n = len(views)
        if n == 0:
            raise ValueError("jpeg_decode_batch expects a non-empty batch")
        frames, set_index, set_list = np.zeros(n, JPEG_FRAME_DTYPE), {}, []
        for i, v in enumerate(views):
            fr, ts = _jpeg_parse_raw(v, f"frame {i}")
            key = ts.tobytes()
            if key not in set_index:
                set_index[key] = len(set_list)
                set_list.append(key)
            frames[i] = fr[0]
            frames[i]["table_set"] = set_index[key]
            if (fr["height"][0], fr["width"][0]) != (frames[0]["height"], frames[0]["width"]):
                raise ValueError(f"frame {i} is {fr['height'][0]} x {fr['width'][0]}, the batch is "
                                 f"{frames[0]['height']} x {frames[0]['width']}")
        sets = np.frombuffer(b"".join(set_list), JPEG_TABLE_SET_DTYPE)
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise ValueError("jpeg_decode_batch decodes on a GPU")
        max_file = max(v.size for v in views)
        offs = np.zeros(n, np.int64)
        pos = 0
        for i, v in enumerate(views):
            offs[i] = pos
            pos += (v.size + 15) & ~15
        lens = np.array([v.size for v in views], np.int32)
        packed = np.zeros(pos, np.uint8)
        for o, v in zip(offs, views):
            packed[o:o + v.size] = v
        blob_parts = [frames.tobytes(), sets.tobytes(), offs.tobytes(), lens.tobytes(), packed.tobytes()]
    h, w = int(frames[0]["height"]), int(frames[0]["width"])
    mcus = -(-h // 16) * -(-w // 16)
    ri = frames["restart_interval"].astype(np.int64)
    max_seg = int(np.max(np.where(ri > 0, -(-mcus // np.maximum(ri, 1)), 1)))

    out = _buffer("out", out, torch.uint8, (n, h, w, 3), dev, "the decoding device")
    status = _buffer("status", status, torch.int32, (n,), dev, "the decoding device")
    need = int(_lib.lib().vlfm_jpeg_decode_scratch_bytes(n, h, w, max_file))
    if need == 0:
        raise ValueError(f"{n} files of {h} x {w} and up to {max_file} bytes are not a batch the decoder takes")
    scratch = _scratch(scratch, need, dev)
    _no_overlap(([("the files", files), ("lengths", lengths)] if device_form else [])
                + [("out", out), ("status", status), ("scratch", scratch)])

    # one upload: frame records, table sets and (host form) offsets, lengths and the files, each part 16-byte aligned
    starts, total = [], 0
    for part in blob_parts:
        starts.append(total)
        total += (len(part) + 15) & ~15
    host = np.zeros(total, np.uint8)
    for s, part in zip(starts, blob_parts):
        host[s:s + len(part)] = np.frombuffer(part, np.uint8)
    blob = torch.from_numpy(host).to(dev)
    base = blob.data_ptr()
    assert base % 16 == 0
    with torch.cuda.device(dev):
        if device_form:
            args = (files.data_ptr(), files.numel(), None, cap, lengths.data_ptr(), n, h, w, base, base + starts[1],
                    1, base + starts[2], len(header))
        else:
            args = (base + starts[4], total - starts[4], base + starts[2], 0, base + starts[3], n, h, w, base,
                    base + starts[1], len(sets), None, 0)
        _lib.check(_lib.lib().vlfm_jpeg_decode_batched(*args, max_seg, max_file, int(channel_order == "rgb"), out.data_ptr(),
                                                       status.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream()),
                   "jpeg_decode_batched")
    return out, status


def jpeg_decode_batch_checked(files, lengths=None, header=None, channel_order: str = "bgr", out=None, status=None,
                              scratch=None, device=None):
    """``jpeg_decode_batch`` with one synchronisation: returns ``out`` alone and raises ValueError naming the frames whose
    stream is damaged, and how."""
    out, status = jpeg_decode_batch(files, lengths, header, channel_order, out, status, scratch, device)
    st = status.cpu().numpy()                               # (waits for the decoder)
    bad = np.nonzero(st)[0]
    if bad.size:
        raise ValueError("damaged JPEG streams: " + ", ".join(
            f"frame {int(i)} ({JPEG_STATUS.get(int(st[i]), int(st[i]))})" for i in bad))
    return out


def str_to_image_batch(strings, device=None):
    """``str_to_image`` of server_wrapper.py:64-68 for a batch: base64 texts of JPEG files of one size to a ``[n,H,W,3]`` uint8
    device tensor, in the slot order ``cv2.imdecode`` gives (B, G, R).  One synchronisation (``jpeg_decode_batch_checked``)."""
    import base64

    return jpeg_decode_batch_checked([base64.b64decode(s) for s in strings], channel_order="bgr", device=device)
