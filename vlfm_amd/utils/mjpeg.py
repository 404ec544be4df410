"""Raw Motion-JPEG: JPEG files written back to back.  Every file starts with SOI (FF D8) and ends with EOI (FF D9), and
inside a baseline file neither pair occurs anywhere else (entropy-coded FF bytes are followed by 00), so the stream needs no
container: video players read it as it is (``ffplay -f mjpeg``), and it splits back into its files at the markers."""
from __future__ import annotations

import os
from typing import List

SOI, EOI = b"\xff\xd8", b"\xff\xd9"


class MjpegWriter:
    """``with MjpegWriter(path) as w: w.append(jpeg_bytes)`` -- one frame per call, e.g. the files of
    ``BatchedEpisodes.render_jpeg()`` or ``transport.jpeg_encode_batch_bytes``."""

    def __init__(self, path) -> None:
        self.path = os.fspath(path)
        self.frames = 0
        self._f = open(self.path, "wb")

    def append(self, jpeg: bytes) -> None:
        if self._f is None:
            raise ValueError("append to a closed MjpegWriter")
        jpeg = bytes(jpeg)
        if not (jpeg.startswith(SOI) and jpeg.endswith(EOI)):
            raise ValueError("append expects one whole JPEG file (SOI ... EOI)")
        self._f.write(jpeg)
        self.frames += 1

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self) -> "MjpegWriter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def split_mjpeg(data: bytes) -> List[bytes]:
    """The files of a raw Motion-JPEG stream of baseline files without thumbnails (what ``MjpegWriter`` writes)."""
    out, pos = [], 0
    while pos < len(data):
        if data[pos:pos + 2] != SOI:
            raise ValueError(f"no SOI at byte {pos}")
        end = data.find(EOI, pos + 2)
        if end < 0:
            raise ValueError(f"no EOI behind byte {pos}")
        out.append(data[pos:end + 2])
        pos = end + 2
    return out


def read_mjpeg(path, device=None, batch: int = 64, channel_order: str = "rgb"):
    """The frames of a raw Motion-JPEG file, decoded on the GPU: a generator of ``[k,H,W,3]`` uint8 device tensors, k <=
    ``batch`` (``transport.jpeg_decode_batch_checked`` over ``split_mjpeg``).  Raises ValueError if the frames of one batch
    differ in size or a stream is damaged."""
    from ..vlm.transport import jpeg_decode_batch_checked

    if batch < 1:
        raise ValueError("batch must be at least 1")
    with open(os.fspath(path), "rb") as f:
        files = split_mjpeg(f.read())
    for i in range(0, len(files), batch):
        yield jpeg_decode_batch_checked(files[i:i + batch], channel_order=channel_order, device=device)
