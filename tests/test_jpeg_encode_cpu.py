"""The JPEG encoder's host side, without a GPU: the NumPy restatement tests/jpeg_huff_ref.py (frame header, dummy blocks,
Huffman coding, stuffing) equals the installed Pillow's file byte for byte; the library's header, bound and scratch-size
functions; the Motion-JPEG writer.  Every comparison is equality of bytes."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_huff_ref  # noqa: E402
import jpeg_ref  # noqa: E402

SMALL = [hw for hw in jpeg_ref.SIZES if hw[0] * hw[1] <= 33 * 47] + [(33, 40)]
LARGE = [(480, 640), (1000, 1000)]
QUALITIES = [1, 50, 75, 90, 100]


def _first_difference(a: bytes, b: bytes):
    n = min(len(a), len(b))
    d = next((i for i in range(n) if a[i] != b[i]), n)
    return len(a), len(b), d


@pytest.mark.parametrize("hw", SMALL + LARGE, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("kind", ["noise", "gradient"])
def test_restatement_equals_pillow_q90(hw, kind):
    img = jpeg_ref.frame(kind, *hw, seed=hw[0] + hw[1])
    got, want = jpeg_huff_ref.encode(img, 90), jpeg_huff_ref.pillow_bytes(img, 90)
    assert got == want, _first_difference(got, want)


@pytest.mark.parametrize("hw", SMALL, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_restatement_equals_pillow_over_classes_and_qualities(hw):
    for i, kind in enumerate(jpeg_ref.CONTENT):
        img = jpeg_ref.frame(kind, *hw, seed=i)
        for q in QUALITIES:
            for rgb in (False, True):
                got, want = jpeg_huff_ref.encode(img, q, rgb), jpeg_huff_ref.pillow_bytes(img, q, rgb)
                assert got == want, (kind, q, rgb) + _first_difference(got, want)


def test_dummy_blocks_are_not_the_dct_of_replicated_pixels():
    """17 x 9: one real block column and three real block rows in a 2 x 1 MCU grid.  Coding the edge-replicated 32 x 16
    frame instead (the plausible simpler rule) gives another file."""
    img = jpeg_ref.frame("noise", 17, 9, seed=5)
    big = np.pad(img, ((0, 15), (0, 7), (0, 0)), mode="edge")
    simple = jpeg_huff_ref.pack(*jpeg_huff_ref.entropy_tokens(jpeg_huff_ref.scan_blocks(big, 90)))
    exact = jpeg_huff_ref.pack(*jpeg_huff_ref.entropy_tokens(jpeg_huff_ref.scan_blocks(img, 90)))
    assert simple != exact
    assert jpeg_huff_ref.header(90, 17, 9) + exact + b"\xff\xd9" == jpeg_huff_ref.pillow_bytes(img, 90)


def _lib():
    from vlfm_amd import _lib

    return _lib


@pytest.mark.parametrize("q,h,w", [(90, 480, 640), (1, 1, 1), (50, 1000, 1000), (100, 479, 641), (75, 720, 1280)])
def test_library_header_equals_pillow(q, h, w):
    L = _lib()
    buf, n = np.zeros(1024, np.uint8), ctypes.c_size_t(0)
    assert L.lib().vlfm_jpeg_header_host(q, h, w, buf.ctypes.data, buf.size, ctypes.byref(n)) == 0
    assert n.value == jpeg_huff_ref.HEADER_BYTES == 623
    want = jpeg_huff_ref.pillow_bytes(jpeg_ref.frame("gradient", h, w), q)
    assert buf[:623].tobytes() == want[:623]
    assert buf[:623].tobytes() == jpeg_huff_ref.header(q, h, w)
    assert not buf[623:].any()
    # too small a buffer: the length is still reported, nothing is written
    small = np.zeros(622, np.uint8)
    assert L.lib().vlfm_jpeg_header_host(q, h, w, small.ctypes.data, small.size, ctypes.byref(n)) == L.VLFM_ERR_CAPACITY
    assert n.value == 623 and not small.any()
    assert L.lib().vlfm_jpeg_header_host(0, h, w, buf.ctypes.data, buf.size, ctypes.byref(n)) == L.VLFM_ERR_INVALID
    assert L.lib().vlfm_jpeg_header_host(q, 0, w, buf.ctypes.data, buf.size, ctypes.byref(n)) == L.VLFM_ERR_INVALID
    assert L.lib().vlfm_jpeg_header_host(q, h, 65501, buf.ctypes.data, buf.size, ctypes.byref(n)) == L.VLFM_ERR_INVALID


def test_transport_header_and_abi_version():
    from vlfm_amd.vlm.transport import jpeg_header

    assert _lib().lib().vlfm_abi_version() >= 12
    assert jpeg_header(90, 480, 640) == jpeg_huff_ref.header(90, 480, 640)


@pytest.mark.parametrize("hw", SMALL + LARGE + [(720, 1280), (479, 641)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_bound_is_at_least_pillows_noise_at_q100(hw):
    L = _lib().lib()
    bound = L.vlfm_jpeg_encode_bound(*hw)
    blocks = 6 * -(-hw[0] // 16) * -(-hw[1] // 16)
    assert bound == 623 + 2 * -(-blocks * 1660 // 8) + 2        # the derivation of include/vlfm_amd.h
    assert bound >= len(jpeg_huff_ref.pillow_bytes(jpeg_ref.frame("noise", *hw, seed=1), 100))
    stream = (bound - 625) // 2                                  # coefficients + the unstuffed stream at the bound, at least
    assert L.vlfm_jpeg_encode_scratch_bytes(1, *hw) >= 128 * blocks + stream
    assert L.vlfm_jpeg_encode_scratch_bytes(3, *hw) >= 3 * (128 * blocks + stream)


def test_worst_block_reaches_no_more_than_the_bound_per_block():
    """The longest codes of the standard tables are what the bound assumes: 16-bit AC codes, DC codes of at most 11."""
    assert max(jpeg_huff_ref.AC_TABLES[0][1].max(), jpeg_huff_ref.AC_TABLES[1][1].max()) == 16
    assert max(jpeg_huff_ref.DC_TABLES[0][1].max(), jpeg_huff_ref.DC_TABLES[1][1].max()) == 11


def test_bound_and_scratch_are_zero_for_invalid_sizes():
    L = _lib().lib()
    for h, w in [(0, 640), (480, 0), (-1, 640), (480, -5), (65501, 640), (480, 65501), (65500, 65500)]:
        assert L.vlfm_jpeg_encode_bound(h, w) == 0, (h, w)
        assert L.vlfm_jpeg_encode_scratch_bytes(1, h, w) == 0, (h, w)
    assert L.vlfm_jpeg_encode_scratch_bytes(0, 480, 640) == 0
    assert L.vlfm_jpeg_encode_scratch_bytes(-3, 480, 640) == 0
    assert L.vlfm_jpeg_encode_bound(1, 1) > 0 and L.vlfm_jpeg_encode_bound(8000, 8000) > 0


# (n, H, W): roundtrip scratch, encode scratch, encode bound, decode scratch at max_file_bytes 1000 and 65536.  Recorded from
# the library of the commit before the three JPEG translation units were folded onto csrc/jpeg_common.h (795fde3), built and
# queried on the CPU before the first edit: the fold must not move a size.
SIZES_BEFORE_THE_FOLD = {
    (1, 1, 1): (384, 2112, 3115, 2240, 67008),
    (1, 16, 16): (384, 2112, 3115, 2240, 67008),
    (1, 17, 9): (768, 4128, 5605, 3392, 68160),
    (1, 33, 47): (3456, 18400, 23035, 11488, 76256),
    (1, 480, 640): (460800, 2445920, 2988625, 1388288, 1453056),
    (1, 479, 641): (472320, 2507056, 3063325, 1422960, 1487728),
    (1, 1000, 1000): (1524096, 8089744, 9883435, 4589248, 4654016),
    (3, 1, 1): (1152, 6256, 3115, 6704, 201008),
    (3, 16, 16): (1152, 6256, 3115, 6704, 201008),
    (3, 17, 9): (2304, 12320, 5605, 10176, 204480),
    (3, 33, 47): (10368, 55152, 23035, 34448, 228752),
    (3, 480, 640): (1382400, 7337696, 2988625, 4164832, 4359136),
    (3, 479, 641): (1416960, 7521120, 3063325, 4268880, 4463184),
    (3, 1000, 1000): (4572288, 24269184, 9883435, 13767728, 13962032),
}


def test_scratch_sizes_and_bound_do_not_move():
    L = _lib().lib()
    for (n, h, w), want in SIZES_BEFORE_THE_FOLD.items():
        got = (L.vlfm_jpeg_scratch_bytes(n, h, w), L.vlfm_jpeg_encode_scratch_bytes(n, h, w), L.vlfm_jpeg_encode_bound(h, w),
               L.vlfm_jpeg_decode_scratch_bytes(n, h, w, 1000), L.vlfm_jpeg_decode_scratch_bytes(n, h, w, 65536))
        assert got == want, (n, h, w)


def test_mjpeg_writer_output_splits_back_into_its_files(tmp_path):
    from vlfm_amd.utils.mjpeg import MjpegWriter, split_mjpeg

    files = [jpeg_huff_ref.pillow_bytes(jpeg_ref.frame(k, 33, 40, seed=i), q)
             for i, (k, q) in enumerate([("noise", 100), ("gradient", 90), ("constant", 1), ("checker1", 75)])]
    path = tmp_path / "a.mjpeg"
    with MjpegWriter(path) as w:
        for f in files:
            w.append(f)
        assert w.frames == 4
        with pytest.raises(ValueError):
            w.append(files[0][:-2])
    with pytest.raises(ValueError):
        w.append(files[0])                                   # closed
    w.close()                                                # closing twice is fine
    data = path.read_bytes()
    assert data == b"".join(files)
    assert split_mjpeg(data) == files
    from PIL import Image
    import io

    assert all(Image.open(io.BytesIO(f)).size == (40, 33) for f in split_mjpeg(data))
