"""No GPU: the NumPy JPEG decoder (jpeg_dec_ref.py) against Pillow, the model of the kernel's in-wave Huffman scheme against
the sequential decoder (good and damaged streams, every index asserted in range), and the host parser of the C ABI."""
import inspect
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_dec_ref as dec
import jpeg_huff_ref as huff
import jpeg_ref

SIZES = [(16, 16), (8, 8), (1, 1), (17, 33), (33, 47), (48, 80), (2, 3)]
QUALITIES = [30, 90, 100]
WRITERS = {"default": {}, "optimize": {"optimize": True}, "restart_blocks_1": {"restart_marker_blocks": 1},
           "restart_rows_1": {"restart_marker_rows": 1}, "optimize_restart_3": {"optimize": True, "restart_marker_blocks": 3}}


def _pillow_has_restart() -> bool:
    try:
        b = io.BytesIO()
        Image.new("RGB", (32, 32)).save(b, format="JPEG", restart_marker_blocks=1)
        return b"\xff\xdd" in b.getvalue()
    except Exception:  # noqa: BLE001
        return False


HAS_RESTART = _pillow_has_restart()


def pillow_file(x, q, **kw):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(x[..., ::-1])).save(b, format="JPEG", quality=q, subsampling="4:2:0", **kw)
    return b.getvalue()


@pytest.mark.parametrize("writer", list(WRITERS))
def test_ref_and_wave_model_equal_pillow(writer):
    """630 files in all: 7 sizes x 6 content classes x 3 qualities x 5 writers.  The sequential decoder equals Pillow in pixels;
    the in-wave model equals the sequential decoder in coefficients with status 0."""
    kw = WRITERS[writer]
    if any(k.startswith("restart") for k in kw) and not HAS_RESTART:
        pytest.skip("the installed Pillow has no restart_marker_* keywords")
    for h, w in SIZES:
        for kind in jpeg_ref.CONTENT:
            for q in QUALITIES:
                data = pillow_file(jpeg_ref.frame(kind, h, w, 1), q, **kw)
                coef = dec.decode_coefficients(data)
                info = dec.parse(data)
                assert np.array_equal(dec.pixels(coef, info), dec.pillow_pixels(data)), (h, w, kind, q)
                assert np.array_equal(dec.pixels(coef, info, True), dec.pillow_pixels(data, True)), (h, w, kind, q)
                wave, status = dec.decode_coefficients_wave(data, info)
                assert status == 0 and np.array_equal(wave, coef), (h, w, kind, q, status)


@pytest.mark.parametrize("ri", [1, 2, 3, 5, 9, 10])
def test_restart_writer(ri):
    for h, w in [(16, 16), (17, 33), (33, 47), (48, 80), (2, 3)]:
        for kind in ("noise", "gradient", "checker1", "hot_pixel"):
            for q in QUALITIES:
                x = jpeg_ref.frame(kind, h, w, 2)
                data = dec.restart_file(x, q, ri)
                if HAS_RESTART:
                    assert data == pillow_file(x, q, restart_marker_blocks=ri), (h, w, kind, q)
                assert np.array_equal(dec.decode(data), dec.pillow_pixels(data)), (h, w, kind, q)
                wave, status = dec.decode_coefficients_wave(data)
                assert status == 0 and np.array_equal(wave, huff.scan_blocks(x, q))


@pytest.mark.skipif(not HAS_RESTART, reason="the installed Pillow has no restart_marker_* keywords")
def test_restart_rows_is_one_mcu_row():
    x = jpeg_ref.frame("noise", 33, 47, 4)
    assert dec.restart_file(x, 90, 3) == pillow_file(x, 90, restart_marker_rows=1)


@pytest.mark.parametrize("hw", [(16, 16), (9, 17), (33, 47), (1, 15)])
def test_own_files_come_back_as_scan_blocks(hw):
    for kind in jpeg_ref.CONTENT:
        x = jpeg_ref.frame(kind, *hw, 5)
        data = huff.encode(x, 90)
        want = huff.scan_blocks(x, 90)                       # (dummy edge blocks included)
        assert np.array_equal(dec.decode_coefficients(data), want)
        wave, status = dec.decode_coefficients_wave(data)
        assert status == 0 and np.array_equal(wave, want)


@pytest.mark.parametrize("kind", ["full", "last", "sparse", "zeros"])
@pytest.mark.parametrize("ri", [0, 1, 4])
def test_crafted_coefficients_come_back(kind, ri):
    zz = dec.crafted(kind)
    data = dec.coefficient_file(zz, 100 if kind == "full" else 90, 32, 48, ri)
    assert np.array_equal(dec.decode_coefficients(data), zz)
    trace = []
    wave, status = dec.decode_coefficients_wave(data, trace=trace)
    assert status == 0 and np.array_equal(wave, zz)
    if kind == "full":
        bits = 8 * (len(data) - 623) / zz.shape[0]
        assert bits > 1500
    if kind == "zeros" and ri == 0:
        assert max(t["blocks_ended"] for t in trace) >= 12   # a dozen blocks end inside one window
    # tokens straddle window boundaries: some window starts at a bit position that is no multiple of 64
    assert kind == "zeros" or any(t["pos"] % 64 for t in trace)


@pytest.mark.parametrize("name,data", dec.damaged_streams(), ids=[n for n, _ in dec.damaged_streams()])
def test_wave_model_on_damaged_streams(name, data):
    """The model never forms an index out of range (it asserts each one) and reports a status instead."""
    coef, status = dec.decode_coefficients_wave(data)
    assert coef.shape == (6 * 15, 64)
    if not name.startswith("flip"):                          # (a flipped amplitude bit is a valid stream of another image)
        assert status != 0, name


def test_parse_host_equals_ref_parser():
    from vlfm_amd.vlm import transport

    x = jpeg_ref.frame("noise", 33, 47, 3)
    files = [pillow_file(x, 90), pillow_file(x, 30, optimize=True), dec.restart_file(x, 100, 3), huff.encode(x, 90),
             dec.coefficient_file(dec.crafted("full"), 100, 32, 48)]
    files.append(dec.insert_comment(files[0], 37))
    files.append(files[1][:2] + b"\xff\xff\xff" + files[1][2:])           # fill bytes in front of a marker
    for data in files:
        got, want = transport.jpeg_parse(data), dec.parse(data)
        for k in ("height", "width", "restart_interval", "scan_offset"):
            assert got[k] == want[k], k
        assert np.array_equal(got["quant"], want["quant"])
        for kind in ("dc", "ac"):
            for c in range(3):
                for k in ("limit", "delta", "vals"):
                    assert np.array_equal(got[kind][c][k].astype(np.int64), want[kind][c][k]), (kind, c, k)
        assert np.array_equal(dec.decode(data), dec.pillow_pixels(data)) or data is files[4]


def _patched(data: bytes, marker: int, edit) -> bytes:
    i = data.index(bytes([0xFF, marker]))
    b = bytearray(data)
    edit(b, i + 4)
    return bytes(b)


def test_parse_host_refusals():
    from vlfm_amd.vlm import transport

    x = jpeg_ref.frame("gradient", 32, 48, 3)
    good = pillow_file(x, 90)
    rgb = Image.fromarray(x)

    def save(**kw):
        b = io.BytesIO()
        kw.setdefault("quality", 90)
        (kw.pop("image", None) or rgb).save(b, format="JPEG", **kw)
        return b.getvalue()

    dqt = good.index(b"\xff\xdb")
    dht = good.index(b"\xff\xc4")
    dht_len = int.from_bytes(good[dht + 2:dht + 4], "big")
    sos = good.index(b"\xff\xda")
    refused = {
        "progressive": (save(progressive=True), "baseline"),
        "444": (save(subsampling="4:4:4"), "sampling"),
        "grey": (save(image=rgb.convert("L")), "three components"),
        "dqt16": (good[:dqt + 4] + b"\x10" + good[dqt + 5:], "16-bit"),
        "no_dht": (good[:dht] + good[dht + 2 + dht_len:], "no segment defines"),
        "zero_height": (_patched(good, 0xC0, lambda b, i: b.__setitem__(slice(i + 1, i + 3), b"\x00\x00")), "zero"),
        "zero_width": (_patched(good, 0xC0, lambda b, i: b.__setitem__(slice(i + 3, i + 5), b"\x00\x00")), "zero"),
        "app14": (good[:sos] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + good[sos:], "Adobe"),
        "12bit": (_patched(good, 0xC0, lambda b, i: b.__setitem__(i, 12)), "8-bit"),
        "arithmetic": (good.replace(b"\xff\xc0", b"\xff\xc9", 1), "baseline"),
        "not_jpeg": (b"\x89PNG" + good[4:], "SOI"),
        "header_only": (good[:sos], "scan"),
    }
    for name, (data, word) in refused.items():
        with pytest.raises(ValueError, match=word):
            transport.jpeg_parse(data)
        with pytest.raises(ValueError):
            dec.parse(data)
    # accepted: a COM segment, fill bytes, and a prefix that ends behind SOS
    for data in (dec.insert_comment(good, 5), good[:2] + b"\xff\xff" + good[2:]):
        assert transport.jpeg_parse(data)["height"] == 32
        assert np.array_equal(dec.decode(data), dec.pillow_pixels(good))
    assert transport.jpeg_parse(good[:sos + 14])["scan_offset"] == sos + 14


def test_abi_and_signatures():
    from vlfm_amd import _lib
    from vlfm_amd.utils import mjpeg
    from vlfm_amd.vlm import transport

    L = _lib.lib()
    assert L.vlfm_abi_version() >= 14
    assert L.vlfm_jpeg_decode_chunk_bytes() >= 64
    assert L.vlfm_jpeg_decode_scratch_bytes(1, 16, 16, 1000) > 768 + 384 + 1000
    assert L.vlfm_jpeg_decode_scratch_bytes(0, 16, 16, 1000) == 0 and L.vlfm_jpeg_decode_scratch_bytes(1, 0, 16, 1000) == 0
    for fn in (transport.jpeg_decode_batch, transport.jpeg_decode_batch_checked):
        assert {"files", "lengths", "header", "channel_order", "out", "status", "scratch"} <= set(
            inspect.signature(fn).parameters)
    assert inspect.signature(mjpeg.read_mjpeg).parameters["channel_order"].default == "rgb"
    with pytest.raises(ValueError, match="channel_order"):
        transport.jpeg_decode_batch([b""], channel_order="xyz")
