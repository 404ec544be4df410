"""-m gpu: the batched JPEG decoder (csrc/jpeg_decode.hip, transport.jpeg_decode_batch) against Pillow, against the encoder's
coefficients, against jpeg_roundtrip_batch, and on damaged streams (status codes, neighbours complete, guard bytes intact)."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_dec_ref as dec
import jpeg_huff_ref as huff
import jpeg_ref

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (2, 3), (8, 8), (16, 16), (1, 15), (17, 9), (9, 17), (33, 47), (48, 80)]
GUARD = 4096


def T():
    from vlfm_amd.vlm import transport

    return transport


def pillow_file(x, q, **kw):
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(x[..., ::-1])).save(b, format="JPEG", quality=q, subsampling="4:2:0", **kw)
    return b.getvalue()


def coefficients(scratch, n, h, w):
    mcus = -(-h // 16) * -(-w // 16)
    return scratch[:n * mcus * 768].view(torch.int16).cpu().numpy().reshape(n, mcus * 6, 64).astype(np.int64)


@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_pixels_equal_pillow(gpu_device, hw):
    """Every content class x q in {30, 90, 100} x writer (Pillow default, Pillow optimize=True, restart files with Ri in {1, 3,
    MCUs per row}) of one size in one call per channel order: 90 files, many table sets and segment counts."""
    h, w = hw
    files = []
    for kind in jpeg_ref.CONTENT:
        for q in (30, 90, 100):
            x = jpeg_ref.frame(kind, h, w, 3)
            files += [pillow_file(x, q), pillow_file(x, q, optimize=True)]
            files += [dec.restart_file(x, q, ri) for ri in (1, 3, -(-w // 16))]
    for order in ("bgr", "rgb"):
        out, status = T().jpeg_decode_batch(files, channel_order=order, device=gpu_device)
        got, st = out.cpu().numpy(), status.cpu().numpy()
        assert not st.any(), st
        for i, f in enumerate(files):
            assert np.array_equal(got[i], dec.pillow_pixels(f, order == "rgb")), (i, order)


def test_coefficient_buffer(gpu_device):
    """This package's own files come back as the encoder's coefficients (dummy edge blocks included); crafted files -- every
    coefficient +-1023, a coefficient at zigzag 63, sparse, all zero; with and without restart markers -- as the given ones."""
    for h, w in [(33, 47), (9, 17), (48, 80)]:
        xs = [jpeg_ref.frame(kind, h, w, 5) for kind in jpeg_ref.CONTENT]
        files = [huff.encode(x, 90) for x in xs]
        scratch = T().jpeg_decode_scratch(len(files), h, w, max(map(len, files)), gpu_device)
        _, status = T().jpeg_decode_batch(files, scratch=scratch, device=gpu_device)
        assert not status.cpu().numpy().any()
        got = coefficients(scratch, len(files), h, w)
        for i, x in enumerate(xs):
            assert np.array_equal(got[i], huff.scan_blocks(x, 90)), (h, w, i)
    want, files = [], []
    for kind in ("full", "last", "sparse", "zeros"):
        for ri in (0, 1, 4):
            want.append(dec.crafted(kind))
            files.append(dec.coefficient_file(want[-1], 100 if kind == "full" else 90, 32, 48, ri))
    scratch = T().jpeg_decode_scratch(len(files), 32, 48, max(map(len, files)), gpu_device)
    _, status = T().jpeg_decode_batch(files, scratch=scratch, device=gpu_device)
    assert not status.cpu().numpy().any()
    assert np.array_equal(coefficients(scratch, len(files), 32, 48), np.stack(want))


@pytest.mark.parametrize("shape", [(2, 48, 80), (2, 33, 47), (3, 480, 640)], ids=["48x80", "33x47", "3x480x640"])
def test_round_trip(gpu_device, shape):
    """decode(encode_batch(x)) == jpeg_roundtrip_batch(x): through the device form (no host copy of the files) and the host form."""
    n, h, w = shape
    x = torch.from_numpy(np.stack([jpeg_ref.frame(k, h, w, 9) for k in ("noise", "gradient", "hot_pixel")[:n]])).to(gpu_device)
    want = T().jpeg_roundtrip_batch(x, 90)
    files, lengths = T().jpeg_encode_batch(x, 90)
    out, status = T().jpeg_decode_batch(files, lengths, header=T().jpeg_header(90, h, w))
    assert not status.cpu().numpy().any() and torch.equal(out, want)
    host = T().jpeg_encode_batch_bytes(x, 90)
    assert torch.equal(T().jpeg_decode_batch_checked(host, device=gpu_device), want)
    rgb = T().jpeg_decode_batch_checked(host, channel_order="rgb", device=gpu_device)
    assert torch.equal(rgb, want.flip(-1))


def test_mixed_batch_and_batch_invariance(gpu_device):
    x = [jpeg_ref.frame(k, 48, 80, 4) for k in ("noise", "gradient", "checker8")]
    files = [pillow_file(x[0], 30), pillow_file(x[1], 90, optimize=True), dec.restart_file(x[2], 100, 1)]
    infos = [T().jpeg_parse(f) for f in files]
    assert [i["restart_interval"] for i in infos] == [0, 0, 1]
    assert len({i["quant"].tobytes() for i in infos}) == 3
    want = np.stack([dec.pillow_pixels(f) for f in files])
    out, status = T().jpeg_decode_batch(files, device=gpu_device)
    assert not status.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), want)
    alone = T().jpeg_decode_batch_checked(files[2:], device=gpu_device)
    many = T().jpeg_decode_batch_checked([files[i % 3] for i in range(64)], device=gpu_device).cpu().numpy()
    assert np.array_equal(alone.cpu().numpy()[0], want[2])
    for i in range(64):
        assert np.array_equal(many[i], want[i % 3]), i


def test_chunk_boundary(gpu_device):
    """An FF 00 pair, and an RSTn marker, whose two bytes lie in different chunks of the marker scan: a COM segment of chosen
    length in front of SOS (Pillow ignores it) moves the pair onto the boundary."""
    from vlfm_amd import _lib

    chunk = int(_lib.lib().vlfm_jpeg_decode_chunk_bytes())
    x = jpeg_ref.frame("noise", 48, 80, 6)
    files = []
    for base, pair in ((pillow_file(x, 100), b"\xff\x00"), (dec.restart_file(x, 100, 1), b"\xff\xd3")):
        assert len(base) > chunk
        p = base.index(pair, max(dec.parse(base)["scan_offset"], 700))
        moved = dec.insert_comment(base, (chunk - 1 - (p + 4)) % chunk)
        q = moved.index(pair, dec.parse(moved)["scan_offset"])
        assert q % chunk == chunk - 1 and q > dec.parse(moved)["scan_offset"]      # the straddle really occurs
        files.append(moved)
    for f in files:
        assert np.array_equal(T().jpeg_decode_batch_checked([f], device=gpu_device).cpu().numpy()[0], dec.pillow_pixels(f))


def _guarded(nbytes, device, dtype=torch.uint8):
    big = torch.full((2 * GUARD + nbytes,), 0xA5, dtype=torch.uint8, device=device)
    return big, big[GUARD:GUARD + nbytes].view(dtype)


def _guards_intact(big, nbytes):
    return bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + nbytes:] == 0xA5).all())


def test_unaligned_out(gpu_device):
    """Host form into an `out` that starts one byte into a sentinel-filled buffer: the pixel half decides on 16-byte stores
    from the pointer as well as from 3W % 16 (at 48x64 the pointer alone decides).  Pixels equal Pillow, sentinels intact.  (This pins the results, not the flag: the
    hardware takes a 16-byte store at any address, so a wrongly set flag would cost speed and show here only as a fault.)"""
    for (n, h, w), order in (((2, 48, 64), "bgr"), ((2, 33, 47), "rgb")):
        files = [pillow_file(jpeg_ref.frame("noise", h, w, i), 90) for i in range(n)]
        nbytes = n * h * w * 3
        big = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=gpu_device)
        out = big[1:1 + nbytes].view(n, h, w, 3)
        assert out.data_ptr() % 16 == 1
        got, status = T().jpeg_decode_batch(files, channel_order=order, out=out, device=gpu_device)
        assert got.data_ptr() == out.data_ptr() and not status.cpu().numpy().any()
        px = out.cpu().numpy()
        for i, f in enumerate(files):
            assert np.array_equal(px[i], dec.pillow_pixels(f, order == "rgb")), (h, w, i)
        assert bool((big[:1] == 0xA5).all()) and bool((big[1 + nbytes:] == 0xA5).all()), (h, w)


def test_damaged_streams(gpu_device):
    """Each damaged 48 x 80 file sits between two good ones.  The CPU model (test_jpeg_decode_cpu.py) has run the same bytes with
    every index asserted in range.  Status non-zero where the model's is, neighbours equal Pillow, guard bytes intact."""
    good = pillow_file(jpeg_ref.frame("gradient", 48, 80, 2), 90, optimize=True)
    want = dec.pillow_pixels(good)
    damaged = dec.damaged_streams()
    files = [good]
    for _, data in damaged:
        files += [data, good]
    n = len(files)
    max_file = max(map(len, files))
    need = T().jpeg_decode_scratch(n, 48, 80, max_file, gpu_device).numel()
    big_o, out = _guarded(n * 48 * 80 * 3, gpu_device)
    big_s, status = _guarded(4 * n, gpu_device, torch.int32)
    big_x, scratch = _guarded(need, gpu_device)
    T().jpeg_decode_batch(files, out=out.view(n, 48, 80, 3), status=status, scratch=scratch, device=gpu_device)
    torch.cuda.synchronize()
    st, px = status.cpu().numpy(), out.view(n, 48, 80, 3).cpu().numpy()
    assert _guards_intact(big_o, out.numel()) and _guards_intact(big_s, 4 * n) and _guards_intact(big_x, need)
    for i in range(0, n, 2):
        assert st[i] == 0 and np.array_equal(px[i], want), i
    for j, (name, data) in enumerate(damaged):
        model = dec.decode_coefficients_wave(data)[1]
        assert st[2 * j + 1] == model, (name, st[2 * j + 1], model)
        if not name.startswith("flip"):
            assert st[2 * j + 1] != 0, name
    with pytest.raises(ValueError, match="frame 1 "):
        T().jpeg_decode_batch_checked(files[:3], device=gpu_device)


def test_damaged_device_form(gpu_device):
    """Device form: a lengths[i] shorter than the header, a slot that does not start with the header, a length past the slot."""
    x = torch.from_numpy(np.stack([jpeg_ref.frame("noise", 48, 80, s) for s in range(7)])).to(gpu_device)
    want = T().jpeg_roundtrip_batch(x, 90)
    files, lengths = T().jpeg_encode_batch(x, 90)
    files, lengths = files.clone(), lengths.clone()
    lengths[1] = 100
    files[3, 200] ^= 1
    lengths[5] = files.shape[1] + 12345
    n = 7
    need = T().jpeg_decode_scratch(n, 48, 80, files.shape[1], gpu_device).numel()
    big_o, out = _guarded(n * 48 * 80 * 3, gpu_device)
    big_s, status = _guarded(4 * n, gpu_device, torch.int32)
    big_x, scratch = _guarded(need, gpu_device)
    T().jpeg_decode_batch(files, lengths, header=T().jpeg_header(90, 48, 80), out=out.view(n, 48, 80, 3), status=status,
                          scratch=scratch)
    torch.cuda.synchronize()
    st = status.cpu().numpy()
    assert _guards_intact(big_o, out.numel()) and _guards_intact(big_s, 4 * n) and _guards_intact(big_x, need)
    assert st[1] == 2 and st[3] == 1 and st[5] == 0 and not st[[0, 2, 4, 6]].any(), st
    got = out.view(n, 48, 80, 3)
    for i in (0, 2, 4, 5, 6):                                  # (frame 5's file is whole: its surplus length is clamped to the slot)
        assert torch.equal(got[i], want[i]), i
    with pytest.raises(ValueError, match="header"):
        T().jpeg_decode_batch(files, lengths, header=T().jpeg_header(90, 48, 80)[:-1])


def test_argument_errors(gpu_device):
    t = T()
    x = jpeg_ref.frame("gradient", 16, 16, 1)
    good = pillow_file(x, 90)
    dev = torch.device(gpu_device)
    ok_out = torch.empty((1, 16, 16, 3), dtype=torch.uint8, device=dev)
    bad_calls = [
        dict(files=[]),
        dict(files=[good], channel_order="gbr"),
        dict(files=[good, pillow_file(jpeg_ref.frame("gradient", 16, 32, 1), 90)]),
        dict(files=[good, pillow_file(x, 90, progressive=True)]),
        dict(files=[good], out=ok_out.float()),
        dict(files=[good], out=ok_out.cpu()),
        dict(files=[good], out=torch.empty((1, 16, 16, 6), dtype=torch.uint8, device=dev)[..., ::2]),
        dict(files=[good], out=torch.empty((2, 16, 16, 3), dtype=torch.uint8, device=dev)),
        dict(files=[good], status=torch.empty(1, dtype=torch.int64, device=dev)),
        dict(files=[good], scratch=torch.empty(16, dtype=torch.uint8, device=dev)),
        dict(files=[good], lengths=torch.zeros(1, dtype=torch.int32, device=dev)),
        dict(files=[12345]),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            t.jpeg_decode_batch(device=gpu_device, **kw)
    with pytest.raises(ValueError, match="frame 1"):
        t.jpeg_decode_batch([good, pillow_file(x, 90, progressive=True)], device=gpu_device)
    need = t.jpeg_decode_scratch(1, 16, 16, len(good), gpu_device).numel()
    buf = torch.empty(need + 16 * 16 * 3 + 64, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="overlap"):
        t.jpeg_decode_batch([good], out=buf[:768].view(1, 16, 16, 3), scratch=buf, device=gpu_device)
    dfiles, dlen = t.jpeg_encode_batch(torch.from_numpy(x[None]).to(dev), 90)
    hdr = t.jpeg_header(90, 16, 16)
    for kw in (dict(lengths=None), dict(lengths=dlen.long()), dict(lengths=dlen, header=None), dict(lengths=dlen.cpu())):
        kw.setdefault("header", hdr)
        with pytest.raises(ValueError):
            t.jpeg_decode_batch(dfiles, **kw)
    with pytest.raises(ValueError):
        t.jpeg_decode_batch(dfiles[:, ::2], dlen, header=hdr)


def test_str_to_image_batch_and_read_mjpeg(gpu_device, tmp_path):
    from vlfm_amd.harness import BatchedEpisodes
    from vlfm_amd.utils.mjpeg import MjpegWriter, read_mjpeg

    x = torch.from_numpy(np.stack([jpeg_ref.frame(k, 33, 47, 8) for k in ("noise", "gradient", "checker8")])).to(gpu_device)
    back = T().str_to_image_batch(T().image_to_str_batch(x, 90), device=gpu_device)
    assert torch.equal(back, T().jpeg_roundtrip_batch(x, 90))

    sim = BatchedEpisodes(4, device=gpu_device, use_blip2=False, episode_len=500)
    written = {}
    for _ in range(3):
        sim.step()
        for name, frames in sim.render_jpeg().items():
            written.setdefault(name, []).extend(frames)
    for name, frames in written.items():
        path = tmp_path / f"{name}.mjpeg"
        with MjpegWriter(path) as wr:
            for f in frames:
                wr.append(f)
        got = torch.cat(list(read_mjpeg(path, device=gpu_device, batch=5))).cpu().numpy()
        assert got.shape[0] == len(frames) == 12
        for i, f in enumerate(frames):
            assert np.array_equal(got[i], dec.pillow_pixels(f, True)), (name, i)
    mixed = tmp_path / "mixed.mjpeg"
    with MjpegWriter(mixed) as wr:
        wr.append(pillow_file(jpeg_ref.frame("noise", 16, 16, 1), 90))
        wr.append(pillow_file(jpeg_ref.frame("noise", 16, 32, 1), 90))
    with pytest.raises(ValueError, match="frame 1"):
        list(read_mjpeg(mixed, device=gpu_device))
