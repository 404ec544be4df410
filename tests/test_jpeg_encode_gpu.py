"""-m gpu: the device JPEG encoder (``transport.jpeg_encode_batch``, csrc/jpeg_codec.hip + csrc/jpeg_entropy.hip) writes, byte
for byte, the file the installed Pillow writes for the same frame (``save(format="JPEG", quality=q, subsampling="4:2:0")``):
at every size, content class, quality, channel order and batch size; never outside a frame's slot; and through
``BatchedEpisodes.render_jpeg`` and ``image_to_str_batch``.  Every comparison is equality of bytes."""
import base64
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_huff_ref  # noqa: E402
import jpeg_ref  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 4096
ORDERS = ["bgr", "rgb"]


def _natural(rng, h, w):
    """A seeded frame with smooth structure, edges and sensor noise (distinct per draw)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b, c = rng.uniform(3, 40, 3)
    img = np.stack([127 + 100 * np.sin(xx / a + rng.uniform(0, 6)), 127 + 100 * np.cos(yy / b + rng.uniform(0, 6)),
                    (xx + yy) * c % 256], axis=-1)
    for _ in range(4):
        y0, x0 = rng.integers(0, h), rng.integers(0, w)
        img[y0:y0 + rng.integers(1, h // 2 + 2), x0:x0 + rng.integers(1, w // 2 + 2)] = rng.integers(0, 256, 3)
    return np.clip(img + rng.normal(0, rng.uniform(0, 12), img.shape), 0, 255).astype(np.uint8)


def _batch(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return np.stack([_natural(rng, h, w) if i % 3 else rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for i in range(n)])


def _pillow(frames, q, order):
    return [jpeg_huff_ref.pillow_bytes(f, q, rgb_order=(order == "rgb")) for f in frames]


def _encode(x, q, order, capacity=None):
    """jpeg_encode_batch of the device tensor ``x``, twice: into buffers of its own, and into sentinel-filled slots with a
    guard region behind the last.  Checks that the input is unchanged, that both calls agree and that no byte behind a
    file's end (or behind the slot, for a file that does not fit) was written; returns (what each slot holds of its file,
    the lengths)."""
    from vlfm_amd.vlm.transport import jpeg_encode_batch, jpeg_encode_bound

    n, h, w, _ = x.shape
    cap = jpeg_encode_bound(h, w) if capacity is None else capacity
    x_before = x.clone()
    out, lengths = jpeg_encode_batch(x, q, order, capacity=cap)
    assert out.shape == (n, cap) and out.dtype == torch.uint8 and lengths.shape == (n,) and lengths.dtype == torch.int32
    # a second call into caller-provided buffers: sentinel-filled slots back to back, a guard region behind the last
    flat = torch.full((n * cap + GUARD,), SENTINEL, dtype=torch.uint8, device=x.device)
    out2 = flat[:n * cap].view(n, cap)
    len2 = torch.full((n,), -1, dtype=torch.int32, device=x.device)
    got = jpeg_encode_batch(x, q, order, capacity=cap, out=out2, lengths=len2)
    assert got[0].data_ptr() == out2.data_ptr() and got[1].data_ptr() == len2.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(x, x_before), "input changed"
    lens = len2.cpu().numpy().astype(np.int64)
    assert np.array_equal(lens, lengths.cpu().numpy())
    host = flat.cpu().numpy()
    assert np.all(host[n * cap:] == SENTINEL), "wrote behind the last slot"
    first = out.cpu().numpy()
    files = []
    for i in range(n):
        used = int(min(lens[i], cap))
        slot = host[i * cap:(i + 1) * cap]
        assert np.all(slot[used:] == SENTINEL), f"frame {i}: wrote behind its file's end"
        assert np.array_equal(first[i, :used], slot[:used]), f"frame {i}: two calls, two results"
        files.append(slot[:used].tobytes())
    return files, lens


def _diff(a: bytes, b: bytes):
    n = min(len(a), len(b))
    return len(a), len(b), next((i for i in range(n) if a[i] != b[i]), n)


def _check(frames, q, order, device):
    files, lens = _encode(torch.from_numpy(frames).to(device), q, order)
    want = _pillow(frames, q, order)
    for i in range(len(frames)):
        assert lens[i] == len(want[i]) and files[i] == want[i], (frames.shape, q, order, i) + _diff(files[i], want[i])
    return files


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("hw", jpeg_ref.SIZES + [(33, 40)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_device_bytes_equal_pillow_over_sizes_and_classes_q90(gpu_device, hw, order):
    frames = np.stack([jpeg_ref.frame(k, *hw, seed=i) for i, k in enumerate(jpeg_ref.CONTENT)])
    files = _check(frames, 90, order, gpu_device)
    if hw[0] * hw[1] <= 480 * 640:     # ... and the restatement, which says why
        assert files[0] == jpeg_huff_ref.encode(frames[0], 90, order == "rgb")


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("q", [1, 50, 100])
@pytest.mark.parametrize("hw", [(480, 640), (479, 641), (1000, 1000), (17, 9), (1, 1), (33, 40)],
                         ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_device_bytes_equal_pillow_at_other_qualities(gpu_device, hw, q, order):
    """479x641: dummy blocks at the right edge only; 1000x1000 and 17x9: a dummy bottom row; 33x40: both."""
    frames = np.stack([jpeg_ref.frame(k, *hw, seed=10 + i) for i, k in enumerate(jpeg_ref.CONTENT)])
    _check(frames, q, order, gpu_device)


_CACHE = {}


def _big_batch(gpu_device):
    if "b256" not in _CACHE:
        frames = _batch(256, 480, 640, seed=256)
        _CACHE["b256"] = frames, _check(frames, 90, "bgr", gpu_device)
    return _CACHE["b256"]


@pytest.mark.parametrize("n", [1, 3, 64, 256])
def test_batches_of_distinct_640x480_frames(gpu_device, n):
    if n == 256:
        _big_batch(gpu_device)
    else:
        _check(_batch(n, 480, 640, seed=n), 90, "bgr", gpu_device)


def test_sixteen_1280x720_frames(gpu_device):
    _check(_batch(16, 720, 1280, seed=16), 90, "rgb", gpu_device)


def test_frame_alone_equals_frame_inside_the_batch(gpu_device):
    frames, files = _big_batch(gpu_device)
    for i in (0, 1, 97, 255):
        alone, _ = _encode(torch.from_numpy(frames[i:i + 1]).to(gpu_device), 90, "bgr")
        assert alone[0] == files[i], i


@pytest.mark.parametrize("hw", [(48, 64), (479, 641)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_input_view_at_an_odd_byte_offset(gpu_device, hw):
    """48x64: rows of 3W % 16 == 0 bytes read from a pointer that is not 16-byte aligned; 479x641: byte loads anyway."""
    from vlfm_amd.vlm.transport import jpeg_encode_batch_bytes

    frames = _batch(5, *hw, seed=hw[0])
    for offset in (1, 3):
        raw = torch.zeros(frames.size + offset, dtype=torch.uint8, device=gpu_device)
        x = raw[offset:].view(frames.shape)
        x.copy_(torch.from_numpy(frames))
        assert x.data_ptr() % 2 == 1
        files, _ = _encode(x, 75, "bgr")
        assert files == _pillow(frames, 75, "bgr")
        assert jpeg_encode_batch_bytes(x, 75, "rgb") == _pillow(frames, 75, "rgb")


def test_decoded_bgr_files_equal_the_shipped_round_trip(gpu_device):
    """What ``jpeg_roundtrip_batch`` says the server sees is what decoding the encoder's file gives."""
    from PIL import Image

    from vlfm_amd.vlm.transport import jpeg_encode_batch_bytes, jpeg_roundtrip_batch

    for hw in [(480, 640), (33, 40), (17, 9)]:
        frames = _batch(4, *hw, seed=7 + hw[0])
        x = torch.from_numpy(frames).to(gpu_device)
        files = jpeg_encode_batch_bytes(x, 90, "bgr")
        trip = jpeg_roundtrip_batch(x, 90).cpu().numpy()
        for i, f in enumerate(files):
            back = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[..., ::-1]
            assert np.array_equal(back, trip[i]), (hw, i)


def test_a_frame_that_does_not_fit_stays_inside_its_slot(gpu_device):
    """Gradient 480x640 at q 50 (fits 65 536 bytes) next to noise 480x640 at q 100 (does not); the lengths come from Pillow.
    A call has one quality, so that pair is two calls into neighbouring slots of one buffer; the same two frames then go
    through one call at q 50 (frame 0 fits, frame 1 does not) and at q 100 (neither fits)."""
    from vlfm_amd.vlm.transport import jpeg_encode_batch, jpeg_encode_batch_bytes

    cap = 65536
    f0, f1 = jpeg_ref.frame("gradient", 480, 640, seed=1), jpeg_ref.frame("noise", 480, 640, seed=2)
    want = [jpeg_huff_ref.pillow_bytes(f0, 50), jpeg_huff_ref.pillow_bytes(f1, 100)]
    assert len(want[0]) <= cap < len(want[1])
    flat = torch.full((2 * (cap + GUARD),), SENTINEL, dtype=torch.uint8, device=gpu_device)
    slots = [flat[i * (cap + GUARD):i * (cap + GUARD) + cap].view(1, cap) for i in range(2)]
    lens = torch.zeros(2, dtype=torch.int32, device=gpu_device)
    for i, (f, q) in enumerate([(f0, 50), (f1, 100)]):
        jpeg_encode_batch(torch.from_numpy(f[None]).to(gpu_device), q, "bgr", capacity=cap, out=slots[i],
                          lengths=lens[i:i + 1])
    torch.cuda.synchronize()
    host = flat.cpu().numpy().reshape(2, cap + GUARD)
    assert lens.cpu().tolist() == [len(want[0]), len(want[1])]
    assert host[0, :len(want[0])].tobytes() == want[0]
    assert np.all(host[0, len(want[0]):] == SENTINEL)
    assert host[1, :cap].tobytes() == want[1][:cap]            # cut at the capacity, right up to it
    assert np.all(host[:, cap:] == SENTINEL), "guard regions behind the slots were touched"
    # the same inside one batch: [gradient, noise] at q 100 and at q 50 -- the noise frame overflows at both
    x = torch.from_numpy(np.stack([f0, f1])).to(gpu_device)
    for q in (50, 100):
        w = _pillow([f0, f1], q, "bgr")
        assert len(w[1]) > cap
        files, lengths = _encode(x, q, "bgr", capacity=cap)
        assert lengths.tolist() == [len(w[0]), len(w[1])]
        assert files[1] == w[1][:cap]
        if len(w[0]) <= cap:
            assert files[0] == w[0]
        else:
            assert files[0] == w[0][:cap]
        with pytest.raises(ValueError, match=r"\b1\b") as exc:
            jpeg_encode_batch_bytes(x, q, "bgr", capacity=cap)
        if len(w[0]) <= cap:
            assert "[1]" in str(exc.value)
    assert len(_pillow([f0], 50, "bgr")[0]) <= cap             # (so q 50 above did check a complete frame 0)


def test_bad_arguments_raise_value_error(gpu_device):
    from vlfm_amd.vlm.transport import jpeg_encode_batch, jpeg_encode_bound, jpeg_encode_scratch

    x = torch.zeros((2, 16, 24, 3), dtype=torch.uint8, device=gpu_device)
    cap = jpeg_encode_bound(16, 24)

    def u8(*shape, **kw):
        return torch.empty(shape, dtype=torch.uint8, device=kw.get("device", gpu_device))

    big = jpeg_encode_scratch(4, 16, 24, gpu_device)
    assert big.numel() >= 2 * cap
    cases = [
        lambda: jpeg_encode_batch(x.float()),
        lambda: jpeg_encode_batch(x[0]),
        lambda: jpeg_encode_batch(torch.zeros((2, 16, 24, 4), dtype=torch.uint8, device=gpu_device)),
        lambda: jpeg_encode_batch(x.cpu()),
        lambda: jpeg_encode_batch(x.cpu().numpy()),
        lambda: jpeg_encode_batch(x[:, :, ::2]),
        lambda: jpeg_encode_batch(x.permute(0, 2, 1, 3)),
        lambda: jpeg_encode_batch(x[:0]),
        lambda: jpeg_encode_batch(x, 0),
        lambda: jpeg_encode_batch(x, 101),
        lambda: jpeg_encode_batch(x, 90.0),
        lambda: jpeg_encode_batch(x, True),
        lambda: jpeg_encode_batch(x, 90, "gbr"),
        lambda: jpeg_encode_batch(x, 90, "bgr", capacity=0),
        lambda: jpeg_encode_batch(x, 90, "bgr", capacity=-4),
        lambda: jpeg_encode_batch(x, 90, "bgr", capacity=1.5),
        lambda: jpeg_encode_batch(x, out=u8(2, cap + 1), capacity=cap),
        lambda: jpeg_encode_batch(x, out=u8(1, cap)),
        lambda: jpeg_encode_batch(x, out=u8(2, cap).to(torch.int16)),
        lambda: jpeg_encode_batch(x, out=u8(2, cap, device="cpu")),
        lambda: jpeg_encode_batch(x, out=u8(2, 2 * cap)[:, ::2]),
        lambda: jpeg_encode_batch(x, lengths=torch.zeros(3, dtype=torch.int32, device=gpu_device)),
        lambda: jpeg_encode_batch(x, lengths=torch.zeros(2, dtype=torch.int64, device=gpu_device)),
        lambda: jpeg_encode_batch(x, lengths=torch.zeros(2, dtype=torch.int32)),
        lambda: jpeg_encode_batch(x, scratch=jpeg_encode_scratch(1, 16, 24, gpu_device)),
        lambda: jpeg_encode_batch(x, scratch=jpeg_encode_scratch(2, 16, 24, gpu_device).float()),
        lambda: jpeg_encode_batch(x, scratch=jpeg_encode_scratch(2, 16, 24, gpu_device)[1:]),
        lambda: jpeg_encode_batch(x, out=big[:2 * cap].view(2, cap), scratch=big),
    ]
    for i, call in enumerate(cases):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"case {i} did not raise")
    out, lengths = jpeg_encode_batch(x, scratch=jpeg_encode_scratch(2, 16, 24, gpu_device))   # the right scratch is accepted
    assert lengths.cpu().tolist() == [len(jpeg_huff_ref.pillow_bytes(np.zeros((16, 24, 3), np.uint8), 90))] * 2


def test_batched_episodes_render_jpeg(gpu_device):
    from PIL import Image

    from vlfm_amd.harness import BatchedEpisodes

    sim = BatchedEpisodes(8, device=gpu_device, use_blip2=False, world="rooms", episode_len=500, render_trajectories=True)
    for _ in range(20):
        sim.step()
    frames = {k: v.cpu().numpy() for k, v in sim.render().items()}
    files = sim.render_jpeg()
    assert set(files) == set(frames) == {"value_map", "obstacle_map"}
    for name, fs in files.items():
        assert len(fs) == 8
        for e, f in enumerate(fs):
            assert f == jpeg_huff_ref.pillow_bytes(frames[name][e], 90, rgb_order=True), (name, e)
            assert Image.open(io.BytesIO(f)).size == (1000, 1000)
    some = sim.render_jpeg(env_ids=[5, 2], quality=50)
    for name, fs in some.items():
        assert fs == [jpeg_huff_ref.pillow_bytes(frames[name][e], 50, rgb_order=True) for e in (5, 2)], name


def test_image_to_str_batch_round_trips_through_base64(gpu_device):
    from vlfm_amd.vlm.transport import image_to_str_batch

    frames = _batch(3, 480, 640, seed=11)
    strs = image_to_str_batch(torch.from_numpy(frames).to(gpu_device), 90)
    assert all(isinstance(s, str) for s in strs)
    assert [base64.b64decode(s) for s in strs] == _pillow(frames, 90, "bgr")
