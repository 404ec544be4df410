"""NumPy / Python restatement of the baseline 4:2:0 JPEG decoder (csrc/jpeg_decode.hip, ``transport.jpeg_decode_batch``).

Test infrastructure, like jpeg_ref.py and jpeg_huff_ref.py, from which the pixel half and the encoder's pieces come by import:

* ``parse``: the markers in front of the scan (what ``vlfm_jpeg_parse_host`` fills).
* ``unstuff``: byte unstuffing and the split at RSTn.
* ``decode_coefficients``: a plain sequential Huffman decoder with the file's own tables -> the encoder's coefficient layout
  ([6 * MCUs, 64] in zigzag order, blocks in scan order, absolute DC values).
* ``decode_coefficients_wave``: a model of the kernel's in-wave scheme -- 64 candidate tokens per window, a chain walk over
  them -- that asserts every index it forms is in range and returns a status for a damaged stream instead of raising.
* ``pixels`` / ``decode``: coefficients -> frame through jpeg_ref's IDCT, upsampling and colour conversion.
* ``restart_file`` / ``coefficient_file``: writers of files with restart markers and of files from given coefficients.
"""
from __future__ import annotations

import numpy as np

import jpeg_huff_ref as huff
import jpeg_ref

ZIGZAG = huff.ZIGZAG
BAD_HEADER, BAD_LENGTH, BAD_EOI, BAD_RESTART, BAD_CODE, BAD_SIZE, BAD_INDEX, BAD_BITS = range(1, 9)
STAGE_BYTES = 1024


class Unsupported(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------- parsing
def derive(bits, vals):
    """The compare form of a Huffman table: a left-aligned 16-bit window x has code length 1 + #{l : x >= limit[l]} and
    symbol vals[(x >> (16 - len)) - delta[len - 1]]."""
    limit, delta = np.zeros(16, np.int64), np.zeros(16, np.int64)
    code = k = 0
    for l in range(1, 17):
        delta[l - 1] = code - k
        code += bits[l - 1]
        k += bits[l - 1]
        if code > (1 << l):
            raise Unsupported("malformed marker segment")
        limit[l - 1] = code << (16 - l)
        code <<= 1
    v = np.zeros(256, np.int64)
    v[:len(vals)] = list(vals)
    return {"limit": limit, "delta": delta, "vals": v, "bits": list(bits), "symbols": list(vals)}


def parse(data: bytes) -> dict:
    """height, width, restart_interval, scan_offset, quant [3,64] (natural order), dc / ac: per component a derived table."""
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Unsupported("not a JPEG file")
    quant, hts, sof, ri = {}, {}, None, 0
    i = 2
    while True:
        if i + 1 >= len(data):
            raise Unsupported("no scan")
        if data[i] != 0xFF:
            raise Unsupported("malformed marker segment")
        while i + 1 < len(data) and data[i + 1] == 0xFF:
            i += 1
        m = data[i + 1]
        i += 2
        sl = int.from_bytes(data[i:i + 2], "big")
        s = data[i + 2:i + sl]
        if sl < 2 or i + sl > len(data):
            raise Unsupported("no scan")
        if m == 0xC0:
            if sof is not None:
                raise Unsupported("hierarchical")
            if s[0] != 8:
                raise Unsupported("precision")
            h, w = int.from_bytes(s[1:3], "big"), int.from_bytes(s[3:5], "big")
            if h == 0 or w == 0:
                raise Unsupported("zero dimension")
            if s[5] != 3:
                raise Unsupported("components")
            comps = [(s[6 + 3 * c], s[7 + 3 * c], s[8 + 3 * c]) for c in range(3)]
            if [c[1] for c in comps] != [0x22, 0x11, 0x11]:
                raise Unsupported("sampling")
            sof = (h, w, comps)
        elif (0xC1 <= m <= 0xCF and m != 0xC4) or m in (0xDE, 0xDF):
            raise Unsupported("process")
        elif m == 0xDC:
            raise Unsupported("DNL")
        elif m == 0xDB:
            j = 0
            while j < len(s):
                if s[j] >> 4:
                    raise Unsupported("16-bit quantisation table")
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = list(s[j + 1:j + 65])
                quant[s[j] & 15] = t
                j += 65
        elif m == 0xC4:
            j = 0
            while j < len(s):
                bits = list(s[j + 1:j + 17])
                n = sum(bits)
                hts[(s[j] >> 4, s[j] & 15)] = derive(bits, s[j + 17:j + 17 + n])
                j += 17 + n
        elif m == 0xDD:
            ri = int.from_bytes(s[:2], "big")
        elif m == 0xEE and s[:5] == b"Adobe":
            raise Unsupported("Adobe")
        elif m == 0xDA:
            if sof is None:
                raise Unsupported("no frame header")
            if s[0] != 3 or [s[1 + 2 * c] for c in range(3)] != [c[0] for c in sof[2]] or tuple(s[7:10]) != (0, 63, 0):
                raise Unsupported("scan")
            try:
                return {"height": sof[0], "width": sof[1], "restart_interval": ri, "scan_offset": i + sl,
                        "quant": np.stack([quant[c[2]] for c in sof[2]]),
                        "dc": [hts[(0, s[2 + 2 * c] >> 4)] for c in range(3)],
                        "ac": [hts[(1, s[2 + 2 * c] & 15)] for c in range(3)]}
            except KeyError:
                raise Unsupported("missing table") from None
        i += sl


def unstuff(data: bytes, scan_offset: int):
    """(segments, status): the unstuffed bytes of every restart segment of the scan; status BAD_EOI / BAD_RESTART / 0."""
    segs, cur, i, n, status, nrst = [], bytearray(), scan_offset, len(data), 0, 0
    while True:
        if i >= n:
            status = BAD_EOI
            break
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        if i + 1 >= n:
            status = BAD_EOI
            break
        nx = data[i + 1]
        if nx == 0:
            cur.append(0xFF)
            i += 2
        elif nx == 0xFF:
            i += 1
        elif 0xD0 <= nx <= 0xD7:
            if (nx & 7) != (nrst & 7):
                status = BAD_RESTART
            nrst += 1
            segs.append(bytes(cur))
            cur = bytearray()
            i += 2
        else:
            if nx != 0xD9:
                status = BAD_EOI
            break
    segs.append(bytes(cur))
    return segs, status


def _geometry(info):
    mh, mw = -(-info["height"] // 16), -(-info["width"] // 16)
    mcus = mh * mw
    ri = info["restart_interval"] or mcus
    return mh, mw, mcus, ri, -(-mcus // ri)


# ------------------------------------------------------------------------------------------- the sequential decoder
def _code_dict(t):
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(t["bits"][l - 1]):
            out[(l, code)] = t["symbols"][k]
            code += 1
            k += 1
        code <<= 1
    return out


class _Bits:
    def __init__(self, data: bytes):
        self.v, self.n, self.pos = int.from_bytes(data, "big") if data else 0, 8 * len(data), 0

    def take(self, k: int) -> int:
        if self.pos + k > self.n:
            raise EOFError
        self.pos += k
        return (self.v >> (self.n - self.pos)) & ((1 << k) - 1)


def _symbol(br, codes):
    code = 0
    for l in range(1, 17):
        code = code << 1 | br.take(1)
        if (l, code) in codes:
            return codes[(l, code)]
    raise ValueError("no such code")


def _extend(v, size):
    return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1


def decode_coefficients(data: bytes) -> np.ndarray:
    """[6 * MCUs, 64] zigzag coefficients of a good file; raises on a damaged one."""
    info = parse(data)
    mh, mw, mcus, ri, nseg = _geometry(info)
    segs, status = unstuff(data, info["scan_offset"])
    if status or len(segs) != nseg:
        raise ValueError(f"scan status {status}, {len(segs)} segments for {nseg}")
    dc, ac = [_code_dict(t) for t in info["dc"]], [_code_dict(t) for t in info["ac"]]
    out = np.zeros((mcus * 6, 64), np.int64)
    for s, seg in enumerate(segs):
        br, pred = _Bits(seg), [0, 0, 0]
        for mcu in range(s * ri, min((s + 1) * ri, mcus)):
            for blk in range(6):
                c = 0 if blk < 4 else blk - 3
                size = _symbol(br, dc[c])
                pred[c] += _extend(br.take(size), size)
                out[mcu * 6 + blk, 0] = pred[c]
                k = 1
                while k < 64:
                    sym = _symbol(br, ac[c])
                    run, size = sym >> 4, sym & 15
                    if size == 0:
                        if run != 15:
                            break
                        k += 16
                        continue
                    k += run
                    if k > 63:
                        raise ValueError("zigzag index past 63")
                    out[mcu * 6 + blk, k] = _extend(br.take(size), size)
                    k += 1
    return out


# --------------------------------------------------------------------------------------- the model of the wave scheme
def _candidates(t, peek):
    """The kernel's ``candidate`` for 64 lanes: (value, run, size, total length, bad)."""
    x = peek >> 16
    ln = 1 + (x[:, None] >= t["limit"][None, :]).sum(1)
    bad = ln > 16
    lc = np.minimum(ln, 16)
    idx = (x >> (16 - lc)) - t["delta"][lc - 1]
    idx = np.clip(idx, 0, 255)
    sym = t["vals"][idx]
    size, run = sym & 15, sym >> 4
    assert np.all(lc + size <= 31)
    amp = np.where(size > 0, ((peek << lc) & 0xFFFFFFFF) >> (32 - np.maximum(size, 1)), 0)
    val = np.where(size > 0, np.where(amp >> np.maximum(size - 1, 0), amp, amp - (1 << size) + 1), 0)
    return val, run, size, lc + size, bad


def decode_segment_wave(seg_stream: np.ndarray, b0: int, b1: int, info, mcu0: int, mcu1: int, out: np.ndarray,
                        trace=None) -> int:
    """One wavefront's work: the segment is bytes [b0, b1) of the frame's unstuffed stream ``seg_stream`` (padded like the
    kernel's buffer).  Stores into ``out`` ([6 * MCUs * 64] flat) and returns the status."""
    ubytes = seg_stream.size
    tabs = info["dc"] + info["ac"]
    seg_bits = (b1 - b0) * 8
    pos, mcu, blk, k, pred = 0, mcu0, 0, 0, [0, 0, 0]
    lanes = np.arange(64)
    stage_base, stage = None, np.zeros(STAGE_BYTES, np.int64)
    while mcu < mcu1:
        need_hi = b0 + ((pos + 63) >> 3) + 8
        if stage_base is None or need_hi > stage_base + STAGE_BYTES:
            stage_base = (b0 + (pos >> 3)) & ~15
            for lane in range(64):
                at = stage_base + 16 * lane
                stage[16 * lane:16 * lane + 16] = seg_stream[at:at + 16] if at + 16 <= ubytes else 0
        p = pos + lanes
        bi = b0 + (p >> 3) - stage_base
        assert bi.min() >= 0 and bi.max() + 8 <= STAGE_BYTES
        w = np.zeros(64, np.int64)
        base = (bi >> 2) * 4
        for j in range(8):
            w = w << 8 | stage[base + j]
        peek = ((w << (8 * (bi & 3) + (p & 7))) >> 32) & 0xFFFFFFFF
        cands = [_candidates(t, peek) for t in tabs]
        off, marks = 0, []
        err = 0
        while off < 64:
            comp = 0 if blk < 4 else blk - 3
            val, run, size, tl, bad = (int(a[off]) for a in cands[comp if k == 0 else 3 + comp])
            assert 1 <= tl <= 31
            if bad:
                err = BAD_CODE
                break
            if pos + off + tl > seg_bits:
                err = BAD_BITS
                break
            end_block, at = False, -1
            if k == 0:
                if size > 11:
                    err = BAD_SIZE
                    break
                pred[comp] += val
                at, v, k = (mcu * 6 + blk) * 64, pred[comp], 1
            elif size == 0:
                if run == 15:
                    k += 16
                    end_block = k >= 64
                else:
                    end_block = True
            else:
                if size > 10:
                    err = BAD_SIZE
                    break
                k += run
                if k > 63:
                    err = BAD_INDEX
                    break
                at, v = (mcu * 6 + blk) * 64 + k, val
                k += 1
                end_block = k >= 64
            if at >= 0:
                marks.append((off, at, v))
            off += tl
            if end_block:
                k = 0
                blk += 1
                if blk == 6:
                    blk = 0
                    mcu += 1
                    if mcu == mcu1:
                        break
        assert len({m[0] for m in marks}) == len(marks)
        for _, at, v in marks:
            assert mcu0 * 384 <= at < mcu1 * 384, "a coefficient index outside the segment's blocks"
            out[at] = ((v + 32768) & 0xFFFF) - 32768
        if trace is not None:
            trace.append({"pos": pos, "tokens": len(marks), "advance": off,
                          "blocks_ended": sum(1 for m in marks if m[1] % 64 == 0)})
        pos += off
        if err:
            return err
    return 0


def decode_coefficients_wave(data: bytes, info=None, trace=None):
    """(coefficients [6 * MCUs, 64], status) by the kernel's scheme: scan statuses as the device reports them, one
    ``decode_segment_wave`` per restart segment.  Never raises for a damaged scan."""
    info = info or parse(data)
    mh, mw, mcus, ri, nseg = _geometry(info)
    status = 0
    if len(data) <= info["scan_offset"]:
        return np.zeros((mcus * 6, 64), np.int64), BAD_LENGTH
    segs, st = unstuff(data, info["scan_offset"])
    status = max(status, st)
    if len(segs) != nseg:
        status = max(status, BAD_RESTART)
    stream = b"".join(segs)
    starts = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    seg_tab = [int(starts[min(s, len(segs))]) for s in range(nseg + 1)]
    seg_tab[nseg] = len(stream)
    ubytes = ((len(data) + 15) & ~15) + 32
    buf = np.zeros(ubytes, np.int64)
    buf[:len(stream)] = list(stream)
    out = np.zeros(mcus * 384, np.int64)
    for s in range(nseg):
        b0 = min(seg_tab[s], len(stream))
        b1 = max(min(seg_tab[s + 1], len(stream)), b0)
        status = max(status, decode_segment_wave(buf, b0, b1, info, s * ri, min((s + 1) * ri, mcus), out, trace))
    return out.reshape(-1, 64), status


# -------------------------------------------------------------------------------------------------------------- pixels
def pixels(coef: np.ndarray, info, rgb_order: bool = False) -> np.ndarray:
    """[6 * MCUs, 64] zigzag coefficients -> the (H,W,3) uint8 frame (slot 0 = B unless ``rgb_order``)."""
    h, w = info["height"], info["width"]
    mh, mw = -(-h // 16), -(-w // 16)
    nat = np.zeros((mh, mw, 6, 64), np.int64)
    nat[..., ZIGZAG] = coef.reshape(mh, mw, 6, 64)
    q = info["quant"]
    y = np.zeros((2 * mh, 2 * mw, 8, 8), np.int64)
    for k in range(4):
        y[k >> 1::2, k & 1::2] = (nat[:, :, k] * q[0]).reshape(mh, mw, 8, 8)
    yp = jpeg_ref._unblocks(jpeg_ref.idct_islow(y))[:h, :w]
    planes = [jpeg_ref.upsample_h2v2(jpeg_ref._unblocks(jpeg_ref.idct_islow((nat[:, :, 3 + c] * q[c]).reshape(mh, mw, 8, 8))),
                                     h, w) for c in (1, 2)]
    out = jpeg_ref.ycc_to_rgb_slots(yp, planes[0], planes[1])
    return np.ascontiguousarray(out[..., ::-1]) if rgb_order else out


def decode(data: bytes, rgb_order: bool = False) -> np.ndarray:
    return pixels(decode_coefficients(data), parse(data), rgb_order)


def pillow_pixels(data: bytes, rgb_order: bool = False) -> np.ndarray:
    import io

    from PIL import Image

    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return np.ascontiguousarray(rgb if rgb_order else rgb[..., ::-1])


# -------------------------------------------------------------------------------------------------------------- writers
def _scan(zz: np.ndarray, ri: int) -> bytes:
    mcus = zz.shape[0] // 6
    if not ri:
        return huff.pack(*huff.entropy_tokens(zz))
    out = b""
    for i, m0 in enumerate(range(0, mcus, ri)):
        if i:
            out += bytes([0xFF, 0xD0 + ((i - 1) & 7)])
        out += huff.pack(*huff.entropy_tokens(zz[6 * m0:6 * min(m0 + ri, mcus)]))
    return out


def coefficient_file(zz: np.ndarray, quality: int, h: int, w: int, ri: int = 0) -> bytes:
    """The file whose scan holds the given [6 * MCUs, 64] zigzag coefficients, with the standard tables of ``quality``;
    ``ri`` > 0 adds DRI directly in front of SOS and codes every run of ``ri`` MCUs on its own."""
    head = huff.header(quality, h, w)
    if ri:
        sos = head.rindex(b"\xff\xda")
        head = head[:sos] + b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big") + head[sos:]
    return head + _scan(np.asarray(zz, np.int64), ri) + b"\xff\xd9"


def restart_file(image: np.ndarray, quality: int, ri: int, rgb_order: bool = False) -> bytes:
    """What Pillow's ``restart_marker_blocks=ri`` writes for the frame."""
    h, w = image.shape[:2]
    return coefficient_file(huff.scan_blocks(image, quality, rgb_order), quality, h, w, ri)


def insert_comment(data: bytes, length: int) -> bytes:
    """The file with a COM segment of ``length`` payload bytes directly in front of SOS."""
    sos = parse(data)["scan_offset"] - 14
    assert data[sos:sos + 2] == b"\xff\xda"
    return data[:sos] + b"\xff\xfe" + (length + 2).to_bytes(2, "big") + b"c" * length + data[sos:]


def damaged_streams():
    """(name, file bytes) of damaged 48 x 80 files: the CPU model and the device are fed the same ones."""
    x = jpeg_ref.frame("noise", 48, 80, 11)
    good = huff.encode(x, 90)
    rst = restart_file(x, 90, 5)
    out = [("truncated", good[:623 + (len(good) - 623) // 2] + b"\xff\xd9"), ("cut_no_eoi", good[:len(good) // 2])]
    for frac in (0.01, 0.3, 0.6, 0.95):
        pos = 623 + int((len(good) - 625) * frac)
        b = bytearray(good)
        b[pos] ^= 0x10
        if b[pos] == 0xFF or b[pos - 1] == 0xFF:
            b[pos] ^= 0x30
        out.append((f"flip_{frac}", bytes(b)))
    i0 = rst.index(b"\xff\xd0", 629)
    i1 = rst.index(b"\xff\xd1", i0)
    sw = bytearray(rst)
    sw[i0 + 1], sw[i1 + 1] = 0xD1, 0xD0
    out.append(("swapped_rst", bytes(sw)))
    out.append(("missing_rst", rst[:i1] + rst[i1 + 2:]))
    out.append(("all_ones", good[:623] + b"\xff\x00" * 300 + b"\xff\xd9"))
    out.append(("all_zero", good[:623] + b"\x00" * 300 + b"\xff\xd9"))
    return out


def crafted(kind: str, mcus: int = 6) -> np.ndarray:
    """[6 * mcus, 64] zigzag coefficients no encoder would make from pixels: compared in coefficients only."""
    rng = np.random.default_rng(7)
    zz = np.zeros((6 * mcus, 64), np.int64)
    if kind == "full":                                       # every coefficient +-1023: blocks longer than 1 500 bits
        zz[:] = rng.choice([-1023, 1023], zz.shape)
    elif kind == "last":                                     # a coefficient at zigzag 63: no EOB; long zero runs (ZRLs)
        zz[:, 63] = rng.integers(1, 200, zz.shape[0])
        zz[:, 0] = rng.integers(-500, 500, zz.shape[0])
    elif kind == "sparse":
        m = rng.random(zz.shape) < 0.05
        zz[m] = rng.integers(-200, 201, int(m.sum()))
    elif kind == "zeros":                                    # 32 bits per MCU: a dozen blocks end inside every window
        pass
    return zz
