"""NumPy restatement of the baseline JPEG file that Pillow's ``save(format="JPEG", quality=q, subsampling="4:2:0")`` writes
through libjpeg-turbo: the 623-byte frame header, then one interleaved Huffman-coded scan with the standard (Annex K) tables.

Test infrastructure, like jpeg_ref.py, from which the quantised coefficients come by import: the oracle that the device
encoder (csrc/jpeg_codec.hip, ``transport.jpeg_encode_batch``) is explained by, itself held to Pillow byte for byte in
test_jpeg_encode_cpu.py.  Each step names the libjpeg routine it restates.

Channel order: ``rgb_order=False`` reads slot 2 of a pixel as R (what cv2.imencode does with the reference's RGB frame, and
the convention of jpeg_ref.py); ``rgb_order=True`` reads slot 0 as R (``Image.fromarray(rgb).save``).
"""
from __future__ import annotations

import numpy as np

import jpeg_ref

# jutils.c jpeg_natural_order: ZIGZAG[k] is the natural (row-major) index of the k-th coefficient in zigzag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63], np.int64)

# jcparam.c std_huff_tables (JPEG Annex K.3 - K.6): BITS[1..16] and HUFFVAL
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa]

HEADER_BYTES = 623


def _derive(bits, vals):
    """jchuff.c jpeg_make_c_derived_tbl: (code[256], length[256]) indexed by symbol; length 0 = no code."""
    assert sum(bits) == len(vals)
    code = np.zeros(256, np.int64)
    length = np.zeros(256, np.int64)
    c, k = 0, 0
    for n in range(1, 17):
        for _ in range(bits[n - 1]):
            code[vals[k]], length[vals[k]] = c, n
            c += 1
            k += 1
        c <<= 1
    return code, length


DC_TABLES = [_derive(DC_LUMA_BITS, DC_VALS), _derive(DC_CHROMA_BITS, DC_VALS)]
AC_TABLES = [_derive(AC_LUMA_BITS, AC_LUMA_VALS), _derive(AC_CHROMA_BITS, AC_CHROMA_VALS)]


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(quality: int, h: int, w: int) -> bytes:
    """Rule 1: SOI, APP0 (jcmarker.c emit_jfif_app0), DQT x 2, SOF0, DHT x 4, SOS -- 623 bytes for any (q, H, W)."""
    qt = jpeg_ref.quant_tables(quality)
    out = b"\xff\xd8"
    out += _segment(0xE0, b"JFIF\x00" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i in range(2):                                       # emit_dqt: 8-bit precision, entries in zigzag order
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in qt[i][ZIGZAG]))
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes(
        [3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


def scan_blocks(image: np.ndarray, quality: int, rgb_order: bool = False) -> np.ndarray:
    """Rules 2 and 3: the quantised coefficients of every block of the scan, [6 * MCUs, 64] in zigzag order, blocks in
    scan order (MCUs row-major; Y00 Y01 Y10 Y11 Cb Cr), with jccoefct.c compress_data's dummy blocks at the right and
    bottom edges: AC all zero, DC that of the block coded just before it in the MCU."""
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    h, w = image.shape[:2]
    qt = jpeg_ref.quant_tables(quality)
    y_pad, cb_pad, cr_pad = jpeg_ref.encode_planes(image[..., ::-1] if rgb_order else image)
    mh, mw = -(-h // 16), -(-w // 16)
    bh, bw = -(-h // 8), -(-w // 8)                          # real luma block rows / columns
    yq = jpeg_ref.quantize(jpeg_ref.fdct_islow(jpeg_ref._blocks(y_pad) - 128), qt[0]).reshape(2 * mh, bw, 64)
    cq = [jpeg_ref.quantize(jpeg_ref.fdct_islow(jpeg_ref._blocks(p) - 128), qt[1]).reshape(mh, mw, 64)
          for p in (cb_pad, cr_pad)]
    out = np.zeros((mh, mw, 6, 64), np.int64)
    for k in range(4):
        r, c = k >> 1, k & 1
        rows, cols = np.arange(mh) * 2 + r, np.arange(mw) * 2 + c
        real = (rows < bh)[:, None] & (cols < bw)[None, :]
        blk = yq[np.minimum(rows, 2 * mh - 1)][:, np.minimum(cols, bw - 1)]
        out[:, :, k] = np.where(real[..., None], blk, 0)
        if k:
            out[:, :, k, 0] = np.where(real, blk[..., 0], out[:, :, k - 1, 0])
    out[:, :, 4], out[:, :, 5] = cq
    return out.reshape(-1, 64)[:, ZIGZAG]


def _bit_length(a: np.ndarray) -> np.ndarray:
    n = np.zeros(a.shape, np.int64)
    v = np.abs(a)
    while np.any(v):
        n += v > 0
        v = v >> 1
    return n


def entropy_tokens(zz: np.ndarray):
    """Rules 4 and 5 (jchuff.c encode_one_block): (value, bit length) of every token of the scan, in stream order.  One
    token per DC difference, per non-zero AC coefficient (its ZRLs, its run/size code and its amplitude bits together:
    at most 3 * 11 + 16 + 10 = 59 bits) and per EOB."""
    nb = zz.shape[0]
    comp = np.array([0, 0, 0, 0, 1, 2])[np.arange(nb) % 6]
    tab = (comp > 0).astype(np.int64)
    # DC: difference to the previous block of the same component, predictor 0 at the start of the scan
    dc = zz[:, 0]
    diff = np.zeros(nb, np.int64)
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        diff[idx] = dc[idx] - np.concatenate([[0], dc[idx][:-1]])
    size = _bit_length(diff)
    amp = np.where(diff >= 0, diff, diff - 1) & ((1 << size) - 1)
    dcode = np.stack([DC_TABLES[0][0], DC_TABLES[1][0]])[tab, size]
    dlen = np.stack([DC_TABLES[0][1], DC_TABLES[1][1]])[tab, size]
    keys = [np.arange(nb) * 65]                              # stream order key: block * 65 + position
    vals = [(dcode << size) | amp]
    lens = [dlen + size]
    # AC
    accode = np.stack([AC_TABLES[0][0], AC_TABLES[1][0]])
    aclen = np.stack([AC_TABLES[0][1], AC_TABLES[1][1]])
    b, k = np.nonzero(zz[:, 1:])
    k = k + 1
    prev = np.where(np.concatenate([[True], b[1:] != b[:-1]]), 0, np.concatenate([[0], k[:-1]]))
    run = k - prev - 1
    v = zz[b, k]
    size = _bit_length(v)
    assert size.size == 0 or size.max() <= 10
    amp = np.where(v >= 0, v, v - 1) & ((1 << size) - 1)
    t = tab[b]
    sym = ((run & 15) << 4) | size
    val = (accode[t, sym] << size) | amp
    ln = aclen[t, sym] + size
    zrl_code, zrl_len = accode[t, 0xF0], aclen[t, 0xF0]
    for z in (1, 2, 3):                                      # run >> 4 ZRL codes in front
        m = (run >> 4) >= z
        val = np.where(m, val | (zrl_code << ln), val)
        ln = np.where(m, ln + zrl_len, ln)
    keys.append(b * 65 + k)
    vals.append(val)
    lens.append(ln)
    eob = np.nonzero(zz[:, 63] == 0)[0]
    keys.append(eob * 65 + 64)
    vals.append(accode[tab[eob], 0])
    lens.append(aclen[tab[eob], 0])
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(vals)[order], np.concatenate(lens)[order]


def pack(vals: np.ndarray, lens: np.ndarray) -> bytes:
    """Rule 6: MSB first, the last byte padded with 1-bits, every 0xFF followed by 0x00."""
    off = np.cumsum(lens) - lens
    total = int(lens.sum())
    bits = np.ones(-(-total // 8) * 8, np.uint8)
    for j in range(int(lens.max())):
        m = lens > j
        bits[off[m] + j] = (vals[m] >> (lens[m] - 1 - j)) & 1
    data = np.packbits(bits)
    ff = np.nonzero(data == 0xFF)[0]
    return np.insert(data, ff + 1, 0).tobytes()


def encode(image: np.ndarray, quality: int = 90, rgb_order: bool = False) -> bytes:
    """The whole file for an (H,W,3) uint8 frame."""
    h, w = image.shape[:2]
    vals, lens = entropy_tokens(scan_blocks(image, quality, rgb_order))
    return header(quality, h, w) + pack(vals, lens) + b"\xff\xd9"


def pillow_bytes(image: np.ndarray, quality: int = 90, rgb_order: bool = False) -> bytes:
    """What the tests compare against: the installed Pillow's file for the same frame."""
    import io

    from PIL import Image

    buf = io.BytesIO()
    img = np.ascontiguousarray(image if rgb_order else image[..., ::-1])
    Image.fromarray(img).save(buf, format="JPEG", quality=int(quality), subsampling="4:2:0")
    return buf.getvalue()
