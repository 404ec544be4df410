// jpeg_decode.hip -- gfx950 baseline JPEG decoder for a batch of files of one size: the frames libjpeg-turbo decodes as Pillow
// drives it (Image.open(...).convert("RGB")), bit for bit, for files an encoder made from 8-bit pixels.  tests/jpeg_dec_ref.py
// is the NumPy form, held to Pillow.  The pixel half (dequantise, islow IDCT, range limit, h2v2 fancy upsampling, colour) is
// jpeg_codec.hip's; this file is the entropy side: the host parser of the markers in front of the scan, byte unstuffing and
// restart segments, Huffman decoding with the file's own tables, DC prediction.
//
// Six launches per call, whatever the batch, and no host round trip between them:
//
//   jpeg_scan_count_kernel    one workgroup per 4096 file bytes: how many scan bytes stay after unstuffing, how many RSTn
//                             there are, where the first other marker is; compares the header in the device form.
//   jpeg_scan_offsets_kernel  one workgroup per frame: the first chunk with a terminating marker, exclusive scans of the counts
//                             of the chunks up to it; EOI and RSTn count checks; presets the frame's segment table.
//   jpeg_unstuff_kernel       one workgroup per 4096 file bytes: copies the bytes that stay, writes the start of the segment
//                             behind every RSTn and checks that the RSTn indices run 0..7 in order.
//   jpeg_huffman_kernel       one wavefront per (frame, restart segment).  Per window the 64 lanes look at 64 consecutive
//                             bit positions and each computes the token that would start at its position under each of the
//                             frame's six tables (canonical-Huffman compares against limit[l], no branch); then the wavefront
//                             walks the real chain from the window's entry position -- a scalar loop over readlane'd token
//                             records with state (position, block in MCU, zigzag index, DC predictors) -- and marks the lanes
//                             that are real token starts; those store their coefficients in parallel.  The next window
//                             starts where the chain left this one.  Cost is linear in the bits whatever they are.
//   jpeg_idct_kernel          (jpeg_codec.hip) coefficients x the frame's quantisation tables -> decoded planes.
//   jpeg_upsample_kernel<*>   (jpeg_codec.hip) planes -> frames.
//
// No workgroup waits for another one.  Every index formed from a stream's bits or length fields is range-checked or clamped
// before it is used for a load or a store; what is wrong with a stream ends up in the frame's status word.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "jpeg_common.h"
#include "profile.h"

namespace vlfm {
namespace jpeg {

constexpr int DCHUNK = 4096;          // file bytes per scan workgroup: 256 threads x 16 B
constexpr int STAGE_BYTES = 1024;     // unstuffed stream bytes a wavefront stages in LDS: 64 lanes x 16 B
constexpr uint32_t NONE = 0xffffffffu;
enum { KEEP = 0, DROP = 1, RST = 2, TERM = 3 };

struct Files {
    const uint8_t* base;
    size_t bytes;               // no byte at or past base + bytes is read
    const int64_t* offsets;     // or null: file f at f * stride, at most stride bytes
    size_t stride;
    const int32_t* lengths;
    size_t max_file;            // at most this much of a file is looked at
    const uint8_t* header;      // or null
    int header_bytes;
};

struct DecLayout {
    int n, mcus, chunks, max_seg;
    size_t ubytes;                                                  // unstuffed stream bytes per frame (16-byte multiple)
    size_t plane_off, stream_off, rec_off, meta_off, seg_off, total;   // byte offsets into the scratch; coefficients at 0
};

struct ChunkRec { uint32_t kept, rst, term, pad; };   // after the offsets kernel: kept and rst are exclusive prefix sums
struct FrameMeta { uint32_t kept, end, nseg, pad; };  // unstuffed bytes, file offset of the terminating marker, segments

// Where file f lies and how much of it may be read.
__device__ __forceinline__ const uint8_t* file_span(const Files& fl, int f, uint32_t* len) {
    size_t off = fl.offsets ? (size_t)fl.offsets[f] : (size_t)f * fl.stride;
    off = off < fl.bytes ? off : fl.bytes;
    size_t room = fl.bytes - off;
    if (!fl.offsets && room > fl.stride) room = fl.stride;
    if (room > fl.max_file) room = fl.max_file;
    const int32_t l = fl.lengths[f];
    *len = (uint32_t)(l <= 0 ? 0 : (size_t)l < room ? (size_t)l : room);
    return fl.base + off;
}

__device__ __forceinline__ uint32_t scan_start(const vlfm_jpeg_frame& fr, uint32_t len) {
    const int32_t s = fr.scan_offset;
    return s <= 0 ? 0u : (uint32_t)s < len ? (uint32_t)s : len;
}

__device__ __forceinline__ uint32_t segments(const vlfm_jpeg_frame& fr, int mcus, int max_seg) {
    const int ri = fr.restart_interval;
    const int ns = ri <= 0 ? 1 : (mcus + ri - 1) / ri;
    return (uint32_t)(ns < max_seg ? ns : max_seg);
}

// What byte i of the scan [scan0, len) of a file is: a byte that stays, one that goes (the zero behind a data 0xFF, the
// second byte of a marker, a fill 0xFF), the first byte of RSTn (its index to *idx), or the first byte of any other marker.
__device__ __forceinline__ int classify(const uint8_t* p, uint32_t scan0, uint32_t len, uint32_t i, int* idx) {
    const uint32_t b = p[i];
    if (b == 0xffu) {
        if (i + 1 >= len) return TERM;
        const uint32_t nx = p[i + 1];
        if (nx == 0) return KEEP;
        if (nx == 0xffu) return DROP;
        if ((nx & 0xf8u) == 0xd0u) {
            *idx = (int)(nx & 7u);
            return RST;
        }
        return TERM;
    }
    return (i > scan0 && p[i - 1] == 0xffu) ? DROP : KEEP;
}

// Exclusive sums of a and b over the 256 threads of the workgroup; the sums to *ta, *tb.  `part` holds 8 words.
__device__ __forceinline__ void block_exclusive_sum2(uint32_t a, uint32_t b, uint32_t* part, uint32_t* ea, uint32_t* eb,
                                                     uint32_t* ta, uint32_t* tb) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t ia = wave_inclusive_sum(a, lane), ib = wave_inclusive_sum(b, lane);
    __syncthreads();
    if (lane == 63) {
        part[wave] = ia;
        part[4 + wave] = ib;
    }
    __syncthreads();
    uint32_t ba = 0, bb = 0, sa = 0, sb = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t pa = part[w], pb = part[4 + w];
        ba += w < wave ? pa : 0;
        bb += w < wave ? pb : 0;
        sa += pa;
        sb += pb;
    }
    *ea = ba + ia - a;
    *eb = bb + ib - b;
    *ta = sa;
    *tb = sb;
}

// The kinds of the 16 bytes [i0, i0 + 16) of a file, 2 bits each (bytes outside [scan0, end) count as DROP), and the RSTn
// indices, 3 bits each.
__device__ __forceinline__ void kinds16(const uint8_t* p, uint32_t scan0, uint32_t len, uint32_t end, uint32_t i0,
                                        uint32_t* kinds, uint64_t* idxs) {
    uint32_t k = 0;
    uint64_t ix = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t i = i0 + j;
        int kind = DROP, idx = 0;
        if (i >= scan0 && i < end) kind = classify(p, scan0, len, i, &idx);
        k |= (uint32_t)kind << (2 * j);
        ix |= (uint64_t)idx << (3 * j);
    }
    *kinds = k;
    *idxs = ix;
}

__global__ void __launch_bounds__(256) jpeg_scan_count_kernel(Files fl, const vlfm_jpeg_frame* __restrict__ frames, int chunks,
                                                              ChunkRec* __restrict__ recs, int32_t* __restrict__ status) {
    __shared__ uint32_t part[8];
    __shared__ uint32_t term;
    const int f = blockIdx.x / chunks, c = blockIdx.x - f * chunks, t = threadIdx.x;
    uint32_t len;
    const uint8_t* p = file_span(fl, f, &len);
    const uint32_t scan0 = scan_start(frames[f], len);
    const uint32_t i0 = (uint32_t)c * DCHUNK + (uint32_t)t * 16;
    if (t == 0) term = NONE;
    __syncthreads();
    if (fl.header) {
        bool same = true;
        for (int j = 0; j < 16; ++j) {
            const uint32_t i = i0 + j;
            if (i < (uint32_t)fl.header_bytes) same = same && i < len && p[i] == fl.header[i];
        }
        if (!same) atomicMax(&status[f], (int32_t)VLFM_JPEG_BAD_HEADER);
    }
    uint32_t kinds;
    uint64_t idxs;
    kinds16(p, scan0, len, len, i0, &kinds, &idxs);
    uint32_t first = NONE;
#pragma unroll
    for (int j = 15; j >= 0; --j)
        if (((kinds >> (2 * j)) & 3u) == TERM) first = i0 + j;
    if (first != NONE) atomicMin(&term, first);
    __syncthreads();
    const uint32_t stop = term;
    uint32_t kept = 0, rst = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t kind = (kinds >> (2 * j)) & 3u;
        const bool live = i0 + j < stop;
        kept += (live && kind == KEEP) ? 1 : 0;
        rst += (live && kind == RST) ? 1 : 0;
    }
    uint32_t ek, er, tk, tr;
    block_exclusive_sum2(kept, rst, part, &ek, &er, &tk, &tr);
    if (t == 0) recs[(size_t)f * chunks + c] = ChunkRec{tk, tr, stop, 0};
}

__global__ void __launch_bounds__(256) jpeg_scan_offsets_kernel(Files fl, const vlfm_jpeg_frame* __restrict__ frames,
                                                                int chunks, int mcus, int max_seg,
                                                                ChunkRec* __restrict__ recs, FrameMeta* __restrict__ meta,
                                                                uint32_t* __restrict__ seg, int32_t* __restrict__ status) {
    __shared__ uint32_t part[8];
    __shared__ uint32_t cstar;
    const int f = blockIdx.x, t = threadIdx.x;
    ChunkRec* fr = recs + (size_t)f * chunks;
    uint32_t len;
    const uint8_t* p = file_span(fl, f, &len);
    const uint32_t scan0 = scan_start(frames[f], len);
    if (t == 0) cstar = NONE;
    __syncthreads();
    const int per = (chunks + 255) / 256;
    const int i0 = min(t * per, chunks), i1 = min(i0 + per, chunks);
    for (int i = i0; i < i1; ++i)
        if (fr[i].term != NONE) {
            atomicMin(&cstar, (uint32_t)i);
            break;
        }
    __syncthreads();
    const uint32_t last = cstar;                         // the chunk with the terminating marker, or NONE
    uint32_t sk = 0, sr = 0;
    for (int i = i0; i < i1; ++i)
        if ((uint32_t)i <= last) {
            sk += fr[i].kept;
            sr += fr[i].rst;
        }
    uint32_t ok, orr, tk, tr;
    block_exclusive_sum2(sk, sr, part, &ok, &orr, &tk, &tr);
    for (int i = i0; i < i1; ++i) {
        const uint32_t k = fr[i].kept, r = fr[i].rst;
        fr[i].kept = ok;
        fr[i].rst = orr;
        if ((uint32_t)i <= last) {
            ok += k;
            orr += r;
        }
    }
    // (a file that ends before its scan has no segments: nothing is decoded from it)
    const uint32_t nseg = len <= scan0 ? 0u : segments(frames[f], mcus, max_seg);
    const uint32_t end = last == NONE ? len : fr[last].term;   // (term is not rewritten above)
    uint32_t* fs = seg + (size_t)f * (max_seg + 1);
    for (uint32_t s = t; s <= nseg; s += 256) fs[s] = s == 0 ? 0 : tk;
    if (t == 0) {
        meta[f] = FrameMeta{tk, end, nseg, 0};
        int bad = 0;
        if (tr + 1 != nseg) bad = VLFM_JPEG_BAD_RESTART;
        if (last == NONE || end + 1 >= len || p[end + 1] != 0xd9) bad = VLFM_JPEG_BAD_EOI;
        if (len <= scan0) bad = VLFM_JPEG_BAD_LENGTH;
        if (bad) atomicMax(&status[f], (int32_t)bad);
    }
}

__global__ void __launch_bounds__(256) jpeg_unstuff_kernel(Files fl, const vlfm_jpeg_frame* __restrict__ frames, int chunks,
                                                           int max_seg, const ChunkRec* __restrict__ recs,
                                                           const FrameMeta* __restrict__ meta, uint8_t* __restrict__ ustream,
                                                           size_t ubytes, uint32_t* __restrict__ seg,
                                                           int32_t* __restrict__ status) {
    __shared__ uint32_t part[8];
    const int f = blockIdx.x / chunks, c = blockIdx.x - f * chunks, t = threadIdx.x;
    const FrameMeta fm = meta[f];
    if ((uint32_t)c * DCHUNK >= fm.end) return;
    uint32_t len;
    const uint8_t* p = file_span(fl, f, &len);
    const uint32_t scan0 = scan_start(frames[f], len);
    const uint32_t i0 = (uint32_t)c * DCHUNK + (uint32_t)t * 16;
    uint32_t kinds;
    uint64_t idxs;
    kinds16(p, scan0, len, min(fm.end, len), i0, &kinds, &idxs);
    uint32_t kept = 0, rst = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t kind = (kinds >> (2 * j)) & 3u;
        kept += kind == KEEP ? 1 : 0;
        rst += kind == RST ? 1 : 0;
    }
    uint32_t ek, er, tk, tr;
    block_exclusive_sum2(kept, rst, part, &ek, &er, &tk, &tr);
    const ChunkRec rec = recs[(size_t)f * chunks + c];
    uint32_t pos = rec.kept + ek, j_rst = rec.rst + er;
    uint8_t* us = ustream + (size_t)f * ubytes;
    uint32_t* fs = seg + (size_t)f * (max_seg + 1);
    bool order = true;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t kind = (kinds >> (2 * j)) & 3u;
        if (kind == KEEP) {
            if (pos < ubytes) us[pos] = p[i0 + j];
            ++pos;
        } else if (kind == RST) {
            order = order && (uint32_t)((idxs >> (3 * j)) & 7u) == (j_rst & 7u);
            if (j_rst + 1 < fm.nseg) fs[j_rst + 1] = pos;
            ++j_rst;
        }
    }
    if (!order) atomicMax(&status[f], (int32_t)VLFM_JPEG_BAD_RESTART);
}

// The token that starts at a lane's bit position under table h, from the 32 stream bits `peek` behind that position:
// value (16 bits, signed) | run << 16 | size << 20 | total bit length << 24 | no-such-code << 30.
__device__ __forceinline__ uint32_t candidate(const vlfm_jpeg_huff& h, uint32_t peek) {
    const uint32_t x = peek >> 16;
    int len = 1;
#pragma unroll
    for (int l = 0; l < 16; ++l) len += x >= h.limit[l] ? 1 : 0;
    const uint32_t bad = len > 16 ? 1u : 0u;
    const int lc = len > 16 ? 16 : len;
    int idx = (int)(x >> (16 - lc)) - h.delta[lc - 1];
    idx = idx < 0 ? 0 : idx > 255 ? 255 : idx;
    const uint32_t sym = h.vals[idx];
    const int size = (int)(sym & 15u);
    int val = 0;
    if (size) {
        const int amp = (int)((peek << lc) >> (32 - size));                 // lc + size <= 31
        val = (amp >> (size - 1)) ? amp : amp - (1 << size) + 1;           // jdhuff.h HUFF_EXTEND
    }
    return ((uint32_t)val & 0xffffu) | (sym >> 4) << 16 | (uint32_t)size << 20 | (uint32_t)(lc + size) << 24 | bad << 30;
}

__global__ void __launch_bounds__(64) jpeg_huffman_kernel(const vlfm_jpeg_frame* __restrict__ frames,
                                                          const vlfm_jpeg_table_set* __restrict__ sets, int n_sets, int mcus,
                                                          int max_seg, const FrameMeta* __restrict__ meta,
                                                          const uint32_t* __restrict__ seg,
                                                          const uint8_t* __restrict__ ustream, size_t ubytes,
                                                          int16_t* __restrict__ coef, int32_t* __restrict__ status) {
    __shared__ vlfm_jpeg_huff tab[6];                      // DC of Y, Cb, Cr; AC of Y, Cb, Cr
    __shared__ uint32_t stage[STAGE_BYTES / 4 + 4];
    const int lane = threadIdx.x;
    const int f = blockIdx.x / max_seg, s = blockIdx.x - f * max_seg;
    const vlfm_jpeg_frame fr = frames[f];
    const FrameMeta fm = meta[f];
    if ((uint32_t)s >= fm.nseg) return;
    const int ri = fr.restart_interval <= 0 ? mcus : fr.restart_interval;
    const long long first = (long long)s * ri;
    if (first >= mcus) return;
    const int mcu0 = (int)first, mcu1 = (int)min((long long)mcus, first + ri);

    {   // the frame's tables, 16 bytes per lane and step
        const int set = min(max(fr.table_set, 0), n_sets - 1);
        const uint4* src = reinterpret_cast<const uint4*>(sets[set].dc);
        uint4* dst = reinterpret_cast<uint4*>(tab);
        for (int i = lane; i < (int)(6 * sizeof(vlfm_jpeg_huff) / 16); i += 64) dst[i] = src[i];
        if (lane < 4) stage[STAGE_BYTES / 4 + lane] = 0;
    }
    {   // every block of the segment starts as zeros
        uint4* z = reinterpret_cast<uint4*>(coef + ((size_t)f * mcus + mcu0) * 384);
        const size_t nz = (size_t)(mcu1 - mcu0) * 48;
        for (size_t i = lane; i < nz; i += 64) z[i] = make_uint4(0, 0, 0, 0);
    }
    __threadfence();
    __syncthreads();

    const uint32_t kept = fm.kept < ubytes ? fm.kept : (uint32_t)ubytes;
    const uint32_t* fs = seg + (size_t)f * (max_seg + 1);
    const uint32_t b0 = min(fs[s], kept), b1 = max(min(fs[s + 1], kept), b0);   // the segment's unstuffed bytes
    const uint32_t seg_bits = (b1 - b0) * 8;
    const uint8_t* us = ustream + (size_t)f * ubytes;
    int16_t* cf = coef + (size_t)f * mcus * 384;

    uint32_t pos = 0;                                      // bit position in the segment
    int mcu = mcu0, blk = 0, k = 0, err = 0;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    uint32_t stage_base = NONE;
    while (mcu < mcu1 && err == 0) {
        const uint32_t need_hi = b0 + ((pos + 63) >> 3) + 8;
        if (stage_base == NONE || need_hi > stage_base + STAGE_BYTES) {   // every byte a lane looks at is a staged one
            __syncthreads();
            stage_base = (b0 + (pos >> 3)) & ~15u;
            const size_t at = (size_t)stage_base + 16 * (size_t)lane;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (at + 16 <= ubytes) v = *reinterpret_cast<const uint4*>(us + at);
            reinterpret_cast<uint4*>(stage)[lane] = v;
            __syncthreads();
        }
        const uint32_t p = pos + (uint32_t)lane;
        const uint32_t bi = b0 + (p >> 3) - stage_base;   // bi + 8 <= STAGE_BYTES: the two words below lie in `stage`
        const uint32_t w0 = stage[bi >> 2], w1 = stage[(bi >> 2) + 1];
        const uint64_t v64 = (uint64_t)__builtin_bswap32(w0) << 32 | __builtin_bswap32(w1);
        const uint32_t peek = (uint32_t)((v64 << (8 * (bi & 3u) + (p & 7u))) >> 32);
        const uint32_t cd0 = candidate(tab[0], peek), cd1 = candidate(tab[1], peek), cd2 = candidate(tab[2], peek);
        const uint32_t ca0 = candidate(tab[3], peek), ca1 = candidate(tab[4], peek), ca2 = candidate(tab[5], peek);

        int off = 0, my_at = -1, my_val = 0;
        while (off < 64) {
            const int comp = blk < 4 ? 0 : blk - 3;
            const uint32_t cand = k == 0 ? (comp == 0 ? cd0 : comp == 1 ? cd1 : cd2) : (comp == 0 ? ca0 : comp == 1 ? ca1 : ca2);
            const uint32_t r = (uint32_t)__builtin_amdgcn_readlane((int)cand, __builtin_amdgcn_readfirstlane(off));
            const int tl = (int)((r >> 24) & 63u), size = (int)((r >> 20) & 15u), run = (int)((r >> 16) & 15u);
            const int val = (int)(int16_t)(r & 0xffffu);
            if (r >> 30 & 1u) { err = VLFM_JPEG_BAD_CODE; break; }
            if (pos + (uint32_t)off + (uint32_t)tl > seg_bits) { err = VLFM_JPEG_BAD_BITS; break; }
            bool end_block = false;
            int at = -1, v = 0;
            if (k == 0) {
                if (size > 11) { err = VLFM_JPEG_BAD_SIZE; break; }
                if (comp == 0) v = pred0 += val;
                else if (comp == 1) v = pred1 += val;
                else v = pred2 += val;
                at = (mcu * 6 + blk) * 64;
                k = 1;
            } else if (size == 0) {
                if (run == 15) {                            // ZRL
                    k += 16;
                    end_block = k >= 64;
                } else {
                    end_block = true;                       // EOB
                }
            } else {
                if (size > 10) { err = VLFM_JPEG_BAD_SIZE; break; }
                k += run;
                if (k > 63) { err = VLFM_JPEG_BAD_INDEX; break; }
                at = (mcu * 6 + blk) * 64 + k;
                v = val;
                end_block = ++k >= 64;
            }
            if (at >= 0 && lane == off) {
                my_at = at;
                my_val = v;
            }
            off += tl;
            if (end_block) {
                k = 0;
                if (++blk == 6) {
                    blk = 0;
                    if (++mcu == mcu1) break;
                }
            }
        }
        // (mcu0 <= mcu < mcu1, blk < 6, k < 64 at every mark: the index lies in the segment's own blocks)
        if (my_at >= mcu0 * 384 && my_at < mcu1 * 384) cf[my_at] = (int16_t)my_val;
        pos += (uint32_t)off;
    }
    if (err && lane == 0) atomicMax(&status[f], (int32_t)err);
}

}  // namespace jpeg
}  // namespace vlfm

// ================================================================================================ host side, C ABI
using namespace vlfm;
using namespace vlfm::jpeg;

namespace {
enum {
    R_NOT_JPEG = 1, R_MALFORMED, R_PROCESS, R_PRECISION, R_COMPONENTS, R_SAMPLING, R_SCAN, R_QUANT16, R_NO_TABLE, R_ADOBE,
    R_DIMENSION, R_NO_SCAN, R_COUNT
};
const char* const kReasons[R_COUNT] = {
    "ok",
    "not a JPEG file (no SOI marker)",
    "malformed marker segment",
    "not a baseline sequential frame (progressive, extended, lossless, arithmetic or hierarchical)",
    "samples are not 8-bit",
    "not three components",
    "sampling factors are not 2x2, 1x1, 1x1 (4:2:0)",
    "not one interleaved scan of all three components with Ss = 0, Se = 63, Ah = Al = 0 (or a DNL segment)",
    "16-bit quantisation table",
    "a component selects a table that no segment defines",
    "Adobe APP14 segment",
    "a frame dimension is zero",
    "no frame header and scan in front of the end of the data"};

// jdhuff.c jpeg_make_d_derived_tbl, in the compare form: codes of each length in increasing order, as the symbols are listed.
bool derive(const uint8_t* bits, const uint8_t* vals, int count, vlfm_jpeg_huff* h) {
    memset(h, 0, sizeof *h);
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        h->delta[l - 1] = (int32_t)code - k;
        code += bits[l - 1];
        k += bits[l - 1];
        if (code > (1u << l)) return false;
        h->limit[l - 1] = code << (16 - l);
        code <<= 1;
    }
    if (k != count || k > 256) return false;
    memcpy(h->vals, vals, (size_t)k);
    return true;
}

bool layout(int n, int H, int W, size_t max_file_bytes, DecLayout* l) {
    Geometry g;
    if (!geometry(n, H, W, &g) || max_file_bytes == 0 || max_file_bytes > 0x7fffffffu) return false;
    const size_t mcus = g.mcus();
    l->n = n;
    l->mcus = (int)mcus;
    l->chunks = (int)((max_file_bytes + DCHUNK - 1) / DCHUNK);
    l->ubytes = align16(max_file_bytes) + 32;
    l->plane_off = align16((size_t)n * mcus * 768);
    l->stream_off = l->plane_off + align16((size_t)n * mcus * 384);
    l->rec_off = l->stream_off + (size_t)n * l->ubytes;
    l->meta_off = l->rec_off + (size_t)n * l->chunks * sizeof(ChunkRec);
    l->seg_off = l->meta_off + (size_t)n * sizeof(FrameMeta);
    l->total = l->seg_off + align16((size_t)n * (mcus + 1) * 4);
    return true;
}
}  // namespace

extern "C" const char* vlfm_jpeg_parse_reason(int code) {
    return code >= 0 && code < R_COUNT ? kReasons[code] : "unknown reason";
}

extern "C" size_t vlfm_jpeg_decode_chunk_bytes(void) { return DCHUNK; }

extern "C" int vlfm_jpeg_parse_host(const uint8_t* p, size_t len, vlfm_jpeg_frame* frame, vlfm_jpeg_table_set* set) {
    if (!p || !frame || !set) return fail(VLFM_ERR_INVALID, "jpeg_parse_host: bad argument");
    memset(frame, 0, sizeof *frame);
    memset(set, 0, sizeof *set);
    if (len < 4 || p[0] != 0xff || p[1] != 0xd8) return R_NOT_JPEG;
    uint16_t quant[4][64];
    bool have_q[4] = {false, false, false, false}, have_h[2][4] = {};
    static thread_local vlfm_jpeg_huff huff[2][4];
    int comp_id[3] = {0, 0, 0}, comp_q[3] = {0, 0, 0};
    bool sof = false;
    size_t i = 2;
    for (;;) {
        if (i + 1 >= len || p[i] != 0xff) return i + 1 >= len ? R_NO_SCAN : R_MALFORMED;
        while (i + 1 < len && p[i + 1] == 0xff) ++i;      // fill bytes
        if (i + 1 >= len) return R_NO_SCAN;
        const int m = p[i + 1];
        i += 2;
        if (m == 0xd9) return R_NO_SCAN;
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd8)) return R_MALFORMED;   // markers without a segment have no place here
        if (i + 2 > len) return R_NO_SCAN;
        const size_t sl = (size_t)p[i] << 8 | p[i + 1];
        if (sl < 2 || i + sl > len) return i + sl > len && sl >= 2 ? R_NO_SCAN : R_MALFORMED;
        const uint8_t* s = p + i + 2;
        const size_t n = sl - 2;
        if (m == 0xc0) {
            if (sof) return R_PROCESS;                    // a second frame: hierarchical
            if (n < 6) return R_MALFORMED;
            if (s[0] != 8) return R_PRECISION;
            frame->height = s[1] << 8 | s[2];
            frame->width = s[3] << 8 | s[4];
            if (frame->height == 0 || frame->width == 0) return R_DIMENSION;
            if (s[5] != 3) return R_COMPONENTS;
            if (n != 15) return R_MALFORMED;
            for (int c = 0; c < 3; ++c) {
                comp_id[c] = s[6 + 3 * c];
                if (s[7 + 3 * c] != (c == 0 ? 0x22 : 0x11)) return R_SAMPLING;
                comp_q[c] = s[8 + 3 * c];
                if (comp_q[c] > 3) return R_MALFORMED;
            }
            sof = true;
        } else if ((m >= 0xc1 && m <= 0xcf && m != 0xc4) || m == 0xde || m == 0xdf) {
            return R_PROCESS;                             // other SOFn, JPG, DAC (0xcc), DHP, EXP
        } else if (m == 0xdc) {
            return R_SCAN;                                // DNL
        } else if (m == 0xdb) {
            size_t j = 0;
            while (j < n) {
                const int pq = s[j] >> 4, tq = s[j] & 15;
                if (pq > 1 || tq > 3) return R_MALFORMED;
                if (pq == 1) return R_QUANT16;
                if (j + 65 > n) return R_MALFORMED;
                for (int z = 0; z < 64; ++z) quant[tq][kNaturalOrder[z]] = s[j + 1 + z];
                have_q[tq] = true;
                j += 65;
            }
        } else if (m == 0xc4) {
            size_t j = 0;
            while (j < n) {
                if (j + 17 > n) return R_MALFORMED;
                const int tc = s[j] >> 4, th = s[j] & 15;
                if (tc > 1 || th > 3) return R_MALFORMED;
                int count = 0;
                for (int l = 0; l < 16; ++l) count += s[j + 1 + l];
                if (count > 256 || j + 17 + (size_t)count > n) return R_MALFORMED;
                if (!derive(s + j + 1, s + j + 17, count, &huff[tc][th])) return R_MALFORMED;
                have_h[tc][th] = true;
                j += 17 + (size_t)count;
            }
        } else if (m == 0xdd) {
            if (n != 2) return R_MALFORMED;
            frame->restart_interval = s[0] << 8 | s[1];
        } else if (m == 0xee) {
            if (n >= 5 && memcmp(s, "Adobe", 5) == 0) return R_ADOBE;
        } else if (m == 0xda) {
            if (!sof) return R_NO_SCAN;
            if (n < 1) return R_MALFORMED;
            if (s[0] != 3) return R_SCAN;
            if (n != 10) return R_MALFORMED;
            for (int c = 0; c < 3; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) return R_SCAN;   // (interleaved scans list components in frame order)
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) return R_MALFORMED;
                if (!have_q[comp_q[c]] || !have_h[0][td] || !have_h[1][ta]) return R_NO_TABLE;
                memcpy(set->quant[c], quant[comp_q[c]], sizeof quant[0]);
                set->dc[c] = huff[0][td];
                set->ac[c] = huff[1][ta];
            }
            if (s[7] != 0 || s[8] != 63 || s[9] != 0) return R_SCAN;
            for (int c = 0; c < 3; ++c)
                for (int z = 0; z < 64; ++z)
                    if (set->quant[c][z] == 0) return R_MALFORMED;
            frame->scan_offset = (int32_t)(i + sl);
            return VLFM_OK;
        }
        // APPn, COM and anything else with a length: skipped
        i += sl;
    }
}

extern "C" size_t vlfm_jpeg_decode_scratch_bytes(int n, int H, int W, size_t max_file_bytes) {
    DecLayout l;
    return layout(n, H, W, max_file_bytes, &l) ? l.total : 0;
}

extern "C" int vlfm_jpeg_decode_batched(const uint8_t* d_files, size_t files_bytes, const int64_t* d_offsets, size_t stride,
                                        const int32_t* d_lengths, int n, int H, int W, const vlfm_jpeg_frame* d_frames,
                                        const vlfm_jpeg_table_set* d_sets, int n_sets, const uint8_t* d_header,
                                        int header_bytes, int max_segments, size_t max_file_bytes, int rgb_order,
                                        uint8_t* d_out, int32_t* d_status, void* d_scratch, size_t scratch_bytes,
                                        void* stream) {
    DecLayout l;
    if (!d_files || !d_lengths || !d_frames || !d_sets || !d_out || !d_status || n_sets <= 0 || files_bytes == 0 ||
        (rgb_order != 0 && rgb_order != 1) || (!d_offsets && stride == 0) ||
        (d_header && (header_bytes <= 0 || (size_t)header_bytes > max_file_bytes)))
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: bad argument");
    if (!layout(n, H, W, max_file_bytes, &l))
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: bad frame size or file size");
    if (max_segments < 1 || max_segments > l.mcus)
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: max_segments must be 1 .. the MCU count");
    if ((size_t)l.mcus * 384 > 0x7fffffff)
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: frame too large for 32-bit coefficient indices");
    if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 15))
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: scratch must be a 16-byte aligned device buffer");
    if ((reinterpret_cast<uintptr_t>(d_sets) & 15))
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: the table sets must be 16-byte aligned");
    if (scratch_bytes < l.total) return fail(VLFM_ERR_CAPACITY, "jpeg_decode_batched: scratch too small");
    const size_t scan_grid = (size_t)n * l.chunks, huff_grid = (size_t)n * max_segments;
    if (scan_grid > 0x7fffffff || huff_grid > 0x7fffffff)
        return fail(VLFM_ERR_INVALID, "jpeg_decode_batched: batch too large for one launch");
    l.max_seg = max_segments;

    uint8_t* base = static_cast<uint8_t*>(d_scratch);
    int16_t* coef = reinterpret_cast<int16_t*>(base);
    uint8_t* planes = base + l.plane_off;
    uint8_t* ustream = base + l.stream_off;
    ChunkRec* recs = reinterpret_cast<ChunkRec*>(base + l.rec_off);
    FrameMeta* meta = reinterpret_cast<FrameMeta*>(base + l.meta_off);
    uint32_t* seg = reinterpret_cast<uint32_t*>(base + l.seg_off);
    hipStream_t st = (hipStream_t)stream;
    Files fl{d_files, files_bytes, d_offsets, stride, d_lengths, max_file_bytes, d_header, d_header ? header_bytes : 0};

    if (hipMemsetAsync(d_status, 0, (size_t)n * 4, st) != hipSuccess)
        return fail(VLFM_ERR_HIP, "jpeg_decode_batched: clearing the status words failed");
    {
        VLFM_TIMED("jpeg_scan_count_kernel", st);
        VLFM_KLAUNCH(jpeg_scan_count_kernel, dim3((unsigned)scan_grid), dim3(256), 0, st, fl, d_frames, l.chunks, recs,
                     d_status);
    }
    if (int rc = check_launch("jpeg_scan_count_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_scan_offsets_kernel", st);
        VLFM_KLAUNCH(jpeg_scan_offsets_kernel, dim3((unsigned)n), dim3(256), 0, st, fl, d_frames, l.chunks, l.mcus, l.max_seg,
                     recs, meta, seg, d_status);
    }
    if (int rc = check_launch("jpeg_scan_offsets_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_unstuff_kernel", st);
        VLFM_KLAUNCH(jpeg_unstuff_kernel, dim3((unsigned)scan_grid), dim3(256), 0, st, fl, d_frames, l.chunks, l.max_seg, recs,
                     meta, ustream, l.ubytes, seg, d_status);
    }
    if (int rc = check_launch("jpeg_unstuff_kernel")) return rc;
    {
        VLFM_TIMED("jpeg_huffman_kernel", st);
        VLFM_KLAUNCH(jpeg_huffman_kernel, dim3((unsigned)huff_grid), dim3(64), 0, st, d_frames, d_sets, n_sets, l.mcus,
                     l.max_seg, meta, seg, ustream, l.ubytes, coef, d_status);
    }
    if (int rc = check_launch("jpeg_huffman_kernel")) return rc;
    return launch_pixels(coef, d_frames, d_sets, n_sets, n, H, W, rgb_order, planes, d_out, st);
}
