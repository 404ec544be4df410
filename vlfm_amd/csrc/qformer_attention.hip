// qformer_attention.hip -- the Q-Former's cross-attention in f32: softmax(q K^T * scale) V for at most 32 queries against the at
// most 257 image tokens of one image, head width 64 (reference: the BertSelfAttention of LAVIS' Qformer.py behind
// vlfm/vlm/blip2itm.py:52, cross-attention branch; every operand f32 as LAVIS keeps the Q-Former).
//
// K and V come from the block-major result of the pair GEMM (gemm_f16.hip, EPI_PAIR_F32): block `blk` is [M_total][64] f32, so
// one (image, head) is T x 256 B CONTIGUOUS -- the kernel streams 2 x 65.8 KB per item once and is bound by that stream; the
// arithmetic (6.5 GFLOP per layer at 256 images) runs on v_mfma_f32_32x32x2_f32 under it.  No f16 anywhere.
//
// One workgroup (4 wavefronts) per (image, head) item, persistent: workgroup w walks items w, w + grid, ...; item -> XCD item & 7,
// image (item >> 3) / heads * 8 + XCD: the heads of an image (which share its 32 query rows) meet in one L2.
//   * Keys are split over the wavefronts in tiles of 32: wavefront v owns tiles v, v + 4, ... of K AND of V and is the only one
//     that loads or reads them (LDS-DMA, 16 B per lane, wavefront-private rows: no workgroup barrier guards an operand).  The
//     T % 32 keys behind the last full tile (ONE at T = 257) go to the next wavefront in turn and run on the vector ALU.
//   * As in sam_ops.hip's window attention, S^T = K Q^T with the keys as the M index: a lane then holds, for ONE query (lane & 31),
//     the scores of 16 keys of the tile -- the online softmax is lane-local plus one exchange with lane ^ 32 -- and the
//     probabilities are already the B operand of O^T = V^T P^T.  The MFMA's two k-slots are the two halves of the head:
//     lane half g multiplies dims [32 g, 32 g + 32), read as eight ds_read_b128.
//   * Bank conflicts: the 16-byte chunk a lane FETCHES is permuted within its row (the DMA lands linearly).  K: chunk ^ (row & 15)
//     -- 16 rows' reads of one chunk index hit 16 different chunks.  V: chunk ^ 8 for rows with bit 2 set -- the two rows (key,
//     key + 4) the two lane halves read in one PV step lie in different halves of the banks.
//   * A tile of the NEXT item is requested as soon as the wavefront has consumed the same tile of this one (its reads retired:
//     lgkmcnt(0)) -- K behind the fragment reads, in front of the score MFMAs; V behind the P V MFMAs --, so the next item streams in
//     under the current item's arithmetic; one vmcnt(0) per item.
//   * The partial (m, l, O) of wavefronts 1-3 go through 26 KB of LDS to wavefront 0 (same lane layout: the merge is lane-local),
//     which normalises and stores 16 B per lane.  Two barriers per item: partials written / partials read.
// LDS at T = 257: 2 x 260 rows x 256 B + 26 112 B = 159 232 B.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vlfm_amd.h"
#include "mfma.h"
#include "profile.h"
#include "status.h"

namespace vlfm {

constexpr int QA_ROWB = 256;                       // one key / value row of a head: 64 f32
constexpr int QA_MERGE_REGS = 34;                  // 32 output registers + m + l
constexpr int QA_MERGE = 3 * QA_MERGE_REGS * 64 * 4;
constexpr int QA_MAX_T = 257, QA_MAX_Q = 32;

struct QaArgs {
    const float* q;      // [B][Q][heads * 64]
    const float* kv;     // [blocks][M_total][64]
    float* out;          // [B][Q][heads * 64]
    int B, T, Q, heads, k_block0, v_block0, M_total;
    int rows_pad;        // T rounded up to the 4 rows of one DMA instruction
    float scale_log2e;
};

struct QaKernel {
    const QaArgs& a;
    unsigned char* smem;
    lds_ptr lds;
    int lane, wave, col, g, voff;

    __device__ QaKernel(const QaArgs& a_, unsigned char* smem_) : a(a_), smem(smem_), lds((lds_ptr)smem_) {
        lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        col = lane & 31;
        g = lane >> 5;
        voff = a.rows_pad * QA_ROWB;
    }
    __device__ inline const unsigned char* block(int block0, int b, int h) const {
        return reinterpret_cast<const unsigned char*>(a.kv + ((size_t)(block0 + h) * (size_t)a.M_total + (size_t)b * (size_t)a.T) * 64);
    }
    // rows [row0, row0 + 4 n_ins) of K (V: voff behind them) of an item -> LDS, rows beyond T re-read row T - 1 (never used)
    __device__ inline void issue_k(const unsigned char* kg, int row0, int n_ins) const {
        const int r4 = lane >> 4, p = lane & 15;
        for (int ins = 0; ins < n_ins; ins++) {
            const int row = row0 + 4 * ins + r4, src_row = min(row, a.T - 1);
            const int dst = __builtin_amdgcn_readfirstlane((row0 + 4 * ins) * QA_ROWB);
            __builtin_amdgcn_global_load_lds((gbl_ptr)(kg + (size_t)src_row * QA_ROWB + ((p ^ (row & 15)) << 4)), lds + dst, 16, 0, 0);
        }
    }
    __device__ inline void issue_v(const unsigned char* vg, int row0, int n_ins) const {
        const int r4 = lane >> 4, p = lane & 15;
        for (int ins = 0; ins < n_ins; ins++) {
            const int row = row0 + 4 * ins + r4, src_row = min(row, a.T - 1);
            const int dst = __builtin_amdgcn_readfirstlane(voff + (row0 + 4 * ins) * QA_ROWB);
            __builtin_amdgcn_global_load_lds((gbl_ptr)(vg + (size_t)src_row * QA_ROWB + ((p ^ (((row >> 2) & 1) << 3)) << 4)),
                                             lds + dst, 16, 0, 0);
        }
    }
    __device__ inline void issue_rows(const unsigned char* kg, const unsigned char* vg, int row0, int n_ins) const {
        issue_k(kg, row0, n_ins);
        issue_v(vg, row0, n_ins);
    }
    // this lane's half of its query row: dims [32 g, 32 g + 32) of query min(col, Q - 1)
    __device__ inline void load_q(int b, int h, float (&qn)[32]) const {
        const float* src = a.q + ((size_t)b * a.Q + min(col, a.Q - 1)) * ((size_t)a.heads * 64) + (size_t)h * 64 + 32 * g;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const floatx4 v = *reinterpret_cast<const floatx4*>(src + 4 * c);
            qn[4 * c] = v[0]; qn[4 * c + 1] = v[1]; qn[4 * c + 2] = v[2]; qn[4 * c + 3] = v[3];
        }
    }
};

__device__ __forceinline__ void qa_item(int w, int heads, int& b, int& h) {
    const int xcd = w & 7, idx = w >> 3;
    b = (idx / heads) * 8 + xcd;
    h = idx % heads;
}

__global__ __launch_bounds__(256) void qformer_cross_attention_kernel(QaArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    QaKernel k(a, smem);
    const int lane = k.lane, wave = k.wave, col = k.col, g = k.g;
    const int n_full = a.T >> 5, n_left = a.T & 31, left_wave = n_full & 3, left_ins = (n_left + 3) >> 2;
    const int stride = gridDim.x;     // a multiple of 8: a workgroup stays on its XCD's items
    const int moff = 2 * k.voff;
    int w = blockIdx.x, b, h;
    qa_item(w, a.heads, b, h);
    if (b >= a.B) return;             // (images of an XCD ascend with the item: nothing behind it either)

    float qn[32];
    k.load_q(b, h, qn);
    {
        const unsigned char* kg = k.block(a.k_block0, b, h);
        const unsigned char* vg = k.block(a.v_block0, b, h);
        for (int t = wave; t < n_full; t += 4) k.issue_rows(kg, vg, 32 * t, 8);
        if (n_left != 0 && wave == left_wave) k.issue_rows(kg, vg, 32 * n_full, left_ins);
    }
    for (;;) {
        wait_vmcnt<0>();       // this wavefront's tiles of the item and its query row
        asm volatile("" ::: "memory");
        float qf[32];
#pragma unroll
        for (int s = 0; s < 32; s++) qf[s] = qn[s];
        const int nw = w + stride;
        int nb, nh;
        qa_item(nw, a.heads, nb, nh);
        const bool more = nb < a.B;
        const unsigned char* kg = k.block(a.k_block0, more ? nb : b, more ? nh : h);
        const unsigned char* vg = k.block(a.v_block0, more ? nb : b, more ? nh : h);
        if (more) k.load_q(nb, nh, qn);

        float m = -INFINITY, l = 0.f;
        floatx16 o0, o1;
#pragma unroll
        for (int r = 0; r < 16; r++) { o0[r] = 0.f; o1[r] = 0.f; }
        for (int t = wave; t < n_full; t += 4) {
            // ---- S^T tile: 32 keys x 32 queries, K = 64 as 32 steps of 2
            const unsigned char* kb = smem + (32 * t + col) * QA_ROWB;
            float kf[32];
#pragma unroll
            for (int c = 0; c < 8; c++) {
                const floatx4 v = *reinterpret_cast<const floatx4*>(kb + (((8 * g + c) ^ (col & 15)) << 4));
                kf[4 * c] = v[0]; kf[4 * c + 1] = v[1]; kf[4 * c + 2] = v[2]; kf[4 * c + 3] = v[3];
            }
            // the K rows are in registers: the same tile of the next item's K takes their place while this one is multiplied
            wait_lgkmcnt0();
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" ::: "memory");
            if (more) k.issue_k(kg, 32 * t, 8);
            floatx16 acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 32; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[s], qf[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] *= a.scale_log2e;
            float tm = acc[0];
#pragma unroll
            for (int r = 1; r < 16; r++) tm = fmaxf(tm, acc[r]);
            tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
            const float mn = fmaxf(m, tm);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);      // first tile: exp2(-inf) = 0
            m = mn;
            l *= alpha;
#pragma unroll
            for (int r = 0; r < 16; r++) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
            for (int r = 0; r < 16; r++) { const float pj = __builtin_amdgcn_exp2f(acc[r] - mn); l += pj; acc[r] = pj; }
            // ---- O^T += V^T P^T: accumulator register r of lane half g is key 32 t + (r & 3) + 8 (r >> 2) + 4 g (bit 2 of the row = g)
            const float* vb = reinterpret_cast<const float*>(smem + k.voff + (32 * t + 4 * g) * QA_ROWB);
            const int c0 = (((col >> 2) ^ (8 * g)) << 2) + (col & 3), c1 = (((8 + (col >> 2)) ^ (8 * g)) << 2) + (col & 3);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int ro = ((r & 3) + 8 * (r >> 2)) * 64;
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb[ro + c0], acc[r], o0, 0, 0, 0);
                o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vb[ro + c1], acc[r], o1, 0, 0, 0);
            }
            // ... and so are the V rows now
            wait_lgkmcnt0();
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" ::: "memory");
            if (more) k.issue_v(vg, 32 * t, 8);
        }
        if (n_left != 0 && wave == left_wave) {
            // ---- the keys behind the last full tile, one at a time on the vector ALU (every lane half sums its 32 dims)
            for (int j = 32 * n_full; j < a.T; j++) {
                const unsigned char* kr = smem + j * QA_ROWB;
                float part = 0.f;
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    const floatx4 v = *reinterpret_cast<const floatx4*>(kr + (((8 * g + c) ^ (j & 15)) << 4));
#pragma unroll
                    for (int e = 0; e < 4; e++) part = fmaf(v[e], qf[4 * c + e], part);
                }
                const float s = (part + __shfl_xor(part, 32, 64)) * a.scale_log2e;
                const float mn = fmaxf(m, s);
                const float alpha = __builtin_amdgcn_exp2f(m - mn), pj = __builtin_amdgcn_exp2f(s - mn);
                m = mn;
                l = l * alpha + (g == 0 ? pj : 0.f);     // (l is a per-half partial sum: the two halves are added below)
                const unsigned char* vr = smem + k.voff + j * QA_ROWB;
                const int sw = ((j >> 2) & 1) << 3;
#pragma unroll
                for (int q4 = 0; q4 < 4; q4++) {
                    const floatx4 v0 = *reinterpret_cast<const floatx4*>(vr + (((2 * q4 + g) ^ sw) << 4));
                    const floatx4 v1 = *reinterpret_cast<const floatx4*>(vr + (((8 + 2 * q4 + g) ^ sw) << 4));
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        o0[4 * q4 + e] = fmaf(pj, v0[e], o0[4 * q4 + e] * alpha);
                        o1[4 * q4 + e] = fmaf(pj, v1[e], o1[4 * q4 + e] * alpha);
                    }
                }
            }
            wait_lgkmcnt0();
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" ::: "memory");
            if (more) k.issue_rows(kg, vg, 32 * n_full, left_ins);
        }
        l += __shfl_xor(l, 32, 64);

        // ---- partials of wavefronts 1-3 -> wavefront 0 ([wavefront][register][lane]: conflict-free both ways)
        float* sc = reinterpret_cast<float*>(smem + moff);
        if (wave != 0) {
            float* mine = sc + (wave - 1) * QA_MERGE_REGS * 64 + lane;
#pragma unroll
            for (int r = 0; r < 16; r++) { mine[r * 64] = o0[r]; mine[(16 + r) * 64] = o1[r]; }
            mine[32 * 64] = m;
            mine[33 * 64] = l;
            wait_lgkmcnt0();
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (wave == 0) {
            // (wavefront 0 always owns a key -- tile 0, or the only keys when T < 32 -- so its m is finite)
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const float* src = sc + v * QA_MERGE_REGS * 64 + lane;
                const float m2 = src[32 * 64], l2 = src[33 * 64];
                const float mn = fmaxf(m, m2);
                const float a1 = __builtin_amdgcn_exp2f(m - mn), a2 = __builtin_amdgcn_exp2f(m2 - mn);
                m = mn;
                l = l * a1 + l2 * a2;
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    o0[r] = o0[r] * a1 + src[r * 64] * a2;
                    o1[r] = o1[r] * a1 + src[(16 + r) * 64] * a2;
                }
            }
            if (col < a.Q) {
                const float inv = 1.0f / l;
                // o0[r] / o1[r] = channel (r & 3) + 8 (r >> 2) + 4 g (+ 32) of query col
                float* orow = a.out + ((size_t)b * a.Q + col) * ((size_t)a.heads * 64) + (size_t)h * 64 + 4 * g;
#pragma unroll
                for (int q4 = 0; q4 < 4; q4++) {
                    const floatx4 s0 = {o0[4 * q4] * inv, o0[4 * q4 + 1] * inv, o0[4 * q4 + 2] * inv, o0[4 * q4 + 3] * inv};
                    const floatx4 s1 = {o1[4 * q4] * inv, o1[4 * q4 + 1] * inv, o1[4 * q4 + 2] * inv, o1[4 * q4 + 3] * inv};
                    *reinterpret_cast<floatx4*>(orow + 8 * q4) = s0;
                    *reinterpret_cast<floatx4*>(orow + 32 + 8 * q4) = s1;
                }
            }
            wait_lgkmcnt0();
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();      // the partials are read: the next item's may be written
        asm volatile("" ::: "memory");
        if (!more) break;
        w = nw; b = nb; h = nh;
    }
}

}  // namespace vlfm

using namespace vlfm;

// out[b][q][h * 64 ..] = softmax_t(scale * <q[b][q][h], K[b][t][h]>) . V[b][t][h] in f32, K / V read from the block-major f32 tensor
// vlfm_gemm_f16_pair_f32_nt writes: head h of K is block k_block0 + h, of V block v_block0 + h, image b rows [b T, (b + 1) T) of
// the m_total rows of a block.  Head width 64; 1 <= queries <= 32, 1 <= tokens <= 257; anything else: VLFM_ERR_INVALID.
extern "C" int vlfm_qformer_cross_attention_f32(const void* d_q, const void* d_kv_blocks, void* d_out, int batch, int tokens,
                                                int queries, int heads, int k_block0, int v_block0, int m_total, float scale,
                                                void* stream) {
    if (batch == 0) return VLFM_OK;
    if (!d_q || !d_kv_blocks || !d_out || batch < 0 || tokens < 1 || tokens > QA_MAX_T || queries < 1 || queries > QA_MAX_Q || heads < 1 ||
        k_block0 < 0 || v_block0 < 0 || (long long)batch * tokens > (long long)m_total)
        return fail(VLFM_ERR_INVALID, "qformer_cross_attention_f32: head width 64, 1-32 queries, 1-257 tokens, batch * tokens <= m_total");
    if ((((uintptr_t)d_q | (uintptr_t)d_kv_blocks | (uintptr_t)d_out) & 15) != 0)
        return fail(VLFM_ERR_INVALID, "qformer_cross_attention_f32: pointers must be 16-byte aligned");
    QaArgs a;
    a.q = (const float*)d_q; a.kv = (const float*)d_kv_blocks; a.out = (float*)d_out;
    a.B = batch; a.T = tokens; a.Q = queries; a.heads = heads; a.k_block0 = k_block0; a.v_block0 = v_block0; a.M_total = m_total;
    a.rows_pad = (tokens + 3) & ~3;
    a.scale_log2e = scale * 1.4426950408889634f;
    const size_t lds = 2 * (size_t)a.rows_pad * QA_ROWB + QA_MERGE;
    const void* fn = reinterpret_cast<const void*>(qformer_cross_attention_kernel);
    static LdsOptIn opt;
    if (!opt.ensure(fn, lds)) return fail(VLFM_ERR_HIP, "qformer_cross_attention_f32: cannot opt in to the LDS size");
    const long long items = (long long)((batch + 7) / 8) * 8 * heads;
    const int n_cu = device_cu_count() & ~7;
    const dim3 grid((unsigned)(items < n_cu ? items : n_cu)), block(256);
    VLFM_TIMED("qformer_cross_attention_kernel", stream);
    VLFM_KLAUNCH(qformer_cross_attention_kernel, grid, block, lds, stream, a);
    return check_launch("qformer_cross_attention_kernel");
}
