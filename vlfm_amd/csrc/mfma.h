// What the matrix-core kernels share (gemm_f16.hip, gemm_f32.hip, conv_nhwc.hip, vit_attention.hip, qformer_attention.hip): operand
// vector types, the address-space aliases of LDS-DMA, counted waits, the 128-byte-row swizzle and the per-XCD tile remap.  Only what
// at least two of them use lives here.
#pragma once
#include <hip/hip_runtime.h>
namespace vlfm {

typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

using lds_ptr = __attribute__((address_space(3))) unsigned char*;
using gbl_ptr = const __attribute__((address_space(1))) unsigned char*;

// s_waitcnt through the builtin (the compiler's own scoreboard sees it; beside inline-asm waits it re-waits for everything at
// the loop head): simm16 = vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt_hi[15:14], a field of all ones = "do not wait for it".
template <int N>
__device__ __forceinline__ void wait_vmcnt() {          // at most N vector-memory operations (LDS-DMA loads, loads, stores) in flight
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    constexpr int simm16 = 0x0F70 | (N & 15) | ((N >> 4) << 14);
    __builtin_amdgcn_s_waitcnt(simm16);
}
__device__ __forceinline__ void wait_lgkmcnt0() { __builtin_amdgcn_s_waitcnt(0xC07F); }     // every LDS operation has returned

// Byte offset of logical 16-byte slot `slot` inside 128-byte row `row`: the slot is XORed with (row >> 1) & 7, so that the 16 rows
// a ds_read_b128 group touches hit 16 different bank groups.  Staging (the slot a lane FETCHES for the place it lands at) and the
// fragment reads must use the same permutation; it is its own inverse.
__host__ __device__ constexpr int swz128(int row, int slot) { return (slot ^ ((row >> 1) & 7)) << 4; }

// Workgroup ids go round-robin over the 8 XCDs: position in a list of nwg tiles such that every XCD gets a contiguous range
// (a bijection of [0, nwg): XCDs below nwg % 8 take one tile more).
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

}  // namespace vlfm
