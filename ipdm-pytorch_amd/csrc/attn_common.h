// Device helpers shared by the attention kernels (attn.hip: exact f32; attn_bx3.hip: bf16 matrix pipe, 3-way split).
// The key-slice recurrence lives here once: the split grid + attention_combine_kernel and a workgroup that walks its slices
// itself (zseq) must apply the same float operations in the same order, whichever kernel produced the slices.
#pragma once
#include <hip/hip_runtime.h>
#include "kernel_util.h"      // crow: the row of an accumulator register of the 32x32 MFMAs

namespace ipdm {
namespace attn {

constexpr float LOG2E = 1.4426950408889634f;

// Maximum / sum over the two halves of the wave (lanes l and l ^ 32) by v_permlane32_swap (gfx950): one VALU instruction
// turns two copies of x into {lo, lo} and {hi, hi}.  As __shfl_xor(x, 32) the exchange is a ds_bpermute, an LDS round trip
// of ~100 cycles that the softmax waits for once per key block (the row maximum feeds every exponential).  Inline
// assembly: the builtin mis-pairs its two results when both inputs are the same value; the two wait states are the
// VALU-write -> permlane-read hazard the compiler would insert itself.
__device__ inline float halves_max(float x)
{
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}
__device__ inline float halves_sum(float x)
{
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return a + b;
}

// Key slices (short sequences, attention_kv_split): every slice is reduced with a FRESH running maximum / sum / output, and
// the slices are folded in ascending order by this recurrence -- by the workgroup itself when it walks all slices of its
// queries (zseq), or by attention_combine_kernel when the slices ran as separate workgroups (zsplit).  The same float
// operations in the same order in both, so how a launch is scheduled (it depends on the batch size) never changes a bit.
//   M' = max(M, m_k);  a = 2^((M - M') log2e);  b = 2^((m_k - M') log2e);  num = num a + o_k b;  den = den a + l_k b
struct SliceWeights { float a, b; };
__device__ inline SliceWeights slice_weights(float &M, float m_k)
{
    const float Mn = fmaxf(M, m_k);
    SliceWeights w;
    w.a = __builtin_amdgcn_exp2f((M - Mn) * LOG2E);        // first slice: M = -inf -> 0
    w.b = __builtin_amdgcn_exp2f((m_k - Mn) * LOG2E);
    M = Mn;
    return w;
}
__device__ inline float slice_fold(float acc, float v, SliceWeights w) { return fmaf(acc, w.a, v * w.b); }

}  // namespace attn
}  // namespace ipdm
