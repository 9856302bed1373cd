// The one-line device helpers and vector types that the kernels of both libraries share.  Everything here is inlined text: moving a
// helper in here leaves the including kernel's code as it was (tools/isa_equal.py).
#pragma once
#include <hip/hip_runtime.h>

namespace ipdm {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Per-lane (VGPR) buffer offset that is out of range: loads return 0 and stores are dropped, no branch.  The hardware
// compares the VGPR offset with (num_records - scalar offset), so the SCALAR offset must always stay inside the buffer:
// invalid elements are always killed through the per-lane offset, never through the scalar one.
constexpr int OOB = 0x7fffffff;

// one dword through a buffer resource: per-lane byte offset voff (range-checked), wave-uniform byte offset soff
__device__ inline float bload(__amdgpu_buffer_rsrc_t r, int voff, int soff)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}

// row of accumulator register r (lane half h = lane >> 5) in the output layout of the 32x32 MFMAs
__device__ inline int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The Winograd stage images keep the rows i of the 4x4 transform domain in the order 0, 1, 3, 2: consumer wave ih then holds rows
// (0, 1) or (3, 2) in its accumulators 0-3 / 4-7, and in the output transform BOTH waves keep first + second and send the
// second (T1 resp. T2) -- no wave-dependent selects.
__host__ __device__ constexpr int row_slot(int i) { return i ^ (i >> 1); }

}  // namespace ipdm
