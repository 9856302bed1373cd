// The optimiser update of a training step as ONE launch over a whole parameter set: ipdm_adam_step, and the host-side chunk
// table it walks (ipdm_adam_chunks).
//
// Replaces (reference file:line): self.optimizer.step() of train() (Utils/train_test_utils.py:268) for the optimiser the harness
// builds (:150-151, :164-165): torch.optim.Adam(params, init_lr, weight_decay=1e-5, betas=(0.9, 0.999)) -- weight decay as L2
// folded into the gradient, no amsgrad, no maximize.  torch runs that as a string of foreach launches over the ~400 tensors of a
// UNet; here every tensor of the set is cut into chunks of IPDM_ADAM_CHUNK floats once (on the host, when the optimiser is
// built), and one grid walks the chunk table.
//
// Arithmetic.  Per element, float32, in this order and with no contraction (`#pragma clang fp contract(off)`: the bits do not
// depend on what the compiler would fuse), division and square root correctly rounded:
//   gt = g + wd * p          (skipped when wd == 0, as torch skips it)
//   m' = m + w1 * (gt - m)                                  w1 = float(1 - beta1)      (torch's lerp_ at a weight below one half)
//   v' = b2 * v + w2 * (gt * gt)                            b2 = float(beta2), w2 = float(1 - beta2)
//   p' = p - ss * (m' / (sqrt(v') / bc2s + eps))            ss = float(lr / (1 - beta1^t)), bc2s = float(sqrt(1 - beta2^t))
// The bias corrections and ss are formed on the host in double and handed over as float32, as torch does for a float32 tensor.
// p, m and v are written in place, g is only read.
//
// Shape.  A pure streaming kernel: 16 bytes in and 12 out per element, some twenty VALU operations beside them (the correctly
// rounded division and square root are the bulk) -- two orders under what the vector units deliver per byte of HBM traffic, so
// the only thing to arrange is enough independent 16-byte accesses in flight.  A workgroup is 256 threads (four waves, one per
// SIMD); a thread of a full chunk makes four trips of one 16-byte load per array, the four loads of a trip independent of one
// another.  The kernel holds no LDS and 44 vector registers (the compiler's report: 8 waves per SIMD, no spill -- the build
// refuses one), so a CU keeps eight workgroups: 2048 lanes x 64 bytes per trip is 128 KiB in flight per CU, several times the
// ~50 KiB per CU that cover the HBM latency at full bandwidth (6.3 TB/s x ~2 us over 256 CUs): occupancy, not unrolling, hides it.  The grid is capped
// at 256 CUs x 8 workgroups and strides over the chunk table, so a workgroup handles one chunk of a small parameter set and a
// few of a large one.  A chunk is 4096 floats = 16 KiB per array: large enough that the two records a workgroup reads per chunk
// (56 bytes, scalar loads, cached) are nothing beside its 112 KiB of traffic, small enough that the largest tensors of the
// production networks (3x3 layers from 512 to 256 channels, 288 chunks) spread over the chip instead of serialising on one
// workgroup.  Tensors far below a chunk (the norms' and biases' 64..512 floats, most of the table's rows) leave most of a
// workgroup's lanes idle for one trip; they are a per-mille of the bytes.
//
// Access width.  A chunk goes in 16-byte accesses only when all four of its addresses are 16-byte aligned (chunk offsets are
// multiples of 4096 floats, so that is a property of the tensor); its last len % 4 elements, and every element of a chunk that
// is not aligned (a view that starts at an odd float offset), go one float at a time.  Neither form touches a float outside
// [0, n) of a tensor: the chunk's extent is clamped to the tensor record's n in the kernel, whatever the table says.
// No atomics, no LDS, no cross-lane work: an element is owned by one lane, so a call's bits depend on its inputs alone.
#include <cmath>
#include "common.h"

using namespace ipdm;

static_assert(sizeof(ipdm_adam_tensor) == 40, "ipdm_adam_tensor: four pointers and a 64-bit count");
static_assert(sizeof(ipdm_adam_chunk) == 16, "ipdm_adam_chunk: two 32-bit fields and a 64-bit offset");

namespace {

// the float32 scalars of the element expression (above)
struct AdamCoef { float w1, b2, w2, wd, eps, ss, bc2s; };

__device__ inline void adam_elem(const AdamCoef &k, float &p, float g, float &m, float &v)
{
#pragma clang fp contract(off)
    const float gt = k.wd != 0.f ? g + k.wd * p : g;
    m = m + k.w1 * (gt - m);
    v = k.b2 * v + k.w2 * (gt * gt);
    p = p - k.ss * (m / (sqrtf(v) / k.bc2s + k.eps));
}

__global__ void __launch_bounds__(256) adam_step_kernel(const ipdm_adam_tensor *__restrict__ tensors, int n_tensors,
                                                        const ipdm_adam_chunk *__restrict__ chunks, long n_chunks, AdamCoef k)
{
    for (long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const ipdm_adam_chunk ch = chunks[c];
        if (ch.tensor < 0 || ch.tensor >= n_tensors) continue;
        const ipdm_adam_tensor t = tensors[ch.tensor];
        // a tensor without a gradient this step (g == NULL) is skipped as torch skips it; the extent comes from the RECORD
        if (!t.p || !t.g || !t.m || !t.v || ch.offset < 0 || ch.offset >= t.n || ch.len <= 0) continue;
        const long left = t.n - ch.offset;
        const int len = (long)ch.len < left ? ch.len : (int)left;
        float *p = t.p + ch.offset, *m = t.m + ch.offset, *v = t.v + ch.offset;
        const float *g = t.g + ch.offset;
        const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15u) == 0;
        const int n4 = vec ? len >> 2 : 0;
        for (int i = threadIdx.x; i < n4; i += 256) {
            float4 pv = reinterpret_cast<float4 *>(p)[i], mv = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
            const float4 gv = reinterpret_cast<const float4 *>(g)[i];
            adam_elem(k, pv.x, gv.x, mv.x, vv.x);
            adam_elem(k, pv.y, gv.y, mv.y, vv.y);
            adam_elem(k, pv.z, gv.z, mv.z, vv.z);
            adam_elem(k, pv.w, gv.w, mv.w, vv.w);
            reinterpret_cast<float4 *>(p)[i] = pv;
            reinterpret_cast<float4 *>(m)[i] = mv;
            reinterpret_cast<float4 *>(v)[i] = vv;
        }
        // the tail of an aligned chunk, or the whole of any other
        for (int i = (n4 << 2) + threadIdx.x; i < len; i += 256) {
            float pe = p[i], me = m[i], ve = v[i];
            adam_elem(k, pe, g[i], me, ve);
            p[i] = pe;
            m[i] = me;
            v[i] = ve;
        }
    }
}

}  // namespace

extern "C" int64_t ipdm_adam_chunks(const int64_t *sizes, int32_t n_tensors, ipdm_adam_chunk *out, int64_t cap)
{
    IPDM_REQUIRE(n_tensors >= 0 && (sizes || n_tensors == 0), "adam_chunks: NULL sizes or a negative tensor count (%d)", n_tensors);
    IPDM_REQUIRE(cap >= 0, "adam_chunks: negative capacity");
    int64_t count = 0;
    for (int32_t t = 0; t < n_tensors; ++t) {
        IPDM_REQUIRE(sizes[t] >= 0, "adam_chunks: tensor %d has a negative size (%lld)", t, (long long)sizes[t]);
        for (int64_t off = 0; off < sizes[t]; off += IPDM_ADAM_CHUNK, ++count) {
            if (out && count < cap) {
                const int64_t left = sizes[t] - off;
                out[count].tensor = t;
                out[count].len = (int32_t)(left < IPDM_ADAM_CHUNK ? left : IPDM_ADAM_CHUNK);
                out[count].offset = off;
            }
        }
    }
    return count;
}

extern "C" int ipdm_adam_step(const ipdm_adam_tensor *d_tensors, int32_t n_tensors, const ipdm_adam_chunk *d_chunks, int64_t n_chunks,
                              double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step, void *stream)
{
    IPDM_REQUIRE(n_tensors >= 0 && n_chunks >= 0, "adam_step: negative table size (%d tensors, %lld chunks)", n_tensors,
                 (long long)n_chunks);
    IPDM_REQUIRE(step >= 1, "adam_step: step %lld (the first update is step 1)", (long long)step);
    IPDM_REQUIRE(std::isfinite(lr) && lr >= 0.0, "adam_step: learning rate %g", lr);
    IPDM_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "adam_step: betas (%g, %g) outside [0, 1)", beta1, beta2);
    IPDM_REQUIRE(std::isfinite(eps) && eps >= 0.0, "adam_step: eps %g", eps);
    IPDM_REQUIRE(std::isfinite(weight_decay) && weight_decay >= 0.0, "adam_step: weight decay %g", weight_decay);
    if (n_tensors == 0 || n_chunks == 0) return IPDM_OK;
    IPDM_REQUIRE(d_tensors && d_chunks, "adam_step: NULL tensor or chunk table");
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    AdamCoef k;
    k.w1 = (float)(1.0 - beta1);
    k.b2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.wd = (float)weight_decay;
    k.eps = (float)eps;
    k.ss = (float)(lr / bc1);
    k.bc2s = (float)std::sqrt(bc2);
    // enough workgroups to fill the chip (256 CUs x 8), never more than there are chunks; the rest by the grid stride
    const long grid = n_chunks < 2048 ? (long)n_chunks : 2048;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, d_tensors, (int)n_tensors, d_chunks,
                       (long)n_chunks, k);
    IPDM_LAUNCH_CHECK();
    return IPDM_OK;
}
