// What conv_wino2.hip (f32 MFMA) and conv_wino3.hip (bf16 x 3) share outside their kernel bodies: the compile-time flags, the tile
// geometry, the tile decoder and the launch rule.  The shared parts of the kernel BODIES are the fragments wino_f23_*.inc, included as
// text inside each __global__ function (DESIGN.md §1 says why text): a change here or there is a change to both kernels.
#pragma once
#include <cstdlib>
#include <type_traits>
#include "common.h"
#include "unet_kernels.h"
#include "kernel_util.h"

#ifndef IPDM_WINO2_KO
#define IPDM_WINO2_KO 0             // compile-time timing knock-outs (tools/build_variants.sh; results are WRONG under a knock-out):
#endif                              // 1 no activation, 2 no input transform, 4 no output transform / stores, 8 no window loads, 16 no U loads,
                                    // 32 output transform and exchange kept, but NO residual loads, stores or statistics (the part of the epilogue
                                    // that could move under the next tile's first chunk: an upper bound on what deferring it can buy),
                                    // 64 no exchange (LDS round trip + barrier E; the in-lane form of the 16x16x4 idea would remove exactly this)
#ifndef IPDM_WINO2_STAGGER
#define IPDM_WINO2_STAGGER 0        // conv_wino2 only: 1 = waves 4-7 stage between the two sub-chunks, 2 = every wave does (its chunk lambda)
#endif
#ifndef IPDM_WINO2_SGN
#define IPDM_WINO2_SGN 1            // 1: the GroupNorm scale / shift of the wave's two channels through SCALAR loads (two s_load_dwordx2 per chunk
#endif                              //    instead of four per-lane dword buffer loads: 4 of the 22 vector-memory instructions of a chunk) -- round 5 experiment
                                    // (IPDM_WINO2_SGN 0, IPDM_WINO2_STAGGER and IPDM_WINO2_DEFER are finished experiments whose dead arms STAY: deleting
                                    //  one changes both kernels' code -- NOTEBOOK.md; a measured pull request's work)
#ifndef IPDM_WINO2_PKT
#define IPDM_WINO2_PKT 1            // 1: the input transform of the NCHW instantiations as sixteen packed-f32 adds (0: the scalar form; same bits)
#endif
#ifndef IPDM_WINO2_DEFER
#define IPDM_WINO2_DEFER 0          // 1: the eight 16-byte stores of an interior tile are issued under the NEXT tile's first MFMAs (round 5 experiment)
#endif
#ifndef IPDM_CONV_STAMPS
#define IPDM_CONV_STAMPS 0          // `make stamps`: in-kernel s_memtime stamps of the phases (a stamped build changes what it measures)
#endif

namespace ipdm {

constexpr int KC = 16;                                 // channels per staged chunk: two MFMA sub-chunks of 8 (4 k-steps of 2)
constexpr int TH = 4, TW = 32, BN = 128;               // output pixels / couts of a workgroup tile
constexpr int NW = 8;                                  // waves
constexpr int U_CHUNK_FLOATS = 16 * 2 * 2 * 32 * 4;    // packed f32 weights of one (8-channel chunk, 64-cout tile)
constexpr int XCH_FLOATS = NW * 8 * 64 * 4;            // per wave: 8 x (64 lanes x 16 bytes)
constexpr int XP = 40;                                 // scratch row pitch (34 window columns; planar: columns up to 39)
constexpr int XWAVE = 12 * XP + 64 * 4 + 8;            // per wave: 12 row segments (2 channels x 6 window rows) + a dump slot per lane
static_assert(128 <= XWAVE, "wino_f23: the statistics staging aliases the wave's scratch");

struct TileId { int n, oy0, ox0, co0, ks; };      // ks: slice of the K (input channel) range, ConvArgs::ksplit

__device__ inline TileId decode_tile(const ConvArgs &a, int item)
{
    TileId t;
    t.ks = item % a.ksplit;                            // the K slices of one tile are neighbours in the schedule
    const int tile = item / a.ksplit;
    const int co_t = tile % a.co_tiles;
    int rest = tile / a.co_tiles;
    const int tx = rest % a.tiles_x;
    rest /= a.tiles_x;
    const int ty = rest % a.tiles_y;
    t.n = rest / a.tiles_y;
    t.oy0 = ty * TH;
    t.ox0 = tx * TW;
    t.co0 = co_t * BN;
    return t;
}

// workgroups of a launch over ntiles schedule items: one per CU (fewer tiles: one per tile), rounded up to the eight XCDs the
// kernels' static schedule deals the tiles over
inline unsigned wino_f23_grid(long ntiles)
{
    const int cus = device_cu_count();
    const long G = ntiles < cus ? ntiles : cus;
    return (unsigned)((G + 7) / 8 * 8);
}

// the instantiation <PLANAR, RES> of `kernel` a launch runs
#define IPDM_WINO_F23_PICK(kernel, planar, res)                                                                   \
    ((planar) ? ((res) ? (const void *)kernel<true, true> : (const void *)kernel<true, false>)                    \
              : ((res) ? (const void *)kernel<false, true> : (const void *)kernel<false, false>))

// 512 threads, one schedule-item count; (the caller's launch check reads the error)
inline int wino_f23_launch(const void *fn, size_t lds_bytes, ConvArgs &a, long ntiles, hipStream_t st)
{
    if (int rc = ensure_dynamic_lds(fn, lds_bytes)) return rc;
    int nt = (int)ntiles;
    void *params[] = {&a, &nt};
    (void)hipLaunchKernel(fn, dim3(wino_f23_grid(ntiles)), dim3(512), params, lds_bytes, st);
    return IPDM_OK;
}

}  // namespace ipdm
