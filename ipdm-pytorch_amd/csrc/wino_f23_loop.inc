// The state of the tile loop of conv_wino2_kernel and conv_wino3_kernel (chunk counter, deferred stores, cycle stamps, the tile being
// multiplied) -- TEXT, included inside each kernel behind its prologue (wino_f23.h, DESIGN.md §1).  Defines IPDM_STAMP; the kernel
// undefines it behind its stamp write-out.
    int s = 0;                                             // running chunk index (V stage parity)
    int k = 0;
    // deferred stores (IPDM_WINO2_DEFER): the finished 4-pixel runs of the previous tile, stored two per position under the first
    // sixteen MFMAs of this tile -- their registers are the ones the accumulators started last will take
    // (the stores are issued UNCONDITIONALLY, with an out-of-range offset when there is nothing to store: a conditionally issued
    //  memory operation makes the wait-count pass assume the shorter path, and every wait behind it comes out too strict)
    int d_voff = OOB;
    f32x4 d_v[8];
    size_t d_sample = 0;
    int d_so0 = 0;
    const int d_lane_off4 = ((lk * 4 + odd) * out_plane + (2 * ty + ih) * a.Wo + 4 * txh) * 4;
    typedef unsigned du32x4 __attribute__((ext_vector_type(4)));
    auto deferred_store = [&](int i) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.out + d_sample), 0, a.Cout * out_plane * 4, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(du32x4, d_v[i]), rs, d_voff, d_so0 + (8 * (i >> 1) + 2 * (i & 1)) * plane4, 0);
    };
    const bool stamp = IPDM_CONV_STAMPS && (a.dbg & 8) != 0;
    unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_t = 0;      // stage / multiply / transform / barrier / epilogue
    const unsigned long long st_begin = stamp ? __builtin_amdgcn_s_memtime() : 0;
#define IPDM_STAMP(slot) if (stamp) { __builtin_amdgcn_sched_barrier(0); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); st_acc[slot] += now_ - st_t; st_t = now_; __builtin_amdgcn_sched_barrier(0); }
    if (stamp) st_t = st_begin;
    TileId cur = {g_n, g_oy, g_ox, g_co * BN, g_ks};
