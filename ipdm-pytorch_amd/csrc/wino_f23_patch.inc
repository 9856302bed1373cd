// The lane maps of the input transform and the patch read of conv_wino2_kernel and conv_wino3_kernel -- TEXT, included inside each
// kernel in front of its own transform_patch (wino_f23.h, DESIGN.md §1).  Uses the kernel's xw, lane, lk and PLANAR by name.
    // input transform: the wave transforms the (tile, channel) pairs of its own scratch -- lane map 16 tiles x 2 k-steps x 2
    // channel parities, so that the 32 lanes of an LDS store group write a 64-float span of the [tile][k-step] image at most
    // 2-way conflicted (free)
    // (lane = tile column w_tx, tile row w_ty, channel lk of the wave's two: channel 2 w + lk of the chunk = k step w & 3, k
    //  parity lk of sub-chunk w >> 2)
    const int w_tx = lane & 15, w_ty = (lane >> 4) & 1;
    const float *const xr = xw + (lk * 6 + 2 * w_ty) * XP + 2 * w_tx;
    const int v_slot = (w_tx & 1) * 16 + (w_tx >> 1) * 2 + w_ty;                    // MFMA lane of tile (row w_ty, column w_tx)
    float patch[16];
    f32x2 pp[4][2];                                                                  // the same patch as aligned column pairs (IPDM_WINO2_PKT)
    constexpr int pcol[4] = {0, PLANAR ? 2 : 1, PLANAR ? 1 : 2, 3};                  // register position of patch column c
    auto read_patch = [&]() __attribute__((always_inline)) {
        const float *const xrp = xr - w_tx;                                         // column pairs (tx, tx + 1) of both halves
        if (PLANAR) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                patch[4 * r] = xrp[r * XP]; patch[4 * r + 1] = xrp[r * XP + 1];
                patch[4 * r + 2] = xrp[r * XP + 20]; patch[4 * r + 3] = xrp[r * XP + 21];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x2 lo = *reinterpret_cast<const f32x2 *>(xr + r * XP), hi = *reinterpret_cast<const f32x2 *>(xr + r * XP + 2);
                if (IPDM_WINO2_PKT) { pp[r][0] = lo; pp[r][1] = hi; }
                else { patch[4 * r] = lo[0]; patch[4 * r + 1] = lo[1]; patch[4 * r + 2] = hi[0]; patch[4 * r + 3] = hi[1]; }
            }
        }
    };
