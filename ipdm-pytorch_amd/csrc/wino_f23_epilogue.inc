// The tile epilogue of conv_wino2_kernel and conv_wino3_kernel (bias, output transform, partner exchange, residual, stores, ragged
// edge, fused statistics) -- TEXT, included inside each kernel's tile loop behind its chunks (wino_f23.h, DESIGN.md §1).  The including
// file defines three hooks (possibly empty) in front of the include:
//   IPDM_WINO_F23_XCH          a local definition of `xch`, the exchange buffer, where it is not a kernel-wide constant
//   IPDM_WINO_F23_PRE_OUT      statements in front of the residual loads and the output transform
//   IPDM_WINO_F23_POST_XCH     statements behind the reads of the exchange buffer
        if (IPDM_WINO2_KO & 4) { cur = TileId{g_n, g_oy, g_ox, g_co * BN, g_ks}; continue; }
        // + bias through position (1, 1) (accumulator 5 of the ih = 0 waves), whose output coefficients are all 1
        if (ih == 0) {
            acc[5] = __builtin_amdgcn_mfma_f32_32x32x2f32(nb, 1.0f, acc[5], 0, 0, 0);
            if (k + 1 < n_my) fetch_bias(g_co * BN);        // (describe(k + 1) ran two chunks ago)
        }
        const TileId t = cur;
        cur = TileId{g_n, g_oy, g_ox, g_co * BN, g_ks};
        const size_t sample = ((size_t)t.ks * a.B + t.n) * a.Cout * out_plane;      // (ks > 0 only with a.out = the split workspace [ksplit][B,Cout,Ho,Wo])
        const __amdgpu_buffer_rsrc_t o_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(a.out + sample), 0, a.Cout * out_plane * 4, 0x00020000);
        // (no residual: zero records -- the loads below return 0 and the add stays unconditional)
        const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)((a.res ? a.res : a.out) + sample), 0,
                                                                                   a.res ? a.Cout * out_plane * 4 : 0, 0x00020000);
        // The lanes l and l + 16 (tile columns 2m, 2m + 1) hold 4 consecutive pixels of the row between them.  Registers are
        // taken in pairs (couts c, c + 1): v_permlane16_swap exchanges one half each, after which the lane of the even column
        // owns the 4 pixels of cout c and the other one those of cout c + 1 -- 16-byte stores and residual loads.
        const int py = t.oy0 + 2 * ty + ih, px4 = t.ox0 + 4 * txh;
        const bool rok = py < a.Ho;
        const int lane_off4 = ((lk * 4 + odd) * out_plane + (2 * ty + ih) * a.Wo + 4 * txh) * 4;
        const int voff4 = (rok && px4 + 3 < a.Wo) ? lane_off4 : OOB;             // all four pixels of the lane's run
        const bool ragged = t.ox0 + TW > a.Wo && (a.Wo & 3) != 0;                // (wave-uniform) a run straddles the right edge
        const bool clipped = t.oy0 + TH > a.Ho || t.ox0 + TW > a.Wo;             // (wave-uniform) some lanes own no pixels
        const int nval = a.Wo - px4;                                              // ... then it has 1..3 pixels
        const bool part = ragged && rok && nval > 0 && nval < 4;
        const int so0 = ((t.co0 + hq * 32) * out_plane + min(t.oy0, a.Ho - 1) * a.Wo + t.ox0) * 4;
        IPDM_WINO_F23_XCH
        const float *xr2 = xch + ((swave ^ 1) * 8) * 256 + lane * 4;
        float *sb = xw;                                      // statistics staging: the wave's scratch is idle here
        const f32x2 sgn2 = {sgn, sgn};
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        IPDM_WINO_F23_PRE_OUT
        // ALL residual loads of the tile are issued together, ahead of the transform
        f32x4 rv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            rv[i] = ((IPDM_WINO2_KO & 32) || !RES) ? f32x4{0.0f, 0.0f, 0.0f, 0.0f}
                                         : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r_rsrc, voff4, so0 + (8 * (i >> 1) + 2 * (i & 1)) * plane4, 0));
        __builtin_amdgcn_sched_barrier(0);
        // columns first (in-lane): T_i[b] = sum_j M[i][j] A[j][b],  A^T = [[1,1,1,0],[0,1,-1,-1]]; then the wave's own two
        // rows (first = accumulators 0-3, second = 4-7; ih = 0: rows 0, 1, ih = 1: rows 3, 2 -- row_slot): both waves keep
        // K = first + second and send the second (T1 resp. T2); output row 0 = (T0 + T1) + T2, row 1 = T1 - (T2 + T3).
        f32x2 K0[8], K1[8];                                 // [pair]: output column 0 / 1 of {cout c, cout c + 1}
        {
            float *xo = xch + (swave * 8) * 256 + lane * 4;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int r = 2 * p;
#define IPDM_M(e) f32x2{acc[e][r], acc[e][r + 1]}
                const f32x2 lo0 = (IPDM_M(0) + IPDM_M(1)) + IPDM_M(2), lo1 = (IPDM_M(1) - IPDM_M(2)) - IPDM_M(3);
                const f32x2 hi0 = (IPDM_M(4) + IPDM_M(5)) + IPDM_M(6), hi1 = (IPDM_M(5) - IPDM_M(6)) - IPDM_M(7);
#undef IPDM_M
                K0[p] = lo0 + hi0;
                K1[p] = lo1 + hi1;
                if (!(IPDM_WINO2_KO & 64)) *reinterpret_cast<f32x4 *>(xo + p * 256) = f32x4{hi0[0], hi0[1], hi1[0], hi1[1]};
                else { K0[p] += hi0 * 0.5f; K1[p] += hi1 * 0.5f; }      // (timing only: keeps the values alive without the exchange)
            }
        }
        IPDM_STAMP(5)
        if (!(IPDM_WINO2_KO & 64)) __syncthreads();        // E: both halves of every (tile, cout) are in LDS
        IPDM_STAMP(6)
        f32x4 ko_sum = {0.0f, 0.0f, 0.0f, 0.0f};
        f32x4 gotv[8];                                     // partner's {T[0] c, T[0] c+1, T[1] c, T[1] c+1} of every pair
#pragma unroll
        for (int i = 0; i < 8; ++i) gotv[i] = (IPDM_WINO2_KO & 64) ? f32x4{K0[i][0], K0[i][1], K1[i][0], K1[i][1]} : *reinterpret_cast<const f32x4 *>(xr2 + i * 256);
        IPDM_WINO_F23_POST_XCH
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int g = i >> 1, u = 2 * (i & 1);
            const f32x4 got = gotv[i];
            // ih = 0: K + T2 (output row 0);  ih = 1: T1 - K (output row 1)
            const f32x2 y0 = __builtin_elementwise_fma(K0[i], sgn2, f32x2{got[0], got[1]});       // column 0 of {cout c, c + 1}
            const f32x2 y1 = __builtin_elementwise_fma(K1[i], sgn2, f32x2{got[2], got[3]});       // column 1
            // rows r (even tile column) and r + 1 (odd) of the DPP row pair: the even one gives its cout c + 1 and takes the
            // odd one's cout c  (inline asm: through the builtin this compiler passed component 0 of y0 / y1 as BOTH operands
            // of the swap; s_nop: the swap reads need two wait states after the VALU writes)
            float ya0 = y0[0], yb0 = y0[1], ya1 = y1[0], yb1 = y1[1];
            asm("s_nop 1\n\t"
                "v_permlane16_swap_b32 %0, %1\n\t"
                "v_permlane16_swap_b32 %2, %3"
                : "+v"(ya0), "+v"(yb0), "+v"(ya1), "+v"(yb1));
            f32x4 v = {ya0, ya1, yb0, yb1};
            const int so = so0 + (8 * g + u) * plane4;
            v += rv[i];
            if (IPDM_WINO2_KO & 32) {      // (timing only: ONE store per tile, of the sum of all eight results, keeps the transform alive)
                ko_sum += v;
                if (i == 7) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, ko_sum), o_rsrc, voff4, so, 0);
                continue;
            }
            // (IPDM_WINO2_DEFER: an interior tile -- wave-uniform: every lane owns its whole run -- keeps its runs for the next tile's
            //  first MFMAs; d_v is DEFINED on every path so that its live range ends at the deferred stores)
            if (IPDM_WINO2_DEFER) d_v[i] = v;
            if (!(IPDM_WINO2_DEFER && !clipped && !ragged)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), o_rsrc, voff4, so, 0);
            if (ragged) {            // (wave-uniform) the run that straddles the edge: element by element, by its lane
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int vo1 = (part && e < nval) ? lane_off4 + 4 * e : OOB;
                    float x = v[e];
                    if (RES) x += bload(r_rsrc, vo1, so);          // (the lane's 16-byte residual load was out of range: + 0 above)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), o_rsrc, vo1, so, 0);
                    if (part) v[e] = e < nval ? x : 0.0f;
                }
            }
            if (a.stats) {
                // fused GroupNorm statistics of the output: one row of per-cout {sum, sum of squares} per PIXEL ROW and
                // 32-pixel column block, as conv_ws.hip writes them; the 8 lanes of one tile row in a DPP row share a cout
                float s1 = (v[0] + v[1]) + (v[2] + v[3]);
                float s2 = fmaf(v[3], v[3], fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0])));
                if (clipped) {
                    const bool ok = voff4 != OOB || part;
                    s1 = ok ? s1 : 0.0f; s2 = ok ? s2 : 0.0f;
                }
                asm("s_nop 1\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_ror:2 row_mask:0xf bank_mask:0xf\n\t"
                    "s_nop 0\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_ror:4 row_mask:0xf bank_mask:0xf\n\t"
                    "s_nop 0\n\t"
                    "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
                    "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0xf"
                    : "+v"(s1), "+v"(s2));
                if (txh == 0) *reinterpret_cast<f32x2 *>(sb + (ty * 32 + 8 * g + u + odd + 4 * lk) * 2) = f32x2{s1, s2};
            }
        }
        if (a.stats) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int row_y = t.oy0 + 2 * lk + ih;          // lanes 0-31: tile row 0, lanes 32-63: tile row 1; cout = l31
            if (row_y < a.Ho) {
                float *dst = a.stats + (((size_t)t.n * a.stats_rows + (size_t)row_y * a.tiles_x + t.ox0 / TW) * a.Cout + t.co0 + hq * 32 + l31) * 2;
                *reinterpret_cast<f32x2 *>(dst) = *reinterpret_cast<const f32x2 *>(sb + lane * 2);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (IPDM_WINO2_DEFER && !clipped && !ragged) { d_voff = d_lane_off4; d_sample = sample; d_so0 = so0; }
        // (wait states between the tile's last 16-byte stores and whatever writes their data registers next: gfx950 needs ONE for a
        //  buffer store with an SGPR soffset too, the compiler inserts none -- NOTEBOOK.md round 5; tools/check_store_hazard.py scans
        //  every kernel of the library for the pair at build time)
        asm volatile("s_nop 7");
        IPDM_STAMP(4)
#undef IPDM_WINO_F23_XCH
#undef IPDM_WINO_F23_PRE_OUT
#undef IPDM_WINO_F23_POST_XCH
