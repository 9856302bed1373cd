// The staging role of conv_wino2_kernel and conv_wino3_kernel -- TEXT, included inside each kernel behind its `w_rsrc` (wino_f23.h,
// DESIGN.md §1).  Uses the kernel's a, lds-derived xw, lane, swave, tile_of, Ctot, nchunks, plane_bytes and PLANAR by name.
    // slot u = lane + 64 j  ->  (channel cc, row r, 4-float part); 108 of the 128 slots exist (planar x1: 120)
    int lconst[2], xoff[2], gnoff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int u = lane + 64 * j, cc = u / 54, r = (u - cc * 54) / 9, part = u - cc * 54 - r * 9;
        const bool v = u < 108;
        lconst[j] = v ? (r * a.Ws + 4 * part) * 4 + cc * plane_bytes : OOB;
        xoff[j] = v ? (cc * 6 + r) * XP + (PLANAR ? 2 : 4) * part : 12 * XP + lane * (PLANAR ? 2 : 4);
        gnoff[j] = (v ? cc : 0) * 4;
    }
    // parity-planar x1 ([ch][row & 1][col & 1][H/2][W/2]): 10 lanes per window row (5 x 16 bytes per plane), the scratch row
    // de-interleaved [even window columns: 20][odd: 20] (conv_wino.hip has the reasoning)
    int lconstp[PLANAR ? 2 : 1], xoffp[PLANAR ? 2 : 1], gnoffp[PLANAR ? 2 : 1];
    const int h2 = a.Hs >> 1, w2 = a.Ws >> 1;
    if (PLANAR) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int u = lane + 64 * j, cc = u / 60, r = (u - cc * 60) / 10, part = u - cc * 60 - r * 10;
            const bool v = u < 120;
            const int px = part < 5 ? 1 : 0, py = (r + 1) & 1, yo = (r + 1) / 2 - 1;      // window row r = image row oy0 - 1 + r, oy0 even
            const int xo = px ? 4 * part - 1 : 4 * (part - 5);
            lconstp[PLANAR ? j : 0] = v ? (((py * 2 + px) * h2 + yo) * w2 + xo) * 4 + cc * plane_bytes : OOB;
            xoffp[PLANAR ? j : 0] = v ? (cc * 6 + r) * XP + (px ? 4 * part : 20 + 4 * (part - 5)) : 12 * XP + lane * 4;
            gnoffp[PLANAR ? j : 0] = (v ? cc : 0) * 4;
        }
    }
    // tile descriptors: issue side (g_*: the tile whose chunks are being LOADED), activation side (a_*: one chunk behind)
    int g_n = 0, g_co = 0, g_oy = 0, g_ox = 0, g_ks = 0;
    const float *g_src1 = a.x1, *g_src2 = a.x2 ? a.x2 : a.x1;
    bool g_bord = false;
    int vo[2] = {lconst[0], lconst[1]}, g_so = 0;                        // NCHW offsets of the tile being loaded
    int va[2] = {lconst[0], lconst[1]}, g_sa = 0;                        // the offsets the loads use (planar x1 / NCHW)
    int vop[PLANAR ? 2 : 1] = {}, g_sop = 0;
    unsigned g_vmp = 0xffu, a_vmp = 0xffu, g_vm = 0xffu, g_lsh = 0, a_vm = 0xffu, a_lsh = 0;
    bool a_bord = false;
    auto describe = [&](int k) __attribute__((always_inline)) {
        const TileId tl = decode_tile(a, tile_of(k));
        const int iy0 = tl.oy0 - 1, ix0 = tl.ox0 - 1;
        g_n = tl.n; g_co = tl.co0 / BN; g_oy = tl.oy0; g_ox = tl.ox0; g_ks = tl.ks;
        g_src1 = a.x1 + (size_t)tl.n * a.C1 * (plane_bytes / 4);
        g_src2 = a.x2 ? a.x2 + (size_t)tl.n * a.C2 * (plane_bytes / 4) : g_src1;
        g_bord = tl.oy0 - 1 < 0 || tl.ox0 - 1 < 0 || tl.oy0 + TH + 1 > a.H || tl.ox0 + TW + 1 > a.W;
        const int g_base = (iy0 * a.Ws + ix0) * 4;
        g_so = g_bord ? 0 : g_base;
#pragma unroll
        for (int j = 0; j < 2; ++j) vo[j] = lconst[j];
        if (PLANAR) {
            const int basep = ((tl.oy0 >> 1) * w2 + (tl.ox0 >> 1)) * 4;
            g_sop = g_bord ? 0 : basep;
            g_vmp = 0xffu;
#pragma unroll
            for (int j = 0; j < 2; ++j) vop[PLANAR ? j : 0] = lconstp[PLANAR ? j : 0];
            if (g_bord) {
                g_vmp = 0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int u = lane + 64 * j, cc = u / 60, r = (u - cc * 60) / 10, part = u - cc * 60 - r * 10;
                    const int c0 = part < 5 ? 8 * part : 8 * (part - 5) + 1;
                    const bool rowok = u < 120 && iy0 + r >= 0 && iy0 + r < a.H;
                    vop[PLANAR ? j : 0] = rowok ? lconstp[PLANAR ? j : 0] + basep : OOB;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = c0 + 2 * e, ix = ix0 + c;
                        g_vmp |= (rowok && ix >= 0 && ix < a.W && c < 34) ? 1u << (4 * j + e) : 0u;
                    }
                }
            }
        }
        if (g_bord) {
            g_vm = 0; g_lsh = 0;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int u = lane + 64 * j, cc = u / 54, r = (u - cc * 54) / 9, part = u - cc * 54 - r * 9;
                const bool rowok = u < 108 && iy0 + r >= 0 && iy0 + r < a.H;
                // the 16 bytes of the leftmost part of an image row start one pixel before the row: shifted by one pixel and
                // rotated back after the load (at the very first row they would start before the buffer)
                const bool lsh = rowok && ix0 + 4 * part < 0;
                g_lsh |= lsh ? 1u << j : 0u;
                vo[j] = rowok ? lconst[j] + g_base + (lsh ? 4 : 0) : OOB;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ix = ix0 + 4 * part + e;
                    g_vm |= (rowok && ix >= 0 && ix < a.W && 4 * part + e < 34) ? 1u << (4 * j + e) : 0u;
                }
                // (a load of a border tile may straddle the end of an image row: the next row's pixels, or -- at the last row
                //  of the tensor -- dwords past num_records, which a raw buffer load range-checks one by one and returns as
                //  0: tools/ubench/oob_probe.hip; either way those elements are masked by g_vm)
            }
        }
        const bool starts_in_x1 = g_ks * nchunks * KC < a.C1;      // (a K slice may begin in the skip half of a concat: NCHW)
#pragma unroll
        for (int j = 0; j < 2; ++j) va[j] = (PLANAR && starts_in_x1) ? vop[PLANAR ? j : 0] : vo[j];
        g_sa = (PLANAR && starts_in_x1) ? g_sop : g_so;
    };
    struct Raw { f32x4 v[2]; float sc[2], sh[2]; bool planar; float ssc[2], ssh[2]; };      // (ssc / ssh: wave-uniform, IPDM_WINO2_SGN)
    Raw raw;
    const __amdgpu_buffer_rsrc_t gsc_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(a.act ? a.gn_scale : a.out), 0, a.act ? (a.B * Ctot + 64) * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t gsh_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(a.act ? a.gn_shift : a.out), 0, a.act ? (a.B * Ctot + 64) * 4 : 0, 0x00020000);
    // every iteration issues the same loads, needed or not (past the end of the stream they re-read chunks of the last tile:
    // valid addresses, results unused): with conditional issue the waitcnt pass has to assume the shortest path
    auto issue_raw = [&](int ch) __attribute__((always_inline)) {
        const int c0 = (g_ks * nchunks + ch) * KC;           // (g_*: the item whose chunks are being loaded)
        const bool from1 = c0 < a.C1;
        const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(from1 ? g_src1 : g_src2), 0, (from1 ? a.C1 : a.C2) * plane_bytes, 0x00020000);
        const int cb = ((from1 ? c0 : c0 - a.C1) + 2 * swave) * plane_bytes;
        raw.planar = PLANAR && from1;
        if (PLANAR && c0 == a.C1) {  // (uniform, once per tile) only x1 is stored parity-planar; the skip half of a concat is NCHW
#pragma unroll
            for (int j = 0; j < 2; ++j) va[j] = vo[j];
            g_sa = g_so;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
            raw.v[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, va[j], cb + g_sa, 0));
        const int gso = (g_n * Ctot + c0 + 2 * swave) * 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {                        // (the slot's channel: a per-lane offset; the planar slot map differs)
            const int go = (PLANAR && raw.planar) ? gnoffp[PLANAR ? j : 0] : gnoff[j];
            if (!IPDM_WINO2_SGN) {
                raw.sc[j] = bload(gsc_rsrc, go, gso);
                raw.sh[j] = bload(gsh_rsrc, go, gso);
            }
        }
        if (IPDM_WINO2_SGN && a.act) {          // (uniform address: s_load_dwordx2; the arrays carry a chunk of read-ahead past [B, Ctot])
            const int gi = __builtin_amdgcn_readfirstlane(g_n * Ctot + c0 + 2 * swave);
            const float *__restrict__ ps = a.gn_scale + gi, *__restrict__ ph = a.gn_shift + gi;
            raw.ssc[0] = ps[0]; raw.ssc[1] = ps[1];
            raw.ssh[0] = ph[0]; raw.ssh[1] = ph[1];
        }
    };
    // activate the 8 landed values, zero what lies outside the image, park them in the wave's scratch
    auto activate = [&]() __attribute__((always_inline)) {
        f32x2 d[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) { d[2 * j] = f32x2{raw.v[j][0], raw.v[j][1]}; d[2 * j + 1] = f32x2{raw.v[j][2], raw.v[j][3]}; }
        const bool pl = PLANAR && raw.planar;
        if (a_bord && !pl) {  // (uniform) undo the left-edge shift: {x0, x1, x2, x3} loaded from one pixel further right
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (a_lsh >> j & 1) { d[2 * j + 1] = f32x2{d[2 * j][1], d[2 * j + 1][0]}; d[2 * j] = f32x2{0.0f, d[2 * j][0]}; }
        }
        if (a.act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // which of the wave's two channels a staging slot belongs to is a CONSTANT lane mask (slot u = lane + 64 j, channel u / 54:
                // j = 1 always the second, j = 0 the second from lane 54 on; planar: 60) -- the select takes it as an immediate SGPR pair
                // instead of a compare result the compiler keeps alive (and spills) for the kernel's lifetime
                if (IPDM_WINO2_SGN && !(e & 1)) {
                    if (e == 0) {      // slot j = 0: lanes 0..53 (planar x1: 0..59) hold the wave's first channel, the rest its second
                        const unsigned long long m = (unsigned long long)((PLANAR && raw.planar) ? 0xf0000000u : 0xffc00000u) << 32;
                        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(raw.sc[0]) : "v"(raw.ssc[0]), "v"(raw.ssc[1]), "s"(m));
                        asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(raw.sh[0]) : "v"(raw.ssh[0]), "v"(raw.ssh[1]), "s"(m));
                    } else {           // slot j = 1: the second channel (the lanes without a slot park what they compute in their dump slot)
                        raw.sc[1] = raw.ssc[1];
                        raw.sh[1] = raw.ssh[1];
                    }
                }
                const f32x2 sc2 = {raw.sc[e >> 1], raw.sc[e >> 1]}, sh2 = {raw.sh[e >> 1], raw.sh[e >> 1]};
                d[e] = __builtin_elementwise_fma(d[e], sc2, sh2);
            }
            if (a.act == 2) {
                f32x2 ex[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) ex[e] = d[e] * -1.4426950408889634f;
#pragma unroll
                for (int e = 0; e < 4; ++e) { ex[e][0] = __builtin_amdgcn_exp2f(ex[e][0]); ex[e][1] = __builtin_amdgcn_exp2f(ex[e][1]); }
#pragma unroll
                for (int e = 0; e < 4; ++e) ex[e] = ex[e] + 1.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e) { ex[e][0] = __builtin_amdgcn_rcpf(ex[e][0]); ex[e][1] = __builtin_amdgcn_rcpf(ex[e][1]); }
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = d[e] * ex[e];
            }
        }
        if (a_bord) {
            const unsigned vm = pl ? a_vmp : a_vm;
            // per-element zeroing as v_bfe_i32 + v_and_b32 on the lane's bit mask (eight v_cndmask on eight 64-bit SGPR masks recomputed per
            // tile held sixteen SGPRs through the chunk loop -> spills): bit e of the mask, sign-extended: 0 / ~0 (volatile: not to be hoisted
            // into eight live registers).  On SCALARS: a bit_cast of `d[e >> 1][e & 1]` in this unrolled loop was compiled as component 0 of
            // the UPDATED vector for the odd elements (round 6: 46 GPU tests red; the same compiler behaviour as NOTEBOOK.md round 5,
            // `tools/experiments/dbg_up2.py`)
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = d[e >> 1][e & 1];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int keep;
                asm volatile("v_bfe_i32 %0, %1, %2, 1" : "=v"(keep) : "v"(vm), "n"(e));
                f[e] = __builtin_bit_cast(float, __builtin_bit_cast(int, f[e]) & keep);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) d[e] = f32x2{f[2 * e], f[2 * e + 1]};
        }
        if (pl) {            // every other window column: the de-interleaved half of the scratch row
#pragma unroll
            for (int j = 0; j < 2; ++j)
                *reinterpret_cast<f32x4 *>(xw + xoffp[PLANAR ? j : 0]) = f32x4{d[2 * j][0], d[2 * j][1], d[2 * j + 1][0], d[2 * j + 1][1]};
        } else if (PLANAR) { // four consecutive columns into the de-interleaved row (one scratch format per instantiation)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float *dst = xw + xoff[j];
                dst[0] = d[2 * j][0]; dst[1] = d[2 * j + 1][0];
                dst[20] = d[2 * j][1]; dst[21] = d[2 * j + 1][1];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
                *reinterpret_cast<f32x4 *>(xw + xoff[j]) = f32x4{d[2 * j][0], d[2 * j][1], d[2 * j + 1][0], d[2 * j + 1][1]};
        }
    };
