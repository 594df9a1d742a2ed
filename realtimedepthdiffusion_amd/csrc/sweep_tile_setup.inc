// sweep_tile_setup.inc -- included INSIDE the body of k_sweep_blocked (sweep_blocked.hip), kept apart for readability: from the raw tile loads
// vxr[], vpr[] (x_k, x_{k-1}), mr[] (metadata) and mup (metadata of the row above the block) to the register-resident tile: a[], b[],
// the right / down weights, the divisor and its reciprocal per pixel, the Dirichlet bits.
// Expects in scope: LX, G, lut[], tid-derived lx, x0, y0, colok, rows, cols, tile_inside, and the declarations of a, b, wr, wd, wl0, wu0,
// cnt, rcp, unsafe, dirichlet.
//
// Round 6.  A launch per block of 8 sweeps pays this setup 125 times per 4K solve, and in round 5's form it was 428 VALU instructions per
// thread (35.7 per pixel against 116 for the 8 sweeps behind it) wrapped in 41 exec-masked regions: every `cond ? lut[i] : 0` guarded
// its LDS read with a branch, so the 28 table gathers of a thread were issued and WAITED FOR one by one (24 s_waitcnt), and 118 v_mov
// zero-filled the joins.  Now (a) a gather is never conditional -- the INDEX is selected: entry 256 of the table is 0, the reference's own
// "no neighbour" (src/GPUSolver.cu:140-218 stores index 256, :270 sets its weight to 0) -- so all gathers of a thread are in flight
// together behind one wait; and (b) a workgroup whose whole extended tile (and the row above it) lies inside the image -- 90 % of the
// tiles at 4K, 95 % at 8K, a wave-uniform test on the tile's coordinates -- takes a path without any of the border selects.  Same
// values either way: a select whose condition holds for every pixel of the tile is the identity.
    auto finish_setup = [&]() {
        // (lane 0 of a tile row that is not at the image border lies in the discarded halo: wl0 = 0 is fine there)
#pragma unroll
        for (int g = 0; g < G; g++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float wl = i == 0 ? wl0[g] : wr[g][i - 1];
                const float wu = g == 0 ? wu0[i] : wd[g - 1][i];
                float c = 0.0f;                    // count accumulates left, right, up, down (:82,88,94,100)
                c += wl; c += wr[g][i]; c += wu; c += wd[g][i];
                cnt[g][i] = c == 0.0f ? 1.0f : c;
                rcp[g][i] = rcp_rn(cnt[g][i]);          // correctly rounded reciprocal, once per launch
                unsafe |= cnt[g][i] < 0x1p-126f;
            }
    };
    if (tile_inside) {
        // every pixel of the extended tile, its right and lower neighbours and the row above it are inside the image: no selects
#pragma unroll
        for (int g = 0; g < G; g++) {
            const auto vx = vxr[g], vp = vpr[g];
            const uint4 m = mr[g];
            const float xv[4] = {vx.x, vx.y, vx.z, vx.w}, pv[4] = {vp.x, vp.y, vp.z, vp.w};
            const uint32_t mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                a[g][i] = xv[i];
                b[g][i] = pv[i];
                wr[g][i] = lut[mv[i] & 255];
                wd[g][i] = lut[(mv[i] >> 8) & 255];
                dirichlet |= ((mv[i] >> 16) & 1u) << (g * 4 + i);
            }
            if (lx == LX - 1) wr[g][3] = 0.0f;           // (see below)
            wl0[g] = lane_from_prev(wr[g][3]);
        }
        {
            const uint32_t mv[4] = {mup.x, mup.y, mup.z, mup.w};
#pragma unroll
            for (int i = 0; i < 4; i++) wu0[i] = lut[(mv[i] >> 8) & 255];
        }
        finish_setup();
    } else {
#pragma unroll
        for (int g = 0; g < G; g++) {
            const int y = y0 + g;
            const bool ok = colok && y >= 0 && y < rows;
            const auto vx = vxr[g], vp = vpr[g];
            const uint4 m = mr[g];
            const float xv[4] = {vx.x, vx.y, vx.z, vx.w}, pv[4] = {vp.x, vp.y, vp.z, vp.w};
            const uint32_t mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const bool in = ok && x0 + i < cols;
                a[g][i] = in ? xv[i] : 0.0f;
                b[g][i] = in ? pv[i] : 0.0f;
                // the gather itself is unconditional: entry 256 of the table is the weight of "no neighbour", 0
                wr[g][i] = lut[(in && x0 + i + 1 < cols) ? (mv[i] & 255) : 256u];
                wd[g][i] = lut[(in && y + 1 < rows) ? ((mv[i] >> 8) & 255) : 256u];
                if (in && (mv[i] & kMetaDirichlet)) dirichlet |= 1u << (g * 4 + i);
            }
            // The right weight of a tile row's LAST pixel becomes 0 (at the image border it is 0 anyway, elsewhere that pixel is discarded
            // halo): the weight towards the pixel left of a block is then the previous lane's wr[g][3] for EVERY lane (0 for lane 0 by
            // bound_ctrl, 0 where the previous lane ends another tile row or lies outside the image), and the sweep takes the whole left
            // term -- weight times value, formed in the previous lane -- through one DPP operand instead of keeping wl0[] in registers.
            if (lx == LX - 1) wr[g][3] = 0.0f;
            wl0[g] = lane_from_prev(wr[g][3]);           // (for the divisor below only; +1 % at 1080p: three registers fewer in the 128-register tile)
        }
        {   // weights towards the row above the block: the down-weights of row y0-1
            const int y = y0 - 1;
            const uint4 m = mup;
            const bool ok = colok && y >= 0 && y + 1 < rows;
            const uint32_t mv[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int i = 0; i < 4; i++) wu0[i] = lut[(ok && x0 + i < cols) ? ((mv[i] >> 8) & 255) : 256u];
        }
        finish_setup();
    }
    // (or the solve's input holds depths outside the 3-operation divide's domain: persist_sync.hpp kSyncWild)
    const bool wave_unsafe = __builtin_amdgcn_ballot_w64(unsafe) != 0 || wild_word == wild_seq;
    // the update's last operation runs under an EXEC mask of the FREE pixels (sweep_common.hpp masked_fmac4): one lane mask per pixel
    // of the thread, in SGPR pairs (where the v_cndmask form kept its masks), and a Dirichlet pixel's value in BOTH iterates
    unsigned long long free_mask[G][4];
#pragma unroll
    for (int g = 0; g < G; g++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bool dir = (dirichlet >> (g * 4 + i)) & 1u;
            free_mask[g][i] = __builtin_amdgcn_ballot_w64(!dir);
            b[g][i] = dir ? a[g][i] : b[g][i];
        }
