// k_levels_body.inc -- the body of the level kernel (k_levels.hip has the description), as text that each of its two families includes:
// k_band_levels (k_levels.hip: a workgroup is ONE slot, two turn-taking waves) and k_band_levels2 (k_levels2.hip: a workgroup is TWO
// slots of one image, four waves).  Included text and not a function: lifted into a function the row loop comes out scheduled
// differently (as vpath1_walk.inc).  What differs between the families is named by the macros the including file defines:
//   LV_NT            threads of a workgroup (the set-up loops' stride)
//   LV_SLOT_STATE    declares what LV_POLLED and LV_A name: a slot's own words in LDS
//   LV_WAVE          declares q (and whatever else says which slot of the workgroup the wave belongs to)
//   LV_BLOCK         declares slot and image from blockIdx.x (dbg is in scope)
//   LV_INIT_FLAGS    clears s_fail and every slot's LV_POLLED
//   LV_AFTER_SETUP   what the waves of a slot that does not exist do once the workgroup's tables stand
//   LV_LEVEL_END     the hand-over that ends an iteration of the level loop: the workgroup's waves meet
//   LV_TRACK         1: the row loop keeps which rows and lanes changed and store_u writes only those (store_rows); 0: every row, as ever
//   LV_DBG, LV_STATS, LV_TIME    the translation unit's device globals (switches, event counters, the timing build's cycle counts)
    static_assert(DELTA >= 1 && DELTA <= LQR_FAST_MAX_DELTA && (DELTA <= 4 || RIG) && (RIG || !RIGM), "delta_x 1 .. 10 (5 .. 10: the rigidity form, with a zero table if there is none); a rigidity mask only matters with rigidity");
    constexpr int PX = 2, HALO = 32, OWN = LV_OWN, HL = 16, R = lv_rows(DELTA, RIGM), TILE = 128;
    static_assert(R * DELTA <= HALO, "a level's errors stay inside the halo");
    static_assert(HL == 16 && R <= 32, "lv_own_or: the own lanes are two whole rows of 16 lanes; a level's rows fit one word");
    typedef LaneVec<2>::F FV;
    typedef LaneVec<2>::L LV;
    typedef GLOBAL_AS FV GFV;
    typedef GLOBAL_AS LV GLV;
    typedef GLOBAL_AS unsigned long long gu64;
    __shared__ int s_tlo[LV_MAX_LEVELS], s_thi[LV_MAX_LEVELS];      // per level: columns the carve touched on its rows
    __shared__ int s_fail;                        // 1: a spin timed out (results invalid), 2: the image stopped (collision): leave at the next barrier
    LV_SLOT_STATE                                 // LV_POLLED: last level whose barrier the slot has passed; LV_A[2]: the active set of a level (by parity), from the wave that received it to its partner
        const int tid = threadIdx.x, lane = tid & 63;
    LV_WAVE                                       // q: which of its slot's two turn-taking waves this one is
    // A one-dimensional grid of 8 * ceil(n_img / 8) * P workgroups.  Workgroup b is observed to run on XCD b mod 8 (no promise: speed
    // only, the protocol is placement-independent): the P slots of an image are the workgroups b = xcd + 8 (P g + slot), image = 8 g +
    // xcd -- all on one XCD, whose L2 then serves the level hand-overs' reads a little sooner (handoff-1to1: cross-XCD +0.1 - 0.3 us)
    const int dbg = __builtin_amdgcn_readfirstlane(LV_DBG);
    // (lv_grid / lv_block in lqr_geom.h state this map and the test checks it there; here it stays in the kernel's own text: through the
    // function the instruction stream differs)
    // (debug switch 8: consecutive workgroups = the slots of one image, i.e. on DIFFERENT XCDs -- the placement the near copies do
    // not serve; the tests run it to show that nothing but speed depends on where the slots sit)
    LV_BLOCK                                      // slot, image
    if (image >= n_img) return;
    const int nblk = (h + R - 1) / R;
    const int ntiles = lv_tiles(w);
    GCarver c = gview(cs[image]);
    if constexpr (RIG && DELTA == 1 && !RIGM) { c.en = uni_ptr(c.en); c.m = uni_ptr(c.m); c.least = uni_ptr(c.least); }      // (see LEAN below)
    const size_t near_off = lv_near_off(ntiles);      // the near copies (see the header)
    gu64 *ex_img = (gu64 *) exch + exch_image_off(image, near_off);
    gu64 *flagw = ex_img;                                    // [2 parities][LV_PMAX slots][2 tiles]
    gu64 *gran = ex_img + LV_FLAG_WORDS;                      // [2 parities][ntiles][OWN]
    const float INF = __int_as_float(0x7f800000);
    const float rig_l = p.rigmap[0], rig_r = p.rigmap[2];
    float rg[2 * DELTA + 1];
#pragma unroll
    for (int i = 0; i < 2 * DELTA + 1; i++) rg[i] = p.rigmap[i];
    // which lanes of the barrier poll hold the words of the slot of tile `lane`, of tile `lane + 1`, of tile `lane - 1`
    const int ix_own = 2 * (lane % P), ix_right = 2 * ((lane + 1) % P), ix_left = 2 * ((lane + P - 1) % P);

    // ---- carve-touched columns per level (as k_band_tiles / k_band_update_tw)
    for (int i = tid; i < nblk; i += LV_NT) { s_tlo[i] = 1 << 30; s_thi[i] = -1; }
    LV_INIT_FLAGS                                       // (flags: through LDS_FLAG once the waves run apart)
    __syncthreads();
    for (int y = tid; y < h; y += LV_NT) {
        const int v0 = c.seam_x[y], vm = c.seam_x[max(y - 1, 0)], vp = c.seam_x[min(y + 1, h - 1)];
        // pixels of row y whose inputs the carve changed: the energy next to the seam on rows y - 1 .. y + 1, and the pixels whose
        // parent window (DELTA either way on row y - 1) straddles the seam there: [min - DELTA - 1, max + DELTA]
        const int t0 = max(min(min(v0, vm), vp) - DELTA - 1, 0), t1 = min(max(max(v0, vm), vp) + DELTA, w - 1);
        atomicMin(&s_tlo[y / R], t0); atomicMax(&s_thi[y / R], t1);
    }
    __syncthreads();
    // tiles within reach of a level's touched columns (own_hi + HALO + 2 >= lo  and  own_lo - HALO - 2 <= hi), as one mask per
    // level, worked out once (the level loop reads one LDS word)
    __shared__ unsigned long long s_tm[LV_MAX_LEVELS + 2];
    for (int L = tid; L < nblk + 2; L += LV_NT) {
        unsigned long long m = 0ull;
        if (L < nblk && s_thi[L] >= s_tlo[L]) {
            const int a = max(0, (s_tlo[L] - (OWN - 1 + HALO + 2) + OWN - 1) / OWN), b = min(ntiles - 1, (s_thi[L] + HALO + 2) / OWN);
            m = ((b - a >= 63) ? ~0ull : ((1ull << (b - a + 1)) - 1ull)) << a;
        }
        s_tm[L] = m;
    }
    __syncthreads();
    LV_AFTER_SETUP
    auto touch_mask = [&](int L) -> LvMask {
        LvMask m;
        m.lo = uni64(s_tm[L]);
        return m;
    };
    // tiles of this slot's residue (t mod P == slot), and of residue 0: no integer division inside the level loop (a lone wave pays
    // ~40 instructions x 4-5 cycles for each: five of them were 2 000 cycles per level)
    unsigned long long res_mine = 0ull;
    for (int t = slot; t < LV_MAX_TILES; t += P) res_mine |= 1ull << t;
    res_mine = uni64(res_mine);
    // the which-th (0, 1) tile of this slot's residue in a set, -1: none
    auto my_tile = [&](const LvMask &A, int which) -> int {
        unsigned long long m = A.lo & res_mine;
        if (which && m) m &= m - 1ull;
        return m ? __builtin_ctzll(m) : -1;
    };
    // does ANY slot have three tiles in the set?  (identical decision in every slot)
    auto any_collision = [&](const LvMask &A) -> bool {
        const int a = A.first(), b = A.last();
        if (a < 0 || b - a < 2 * P) return false;            // a window of 2 P consecutive tiles: at most two per residue
        unsigned long long res_zero = 0ull;                  // (worked out here: the wide window is rare, and two scalar registers held
        for (int t = 0; t < LV_MAX_TILES; t += P) res_zero |= 1ull << t;      //  across the row loop cost it its free compare registers)
        for (int r = 0; r < P; r++)
            if (__popcll(A.lo & (res_zero << r)) > 2) return true;
        return false;
    };
    // the tile of this slot's residue nearest to [a, b] (-1: the slot has no tile in the image)
    auto nearest_tile = [&](int a, int b) -> int {
        const unsigned long long up_m = res_mine & (~0ull << a), dn_m = res_mine & (b >= 63 ? ~0ull : ((1ull << (b + 1)) - 1ull));
        const int up = up_m ? __builtin_ctzll(up_m) : -1, dn = dn_m ? 63 - __builtin_clzll(dn_m) : -1;
        if (up >= 0 && up <= b) return up;                   // inside
        if (up < 0 || up >= ntiles) return dn;
        if (dn < 0) return up;
        return (up - b <= a - dn) ? up : dn;
    };

    // ---- geometry of the tile staged in this wave's registers
    int cur_t = -1, cur_L = -1;
    bool cur_full = false;
    int x0 = 0;
    unsigned lo_off = 0;
    // The per-lane predicates of the staged tile (inside the image? an own column? a tile that reaches over the border?).  As booleans
    // each is a pair of scalar registers held across the whole level loop, and scalar registers are what the row loop runs out of:
    // its compares then go through VCC one after the other (4 hazard nops per row, -8 %; DESIGN.md 4.16).  The rigidity
    // instantiations (LEAN) therefore work them out from x0 where they are needed -- one unsigned compare each, on a copy the
    // compiler cannot see through -- and get the fast row schedule (296 -> 275 us at 16 images); the plain instantiations have the
    // fast schedule WITH the booleans and lose 4 % without them (255 -> 267 us at 8 images: 38 more s_waitcnt in the rows), so
    // they keep them.  tests/test_kernel_budgets.py watches both.
    constexpr bool LEAN = RIG && DELTA == 1 && !RIGM;       // (measured: delta_x 2 with rigidity 440 -> 456 us WITH it, so only here)
    bool in[PX] = {false, false}, own = false, interior = false;
    const bool own_lane = lane >= HL && lane < 64 - HL;
    auto X0 = [&]() -> int { int v = x0; asm volatile("" : "+v"(v)); return v; };
    auto in_k = [&](int k) -> bool { if constexpr (LEAN) return (unsigned) (X0() + k) < (unsigned) w; else return in[k]; };
    auto is_own = [&]() -> bool { if constexpr (LEAN) return own_lane && X0() < w; else return own; };
    auto is_interior = [&]() -> bool {
        if constexpr (LEAN) { const int t0 = __builtin_amdgcn_readfirstlane(X0()); return t0 >= 0 && t0 + TILE <= w; }
        else return interior;
    };
    auto set_tile = [&](int t) {
        x0 = t * OWN - HALO + PX * lane;
        lo_off = (unsigned) min(max(x0, 0), stride - PX);
        if constexpr (!LEAN) {
#pragma unroll
            for (int k = 0; k < PX; k++) in[k] = x0 + k >= 0 && x0 + k < w;
            own = own_lane && x0 < w;
            interior = (x0 - PX * lane >= 0) && (x0 - PX * lane + TILE <= w);
        }
    };
    // the tile that owns this lane's columns when the wave works on tile t, and the lane's first column inside that tile
    auto owner_of = [&](int t) -> int { return lane < HL ? t - 1 : lane >= 64 - HL ? t + 1 : t; };
    const int owner_col = lane < HL ? HALO + PX * lane : lane >= 64 - HL ? PX * (lane - (64 - HL)) : PX * (lane - HL);
    FV q_e[R], q_mo[R], q_ab, q_rf[RIGM ? R : 1];
    LV q_lo[R];
    q_ab[0] = q_ab[1] = INF;
    auto issue_full = [&](int L) {              // inputs of level L for the tile set_tile() chose, and the row above them
        const int ybase = L * R;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const unsigned row = (unsigned) min(ybase + r, h - 1) * (unsigned) stride;
            const unsigned ro = row + lo_off, ro4 = (row << 2) + (lo_off << 2);
            q_e[r] = *(const GFV *) ((const gu8 *) c.en + ro4);
            q_mo[r] = *(const GFV *) ((const gu8 *) c.m + ro4);
            q_lo[r] = *(const GLV *) (c.least + ro);
            if (RIGM) q_rf[RIGM ? r : 0] = *(const GFV *) ((const gu8 *) c.rig + ro4);
        }
        q_ab = *(const GFV *) ((const gu8 *) c.m + ((((unsigned) max(ybase - 1, 0) * (unsigned) stride) + lo_off) << 2));
    };
    float mp[PX] = {INF, INF};
    int acc_l0 = 0, acc_l1 = 0;                 // XOR of old and new m on the level's last row (pixel 0 / 1 of the lane)
    // bit r: the keep rule changed a pixel of this lane on row r (ch[]: a pixel it leaves alone gets mc = mo and the back pointer it had,
    // which is what the level's loads read from the very address its stores go to).  One VGPR, reduced over the own lanes once, after
    // the rows (lv_own_or: the rows some own lane changed; a ballot: the own lanes that changed any row); store_u writes only those
    // rows, from only those lanes, of an interior tile (store_rows, lqrhip_set_levels_store; 0: every row from every lane)
    unsigned chg_rows = 0;
    auto batch_u = [&](int ybase) {
        const int nr = min(R, h - ybase);       // (the image's last level computes surplus rows from copies of its last row)
        chg_rows = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            float mc[PX], e[PX], mo[PX];
            uint32_t lnew = 0;
            bool ch[PX];
#pragma unroll
            for (int k = 0; k < PX; k++) { e[k] = q_e[r][k]; mo[k] = q_mo[r][k]; }
            if constexpr (DELTA == 1 && !RIGM) {
                const float left = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(mp[PX - 1]), DPP_WAVE_SHR1, 0xf, 0xf, true));
                const float right = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(mp[0]), DPP_WAVE_SHL1, 0xf, 0xf, true));
                dp_row<PX, LR, RIG, true, false>(mp, left, right, e, mo, (uint32_t) q_lo[r], in, rig_l, rig_r, mc, lnew, ch);
            } else {
                float nl[DELTA], nr[DELTA], rf[PX];
                lane_reach<PX, DELTA>(mp, nl, nr);
#pragma unroll
                for (int k = 0; k < PX; k++) rf[k] = RIGM ? q_rf[RIGM ? r : 0][k] : 1.0f;
                dp_row_g<PX, DELTA, LR, RIG, RIGM, true, false>(mp, nl, nr, e, mo, (uint32_t) q_lo[r], in, rg, rf, mc, lnew, ch);
            }
            if (r == 0 && ybase == 0) {          // row 0: m = en, whatever stood there (update_mmap's first row)
#pragma unroll
                for (int k = 0; k < PX; k++) mc[k] = e[k];
                lnew = 0;
                if constexpr (LV_TRACK) chg_rows |= 1u;                  // (counted as changed whatever ch says)
            }
            if constexpr (LV_TRACK) {
                // (two selects and one three-way OR: OR-ing the two compares first holds both scalar-register pairs for one more instruction)
                unsigned b0 = ch[0] ? (1u << r) : 0u;
                asm("" : "+v"(b0));
                chg_rows |= b0 | (ch[1] ? (1u << r) : 0u);
            }
            if (r == R - 1) {
                const int msk = (r < nr) ? -1 : 0;
                acc_l0 = (__float_as_int(mc[0]) ^ __float_as_int(mo[0])) & msk;
                acc_l1 = (__float_as_int(mc[1]) ^ __float_as_int(mo[1])) & msk;
            }
#pragma unroll
            for (int k = 0; k < PX; k++) { mp[k] = mc[k]; q_mo[r][k] = mc[k]; }
            q_lo[r] = (LV) lnew;
        }
    };
    // rows: bit r set = row r is written (wave-uniform; the rows past the image's end are never); lanes: the lanes that write (one
    // condition around all the rows; ~0: every lane, those that own nothing to the spare row below the image, as k_dp_tile_p)
    auto store_u = [&](int ybase, unsigned rows, unsigned long long lanes) {
        const bool own_ = is_own();
        const unsigned inc = own_ ? (unsigned) stride : 0u;
        const unsigned so0 = own_ ? (unsigned) ybase * (unsigned) stride + (unsigned) x0 : (unsigned) h * (unsigned) stride + (unsigned) (PX * lane);
        if (__builtin_amdgcn_inverse_ballot_w64(lanes)) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if ((rows >> r) & 1u) {
                    // (the row's offset worked out where it is written, one 24-bit multiply-add -- a stride is far below 2^24: as a
                    // running sum a skipped row pays its two additions)
                    const unsigned so = so0 + __umul24((unsigned) r, inc);
                    *(GFV *) ((gu8 *) c.m + (so << 2)) = q_mo[r];
                    *(GLV *) (c.least + so) = q_lo[r];
                }
            }
        }
    };
    // The barrier that ends level L - 1 (L >= 1): wait until all 2 P words of the slots carry its tag.  With spec_t >= 0 the
    // granules of the row above level L for tile spec_t (the tile this wave expects to have) are fetched in the same poll, so
    // that barrier, active set and halo cost ONE round trip through memory; prev = A_{L-1} says which tiles published.
    // Returns 0, or 1 on a time-out.  fw: this lane's word (lanes < 2 P); g: this lane's granules (valid if spec_t was right).
    auto wait_level = [&](int L, int spec_t, const LvMask &prev, unsigned long long &fw, unsigned long long (&g)[PX]) -> int {
        const unsigned want = ((unsigned) epoch << 10) | (unsigned) L;
        gu64 *fsrc = flagw + (size_t) ((L - 1) & 1) * 2 * LV_PMAX + (lane < 2 * P ? lane : 0);
        const bool need_g = spec_t >= 0 && prev.has(owner_of(spec_t)) && (in_k(0) || in_k(1));
        gu64 *gsrc = gran + ((size_t) ((L - 1) & 1) * ntiles + (need_g ? owner_of(spec_t) : 0)) * OWN + (need_g ? owner_col : 0);
        int sp = 0;
        while (true) {
            const size_t off = (!(dbg & 4) && (sp & 3) != 3) ? near_off : 0;
            fw = __hip_atomic_load(fsrc + off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (spec_t >= 0) {
#pragma unroll
                for (int k = 0; k < PX; k++) g[k] = __hip_atomic_load(gsrc + off + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const bool okf = __all(lane >= 2 * P || (unsigned) (fw >> 32) == want);
            bool okg = true;
#pragma unroll
            for (int k = 0; k < PX; k++) okg &= (unsigned) (g[k] >> 32) == want;
            if (okf && __all(!need_g || okg)) return 0;
            if (dbg & 2) __builtin_amdgcn_s_sleep(16); else if (okf || sp < 8) __builtin_amdgcn_s_sleep(1); else if (sp < 64) __builtin_amdgcn_s_sleep(8); else __builtin_amdgcn_s_sleep(48);
            ++sp;
            if ((sp & 255) == 0 && dev_failed(dev_err)) return 1;
            if (sp > (1 << 18)) { if (lane == 0) dev_fail(dev_err, DEVERR_TILE_TIMEOUT); return 1; }
        }
    };
    // the row above level L (L >= 1) for the tile set_tile() chose: per column from its tile's granules if that tile was active
    // in level L - 1, else from memory (q_ab: nothing changed there).  have_g: g holds this tile's granules already.
    auto row_above = [&](int L, int t, const LvMask &prev, bool have_g, unsigned long long (&g)[PX]) -> int {
        const int u = owner_of(t);
        const bool from_gran = prev.has(u) && (in_k(0) || in_k(1));
        if (!have_g) {
            gu64 *src = gran + ((size_t) ((L - 1) & 1) * ntiles + (from_gran ? u : 0)) * OWN + (from_gran ? owner_col : 0);
            const unsigned want = ((unsigned) epoch << 10) | (unsigned) L;
            int sp = 0;
            while (true) {
                const size_t off = (!(dbg & 4) && (sp & 3) != 3) ? near_off : 0;
#pragma unroll
                for (int k = 0; k < PX; k++) g[k] = __hip_atomic_load(src + off + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bool ok = true;
#pragma unroll
                for (int k = 0; k < PX; k++) ok &= (unsigned) (g[k] >> 32) == want;
                if (__all(ok || !from_gran)) break;
                __builtin_amdgcn_s_sleep(1);                 // (the words were there: the granules are on their way)
                if (++sp > (1 << 16)) { if (lane == 0) dev_fail(dev_err, DEVERR_TILE_TIMEOUT); return 1; }
            }
        }
#pragma unroll
        for (int k = 0; k < PX; k++) mp[k] = !in_k(k) ? INF : from_gran ? __uint_as_float((unsigned) g[k]) : q_ab[k];
        return 0;
    };
    // ---- the level loop.  ONE site each for the loads, the 32 rows and the stores of the staging registers (a second site of any of
    // them makes the register allocator keep two sets: 330 spilled VGPRs).  Wave q receives the barrier of the levels of its
    // parity and takes the slot's FIRST tile there; in the other levels it stores what it holds, takes the slot's SECOND tile if
    // there is one, else prefetches its own next level.  Iteration nblk only closes the last level.
    unsigned n_proc = 0, n_idle = 0, n_sync = 0, n_two = 0;             // (32 bits: scalar registers are what the row loop is short of)
    int hold_L = -1;                            // the level whose (unstored) results sit in this wave's registers
    unsigned hold_rows = 0;                     // ... and its rows that an own lane changed (lv_own_or of chg_rows)
    unsigned long long hold_lanes = 0;          // ... and its own lanes that changed a pixel on any row
    unsigned n_rows = 0;                        // rows stored (low half) and rows skipped (high half): a wave has at most LV_MAX_LEVELS * 32 rows
    static_assert(LV_MAX_LEVELS * 32 < (1 << 16), "two counts of rows in one word");
#ifdef LQR_TIMING
    unsigned long long ltt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long ltprev = __builtin_readcyclecounter();
    const unsigned long long ltstart = ltprev;
#endif
    for (int L = 0; L <= nblk; L++) {
        const bool mine = (L & 1) == q;
        int t = -1;
        bool have_g = false, passed = false;
        unsigned long long g[PX] = {0ull, 0ull};
        LvMask A = {0ull}, A_prev = {0ull};
        if (L > 0) A_prev.lo = uni64(LV_A[(L - 1) & 1]);       // (written before the barrier that ended iteration L - 1)
        LTT(8);
        if (mine) {
            // ---- the barrier of level L - 1 and the active set of level L
            unsigned long long fw = 0;
            A = touch_mask(L);
            passed = true;
            if (L > 0) {
                const int spec_t = (hold_L < 0 && cur_full && cur_L == L && L < nblk && !(dbg & 1)) ? cur_t : -1;
                LJIT(1);
                const int wl_rc = wait_level(L, spec_t, A_prev, fw, g);
                LJIT(2);
                LTT(0);
                if (wl_rc) { LDS_FLAG(s_fail) = 1; passed = false; }
                else if (L < nblk) {
                    // tile `lane` is active in level L iff its own slot's words say "own pixels changed", or the tile to its right says
                    // "left 32 changed", or the tile to its left "right 32 changed" (six words, fetched across the lanes; one ballot)
                    const int wl = (int) (unsigned) fw;
                    bool act = false;
                    unsigned wo[2], wr[2], wlf[2];          // (all six fetches issued before the first is waited for: one LDS latency instead of two)
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        wo[i] = (unsigned) __builtin_amdgcn_ds_bpermute((ix_own + i) << 2, wl);
                        wr[i] = (unsigned) __builtin_amdgcn_ds_bpermute((ix_right + i) << 2, wl);
                        wlf[i] = (unsigned) __builtin_amdgcn_ds_bpermute((ix_left + i) << 2, wl);
                    }
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        act |= (wo[i] & 0x900u) == 0x900u && (int) (wo[i] & 0xffu) == lane;
                        act |= (wr[i] & 0xa00u) == 0xa00u && (int) (wr[i] & 0xffu) == lane + 1;
                        act |= (wlf[i] & 0xc00u) == 0xc00u && (int) (wlf[i] & 0xffu) == lane - 1;
                    }
                    A.lo |= __ballot(act && lane < ntiles);
                    have_g = spec_t >= 0;
                }
            }
            if (lane == 0) { LV_A[L & 1] = A.lo; if (passed) LDS_FLAG(LV_POLLED) = L; }        // level L - 1 may be stored now (not after a time-out)
        } else {
            int spins = 0;
            while (LDS_FLAG(LV_POLLED) < L && LDS_FLAG(s_fail) != 1 && ++spins < (1 << 24)) __builtin_amdgcn_s_sleep(1);
            passed = LDS_FLAG(LV_POLLED) >= L;
            if (passed) A.lo = uni64(LV_A[L & 1]);
            else if (LDS_FLAG(s_fail) != 1) { LDS_FLAG(s_fail) = 1; if (lane == 0) dev_fail(dev_err, DEVERR_TILE_TIMEOUT); }     // (ADVICE r5: never fall through silently)
            LTT(2);
        }
        // ---- STORE: level L - 1 is final and every slot has consumed its inputs
        LTT(1);
        LJIT(3);
        if (hold_L >= 0 && passed) {
            // a row that no own lane changed, and a lane that changed nothing on any row, hold what the loads read from these addresses: not
            // written again (nor do the lanes that own nothing write to the spare row then).  A tile that reaches over the frame's border
            // is written whole: its own lanes can hold pixels outside the frame (+inf, whatever stood there).
            // (x0, and with it is_interior() and is_own(), must still be the HELD tile's here: set_tile runs only in LOAD, below STORE)
            const bool part = LV_TRACK && store_rows && is_interior();
            const int nr = min(R, h - hold_L * R);
            const unsigned all = nr >= 32 ? ~0u : (1u << nr) - 1u;
            const unsigned rows = (unsigned) __builtin_amdgcn_readfirstlane((int) (part ? hold_rows & all : all));      // (a scalar: the rows' branches are scalar ones)
            n_rows += (unsigned) __builtin_popcount(rows) + ((unsigned) __builtin_popcount(all & ~rows) << 16);
            store_u(hold_L * R, rows, uni64(part ? hold_lanes : ~0ull));
            hold_L = -1;
        }
        LTT(3);
        if (L == nblk) break;
        if (mine && passed && any_collision(A)) {
            // three active tiles on one slot: the image stops here (every slot decides the same); rows from 32 L on are the sweep's
            if (slot == 0 && lane == 0) { __hip_atomic_fetch_min(c.flags + FLAG_OVF_ROW, L * R, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); atomicAdd(&LV_STATS[0], 1ull); }
            LDS_FLAG(s_fail) = 2;
            passed = false;
        }
        // (no look at s_fail here: a partner that stops the image or times out in this iteration is not waited for -- what this wave
        // then computes or publishes for level L is never stored nor read, every slot takes the same decision and leaves at the
        // barrier below; an LDS read is ~130 cycles of a level's ~8 700.  The read in front of the word store STAYS: without it
        // the compiler's schedule of the row loop flips to the slow one, DESIGN.md 4.16)
        if (passed) t = my_tile(A, mine ? 0 : 1);
        if (!mine && t < 0 && passed && lane == 0) {       // no second tile: said right away
            const unsigned long long tag = (unsigned long long) (((unsigned) epoch << 10) | (unsigned) (L + 1)) << 32;
            gu64 *fdst = flagw + (size_t) (L & 1) * 2 * LV_PMAX + 2 * slot + 1;
            if (!(dbg & 4)) __hip_atomic_store(fdst + near_off, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(fdst, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // ---- LOAD: the tile of this level if it is not what was prefetched (synchronous), else -- the other wave -- the prefetch for
        // its next level: the tile this slot is expected to have then
        {
            int ld_t = -1, ld_L = L;
            if (t >= 0) {
                if (!(cur_full && cur_t == t && cur_L == L)) { ld_t = t; n_sync++; have_g = false; }
                if (!mine) n_two++;
            } else if (!mine && passed && L + 1 < nblk) {
                LvMask M = touch_mask(L + 1);
                M.lo |= A.lo;
                int pt = my_tile(M, 0);
                if (pt < 0 && M.first() >= 0) { pt = nearest_tile(M.first(), M.last()); if (pt < M.first() - 1 || pt > M.last() + 1 || pt >= ntiles) pt = -1; }
                ld_t = pt; ld_L = L + 1;
                cur_t = -1; cur_L = ld_L; cur_full = false;
            }
            LTT(1);
            LJIT(4);
            if (ld_t >= 0) { set_tile(ld_t); issue_full(ld_L); cur_t = ld_t; cur_L = ld_L; cur_full = true; }
#ifdef LQR_TIMING
            if (t >= 0 && ld_t >= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            LTT(4);
        }
        // ---- the 32 rows of the tile, its last row to the granules
        unsigned word = 0;
        if (t >= 0) {
            n_proc++;
            if (L > 0 && row_above(L, t, A_prev, have_g, g)) LDS_FLAG(s_fail) = 1;
#ifdef LQR_TIMING
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            LTT(5);
            if (!is_interior()) {
                // outside the image the energy AND the old value become +inf (see k_dp_tile_p)
                const bool ik[PX] = {in_k(0), in_k(1)};
#pragma unroll
                for (int r = 0; r < R; r++)
#pragma unroll
                    for (int k = 0; k < PX; k++) { q_e[r][k] = ik[k] ? q_e[r][k] : INF; q_mo[r][k] = ik[k] ? q_mo[r][k] : INF; }
            }
            batch_u(L * R);
            if constexpr (LV_TRACK) { hold_rows = lv_own_or(chg_rows); hold_lanes = __ballot(own_lane && chg_rows != 0u); }
            LTT(6);
            hold_L = L;
            cur_full = false;                    // (the registers hold results now)
            LJIT(5);
            if (L + 1 < nblk && own_lane) {
                gu64 *dst = gran + ((size_t) (L & 1) * ntiles + t) * OWN + PX * (lane - HL);
                const unsigned long long tag = (unsigned long long) (((unsigned) epoch << 10) | (unsigned) (L + 1)) << 32;
#pragma unroll
                for (int k = 0; k < PX; k++) {
                    if (!(dbg & 4)) __hip_atomic_store(dst + near_off + k, tag | __float_as_uint(mp[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_store(dst + k, tag | __float_as_uint(mp[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            const bool chg = own_lane && (acc_l0 | acc_l1) != 0;
            const bool any_o = __any(chg), any_l = __any(chg && lane < 32), any_r = __any(chg && lane >= 32);
            word = 0x800u | (any_o ? 0x100u : 0u) | (any_l ? 0x200u : 0u) | (any_r ? 0x400u : 0u) | (unsigned) t;
        } else if (mine && passed) n_idle++;
        // the slot's word for this wave's tile of the level (its granules were issued above; a reader checks their tags itself)
        LJIT(6);
        if (lane == 0 && (t >= 0 || mine) && LDS_FLAG(s_fail) == 0) {
            const unsigned long long tag = (unsigned long long) (((unsigned) epoch << 10) | (unsigned) (L + 1)) << 32;
            gu64 *fdst = flagw + (size_t) (L & 1) * 2 * LV_PMAX + 2 * slot + (mine ? 0 : 1);
            if (!(dbg & 4)) __hip_atomic_store(fdst + near_off, tag | word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(fdst, tag | word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        LTT(7);
        LV_LEVEL_END
        LTT(8);
        if (LDS_FLAG(s_fail)) return;    // 1: a time-out, results are invalid anyway; 2: the image stopped at this level (level L - 1 was stored above)
    }
#ifdef LQR_TIMING
    if (image == 0 && lane == 0 && slot < 16) { ltt[9] = __builtin_readcyclecounter() - ltstart; for (int i = 0; i < 10; i++) LV_TIME[slot][q][i] = ltt[i]; }
#endif
    if (lane == 0) { atomicAdd(&LV_STATS[2], (unsigned long long) n_proc); atomicAdd(&LV_STATS[3], (unsigned long long) n_idle); if (n_two) atomicAdd(&LV_STATS[4], (unsigned long long) n_two); }
    if (lane == 0 && n_sync) atomicAdd(&LV_STATS[1], (unsigned long long) n_sync);
    if (lane == 0 && n_rows) { atomicAdd(&LV_STATS[5], (unsigned long long) (n_rows & 0xffffu)); atomicAdd(&LV_STATS[6], (unsigned long long) (n_rows >> 16)); }
