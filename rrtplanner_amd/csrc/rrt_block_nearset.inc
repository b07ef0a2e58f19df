// rrt_block_nearset.inc -- textual part of rrt_block_body (rrt_block.h), included inside the function body: the near set of one sample: the record stream of the ball's cells, the parked entries, the walk of the open candidates
// (stream_cells, consume_*, snapshot_parent, finish_parent).
// Not a translation unit of its own: every name it uses is a local of rrt_block_body.

    // ---- the near set of one sample (within :176-181, choose parent :511-521) ----------------------------------------
    // First entry in (cost, index) order with cost < bound and a free line of sight, over the snapshot nodes [0, j0).
    // Three steps, used by one wave on its own (snapshot_parent) or by the waves of a sample's group (owner phase of
    // teams whose members hold fewer samples than waves):
    //   stream_cells   the 16-byte records of the cells the radius ball touches are streamed once (this wave's share of the
    //                  cells).  Every entry whose vcost alone is below the bound is parked in this wave's HBM list
    //                  {index, d2, vcost}; the two cheapest entries are found on the fly under a screen that tightens to
    //                  the second cheapest so far.
    //   consume_list   only when both are blocked: the parked list is priced and the entries still open are tested.
    //   count_tests    the statistics as the sequential loop counts them.
    // Where one wave resolves a sample (BSM == 16) the first 256 entries of its list live in LDS, the rest in HBM: a sample whose
    // two cheapest candidates are blocked reads its list back several times, and that sample is the one its whole block waits
    // for.  Groups of waves (each with a share of the ball) keep their lists in HBM.
    // GQ: the workers of a big pipelined team (a group of waves per sample).  A sample whose two cheapest candidates are blocked puts its
    // open candidates into ONE queue per group, in the half of brec only a committer uses, and all the group's waves test them eight
    // per wave and memory round trip (see the owner phase).  (Round 4 also kept the waves' parked lists there: no gain, dropped.)
    constexpr bool GQ = PIPE && ROLE == ROLE_WORK && BSM < 16;
    constexpr uint32_t OQCAP = (uint32_t)(SB * BREC_WORDS * 8 / 16 / (BSM < 16 ? BSM : 1));
    constexpr bool GLIST = false;
    constexpr bool LDSLIST = BSM >= 16 || GLIST;
    constexpr uint32_t LCAP = BSM >= 16 ? (uint32_t)BLOCK_LIST_CAP : (uint32_t)(SB * BREC_WORDS * 8 / 16 / NWAVE);
    const uint32_t clist_cap = SH == 2 ? (uint32_t)(bv.spill_stride / (2 * NWAVE * (2 * G + 1)))  // the engine sizes the spill area per team member
                                       : (uint32_t)(bv.spill_stride / (2 * NWAVE * (G + (PIPE ? 1 : 0))));
    u32x4 *const clist_base = reinterpret_cast<u32x4 *>(spill) + (size_t)(g * NWAVE) * (size_t)clist_cap;  // this member's 16 lists (and go2goal's scratch)
    u32x4 *const clist = clist_base + (size_t)wave * (size_t)clist_cap;
    RRT_LDS u32x4 *const clist_l =
        GLIST ? (RRT_LDS u32x4 *)&brec[PIPE ? 1 : 0][0] + (size_t)wave * LCAP
              : (RRT_LDS u32x4 *)(smem + (size_t)lds_chunks * CHUNK * sizeof(uint32_t) + (size_t)MAX_CELLS * sizeof(uint32_t)) + (size_t)wave * LCAP;
    auto lget = [&](uint32_t p) -> u32x4 {
        if (LDSLIST && p < LCAP) return clist_l[p];
        return clist[p];
    };
    auto lput = [&](uint32_t p, u32x4 e) {
        if (LDSLIST && p < LCAP) clist_l[p] = e;
        else clist[p] = e;
    };
    auto lput_y = [&](uint32_t p, uint32_t y) {
        if (LDSLIST && p < LCAP) clist_l[p].y = y;
        else clist[p].y = y;
    };
    // the list of another wave of this workgroup (the cooperative test of a blocked sample's candidates)
    RRT_LDS u32x4 *const clist_l0 = clist_l - (size_t)wave * LCAP;  // wave 0's
    auto lget_w = [&](int w, uint32_t p) -> u32x4 {
        if (LDSLIST && p < LCAP) return clist_l0[(size_t)w * LCAP + p];
        return (clist_base + (size_t)w * (size_t)clist_cap)[p];
    };
    auto lput_y_w = [&](int w, uint32_t p, uint32_t y) {
        if (LDSLIST && p < LCAP) clist_l0[(size_t)w * LCAP + p].y = y;
        else (clist_base + (size_t)w * (size_t)clist_cap)[p].y = y;
    };
    // single-precision screen: vcost + sqrt(d2) evaluated in f32 is within a few f32 ulps (< 4e-7 relative) of the f64 value
    auto screen_of = [](double c) -> float { return (float)c * (1.0f + 1.0e-6f) + 4.0e-3f; };
    auto hi_of = [](double c) -> uint32_t { return (uint32_t)((unsigned long long)__double_as_longlong(c) >> 32); };
    const float FINF = __uint_as_float(0x7f800000u);

    // nn_d2 / nn_idx: the nearest of the hits (smallest d2, lowest index among equals; NONE / NONE without a hit).  A hit lies
    // within r_rewire, and every node outside the streamed cells is farther than that: if there is a hit, this IS the nearest
    // node of the whole snapshot (near()[0], rrt.py:150-155) -- the brute-force scan is only needed when the ball is empty.
    // Top2::wave_reduce with the entries' coordinates riding along: lane values (tt, fx1, fx2) -> the wave's two cheapest in tt and
    // their coordinates in (ox1, ox2).  (An index names one record, so one lane holds each winner.)
    auto top2_reduce_xy = [&](Top2 &tt, uint32_t fx1, uint32_t fx2, uint32_t &ox1, uint32_t &ox2) {
        double bc = tt.c1;
        uint32_t bi = tt.i1;
        wave_min_f64_idx(bc, bi);
        const bool own = tt.i1 != NONE && tt.c1 == bc && tt.i1 == bi;
        double sc = own ? tt.c2 : tt.c1;
        uint32_t si = own ? tt.i2 : tt.i1;
        const uint32_t sxy = own ? fx2 : fx1;
        const double sc_l = sc;
        const uint32_t si_l = si;
        wave_min_f64_idx(sc, si);
        const u64 m1 = __ballot(own), m2 = __ballot(si_l != NONE && sc_l == sc && si_l == si);
        ox1 = m1 ? (uint32_t)__builtin_amdgcn_readlane((int)fx1, (int)__builtin_ctzll(m1)) : 0u;
        ox2 = m2 ? (uint32_t)__builtin_amdgcn_readlane((int)sxy, (int)__builtin_ctzll(m2)) : 0u;
        tt.c1 = bc;
        tt.i1 = bi;
        tt.c2 = sc;
        tt.i2 = si;
    };
    // sx: what the stream also knows about its answers from the records themselves (wave-uniform after the call): the coordinates of
    // the two cheapest entries, the coordinates and vcost of the nearest hit
    struct StreamExtra {
        uint32_t x1, x2, nn_xy, nn_vlo, nn_vhi;
    } sx = {0u, 0u, 0u, 0u, 0u};
    auto stream_cells = [&](uint32_t X, int j0, bool check_j0, double bound, double lbc, uint32_t lbi, int part, int nparts, Top2 &tt,
                            uint32_t &nnear_part, uint32_t &nlist, uint32_t &nn_d2, uint32_t &nn_idx) {
        uint32_t fx1 = 0, fx2 = 0, lxy = 0, lvlo = 0, lvhi = 0;  // this lane's: coordinates of its two cheapest, its nearest hit's coordinates and vcost
        const int x = ux(X), y = uy(X);
        const int cx0 = (x - rad < 0 ? 0 : x - rad) >> cshift, cx1 = (x + rad > W - 1 ? W - 1 : x + rad) >> cshift;
        const int cy0 = (y - rad < 0 ? 0 : y - rad) >> cshift, cy1 = (y + rad > H - 1 ? H - 1 : y + rad) >> cshift;
        const int ny = cy1 - cy0 + 1, ncr = (cx1 - cx0 + 1) * ny;
        const float boundf = screen_of(bound);
        const uint32_t boundhi = hi_of(bound);  // vcost >= bound  <=>  its high word > boundhi or (== and ...): `<=` keeps a superset
        tt.init();
        float m1 = FINF, m2 = FINF;  // this lane's two cheapest verified entries, rounded up to f32
        uint32_t hits = 0;
        uint32_t ld2 = NONE, lidx = NONE;  // this lane's nearest hit
        nlist = 0;
        float T = boundf;            // wave-uniform screen, tightens to the second cheapest so far
        uint32_t Thi = hi_of((double)boundf);
        // one 16-byte record per lane: hit test, parking, the screens and the exact price (rrt.py:176-181, :515-518)
        auto eval_record = [&](const u32x4 rc, bool &dirty) {
            const uint32_t d2 = dist2(rc.x, X);
            const bool hit = d2 < r2h && (!check_j0 || rc.y < (uint32_t)j0);
            hits += hit ? 1u : 0u;
            if (hit && (d2 < ld2 || (d2 == ld2 && rc.y < lidx))) {
                ld2 = d2;
                lidx = rc.y;
                lxy = rc.x;
                lvlo = rc.z;
                lvhi = rc.w;
            }
            if (!star) return;  // RRTStandard: the stream only names the nearest node
            // park everything whose vcost alone can be below the bound (the high word of a non-negative f64 is monotone)
            const bool park = hit && rc.w <= boundhi;
            const unsigned long long pm = __ballot(park);
            if (pm == 0) return;
            if (park) {
                const uint32_t pos = nlist + (uint32_t)__builtin_popcountll(pm & ((1ull << lane) - 1ull));
                if (pos < clist_cap) lput(pos, u32x4{rc.y, rc.x, rc.z, rc.w});  // {index, xy, vcost}: whoever tests the entry has its coordinates at hand
            }
            nlist += (uint32_t)__builtin_popcountll(pm);
            // screens, cheapest first; none rejects an entry that belongs to the two cheapest
            const bool pre = park && rc.w <= Thi;
            if (__ballot(pre) == 0) return;
            const double V = __longlong_as_double((long long)(((unsigned long long)rc.w << 32) | rc.z));
            const bool maybe = pre && ((float)V + __builtin_amdgcn_sqrtf((float)d2) < T);
            if (__ballot(maybe) == 0) return;
            if (maybe) {
                const double cn = V + sqrt_u24(d2);
                const bool in = cn < bound && !key_lt(cn, rc.y, lbc, lbi);  // rrt.py:518, strict
                if (in) {
                    // (the coordinates follow the pair as selects of values: written as conditional assignments, fx1 / fx2 were
                    //  stored behind a select of addresses and lived in scratch memory)
                    const bool b1 = key_lt(cn, rc.y, tt.c1, tt.i1);
                    const bool b2 = key_lt(cn, rc.y, tt.c2, tt.i2);
                    fx2 = b1 ? fx1 : (b2 ? rc.x : fx2);
                    fx1 = b1 ? rc.x : fx1;
                    tt.fold(cn, rc.y);
                }
                // (m1, m2) <- the two smallest of {m1, m2, cu}, without branches: written as conditional assignments the pair
                // ends up behind a select of addresses and lives in scratch memory, a store and two loads per priced record
                const float cu = in ? screen_of(cn) : FINF;
                const float lo = __builtin_fminf(m1, cu), hi = __builtin_fmaxf(m1, cu);
                m1 = lo;
                m2 = __builtin_fminf(m2, hi);
            }
            dirty = true;
        };
        auto tighten = [&]() {  // the screen follows (an upper bound of) the wave's second cheapest so far
            const float w1 = wave_min_f32_nonneg(m1);
            const float w2 = wave_min_f32_nonneg(m1 == w1 ? m2 : m1);
            T = w2 < boundf ? w2 : boundf;
            Thi = hi_of((double)T);
        };
        // The records of all touched cells as ONE stream: lane l of a step takes record 64 * step + l of the concatenation of
        // the cells' arrays, so a step is 64 live records whatever the fill of the single cells (a cell holds 10 - 30 nodes
        // at these densities: cell by cell three lanes in four would idle).  Exclusive prefix sum of the fill counts over the
        // lanes; a lane finds its cell by bisection over that prefix (ds_bpermute: the prefix stays in registers).  The cells of
        // the ball's bounding box are taken 64 at a time (one slab unless the radius is far beyond the cell size).
        for (int cbase = 0; cbase < ncr; cbase += 64) {
            uint32_t tcnt = 0, toff = 0;  // lane c: fill count and record offset of cell cbase + c
            if (cbase + lane < ncr) {
                const int ci = cbase + lane, ccx = cx0 + ci / ny, ccy = cy0 + ci % ny, cell = ccx * ncy + ccy;
#ifndef RRT_NO_CELL_CULL
                // a cell beyond the radius holds no hit (the corners of the box)
                const int xl = ccx << cshift, xh = xl + (1 << cshift) - 1, yl = ccy << cshift, yh = yl + (1 << cshift) - 1;
                const int ddx = x < xl ? xl - x : (x > xh ? x - xh : 0), ddy = y < yl ? yl - y : (y > yh ? y - yh : 0);
                tcnt = (uint32_t)(ddx * ddx + ddy * ddy) < r2h ? cellcnt[cell] : 0u;
#else
                tcnt = cellcnt[cell];
#endif
                toff = (uint32_t)cell * (uint32_t)ccap;
            }
            uint32_t incl = tcnt;
            incl = wave_incl_sum_u32(incl);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            const uint32_t pre = incl - tcnt;  // lanes past the last cell hold `total`: never <= a live record number
            int cur_c = 0;  // (SCATTER) the cell the last step ended in
            for (uint32_t base = (uint32_t)part * (64u * CG); base < total; base += (uint32_t)nparts * (64u * CG)) {  // CG steps in flight
                u32x4 rc[CG];
                bool live[CG];
#pragma unroll
                for (int g2 = 0; g2 < CG; ++g2) {
                    const uint32_t idx = base + 64u * (uint32_t)g2 + (uint32_t)lane;
                    uint32_t lo = 0;  // the largest cell c with pre[c] <= idx (an empty cell shares its prefix with its successor)
                    if constexpr (SCATTER) {
                        // one wave walks the whole stream step by step: the cells that begin in this step name themselves in the slot
                        // of their first record (stream_cell_of, rrt_cell_stream.h)
                        const int cv = stream_cell_of((volatile RRT_LDS uint32_t *)L.slots[wave], pre, tcnt, base + 64u * (uint32_t)g2, lane, cur_c);
                        cur_c = __builtin_amdgcn_readlane(cv, 63);
                        lo = (uint32_t)cv;
                    } else {
#pragma unroll
                        for (uint32_t bit = 32; bit != 0; bit >>= 1) {
                            const uint32_t cand = lo + bit;
                            const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(cand << 2), (int)pre);
                            lo = v <= idx ? cand : lo;
                        }
                    }
                    const uint32_t cpre = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lo << 2), (int)pre);
                    const uint32_t coff = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lo << 2), (int)toff);
                    live[g2] = idx < total;
                    rc[g2] = ld_rec<COH>(cellrec + (live[g2] ? coff + (idx - cpre) : 0u));  // {xy, index, vcost}; (record 0 exists: every cell array has a slot)
                }
                bool dirty = false;
#pragma unroll
                for (int g2 = 0; g2 < CG; ++g2) {
                    if (base + 64u * (uint32_t)g2 >= total) continue;
                    if (!live[g2]) rc[g2].x = 0x7fff7fffu;  // never within the radius
                    eval_record(rc[g2], dirty);
                }
                if (dirty) tighten();
            }
        }
        nnear_part = wave_sum_u32(hits);
        top2_reduce_xy(tt, fx1, fx2, sx.x1, sx.x2);
        nn_d2 = ld2;
        nn_idx = lidx;
        wave_min_key_idx(nn_d2, nn_idx);
        {
            const u64 mn = __ballot(lidx != NONE && ld2 == nn_d2 && lidx == nn_idx);
            const int ln_ = mn ? (int)__builtin_ctzll(mn) : 0;
            sx.nn_xy = (uint32_t)__builtin_amdgcn_readlane((int)lxy, ln_);
            sx.nn_vlo = (uint32_t)__builtin_amdgcn_readlane((int)lvlo, ln_);
            sx.nn_vhi = (uint32_t)__builtin_amdgcn_readlane((int)lvhi, ln_);
        }
    };

    // Price this wave's parked entries once and compact the ones still open (cost < bound, key >= lower bound) to the front
    // of the list as {index, cells, cost}, then test them.  A sample behind a wall has dozens of cheaper-but-blocked
    // candidates; two per memory round trip made it the straggler of its block:
    // every open entry is tested, one line of sight per LANE.
    // (wc, wi) = the cheapest passing entry; every entry with a key up to it has been tested and holds its cell count.
    // amin: a single-precision lower bound of the cheapest parked entry that is NOT below the bound (+inf: none).
    auto consume_price = [&](uint32_t X, double bound, double lbc, uint32_t lbi, uint32_t nlist, uint32_t &nval, float &amin) {
        const float boundf = screen_of(bound);
        nval = 0;
        float am = FINF;
        for (uint32_t p0 = 0; p0 < nlist; p0 += 64) {
            const uint32_t p = p0 + (uint32_t)lane;
            u32x4 e = {NONE, 0u, 0u, 0u};
            if (p < nlist) e = lget(p);  // {index, xy, vcost}
            const double V = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
            const uint32_t ed2 = dist2(e.y, X);
            double cn = f64_inf();
            if (p < nlist) {
                const float cf = (float)V + __builtin_amdgcn_sqrtf((float)ed2);
                bool below = false;  // certainly below the bound (such an entry is open, or one of the tested ones under the lower bound)
                if (cf < boundf) {
                    const double c = V + sqrt_u24(ed2);
                    below = c < bound;
                    if (below && !key_lt(c, e.x, lbc, lbi)) cn = c;
                }
                if (!below) am = __builtin_fminf(am, __builtin_fmaxf(cf * (1.0f - 1.0e-6f) - 4.0e-3f, 0.0f));
            }
            const bool open = cn < bound;
            const unsigned long long om = __ballot(open);
            if (open) {  // positions at or below the ones this iteration has read
                const unsigned long long cb = (unsigned long long)__double_as_longlong(cn);
                // {index, xy, cost}: the test of an entry reads its coordinates from the second word and leaves the cells it read there
                lput(nval + (uint32_t)__builtin_popcountll(om & ((1ull << lane) - 1ull)), u32x4{e.x, e.y, (uint32_t)cb, (uint32_t)(cb >> 32)});
            }
            nval += (uint32_t)__builtin_popcountll(om);
        }
        amin = wave_min_f32_nonneg(am);
#if defined(RRT_STAMPS) && defined(RRT_STAMPS_OWNER)
        if (PIPE && g == 1 && t == 0) {
            L.dbg[9] += nval;
            L.dbg[10] += 1;
            L.dbg[11] += nlist;
        }
#endif
    };
    auto consume_walk = [&](uint32_t X, uint32_t nval, double &wc, uint32_t &wi) {
        wc = f64_inf();
        wi = NONE;
        if (nval == 0) return;  // every entry was tried
#ifndef RRT_WALKB
#define RRT_WALKB 8
#endif
        if (nval <= (uint32_t)RRT_WALKB && rad < 64) {
            // a handful (a wave's share of a group's ball, a committer's second search): four segments per memory round trip,
            // 64 cells of each at once, instead of lane-by-lane walks of up to four round trips
            for (uint32_t b0 = 0; b0 < nval; b0 += 4) {
                const uint32_t pq = b0 + (uint32_t)(lane & 3);
                u32x4 e = {NONE, 0u, 0u, 0x7ff00000u};
                if (pq < nval) e = lget(pq);
                const uint32_t axy = pq < nval ? e.y : X;
                uint32_t a4[4];
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) a4[q4] = (uint32_t)__builtin_amdgcn_readlane((int)axy, q4);
                bool ok4[4];
                int cells4[4];
                los_batch_n<4>(og, H, a4, (int)(nval - b0 < 4u ? nval - b0 : 4u), X, lane, ok4, cells4);
                uint32_t res = 0;
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4)
                    if (lane == q4) res = (uint32_t)cells4[q4] | (ok4[q4] ? 0u : 0x80000000u);
                double cn = f64_inf();
                uint32_t ci = NONE;
                if (lane < 4 && pq < nval) {
                    lput_y(pq, res & 0x7fffffffu);
                    if ((res >> 31) == 0u) {
                        cn = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
                        ci = e.x;
                    }
                }
                wave_min_f64_idx(cn, ci);
                if (ci != NONE && key_lt(cn, ci, wc, wi)) {
                    wc = cn;
                    wi = ci;
                }
            }
            return;
        }
        // one line of sight PER LANE, 64 entries at a time, every open entry tested (each lane walks its own segment, 16 cell
        // loads in flight); the answer is the cheapest passing entry.  (Ranking up to 16 open entries and testing them in
        // (cost, index) order, one wave per line of sight and 8 in flight, was measured slower on every bench workload:
        // profiles/r02_experiments.md.)
        // A short list spreads every segment over 2 or 4 lanes (16-cell pieces dealt round-robin), so that up to 16 / 32 open
        // entries are through after one / two memory round trips instead of four.
        for (uint32_t p0 = 0; p0 < nval;) {
            const uint32_t rem = nval - p0;
            // log2 of the lanes per entry (single CUs only: on teams the same split measured slower, profiles/r02_experiments.md)
            const int sh = G > 1 ? 0 : (rem <= 16 ? 2 : (rem <= 32 ? 1 : 0));
            const int S = 1 << sh, part = lane & (S - 1);
            const uint32_t p = p0 + ((uint32_t)lane >> sh);
            const bool have = p < nval;
            u32x4 e = {NONE, 0u, 0u, 0x7ff00000u};
            if (have) e = lget(p);
            const uint32_t axy = have ? e.y : X;
            const rrt_line_t ln = rrt_line_setup(ux(axy), uy(axy), ux(X), uy(X));
            const int L = ln.major;
            constexpr int WU = 16, NOHIT = 0x7fffffff;
            int fb = NOHIT;  // first blocked cell among this lane's pieces
            for (int it = 0;; ++it) {
                const unsigned long long hitm = __ballot(fb != NOHIT);
                const bool grp_hit = ((hitm >> (lane & ~(S - 1))) & ((1ull << S) - 1ull)) != 0;
                if (!__any(!grp_hit && it * S * WU <= L)) break;  // (after a full round every cell below (it S WU) has been read)
                const int k0 = (it * S + part) * WU;
                uint8_t v[WU];
#pragma unroll
                for (int u = 0; u < WU; ++u) {  // unconditional loads (clamped to the segment's last cell)
                    const int kk = (k0 + u) < L ? (k0 + u) : L;
                    int x, y;
                    rrt_line_cell(&ln, kk, &x, &y);
                    v[u] = og[(uint32_t)(x * H + y)];
                }
#pragma unroll
                for (int u = 0; u < WU; ++u)
                    if (fb == NOHIT && k0 + u <= L && v[u] != 0) fb = k0 + u;
            }
            if (sh >= 1) {
                const int o = __builtin_amdgcn_update_dpp(NOHIT, fb, 0xB1, 0xf, 0xf, false);  // lane ^ 1
                fb = o < fb ? o : fb;
            }
            if (sh >= 2) {
                const int o = __builtin_amdgcn_update_dpp(NOHIT, fb, 0x4E, 0xf, 0xf, false);  // lane ^ 2
                fb = o < fb ? o : fb;
            }
            const bool blocked = fb != NOHIT;
            const int cells = blocked ? fb + 1 : L + 1;
            if (have && part == 0) lput_y(p, (uint32_t)cells);  // cells read by this test, for count_tests
            double cn = f64_inf();
            uint32_t ci = NONE;
            if (have && part == 0 && !blocked) {
                cn = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
                ci = e.x;
            }
            p0 += 64u >> sh;
            wave_min_f64_idx(cn, ci);
            if (ci != NONE && key_lt(cn, ci, wc, wi)) {
                wc = cn;
                wi = ci;
            }
        }
    };

    auto consume_list = [&](uint32_t X, double bound, double lbc, uint32_t lbi, uint32_t nlist, double &wc, uint32_t &wi, uint32_t &nval,
                            float &amin) {
        consume_price(X, bound, lbc, lbi, nlist, nval, amin);
        consume_walk(X, nval, wc, wi);
    };

    // The tests the sequential loop makes over a consumed list: up to and including the first passing entry (wc, wi), or all.
    auto count_tests = [&](uint32_t nval, double wc, uint32_t wi, uint32_t &ntests, uint32_t &tcells) {
        uint32_t nt = 0, tcl = 0;
        for (uint32_t p = (uint32_t)lane; p < nval; p += 64) {
            const u32x4 e = lget(p);
            const double cn = __longlong_as_double((long long)(((unsigned long long)e.w << 32) | e.z));
            if (wi == NONE || !key_lt(wc, wi, cn, e.x)) {
                nt += 1;
                tcl += e.y;
            }
        }
        ntests += wave_sum_u32(nt);
        tcells += wave_sum_u32(tcl);
    };

    // One whole wave on its own.  Returns (pc, pi) or (inf, NONE); nnear = |within| over nodes [0, j0).
    auto snapshot_parent = [&](uint32_t X, int j0, bool check_j0, double bound, double &pc, uint32_t &pi, uint32_t &nnear,
                               uint32_t &ntests, uint32_t &tcells, double lbc = -1.0, uint32_t lbi = 0) {
        pc = f64_inf();
        pi = NONE;
        nnear = 0;
        if (r2 == 0) return;
        for (;;) {
            Top2 tt;
            uint32_t nlist = 0;
            uint32_t nd2, nidx;
            stream_cells(X, j0, check_j0, bound, lbc, lbi, 0, 1, tt, nnear, nlist, nd2, nidx);
            if (tt.i1 == NONE) return;
            // the two cheapest, both lines of sight in flight together (rrt.py:519); the second counts only if needed
            bool ok1, ok2;
            int cc1, cc2;
            los_wave2(og, H, node_xy(tt.i1), tt.i2 != NONE ? node_xy(tt.i2) : X, tt.i2 != NONE, X, lane, ok1, cc1, ok2, cc2);
            ntests += 1;
            tcells += (uint32_t)cc1;
            if (ok1) {
                pc = tt.c1;
                pi = tt.i1;
                return;
            }
            if (tt.i2 == NONE) return;
            ntests += 1;
            tcells += (uint32_t)cc2;
            if (ok2) {
                pc = tt.c2;
                pi = tt.i2;
                return;
            }
            lbc = tt.c2;
            lbi = tt.i2 + 1;
            if (nlist > clist_cap) continue;  // the list overflowed: stream the cells again above the new lower bound
            uint32_t nval = 0;
            float am_;
            consume_list(X, bound, lbc, lbi, nlist, pc, pi, nval, am_);
            count_tests(nval, pc, pi, ntests, tcells);
            return;
        }
    };

