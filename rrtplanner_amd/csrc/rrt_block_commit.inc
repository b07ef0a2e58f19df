// rrt_block_commit.inc -- textual part of rrt_block_body (rrt_block.h), included inside the function body: the commit of a block (member 0): the records and the optimistic picture, the fast settle, the parallel rounds, the ordered
// loop, the store pass and the publication; a pipelined committer's prefetch of the next block.
// Not a translation unit of its own: every name it uses is a local of rrt_block_body.

        // ---------------- C: commit (member 0; wave 0, one lane per sample) ----------------
        // References to nodes the commit itself inserts are kept as sample references until the store pass knows every node
        // index: 0x80000000 + 64 set + kk = sample kk of previous block `set` (pipelined teams: oldest first), set = NP: of this block.
        // They compare like the node indices they stand for (above every snapshot index, previous block first, sample order).
        BRec r;
        r.d2s = r.vs = r.los_s = r.flags = r.vbest = r.pstat = r.nnear = 0;
        r.amin = 0.0f;
        r.nnmask = r.rmask = r.dupmask = 0;
#pragma unroll
        for (int p2 = 0; p2 < NPMAX; ++p2) r.pnn[p2] = r.pr[p2] = r.pdup[p2] = 0;
        r.Vs = r.cbest = r.pc = 0.0;
        const u64 lbit = 1ull << lane;
        const u64 ltmask = lbit - 1ull;  // lanes below
        bool acc0 = false, goalhit = false, remote_ok = true;
        u64 harm = 0, acc_exact = 0, fin = 0, fin_acc = 0;  // fin: samples already re-resolved (by the parallel rounds)
        u64 popt = 0, inter = 0, known = 0, aknown = 0;  // parallel rounds: samples whose final result is known, the accepted ones
        bool rounds_on = false;
        bool pbad = false;  // an inserted sample of a previous block affects this sample
        // FASTC (a committer whose records carry the in-flight lines of sight, PL_MAX): psurv = the list entries of PREVIOUS blocks
        // that were inserted and would be tried as this sample's parent before the snapshot's choice (their costs are exact);
        // lists: this sample's list is usable (not void); such a sample is settled lane-parallel, without a round (fast_settle)
        constexpr bool FASTC = PIPE && BSM < 16;
        uint32_t psurv = 0, nent = 0;
        bool lists = false;
        // harm: the earlier samples within r_rewire that, once inserted at their cost, would be tried as this sample's parent
        // before the snapshot's choice: cost-through-it < cost through the snapshot parent (ties go to the lower index = the
        // snapshot, rrt.py:518-521).  A single-precision bound settles almost every pair; bit k is re-evaluated when sample
        // k's cost becomes exact.
        // nc + sqrt(d2) < cb, decided in single precision on either side whenever the margin allows (|error| of the f32 sum
        // < 1e-3 below 2^12 + relative 2e-7): the f64 square root only runs for close calls.
        auto cheaper_through = [&](double nc, uint32_t d2, double cb) -> bool {
            const float f = (float)nc + __builtin_amdgcn_sqrtf((float)d2), cf = (float)cb;
            if (f * (1.0f - 1.0e-6f) - 4.0e-3f >= cf * (1.0f + 1.0e-6f) + 4.0e-3f) return false;
            if (f * (1.0f + 1.0e-6f) + 4.0e-3f < cf * (1.0f - 1.0e-6f) - 4.0e-3f) return true;
            return nc + sqrt_u24(d2) < cb;
        };
        auto harmful = [&](int kk) -> bool { return cheaper_through(newcost[kk], dist2(xq_lds[kk], xv), r.cbest); };
        // Sample k on its own, re-resolved against snapshot + inserted nodes of this block (accepted: acc_k) and of the previous
        // ones (ap[], their count bases jp[]): any wave.  Its record in LDS is replaced by the final one; returns acceptance and cost.
        // Block references: 0x80000000 + 64 * set + kk with set 0 = the oldest previous block ... NP = this block.
        auto resolve_sample = [&](int k, u64 acc_k, const u64 (&ap)[NP], const int (&jp)[NP], bool check_full, bool &acc, double &cbest) {
#if defined(RRT_STAMPS) && !defined(RRT_STAMPS_LIGHT)
            const unsigned long long rs0 = __builtin_amdgcn_s_memtime();
            bool rs_redo = false;
#endif
            BRecWords rku;  // the same record in every lane: kept in scalar registers
            rku.r = brec[bsel][k];
#pragma unroll
            for (int w = 0; w < BREC_WORDS; ++w) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rku.w[w]);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(rku.w[w] >> 32));
                rku.w[w] = ((u64)hi << 32) | lo;
            }
            const BRec &rk = rku.r;
            const uint32_t Xk = (uint32_t)__builtin_amdgcn_readlane((int)xv, k);
            uint32_t vn = rk.vs, d2n = rk.d2s;
            double Vn = rk.Vs;
            bool nocoll = (rk.los_s >> 31) != 0;
            uint32_t cells = rk.los_s & 0x7fffffffu;
            double pc = rk.pc;
            uint32_t pi = (rk.pc < f64_inf()) ? rk.vbest : NONE, nnear = rk.nnear;
            uint32_t ntests = rk.pstat >> 20, tcells = rk.pstat & 0xfffffu;
            const uint32_t xo = (lane < SB) ? xq_lds[lane] : Xk;  // lane kk: sample kk
            const uint32_t dk = dist2(xo, Xk);
            // pipelined: lane kk also stands for sample kk of each previous block (inserted ones: ap[p], exact costs)
            uint32_t xop[NP], dkp[NP];
            u64 pnm[NP], pany = 0;
            bool pdup_hit = false;
#pragma unroll
            for (int p2 = 0; p2 < NP; ++p2) {
                xop[p2] = PIPE ? xqp_lds[p2][lane] : Xk;
                dkp[p2] = dist2(xop[p2], Xk);
                pnm[p2] = PIPE ? (rk.pnn[p2] & ap[p2]) : 0ull;
                pany |= pnm[p2];
                pdup_hit = pdup_hit || (PIPE && (rk.pdup[p2] & ap[p2]) != 0);
            }
            const int snapj = PIPE ? jp[NP - 1] : j0;  // the node count the sample's owner resolved it against
            const bool dup = (rk.flags & 1u) != 0 || (rk.dupmask & acc_k) != 0 || pdup_hit;
            const u64 nm = rk.nnmask & acc_k;
            bool nn_inblock = false;
            if (nm | pany) {  // nearest is an inserted block node: smallest distance, lowest node index on ties (oldest block first)
                nn_inblock = true;
                uint32_t bestd = NONE, axy = Xk;
#pragma unroll
                for (int p2 = NP - 1; p2 >= 0; --p2) {
                    if (pnm[p2] != 0) {
                        uint32_t kdp = (pnm[p2] & lbit) ? dkp[p2] : NONE, kkp = (uint32_t)lane;
                        wave_min_key_idx(kdp, kkp);
                        if (kdp < bestd) {
                            bestd = kdp;
                            vn = 0x80000000u + (uint32_t)(NP - 1 - p2) * 64u + kkp;
                            Vn = prevcost[p2][kkp];
                            axy = (uint32_t)__builtin_amdgcn_readlane((int)xop[p2], (int)kkp);
                        }
                    }
                }
                if (nm != 0) {
                    uint32_t kd = (nm & lbit) ? dk : NONE, kk = (uint32_t)lane;
                    wave_min_key_idx(kd, kk);
                    if (kd < bestd) {
                        bestd = kd;
                        vn = 0x80000000u + (uint32_t)NP * 64u + kk;
                        Vn = newcost[kk];
                        axy = (uint32_t)__builtin_amdgcn_readlane((int)xo, (int)kk);
                    }
                }
                d2n = bestd;
                int cc = 0;
                nocoll = los_wave(og, H, axy, Xk, lane, cc);  // rrt.py:424
                cells = (uint32_t)cc;
            }
            acc = nocoll && !dup && !(check_full && j0 + __builtin_popcountll(acc_k) == n);  // rrt.py:425
            uint32_t vbest = vn;
            cbest = Vn + sqrt_u24(d2n);
            if (acc && star) {
                const double cnear = cbest;
                if (nn_inblock) {
                    // (only when the ball can hold an entry between the two bounds: the owner's lower bound of the cheapest entry at
                    //  or above its bound says so -- nearly never, and the search of the ball is what makes a round slow)
                    if (pi == NONE && (double)rk.amin < cnear && cnear > rk.Vs + sqrt_u24(rk.d2s)) {  // entries between the two bounds were never priced: redo the snapshot
                                                          // part (a parent found below the old bound stays the cheapest: same tests)
                        ntests = 0;
                        tcells = 0;
#if defined(RRT_STAMPS) && !defined(RRT_STAMPS_LIGHT)
                        rs_redo = true;
#endif
                        snapshot_parent(Xk, snapj, true, cnear, pc, pi, nnear, ntests, tcells);
                    } else if (pi != NONE && !(pc < cnear)) {
                        pc = f64_inf();
                        pi = NONE;
                    }
                }
                // inserted block nodes within r_rewire, in (cost, index) order, while they beat the snapshot's best
                u64 rm = rk.rmask & acc_k;
                u64 rmp[NP], rmany = rm;
                nnear += (uint32_t)__builtin_popcountll(rm);
#pragma unroll
                for (int p2 = 0; p2 < NP; ++p2) {
                    rmp[p2] = PIPE ? (rk.pr[p2] & ap[p2]) : 0ull;
                    rmany |= rmp[p2];
                    nnear += (uint32_t)__builtin_popcountll(rmp[p2]);
                }
                while (rmany) {
                    // every lane's cheapest candidate among "its" sample of this block and of the previous ones, then ONE
                    // (cost, reference) minimum over the wave
                    double cn = f64_inf();
                    uint32_t ci = NONE;
                    if (rm & lbit) {
                        const double c = newcost[lane] + sqrt_u24(dk);
                        if (c < cnear) {
                            cn = c;
                            ci = 0x80000000u + (uint32_t)NP * 64u + (uint32_t)lane;
                        }
                    }
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2) {
                        if (PIPE && (rmp[p2] & lbit)) {
                            const double c = prevcost[p2][lane] + sqrt_u24(dkp[p2]);
                            const uint32_t ref = 0x80000000u + (uint32_t)(NP - 1 - p2) * 64u + (uint32_t)lane;
                            if (c < cnear && key_lt(c, ref, cn, ci)) {
                                cn = c;
                                ci = ref;
                            }
                        }
                    }
                    wave_min_f64_idx(cn, ci);
                    if (ci == NONE || !key_lt(cn, ci, pc, pi)) break;
                    const uint32_t kk = ci & 63u;
                    const int set = (int)((ci - 0x80000000u) >> 6);  // 0 .. NP-1: previous blocks, oldest first; NP: this block
                    uint32_t axy = (uint32_t)__builtin_amdgcn_readlane((int)xo, (int)kk);
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2)
                        if (set == NP - 1 - p2) axy = (uint32_t)__builtin_amdgcn_readlane((int)xop[p2], (int)kk);
                    int cc = 0;
                    const bool ok = los_wave(og, H, axy, Xk, lane, cc);  // rrt.py:519
                    ntests += 1;
                    tcells += (uint32_t)cc;
                    if (ok) {
                        pc = cn;
                        pi = ci;
                        break;
                    }
                    if (set == NP) rm &= ~(1ull << kk);
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2)
                        if (set == NP - 1 - p2) rmp[p2] &= ~(1ull << kk);
                    rmany = rm;
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2) rmany |= rmp[p2];
                }
                if (pi != NONE) {
                    vbest = pi;
                    cbest = pc;
                }
            }
            if (lane == 0) {  // the final record of this sample (pad = 1: nnear already counts the block's nodes)
                BRec &f = brec[bsel][k];
                f.vs = vn;
                f.los_s = cells;
                f.cbest = cbest;
                f.vbest = vbest;
                f.pstat = (ntests << 20) | (tcells & 0xfffffu);
                f.nnear = nnear;
                f.flags = rk.flags | 2u;
                newcost[k] = cbest;
            }
#if defined(RRT_STAMPS) && !defined(RRT_STAMPS_LIGHT)
            if (t == 0) {
                dbg[rs_redo ? 10 : 12] += __builtin_amdgcn_s_memtime() - rs0;
                dbg[rs_redo ? 11 : 5] += 1;
            }
#endif
        };

        // FASTC: this lane's sample keeps its nearest vertex and its acceptance; inserted samples in flight (hm: of this block, by sample;
        // ps: of the previous blocks, by list position) are cheaper than its snapshot parent.  The walk of rrt.py:515-521 tries them in
        // (cost, index) order until one has a free line of sight -- the record's list holds every such test's answer, so the lane
        // settles it alone: the first free one becomes the parent; the blocked ones in front of it (or all of them, if none is free) are
        // the tests the walk made.  The sample's record in LDS is replaced by the final one, as a round would.
        auto fast_settle = [&](u64 hm, uint32_t ps, uint32_t ne, u64 rmask_own) {
            if constexpr (FASTC) {
                BRec &f = brec[bsel][lane];
                // candidates by list position: the previous blocks' (ps), and this block's (sample kk sits behind all previous-block
                // entries, at its rank among the earlier samples of this block within r_rewire)
                const uint32_t own0 = ne - (uint32_t)__builtin_popcountll(rmask_own);
                uint32_t cm = ps;
                while (hm) {
                    const int kk = __builtin_ctzll(hm);
                    hm &= hm - 1;
                    cm |= 1u << (own0 + (uint32_t)__builtin_popcountll(rmask_own & lowmask64(kk)));
                }
                auto entry_of = [&](uint32_t pe) -> uint32_t { return (uint32_t)(f.plist[pe >> 2] >> (16u * (pe & 3u))) & 0xffffu; };
                auto entry_cost = [&](uint32_t e16) -> double {
                    const int kk = (int)(e16 & 63u), set = (int)((e16 >> 6) & 3u);
                    if (set == NP) return newcost[kk] + sqrt_u24(dist2(xq_lds[kk], xv));
                    return prevcost[NP - 1 - set][kk] + sqrt_u24(dist2(xqp_lds[NP - 1 - set][kk], xv));
                };
                double bc = f64_inf();
                uint32_t bref = NONE, bcells = 0, nblocked = 0;
                for (uint32_t m = cm; m != 0; m &= m - 1) {
                    const uint32_t e16 = entry_of((uint32_t)__builtin_ctz(m));
                    if ((e16 >> 15) == 0u) {  // blocked
                        nblocked += 1;
                        continue;
                    }
                    const double c = entry_cost(e16);
                    const uint32_t ref = 0x80000000u + (e16 & 0xffu);  // (64 * set + sample: compares like the node index it stands for)
                    if (key_lt(c, ref, bc, bref)) {
                        bc = c;
                        bref = ref;
                        bcells = (e16 >> 8) & 127u;
                    }
                }
                uint32_t nt = bref != NONE ? 1u : 0u, tc = bcells;
                if (nblocked != 0) {  // blocked candidates: the ones in front of the winner (all, without one) were tested
                    for (uint32_t m = cm; m != 0; m &= m - 1) {
                        const uint32_t e16 = entry_of((uint32_t)__builtin_ctz(m));
                        if ((e16 >> 15) != 0u) continue;
                        if (bref == NONE || key_lt(entry_cost(e16), 0x80000000u + (e16 & 0xffu), bc, bref)) {
                            nt += 1;
                            tc += (e16 >> 8) & 127u;
                        }
                    }
                }
                const uint32_t ps0 = f.pstat;
                f.pstat = (((ps0 >> 20) + nt) << 20) | (((ps0 & 0xfffffu) + tc) & 0xfffffu);
                if (bref != NONE) {
                    f.cbest = bc;
                    f.vbest = bref;
                    newcost[lane] = bc;
                }
            }
        };

        // One wave: the SB records of block `ep` from the hand-off area into brec[half].  The block's records are one contiguous
        // piece (64 x BREC_WORDS x 8 bytes), so the wave takes it as whole 16-byte chunks, lane by lane: 80 cache lines instead of
        // 64 x BREC_WORDS separate 8-byte requests to lines another XCD wrote (that fetch was 8 k cycles, profiles/r04_experiments.md).
        auto fetch_records = [&](uint32_t ep, int half) {
            constexpr int NCH = SB * BREC_WORDS * 8 / 16, NIT = (NCH + 63) / 64;  // (the SB records of a block are the front of its 64-record slot)
            static_assert(NCH * 16 == SB * BREC_WORDS * 8, "whole chunks");
            const unsigned char *src = tb + TEAM_OFF_REC + (size_t)(ep % NSLOT) * 64 * BREC_WORDS * 8;
            u32x4 v[NIT];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = it * 64 + lane;
                v[it] = ld_b128_agent(src + 16 * (c < NCH ? c : NCH - 1));
            }
            fence_b128s(v);
            RRT_LDS u32x4 *dst = (RRT_LDS u32x4 *)&brec[half][0];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = it * 64 + lane;
                if (c < NCH) dst[c] = v[it];
            }
        };

        // ---- part A (wave 0): the records, the optimistic picture, and for a pipelined committer the samples that can be
        //      re-resolved side by side ----
        if (wave == 0) {
            if (G > 1) {  // the other members' records: poll the arrival flags, then loads that bypass the L1
                DBGT(7);
                if (PIPE && prefetched) {  // wave 1 fetched them during the last commit
                    remote_ok = uni32(pre_state[bsel]) == 1u;
                } else {
                    remote_ok = team_wait_all(PIPE ? arrive_of(epoch) : t_arrive, 1, PIPE ? G : G - 1, epoch, t_fail, lane);  // (the shift that owns the block)
                    if (PIPE) {
                        if (remote_ok) fetch_records(epoch, bsel);
                    } else if (remote_ok && lane >= BSM && lane < nb) {
                        const gu64 *src = t_rec + (size_t)(epoch % NSLOT) * 64 * BREC_WORDS + (size_t)lane * BREC_WORDS;
                        BRecWords u;
#pragma unroll
                        for (int w = 0; w < BREC_WORDS; ++w) u.w[w] = __hip_atomic_load(src + w, RRT_RLX_AGENT);
                        brec[bsel][lane] = u.r;
                    }
                }
            }
            DBGT(7);
            if (ROLE == ROLE_COMMIT) TSMARK(epoch, 11);
            if (!remote_ok) {
                if (lane == 0) blk.pad0 = 1;
            } else {
                if (lane < nb) r = brec[bsel][lane];  // lane s: sample s
                acc0 = lane < nb && (r.los_s >> 31) != 0 && (r.flags & 1u) == 0;  // accepted if nothing in the block interferes
                goalhit = informed && lane < nb && dist2(xv, xg) < goal_d2;
                if (lane < nb) newcost[lane] = r.cbest;  // optimistic (snapshot-resolved) cost; exact once the sample has committed
                if (PIPE && epoch == 1) {
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2) jp0[p2] = j0;
                }
                if constexpr (FASTC) {
                    nent = (r.flags >> 8) & 0xffu;
                    lists = lane < nb && nent <= (uint32_t)PL_MAX;
                }
                if (lane < nb && acc0) {
                    u64 rm = r.rmask;
                    while (rm) {
                        const int kk = __builtin_ctzll(rm);
                        rm &= rm - 1;
                        if (harmful(kk)) harm |= 1ull << kk;
                    }
                }
                // pipelined: the nodes the previous block inserted are exact; the samples of this block were resolved without them
                if (PIPE && lane < nb) {
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2) {
                        // inserted samples of a previous block that are nearer than this sample's nearest or sit on its cell
                        pbad = pbad || ((r.pnn[p2] | r.pdup[p2]) & A_prev[p2]) != 0;
                        if (acc0) {
                            u64 rm = r.pr[p2] & A_prev[p2];
                            // (FASTC: the list holds the samples within r_rewire oldest block first, sample order within a block: the entry of
                            //  sample kk of previous block p2 sits behind the entries of the older blocks, at its rank among the block's)
                            uint32_t pbase = 0;
#pragma unroll
                            for (int p3 = NP - 1; p3 > p2; --p3) pbase += (uint32_t)__builtin_popcountll(r.pr[p3]);
                            while (rm) {
                                const int kk = __builtin_ctzll(rm);
                                rm &= rm - 1;
                                if (cheaper_through(prevcost[p2][kk], dist2(xqp_lds[p2][kk], xv), r.cbest)) {
                                    if (FASTC && lists) psurv |= 1u << (pbase + (uint32_t)__builtin_popcountll(r.pr[p2] & lowmask64(kk)));
                                    else pbad = true;
                                }
                            }
                        }
                    }
                }
                if (PIPE) {
                    // Which affected samples can be re-resolved at once, each by a wave of its own?  Those whose earlier interacting
                    // samples are all known: at first the ones that keep their snapshot result whatever happens -- not affected
                    // themselves and (transitively) not interacting with an affected one ("tainted"); after a round also the
                    // samples it settled and the ones that turn out to keep their snapshot result given those.
                    popt = __ballot(acc0);
                    inter = (r.nnmask | r.dupmask | r.rmask) & ltmask;
                    const bool slow0 = lane < nb && (((r.nnmask | r.dupmask | harm) & popt & ltmask) != 0 || pbad || psurv != 0);
                    u64 taint = __ballot(slow0);
                    for (int it = 0; it < 6; ++it) {
                        const u64 t2 = taint | __ballot(lane < nb && (inter & taint) != 0);
                        if (t2 == taint) break;
                        taint = t2;
                        if (it == 5) taint = ~0ull;  // no fixed point yet: nothing is known beforehand
                    }
                    known = ~taint;
                    aknown = popt & ~taint;
                    rounds_on = j0 + __builtin_popcountll(popt) < n;  // (not in the run's last block: `j != n` needs exact counts)
                }
            }
        }
        DBGT(1);
        if (PIPE) {  // parallel rounds: wave w re-resolves sample par.list[w]; a round's results make further samples known
            u64 lastmask = 0;
            for (;;) {
                DBGT(2);
                if (wave == 0) {
                    uint32_t cnt = 0;
                    u64 newacc = 0;
                    if (lastmask != 0) {  // the samples the last round settled: final, whatever the ordered loop finds
                        newacc = __ballot(((lastmask >> lane) & 1ull) != 0 && par.accs[lane] != 0u);
                        fin |= lastmask;
                        fin_acc |= newacc;
                        known |= lastmask;
                        aknown |= newacc;
                    }
                    if (remote_ok && rounds_on && (~known & lowmask64(nb)) != 0) {  // (some sample's result is still open)
                        if (newacc != 0) {
                            // their costs are exact now: the later samples they are a candidate parent of look again
                            u64 rm = r.rmask & newacc;
                            if (lane < nb && acc0) {
                                while (rm) {
                                    const int kk = __builtin_ctzll(rm);
                                    rm &= rm - 1;
                                    harm = (harm & ~(1ull << kk)) | (harmful(kk) ? (1ull << kk) : 0ull);
                                }
                            }
                        }
                        u64 L0 = 0;
                        for (;;) {  // samples whose earlier interacting samples are all known: unaffected -> known; affected -> this round
                            const bool ready = lane < nb && (known & lbit) == 0 && (inter & ~known) == 0;
                            const bool hd = (harm & aknown & ltmask) != 0;  // an inserted sample of this block would be tried before the snapshot's choice
                            // sd: the sample has to be resolved again (a round); fd: only its parent is in question and the record holds
                            // every line of sight that question needs -- settled here, by its lane
                            const bool sd = ((r.nnmask | r.dupmask) & aknown & ltmask) != 0 || pbad || (goalhit && acc0) || (hd && !(FASTC && lists));
                            const bool fd = FASTC && !sd && (hd || psurv != 0);
                            const u64 cb = __ballot(ready && !sd && !fd);
                            const u64 fb = FASTC ? __ballot(ready && fd) : 0ull;
                            if (cb == 0 && fb == 0) {
                                L0 = __ballot(ready && sd && !goalhit);  // (a goal hit ends or cuts the block: ordered loop)
                                break;
                            }
                            known |= cb;
                            aknown |= cb & popt;
                            if constexpr (FASTC) {
                                if (fb != 0) {
                                    if (ready && fd) fast_settle(harm & aknown & ltmask, psurv, nent, r.rmask);
                                    fin |= fb;  // final, like the samples a round settled (all of them were accepted at the snapshot and stay so)
                                    fin_acc |= fb;
                                    known |= fb;
                                    aknown |= fb;
#ifdef RRT_STAMPS
                                    if (t == 0) dbg[13] += (unsigned long long)__builtin_popcountll(fb) << 32;  // (upper half: samples settled by their lanes)
#endif
                                    // their costs are exact now: the later samples they are a candidate parent of look again
                                    u64 rm = r.rmask & fb;
                                    if (lane < nb && acc0 && (known & lbit) == 0) {
                                        while (rm) {
                                            const int kk = __builtin_ctzll(rm);
                                            rm &= rm - 1;
                                            harm = (harm & ~(1ull << kk)) | (harmful(kk) ? (1ull << kk) : 0ull);
                                        }
                                    }
                                }
                            }
                        }
                        // the first CW of them (one per wave of this workgroup), in sample order: lane k knows its place in the list
                        const uint32_t place = (uint32_t)__builtin_popcountll(L0 & ltmask);
                        const bool listed = ((L0 >> lane) & 1ull) != 0 && place < (uint32_t)CW;
                        if (listed) par.list[place] = (uint32_t)lane;
                        lastmask = __ballot(listed);
                        cnt = (uint32_t)__builtin_popcountll(lastmask);
#ifdef RRT_STAMPS
                        if (t == 0) dbg[6] += cnt;
                        if (t == 0 && cnt != 0) dbg[13] += 1;
#endif
                        if (lane == 0 && cnt != 0) {
                            par.acc_opt = aknown;
#pragma unroll
                            for (int p2 = 0; p2 < NP; ++p2) {
                                par.aprev[p2] = A_prev[p2];
                                par.jp0[p2] = jp0[p2];
                            }
                        }
                    }
                    if (lane == 0) par.count = cnt;
                }
                DBGT(8);
                __syncthreads();
                const uint32_t cnt = uni32(par.count);
                if (cnt == 0) break;
                if ((uint32_t)wave < cnt) {
                    const int k = (int)uni32(par.list[wave]);
                    bool acc;
                    double cb;
                    u64 ap[NP];
                    int jp[NP];
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2) {
                        ap[p2] = uni64(par.aprev[p2]);
                        jp[p2] = unis32(par.jp0[p2]);
                    }
                    resolve_sample(k, uni64(par.acc_opt) & lowmask64(k), ap, jp, false, acc, cb);
                    if (lane == 0) par.accs[k] = acc ? 1u : 0u;
                }
                __syncthreads();
            }
        }
        DBGT(2);
        // A pipelined committer's last two waves meanwhile fetch the next block: its records (workers that run ahead have handed them
        // over already) and its samples.  Only an Informed block can end early, so the next block is known.  (Behind the rounds, not
        // at the top of the block: there the last records are still ~9 k cycles away and the rounds' first barrier waits for this
        // wave -- measured, profiles/r04_experiments.md.)
        const bool pre_next = PIPE && (!informed || LAG >= 2) && i0 + nb < n;
        const bool pre_smp = pre_next && !informed;
        if (PIPE && wave == CW - 1 && pre_next) {
#ifdef RRT_STAMPS
            const unsigned long long pf0 = __builtin_amdgcn_s_memtime();
#endif
            TSMARK(epoch, 2);
#if defined(RRT_STAMPS) && !defined(RRT_STAMPS_LIGHT)
            bool ok = true;  // team_wait_all, counting who is late
            {
                const u64 t0w = wall_clock64();
                u64 lastmiss = 0;
                for (;;) {
                    const bool mine = lane < G ? __hip_atomic_load(arrive_of(epoch + 1) + 32 * (1 + lane), RRT_RLX_AGENT) >= epoch + 1 : true;
                    const u64 miss = __ballot(!mine);
                    if (miss == 0) break;
                    if (!mine) D->dbg2[lane] += 1;
                    lastmiss = miss;
                    if (__hip_atomic_load(t_fail, RRT_RLX_AGENT) != 0u || wall_clock64() - t0w > TEAM_TIMEOUT_TICKS) {
                        ok = false;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                if (lastmiss != 0 && (lastmiss & (lastmiss - 1)) == 0 && ((lastmiss >> lane) & 1ull)) D->dbg2[64 + lane] += 1;
            }
#else
            const bool ok = team_wait_all(arrive_of(epoch + 1), 1, G, epoch + 1, t_fail, lane);
#endif
#ifdef RRT_STAMPS
            const unsigned long long pf1 = __builtin_amdgcn_s_memtime();
#endif
            TSMARK(epoch, 3);
            if (ok) fetch_records(epoch + 1, bsel ^ 1);
            TSMARK(epoch, 4);
            if (lane == 0) pre_state[bsel ^ 1] = ok ? 1u : 2u;
#ifdef RRT_STAMPS
            if (lane == 0) dbg[14] += ((__builtin_amdgcn_s_memtime() - pf0) & 0xffffffffull) | ((pf1 - pf0) << 32);  // (upper half: the wait for the flags)
#endif
        }
        if (PIPE && wave == CW - 2 && pre_smp) {  // (the samples: a wave of their own, one memory round trip less in a row)
            const int in = i0 + nb;
            const int nbn = (n - in) < SB ? (n - in) : SB;
            if (lane < nbn) xq_next[bsel ^ 1][lane] = at32(samples, (uint32_t)(in + lane));
        }
        // ---- part B (wave 0): decide in order, store, publish ----
        if (wave == 0 && remote_ok) {
            int cur = 0;
            bool cut = false;
            // ---- C1: decide.  Runs of samples that keep their snapshot result are only marked; a sample that can be affected is
            //      re-resolved on its own and its record in LDS replaced by the final one.  Nothing is stored to HBM yet: the
            //      decisions only read the snapshot and the block's samples. ----
            const double c_ell0 = c_ell;
            const bool myacc0 = (fin & lbit) ? (fin_acc & lbit) != 0 : acc0;  // a settled sample's acceptance is known
            while (cur < nb && !cut) {
                const u64 pend = __ballot(myacc0 && lane >= cur);
                const u64 Aopt = acc_exact | (pend & ltmask);  // exact below cur, optimistic in [cur, lane)
                // A sample keeps its snapshot result unless an earlier inserted sample of the block is nearer than its nearest,
                // sits on its cell, or (accepted samples only) is a harmful candidate parent.
                const bool slow = lane >= cur && lane < nb && (fin & lbit) == 0 &&
                                  (((r.nnmask | r.dupmask | harm) & Aopt) != 0 || pbad || psurv != 0 || (goalhit && acc0));
                const unsigned long long bad = __ballot(slow);
                const int k0 = bad ? (int)__builtin_ctzll(bad) : nb;
                acc_exact |= pend & lowmask64(k0) & ~lowmask64(cur);
                cur = k0;
                if (cur >= nb) break;
                // ---- sample `cur` on its own ----
                {
                    const int k = cur;
                    const int jk = j0 + __builtin_popcountll(acc_exact);  // nodes when this sample is tried
                    const uint32_t Xk = (uint32_t)__builtin_amdgcn_readlane((int)xv, k);
                    bool acc;
                    double cbest;
                    resolve_sample(k, acc_exact, A_prev, jp0, true, acc, cbest);

                    if (acc) {
                        if (informed && dist2(Xk, xg) < goal_d2) {  // rrt.py:744-745
                            const bool first = nsoln == 0;
                            nsoln++;
                            if (cbest < cmin_soln) {  // np.argmin keeps the first minimum (rrt.py:632)
                                cmin_soln = cbest;
                                vbest_soln = jk;
                                c_ell = cmin_soln + sqrt_u24(dist2(xg, Xk));
                                cut = true;  // the ellipse changed: later samples of this block are stale (rrt.py:698-700)
                            }
                            if (first) cut = true;  // sampling switches from free space to the ellipse (rrt.py:695)
                        }
                        acc_exact |= 1ull << k;
                        const bool redo = lane > k && lane < nb && acc0 && ((r.rmask >> k) & 1ull) != 0;  // its cost is exact now
                        if (__ballot(redo) != 0 && redo) harm = (harm & ~(1ull << k)) | (harmful(k) ? (1ull << k) : 0ull);
                    }
                    cur = k + 1;
                }
            }
            DBGT(3);
            // ---- C2: commit samples [0, cur) in one lane-parallel pass ----
            {
                if (j0 + __builtin_popcountll(acc_exact) > n) acc_exact &= ~(1ull << (63 - __builtin_clzll(acc_exact)));  // rrt.py:425 `j != n`: only the run's last sample
                const bool inr = lane < cur;
                const BRec f0 = brec[bsel][lane];  // (lanes at and above `cur`: read, never used)
                BRec f = f0;
                // sample references -> node indices, now that every acceptance is known
                auto node_of = [&](uint32_t v) -> uint32_t {
                    if (v == NONE || (v & 0x80000000u) == 0) return v;
                    const int kk = (int)(v & 63u);
                    const int set = (int)((v - 0x80000000u) >> 6);  // 0 .. NP-1: previous blocks, oldest first; NP: this block
                    uint32_t node = (uint32_t)j0 + (uint32_t)__builtin_popcountll(acc_exact & lowmask64(kk));
#pragma unroll
                    for (int p2 = 0; p2 < NP; ++p2)
                        if (set == NP - 1 - p2) node = (uint32_t)jp0[p2] + (uint32_t)__builtin_popcountll(A_prev[p2] & lowmask64(kk));
                    return node;
                };
                f.vs = node_of(f.vs);
                f.vbest = node_of(f.vbest);
                const bool myacc = inr && ((acc_exact >> lane) & 1ull) != 0;
                const int jmine = j0 + __builtin_popcountll(acc_exact & ltmask);  // j as this sample sees it
                if (inr) {
                    statred[lane * 5 + 0] += (unsigned long long)jmine;
                    statred[lane * 5 + 1] += (unsigned long long)(f.los_s & 0x7fffffffu);
                    if (logs) {
                        const size_t o = (size_t)q * bv.n_cap + i0 + lane;
                        bv.nearest_log[o] = (int32_t)f.vs;
                        bv.accept_log[o] = (uint8_t)myacc;
                        bv.cbest_log[o] = ell ? c_ell0 : __longlong_as_double(0x7ff8000000000000ll);
                        bv.j_log[o] = jmine;
                    }
                }
                if (myacc) {
                    if (star) {
                        uint32_t nprevnear = 0;
#pragma unroll
                        for (int p2 = 0; p2 < NP; ++p2) nprevnear += PIPE ? (uint32_t)__builtin_popcountll(f.pr[p2] & A_prev[p2]) : 0u;
                        statred[lane * 5 + 2] += (f.flags & 2u) ? f.nnear
                                                       : f.nnear + (uint32_t)__builtin_popcountll(f.rmask & acc_exact & ltmask) + nprevnear;
                        statred[lane * 5 + 4] += f.pstat >> 20;
                        statred[lane * 5 + 3] += f.pstat & 0xfffffu;
                    }
                    const uint32_t cellbit = (uint32_t)ux(xv) * (uint32_t)H + (uint32_t)uy(xv);
                    if (jmine < lds_nodes) nodes_lds[jmine] = xv;
                    const unsigned long long cb = (unsigned long long)__double_as_longlong(f.cbest);
                    if (G > 1) {
                        // a team: exactly the bytes the other members will read go out write-through (agent-scope stores), so
                        // that publishing the block needs no L2 write-back, only the wait for these stores
                        __hip_atomic_store((gu32 *)&at32(nodes_g, (uint32_t)jmine), xv, RRT_RLX_AGENT);
                        __hip_atomic_store((gu64 *)&at32(vcost, (uint32_t)jmine), (u64)cb, RRT_RLX_AGENT);
                        __hip_atomic_store((gu32 *)&at32(parent, (uint32_t)jmine), f.vbest, RRT_RLX_AGENT);
                    } else {
                        at32(nodes_g, (uint32_t)jmine) = xv;
                        at32(vcost, (uint32_t)jmine) = f.cbest;
                        at32(parent, (uint32_t)jmine) = (int32_t)f.vbest;
                    }
                    atomicOr(&at32(bitmap, cellbit >> 5), 1u << (cellbit & 31));  // rrt.py:426
                    if (cells_on) {  // the node's cell record: near set of RRT*, nearest-neighbour search
                        const int c = cell_of(xv);
                        const uint32_t slot = __hip_atomic_fetch_add(&cellcnt[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        u32x4 rc = {xv, (uint32_t)jmine, (uint32_t)cb, (uint32_t)(cb >> 32)};
                        if (G > 1) {  // (a reader takes a record only after the go flag: two 8-byte halves cannot be seen torn)
                            gu64 *dst = (gu64 *)&at32(cellrec, (uint32_t)c * (uint32_t)ccap + slot);
                            __hip_atomic_store(dst, ((u64)jmine << 32) | xv, RRT_RLX_AGENT);
                            __hip_atomic_store(dst + 1, (u64)cb, RRT_RLX_AGENT);
                        } else {
                            at32(cellrec, (uint32_t)c * (uint32_t)ccap + slot) = rc;
                        }
                    }
                }
                j = j0 + __builtin_popcountll(acc_exact);
                if (PIPE) {  // this block becomes the (newest) previous one
#pragma unroll
                    for (int p2 = NP - 1; p2 > 0; --p2) {
                        xqp_lds[p2][lane] = xqp_lds[p2 - 1][lane];
                        prevcost[p2][lane] = prevcost[p2 - 1][lane];
                        A_prev[p2] = A_prev[p2 - 1];
                        jp0[p2] = jp0[p2 - 1];
                    }
                    xqp_lds[0][lane] = xv;
                    prevcost[0][lane] = f.cbest;
                    A_prev[0] = acc_exact;
                    jp0[0] = j0;
                }
            }
            i = i0 + cur;
            if (lane == 0) {
                BlkState b;
                b.i = i;
                b.j = j;
                b.nsoln = nsoln;
                b.vbest_soln = vbest_soln;
                b.pad0 = 0;
                b.pad1 = (PIPE && cut) ? ST_FLAG_RESTART : 0;
                b.cmin_soln = cmin_soln;
                b.c_ell = c_ell;
                blk = b;
            }
            // state first (write-through), then everything the commit stored, then the flag
            DBGT(9);
            if (G > 1) publish_state(epoch, (PIPE && cut) ? ST_FLAG_RESTART : 0);
            if (ROLE == ROLE_COMMIT) TSMARK(epoch, 1);
            DBGT(4);
        }
