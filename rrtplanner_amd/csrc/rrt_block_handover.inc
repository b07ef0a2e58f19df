// rrt_block_handover.inc -- textual part of rrt_block_body (rrt_block.h), included inside the function body: the hand-over between the members of a team: records to the committer, the commit's state and new vertices back.
// Not a translation unit of its own: every name it uses is a local of rrt_block_body.

        // ---------------- a pipelined team's workers: hand the records of block s over and, instead of waiting for its commit,
        //                  take the nodes of the commit of block s - 1 and go on with block s + 1 ----------------
        if (PIPE && g > 0) {
#ifdef RRT_STAMPS
            if (t == 0 && g <= 64) {
                const unsigned long long dres = __builtin_amdgcn_s_memtime() - wres0;
                if (dres > 26000ull) D->dbg2[192 + g - 1] += 1;
                if (dres > 32000ull) D->dbg2[256 + g - 1] += 1;
                if (dres > 40000ull) D->dbg2[320 + g - 1] += 1;
                if (dres > D->dbg2[384 + g - 1]) D->dbg2[384 + g - 1] = dres;
            }
#endif
            DBGT(0);
            // this worker's next block: the one behind this one, or (two shifts) the one behind the other shift's, which is full if ours exists
            const int i_next = i0 + nb + (SH - 1) * SB;
            const bool more = i_next < n;
            const uint32_t ep_take = epoch + (uint32_t)(SH - 1) - (uint32_t)LAG;  // the commit the next block is resolved against
            const bool take = (int)epoch + SH - 1 > LAG && (more || pipe_inf);  // there is a commit to take (an Informed worker always looks)
            if (wave == 0) {
                if (!void_blk) {
                    const RRT_LDS u64 *src = (const RRT_LDS u64 *)&brec[0][wg * BSM];
                    gu64 *dst = t_rec + (size_t)(epoch % NSLOT) * 64 * BREC_WORDS + (size_t)wg * BSM * BREC_WORDS;
                    for (int w = lane; w < BSM * BREC_WORDS; w += 64) __hip_atomic_store(dst + w, src[w], RRT_RLX_AGENT);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the storing wave drains, then signals
                }
                if (lane == 0) __hip_atomic_store(my_arrive(), epoch, RRT_RLX_AGENT);
                if (g == 1) TSMARK(epoch, 5);
                if (g == 8) TSMARK(epoch, 8);
            }
            // The commit this worker has to take next is some way off: meanwhile it scans the nodes it already has for the NEXT
            // block's samples (known: only an Informed block can be cut short); after the take only the steps that hold new
            // nodes are left.
            pre_i = -1;
            if (!informed && more && !grid_nn) {
                pre_i = i_next;
                pre_j = j0;
                const int nbn = (n - pre_i) < SB ? (n - pre_i) : SB;
                pre_xv = lane < nbn ? at32(samples, (uint32_t)(pre_i + lane)) : 0u;
                uint32_t xsn[BSA];
#pragma unroll
                for (int k = 0; k < BSA; ++k) {
                    const int sk = wg * BSM + k;
                    uint32_t X = (uint32_t)__builtin_amdgcn_readlane((int)pre_xv, sk);
                    if (sk >= nbn) X = (uint32_t)__builtin_amdgcn_readlane((int)pre_xv, 0);
                    xsn[k] = X << 4;
                    pre_best[k] = NONE;
                }
                scan_steps(0, pre_j / CHUNK, pre_j, xsn, pre_best);
            }
            if (wave == 0) {
                bool ok = true;
                // the next block's "previous" samples (a block that has a successor is full).  Written in front of the wait for go, not
                // behind it as before, for every pipelined team: the last reads of xqp_lds are the owner phase's, in front of the barrier
                // that precedes this hand-over, and the next ones are behind the barrier below, so the interval is the same and the
                // stores no longer stand between go and the take
                if (SH == 2) {  // this block, and in front of it the other shift's, which comes from the sample stream
                    xqp_lds[NP - 1][lane] = xv;
                    xqp_lds[0][lane] = more ? at32(samples, (uint32_t)(i0 + nb + lane)) : 0u;
                } else {
#pragma unroll
                    for (int p2 = NP - 1; p2 > 0; --p2) xqp_lds[p2][lane] = xqp_lds[p2 - 1][lane];
                    xqp_lds[0][lane] = xv;
                }
                DBGT(1);
                if (take) {
                    ok = team_wait(t_go, ep_take, t_fail);
                    if (g == 1) TSMARK(epoch, 6);
                    if (g == 8) TSMARK(epoch, 9);
                    DBGT(2);
                    if (!grid_nn) {  // (the scan of the node array reads it with plain loads)
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // ONE acquire per workgroup: drops this CU's L1
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // ... and holds the barrier until it has completed
                    }
                }
                if (lane == 0) blk.pad0 = ok ? 0 : 1;
            }
            __syncthreads();
            if (blk.pad0 != 0) {
                team_failed = true;
                break;
            }
            i = i_next;
            nprev = void_blk ? 0 : (nprev + SH < NP ? nprev + SH : NP);  // (follows the block number, not the worker's own count)
            if (take) {
                BlkWords u;
#pragma unroll
                // (two shifts: the state of epoch b - 1 only.  The slot of epoch b - 2 may hold epoch b + 1 by now, which needs only the other
                //  shift's records; this one is rewritten by epoch b + 2, which needs this worker's own.  Up to 2 SB new nodes.)
                for (int w = 0; w < 5; ++w) u.w[w] = __hip_atomic_load(t_state + (size_t)(ep_take % NSLOT) * 8 + w, RRT_RLX_AGENT);
                if (pipe_inf && ((u.b.pad1 & ST_FLAG_STOP) != 0 || u.b.i >= n)) break;  // the run is over (or waits for the host)
                const int jn = unis32(u.b.j);
                if (t < jn - j0) {  // at most SH * SB new nodes (one pass of the 1 024 threads): append them to this CU's node cache and cell fill counts
                    const uint32_t Xn = ld_u32<COH>(&at32(nodes_g, (uint32_t)(j0 + t)));
                    if (j0 + t < lds_nodes) nodes_lds[j0 + t] = Xn;
                    if (cells_on) __hip_atomic_fetch_add(&cellcnt[cell_of(Xn)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                j = jn;
                if (pipe_inf) {
                    nsoln = unis32(u.b.nsoln);
                    vbest_soln = unis32(u.b.vbest_soln);
                    cmin_soln = unif64(u.b.cmin_soln);
                    c_ell = unif64(u.b.c_ell);
                    if ((u.b.pad1 & ST_FLAG_RESTART) != 0) {
                        // that commit ended early or moved the ellipse: the block just handed over is void; wait for the
                        // committer's empty turn, then start over from the true state without a previous block
                        __syncthreads();  // (every wave has read blk.pad0)
                        if (wave == 0) {
                            const bool ok2 = team_wait(t_go, epoch, t_fail);
                            if (lane == 0) blk.pad0 = ok2 ? 0 : 1;
                        }
                        __syncthreads();
                        if (blk.pad0 != 0) {
                            team_failed = true;
                            break;
                        }
                        BlkWords u2;
#pragma unroll
                        for (int w = 0; w < 5; ++w) u2.w[w] = __hip_atomic_load(t_state + (size_t)(epoch % NSLOT) * 8 + w, RRT_RLX_AGENT);
                        if ((u2.b.pad1 & ST_FLAG_STOP) != 0) break;
                        i = unis32(u.b.i);
                        nprev = 0;
                    }
                }
            }
            __syncthreads();
            if (wave == 0 && g == 1) TSMARK(epoch, 7);
            if (wave == 0 && g == 8) TSMARK(epoch, 10);
            DBGT(3);
            epoch += (uint32_t)(SH - 1);  // (the other shift's block)
            continue;
        }

        // ---------------- team members g > 0: hand the records over, wait for the commit, take the new nodes ----------------
        if (G > 1 && !PIPE && g > 0) {
            if (wave == 0) {
                // this member's 16 records, LDS -> HBM: whole 128-byte lines per wave instruction, write-through (8-byte
                // stores of single lanes are partial-line fabric writes and delay everything queued behind them)
                const RRT_LDS u64 *src = (const RRT_LDS u64 *)&brec[0][g * BSM];
                for (int w = lane; w < BSM * BREC_WORDS; w += 64) __hip_atomic_store(t_rec + (size_t)g * BSM * BREC_WORDS + w, src[w], RRT_RLX_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the storing wave drains, then signals
                if (lane == 0) __hip_atomic_store(t_arrive + 32 * g, epoch, RRT_RLX_AGENT);
            }
            pre_i = -1;
            if (!informed && i0 + nb < n && !grid_nn) {  // the next block's samples are known (only an Informed block can be cut short)
                pre_i = i0 + nb;
                pre_j = j0;
                const int nbn = (n - pre_i) < SB ? (n - pre_i) : SB;
                pre_xv = lane < nbn ? samples[pre_i + lane] : 0u;
                uint32_t xsn[BSA];
#pragma unroll
                for (int k = 0; k < BSA; ++k) {
                    const int sk = g * BSM + k;
                    uint32_t X = (uint32_t)__builtin_amdgcn_readlane((int)pre_xv, sk);
                    if (sk >= nbn) X = (uint32_t)__builtin_amdgcn_readlane((int)pre_xv, 0);
                    xsn[k] = X << 4;
                    pre_best[k] = NONE;
                }
                scan_steps(0, pre_j / CHUNK, pre_j, xsn, pre_best);  // whole steps below the first one the commit can touch
            }
            if (wave == 0) {
                const bool ok = team_wait(t_go, epoch, t_fail);
                if (!grid_nn) {
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // ONE acquire per workgroup: drops this CU's L1
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // ... and holds the barrier until it has completed
                }
                if (lane == 0) blk.pad0 = ok ? 0 : 1;
            }
            __syncthreads();
            if (blk.pad0 != 0) {
                team_failed = true;
                break;
            }
            BlkWords u;
#pragma unroll
            for (int w = 0; w < 5; ++w) u.w[w] = __hip_atomic_load(t_state + w, RRT_RLX_AGENT);  // vector loads past the L1
            i = unis32(u.b.i);
            nsoln = unis32(u.b.nsoln);
            vbest_soln = unis32(u.b.vbest_soln);
            cmin_soln = unif64(u.b.cmin_soln);
            c_ell = unif64(u.b.c_ell);
            const int jn = unis32(u.b.j);
            if (t < jn - j0) {  // at most SB new nodes: append them to this CU's node cache and cell fill counts
                const uint32_t Xn = ld_u32<COH>(&at32(nodes_g, (uint32_t)(j0 + t)));
                if (j0 + t < lds_nodes) nodes_lds[j0 + t] = Xn;
                if (cells_on) __hip_atomic_fetch_add(&cellcnt[cell_of(Xn)], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            j = jn;
            __syncthreads();
            continue;
        }
