// k_pivot_wave2.inc -- TWO waves per matrix (included by k_pivot_wave.hip, configuration pv_wave2).
//
// Reference: as k_pivot_wave.hip -- factorize_bump (src/lu/factorize_bump.rs:12-49), pivot_small (src/lu/pivot.rs:460-833).
//
// Why: one wave per matrix (k_pivot_loop_wave) is the right shape while registers limit how many matrices a CU holds.
// Bases of the 100k size are limited by HBM CAPACITY instead (1536 handles fill the card, 6 waves per CU where 16 fit):
// the idle wave slots are given to the matrices that are there.  The columns of a pivot_small are independent of each
// other, so the two waves of a workgroup each take a contiguous share of them; after that the waves part ways --
// nothing wave 0 has left to do depends on the rows, and the lists and column metadata the NEXT search walks are final
// once the list move is done (unless a column has to be removed):
//
//   wave 0: search + layout -> LDS |B1| its columns |B2| U row, list move, L column, walk of the next search |B3| record ...
//   wave 1:                  (waits) |B1| its columns |B2| all the rows                                        |B3| (waits)
//
// The phases themselves are the flattened passes of k_pivot_wave.hip (same code shape, slot indices offset by the
// wave's first line).  Singleton-column pivots and the general paths are not split: wave 0 runs the former alone, the
// latter are workgroup code already (k_pivot.hip).
//
// Barriers order LDS only (wg_barrier_lds): no wave loads from the arenas what the other wave stored in the same
// phase -- columns and rows are disjoint between the waves, the masks / counts they exchange are in LDS.  Wave 1 has its
// stores behind it at B2 and B3 (wave 0 then loads the column / row metadata it stored), wave 0 at B1 (free: its last
// stores were issued a whole search ago).
//
// Arena positions of re-appended lines come from an LDS atomic, so WHERE a re-appended line lands depends on which
// wave asks first; the totals (and with them every room check, every compaction, every result) do not.

__device__ __forceinline__ void wv2_small(const DevGP &D, Sm *sm, WvWalk &E, int pr, int pc, int nz_col, int nz_row)
{
    const int lane = lane_id(), w = wave_id();
    Scalars *S = D.s;
    Fast *fa = &sm->fa;
    const int cnz1 = nz_col - 1, rnz1 = nz_row - 1;
    const double pivot = fa->pV[0];
    DEV_CHECK(S, pivot != 0.0);
    const double droptol = D.droptol;
    unsigned long long *zw = w ? fa->zw2 : fa->zw;
    double *W = sm->swork + w * WV_WHALF;
    int nexp = 0;
    if (w != 0) {
        // columns of the pivot row -> slot (slot 0 = the pivot column): membership for the rows (this wave, after the
        // columns) and for the list move (wave 0, after B2) -- built here, off wave 0's path
        wv_hclear_t(fa->hsh);
        wave_mem_sync();
        if (lane <= rnz1) wv_hinsert_t(fa->hsh, fa->lJ[lane], lane < rnz1 ? lane + 1 : 0);
    }

    // ================= column file update (pivot.rs:566-691): this wave's columns =================
    {
        const int csplit = fa->csplit;
        const int cbase = w ? csplit : 0, ncol = w ? rnz1 - csplit : csplit;
        const int cs = cbase + lane; // lane = column: its index in the per-line arrays
        const bool mine = lane < ncol;
        int Lj = -1, Lcb = 0, Lcl = 0, Lcap = 0;
        if (mine) {
            Lj = fa->lJ[cs];
            Lcb = fa->lCb[cs];
            Lcl = fa->lCl[cs];
            Lcap = fa->lCap[cs];
        }
        int Tc;
        const int coff = wv_excl_scan(Lcl, &Tc);
        if (mine) {
            fa->sBO[cs] = make_int2(Lcb, coff);
            fa->sCnt[cs] = 0;
        }
        wave_mem_sync();
        WV_T(6);
        // per-lane constants of the paired pass: lane = (column cl_l of the pass, position p_l)
        const int Cper = 64 / cnz1;
        const int cl_l = lane / cnz1, p_l = lane - cl_l * cnz1;
        const bool pairlane = cl_l < Cper;
        const int segs = cl_l * cnz1;
        const unsigned long long segbelow = wv_bits_below(segs);
        const unsigned long long segmask = pairlane ? (wv_bits_below(cnz1) << segs) : 0ull;
        const double pv_l = fa->pV[1 + p_l];
        const int pi_l = fa->pI[1 + p_l];
        const int Gc = WV_WHALF / cnz1; // columns per group (cnz1 <= 63: at least two)
        int nk1 = 0, dst = Lcb, newcap = Lcap;
        double xrj = 0.0;
        int nd3 = 0;
        bool anyc = false;

        for (int c0 = 0; c0 < ncol; c0 += Gc) {
            const int c1 = min(c0 + Gc, ncol);
            const int f0 = __builtin_amdgcn_readlane(coff, c0);
            const int f1 = c1 < ncol ? __builtin_amdgcn_readlane(coff, c1) : Tc;
            const int Tg = f1 - f0;
            const bool ing = lane >= c0 && lane < c1;
            if (ing) {
                const int o = coff - f0;
                atomicOr(&zw[o >> 6], 1ull << (o & 63));
            }
            wave_mem_sync();
            // ---- pass A (see wv_small): entries whose row is in the pivot column leave (value -> W), the others are
            // compressed in place
            const int g0 = cbase + c0; // the group's first column
            int cbv = g0 - 1, carry = 0;
            const auto work_a = [&](const WvPass &P) {
                const WvSeg sg = P.sg;
                const bool valid = P.valid;
                const int2 bo = P.bo;
                const int idx = P.idx;
                const double val = P.val;
                const int p = valid ? wv_hfind_t(fa->hshr, idx) : -1;
                const bool hit = valid && p >= 0;
                const bool keep = valid && !hit;
                const bool ispr = keep && idx == pr;
                if (hit) W[(sg.c - g0) * cnz1 + p] = val;
                const unsigned long long kb = __ballot(keep);
                const int t = valid ? wv_rank(sg, kb, carry) : 0;
                carry = __builtin_amdgcn_readlane(t + (keep ? 1 : 0), 63);
                if (sg.tail) fa->sCnt[sg.c] = t + (keep ? 1 : 0);
                if (ispr) {
                    fa->sX[sg.c] = val;
                    fa->sW[sg.c] = t;
                } else if (keep) {
                    if (t == 0) {
                        fa->sK0i[sg.c] = idx;
                        fa->sK0v[sg.c] = val;
                    } else {
                        wv_st<int>(D.cidx, bo.x + t - 1, idx);
                        wv_st<double>(D.cval, bo.x + t - 1, val);
                    }
                    atomicMax(&fa->sMax[sg.c], (unsigned long long)__double_as_longlong(fabs(val)));
                }
            };
            const int npass = (Tg + 63) >> 6;
            WvPass PA = wv_fetch_z<true>(D, fa, zw, fa->sBO, D.cidx, 0, Tg, f0, cbv), PB = PA;
            for (int k = 0; k < npass; k += 2) {
                PB = wv_fetch_z<true>(D, fa, zw, fa->sBO, D.cidx, k + 1, Tg, f0, cbv);
                work_a(PA);
                PA = wv_fetch_z<true>(D, fa, zw, fa->sBO, D.cidx, k + 2, Tg, f0, cbv);
                work_a(PB);
            }
            WV_T(7);
            wave_mem_sync();
            // ---- per column: kept count, room (file_reappend, file.rs:56-85), the deferred first entry, multiplier
            bool reloc = false;
            if (ing) {
                const int cnt = fa->sCnt[cs], wq = fa->sW[cs];
                DEV_CHECK(S, cnt >= 1);
                nk1 = cnt - 1;
                const int need = nk1 + cnz1;
                reloc = need > Lcap;
                if (reloc) newcap = need + stretch_of(D.stretch, need) + D.pad;
                if (wq > 0) {
                    D.cidx[Lcb + wq - 1] = fa->sK0i[cs];
                    D.cval[Lcb + wq - 1] = fa->sK0v[cs];
                }
                xrj = fa->sX[cs];
            }
            const unsigned long long rlb = __ballot(reloc);
            if (rlb) { // (uniform)
                int tot;
                const int ex = wv_excl_scan(reloc ? newcap : 0, &tot);
                int base = 0;
                if (lane == 0) base = atomicAdd(&sm->cused, tot);
                base = __builtin_amdgcn_readfirstlane(base);
                if (reloc) dst = base + ex;
                nexp += __popcll(rlb);
                wave_mem_sync();
                unsigned long long rest = rlb;
                while (rest) {
                    const int b = __ffsll((long long)rest) - 1;
                    rest &= rest - 1;
                    const int src = __builtin_amdgcn_readlane(Lcb, b), nn = __builtin_amdgcn_readlane(nk1, b), dd = __builtin_amdgcn_readlane(dst, b);
                    for (int t = lane; t < nn; t += 64) {
                        D.cidx[dd + t] = D.cidx[src + t];
                        D.cval[dd + t] = D.cval[src + t];
                    }
                }
            }
            if (ing) {
                fa->sX[cs] = xrj / pivot;
                fa->sDst[cs] = dst + nk1;
            }
            wave_mem_sync();
            WV_T(8);
            // ---- pass B: (column, position) pairs: work -= a * col (pivot.rs:623-625), append what stays above
            // droptol in pivot-column order (:630-664)
            int wbase = 0;
            for (int cb0 = c0; cb0 < c1; cb0 += Cper, wbase += Cper * cnz1) {
                const bool act = pairlane && cb0 + cl_l < c1;
                const int c = cbase + cb0 + cl_l;
                double old = 0.0, a = 0.0;
                int dd = 0;
                if (act) {
                    old = W[wbase + lane];
                    W[wbase + lane] = 0.0;
                    a = fa->sX[c];
                    dd = fa->sDst[c];
                }
                const double x = mulsub(old, a, pv_l);
                const double ax = fabs(x);
                const bool kx = act && ax > droptol;
                const unsigned long long kxb = __ballot(kx);
                if (kx) {
                    const int rank = wave_prefix_count(kxb) - __popcll(kxb & segbelow);
                    wv_st<int>(D.cidx, dd + rank, pi_l);
                    wv_st<double>(D.cval, dd + rank, x);
                    atomicMax(&fa->sMax[c], (unsigned long long)__double_as_longlong(ax));
                }
                if (act && p_l == 0) {
                    const unsigned long long cm = (~kxb & segmask) >> segs; // cancelled positions (pivot.rs:656-660)
                    fa->sNew[c] = __popcll(kxb & segmask);
                    fa->sM[c] = cm;
                    if (cm) {
                        anyc = true;
                        nd3 += __popcll(cm >> 31);
                    }
                }
            }
            wave_mem_sync();
        }
        WV_T(9);
        // ---- per column: new metadata; for wave 0's finish: the new length (list key) and the pivot-row entry (U row)
        bool tiny = false;
        if (mine) {
            const int newlen = nk1 + fa->sNew[cs];
            const double cmx = __longlong_as_double((long long)fa->sMax[cs]);
            fa->sMax[cs] = 0ull;
            D.cbeg[Lj] = dst;
            D.clen[Lj] = newlen;
            D.ccap[Lj] = newcap;
            D.colmax[Lj] = cmx;
            tiny = cmx == 0.0 || cmx < D.abstol;
            fa->lCl[cs] = newlen;
            fa->lXr[cs] = xrj;
        }
        const unsigned long long tinyb = __ballot(tiny), anycb = __ballot(anyc);
        const int d3all = wave_sum_i(nd3);
        if (lane == 0) {
            if (tinyb) fa->tiny = 1;
            if (anycb) fa->anycancel = 1;
            if (d3all) atomicAdd((unsigned long long *)&sm->d3, (unsigned long long)d3all);
        }
    }
    WV_T(10);
    wg_barrier_lds(w != 0); // B2: masks, new lengths and the two flags are in LDS (wave 1's column metadata stores are behind it: wave 0's walk loads them)
    WV_T(17); // (prof build: wave 0's wait for wave 1)
    E.st = 0;
    if (w == 0) {
        int ltail = 0, lkey = -1;
        if (lane < rnz1) { // tails of the columns' new count lists (the keys are final)
            lkey = fa->lCl[lane];
            ltail = D.cblink.hd(lkey);
        }
        // ================= wave 0 finishes the pivot: nothing below depends on the rows =================
        // ---- U row (pivot.rs:666-672)
        const int j = lane <= rnz1 ? fa->lJ[lane] : -1;
        const double xr = lane < rnz1 ? fa->lXr[lane] : 0.0;
        const bool ku = lane < rnz1 && fabs(xr) > droptol;
        const unsigned long long kub = __ballot(ku);
        int uused = sm->uused;
        if (ku) {
            const int d = uused + wave_prefix_count(kub);
            D.uidx[d] = j;
            D.uval[d] = xr;
        }
        uused += __popcll(kub);
        // ---- column count lists (pivot.rs:682-683, :797)
        int fl = 0, bl = 0;
        if (lane <= rnz1) {
            fl = fa->lFl[lane];
            bl = fa->lBl[lane];
        }
        const int mn = wv_list_move(D, fa, j, lkey, lane < rnz1, lane == rnz1, fl, bl, rnz1, D.m + 2, ltail);
        // ---- L column (pivot.rs:778-790)
        double lx = 0.0;
        int li = -1;
        if (lane < cnz1) {
            li = fa->pI[lane + 1];
            lx = fa->pV[lane + 1] / pivot;
        }
        const bool kl = lane < cnz1 && fabs(lx) > droptol;
        const unsigned long long klb = __ballot(kl);
        int lused = sm->lused;
        if (kl) {
            const int d = lused + wave_prefix_count(klb);
            D.lidx[d] = li;
            D.lval[d] = lx;
        }
        lused += __popcll(klb);
        // ---- cleanup (pivot.rs:792-800)
        WAVE_LOCKSTEP(); // (every lane has read sm->lused / sm->uused before lane 0 replaces them)
        if (lane == 0) {
            const int rank = sm->rank;
            D.ubeg[rank + 1] = uused;
            D.lbeg[rank + 1] = lused;
            sm->uused = uused;
            sm->lused = lused;
            if (mn < sm->min_colnz) sm->min_colnz = mn;
            if (fa->tiny) sm->flag_small = 1;
            D.colmax[pc] = pivot;
            D.clen[pc] = 0;
            D.rlen[pr] = 0;
            sm->kinds[3]++;
            sm->nfast[0]++;
        }
        wave_mem_sync();
        WV_T(16);
        // ---- the list walk of the NEXT search (see WvWalk): lists and column metadata are final (unless a column has
        // to be removed, which changes the lists again); it runs while wave 1 updates the rows
        const int K = D.maxsearch;
        if (!fa->tiny && D.search_rows == 0 && !D.no_fast && K >= 1 && K <= KCMAX) ew_begin(D, E, sm->min_colnz);
    }
    // ================= row file update (pivot.rs:695-775): wave 1, all the rows =================
    // (MEASURED, C3 x 1536: starting the rows BEFORE B2 -- the overlap with the pivot row leaves every row whatever the
    // columns do -- with 60-70 % of the columns on wave 0 instead: 1.72 s where this order takes 1.67 s.  The rows then
    // need line tables of their own beside the columns', and those 1 KB more of LDS alone cost 3 %.)
    const int ps = lane, nrow = cnz1; // lane = row
    const bool mine = w != 0 && lane < nrow;
    int Li = -1, Lrb = 0, Lrl = 0, Lrc = 0;
    int rnk = 0, rdst = 0, rnewcap = 0;
    if (w != 0) {
        if (mine) {
            Li = fa->lI[ps];
            Lrb = fa->lRb[ps];
            Lrl = fa->lRl[ps];
            Lrc = fa->lRc[ps];
        }
        int Tr;
        const int roff = wv_excl_scan(Lrl, &Tr);
        if (mine) {
            fa->sBO[ps] = make_int2(Lrb, roff);
            fa->sCnt[ps] = 0;
            atomicOr(&zw[roff >> 6], 1ull << (roff & 63));
        }
        wave_mem_sync();
        WV_T(11);
        {
            int cbv = -1, carry = 0;
            const auto work_r = [&](const WvPass &P) {
                const WvSeg sg = P.sg;
                const bool valid = P.valid;
                const int j = P.idx;
                const bool keep = valid && wv_hfind_t(fa->hsh, j) < 0; // overlap with the pivot row leaves, pivot column included
                const unsigned long long kb = __ballot(keep);
                const int t = valid ? wv_rank(sg, kb, carry) : 0;
                carry = __builtin_amdgcn_readlane(t + (keep ? 1 : 0), 63);
                if (sg.tail) fa->sCnt[sg.c] = t + (keep ? 1 : 0);
                if (keep && t != P.e) wv_st<int>(D.ridx, P.bo.x + t, j);
            };
            const int npass = (Tr + 63) >> 6;
            WvPass PA = wv_fetch_z<false>(D, fa, zw, fa->sBO, D.ridx, 0, Tr, 0, cbv), PB = PA;
            for (int k = 0; k < npass; k += 2) {
                PB = wv_fetch_z<false>(D, fa, zw, fa->sBO, D.ridx, k + 1, Tr, 0, cbv);
                work_r(PA);
                PA = wv_fetch_z<false>(D, fa, zw, fa->sBO, D.ridx, k + 2, Tr, 0, cbv);
                work_r(PB);
            }
        }
        wave_mem_sync();
        WV_T(12);
        rdst = Lrb;
        rnewcap = Lrc;
        {
            bool reloc = false;
            if (mine) {
                rnk = fa->sCnt[ps];
                DEV_CHECK(S, rnk < Lrl); // the pivot-column entry at least has left
                const int need = rnk + rnz1;
                reloc = need > Lrc;
                if (reloc) rnewcap = need + stretch_of(D.stretch, need) + D.pad;
            }
            const unsigned long long rlb = __ballot(reloc);
            if (rlb) {
                int tot;
                const int ex = wv_excl_scan(reloc ? rnewcap : 0, &tot);
                int base = 0;
                if (lane == 0) base = atomicAdd(&sm->rused, tot);
                base = __builtin_amdgcn_readfirstlane(base);
                if (reloc) rdst = base + ex;
                nexp += __popcll(rlb);
                unsigned long long rest = rlb;
                while (rest) {
                    const int b = __ffsll((long long)rest) - 1;
                    rest &= rest - 1;
                    const int src = __builtin_amdgcn_readlane(Lrb, b), nn = __builtin_amdgcn_readlane(rnk, b), dd = __builtin_amdgcn_readlane(rdst, b);
                    for (int t = lane; t < nn; t += 64) D.ridx[dd + t] = D.ridx[src + t];
                }
            }
            if (mine) fa->sDst[ps] = rdst + rnk;
        }
        wave_mem_sync();
        WV_T(13);
    }
    if (w != 0) {
        // ---- append the pattern of the pivot row, minus the cancelled positions (pivot.rs:752-758): (row, position) pairs
        int rnew = rnk + rnz1;
        {
            const int anycancel = fa->anycancel;
            const int Rper = 64 / rnz1;
            const int pl_l = lane / rnz1, q_l = lane - pl_l * rnz1;
            const bool rpair = pl_l < Rper;
            const int rsegs = pl_l * rnz1;
            const unsigned long long rsegbelow = wv_bits_below(rsegs);
            const unsigned long long rsegmask = rpair ? (wv_bits_below(rnz1) << rsegs) : 0ull;
            const int tj_l = fa->tJ[1 + q_l];
            const unsigned long long cm_l = anycancel ? fa->sM[q_l] : 0ull;
            for (int p0 = 0; p0 < nrow; p0 += Rper) {
                const bool act = rpair && p0 + pl_l < nrow;
                const int p = p0 + pl_l;
                const bool ok = act && ((cm_l >> p) & 1ull) == 0ull;
                const unsigned long long okb = __ballot(ok);
                if (ok) {
                    const int rank = wave_prefix_count(okb) - __popcll(okb & rsegbelow);
                    wv_st<int>(D.ridx, fa->sDst[p] + rank, tj_l);
                }
                if (anycancel && act && q_l == 0) fa->sNew[p] = __popcll(okb & rsegmask);
            }
            if (anycancel) {
                wave_mem_sync();
                if (mine) rnew = rnk + fa->sNew[ps];
            }
        }
        if (mine) {
            D.rbeg[Li] = rdst;
            D.rlen[Li] = rnew;
            D.rcap[Li] = rnewcap;
        }
    }
    if (nexp && lane == 0) atomicAdd((unsigned long long *)&sm->nexpand, (unsigned long long)nexp);
    WV_T(14);
    if (w == 0) {
        while (E.st == 1 || E.st == 2) ew_step(D, sm, E, D.maxsearch);
        WV_T(2);
    }
    wg_barrier_lds(w != 0); // B3: (wave 1's metadata stores are behind it: the next search, on wave 0, loads them)
    WV_T(15); // (wave 0's wait for wave 1)
}

// ------------------------------------------------------------------------------------------------
// the pivot loop of one matrix on two waves: factorize_bump (factorize_bump.rs:12-49) + pivot() (pivot.rs:48-112)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pivot_loop_wave2(DevLU *Ds, int stop_at, Sm *sm)
{
    const DevGP D(&Ds[blockIdx.x]);
    Scalars *S = D.s;
    const int lane = lane_id(), w = wave_id(), tid = threadIdx.x;
    const int m = D.m;

    if (S->status != ST_RUNNING) return; // finished or failed in an earlier launch (batch relaunch)
    Fast *fa = &sm->fa;
    if (tid == 0) {
        sm->rank = S->rank;
        sm->rankdef = S->rankdef;
        sm->min_colnz = S->min_colnz;
        sm->min_rownz = S->min_rownz;
        sm->cused = S->cused;
        sm->rused = S->rused;
        sm->lused = S->lused;
        sm->uused = S->uused;
        sm->pr = S->pivot_row;
        sm->pc = S->pivot_col;
        sm->exit_code = 0;
        sm->head_exit = 0;
        sm->need = 0;
        sm->nsearch = 0;
        sm->flops = 0;
        sm->nexpand = 0;
        sm->d3 = 0;
        sm->stop_at = stop_at;
        sm->flag_small = 0;
        fa->kind = 0;
        fa->nxValid = 0;
        fa->anycancel = 0;
        fa->tiny = 0;
#ifdef BLU_PROFILE
        for (int k = 0; k < 48; k++) sm->prof[k] = 0;
        g_pstamp[0] = (long long)__builtin_amdgcn_s_memtime();
#endif
        for (int k = 0; k < 6; k++) sm->kinds[k] = 0;
        sm->nfast[0] = sm->nfast[1] = sm->nfast[2] = sm->nfast[3] = 0;
        g_pivot_err = 0;
        g_pivot_err_line = 0;
    }
    for (int k = tid; k < WV_WCAP; k += 128) sm->swork[k] = 0.0;
    if (tid < 2) sm->wmax[tid] = 0ull;
    if (w == 0) {
        fa->zw[lane] = 0ull; // WV_ZW == 64
        fa->sMax[lane] = 0ull;
    } else {
        fa->zw2[lane] = 0ull;
    }
    __syncthreads();

    WvLines L;
    WvWalk E;
    E.st = 0;
    int rank = sm->rank, rankdef = sm->rankdef;
    bool pending = sm->pc >= 0; // a pivot left pending by a NEED_* exit of the previous launch
    for (;;) {
        // ---- wave 0: loop head (done / stop / error?) and the search; the outcome is in LDS for both waves
        if (w == 0) {
            int head_exit = 0;
            if (g_pivot_err) head_exit = ST_ERROR;
            else if (rank + rankdef >= m) head_exit = ST_DONE;
            else if (stop_at >= 0 && !pending && rank + rankdef >= stop_at) head_exit = ST_STOPPED;
            WAVE_LOCKSTEP();
            if (lane == 0) {
                sm->head_exit = head_exit;
                if (head_exit) sm->exit_code = head_exit;
            }
            if (!head_exit) {
                WV_T(0);
                bool handled = false;
                WvPick P;
                if (!pending) {
                    if (D.search_rows == 0 && !D.no_fast) handled = wv_search(D, sm, L, P, E);
                    if (!handled) {
                        if (D.search_rows == 0) markowitz_wave(D, sm);
                        else if (lane == 0) markowitz_serial(D, sm);
                        wave_mem_sync();
                    }
                }
                if (!handled) {
                    if (lane == 0) setup_pivot_general(D, sm);
                    wave_mem_sync();
                }
            }
        }
        pending = false;
        wg_barrier_lds(w == 0); // B1 (wave 0's stores since the last pivot -- a singleton column's row edits -- are behind it)
        if (sm->head_exit) break;
        const int pr = sm->pr, pc = sm->pc, exit_code = sm->exit_code, nz_col = sm->nzc, nz_row = sm->nzr, kind = fa->kind;
        if (pc < 0) { // no pivot found: the reference asserts (factorize_bump.rs:22)
            if (tid == 0) {
                DEV_CHECK(S, false);
                sm->exit_code = ST_ERROR;
            }
            break;
        }
        if (pr < 0) { // eliminate empty column without choosing a pivot (factorize_bump.rs:24-33)
            wg_barrier_lds(false); // (both waves have read the outcome before thread 0 changes it)
            if (tid == 0) {
                list_remove1(D.cflink, D.cblink, pc);
                sm->pc = -1;
                sm->rankdef = rankdef + 1;
                sm->kinds[5]++;
            }
            rankdef++;
            if (w == 0) wave_mem_sync();
            continue;
        }
        // ---- pivot(): the room check of pivot.rs:70-81 was made by the search; dispatch (:84-94)
        if (exit_code) break;
        bool ok = true;
        if (kind == 1) {
            wv2_small(D, sm, E, pr, pc, nz_col, nz_row);
        } else {
            if (kind == 2) {
                if (w == 0) wv_scol(D, sm, L, pr, pc, nz_row);
            } else if (nz_row == 1) ok = pivot_singleton_row(D, sm);
            else if (nz_col == 1) ok = pivot_singleton_col(D, sm);
            else if (nz_col == 2) ok = pivot_doubleton_col(D, sm);
            else ok = pivot_general(D, sm, nz_col - 1 <= 64);
            if (kind == 0) WV_T(23);
            wg_barrier_lds(false); // (both waves have read the outcome before thread 0 changes it)
        }
        if (!ok) break; // exit_code set, pivot stays pending
        // ---- remove columns whose maximum dropped below abstol (pivot.rs:98-106), record the pivot
        if (tid == 0) {
            if (sm->flag_small && nz_row > 1) {
                for (int pos = D.ubeg[rank]; pos < D.ubeg[rank + 1]; pos++) {
                    const int j = D.uidx[pos];
                    if (D.colmax[j] == 0.0 || D.colmax[j] < D.abstol) remove_col_serial(D, sm, j);
                }
            }
            sm->flops += (long long)(nz_col - 1) * (long long)(nz_row - 1);
            D.pinv[pr] = rank;
            D.qinv[pc] = rank;
            D.prow[rank] = pr;
            D.pcol[rank] = pc;
            sm->pc = -1;
            sm->pr = -1;
            sm->rank = rank + 1;
        }
        rank++;
        if (w == 0) {
            wave_mem_sync();
            WV_T(22);
        }
    }
    __syncthreads();
    if (tid == 0) {
        S->rank = sm->rank;
        S->rankdef = sm->rankdef;
        S->min_colnz = sm->min_colnz;
        S->min_rownz = sm->min_rownz;
        S->cused = sm->cused;
        S->rused = sm->rused;
        S->lused = sm->lused;
        S->uused = sm->uused;
        S->pivot_row = sm->pr;
        S->pivot_col = sm->pc;
        S->need = sm->need;
        S->nsearch_pivot += sm->nsearch;
        S->factor_flops += sm->flops;
        S->nexpand += sm->nexpand;
        S->d3_hits += sm->d3;
        for (int k = 0; k < 6; k++) S->npivot_kind[k] += sm->kinds[k];
        for (int k = 0; k < 4; k++) S->nfast[k] += sm->nfast[k];
#ifdef BLU_PROFILE
        for (int k = 0; k < 48; k++) S->prof[k] += sm->prof[k];
#endif
        if (sm->exit_code == ST_ERROR && g_pivot_err_line) set_error(S, ST_ERROR, g_pivot_err_line);
        if (S->status == ST_RUNNING) S->status = sm->exit_code;
    }
}

// register budget: four waves per SIMD
__global__ void __launch_bounds__(128) BLU_WAVES_PER_EU(4, 4) k_pivot_loop_wave2(DevLU *Ds, int stop_at)
{
    __shared__ Sm smem;
    pivot_loop_wave2(Ds, stop_at, &smem);
}
// The same loop with the registers of THREE waves per SIMD (168 instead of 128 VGPRs: nothing spilled): for a batch of at most
// six workgroups per CU -- 1536 bases, what HBM holds of the 100k size -- the fourth wave would stay empty anyway.
// Pivot kernel 1.510 -> 1.486 s at C3 x 1536.
__global__ void __launch_bounds__(128) BLU_WAVES_PER_EU(3, 3) k_pivot_loop_wave2_r3(DevLU *Ds, int stop_at)
{
    __shared__ Sm smem;
    pivot_loop_wave2(Ds, stop_at, &smem);
}
