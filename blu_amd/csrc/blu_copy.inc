// blu_copy.inc -- blu_hip_copy_batch / blu_hip_clone (included by blu_hip.hip): the complete logical state of one
// handle copied into n others of the same size, in one launch of k_copy_fanout (k_copy.hip) whatever n is.
//
// What is state and what is not:
//   * device: the stage-ordered factors (pinv, qinv, prow, pcol, lbeg, ubeg, L, U up to lused / uused), the canonical
//     factors (rowperm, colperm, the column pointers, m + l_nz / m + u_nz entries), the Scalars, and -- when the update
//     workspace belongs to this factorization -- the maps, pivots, the two files of U up to wused and
//     max(ucused, end of a pending spike), the eta file with a pending row eta, the pivot sequence and the UpdState.
//     The active submatrix (line records, arenas) is dead after a factorization; the packed copies of B, gwork and the
//     scratch arrays carry nothing between calls, nor do iw1 / iw2 / work1 of the update workspace (k_update scatters
//     the row eta into work1 itself).
//   * host: parameters, nupdate, nfactorize, update_cost_denom, the downloaded Scalars and UpdState (the permutation
//     totals live there while the update workspace is not valid), the flop counters and branch of solve_sparse,
//     skip_stats, the timing keys, and the parameter fields of the descriptor as the source's kernels last saw them.
//   * caches keyed by nfactorize: the update workspace is copied with its key; the row-wise L and the sorted U rows are
//     invalidated in the destination (k_build_lt / k_solve_dense rebuild the same bits on demand) -- a destination that
//     held another matrix with the same count must not keep them.
//   * the destination's own: debug knobs, environment-read settings, the workspace pools, the sparse workspace with
//     its marker, the solve buffers, the inputs of its last factorize.  A held solve_sparse_multi result is dropped.
// Capacities: a destination's L, U, arenas and update arenas are reused when they hold at least the source's capacity
// and allocated anew with the source's capacity otherwise; the capacity the destination then works with IS the
// source's (the surplus of a larger allocation lies idle), so the copy asks for storage exactly when the source would
// and L_MEM / U_MEM / W_MEM agree.  A second copy into the same destination allocates nothing.
// Descriptors hold the destination's own pointers: built here on the host per destination, staged with the tables and
// delivered by the kernel to each dD / dO.  One upload, one launch, one synchronize.

namespace {
struct CopySegHost {
    const void *src;
    size_t bytes;
    long long stride;
    std::vector<void *> dst; // one per live destination
};
} // namespace

// free + allocate a pair (or a single array when b is null) of `cap` entries; false: both null
template <class A, class B> static bool copy_regrow(blu_hip *d, A **a, B **b, size_t cap)
{
    dfree(*a);
    if (b) dfree(*b);
    if (!dalloc(d, a, cap)) return false;
    if (b && !dalloc(d, b, cap)) {
        dfree(*a);
        return false;
    }
    return true;
}

// storage of destination d for the state of src; BLU_OK or BLU_ERROR_OUT_OF_MEMORY (d then holds no factorization)
static int copy_prepare(blu_hip *src, blu_hip *d, bool with_upd)
{
    const DevLU &S = src->D;
    DevLU &T = d->D;
    bool ok = true;
    if (T.lcap < S.lcap && !copy_regrow(d, &T.lidx, &T.lval, (size_t)S.lcap)) ok = false, T.lcap = 0;
    else T.lcap = S.lcap;
    if (T.ucap < S.ucap && !copy_regrow(d, &T.uidx, &T.uval, (size_t)S.ucap)) ok = false, T.ucap = 0;
    else T.ucap = S.ucap;
    if (d->out_in_arena) { // the canonical factors d holds go with its arena: placed again below
        d->O.l_rowidx = d->O.u_rowidx = nullptr;
        d->O.l_value = d->O.u_value = nullptr;
        d->out_lcap = d->out_ucap = 0;
        d->out_in_arena = false;
    }
    if (T.carena_cap < S.carena_cap && !copy_regrow(d, &T.cidx, &T.cval, (size_t)S.carena_cap)) ok = false, T.carena_cap = 0;
    else T.carena_cap = S.carena_cap;
    if (T.rarena_cap < S.rarena_cap && !copy_regrow(d, &T.ridx, (int **)nullptr, (size_t)S.rarena_cap)) ok = false, T.rarena_cap = 0;
    else T.rarena_cap = S.rarena_cap;
    // the canonical factors: placed as factorize places them (ensure_out), on d's own arena
    if (ok && !ensure_out(d, (int64_t)src->hs.lused + src->m, (int64_t)src->hs.uused + src->m, false)) ok = false;
    if (ok && with_upd) {
        const UpdWs &SU = src->uw;
        UpdWs &TU = d->uw;
        // (blu_hip_update right after the copy runs on the destination's sparse workspace: it has to exist)
        ok = ensure_sparse_ws(d) == BLU_OK && ensure_upd_fixed(d) == BLU_OK;
        if (ok) {
            if (TU.wcapacity < SU.wcapacity && !copy_regrow(d, &TU.widx, &TU.wval, (size_t)SU.wcapacity)) ok = false, TU.wcapacity = 0;
            else TU.wcapacity = SU.wcapacity;
            if (TU.uccapacity < SU.uccapacity && !copy_regrow(d, &TU.ucidx, &TU.ucval, (size_t)SU.uccapacity)) ok = false, TU.uccapacity = 0;
            else TU.uccapacity = SU.uccapacity;
            if (TU.rcapacity < SU.rcapacity && !copy_regrow(d, &TU.ridx, &TU.rval, (size_t)SU.rcapacity)) ok = false, TU.rcapacity = 0;
            else TU.rcapacity = SU.rcapacity;
        }
    }
    // the parameters as the source's kernels last saw them (fill_desc of its last upload): droptol, stretch and pad are
    // read from the descriptor by the solves and by k_upd_init
    T.m = (int)d->m; // (a handle that never factorized has not filled its descriptor yet)
    T.nzbias = S.nzbias;
    T.maxsearch = S.maxsearch;
    T.pad = S.pad;
    T.search_rows = S.search_rows;
    T.skip_stats = S.skip_stats;
    T.droptol = S.droptol;
    T.abstol = S.abstol;
    T.reltol = S.reltol;
    T.stretch = S.stretch;
    return ok ? BLU_OK : BLU_ERROR_OUT_OF_MEMORY;
}

// d holds no factorization (a member whose storage could not be had)
static void copy_invalidate(blu_hip *d)
{
    d->nupdate = -1;
    d->upd_for_nfact = d->lt_for_nfact = d->rows_for_nfact = -1;
}

// the host mirrors
static void copy_host_state(const blu_hip *src, blu_hip *d, bool with_upd)
{
    d->droptol = src->droptol;
    d->abstol = src->abstol;
    d->reltol = src->reltol;
    d->stretch = src->stretch;
    d->compress_thres = src->compress_thres;
    d->sparse_thres = src->sparse_thres;
    d->realloc_factor = src->realloc_factor;
    d->nzbias = src->nzbias;
    d->maxsearch = src->maxsearch;
    d->pad = src->pad;
    d->search_rows = src->search_rows;
    d->skip_stats = src->skip_stats;
    d->nupdate = src->nupdate;
    d->nfactorize = src->nfactorize;
    d->update_cost_denom = src->update_cost_denom;
    d->hs = src->hs;
    d->ust = src->ust;
    d->sp_l_flops = src->sp_l_flops;
    d->sp_u_flops = src->sp_u_flops;
    d->sp_branch = src->sp_branch;
    d->t_total = src->t_total;
    d->t_pivot = src->t_pivot;
    for (int q = 0; q < 6; q++) d->t_phase[q] = src->t_phase[q];
    d->relaunches = src->relaunches;
    d->last_pivot_kernel = src->last_pivot_kernel;
    d->last_pivot_regs = src->last_pivot_regs;
    d->last_addr_wide = src->last_addr_wide;
    d->narrow_launches = src->narrow_launches;
    // caches keyed by nfactorize: the update workspace came with its key, the row-wise copies are rebuilt on demand
    d->upd_for_nfact = with_upd ? d->nfactorize : -1;
    d->lt_for_nfact = d->rows_for_nfact = -1;
    d->sm_have = false;
    d->sm_ilhs.clear();
    d->sm_xlhs.clear();
}

extern "C" int blu_hip_copy_batch(blu_hip *src, blu_hip **dst, int n, int *status)
{
    if (!src || !dst || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    for (int k = 0; k < n; k++)
        if (!dst[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    {
        std::vector<blu_hip *> all(dst, dst + n);
        all.push_back(src); // (the source among the destinations counts as a handle twice)
        if (has_duplicate(std::move(all))) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT);
    }
    for (int k = 0; k < n; k++)
        if (dst[k]->device != src->device || dst[k]->m != src->m) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT);
    if (hipSetDevice(src->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);

    int64_t counts[6] = {0, 0, 0, 0, 0, 0};
    const int64_t allocs0 = t_dalloc_calls;
    const size_t M = (size_t)src->m;
    const bool valid = src->nupdate >= 0 && src->m > 0;                       // there is device state to copy
    const bool with_upd = valid && src->upd_for_nfact == src->nfactorize;      // ... the update workspace included
    std::vector<int> result(n, BLU_OK);
    std::vector<blu_hip *> live; // the destinations the kernel writes to
    for (int k = 0; k < n; k++) {
        blu_hip *d = dst[k];
        d->err.clear();
        if (!valid) continue;
        result[k] = copy_prepare(src, d, with_upd);
        if (result[k] == BLU_OK) live.push_back(d);
        else copy_invalidate(d);
    }
    bool ok = true;
    if (!live.empty()) {
        const size_t nl = live.size();
        std::vector<CopySegHost> segs;
        auto add = [&](const void *s, size_t bytes, long long stride, auto &&at) {
            if (!bytes) return;
            CopySegHost g;
            g.src = s;
            g.bytes = bytes;
            g.stride = stride;
            g.dst.resize(nl);
            for (size_t k = 0; k < nl; k++) g.dst[k] = (void *)at(live[k]);
            segs.push_back(std::move(g));
        };
        const DevLU &S = src->D;
        const Scalars &hs = src->hs;
        const size_t lused = (size_t)hs.lused, uused = (size_t)hs.uused;
        add(S.pinv, M * 4, 0, [](blu_hip *d) { return d->D.pinv; });
        add(S.qinv, M * 4, 0, [](blu_hip *d) { return d->D.qinv; });
        add(S.prow, M * 4, 0, [](blu_hip *d) { return d->D.prow; });
        add(S.pcol, M * 4, 0, [](blu_hip *d) { return d->D.pcol; });
        add(S.lbeg, (M + 1) * 4, 0, [](blu_hip *d) { return d->D.lbeg; });
        add(S.ubeg, (M + 1) * 4, 0, [](blu_hip *d) { return d->D.ubeg; });
        add(S.lidx, lused * 4, 0, [](blu_hip *d) { return d->D.lidx; });
        add(S.lval, lused * 8, 0, [](blu_hip *d) { return d->D.lval; });
        add(S.uidx, uused * 4, 0, [](blu_hip *d) { return d->D.uidx; });
        add(S.uval, uused * 8, 0, [](blu_hip *d) { return d->D.uval; });
        add(S.s, sizeof(Scalars), 0, [](blu_hip *d) { return d->D.s; });
        const FinishOut &SO = src->O;
        const size_t ln = (size_t)hs.l_nz + M, un = (size_t)hs.u_nz + M;
        add(SO.rowperm, M * 8, 0, [](blu_hip *d) { return d->O.rowperm; });
        add(SO.colperm, M * 8, 0, [](blu_hip *d) { return d->O.colperm; });
        add(SO.l_colptr, (M + 1) * 8, 0, [](blu_hip *d) { return d->O.l_colptr; });
        add(SO.u_colptr, (M + 1) * 8, 0, [](blu_hip *d) { return d->O.u_colptr; });
        add(SO.l_rowidx, ln * 8, 0, [](blu_hip *d) { return d->O.l_rowidx; });
        add(SO.l_value, ln * 8, 0, [](blu_hip *d) { return d->O.l_value; });
        add(SO.u_rowidx, un * 8, 0, [](blu_hip *d) { return d->O.u_rowidx; });
        add(SO.u_value, un * 8, 0, [](blu_hip *d) { return d->O.u_value; });
        if (with_upd) {
            const UpdWs &U = src->uw;
            const UpdState &us = src->ust;
            // the pending spike lies behind ucused; the committed etas end at rbeg[nforrest] = r_nz and a pending row eta
            // (at most m entries) lies behind them: its exact end is on the device only, so up to m entries more
            const size_t wused = (size_t)us.wused;
            size_t ucext = (size_t)us.ucused;
            if (us.ftran_for >= 0) ucext = std::max(ucext, (size_t)us.spike_beg + (size_t)us.spike_len);
            ucext = std::min(ucext, (size_t)U.uccapacity);
            size_t rext = (size_t)us.r_nz + (us.btran_for >= 0 ? M : 0);
            rext = std::min(rext, (size_t)U.rcapacity);
            const size_t nf = (size_t)us.nforrest, plen = std::min((size_t)us.pivotlen, 2 * M + 2);
            add(U.st, sizeof(UpdState), 0, [](blu_hip *d) { return d->uw.st; });
            add(U.pmap, M * 4, 0, [](blu_hip *d) { return d->uw.pmap; });
            add(U.qmap, M * 4, 0, [](blu_hip *d) { return d->uw.qmap; });
            add(U.col_pivot, M * 8, 0, [](blu_hip *d) { return d->uw.col_pivot; });
            add(U.row_pivot, M * 8, 0, [](blu_hip *d) { return d->uw.row_pivot; });
            add(U.wbeg, M * 4, 0, [](blu_hip *d) { return d->uw.wbeg; });
            add(U.wlen, M * 4, 0, [](blu_hip *d) { return d->uw.wlen; });
            add(U.wcap, M * 4, 0, [](blu_hip *d) { return d->uw.wcap; });
            add(U.widx, wused * 4, 0, [](blu_hip *d) { return d->uw.widx; });
            add(U.wval, wused * 8, 0, [](blu_hip *d) { return d->uw.wval; });
            add(U.ucbeg, M * 4, 0, [](blu_hip *d) { return d->uw.ucbeg; });
            add(U.uclen, M * 4, 0, [](blu_hip *d) { return d->uw.uclen; });
            add(U.ucidx, ucext * 4, 0, [](blu_hip *d) { return d->uw.ucidx; });
            add(U.ucval, ucext * 8, 0, [](blu_hip *d) { return d->uw.ucval; });
            add(U.rbeg, std::min(nf + 2, M + 2) * 4, 0, [](blu_hip *d) { return d->uw.rbeg; });
            add(U.eta_row, std::min(nf + 1, M + 1) * 4, 0, [](blu_hip *d) { return d->uw.eta_row; });
            add(U.ridx, rext * 4, 0, [](blu_hip *d) { return d->uw.ridx; });
            add(U.rval, rext * 8, 0, [](blu_hip *d) { return d->uw.rval; });
            add(U.pvrow, plen * 4, 0, [](blu_hip *d) { return d->uw.pvrow; });
            add(U.pvcol, plen * 4, 0, [](blu_hip *d) { return d->uw.pvcol; });
        }
        // the staging block: [segment table | destination pointers | DevLU per destination | FinishOut per destination]
        const size_t nseg = segs.size() + 2;
        Stage blk;
        const auto aS = blk.add<CopySeg>(nseg);
        const auto aP = blk.add<char *>(nseg * nl);
        const auto aD = blk.add<DevLU>(nl);
        const auto aO = blk.add<FinishOut>(nl);
        const size_t total = align_up(blk.bytes);
        if (total > src->cp_stage_cap) {
            dfree(src->cp_stage);
            src->cp_stage_cap = 0;
            if (dalloc(src, &src->cp_stage, total)) src->cp_stage_cap = total;
            else ok = false;
        }
        if (ok) {
            blk.dev = src->cp_stage; // (kept by the source for its next call)
            blk.host_front(total);
            for (size_t k = 0; k < nl; k++) {
                blk.h(aD)[k] = live[k]->D;
                blk.h(aO)[k] = live[k]->O;
            }
            add(blk.d(aD), sizeof(DevLU), (long long)sizeof(DevLU), [](blu_hip *d) { return d->dD; });
            add(blk.d(aO), sizeof(FinishOut), (long long)sizeof(FinishOut), [](blu_hip *d) { return d->dO; });
            CopySeg *sS = blk.h(aS);
            char **sP = blk.h(aP);
            long long ntiles = 0;
            for (size_t s = 0; s < segs.size(); s++) {
                const CopySegHost &g = segs[s];
                uintptr_t align = (uintptr_t)g.src | (uintptr_t)g.stride;
                for (size_t k = 0; k < nl; k++) {
                    sP[s * nl + k] = (char *)g.dst[k];
                    align |= (uintptr_t)g.dst[k];
                }
                sS[s].src = (const char *)g.src;
                sS[s].tile0 = ntiles;
                sS[s].words = (long long)(g.bytes / 4);
                sS[s].stride = g.stride;
                sS[s].vec = (align & 15) == 0;
                sS[s].pad0 = 0;
                ntiles += (sS[s].words + 3) / 4;
                counts[4] += (int64_t)g.bytes;
            }
            counts[5] = counts[4] * (int64_t)nl;
            // destinations per group: as few groups as still give every CU a few workgroups
            const long long per_block = (long long)COPY_THREADS * COPY_TILES;
            const long long tblocks = (ntiles + per_block - 1) / per_block;
            long long group = (long long)nl * tblocks / (4LL * std::max(src->num_cus, 1));
            group = std::max(1LL, std::min(group, 64LL));
            const long long groups = ((long long)nl + group - 1) / group;
            ok = tblocks * groups <= 0x7fffffffLL &&
                 hip_ok(src, hipMemcpyAsync(blk.dev, blk.host.data(), total, hipMemcpyHostToDevice, src->stream), "h2d copy tables");
            counts[2]++;
            if (ok) {
                hipLaunchKernelGGL(k_copy_fanout, dim3((unsigned)(tblocks * groups)), dim3(COPY_THREADS), 0, src->stream, blk.d(aS), (int)segs.size(),
                                   blk.d(aP), (int)nl, (int)group, (int)tblocks, ntiles);
                counts[0]++;
            }
            // (also after a failed upload: the host block must outlive the asynchronous copy)
            ok = hip_ok(src, hipStreamSynchronize(src->stream), "k_copy_fanout") && ok;
            counts[1]++;
        }
        if (!ok) {
            const int code = oom_or_device(src);
            for (int k = 0; k < n; k++)
                if (result[k] == BLU_OK) {
                    result[k] = code;
                    if (dst[k] != src) dst[k]->err = src->err;
                    copy_invalidate(dst[k]);
                }
        }
    }
    for (int k = 0; k < n; k++)
        if (result[k] == BLU_OK) copy_host_state(src, dst[k], with_upd);
    counts[3] = t_dalloc_calls - allocs0;
    memcpy(src->cp_counts, counts, sizeof counts);
    return batch_return(result, status);
}

extern "C" blu_hip *blu_hip_clone(blu_hip *src)
{
    if (!src) return nullptr;
    blu_hip *d = blu_hip_new(src->m, src->b_nz_hint, src->device);
    if (!d) return nullptr;
    if (blu_hip_copy_batch(src, &d, 1, nullptr) < 0) {
        blu_hip_free(d);
        return nullptr;
    }
    return d;
}

// the last blu_hip_copy_batch with this source: launches, synchronizes, host-to-device copies, device allocations made,
// bytes of state per destination (what the kernel reads from the source, a destination's descriptors counted once),
// bytes written to all destinations
extern "C" int blu_hip_dbg_copy_counts(const blu_hip *src, int64_t out[6])
{
    if (!src || !out) return BLU_ERROR_ARGUMENT_MISSING;
    memcpy(out, src->cp_counts, sizeof src->cp_counts);
    return BLU_OK;
}
