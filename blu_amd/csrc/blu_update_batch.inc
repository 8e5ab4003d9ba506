// blu_update_batch.inc -- blu_hip_solve_for_update_batch and blu_hip_update_batch (included by blu_hip.hip): what
// blu_hip_solve_for_update / blu_hip_update (blu_update.inc) do, for many handles in one call.  Each member runs on one
// wave, the members in one launch:
//   k_build_lt_batch    row-wise L of the members that do not have it yet       } first call after a factorization
//   k_upd_init_batch    the mutable copies of U, the maps and the pivot sequence }
//   k_solve_upd_batch   solve_for_update (the body of k_solve_upd, mode 1)
//   k_update_batch      update (the body of k_update)
//   k_gather_lhs_batch  the compressed solutions into one buffer
// A round is one upload (descriptors, what the call hands each member, the packed right-hand sides), one launch, one
// synchronize and one download (every member's UpdState and counters): none of them per member.  Storage requests
// (UPD_NEED_R / _UC / _W) are answered by grow_upd and those members alone are launched again, as blu_update.inc does
// for one handle.
// The pieces blu_hip_solve_sparse_batch (blu_solve_sparse_batch.inc) uses as well are here: run_upd_round,
// build_lt_batch, take_upd_result, take_solve_counters and gather_solutions.  The refusals, the return value and the
// staging block (Stage, stage_alloc / stage_run) are those of blu_batch.inc.

// what a round needs of the host, for the members listed in `list` (indices into hs) ...
struct UpdRound {
    std::vector<int> list;
    std::vector<UpdMember> mem; // mem[s] of list[s]; irhs / xrhs are filled in by the round
    std::vector<UpdResult> res; // OUT
};
// ... and the packed right-hand sides of the whole call: member k's begin at off[k] (indexed by member, not by list)
struct UpdRhs {
    std::vector<int> ir;
    std::vector<double> xr;
    std::vector<size_t> off;
};

template <class Launch>
static int run_upd_round(blu_hip *h0, blu_hip **hs, UpdRound &R, const UpdRhs &rhs, const char *what, Launch launch)
{
    const size_t c = R.list.size();
    Stage S;
    const auto aD = S.add<DevLU>(c);
    const auto aO = S.add<FinishOut>(c);
    const auto aW = S.add<SparseWs>(c);
    const auto aU = S.add<UpdWs>(c);
    const auto aM = S.add<UpdMember>(c);
    const auto aX = S.add<double>(rhs.xr.size());
    const auto aI = S.add<int>(rhs.ir.size());
    const auto aR = S.add<UpdResult>(c); // (written by the kernels: not uploaded)
    if (const int st = stage_alloc(h0, S); st != BLU_OK) return st;
    S.host_front(aR.off);
    for (size_t s = 0; s < c; s++) {
        const int k = R.list[s];
        blu_hip *h = hs[k];
        S.h(aD)[s] = h->D;
        S.h(aO)[s] = h->O;
        S.h(aW)[s] = h->sw;
        S.h(aU)[s] = h->uw;
        UpdMember &M = S.h(aM)[s];
        M = R.mem[s];
        M.irhs = rhs.ir.empty() ? nullptr : S.d(aI) + rhs.off[(size_t)k];
        M.xrhs = rhs.xr.empty() ? nullptr : S.d(aX) + rhs.off[(size_t)k];
    }
    if (!rhs.xr.empty()) memcpy(S.h(aX), rhs.xr.data(), rhs.xr.size() * sizeof(double));
    if (!rhs.ir.empty()) memcpy(S.h(aI), rhs.ir.data(), rhs.ir.size() * sizeof(int));
    R.res.assign(c, UpdResult());
    return stage_run(
        h0, S, "h2d update descriptors", what,
        [&](hipStream_t stream) { launch((int)c, stream, S.d(aD), S.d(aO), S.d(aW), S.d(aU), S.d(aM), S.d(aR)); },
        [&] { return hip_ok(h0, hipMemcpy(R.res.data(), S.d(aR), c * sizeof(UpdResult), hipMemcpyDeviceToHost), "d2h update states"); });
}
// a round without right-hand sides
template <class Launch> static int run_upd_round(blu_hip *h0, blu_hip **hs, UpdRound &R, const char *what, Launch launch)
{
    return run_upd_round(h0, hs, R, UpdRhs(), what, launch);
}

// the row-wise L of the members in `list` (their buffers exist: ensure_lt_ws), one workgroup each in one launch.  If the
// round fails its members get the code in result[]; the caller takes them off its own lists.
static int build_lt_batch(blu_hip *h0, blu_hip **hs, const std::vector<int> &list, std::vector<int> &result)
{
    if (list.empty()) return BLU_OK;
    UpdRound lt;
    UpdMember M;
    memset(&M, 0, sizeof M);
    lt.list = list;
    lt.mem.assign(list.size(), M);
    const int st = run_upd_round(h0, hs, lt, "k_build_lt_batch",
                                 [](int c, hipStream_t stream, const DevLU *dD, const FinishOut *, const SparseWs *dW, const UpdWs *,
                                    const UpdMember *, UpdResult *) { hipLaunchKernelGGL(k_build_lt_batch, dim3(c), dim3(1024), 0, stream, dD, dW); });
    if (st != BLU_OK) fail_members(h0, hs, list, result, st);
    else
        for (int k : list) hs[k]->lt_for_nfact = hs[k]->nfactorize;
    return st;
}

// ensure_upd for the members in `list`: workspaces per member where they do not exist yet, then the row-wise L and the
// update workspace of those that need them in one launch each.  Members that fail get their status in result[] and
// leave the list.
static void ensure_upd_batch(blu_hip *h0, blu_hip **hs, std::vector<int> &list, std::vector<int> &result)
{
    std::vector<int> lt;
    UpdRound init;
    for (int k : list) {
        blu_hip *h = hs[k];
        int st = ensure_sparse_ws(h);
        const bool need_lt = st == BLU_OK && h->lt_for_nfact != h->nfactorize;
        if (need_lt) st = ensure_lt_ws(h);
        const bool need_init = st == BLU_OK && h->upd_for_nfact != h->nfactorize;
        if (need_init) st = ensure_upd_ws(h);
        if (st != BLU_OK) {
            result[k] = st;
            continue;
        }
        if (need_lt) lt.push_back(k);
        if (need_init) { // the totals count over the life of the handle: LU::reset leaves them (lu.rs:329-359)
            UpdMember M;
            memset(&M, 0, sizeof M);
            M.carry[0] = h->ust.nsymperm_total;
            M.carry[1] = h->ust.nunsymperm_total;
            M.carry[2] = h->ust.nforrest_total;
            init.list.push_back(k);
            init.mem.push_back(M);
        }
    }
    keep_pending(list, result);
    if (build_lt_batch(h0, hs, lt, result) != BLU_OK) { // (a member that lost its row-wise L does not go on)
        keep_pending(list, result);
        UpdRound rest;
        for (size_t s = 0; s < init.list.size(); s++)
            if (result[init.list[s]] == kPending) {
                rest.list.push_back(init.list[s]);
                rest.mem.push_back(init.mem[s]);
            }
        init = rest;
    }
    if (init.list.empty()) return;
    const int st = run_upd_round(h0, hs, init, "k_upd_init_batch",
                                 [](int c, hipStream_t stream, const DevLU *dD, const FinishOut *dO, const SparseWs *, const UpdWs *dU,
                                    const UpdMember *dM, UpdResult *dR) {
                                     hipLaunchKernelGGL(k_upd_init_batch, dim3(c), dim3(1024), 0, stream, dD, dO, dU, dM, dR);
                                 });
    if (st != BLU_OK) {
        fail_members(h0, hs, init.list, result, st);
        keep_pending(list, result);
        return;
    }
    for (size_t s = 0; s < init.list.size(); s++) {
        blu_hip *h = hs[init.list[s]];
        h->ust = init.res[s].st;
        h->upd_for_nfact = h->nfactorize;
    }
}

// what the kernel of the update path answered for member h (upd: k_update_batch, else k_solve_upd_batch): its status
// when it is done, or kPending when it asked for storage, got it and is to be launched again
static int take_upd_result(blu_hip *h, const UpdResult &res, bool upd)
{
    h->marker += 4;
    h->ust = res.st;
    const int us = h->ust.status;
    if (us == UPD_OK) {
        if (upd) h->nupdate++;
        return BLU_OK;
    }
    if (upd && us == UPD_SINGULAR) return BLU_ERROR_SINGULAR_UPDATE; // the old factorization is still valid
    if (us == UPD_ERROR) return upd_invariant_violated(h, upd ? "update" : "update path");
    const int g = grow_upd(h);
    return g == BLU_OK ? kPending : g;
}

// the storage-request loop over the members in `active` (run_solve_upd / the loop of blu_hip_update for one handle):
// kind 0 = k_solve_upd_batch as solve_for_update (mode 1), 1 = k_update_batch, 2 = k_solve_upd_batch as solve_sparse
// (mode 0: blu_solve_sparse_batch.inc).  mem[k] is what member k is handed (marker filled in here); on return
// result[k] is set for every member and, for a solve that ended well, out[k] holds its counters.
static void run_upd_batch(blu_hip *h0, blu_hip **hs, std::vector<int> active, std::vector<int> &result, int kind, int tr,
                          const std::vector<UpdMember> &mem, const UpdRhs &rhs, std::vector<UpdResult> &out)
{
    const bool upd = kind == 1;
    const int mode = kind == 0 ? 1 : 0;
    const char *what = upd ? "k_update_batch" : "k_solve_upd_batch";
    for (int attempt = 0; attempt < 64 && !active.empty(); attempt++) {
        UpdRound R;
        for (int k : active) {
            blu_hip *h = hs[k];
            const int st = marker_room(h);
            if (st != BLU_OK) {
                result[k] = st;
                continue;
            }
            UpdMember M = mem[(size_t)k];
            M.marker = h->marker;
            R.list.push_back(k);
            R.mem.push_back(M);
        }
        active.clear();
        if (R.list.empty()) break;
        int st;
        if (upd)
            st = run_upd_round(h0, hs, R, rhs, what,
                               [](int c, hipStream_t stream, const DevLU *dD, const FinishOut *, const SparseWs *dW, const UpdWs *dU,
                                  const UpdMember *dM, UpdResult *dR) { hipLaunchKernelGGL(k_update_batch, dim3(c), dim3(64), 0, stream, dD, dW, dU, dM, dR); });
        else
            st = run_upd_round(h0, hs, R, rhs, what,
                               [mode, tr](int c, hipStream_t stream, const DevLU *dD, const FinishOut *, const SparseWs *dW, const UpdWs *dU,
                                    const UpdMember *dM, UpdResult *dR) {
                                   hipLaunchKernelGGL(k_solve_upd_batch, dim3(c), dim3(64), 0, stream, dD, dW, dU, dM, dR, mode, tr);
                               });
        if (st != BLU_OK) {
            fail_members(h0, hs, R.list, result, st);
            return;
        }
        for (size_t s = 0; s < R.list.size(); s++) {
            const int k = R.list[s];
            result[k] = take_upd_result(hs[k], R.res[s], upd);
            if (result[k] == BLU_OK) out[(size_t)k] = R.res[s];
            else if (result[k] == kPending) active.push_back(k);
        }
    }
    for (int k : active) {
        hs[k]->err = upd ? "update: too many storage requests" : "update path: too many storage requests";
        result[k] = BLU_ERROR_DEVICE;
    }
}

// the counters of a sparse solve that ended well, as fetch_solution takes them
static void take_solve_counters(blu_hip *h, const UpdResult &r)
{
    h->sp_l_flops += r.out[1];
    h->sp_u_flops += r.out[2];
    h->sp_branch = (int)r.out[3];
}

// The compressed solutions of the members in `got` -- member got[s] has off[s + 1] - off[s] entries -- gathered on the
// device, one copy down, and unpacked into the caller's arrays.  Nothing happens when there is no entry at all; if the
// round fails, the members of `got` fail.
static void gather_solutions(blu_hip *h0, blu_hip **hs, const std::vector<int> &got, const std::vector<long long> &off,
                             std::vector<int> &result, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs)
{
    const size_t c = got.size(), tot = (size_t)off.back();
    if (tot == 0) return;
    Stage S;
    const auto aW = S.add<SparseWs>(c);
    const auto aF = S.add<long long>(c + 1);
    const auto aV = S.add<double>(tot); // (values and patterns: written by the kernel, not uploaded)
    const auto aI = S.add<int>(tot);
    S.host_front(aV.off);
    for (size_t s = 0; s < c; s++) S.h(aW)[s] = hs[got[s]]->sw;
    memcpy(S.h(aF), off.data(), (c + 1) * sizeof(long long));
    std::vector<char> down(S.bytes - aV.off);
    int st = stage_alloc(h0, S);
    if (st == BLU_OK)
        st = stage_run(
            h0, S, "h2d gather descriptors", "k_gather_lhs_batch",
            [&](hipStream_t stream) {
                hipLaunchKernelGGL(k_gather_lhs_batch, dim3((unsigned)c), dim3(256), 0, stream, S.d(aW), S.d(aF), S.d(aI), S.d(aV));
            },
            [&] { return hip_ok(h0, hipMemcpy(down.data(), S.d(aV), down.size(), hipMemcpyDeviceToHost), "d2h solutions"); });
    if (st != BLU_OK) {
        fail_members(h0, hs, got, result, st);
        return;
    }
    const double *xv = (const double *)down.data();
    const int *il = (const int *)(down.data() + (aI.off - aV.off));
    for (size_t s = 0; s < c; s++) {
        const int k = got[s];
        for (long long p = off[s]; p < off[s + 1]; p++) { // pattern in the reference's order, values into the caller's (all-zero) lhs
            ilhs[k][p - off[s]] = il[p];
            lhs[k][il[p]] = xv[p];
        }
        nzlhs[k] = off[s + 1] - off[s];
    }
}

// The call behind its refusals as a whole, for the members whose result[k] is still kPending: the checks of each member in
// the order of blu_hip_solve_for_update, the storage-request loop, the counters.  want[k] != 0: member k's kernel leaves
// the compressed solution in its sw.ilhs / sw.xval / sw.out[0] on the device; gather[k] != 0 (only with want[k]): it is
// downloaded into nzlhs[k] / ilhs[k] / lhs[k] as well.  blu_hip_tableau_row_batch (blu_matrix_batch.inc) wants every
// member's and gathers the ones its caller asked for.
static void solve_for_update_batch_core(blu_hip *h0, blu_hip **hs, int n, const int64_t *nzrhs, const uint64_t *const *irhs,
                                        const double *const *xrhs, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, int tr,
                                        const std::vector<char> &want, const std::vector<char> &gather, std::vector<int> &result)
{
    std::vector<int> active;
    for (int k = 0; k < n; k++) {
        if (result[k] != kPending) continue;
        if (hs[k]->nupdate < 0) result[k] = BLU_ERROR_INVALID_CALL;     // solve_for_update.rs:85-86
        else if (hs[k]->m == 0) result[k] = BLU_ERROR_INVALID_ARGUMENT;
        else active.push_back(k);
    }
    ensure_upd_batch(h0, hs, active, result);
    std::vector<UpdMember> mem((size_t)n);
    UpdRhs rhs;
    rhs.off.assign((size_t)n, 0);
    {
        std::vector<int> kept;
        for (int k : active) {
            blu_hip *h = hs[k];
            if (h->ust.nforrest == h->m) { // :87-88
                result[k] = BLU_ERROR_MAXIMUM_UPDATES;
                continue;
            }
            const int64_t nz = tr ? 1 : nzrhs[k];
            bool ok;
            if (tr) {
                ok = irhs[k][0] < (uint64_t)h->m;
            } else {
                ok = nz >= 0 && nz <= h->m;
                for (int64_t q = 0; ok && q < nz; q++) ok = irhs[k][q] < (uint64_t)h->m;
            }
            if (!ok) {
                result[k] = BLU_ERROR_INVALID_ARGUMENT;
                continue;
            }
            UpdMember &M = mem[(size_t)k];
            memset(&M, 0, sizeof M);
            M.want_solution = want[(size_t)k] ? 1 : 0;
            if (gather[(size_t)k]) nzlhs[k] = 0;
            M.nrhs = (int)nz;
            M.nz_sparse = (int)(h->sparse_thres * (double)h->m);
            rhs.off[(size_t)k] = rhs.ir.size();
            for (int64_t q = 0; q < nz; q++) rhs.ir.push_back((int)irhs[k][q]);
            if (!tr) rhs.xr.insert(rhs.xr.end(), xrhs[k], xrhs[k] + nz);
            kept.push_back(k);
        }
        active.swap(kept);
    }
    if (tr) rhs.xr.assign(rhs.ir.size(), 0.0); // (never read: one layout for both systems)
    std::vector<UpdResult> out((size_t)n);
    run_upd_batch(h0, hs, active, result, 0, tr, mem, rhs, out);

    // the counters, then the compressed solutions of every member that asked for one (the empty ones included)
    std::vector<int> got;
    std::vector<long long> off(1, 0);
    for (int k : active) {
        if (result[k] != BLU_OK) continue;
        take_solve_counters(hs[k], out[(size_t)k]);
        if (!gather[(size_t)k]) continue;
        got.push_back(k);
        off.push_back(off.back() + out[(size_t)k].out[0]);
    }
    gather_solutions(h0, hs, got, off, result, nzlhs, ilhs, lhs);
}

extern "C" int blu_hip_solve_for_update_batch(blu_hip **hs, int n, const int64_t *nzrhs, const uint64_t *const *irhs, const double *const *xrhs,
                                              int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, char trans, int *status)
{
    // refusals of the call as a whole: every status[k] carries the code, no handle is touched
    const int tr = (trans == 't' || trans == 'T') ? 1 : 0;
    if (!hs || !irhs || n < 0 || (!tr && (!xrhs || !nzrhs))) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (!irhs[k] || (!tr && !xrhs[k])) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (const int st = batch_handles_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);
    const bool want_any = nzlhs && ilhs && lhs;
    std::vector<char> want((size_t)n, 0);
    for (int k = 0; k < n; k++) want[(size_t)k] = (want_any && ilhs[k] && lhs[k]) ? 1 : 0;
    std::vector<int> result(n, kPending);
    solve_for_update_batch_core(h0, hs, n, nzrhs, irhs, xrhs, nzlhs, ilhs, lhs, tr, want, want, result);
    return batch_return(result, status);
}

extern "C" int blu_hip_update_batch(blu_hip **hs, int n, const double *xtbl, int *status)
{
    if (!hs || !xtbl || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    if (const int st = batch_handles_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);
    std::vector<int> result(n, kPending), active;
    std::vector<UpdMember> mem((size_t)n);
    for (int k = 0; k < n; k++) {
        blu_hip *h = hs[k];
        if (h->nupdate < 0 || h->upd_for_nfact != h->nfactorize || h->ust.ftran_for < 0 || h->ust.btran_for < 0) {
            result[k] = BLU_ERROR_INVALID_CALL;
            continue;
        }
        memset(&mem[(size_t)k], 0, sizeof(UpdMember));
        mem[(size_t)k].xtbl = xtbl[k];
        active.push_back(k);
    }
    std::vector<UpdResult> out((size_t)n);
    run_upd_batch(h0, hs, active, result, 1, 0, mem, UpdRhs(), out);
    return batch_return(result, status);
}
