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

// what a round needs on the device, for the members listed in `list` (indices into hs): descriptors, the UpdMember
// records, the result slots, and the packed right-hand sides of the whole call (ir / xr, member k's at rhs_off[k])
struct UpdRound {
    std::vector<int> list;
    std::vector<UpdMember> mem; // mem[s] of list[s]; irhs / xrhs are filled in here
    std::vector<UpdResult> res; // OUT
};

template <class Launch>
static int run_upd_round(blu_hip *h0, blu_hip **hs, UpdRound &R, const std::vector<int> &ir, const std::vector<double> &xr,
                         const std::vector<size_t> &rhs_off, const char *what, Launch launch)
{
    const size_t c = R.list.size();
    const size_t oD = 0, oO = align_up(oD + c * sizeof(DevLU)), oW = align_up(oO + c * sizeof(FinishOut)), oU = align_up(oW + c * sizeof(SparseWs)),
                 oM = align_up(oU + c * sizeof(UpdWs)), oX = align_up(oM + c * sizeof(UpdMember)), oI = align_up(oX + xr.size() * sizeof(double)),
                 oR = align_up(oI + ir.size() * sizeof(int)), total = oR + c * sizeof(UpdResult);
    char *dbuf = nullptr;
    if (!hip_ok(h0, hipMalloc((void **)&dbuf, total), "hipMalloc")) {
        (void)hipGetLastError();
        return BLU_ERROR_OUT_OF_MEMORY;
    }
    std::vector<char> stage(oR, 0);
    DevLU *sD = (DevLU *)(stage.data() + oD);
    FinishOut *sO = (FinishOut *)(stage.data() + oO);
    SparseWs *sW = (SparseWs *)(stage.data() + oW);
    UpdWs *sU = (UpdWs *)(stage.data() + oU);
    UpdMember *sM = (UpdMember *)(stage.data() + oM);
    for (size_t s = 0; s < c; s++) {
        const int k = R.list[s];
        blu_hip *h = hs[k];
        sD[s] = h->D;
        sO[s] = h->O;
        sW[s] = h->sw;
        sU[s] = h->uw;
        sM[s] = R.mem[s];
        sM[s].irhs = ir.empty() ? nullptr : (const int *)(dbuf + oI) + rhs_off[(size_t)k];
        sM[s].xrhs = xr.empty() ? nullptr : (const double *)(dbuf + oX) + rhs_off[(size_t)k];
    }
    if (!xr.empty()) memcpy(stage.data() + oX, xr.data(), xr.size() * sizeof(double));
    if (!ir.empty()) memcpy(stage.data() + oI, ir.data(), ir.size() * sizeof(int));
    R.res.assign(c, UpdResult());
    hipStream_t stream = h0->stream;
    bool ok = hip_ok(h0, hipMemcpyAsync(dbuf, stage.data(), oR, hipMemcpyHostToDevice, stream), "h2d update descriptors");
    if (ok) {
        launch((int)c, stream, (const DevLU *)(dbuf + oD), (const FinishOut *)(dbuf + oO), (const SparseWs *)(dbuf + oW), (const UpdWs *)(dbuf + oU),
               (const UpdMember *)(dbuf + oM), (UpdResult *)(dbuf + oR));
        ok = hip_ok(h0, hipStreamSynchronize(stream), what) &&
             hip_ok(h0, hipMemcpy(R.res.data(), dbuf + oR, c * sizeof(UpdResult), hipMemcpyDeviceToHost), "d2h update states");
    }
    (void)hipFree(dbuf);
    return ok ? BLU_OK : BLU_ERROR_DEVICE;
}

static void fail_members(blu_hip *h0, blu_hip **hs, const std::vector<int> &list, std::vector<int> &result, int code)
{
    for (int k : list) {
        if (hs[k] != h0) hs[k]->err = h0->err;
        result[k] = code;
    }
}

// ensure_upd for the members in `list`: workspaces per member where they do not exist yet, then the row-wise L and the
// update workspace of those that need them in one launch each.  Members that fail get their status in result[] and
// leave the list.
static void ensure_upd_batch(blu_hip *h0, blu_hip **hs, std::vector<int> &list, std::vector<int> &result)
{
    UpdRound lt, init;
    std::vector<int> kept;
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
        kept.push_back(k);
        UpdMember M;
        memset(&M, 0, sizeof M);
        if (need_lt) {
            lt.list.push_back(k);
            lt.mem.push_back(M);
        }
        if (need_init) { // the totals count over the life of the handle: LU::reset leaves them (lu.rs:329-359)
            M.carry[0] = h->ust.nsymperm_total;
            M.carry[1] = h->ust.nunsymperm_total;
            M.carry[2] = h->ust.nforrest_total;
            init.list.push_back(k);
            init.mem.push_back(M);
        }
    }
    list.swap(kept);
    const std::vector<int> no_i;
    const std::vector<double> no_x;
    const std::vector<size_t> no_off;
    auto drop = [&](const std::vector<int> &failed, int code) {
        fail_members(h0, hs, failed, result, code);
        std::vector<int> rest;
        for (int k : list)
            if (result[k] == kPending) rest.push_back(k);
        list.swap(rest);
    };
    if (!lt.list.empty()) {
        const int st = run_upd_round(h0, hs, lt, no_i, no_x, no_off, "k_build_lt_batch",
                                     [](int c, hipStream_t stream, const DevLU *dD, const FinishOut *, const SparseWs *dW, const UpdWs *,
                                        const UpdMember *, UpdResult *) { hipLaunchKernelGGL(k_build_lt_batch, dim3(c), dim3(1024), 0, stream, dD, dW); });
        if (st != BLU_OK) drop(lt.list, st);
        else
            for (int k : lt.list) hs[k]->lt_for_nfact = hs[k]->nfactorize;
    }
    std::vector<int> todo;
    for (int k : init.list)
        if (result[k] == kPending) todo.push_back(k);
    if (todo.size() != init.list.size()) { // (a member that lost its row-wise L above does not go on)
        UpdRound r2;
        for (size_t s = 0; s < init.list.size(); s++)
            if (result[init.list[s]] == kPending) {
                r2.list.push_back(init.list[s]);
                r2.mem.push_back(init.mem[s]);
            }
        init = r2;
    }
    if (!init.list.empty()) {
        const int st = run_upd_round(h0, hs, init, no_i, no_x, no_off, "k_upd_init_batch",
                                     [](int c, hipStream_t stream, const DevLU *dD, const FinishOut *dO, const SparseWs *, const UpdWs *dU,
                                        const UpdMember *dM, UpdResult *dR) {
                                         hipLaunchKernelGGL(k_upd_init_batch, dim3(c), dim3(1024), 0, stream, dD, dO, dU, dM, dR);
                                     });
        if (st != BLU_OK) drop(init.list, st);
        else
            for (size_t s = 0; s < init.list.size(); s++) {
                blu_hip *h = hs[init.list[s]];
                h->ust = init.res[s].st;
                h->upd_for_nfact = h->nfactorize;
            }
    }
}

// the storage-request loop over the members in `active` (run_solve_upd / the loop of blu_hip_update for one handle):
// kind 0 = k_solve_upd_batch as solve_for_update (mode 1), 1 = k_update_batch, 2 = k_solve_upd_batch as solve_sparse
// (mode 0: blu_solve_sparse_batch.inc).  mem[k] is what member k is handed (marker filled in here); on return
// result[k] is set for every member and, for a solve that ended well, out[k] holds its counters.
static void run_upd_batch(blu_hip *h0, blu_hip **hs, std::vector<int> active, std::vector<int> &result, int kind, int tr,
                          const std::vector<UpdMember> &mem, const std::vector<int> &ir, const std::vector<double> &xr,
                          const std::vector<size_t> &rhs_off, std::vector<UpdResult> &out)
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
            st = run_upd_round(h0, hs, R, ir, xr, rhs_off, what,
                               [](int c, hipStream_t stream, const DevLU *dD, const FinishOut *, const SparseWs *dW, const UpdWs *dU,
                                  const UpdMember *dM, UpdResult *dR) { hipLaunchKernelGGL(k_update_batch, dim3(c), dim3(64), 0, stream, dD, dW, dU, dM, dR); });
        else
            st = run_upd_round(h0, hs, R, ir, xr, rhs_off, what,
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
            blu_hip *h = hs[k];
            h->marker += 4;
            h->ust = R.res[s].st;
            const int us = h->ust.status;
            if (us == UPD_OK) {
                if (upd) h->nupdate++;
                out[(size_t)k] = R.res[s];
                result[k] = BLU_OK;
            } else if (upd && us == UPD_SINGULAR) {
                result[k] = BLU_ERROR_SINGULAR_UPDATE; // the old factorization is still valid
            } else if (us == UPD_ERROR) {
                char buf[128];
                snprintf(buf, sizeof buf, "%s: invariant violated at kernel source line %d", upd ? "update" : "update path", h->ust.err_line);
                h->err = buf;
                h->nupdate = -1; // the factors may be half modified: invalid from here on
                result[k] = BLU_ERROR_DEVICE;
            } else {
                const int g = grow_upd(h);
                if (g == BLU_OK) active.push_back(k);
                else result[k] = g;
            }
        }
    }
    for (int k : active) {
        hs[k]->err = upd ? "update: too many storage requests" : "update path: too many storage requests";
        result[k] = BLU_ERROR_DEVICE;
    }
}

// the refusals the batch entries of the update path and blu_hip_solve_sparse_batch share; BLU_OK = go on
static int upd_batch_refusal(blu_hip **hs, int n)
{
    for (int k = 0; k < n; k++)
        if (!hs[k]) return BLU_ERROR_ARGUMENT_MISSING;
    for (int k = 0; k < n; k++)
        if (hs[k]->device != hs[0]->device) return BLU_ERROR_INVALID_ARGUMENT;
    if (n > 1) { // the same handle twice = two waves on one factorization: rejected
        std::vector<blu_hip *> sorted(hs, hs + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return BLU_ERROR_INVALID_ARGUMENT;
    }
    return BLU_OK;
}

// return value: the most negative error if any member failed, else the largest status
static int upd_batch_return(const std::vector<int> &result, int *status)
{
    int worst_err = 0, worst_pos = BLU_OK;
    for (size_t k = 0; k < result.size(); k++) {
        const int r = result[k] == kPending ? BLU_ERROR_DEVICE : result[k];
        if (status) status[k] = r;
        if (r < 0) worst_err = std::min(worst_err, r);
        else worst_pos = std::max(worst_pos, r);
    }
    return worst_err < 0 ? worst_err : worst_pos;
}

extern "C" int blu_hip_solve_for_update_batch(blu_hip **hs, int n, const int64_t *nzrhs, const uint64_t *const *irhs, const double *const *xrhs,
                                              int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, char trans, int *status)
{
    // refusals of the call as a whole: every status[k] carries the code, no handle is touched
    auto fail_all = [&](int code) {
        if (status)
            for (int k = 0; k < n; k++) status[k] = code;
        return code;
    };
    const int tr = (trans == 't' || trans == 'T') ? 1 : 0;
    if (!hs || !irhs || n < 0 || (!tr && (!xrhs || !nzrhs))) return fail_all(BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (!irhs[k] || (!tr && !xrhs[k])) return fail_all(BLU_ERROR_ARGUMENT_MISSING);
    {
        const int st = upd_batch_refusal(hs, n);
        if (st != BLU_OK) return fail_all(st);
    }
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return fail_all(BLU_ERROR_DEVICE);
    const bool want_any = nzlhs && ilhs && lhs;

    // per member, in the order of blu_hip_solve_for_update
    std::vector<int> result(n, kPending), active;
    for (int k = 0; k < n; k++) {
        if (hs[k]->nupdate < 0) result[k] = BLU_ERROR_INVALID_CALL;     // solve_for_update.rs:85-86
        else if (hs[k]->m == 0) result[k] = BLU_ERROR_INVALID_ARGUMENT;
        else active.push_back(k);
    }
    ensure_upd_batch(h0, hs, active, result);
    std::vector<UpdMember> mem((size_t)n);
    std::vector<size_t> rhs_off((size_t)n, 0);
    std::vector<int> ir;
    std::vector<double> xr;
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
            M.want_solution = (want_any && ilhs[k] && lhs[k]) ? 1 : 0;
            if (M.want_solution) nzlhs[k] = 0;
            M.nrhs = (int)nz;
            M.nz_sparse = (int)(h->sparse_thres * (double)h->m);
            rhs_off[(size_t)k] = ir.size();
            for (int64_t q = 0; q < nz; q++) ir.push_back((int)irhs[k][q]);
            if (!tr) xr.insert(xr.end(), xrhs[k], xrhs[k] + nz);
            kept.push_back(k);
        }
        active.swap(kept);
    }
    if (tr) xr.assign(ir.size(), 0.0); // (never read: one layout for both systems)
    std::vector<UpdResult> out((size_t)n);
    run_upd_batch(h0, hs, active, result, 0, tr, mem, ir, xr, rhs_off, out);

    // the counters as fetch_solution takes them, then the compressed solutions: gathered on the device, one copy down
    std::vector<int> got;
    std::vector<long long> off(1, 0);
    for (int k : active) {
        if (result[k] != BLU_OK) continue;
        blu_hip *h = hs[k];
        h->sp_l_flops += out[(size_t)k].out[1];
        h->sp_u_flops += out[(size_t)k].out[2];
        h->sp_branch = (int)out[(size_t)k].out[3];
        if (!mem[(size_t)k].want_solution) continue;
        got.push_back(k);
        off.push_back(off.back() + out[(size_t)k].out[0]);
    }
    const size_t tot = (size_t)off.back();
    if (tot > 0) {
        const size_t c = got.size();
        const size_t oW = 0, oF = align_up(oW + c * sizeof(SparseWs)), oV = align_up(oF + (c + 1) * sizeof(long long)),
                     oI = align_up(oV + tot * sizeof(double)), total = oI + tot * sizeof(int);
        std::vector<char> stage(oV, 0), down(total - oV);
        for (size_t s = 0; s < c; s++) ((SparseWs *)(stage.data() + oW))[s] = hs[got[s]]->sw;
        memcpy(stage.data() + oF, off.data(), (c + 1) * sizeof(long long));
        char *dbuf = nullptr;
        int st = BLU_OK;
        if (!hip_ok(h0, hipMalloc((void **)&dbuf, total), "hipMalloc")) {
            (void)hipGetLastError();
            st = BLU_ERROR_OUT_OF_MEMORY;
        } else {
            bool ok = hip_ok(h0, hipMemcpyAsync(dbuf, stage.data(), oV, hipMemcpyHostToDevice, h0->stream), "h2d gather descriptors");
            if (ok) {
                hipLaunchKernelGGL(k_gather_lhs_batch, dim3((unsigned)c), dim3(256), 0, h0->stream, (const SparseWs *)(dbuf + oW),
                                   (const long long *)(dbuf + oF), (int *)(dbuf + oI), (double *)(dbuf + oV));
                ok = hip_ok(h0, hipStreamSynchronize(h0->stream), "k_gather_lhs_batch") &&
                     hip_ok(h0, hipMemcpy(down.data(), dbuf + oV, total - oV, hipMemcpyDeviceToHost), "d2h solutions");
            }
            (void)hipFree(dbuf);
            if (!ok) st = BLU_ERROR_DEVICE;
        }
        if (st != BLU_OK) fail_members(h0, hs, got, result, st);
        else {
            const double *xv = (const double *)down.data();
            const int *il = (const int *)(down.data() + (oI - oV));
            for (size_t s = 0; s < c; s++) {
                const int k = got[s];
                for (long long p = off[s]; p < off[s + 1]; p++) { // pattern in the reference's order, values into the caller's (all-zero) lhs
                    ilhs[k][p - off[s]] = il[p];
                    lhs[k][il[p]] = xv[p];
                }
                nzlhs[k] = off[s + 1] - off[s];
            }
        }
    }
    return upd_batch_return(result, status);
}

extern "C" int blu_hip_update_batch(blu_hip **hs, int n, const double *xtbl, int *status)
{
    auto fail_all = [&](int code) {
        if (status)
            for (int k = 0; k < n; k++) status[k] = code;
        return code;
    };
    if (!hs || !xtbl || n < 0) return fail_all(BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    {
        const int st = upd_batch_refusal(hs, n);
        if (st != BLU_OK) return fail_all(st);
    }
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return fail_all(BLU_ERROR_DEVICE);
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
    const std::vector<int> no_i;
    const std::vector<double> no_x;
    const std::vector<size_t> no_off;
    std::vector<UpdResult> out((size_t)n);
    run_upd_batch(h0, hs, active, result, 1, 0, mem, no_i, no_x, no_off, out);
    return upd_batch_return(result, status);
}
