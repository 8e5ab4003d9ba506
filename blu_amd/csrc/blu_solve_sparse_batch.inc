// blu_solve_sparse_batch.inc -- blu_hip_solve_sparse_batch (included by blu_hip.hip): blu_hip_solve_sparse for many
// handles in one call.  Each member runs on one wave, the members of a kind in one launch:
//   k_build_lt_batch      row-wise L of the fresh members of a transposed call that do not have it yet
//   k_solve_sparse_batch  fresh factorizations (nupdate == 0): the body of k_solve_sparse
//   k_solve_upd_batch     updated factorizations (nupdate > 0): the body of k_solve_upd, mode 0
//   k_gather_lhs_batch    the compressed solutions into one buffer
// Everything around the kernels is shared with blu_update_batch.inc: the solves are one round of run_upd_round (one
// upload of descriptors, member records and the packed right-hand sides, one synchronize, one download of the result
// slots) with the fresh members in front and both kernels launched behind each other; build_lt_batch, take_upd_result
// and gather_solutions are the ones of the update entries.  An updated member whose kernel answers with a storage
// request -- unexpected for mode 0 -- is grown and launched again through run_upd_batch, as blu_hip_solve_sparse does
// for one handle.  Refusals and the return value: blu_batch.inc.

// The call behind its refusals as a whole, for the members whose result[k] is still kPending: the checks of each member in
// the order of blu_hip_solve_sparse, the round, the counters.  gather[k] != 0: member k's compressed solution is downloaded
// into nzlhs[k] / ilhs[k] / lhs[k]; every member's stays in its sw.ilhs / sw.xval / sw.out[0] on the device, which is what
// blu_hip_tableau_row_batch (blu_matrix_batch.inc) goes on from.
static void solve_sparse_batch_core(blu_hip *h0, blu_hip **hs, int n, const int64_t *nzrhs, const uint64_t *const *irhs, const double *const *xrhs,
                                    int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, int tr, const std::vector<char> &gather,
                                    std::vector<int> &result)
{
    std::vector<int> fresh, updated, lt;
    for (int k = 0; k < n; k++) {
        if (result[k] != kPending) continue;
        blu_hip *h = hs[k];
        if (h->nupdate < 0) { // solve_sparse.rs:46-47
            result[k] = BLU_ERROR_INVALID_CALL;
            continue;
        }
        bool ok = nzrhs[k] >= 0 && nzrhs[k] <= h->m; // :49-59
        for (int64_t q = 0; ok && q < nzrhs[k]; q++) ok = irhs[k][q] < (uint64_t)h->m;
        if (!ok) {
            result[k] = BLU_ERROR_INVALID_ARGUMENT;
            continue;
        }
        if (gather[(size_t)k]) nzlhs[k] = 0;
        if (h->m == 0) {
            result[k] = BLU_OK;
            continue;
        }
        int st = ensure_sparse_ws(h);
        if (st == BLU_OK && h->marker > 0x7fffffff - 8) { // lu.rs:301-305: reset the marks before the marker overflows
            if (hip_ok(h, hipMemset(h->sw.marked, 0, (size_t)h->m * sizeof(int)), "hipMemset")) h->marker = 0;
            else st = BLU_ERROR_DEVICE;
        }
        const bool need_lt = st == BLU_OK && h->nupdate == 0 && tr && h->lt_for_nfact != h->nfactorize; // the transposed system ends with L'
        if (need_lt) st = ensure_lt_ws(h);
        if (st != BLU_OK) {
            result[k] = st;
            continue;
        }
        if (need_lt) lt.push_back(k);
        (h->nupdate > 0 ? updated : fresh).push_back(k);
    }
    if (build_lt_batch(h0, hs, lt, result) != BLU_OK) keep_pending(fresh, result);
    ensure_upd_batch(h0, hs, updated, result); // (a no-op once an update was made: it needed the same)

    // the round: fresh members in front, every right-hand side of the call packed behind the descriptors
    UpdRound R;
    std::vector<UpdMember> mem((size_t)n);
    UpdRhs rhs;
    rhs.off.assign((size_t)n, 0);
    const int nf = (int)fresh.size();
    for (int pass = 0; pass < 2; pass++)
        for (int k : pass ? updated : fresh) {
            blu_hip *h = hs[k];
            if (pass) {
                const int st = marker_room(h);
                if (st != BLU_OK) {
                    result[k] = st;
                    continue;
                }
            }
            UpdMember &M = mem[(size_t)k];
            memset(&M, 0, sizeof M);
            M.want_solution = 1;
            M.nrhs = (int)nzrhs[k];
            M.nz_sparse = (int)(h->sparse_thres * (double)h->m); // lu/solve_sparse.rs:24
            M.marker = h->marker;
            rhs.off[(size_t)k] = rhs.ir.size();
            for (int64_t q = 0; q < nzrhs[k]; q++) rhs.ir.push_back((int)irhs[k][q]);
            if (nzrhs[k] > 0) rhs.xr.insert(rhs.xr.end(), xrhs[k], xrhs[k] + nzrhs[k]);
            R.list.push_back(k);
            R.mem.push_back(M);
        }
    std::vector<UpdResult> out((size_t)n);
    if (!R.list.empty()) {
        const int st = run_upd_round(h0, hs, R, rhs, "k_solve_sparse_batch",
                                     [nf, tr](int c, hipStream_t stream, const DevLU *dD, const FinishOut *dO, const SparseWs *dW, const UpdWs *dU,
                                              const UpdMember *dM, UpdResult *dR) {
                                         if (nf > 0) hipLaunchKernelGGL(k_solve_sparse_batch, dim3(nf), dim3(64), 0, stream, dD, dO, dW, dM, dR, tr);
                                         if (c > nf)
                                             hipLaunchKernelGGL(k_solve_upd_batch, dim3(c - nf), dim3(64), 0, stream, dD + nf, dW + nf, dU + nf,
                                                                dM + nf, dR + nf, 0, tr);
                                     });
        if (st != BLU_OK) fail_members(h0, hs, R.list, result, st);
        std::vector<int> again; // updated members that asked for storage
        for (size_t s = 0; st == BLU_OK && s < R.list.size(); s++) {
            const int k = R.list[s];
            if ((int)s < nf) {
                hs[k]->marker += 3;
                result[k] = BLU_OK;
            } else {
                result[k] = take_upd_result(hs[k], R.res[s], false);
            }
            if (result[k] == BLU_OK) out[(size_t)k] = R.res[s];
            else if (result[k] == kPending) again.push_back(k);
        }
        if (!again.empty()) run_upd_batch(h0, hs, again, result, 2, tr, mem, rhs, out);
    }

    // the counters as blu_hip_solve_sparse takes them, then the compressed solutions of the members that have entries
    std::vector<int> got;
    std::vector<long long> off(1, 0);
    for (int k : R.list) {
        if (result[k] != BLU_OK) continue;
        take_solve_counters(hs[k], out[(size_t)k]);
        if (out[(size_t)k].out[0] <= 0 || !gather[(size_t)k]) continue;
        got.push_back(k);
        off.push_back(off.back() + out[(size_t)k].out[0]);
    }
    gather_solutions(h0, hs, got, off, result, nzlhs, ilhs, lhs);
}

extern "C" int blu_hip_solve_sparse_batch(blu_hip **hs, int n, const int64_t *nzrhs, const uint64_t *const *irhs, const double *const *xrhs,
                                          int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, char trans, int *status)
{
    // refusals of the call as a whole: every status[k] carries the code, no handle is touched
    if (!hs || !nzrhs || !nzlhs || !ilhs || !lhs || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++) {
        if (!hs[k] || !ilhs[k] || !lhs[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
        if (nzrhs[k] > 0 && (!irhs || !xrhs || !irhs[k] || !xrhs[k])) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    }
    if (const int st = batch_handles_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);
    std::vector<int> result(n, kPending);
    solve_sparse_batch_core(h0, hs, n, nzrhs, irhs, xrhs, nzlhs, ilhs, lhs, (trans == 't' || trans == 'T') ? 1 : 0, std::vector<char>((size_t)n, 1),
                            result);
    return batch_return(result, status);
}
