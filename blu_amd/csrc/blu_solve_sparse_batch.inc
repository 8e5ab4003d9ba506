// blu_solve_sparse_batch.inc -- blu_hip_solve_sparse_batch (included by blu_hip.hip): blu_hip_solve_sparse for many
// handles in one call.  Each member runs on one wave, the members of a kind in one launch:
//   k_build_lt_batch      row-wise L of the fresh members of a transposed call that do not have it yet
//   k_solve_sparse_batch  fresh factorizations (nupdate == 0): the body of k_solve_sparse
//   k_solve_upd_batch     updated factorizations (nupdate > 0): the body of k_solve_upd, mode 0
//   k_gather_lhs_batch    the compressed solutions into one buffer
// The solves are one round of blu_update_batch.inc (run_upd_round: one upload of descriptors, member records and the
// packed right-hand sides, one synchronize, one download of the result slots) with the fresh members in front and both
// kernels launched behind each other.  An updated member whose kernel answers with a storage request -- unexpected for
// mode 0 -- is grown and launched again through run_upd_batch, as blu_hip_solve_sparse does for one handle.

extern "C" int blu_hip_solve_sparse_batch(blu_hip **hs, int n, const int64_t *nzrhs, const uint64_t *const *irhs, const double *const *xrhs,
                                          int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, char trans, int *status)
{
    // refusals of the call as a whole: every status[k] carries the code, no handle is touched
    auto fail_all = [&](int code) {
        if (status)
            for (int k = 0; k < n; k++) status[k] = code;
        return code;
    };
    if (!hs || !nzrhs || !nzlhs || !ilhs || !lhs || n < 0) return fail_all(BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++) {
        if (!hs[k] || !ilhs[k] || !lhs[k]) return fail_all(BLU_ERROR_ARGUMENT_MISSING);
        if (nzrhs[k] > 0 && (!irhs || !xrhs || !irhs[k] || !xrhs[k])) return fail_all(BLU_ERROR_ARGUMENT_MISSING);
    }
    {
        const int st = upd_batch_refusal(hs, n);
        if (st != BLU_OK) return fail_all(st);
    }
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return fail_all(BLU_ERROR_DEVICE);
    const int tr = (trans == 't' || trans == 'T') ? 1 : 0;

    // per member, in the order of blu_hip_solve_sparse
    std::vector<int> result(n, kPending), fresh, updated;
    UpdRound lt;
    for (int k = 0; k < n; k++) {
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
        nzlhs[k] = 0;
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
        if (need_lt) {
            UpdMember M;
            memset(&M, 0, sizeof M);
            lt.list.push_back(k);
            lt.mem.push_back(M);
        }
        (h->nupdate > 0 ? updated : fresh).push_back(k);
    }
    const std::vector<int> no_i;
    const std::vector<double> no_x;
    const std::vector<size_t> no_off;
    if (!lt.list.empty()) {
        const int st = run_upd_round(h0, hs, lt, no_i, no_x, no_off, "k_build_lt_batch",
                                     [](int c, hipStream_t stream, const DevLU *dD, const FinishOut *, const SparseWs *dW, const UpdWs *,
                                        const UpdMember *, UpdResult *) { hipLaunchKernelGGL(k_build_lt_batch, dim3(c), dim3(1024), 0, stream, dD, dW); });
        if (st != BLU_OK) {
            fail_members(h0, hs, lt.list, result, st);
            std::vector<int> rest;
            for (int k : fresh)
                if (result[k] == kPending) rest.push_back(k);
            fresh.swap(rest);
        } else {
            for (int k : lt.list) hs[k]->lt_for_nfact = hs[k]->nfactorize;
        }
    }
    ensure_upd_batch(h0, hs, updated, result); // (a no-op once an update was made: it needed the same)

    // the round: fresh members in front, every right-hand side of the call packed behind the descriptors
    UpdRound R;
    std::vector<UpdMember> mem((size_t)n);
    std::vector<size_t> rhs_off((size_t)n, 0);
    std::vector<int> ir;
    std::vector<double> xr;
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
            rhs_off[(size_t)k] = ir.size();
            for (int64_t q = 0; q < nzrhs[k]; q++) ir.push_back((int)irhs[k][q]);
            if (nzrhs[k] > 0) xr.insert(xr.end(), xrhs[k], xrhs[k] + nzrhs[k]);
            R.list.push_back(k);
            R.mem.push_back(M);
        }
    std::vector<UpdResult> out((size_t)n);
    if (!R.list.empty()) {
        const int st = run_upd_round(h0, hs, R, ir, xr, rhs_off, "k_solve_sparse_batch",
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
            blu_hip *h = hs[k];
            if ((int)s < nf) {
                h->marker += 3;
                out[(size_t)k] = R.res[s];
                result[k] = BLU_OK;
                continue;
            }
            h->marker += 4;
            h->ust = R.res[s].st;
            if (h->ust.status == UPD_OK) {
                out[(size_t)k] = R.res[s];
                result[k] = BLU_OK;
            } else if (h->ust.status == UPD_ERROR) {
                char buf[128];
                snprintf(buf, sizeof buf, "update path: invariant violated at kernel source line %d", h->ust.err_line);
                h->err = buf;
                h->nupdate = -1;
                result[k] = BLU_ERROR_DEVICE;
            } else {
                const int g = grow_upd(h);
                if (g == BLU_OK) again.push_back(k);
                else result[k] = g;
            }
        }
        if (!again.empty()) run_upd_batch(h0, hs, again, result, 2, tr, mem, ir, xr, rhs_off, out);
    }

    // the counters as blu_hip_solve_sparse takes them, then the compressed solutions: gathered on the device, one copy down
    std::vector<int> got;
    std::vector<long long> off(1, 0);
    for (int k : R.list) {
        if (result[k] != BLU_OK) continue;
        blu_hip *h = hs[k];
        h->sp_l_flops += out[(size_t)k].out[1];
        h->sp_u_flops += out[(size_t)k].out[2];
        h->sp_branch = (int)out[(size_t)k].out[3];
        if (out[(size_t)k].out[0] <= 0) continue;
        got.push_back(k);
        off.push_back(off.back() + out[(size_t)k].out[0]);
    }
    if (!got.empty()) {
        const size_t c = got.size(), tot = (size_t)off.back();
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
