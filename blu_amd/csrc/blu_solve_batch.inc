// blu_solve_batch.inc -- blu_hip_solve_dense_batch (included by blu_hip.hip): blu_hip_solve_dense for many handles in
// one call.  Each member's system runs on one wave, the members of a kind in one launch:
//   k_build_lt_batch         row-wise L of the fresh factorizations a forward solve needs and does not have yet
//                            (one workgroup per member; the same array ensure_lt builds, kept for later calls)
//   k_solve_dense_batch      fresh factorizations (nupdate == 0): the sweeps of k_solve_dense
//   k_solve_dense_upd_batch  updated factorizations (nupdate > 0): the body of k_solve_dense_upd
// on one stream, one synchronize at the end.  The per-member descriptors are staged on the host and uploaded once: a
// Stage of blu_batch.inc, whose stage_alloc / stage_run are the round around the launches.  The refusals and the return
// value are those of blu_batch.inc as well.

// the row-wise L buffers alone -- what a forward dense solve reads -- for THIS factorization's L (ensure_lt allocates
// them with the whole solve_sparse workspace; ensure_sparse_ws keeps what is allocated here)
static int ensure_lt_ws(blu_hip *h)
{
    const size_t M = (size_t)h->m;
    SparseWs &W = h->sw;
    if (!W.lt_ptr && !dalloc(h, &W.lt_ptr, M + 1)) return BLU_ERROR_OUT_OF_MEMORY;
    if (!W.lt_cur && !dalloc(h, &W.lt_cur, M)) return BLU_ERROR_OUT_OF_MEMORY;
    const int64_t lnz = std::max<int64_t>((int64_t)h->hs.lused, 1);
    if (lnz > h->sw_ltcap) {
        dfree(W.lt_idx);
        dfree(W.lt_val);
        h->sw_ltcap = 0;
        h->lt_for_nfact = -1;
        if (!dalloc(h, &W.lt_idx, (size_t)lnz) || !dalloc(h, &W.lt_val, (size_t)lnz)) return BLU_ERROR_OUT_OF_MEMORY;
        h->sw_ltcap = lnz;
    }
    return BLU_OK;
}

extern "C" int blu_hip_solve_dense_batch(blu_hip **hs, int n, const double *const *rhs, double *const *lhs, char trans,
                                         int inputs_on_device, int *status)
{
    // refusals of the call as a whole: every status[k] carries the code, no handle is touched
    if (!hs || !rhs || !lhs || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (!rhs[k] || !lhs[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (const int st = batch_handles_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);
    const int tr = (trans == 't' || trans == 'T') ? 1 : 0;

    // per member: its kind, and what it needs before the launches
    std::vector<int> result(n, kPending);
    std::vector<int> fresh_build, fresh_plain, upd; // member indices
    for (int k = 0; k < n; k++) {
        blu_hip *h = hs[k];
        if (h->nupdate < 0) { // solve_dense.rs:25-27
            result[k] = BLU_ERROR_INVALID_CALL;
            continue;
        }
        if (h->m == 0) {
            result[k] = BLU_OK;
            continue;
        }
        const size_t M = (size_t)h->m;
        if (!inputs_on_device) { // staged through the handle's own buffers, as blu_hip_solve_dense does
            if (!h->d_rhs || !h->d_lhs) {
                dfree(h->d_rhs); dfree(h->d_lhs);
                if (!dalloc(h, &h->d_rhs, M) || !dalloc(h, &h->d_lhs, M)) {
                    result[k] = BLU_ERROR_OUT_OF_MEMORY;
                    continue;
                }
            }
        }
        int st = BLU_OK;
        std::vector<int> *kind = &fresh_plain;
        if (h->nupdate > 0) {
            kind = &upd;
            st = ensure_upd(h); // (a no-op once an update was made: it needed the same)
            if (st == BLU_OK) st = marker_room(h);
        } else if (!tr && h->lt_for_nfact != h->nfactorize) {
            kind = &fresh_build;
            st = ensure_lt_ws(h);
        }
        if (st == BLU_OK && !inputs_on_device && !hip_ok(h, hipMemcpy(h->d_rhs, rhs[k], M * 8, hipMemcpyHostToDevice), "h2d rhs"))
            st = BLU_ERROR_DEVICE;
        if (st == BLU_OK) kind->push_back(k);
        else result[k] = st;
    }

    // one staging buffer: descriptors of the fresh members (those that need the row-wise L first), then of the
    // updated ones; read-out descriptors of the fresh ones; SolveMember of all; SparseWs of the builds, then of the
    // updated members; UpdWs of the updated members
    std::vector<int> order(fresh_build);
    order.insert(order.end(), fresh_plain.begin(), fresh_plain.end());
    const int nb = (int)fresh_build.size(), nf = (int)order.size(), nu = (int)upd.size();
    order.insert(order.end(), upd.begin(), upd.end());
    const int na = nf + nu;
    if (na > 0) {
        Stage S;
        const auto aD = S.add<DevLU>((size_t)na);
        const auto aO = S.add<FinishOut>((size_t)nf);
        const auto aM = S.add<SolveMember>((size_t)na);
        const auto aW = S.add<SparseWs>((size_t)(nb + nu));
        const auto aU = S.add<UpdWs>((size_t)nu);
        S.host_front(S.bytes);
        DevLU *sD = S.h(aD);
        FinishOut *sO = S.h(aO);
        SolveMember *sM = S.h(aM);
        SparseWs *sW = S.h(aW);
        UpdWs *sU = S.h(aU);
        for (int s = 0; s < na; s++) {
            const int k = order[s];
            blu_hip *h = hs[k];
            sD[s] = h->D;
            if (s < nf) sO[s] = h->O;
            SolveMember &M = sM[s];
            M.rhs = inputs_on_device ? rhs[k] : h->d_rhs;
            M.lhs = inputs_on_device ? lhs[k] : h->d_lhs;
            M.lt_ptr = h->sw.lt_ptr;
            M.lt_idx = h->sw.lt_idx;
            M.lt_val = h->sw.lt_val;
            M.marker = h->marker;
            M.pad = 0;
            if (s < nb) sW[s] = h->sw;
            if (s >= nf) {
                sW[nb + (s - nf)] = h->sw;
                sU[s - nf] = h->uw;
            }
        }
        auto launch = [&](hipStream_t stream) {
            const DevLU *dD = S.d(aD);
            const SolveMember *dM = S.d(aM);
            const SparseWs *dW = S.d(aW);
            if (nb > 0) hipLaunchKernelGGL(k_build_lt_batch, dim3(nb), dim3(1024), 0, stream, dD, dW);
            if (nf > 0) hipLaunchKernelGGL(k_solve_dense_batch, dim3(nf), dim3(64), 0, stream, dD, S.d(aO), dM, tr);
            if (nu > 0) hipLaunchKernelGGL(k_solve_dense_upd_batch, dim3(nu), dim3(64), 0, stream, dD + nf, dW + nb, S.d(aU), dM + nf, tr);
        };
        if (const int st = stage_alloc(h0, S); st != BLU_OK) {
            for (int k : order) result[k] = st;
        } else if (stage_run(h0, S, "h2d solve descriptors", "k_solve_dense_batch", launch, [] { return true; }) != BLU_OK) {
            fail_members(h0, hs, order, result, BLU_ERROR_DEVICE);
        } else {
            for (int s = 0; s < na; s++) {
                const int k = order[s];
                blu_hip *h = hs[k];
                if (s < nb) h->lt_for_nfact = h->nfactorize;
                if (s >= nf) h->marker += 4;
                result[k] = BLU_OK;
                if (!inputs_on_device && !hip_ok(h, hipMemcpy(lhs[k], h->d_lhs, (size_t)h->m * 8, hipMemcpyDeviceToHost), "d2h lhs"))
                    result[k] = BLU_ERROR_DEVICE;
            }
        }
    }
    return batch_return(result, status);
}
