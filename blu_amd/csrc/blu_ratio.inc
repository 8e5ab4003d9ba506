// blu_ratio.inc -- the dual ratio test on the device (included by blu_hip.hip behind blu_matrix.inc): the reduced costs d
// and the bound status kind of the columns of the resident matrix stay on the device, with the row of the last ratio test.
//   blu_hip_set_duals / _get_duals / _get_ratio_row   upload and download of the state
//   blu_hip_ratio_test          the solve of blu_hip_tableau_row (mx_row_solve), then clear y, k_scatter_lhs, k_at_dot_kind
//                               straight into the kept row, k_ratio_pick, one synchronize, 64 bytes down
//   blu_hip_update_duals        k_duals_axpy from the kept row, then the overrides (one upload, k_duals_set)
//   blu_hip_copy_duals_batch    d and kind of one handle into many: k_duals_fanout
//   blu_hip_ratio_test_batch    the batched solves of blu_hip_tableau_row_batch (mx_batch_row_solves), then per chunk the tiles
//                               and k_at_dot_batch with masks from the host mirrors of kind, and k_ratio_pick_batch
//                               (mx_batch_products with an MxRatio, blu_matrix_batch.inc)
//   blu_hip_update_duals_batch  one packed upload of the steps and the overrides, k_duals_axpy_batch, k_duals_set_batch
// The state is the handle's own: 17 ncol device bytes, a 64-byte record, the overrides of the last step, and a host mirror
// of kind, which is exact because every change of kind comes from the host.  du_drop is how it goes: blu_hip_set_matrix,
// a destination of blu_hip_share_matrix, blu_hip_maxvolume, blu_hip_free.

static_assert(sizeof(RatioRec) == sizeof(blu_ratio_result) && sizeof(blu_ratio_result) == 64, "the record of the pick is blu_ratio_result");

static void du_drop(blu_hip *h)
{
    dfree(h->du_d); dfree(h->du_row); dfree(h->du_kind); dfree(h->du_rec); dfree(h->du_sets);
    h->du_cap = h->du_setcap = 0;
    h->du_set = h->du_row_valid = false;
    std::vector<signed char>().swap(h->du_hkind);
}

static bool kind_ok(int k) { return k == 0 || k == 1 || k == -1 || k == 2; }

// the buffers for the handle's matrix; a kept row does not survive a new allocation
static int du_buffers(blu_hip *h)
{
    const size_t N = (size_t)h->mx_ncol;
    if (h->du_d && (int64_t)N <= h->du_cap) return BLU_OK;
    dfree(h->du_d); dfree(h->du_row); dfree(h->du_kind); dfree(h->du_rec);
    h->du_cap = 0;
    h->du_row_valid = false;
    if (!dalloc(h, &h->du_d, N) || !dalloc(h, &h->du_row, N) || !dalloc(h, &h->du_kind, N) || !dalloc(h, &h->du_rec, 1)) {
        (void)hipGetLastError();
        du_drop(h);
        return BLU_ERROR_OUT_OF_MEMORY;
    }
    h->du_cap = (int64_t)N;
    return BLU_OK;
}

extern "C" int blu_hip_set_duals(blu_hip *h, const double *d, const int8_t *kind)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->mx_set) return BLU_ERROR_INVALID_CALL;
    const size_t N = (size_t)h->mx_ncol;
    if (!h->du_set && N > 0 && (!d || !kind)) return BLU_ERROR_ARGUMENT_MISSING;
    for (size_t j = 0; kind && j < N; j++)
        if (!kind_ok(kind[j])) return BLU_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    const int st = du_buffers(h);
    if (st != BLU_OK) return st;
    if (N && d && !hip_ok(h, hipMemcpy(h->du_d, d, N * 8, hipMemcpyHostToDevice), "h2d duals")) return BLU_ERROR_DEVICE;
    if (N && kind) {
        if (!hip_ok(h, hipMemcpy(h->du_kind, kind, N, hipMemcpyHostToDevice), "h2d kind")) {
            h->du_set = false; // (the mirror no longer tells what the device holds)
            return BLU_ERROR_DEVICE;
        }
        h->du_hkind.assign((const signed char *)kind, (const signed char *)kind + N);
    }
    h->du_set = true;
    return BLU_OK;
}

extern "C" int blu_hip_get_duals(blu_hip *h, double *d, int8_t *kind)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->du_set) return BLU_ERROR_INVALID_CALL;
    const size_t N = (size_t)h->mx_ncol;
    if (N == 0) return BLU_OK;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    if (d && !hip_ok(h, hipMemcpy(d, h->du_d, N * 8, hipMemcpyDeviceToHost), "d2h duals")) return BLU_ERROR_DEVICE;
    if (kind && !hip_ok(h, hipMemcpy(kind, h->du_kind, N, hipMemcpyDeviceToHost), "d2h kind")) return BLU_ERROR_DEVICE;
    return BLU_OK;
}

extern "C" int blu_hip_get_ratio_row(blu_hip *h, double *alpha)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->du_set || !h->du_row_valid) return BLU_ERROR_INVALID_CALL;
    const size_t N = (size_t)h->mx_ncol;
    if (N == 0) return BLU_OK;
    if (!alpha) return BLU_ERROR_ARGUMENT_MISSING;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    return hip_ok(h, hipMemcpy(alpha, h->du_row, N * 8, hipMemcpyDeviceToHost), "d2h kept row") ? BLU_OK : BLU_ERROR_DEVICE;
}

static bool ratio_tols_ok(double pivtol, double dualtol) { return std::isfinite(pivtol) && std::isfinite(dualtol) && pivtol >= 0.0 && dualtol >= 0.0; }
static blu_ratio_result ratio_none()
{
    blu_ratio_result R;
    memset(&R, 0, sizeof R);
    R.q = -1;
    return R;
}

extern "C" int blu_hip_ratio_test(blu_hip *h, int64_t r, int prepare_update, double sigma, double pivtol, double dualtol, blu_ratio_result *out,
                                  int64_t *p_nzlhs, int64_t *ilhs, double *lhs)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->mx_set) return BLU_ERROR_INVALID_CALL;
    if (!h->du_set) return BLU_ERROR_INVALID_CALL;
    if (!out) return BLU_ERROR_ARGUMENT_MISSING;
    if (!(sigma == 1.0 || sigma == -1.0) || !ratio_tols_ok(pivtol, dualtol)) return BLU_ERROR_INVALID_ARGUMENT;
    const int st = mx_row_solve(h, r, prepare_update, p_nzlhs, ilhs, lhs);
    if (st != BLU_OK) return st;
    // step two: the row into the kept-row buffer and the pick on it, all on the device
    memset(h->mx_counts, 0, sizeof h->mx_counts);
    h->du_row_valid = false;
    const size_t N = (size_t)h->mx_ncol;
    if (N == 0) {
        *out = ratio_none();
        h->du_row_valid = true;
        return BLU_OK;
    }
    hipStream_t stream = h->stream;
    if (!hip_ok(h, hipMemsetAsync(h->mx_y, 0, (size_t)h->m * 8, stream), "hipMemset")) return BLU_ERROR_DEVICE;
    mx_scatter(h);
    const MatA A{h->mv_ap, h->mv_ai, h->mv_ax};
    const unsigned waves = (unsigned)((N + 63) / 64), per = ATD_THREADS / 64;
    hipLaunchKernelGGL(k_at_dot_kind, dim3((waves + per - 1) / per), dim3(ATD_THREADS), 0, stream, A, h->mx_y, h->du_kind, (int)N, h->du_row);
    h->mx_counts[0]++;
    if (h->mx_timing) (void)hipEventRecord(h->ev[0], stream);
    hipLaunchKernelGGL(k_ratio_pick, dim3(1), dim3(PICK_THREADS), 0, stream, h->du_row, h->du_d, h->du_kind, (int)N, sigma, pivtol, dualtol,
                       h->du_rec);
    h->mx_counts[0]++;
    if (h->mx_timing) (void)hipEventRecord(h->ev[1], stream);
    const bool ok = hip_ok(h, hipStreamSynchronize(stream), "k_ratio_pick");
    h->mx_counts[1]++;
    if (h->mx_timing && ok) { // (debug: here the events bracket the pick)
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess) h->mx_kernel_s = 1e-3 * (double)ms;
    }
    if (!ok || !hip_ok(h, hipMemcpy(out, h->du_rec, sizeof *out, hipMemcpyDeviceToHost), "d2h record")) return BLU_ERROR_DEVICE;
    h->mx_counts[3] += (int64_t)sizeof *out;
    h->du_row_valid = true;
    return BLU_OK;
}

// the checks of one dual step behind the handle's own: BLU_OK = go on
static int du_step_refusal(const blu_hip *h, int64_t nset, const int64_t *jset, const double *dset, const int8_t *kset)
{
    if (nset > 0 && (!jset || !dset || !kset)) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->du_set || !h->du_row_valid) return BLU_ERROR_INVALID_CALL;
    if (nset < 0) return BLU_ERROR_INVALID_ARGUMENT;
    std::vector<int64_t> js(jset, jset + (nset > 0 ? nset : 0));
    std::sort(js.begin(), js.end());
    if (std::adjacent_find(js.begin(), js.end()) != js.end()) return BLU_ERROR_INVALID_ARGUMENT;
    if (nset > 0 && (js.front() < 0 || js.back() >= h->mx_ncol)) return BLU_ERROR_INVALID_ARGUMENT;
    for (int64_t t = 0; t < nset; t++)
        if (!kind_ok(kset[t])) return BLU_ERROR_INVALID_ARGUMENT;
    return BLU_OK;
}
// workgroups of an elementwise kernel over ncol columns
static unsigned du_blocks(size_t N) { return (unsigned)std::min<size_t>(std::max<size_t>((N + DUALS_THREADS - 1) / DUALS_THREADS, 1), 256); }

extern "C" int blu_hip_update_duals(blu_hip *h, double theta, int64_t nset, const int64_t *jset, const double *dset, const int8_t *kset)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (const int st = du_step_refusal(h, nset, jset, dset, kset); st != BLU_OK) return st;
    const size_t N = (size_t)h->mx_ncol;
    if (N == 0) return BLU_OK;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    if (nset > h->du_setcap) {
        dfree(h->du_sets);
        h->du_setcap = 0;
        if (!dalloc(h, &h->du_sets, (size_t)nset)) {
            (void)hipGetLastError();
            return BLU_ERROR_OUT_OF_MEMORY;
        }
        h->du_setcap = nset;
    }
    hipStream_t stream = h->stream;
    std::vector<DualSet> sets((size_t)nset);
    for (int64_t t = 0; t < nset; t++) sets[(size_t)t] = DualSet{dset[t], (int)jset[t], (int)kset[t]};
    hipLaunchKernelGGL(k_duals_axpy, dim3(du_blocks(N)), dim3(DUALS_THREADS), 0, stream, h->du_d, h->du_row, h->du_kind, theta, (int)N);
    bool ok = true;
    if (nset > 0) {
        ok = hip_ok(h, hipMemcpyAsync(h->du_sets, sets.data(), sets.size() * sizeof(DualSet), hipMemcpyHostToDevice, stream), "h2d overrides");
        if (ok) hipLaunchKernelGGL(k_duals_set, dim3(1), dim3(DUALS_THREADS), 0, stream, h->du_d, h->du_kind, h->du_sets, (int)nset, (int)N);
    }
    ok = hip_ok(h, hipStreamSynchronize(stream), "k_duals_axpy") && ok;
    if (!ok) {
        du_drop(h); // (d is in no known state)
        return BLU_ERROR_DEVICE;
    }
    for (int64_t t = 0; t < nset; t++) h->du_hkind[(size_t)jset[t]] = (signed char)kset[t];
    return BLU_OK;
}

extern "C" int blu_hip_copy_duals_batch(blu_hip *src, blu_hip **dst, int n, int *status)
{
    // refusals of the call as a whole, as blu_hip_share_matrix: every status[k] carries the code, nothing is touched
    if (!src || !dst || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    for (int k = 0; k < n; k++)
        if (!dst[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (!src->mx_set || !src->du_set) return refuse_all(status, n, BLU_ERROR_INVALID_CALL);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (dst[k] == src || dst[k]->device != src->device || dst[k]->m != src->m) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT);
    if (has_duplicate(std::vector<blu_hip *>(dst, dst + n))) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT);
    if (hipSetDevice(src->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);

    const size_t N = (size_t)src->mx_ncol;
    std::vector<int> result(n, kPending), live;
    for (int k = 0; k < n; k++) {
        blu_hip *h = dst[k];
        if (!h->mx_set || h->mv_ap != src->mv_ap) result[k] = BLU_ERROR_INVALID_CALL;
        else if (const int st = du_buffers(h); st != BLU_OK) result[k] = st;
        else live.push_back(k);
    }
    if (N > 0 && !live.empty()) {
        Stage S;
        const StageArr<DualDst> a = S.add<DualDst>(live.size());
        S.host_front(S.bytes);
        for (size_t s = 0; s < live.size(); s++) S.h(a)[s] = DualDst{dst[live[s]]->du_d, dst[live[s]]->du_kind};
        int st = stage_alloc(src, S);
        if (st == BLU_OK) {
            const unsigned nbx = du_blocks(N);
            st = stage_run(src, S, "h2d destinations", "k_duals_fanout",
                           [&](hipStream_t stream) {
                               hipLaunchKernelGGL(k_duals_fanout, dim3(nbx * (unsigned)live.size()), dim3(DUALS_THREADS), 0, stream, src->du_d,
                                                  src->du_kind, S.d(a), (int)N, (int)nbx);
                           },
                           [] { return true; });
        }
        if (st != BLU_OK) {
            for (int k : live) du_drop(dst[k]);
            fail_members(src, dst, live, result, st);
            live.clear();
        }
    }
    for (int k : live) {
        dst[k]->du_hkind = src->du_hkind;
        dst[k]->du_set = true;
        result[k] = BLU_OK;
    }
    return batch_return(result, status);
}

extern "C" int blu_hip_ratio_test_batch(blu_hip **hs, int n, const int64_t *r, int prepare_update, const double *sigma, double pivtol,
                                        double dualtol, blu_ratio_result *out, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs,
                                        int *status)
{
    // refusals of the call as a whole, as blu_hip_tableau_row_batch: every status[k] carries the code, no handle is touched
    if (!hs || !r || !sigma || !out || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (!hs[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (const int st = mx_batch_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    if (!ratio_tols_ok(pivtol, dualtol)) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT);
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);

    // per member, in the order of blu_hip_ratio_test: the matrix, the duals, sigma, then the refusals of its solve
    std::vector<int> result(n, kPending);
    for (int k = 0; k < n; k++) {
        if (!hs[k]->mx_set || !hs[k]->du_set) result[k] = BLU_ERROR_INVALID_CALL;
        else if (!(sigma[k] == 1.0 || sigma[k] == -1.0)) result[k] = BLU_ERROR_INVALID_ARGUMENT;
    }
    mx_batch_row_solves(h0, hs, n, r, prepare_update, nzlhs, ilhs, lhs, result);

    // step two for the members whose solve ended well
    memset(h0->mx_counts, 0, sizeof h0->mx_counts);
    std::vector<int> live;
    for (int k = 0; k < n; k++)
        if (result[k] == BLU_OK) {
            live.push_back(k);
            hs[k]->du_row_valid = false;
        }
    if (!live.empty() && hs[live[0]]->mx_ncol == 0)
        for (int k : live) {
            out[k] = ratio_none();
            hs[k]->du_row_valid = true;
        }
    const MxRatio rt{sigma, pivtol, dualtol, out};
    mx_batch_products(h0, hs, live, nullptr, nullptr, nullptr, result, &rt);
    return batch_return(result, status);
}

extern "C" int blu_hip_update_duals_batch(blu_hip **hs, int n, const double *theta, const int64_t *nset, const int64_t *const *jset,
                                          const double *const *dset, const int8_t *const *kset, int *status)
{
    if (!hs || !theta || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (!hs[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (const int st = mx_batch_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);

    std::vector<int> result(n, kPending), live;
    std::vector<int64_t> ns((size_t)n, 0);
    size_t total = 0;
    for (int k = 0; k < n; k++) {
        ns[(size_t)k] = nset ? nset[k] : 0;
        const bool have = ns[(size_t)k] > 0 && jset && dset && kset;
        result[k] = du_step_refusal(hs[k], ns[(size_t)k], have ? jset[k] : nullptr, have ? dset[k] : nullptr, have ? kset[k] : nullptr);
        if (result[k] != BLU_OK) continue;
        if (hs[k]->mx_ncol == 0) continue; // (nothing to step)
        result[k] = kPending;
        live.push_back(k);
        total += (size_t)ns[(size_t)k];
    }
    if (live.empty()) return batch_return(result, status);
    const size_t N = (size_t)hs[live[0]]->mx_ncol;
    Stage S;
    const StageArr<DualStep> a_step = S.add<DualStep>(live.size());
    const StageArr<DualSet> a_set = S.add<DualSet>(std::max<size_t>(total, 1));
    S.host_front(S.bytes);
    size_t at = 0;
    for (size_t s = 0; s < live.size(); s++) {
        const int k = live[s];
        blu_hip *h = hs[k];
        S.h(a_step)[s] = DualStep{h->du_d, h->du_kind, h->du_row, theta[k], (long long)at, (int)ns[(size_t)k]};
        for (int64_t t = 0; t < ns[(size_t)k]; t++) S.h(a_set)[at++] = DualSet{dset[k][t], (int)jset[k][t], (int)kset[k][t]};
    }
    int st = stage_alloc(h0, S);
    if (st == BLU_OK) {
        const unsigned nbx = du_blocks(N);
        st = stage_run(h0, S, "h2d dual steps", "k_duals_axpy_batch",
                       [&](hipStream_t stream) {
                           hipLaunchKernelGGL(k_duals_axpy_batch, dim3(nbx * (unsigned)live.size()), dim3(DUALS_THREADS), 0, stream, S.d(a_step),
                                              (int)N, (int)nbx);
                           if (total > 0)
                               hipLaunchKernelGGL(k_duals_set_batch, dim3((unsigned)live.size()), dim3(DUALS_THREADS), 0, stream, S.d(a_step),
                                                  S.d(a_set), (int)N);
                       },
                       [] { return true; });
    }
    if (st != BLU_OK) {
        if (st == BLU_ERROR_DEVICE)
            for (int k : live) du_drop(hs[k]); // (d is in no known state)
        fail_members(h0, hs, live, result, st);
        return batch_return(result, status);
    }
    for (int k : live) {
        for (int64_t t = 0; t < ns[(size_t)k]; t++) hs[k]->du_hkind[(size_t)jset[k][t]] = (signed char)kset[k][t];
        result[k] = BLU_OK;
    }
    return batch_return(result, status);
}
