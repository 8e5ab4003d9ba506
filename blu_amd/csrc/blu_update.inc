// blu_update.inc -- host side of the update path (included by blu_hip.hip): the C ABI entries that mirror
//   solve_for_update   src/solve_for_update.rs:73-119 + BLU::solve_for_update  src/blu.rs:257-288
//   update             src/update.rs:49-55          + BLU::update            src/blu.rs:319-335
// and the dispatch of solve_dense / solve_sparse to the kernels that work on an updated factorization.
// As BLU does for Status::Reallocate (blu.rs:277-283, 324-330), storage requests of the kernels are answered
// here and the call is repeated; callers never see them.

static void free_upd(blu_hip *h)
{
    UpdWs &U = h->uw;
    dfree(U.st); dfree(U.pmap); dfree(U.qmap); dfree(U.col_pivot); dfree(U.row_pivot);
    dfree(U.wbeg); dfree(U.wlen); dfree(U.wcap); dfree(U.widx); dfree(U.wval);
    dfree(U.ucbeg); dfree(U.uclen); dfree(U.ucidx); dfree(U.ucval);
    dfree(U.rbeg); dfree(U.eta_row); dfree(U.ridx); dfree(U.rval);
    dfree(U.pvrow); dfree(U.pvcol); dfree(U.iw1); dfree(U.iw2); dfree(U.work1);
    h->upd_alloc_m = -1;
    h->upd_for_nfact = -1;
}

static bool download_upd(blu_hip *h)
{
    return hip_ok(h, hipMemcpy(&h->ust, h->uw.st, sizeof(UpdState), hipMemcpyDeviceToHost), "d2h update state");
}

// the fixed-size (m-dependent) arrays of the update workspace
static int ensure_upd_fixed(blu_hip *h)
{
    UpdWs &U = h->uw;
    const size_t M = (size_t)h->m;
    if (h->upd_alloc_m != h->m) {
        free_upd(h);
        bool a = dalloc(h, &U.st, 1) && dalloc(h, &U.pmap, M) && dalloc(h, &U.qmap, M) && dalloc(h, &U.col_pivot, M) &&
                 dalloc(h, &U.row_pivot, M) && dalloc(h, &U.wbeg, M) && dalloc(h, &U.wlen, M) && dalloc(h, &U.wcap, M) &&
                 dalloc(h, &U.ucbeg, M) && dalloc(h, &U.uclen, M) && dalloc(h, &U.rbeg, M + 2) && dalloc(h, &U.eta_row, M + 1) &&
                 dalloc(h, &U.pvrow, 2 * M + 2) && dalloc(h, &U.pvcol, 2 * M + 2) && dalloc(h, &U.iw1, M + 1) &&
                 dalloc(h, &U.iw2, M + 1) && dalloc(h, &U.work1, M + 1);
        if (!a) return BLU_ERROR_OUT_OF_MEMORY;
        U.wcapacity = U.uccapacity = U.rcapacity = 0;
        h->upd_alloc_m = h->m;
    }
    return BLU_OK;
}

// room for the mutable copies of U, the maps, the pivot sequence and the eta file of THIS factorization
static int ensure_upd_ws(blu_hip *h)
{
    UpdWs &U = h->uw;
    const size_t M = (size_t)h->m;
    {
        const int st = ensure_upd_fixed(h);
        if (st != BLU_OK) return st;
    }
    // arenas: what build_factors asks for (build_factors.rs:160-177) plus room for a few hundred updates
    const int64_t u_nz = h->hs.u_nz;
    const int64_t extra = h->upd_extra >= 0 ? h->upd_extra : 4 * std::max<int64_t>(h->b_nz_hint, (int64_t)M) + 1024;
    const int64_t wneed = std::min<int64_t>(u_nz + (int64_t)(h->stretch * (double)u_nz) + (int64_t)M * h->pad + extra, kIntMax);
    const int64_t ucneed = std::min<int64_t>(u_nz + (int64_t)M + 1 + extra, kIntMax);
    const int64_t rneed = std::min<int64_t>(extra, kIntMax);
    if (wneed > U.wcapacity) {
        dfree(U.widx); dfree(U.wval);
        if (!dalloc(h, &U.widx, (size_t)wneed) || !dalloc(h, &U.wval, (size_t)wneed)) return BLU_ERROR_OUT_OF_MEMORY;
        U.wcapacity = (int)wneed;
    }
    if (ucneed > U.uccapacity) {
        dfree(U.ucidx); dfree(U.ucval);
        if (!dalloc(h, &U.ucidx, (size_t)ucneed) || !dalloc(h, &U.ucval, (size_t)ucneed)) return BLU_ERROR_OUT_OF_MEMORY;
        U.uccapacity = (int)ucneed;
    }
    if (rneed > U.rcapacity) {
        dfree(U.ridx); dfree(U.rval);
        if (!dalloc(h, &U.ridx, (size_t)rneed) || !dalloc(h, &U.rval, (size_t)rneed)) return BLU_ERROR_OUT_OF_MEMORY;
        U.rcapacity = (int)rneed;
    }
    return BLU_OK;
}

// the mutable copies of U, the maps, the pivot sequence and the eta file of THIS factorization
static int ensure_upd(blu_hip *h)
{
    int st = ensure_lt(h); // sparse workspace + row-wise L
    if (st != BLU_OK) return st;
    if (h->upd_for_nfact == h->nfactorize) return BLU_OK;
    st = ensure_upd_ws(h);
    if (st != BLU_OK) return st;
    UpdWs &U = h->uw;
    // the totals count over the life of the handle: LU::reset leaves them (lu.rs:329-359), k_upd_init starts from zero
    const long long nsymperm_total = h->ust.nsymperm_total, nunsymperm_total = h->ust.nunsymperm_total, nforrest_total = h->ust.nforrest_total;
    hipLaunchKernelGGL(k_upd_init, dim3(1), dim3(1024), 0, h->stream, h->dD, h->dO, U);
    if (!hip_ok(h, hipStreamSynchronize(h->stream), "k_upd_init")) return BLU_ERROR_DEVICE;
    if (!download_upd(h)) return BLU_ERROR_DEVICE;
    h->ust.nsymperm_total = nsymperm_total;
    h->ust.nunsymperm_total = nunsymperm_total;
    h->ust.nforrest_total = nforrest_total;
    if (!hip_ok(h, hipMemcpy(U.st, &h->ust, sizeof(UpdState), hipMemcpyHostToDevice), "h2d update state")) return BLU_ERROR_DEVICE;
    h->upd_for_nfact = h->nfactorize;
    return BLU_OK;
}

// answer a storage request of the update kernels (the device counterpart of lu_realloc_obj, blu.rs:345-377)
static int grow_upd(blu_hip *h)
{
    h->upd_grows++;
    UpdWs &U = h->uw;
    const UpdState &s = h->ust;
    if (s.status == UPD_NEED_R) {
        const size_t keep = 0; // filled below
        (void)keep;
        std::vector<int> rb(1);
        if (!hip_ok(h, hipMemcpy(rb.data(), U.rbeg + s.nforrest, sizeof(int), hipMemcpyDeviceToHost), "d2h rbeg")) return BLU_ERROR_DEVICE;
        const int64_t n = grown(h, U.rcapacity, s.need);
        if (n <= U.rcapacity) return BLU_ERROR_OUT_OF_MEMORY;
        if (!dgrow(h, &U.ridx, (size_t)rb[0], (size_t)n) || !dgrow(h, &U.rval, (size_t)rb[0], (size_t)n)) return BLU_ERROR_OUT_OF_MEMORY;
        U.rcapacity = (int)n;
    } else if (s.status == UPD_NEED_UC) {
        const int64_t n = grown(h, U.uccapacity, s.need);
        if (n <= U.uccapacity) return BLU_ERROR_OUT_OF_MEMORY;
        if (!dgrow(h, &U.ucidx, (size_t)s.ucused, (size_t)n) || !dgrow(h, &U.ucval, (size_t)s.ucused, (size_t)n)) return BLU_ERROR_OUT_OF_MEMORY;
        U.uccapacity = (int)n;
    } else if (s.status == UPD_NEED_W) {
        const int64_t n = grown(h, U.wcapacity, s.need);
        if (n <= U.wcapacity) return BLU_ERROR_OUT_OF_MEMORY;
        // the pending spike sits behind ucused in the column arena: untouched by this
        if (!dgrow(h, &U.widx, (size_t)s.wused, (size_t)n) || !dgrow(h, &U.wval, (size_t)s.wused, (size_t)n)) return BLU_ERROR_OUT_OF_MEMORY;
        U.wcapacity = (int)n;
    } else {
        return BLU_ERROR_DEVICE;
    }
    return BLU_OK;
}

static int marker_room(blu_hip *h)
{
    if (h->marker > 0x7fffffff - 16) { // lu.rs:301-305: reset the marks before the marker overflows
        if (!hip_ok(h, hipMemset(h->sw.marked, 0, (size_t)h->m * sizeof(int)), "hipMemset")) return BLU_ERROR_DEVICE;
        h->marker = 0;
    }
    return BLU_OK;
}

static int upload_rhs(blu_hip *h, int64_t nzrhs, const uint64_t *irhs, const double *xrhs)
{
    if (nzrhs > h->rhs_cap) {
        dfree(h->d_irhs);
        dfree(h->d_xrhs);
        if (!dalloc(h, &h->d_irhs, (size_t)nzrhs) || !dalloc(h, &h->d_xrhs, (size_t)nzrhs)) return BLU_ERROR_OUT_OF_MEMORY;
        h->rhs_cap = nzrhs;
    }
    if (nzrhs > 0) {
        std::vector<int> ir((size_t)nzrhs);
        for (int64_t n = 0; n < nzrhs; n++) ir[(size_t)n] = (int)irhs[n];
        if (!hip_ok(h, hipMemcpy(h->d_irhs, ir.data(), (size_t)nzrhs * sizeof(int), hipMemcpyHostToDevice), "h2d irhs")) return BLU_ERROR_DEVICE;
        if (xrhs && !hip_ok(h, hipMemcpy(h->d_xrhs, xrhs, (size_t)nzrhs * sizeof(double), hipMemcpyHostToDevice), "h2d xrhs"))
            return BLU_ERROR_DEVICE;
    }
    return BLU_OK;
}

// compressed solution -> the caller's (all-zero) lhs, pattern in the reference's order
static int fetch_solution(blu_hip *h, int64_t *p_nzlhs, int64_t *ilhs, double *lhs)
{
    long long out[4];
    if (!hip_ok(h, hipMemcpy(out, h->sw.out, sizeof out, hipMemcpyDeviceToHost), "d2h out")) return BLU_ERROR_DEVICE;
    const size_t nz = (size_t)out[0];
    h->sp_l_flops += out[1];
    h->sp_u_flops += out[2];
    h->sp_branch = (int)out[3];
    if (p_nzlhs && ilhs && lhs) {
        if (nz > 0) {
            std::vector<int> il(nz);
            std::vector<double> xv(nz);
            if (!hip_ok(h, hipMemcpy(il.data(), h->sw.ilhs, nz * sizeof(int), hipMemcpyDeviceToHost), "d2h ilhs") ||
                !hip_ok(h, hipMemcpy(xv.data(), h->sw.xval, nz * sizeof(double), hipMemcpyDeviceToHost), "d2h xval"))
                return BLU_ERROR_DEVICE;
            for (size_t n = 0; n < nz; n++) {
                ilhs[n] = il[n];
                lhs[il[n]] = xv[n];
            }
        }
        *p_nzlhs = (int64_t)nz;
    }
    return BLU_OK;
}

// UPD_ERROR of `who` ("update": k_update; "update path": the solves on updated factors, where mode 1 may already have
// written an eta row or the spike): the factors may be half modified, so they are invalid from here on
static int upd_invariant_violated(blu_hip *h, const char *who)
{
    char buf[128];
    snprintf(buf, sizeof buf, "%s: invariant violated at kernel source line %d", who, h->ust.err_line);
    h->err = buf;
    h->nupdate = -1;
    return BLU_ERROR_DEVICE;
}

// one launch of k_solve_upd with the storage-request loop around it; the right-hand side is on the device already
// (h->d_irhs / h->d_xrhs after upload_rhs, or a column of the resident A of blu_hip_maxvolume)
static int run_solve_upd(blu_hip *h, int mode, int want, int64_t nzrhs, int tr, const int *d_irhs, const double *d_xrhs)
{
    const int nz_sparse = (int)(h->sparse_thres * (double)h->m);
    for (int attempt = 0; attempt < 64; attempt++) {
        int st = marker_room(h);
        if (st != BLU_OK) return st;
        hipLaunchKernelGGL(k_solve_upd, dim3(1), dim3(64), 0, h->stream, h->dD, h->sw, h->uw, mode, want, (int)nzrhs, d_irhs, d_xrhs, tr,
                           h->marker, nz_sparse);
        if (!hip_ok(h, hipStreamSynchronize(h->stream), "k_solve_upd")) return BLU_ERROR_DEVICE;
        h->marker += 4;
        if (!download_upd(h)) return BLU_ERROR_DEVICE;
        if (h->ust.status == UPD_OK) return BLU_OK;
        if (h->ust.status == UPD_ERROR) return upd_invariant_violated(h, "update path");
        st = grow_upd(h);
        if (st != BLU_OK) return st;
    }
    h->err = "update path: too many storage requests";
    return BLU_ERROR_DEVICE;
}

// solve_for_update -- src/solve_for_update.rs:73-119, BLU::solve_for_update src/blu.rs:257-288
extern "C" int blu_hip_solve_for_update(blu_hip *h, int64_t nzrhs, const uint64_t *irhs, const double *xrhs, int64_t *p_nzlhs,
                                        int64_t *ilhs, double *lhs, char trans)
{
    if (!h || !irhs) return BLU_ERROR_ARGUMENT_MISSING;
    const int tr = (trans == 't' || trans == 'T') ? 1 : 0;
    if (!tr && !xrhs) return BLU_ERROR_ARGUMENT_MISSING;        // solve_for_update.rs:83-84
    if (h->nupdate < 0) return BLU_ERROR_INVALID_CALL;           // :85-86
    if (h->m == 0) return BLU_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    int st = ensure_upd(h);
    if (st != BLU_OK) return st;
    if (h->ust.nforrest == h->m) return BLU_ERROR_MAXIMUM_UPDATES; // :87-88
    bool ok;
    if (tr) {
        ok = irhs[0] < (uint64_t)h->m;
    } else {
        ok = nzrhs >= 0 && nzrhs <= h->m;
        for (int64_t n = 0; ok && n < nzrhs; n++) ok = irhs[n] < (uint64_t)h->m;
    }
    if (!ok) return BLU_ERROR_INVALID_ARGUMENT;
    const int want = (p_nzlhs && ilhs && lhs) ? 1 : 0;
    if (want) *p_nzlhs = 0;
    st = upload_rhs(h, tr ? 1 : nzrhs, irhs, tr ? nullptr : xrhs);
    if (st != BLU_OK) return st;
    st = run_solve_upd(h, 1, want, tr ? 1 : nzrhs, tr, h->d_irhs, h->d_xrhs);
    if (st != BLU_OK) return st;
    return fetch_solution(h, p_nzlhs, ilhs, lhs);
}

// update -- src/update.rs:49-55, BLU::update src/blu.rs:319-335
extern "C" int blu_hip_update(blu_hip *h, double xtbl)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (h->nupdate < 0 || h->upd_for_nfact != h->nfactorize || h->ust.ftran_for < 0 || h->ust.btran_for < 0) return BLU_ERROR_INVALID_CALL;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    for (int attempt = 0; attempt < 64; attempt++) {
        int st = marker_room(h);
        if (st != BLU_OK) return st;
        hipLaunchKernelGGL(k_update, dim3(1), dim3(64), 0, h->stream, h->dD, h->sw, h->uw, xtbl, h->marker);
        if (!hip_ok(h, hipStreamSynchronize(h->stream), "k_update")) return BLU_ERROR_DEVICE;
        h->marker += 4;
        if (!download_upd(h)) return BLU_ERROR_DEVICE;
        if (h->ust.status == UPD_OK) {
            h->nupdate++;
            return BLU_OK;
        }
        if (h->ust.status == UPD_SINGULAR) return BLU_ERROR_SINGULAR_UPDATE; // the old factorization is still valid
        if (h->ust.status == UPD_ERROR) return upd_invariant_violated(h, "update");
        st = grow_upd(h);
        if (st != BLU_OK) return st;
    }
    h->err = "update: too many storage requests";
    return BLU_ERROR_DEVICE;
}

// solve_sparse / solve_dense after at least one update
static int solve_sparse_updated(blu_hip *h, int64_t nzrhs, const uint64_t *irhs, const double *xrhs, int64_t *p_nzlhs, int64_t *ilhs,
                                double *lhs, int tr)
{
    int st = ensure_upd(h);
    if (st != BLU_OK) return st;
    st = upload_rhs(h, nzrhs, irhs, xrhs);
    if (st != BLU_OK) return st;
    st = run_solve_upd(h, 0, 1, nzrhs, tr, h->d_irhs, h->d_xrhs);
    if (st != BLU_OK) return st;
    return fetch_solution(h, p_nzlhs, ilhs, lhs);
}
static int solve_dense_updated(blu_hip *h, int tr)
{
    int st = ensure_upd(h);
    if (st != BLU_OK) return st;
    st = marker_room(h);
    if (st != BLU_OK) return st;
    hipLaunchKernelGGL(k_solve_dense_upd, dim3(1), dim3(64), 0, h->stream, h->dD, h->sw, h->uw, h->d_rhs, h->d_lhs, tr, h->marker);
    if (!hip_ok(h, hipStreamSynchronize(h->stream), "k_solve_dense_upd")) return BLU_ERROR_DEVICE;
    h->marker += 4;
    return BLU_OK;
}

// debug / test hook: room (entries) the arenas of the update path get beyond what the fresh factors need;
// small values force the storage-request loop (default -1: 4*max(b_nz, m) + 1024)
extern "C" int blu_hip_dbg_set_upd_extra(blu_hip *h, int64_t extra)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    h->upd_extra = extra;
    h->upd_for_nfact = -1;
    return BLU_OK;
}
// storage requests of the update kernels this handle has answered so far (tests: the knob above did force some)
extern "C" int64_t blu_hip_dbg_upd_grows(const blu_hip *h) { return h ? h->upd_grows : 0; }
