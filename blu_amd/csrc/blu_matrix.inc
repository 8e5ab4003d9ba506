// blu_matrix.inc -- the resident constraint matrix (included by blu_hip.hip): the rectangular A of a simplex code kept on
// the device with a public lifetime, and the products of an iteration with it.
//   blu_hip_set_matrix                uploads A into the buffers of blu_hip_maxvolume (mv_upload) after validating it;
//                                     every row index is below m from then on, which k_at_dot relies on
//   blu_hip_share_matrix              the matrix of one handle held by many: the arrays of A and the host offsets move into a
//                                     reference-counted block (MatShare) that the holders' mv_* / mx_hp fields alias; mx_detach
//                                     (blu_maxvolume.inc) is how a holder leaves.  The batched products: blu_matrix_batch.inc
//   blu_hip_factorize_columns         blu_hip_factorize of A[:, basis] with an m-sized upload (mv_factorize)
//   blu_hip_solve_for_update_column   the forward blu_hip_solve_for_update of column j, nothing uploaded
//   blu_hip_tableau_row               row r of B^-1 A: the transposed solve of e_r as its single entry makes it, then on the
//                                     device clear y, k_scatter_lhs, k_at_dot, and one download of ncol doubles
//   blu_hip_price                     z = A' y for a dense host y: one upload, k_at_dot, one download
// blu_hip_maxvolume overwrites the same buffers with a matrix nobody validated and clears the set flag.

static void free_matrix(blu_hip *h)
{
    dfree(h->mx_y); dfree(h->mx_out); dfree(h->mx_skip);
    h->mx_ycap = h->mx_colcap = 0;
    h->mx_set = false;
    du_drop(h);
}

// what a handle with a matrix of ncol columns has besides A: y (m doubles), the products and the skip bytes (ncol each)
static int mx_work_buffers(blu_hip *h, int64_t ncol)
{
    const size_t M = (size_t)h->m, N = (size_t)ncol;
    if ((int64_t)M > h->mx_ycap) {
        dfree(h->mx_y);
        h->mx_ycap = 0;
        if (!dalloc(h, &h->mx_y, M)) return BLU_ERROR_OUT_OF_MEMORY;
        h->mx_ycap = (int64_t)M;
    }
    if ((int64_t)N > h->mx_colcap) {
        dfree(h->mx_out); dfree(h->mx_skip);
        h->mx_colcap = 0;
        if (!dalloc(h, &h->mx_out, N) || !dalloc(h, &h->mx_skip, N)) return BLU_ERROR_OUT_OF_MEMORY;
        h->mx_colcap = (int64_t)N;
    }
    return BLU_OK;
}

extern "C" int blu_hip_set_matrix(blu_hip *h, int64_t ncol, const uint64_t *a_p, const uint64_t *a_i, const double *a_x)
{
    // refusals before anything is touched: the previous matrix stays
    if (!h || !a_p) return BLU_ERROR_ARGUMENT_MISSING;
    if (ncol < 0 || ncol > kIntMax) return BLU_ERROR_INVALID_ARGUMENT;
    for (int64_t j = 0; j < ncol; j++)
        if (a_p[j + 1] < a_p[j]) return BLU_ERROR_INVALID_ARGUMENT;
    const uint64_t base = a_p[0], nz = a_p[ncol] - base;
    if (nz > (uint64_t)kIntMax) return BLU_ERROR_INVALID_ARGUMENT; // (32-bit device indices)
    if (nz > 0 && (!a_i || !a_x)) return BLU_ERROR_ARGUMENT_MISSING;
    for (uint64_t q = 0; q < nz; q++)
        if (a_i[base + q] >= (uint64_t)h->m) return BLU_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    h->mx_set = false; // (from here on the buffers change)
    du_drop(h);
    const size_t N = (size_t)ncol;
    int st = mx_work_buffers(h, ncol);
    if (st != BLU_OK) return st;
    st = mv_upload(h, ncol, a_p, a_i, a_x);
    if (st != BLU_OK) return st;
    h->mx_hp_own.resize(N + 1);
    for (size_t j = 0; j <= N; j++) h->mx_hp_own[j] = a_p[j] - base;
    h->mx_hp = h->mx_hp_own.data();
    h->mx_ncol = ncol;
    h->mx_set = true;
    return BLU_OK;
}

// the block that owns h's set matrix; a handle that owns its arrays itself hands them over and becomes the first holder
static MatShare *mx_share_block(blu_hip *h)
{
    if (h->mx_share) return h->mx_share;
    MatShare *S = new MatShare();
    S->refs = 1;
    S->ap = h->mv_ap;
    S->ai64 = h->mv_ai64;
    S->ai = h->mv_ai;
    S->ax = h->mv_ax;
    S->hp = std::move(h->mx_hp_own);
    S->bt = nullptr;
    S->bt_cap = 0;
    S->bt_limit = -1;
    S->rt = nullptr;
    S->rt_cap = 0;
    h->mx_hp = S->hp.data();
    h->mx_share = S;
    return S;
}

// Every dst[k] holds the matrix src holds afterwards: no device copy of A and no launch.  A destination lets go of the
// matrix it has (its own arrays are freed, a shared one is detached), gets y / products / skip bytes of its own, and
// aliases the block.
extern "C" int blu_hip_share_matrix(blu_hip *src, blu_hip **dst, int n, int *status)
{
    // refusals of the call as a whole: every status[k] carries the code, nothing is touched
    if (!src || !dst || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    for (int k = 0; k < n; k++)
        if (!dst[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (!src->mx_set) return refuse_all(status, n, BLU_ERROR_INVALID_CALL);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (dst[k] == src || dst[k]->device != src->device || dst[k]->m != src->m) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT);
    if (has_duplicate(std::vector<blu_hip *>(dst, dst + n))) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT);
    if (hipSetDevice(src->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);

    MatShare *S = mx_share_block(src);
    std::vector<int> result(n, kPending);
    for (int k = 0; k < n; k++) {
        blu_hip *h = dst[k];
        du_drop(h); // (the resident duals of a destination go, blu_ratio.inc)
        if (h->mx_share == S && h->mx_set) { // (holds it already)
            result[k] = BLU_OK;
            continue;
        }
        h->mx_set = false;
        mx_detach(h);
        dfree(h->mv_ap); dfree(h->mv_ai64); dfree(h->mv_ai); dfree(h->mv_ax);
        h->mv_pcap = h->mv_nzcap = 0;
        std::vector<uint64_t>().swap(h->mx_hp_own);
        h->mx_hp = nullptr;
        result[k] = mx_work_buffers(h, src->mx_ncol);
        if (result[k] != BLU_OK) continue; // (left without a matrix)
        S->refs++;
        h->mx_share = S;
        h->mv_ap = S->ap;
        h->mv_ai64 = S->ai64;
        h->mv_ai = S->ai;
        h->mv_ax = S->ax;
        h->mx_hp = S->hp.data();
        h->mx_ncol = src->mx_ncol;
        h->mx_set = true;
    }
    return batch_return(result, status);
}

// handles that hold h's matrix, h included; 0 when none is set
extern "C" int blu_hip_dbg_matrix_holders(const blu_hip *h)
{
    if (!h || !h->mx_set) return 0;
    return h->mx_share ? h->mx_share->refs : 1;
}
// what tells one resident matrix from another (the device pointer of its offsets); NULL when none is set
extern "C" const void *blu_hip_dbg_matrix_id(const blu_hip *h) { return h && h->mx_set ? (const void *)h->mv_ap : nullptr; }

extern "C" int blu_hip_factorize_columns(blu_hip *h, const int64_t *basis)
{
    if (!h || !basis) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->mx_set) return BLU_ERROR_INVALID_CALL;
    for (int64_t i = 0; i < h->m; i++)
        if (basis[i] < 0 || basis[i] >= h->mx_ncol) return BLU_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    return mv_factorize(h, h->mx_hp, basis, h->mx_hp[(size_t)h->mx_ncol]);
}

// the checks of the forward blu_hip_solve_for_update in their order (blu_update.inc), the column taken from the resident A
extern "C" int blu_hip_solve_for_update_column(blu_hip *h, int64_t j, int64_t *p_nzlhs, int64_t *ilhs, double *lhs)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->mx_set) return BLU_ERROR_INVALID_CALL;
    if (h->nupdate < 0) return BLU_ERROR_INVALID_CALL;
    if (h->m == 0) return BLU_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    int st = ensure_upd(h);
    if (st != BLU_OK) return st;
    if (h->ust.nforrest == h->m) return BLU_ERROR_MAXIMUM_UPDATES;
    if (j < 0 || j >= h->mx_ncol) return BLU_ERROR_INVALID_ARGUMENT;
    const uint64_t off = h->mx_hp[(size_t)j], n = h->mx_hp[(size_t)j + 1] - off;
    if (n > (uint64_t)h->m) return BLU_ERROR_INVALID_ARGUMENT; // (its indices are below m: blu_hip_set_matrix)
    const int want = (p_nzlhs && ilhs && lhs) ? 1 : 0;
    if (want) *p_nzlhs = 0;
    st = run_solve_upd(h, 1, want, (int64_t)n, 0, h->mv_ai + off, h->mv_ax + off);
    if (st != BLU_OK) return st;
    return fetch_solution(h, p_nzlhs, ilhs, lhs);
}

// skip[0..ncol) as bytes into the handle's buffer; counts the copy
static int mx_upload_skip(blu_hip *h, const int64_t *skip)
{
    const size_t N = (size_t)h->mx_ncol;
    std::vector<unsigned char> sk(N);
    for (size_t j = 0; j < N; j++) sk[j] = skip[j] != 0;
    if (!hip_ok(h, hipMemcpy(h->mx_skip, sk.data(), N, hipMemcpyHostToDevice), "h2d skip")) return BLU_ERROR_DEVICE;
    h->mx_counts[2]++;
    return BLU_OK;
}

// out[j] = A[:, j] . mx_y for every column, then the one synchronize and the one download of the call
static int mx_product(blu_hip *h, const int64_t *skip, double *out)
{
    const size_t N = (size_t)h->mx_ncol;
    const MatA A{h->mv_ap, h->mv_ai, h->mv_ax};
    const unsigned waves = (unsigned)((N + 63) / 64), per = ATD_THREADS / 64;
    if (h->mx_timing) (void)hipEventRecord(h->ev[0], h->stream);
    hipLaunchKernelGGL(k_at_dot, dim3((waves + per - 1) / per), dim3(ATD_THREADS), 0, h->stream, A, h->mx_y, skip ? h->mx_skip : nullptr,
                       (int)N, h->mx_out);
    h->mx_counts[0]++;
    if (h->mx_timing) (void)hipEventRecord(h->ev[1], h->stream);
    const bool ok = hip_ok(h, hipStreamSynchronize(h->stream), "k_at_dot");
    h->mx_counts[1]++;
    if (h->mx_timing && ok) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess) h->mx_kernel_s = 1e-3 * (double)ms;
    }
    if (!ok || !hip_ok(h, hipMemcpy(out, h->mx_out, N * 8, hipMemcpyDeviceToHost), "d2h products")) return BLU_ERROR_DEVICE;
    h->mx_counts[3] += (int64_t)(N * 8);
    return BLU_OK;
}

// step one of blu_hip_tableau_row and blu_hip_ratio_test (blu_ratio.inc): the transposed solve of e_r, as the single entry
// makes it; the solution is downloaded only if asked for
static int mx_row_solve(blu_hip *h, int64_t r, int prepare_update, int64_t *p_nzlhs, int64_t *ilhs, double *lhs)
{
    const bool fetch = p_nzlhs && ilhs && lhs;
    const uint64_t ir = (uint64_t)r;
    int st;
    if (prepare_update) { // blu_hip_solve_for_update(h, ., [r], ., 'T') with a solution
        if (h->nupdate < 0) return BLU_ERROR_INVALID_CALL;
        if (h->m == 0) return BLU_ERROR_INVALID_ARGUMENT;
        if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
        st = ensure_upd(h);
        if (st != BLU_OK) return st;
        if (h->ust.nforrest == h->m) return BLU_ERROR_MAXIMUM_UPDATES;
        if (ir >= (uint64_t)h->m) return BLU_ERROR_INVALID_ARGUMENT;
        if (fetch) *p_nzlhs = 0;
        st = upload_rhs(h, 1, &ir, nullptr);
        if (st == BLU_OK) st = run_solve_upd(h, 1, 1, 1, 1, h->d_irhs, h->d_xrhs);
        if (st == BLU_OK) st = fetch_solution(h, fetch ? p_nzlhs : nullptr, ilhs, lhs);
    } else { // blu_hip_solve_sparse(h, 1, [r], [1.0], ..., 'T')
        if (h->nupdate < 0) return BLU_ERROR_INVALID_CALL;
        if (ir >= (uint64_t)h->m) return BLU_ERROR_INVALID_ARGUMENT;
        const double one = 1.0;
        st = solve_sparse_core(h, 1, &ir, &one, fetch ? p_nzlhs : nullptr, ilhs, lhs, 1);
    }
    return st;
}

// the launch of k_scatter_lhs over the solution the solve left on the device, into the cleared mx_y; counts itself
static void mx_scatter(blu_hip *h)
{
    const size_t M = (size_t)h->m;
    hipLaunchKernelGGL(k_scatter_lhs, dim3((unsigned)std::min<size_t>((M + 255) / 256, 64)), dim3(256), 0, h->stream, h->sw.out, h->sw.ilhs,
                       h->sw.xval, (int)M, h->mx_y);
    h->mx_counts[0]++;
}

extern "C" int blu_hip_tableau_row(blu_hip *h, int64_t r, int prepare_update, const int64_t *skip, double *alpha, int64_t *p_nzlhs,
                                   int64_t *ilhs, double *lhs)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->mx_set) return BLU_ERROR_INVALID_CALL;
    if (h->mx_ncol > 0 && !alpha) return BLU_ERROR_ARGUMENT_MISSING;
    int st = mx_row_solve(h, r, prepare_update, p_nzlhs, ilhs, lhs);
    if (st != BLU_OK) return st;
    // step two: alpha = A' y with y scattered from the compressed solution on the device
    memset(h->mx_counts, 0, sizeof h->mx_counts);
    if (h->mx_ncol == 0) return BLU_OK;
    if (!hip_ok(h, hipMemsetAsync(h->mx_y, 0, (size_t)h->m * 8, h->stream), "hipMemset")) return BLU_ERROR_DEVICE;
    if (skip) {
        st = mx_upload_skip(h, skip);
        if (st != BLU_OK) return st;
    }
    mx_scatter(h);
    return mx_product(h, skip, alpha);
}

extern "C" int blu_hip_price(blu_hip *h, const double *y, const int64_t *skip, double *z)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->mx_set) return BLU_ERROR_INVALID_CALL;
    if ((h->m > 0 && !y) || (h->mx_ncol > 0 && !z)) return BLU_ERROR_ARGUMENT_MISSING;
    memset(h->mx_counts, 0, sizeof h->mx_counts);
    if (h->mx_ncol == 0) return BLU_OK;
    if (h->m == 0) { // (every column is empty)
        for (int64_t j = 0; j < h->mx_ncol; j++) z[j] = 0.0;
        return BLU_OK;
    }
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    if (!hip_ok(h, hipMemcpy(h->mx_y, y, (size_t)h->m * 8, hipMemcpyHostToDevice), "h2d y")) return BLU_ERROR_DEVICE;
    h->mx_counts[2]++;
    if (skip) {
        const int st = mx_upload_skip(h, skip);
        if (st != BLU_OK) return st;
    }
    return mx_product(h, skip, z);
}

// the part of the last blu_hip_tableau_row behind its solve, or the last blu_hip_price: kernel launches, synchronizes,
// host-to-device copies, bytes downloaded
extern "C" int blu_hip_dbg_matrix_counts(const blu_hip *h, int64_t out[4])
{
    if (!h || !out) return BLU_ERROR_ARGUMENT_MISSING;
    for (int k = 0; k < 4; k++) out[k] = h->mx_counts[k];
    return BLU_OK;
}
// debug hook of tools/tableau_probe.py: with on != 0 k_at_dot is bracketed by two events (off by default: two event
// records per call), and its device seconds in the last call are kept
extern "C" int blu_hip_dbg_set_matrix_timing(blu_hip *h, int on)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    h->mx_timing = on ? 1 : 0;
    return BLU_OK;
}
extern "C" double blu_hip_dbg_matrix_kernel_seconds(const blu_hip *h) { return h ? h->mx_kernel_s : 0.0; }
