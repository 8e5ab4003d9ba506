// blu_maxvolume.inc -- blu_hip_maxvolume (included by blu_hip.hip): one pass of maxvolume (src/maxvolume.rs:64-224) behind
// the C ABI.  The specification is the loop of blu_amd/maxvolume.py over blu_hip_factorize / blu_hip_solve_for_update /
// blu_hip_update on the same handle; the pass takes that loop's decisions and leaves the handle as the loop leaves it,
// statistics included, but prices the candidate columns in chunks:
//   k_price_multi   one wave per candidate on a slot of the pool of blu_hip_solve_sparse_multi: the mode-0 solve of its
//                   column of the resident A (the forward solve_for_update with a solution is that solve plus the stored
//                   spike), then the scan for the largest entry
//   k_price_pick    one wave: the first candidate that is taken or refused, the flop counters of those in front of it into
//                   the update state, one 64-byte record for the host
// A candidate that is taken is solved again through the single mode-1 path (it stores the spike and counts itself), then
// the transposed solve, the update and the refactorization rule as in the loop; what the chunk priced behind it is thrown
// away and priced again against the new factors.  A is uploaded once per pass.

// The handle lets go of a matrix it holds with others (blu_hip_share_matrix): the reference is dropped, the last holder
// frees the arrays, and the handle goes on as one that never had buffers.  The two places that write or free the arrays
// of A -- mv_upload and free_maxvolume -- come through here first.
static void mx_detach(blu_hip *h)
{
    MatShare *S = h->mx_share;
    if (!S) return;
    if (--S->refs == 0) {
        dfree(S->ap); dfree(S->ai64); dfree(S->ai); dfree(S->ax); dfree(S->bt); dfree(S->rt);
        delete S;
    }
    h->mx_share = nullptr;
    h->mv_ap = nullptr;
    h->mv_ai64 = nullptr;
    h->mv_ai = nullptr;
    h->mv_ax = nullptr;
    h->mv_pcap = h->mv_nzcap = 0;
    h->mx_hp = nullptr;
    h->mx_set = false;
}

static void free_maxvolume(blu_hip *h)
{
    mx_detach(h);
    dfree(h->mv_ap); dfree(h->mv_ai64); dfree(h->mv_ai); dfree(h->mv_ax); dfree(h->mv_cols); dfree(h->mv_rec);
    h->mv_pcap = h->mv_nzcap = h->mv_colscap = 0;
}

// A[:, 0..ncol) into the handle's buffers: offsets relative to a_p[0], row indices twice, values
static int mv_upload(blu_hip *h, int64_t ncol, const uint64_t *a_p, const uint64_t *a_i, const double *a_x)
{
    const uint64_t base = a_p[0];
    const size_t np = (size_t)ncol + 1, nz = (size_t)(a_p[ncol] - base);
    mx_detach(h);
    if ((int64_t)np > h->mv_pcap) {
        dfree(h->mv_ap);
        h->mv_pcap = 0;
        if (!dalloc(h, &h->mv_ap, np)) return BLU_ERROR_OUT_OF_MEMORY;
        h->mv_pcap = (int64_t)np;
    }
    if ((int64_t)nz > h->mv_nzcap) {
        dfree(h->mv_ai64); dfree(h->mv_ai); dfree(h->mv_ax);
        h->mv_nzcap = 0;
        if (!dalloc(h, &h->mv_ai64, nz) || !dalloc(h, &h->mv_ai, nz) || !dalloc(h, &h->mv_ax, nz)) return BLU_ERROR_OUT_OF_MEMORY;
        h->mv_nzcap = (int64_t)nz;
    }
    if (!h->mv_rec && !dalloc(h, &h->mv_rec, 8)) return BLU_ERROR_OUT_OF_MEMORY;
    std::vector<long long> ap(np);
    for (size_t j = 0; j < np; j++) ap[j] = (long long)(a_p[j] - base);
    std::vector<int> ai(nz);
    for (size_t q = 0; q < nz; q++) ai[q] = a_i[base + q] < 0x7fffffffull ? (int)a_i[base + q] : 0x7fffffff;
    bool ok = hip_ok(h, hipMemcpy(h->mv_ap, ap.data(), np * sizeof(long long), hipMemcpyHostToDevice), "h2d a_p");
    if (nz)
        ok = ok && hip_ok(h, hipMemcpy(h->mv_ai64, a_i + base, nz * 8, hipMemcpyHostToDevice), "h2d a_i") &&
             hip_ok(h, hipMemcpy(h->mv_ai, ai.data(), nz * sizeof(int), hipMemcpyHostToDevice), "h2d a_i") &&
             hip_ok(h, hipMemcpy(h->mv_ax, a_x + base, nz * 8, hipMemcpyHostToDevice), "h2d a_x");
    return ok ? BLU_OK : BLU_ERROR_DEVICE;
}

// factorize A[:, basis] (maxvolume.rs:180-197) from the resident A: begin / end of the basis columns are a small upload
static int mv_factorize(blu_hip *h, const uint64_t *a_p, const int64_t *basis, uint64_t nz)
{
    const size_t M = (size_t)h->m;
    const uint64_t base = a_p[0];
    std::vector<uint64_t> bb(M), be(M);
    for (size_t i = 0; i < M; i++) {
        bb[i] = a_p[basis[i]] - base;
        be[i] = a_p[basis[i] + 1] - base;
    }
    if ((int64_t)M > h->ob_mcap) {
        dfree(h->ob_begin); dfree(h->ob_end);
        h->ob_mcap = 0;
        if (!dalloc(h, &h->ob_begin, M) || !dalloc(h, &h->ob_end, M)) return BLU_ERROR_OUT_OF_MEMORY;
        h->ob_mcap = (int64_t)M;
    }
    if (M && (!hip_ok(h, hipMemcpy(h->ob_begin, bb.data(), M * 8, hipMemcpyHostToDevice), "h2d b_begin") ||
              !hip_ok(h, hipMemcpy(h->ob_end, be.data(), M * 8, hipMemcpyHostToDevice), "h2d b_end")))
        return BLU_ERROR_DEVICE;
    return factorize_device_impl(h, (const uint64_t *)h->ob_begin, (const uint64_t *)h->ob_end, (const uint64_t *)h->mv_ai64, h->mv_ax, nz);
}

extern "C" int blu_hip_maxvolume(blu_hip *h, int64_t ncol, const uint64_t *a_p, const uint64_t *a_i, const double *a_x, int64_t *basis,
                                 int64_t *isbasic, double volumetol, int64_t *p_nupdate)
{
    // refusals before anything is touched
    if (!h || !a_p || !basis || !isbasic) return BLU_ERROR_ARGUMENT_MISSING;
    if (ncol < 0 || ncol > kIntMax) return BLU_ERROR_INVALID_ARGUMENT;
    for (int64_t j = 0; j < ncol; j++)
        if (a_p[j + 1] < a_p[j]) return BLU_ERROR_INVALID_ARGUMENT;
    const uint64_t nz = a_p[ncol] - a_p[0];
    if (nz > 0 && (!a_i || !a_x)) return BLU_ERROR_ARGUMENT_MISSING;
    const int64_t m = h->m;
    for (int64_t i = 0; i < m; i++)
        if (basis[i] < 0 || basis[i] >= ncol) return BLU_ERROR_INVALID_ARGUMENT;
    int64_t nupdate = 0;
    auto done = [&](int code) {
        if (p_nupdate) *p_nupdate = nupdate;
        return code;
    };
    if (volumetol < 1.0) return done(BLU_ERROR_INVALID_ARGUMENT); // maxvolume.rs:84-91
    memset(h->mv_counts, 0, sizeof h->mv_counts);
    if (nz > (uint64_t)kIntMax) { // (32-bit device indices: what the loop's first factorize answers)
        reset_lu(h);
        return done(BLU_ERROR_INVALID_ARGUMENT);
    }
    if (hipSetDevice(h->device) != hipSuccess) return done(BLU_ERROR_DEVICE);
    h->mx_set = false; // (blu_matrix.inc: the buffers of a set matrix get an A nobody validated)
    du_drop(h);
    int st = mv_upload(h, ncol, a_p, a_i, a_x);
    if (st != BLU_OK) return done(st);
    st = mv_factorize(h, a_p, basis, nz);
    if (st != BLU_OK) return done(st); // (WARNING_SINGULAR_MATRIX: the algorithm failed, maxvolume.rs:61-62)

    hipStream_t stream = h->stream;
    const int nz_sparse = (int)(h->sparse_thres * (double)m);
    const PriceA A{h->mv_ap, h->mv_ai, h->mv_ax};
    int64_t max_slots = 0; // of the pool: the byte limit and the slot limit of blu_hip_solve_sparse_multi
    if (m > 0) {
        const int64_t limit = h->sm_ws_bytes >= 0 ? h->sm_ws_bytes : kSparseMultiWsBytes;
        max_slots = std::min<int64_t>(std::max<int64_t>(limit / sparse_multi_slot_bytes(h), 1), kSparseMultiMaxSlots);
    }
    int64_t cur = h->mv_chunk > 0 ? h->mv_chunk : 64;
    std::vector<int> cols;
    auto fail = [&](int code) { // a failure behind a launch may leave slots in the middle of a solve: the pool is dropped
        (void)hipStreamSynchronize(stream);
        if (code == BLU_ERROR_DEVICE) free_sparse_multi_pool(h);
        return done(code);
    };
    for (int64_t cursor = 0; cursor < ncol;) {
        // the next candidates at or behind the cursor
        const int64_t want = m > 0 ? std::min<int64_t>(cur, max_slots) : 1;
        cols.clear();
        for (int64_t j = cursor; j < ncol && (int64_t)cols.size() < want; j++)
            if (!isbasic[j]) cols.push_back((int)j);
        int64_t nc = (int64_t)cols.size();
        if (nc == 0) break;
        // what blu_hip_solve_for_update answers before it looks at the column
        if (m == 0) return done(BLU_ERROR_INVALID_ARGUMENT);
        st = ensure_upd(h);
        if (st != BLU_OK) return done(st);
        if (h->ust.nforrest == m) return done(BLU_ERROR_MAXIMUM_UPDATES);
        {
            int64_t got = 0;
            st = ensure_sparse_multi(h, nc, &got);
            if (st != BLU_OK) return done(st);
            if (got < nc) {
                max_slots = got;
                nc = got;
                cols.resize((size_t)nc);
            }
        }
        if (nc > h->mv_colscap) {
            dfree(h->mv_cols);
            h->mv_colscap = 0;
            if (!dalloc(h, &h->mv_cols, (size_t)nc)) return done(BLU_ERROR_OUT_OF_MEMORY);
            h->mv_colscap = nc;
        }
        if (h->sm_marker > 0x7fffffff - 16) { // lu.rs:301-305: reset the marks before the marker overflows
            if (!hip_ok(h, hipMemsetAsync(h->sm_pool.marked, 0, (size_t)h->sm_slots * (size_t)m * sizeof(int), stream), "hipMemset"))
                return fail(BLU_ERROR_DEVICE);
            h->sm_marker = 0;
        }
        long long rec[8];
        if (!hip_ok(h, hipMemcpyAsync(h->mv_cols, cols.data(), (size_t)nc * sizeof(int), hipMemcpyHostToDevice, stream), "h2d candidates"))
            return fail(BLU_ERROR_DEVICE);
        hipLaunchKernelGGL(k_price_multi, dim3((unsigned)nc), dim3(64), 0, stream, h->dD, h->sm_pool, h->sw, h->uw, A, h->mv_cols, h->sm_marker,
                           nz_sparse);
        hipLaunchKernelGGL(k_price_pick, dim3(1), dim3(64), 0, stream, h->sm_pool, h->uw, h->mv_cols, (int)nc, volumetol, h->mv_rec);
        if (!hip_ok(h, hipStreamSynchronize(stream), "k_price_multi")) return fail(BLU_ERROR_DEVICE);
        h->sm_marker += 4;
        if (!hip_ok(h, hipMemcpy(rec, h->mv_rec, sizeof rec, hipMemcpyDeviceToHost), "d2h pick record")) return fail(BLU_ERROR_DEVICE);
        const int kind = (int)(rec[0] & 255), branch = (int)(rec[0] >> 8);
        const int64_t p = rec[1];
        if (kind < 0 || kind > 2 || p < 0 || p > nc || (kind == 0) != (p == nc) || (kind && rec[2] != cols[(size_t)p]) || rec[3] < 0 || rec[3] >= m) {
            h->err = "k_price_pick: record out of range"; // (never a valid state)
            return fail(BLU_ERROR_DEVICE);
        }
        h->mv_counts[0] += 1;
        h->mv_counts[1] += nc;
        // the candidates in front of the event, as their single calls leave the handle (fetch_solution; the host mirror
        // of what k_price_pick added to the update state)
        h->sp_l_flops += rec[5];
        h->sp_u_flops += rec[6];
        if (branch) h->sp_branch = branch;
        h->ust.status = UPD_OK;
        h->ust.l_flops += rec[5];
        h->ust.u_flops += rec[6];
        h->ust.r_flops += rec[7];
        h->ust.update_cost_numer += (double)rec[7];
        if (kind == 2) return done(BLU_ERROR_INVALID_ARGUMENT); // more than m entries or an index >= m, now that its turn has come
        if (kind == 0) {
            cursor = (int64_t)cols[(size_t)nc - 1] + 1;
            if (h->mv_chunk <= 0) cur = std::min<int64_t>(cur * 4, max_slots);
            continue;
        }
        // candidate j enters the basis at position imax (maxvolume.rs:138-142)
        const int64_t j = rec[2], imax = rec[3];
        double xtbl;
        memcpy(&xtbl, &rec[4], sizeof xtbl);
        h->mv_counts[2] += nc - p - 1;
        h->mv_counts[3] += 1;
        // its solve_for_update, now with the spike stored; the solution stays on the device.  The loop makes this solve
        // before it touches the basis: a failure here leaves basis, isbasic and nupdate as they were
        const uint64_t off = a_p[j] - a_p[0];
        st = run_solve_upd(h, 1, 1, (int64_t)(a_p[j + 1] - a_p[j]), 0, h->mv_ai + off, h->mv_ax + off);
        if (st == BLU_OK) st = fetch_solution(h, nullptr, nullptr, nullptr);
        if (st != BLU_OK) return done(st);
        isbasic[basis[imax]] = 0;
        isbasic[j] = 1;
        basis[imax] = j;
        nupdate++;
        // the row eta for position imax
        const uint64_t im = (uint64_t)imax;
        st = upload_rhs(h, 1, &im, nullptr);
        if (st == BLU_OK) st = run_solve_upd(h, 1, 0, 1, 1, h->d_irhs, h->d_xrhs);
        if (st == BLU_OK) st = fetch_solution(h, nullptr, nullptr, nullptr);
        if (st != BLU_OK) return done(st);
        st = blu_hip_update(h, xtbl);
        if (st != BLU_OK) return done(st);
        // refactorize_if_needed (maxvolume.rs:199-224)
        if (h->ust.nforrest == m || h->ust.pivot_error > 1e-8 || blu_hip_get_stat(h, BLU_STAT_UPDATE_COST) > 1.0) {
            st = mv_factorize(h, a_p, basis, nz);
            if (st != BLU_OK) return done(st);
        }
        cursor = j + 1;
        if (h->mv_chunk <= 0) cur = std::max<int64_t>(64, 2 * (p + 1));
    }
    return done(BLU_OK);
}

// debug / test hooks: a fixed number of candidates per chunk of blu_hip_maxvolume (n <= 0: the policy -- 64, times 4 after
// a chunk without a hit up to the pool's slots, max(64, 2 (p + 1)) after a hit at position p); results do not depend on it
extern "C" int blu_hip_dbg_set_maxvolume_chunk(blu_hip *h, int64_t n)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    h->mv_chunk = n > 0 ? n : 0;
    return BLU_OK;
}
// the last pass: chunks launched, candidates priced, candidates discarded behind a hit, hits
extern "C" int blu_hip_dbg_maxvolume_counts(const blu_hip *h, int64_t out[4])
{
    if (!h || !out) return BLU_ERROR_ARGUMENT_MISSING;
    for (int k = 0; k < 4; k++) out[k] = h->mv_counts[k];
    return BLU_OK;
}
