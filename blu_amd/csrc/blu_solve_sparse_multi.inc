// blu_solve_sparse_multi.inc -- blu_hip_solve_sparse_multi / blu_hip_get_sparse_multi (included by blu_hip.hip):
// blu_hip_solve_sparse for many right-hand sides on ONE handle in one call.  Each right-hand side runs on one wave with
// a workspace of its own out of the handle's pool (SparseSlots, k_solve_sparse.hip); the factors are shared:
//   k_build_lt            row-wise L of a fresh factorization, if a transposed call needs it and it does not exist yet
//                         (the same array ensure_lt builds, kept for later calls)
//   k_solve_sparse_multi  fresh factorization (nupdate == 0): the body of k_solve_sparse, one workgroup per column
//   k_solve_upd_multi     updated factorization: the body of k_solve_upd, mode 0, without its writes to the UpdState
//   k_upd_add_flops       ... which one lane makes once, behind the last chunk
//   k_gather_lhs_multi    the compressed solutions of a chunk into the result buffer of the call
// The columns go in chunks of C slots.  A chunk is one upload (its right-hand sides, packed), the solve launch, one
// synchronize, one download of the slots' counters and the gather launch; the call ends with one synchronize and the
// download of the gathered solutions, which stay on the host until the next call.  The counters size the result buffer,
// so the host waits for every chunk's solves before it launches the next chunk: chunks are serial, only the gather of
// one chunk overlaps the upload of the next.

static const int64_t kSparseMultiWsBytes = (int64_t)1 << 30;
// slots per chunk at the most: far more than the chip runs at once (24 KB of LDS each), and k_gather_lhs_multi sums the
// counters in front of every slot
static const int64_t kSparseMultiMaxSlots = 8192;

// bytes of one slot: the nine private arrays of SparseWs (six of int, three of double: 48 bytes per row) and its counters
static int64_t sparse_multi_slot_bytes(const blu_hip *h) { return 48 * (int64_t)h->m + 8 * (int64_t)sizeof(long long); }

static void free_sparse_multi_pool(blu_hip *h)
{
    SparseSlots &P = h->sm_pool;
    dfree(P.marked); dfree(P.psym); dfree(P.pat); dfree(P.pstack); dfree(P.estack); dfree(P.ilhs);
    dfree(P.work); dfree(P.xlhs); dfree(P.xval); dfree(P.out);
    h->sm_slots = 0;
    h->sm_marker = 0;
}
static void free_sparse_multi(blu_hip *h)
{
    free_sparse_multi_pool(h);
    dfree(h->sm_stage);
    h->sm_stage_cap = 0;
    dfree(h->sm_gidx);
    dfree(h->sm_gval);
    h->sm_gcap = 0;
}

// a pool of `want` slots; halved until the allocation succeeds.  A new pool starts as the handle's own workspace does:
// marks, work and xlhs all zero, marker 0.
static int ensure_sparse_multi(blu_hip *h, int64_t want, int64_t *got)
{
    if (want <= h->sm_slots) {
        *got = want;
        return BLU_OK;
    }
    free_sparse_multi_pool(h);
    SparseSlots &P = h->sm_pool;
    for (int64_t C = want; C >= 1; C /= 2) {
        const size_t n = (size_t)C * (size_t)h->m;
        bool ok = dalloc(h, &P.marked, n) && dalloc(h, &P.psym, n) && dalloc(h, &P.pat, n) && dalloc(h, &P.pstack, n) && dalloc(h, &P.estack, n) &&
                  dalloc(h, &P.ilhs, n) && dalloc(h, &P.work, n) && dalloc(h, &P.xlhs, n) && dalloc(h, &P.xval, n) && dalloc(h, &P.out, (size_t)C * 8);
        if (ok) {
            ok = hip_ok(h, hipMemset(P.marked, 0, n * sizeof(int)), "hipMemset") && hip_ok(h, hipMemset(P.work, 0, n * sizeof(double)), "hipMemset") &&
                 hip_ok(h, hipMemset(P.xlhs, 0, n * sizeof(double)), "hipMemset");
            if (!ok) {
                free_sparse_multi_pool(h);
                return BLU_ERROR_DEVICE;
            }
            P.m = h->m;
            h->sm_slots = C;
            h->sm_marker = 0;
            *got = C;
            return BLU_OK;
        }
        (void)hipGetLastError();
        free_sparse_multi_pool(h);
    }
    return BLU_ERROR_OUT_OF_MEMORY;
}

extern "C" int blu_hip_solve_sparse_multi(blu_hip *h, int64_t nrhs, const int64_t *rhs_ptr, const uint64_t *irhs, const double *xrhs, char trans,
                                          int64_t *lhs_ptr, int *status)
{
    // refusals of the call as a whole: nothing is written, nothing in the handle changes
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (h->nupdate < 0) return BLU_ERROR_INVALID_CALL; // solve_sparse.rs:46-47
    if (!rhs_ptr || !lhs_ptr) return BLU_ERROR_ARGUMENT_MISSING;
    if (nrhs > 0 && rhs_ptr[nrhs] > rhs_ptr[0] && (!irhs || !xrhs)) return BLU_ERROR_ARGUMENT_MISSING;
    if (nrhs < 0 || rhs_ptr[0] < 0) return BLU_ERROR_INVALID_ARGUMENT;
    for (int64_t j = 0; j < nrhs; j++)
        if (rhs_ptr[j + 1] < rhs_ptr[j]) return BLU_ERROR_INVALID_ARGUMENT;

    // per column, as blu_hip_solve_sparse checks its right-hand side (solve_sparse.rs:49-59)
    const int64_t m = h->m;
    std::vector<int> result((size_t)nrhs, BLU_OK);
    int64_t nvalid = 0;
    for (int64_t j = 0; j < nrhs; j++) {
        bool ok = rhs_ptr[j + 1] - rhs_ptr[j] <= m;
        for (int64_t q = rhs_ptr[j]; ok && q < rhs_ptr[j + 1]; q++) ok = irhs[q] < (uint64_t)m;
        if (ok) nvalid++;
        else result[(size_t)j] = BLU_ERROR_INVALID_ARGUMENT;
    }
    std::vector<long long> nz((size_t)nrhs, 0), branch((size_t)nrhs, 0);
    std::vector<int> il;
    std::vector<double> xv;
    long long l_flops = 0, u_flops = 0, r_flops = 0;
    const bool updated = h->nupdate > 0;
    int64_t chunk = 0; // slots per chunk, once the launches were reached
    const int tr = (trans == 't' || trans == 'T') ? 1 : 0;

    if (m > 0 && nvalid > 0) {
        if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
        // what the solves need of the handle, as the single entry prepares it
        bool build_lt = false;
        if (updated) { // mutable U, row etas, pivot sequence (k_update.hip)
            const int st = ensure_upd(h);
            if (st != BLU_OK) return st;
        } else if (tr && h->lt_for_nfact != h->nfactorize) { // the transposed system ends with L': row-wise L
            const int st = ensure_lt_ws(h);
            if (st != BLU_OK) return st;
            build_lt = true;
        }
        // chunk size: the byte limit, then what can be allocated
        const int64_t limit = h->sm_ws_bytes >= 0 ? h->sm_ws_bytes : kSparseMultiWsBytes;
        int64_t C = std::min<int64_t>(nrhs, std::max<int64_t>(limit / sparse_multi_slot_bytes(h), 1));
        C = std::min<int64_t>(C, kSparseMultiMaxSlots);
        {
            const int st = ensure_sparse_multi(h, C, &C);
            if (st != BLU_OK) return st;
        }
        chunk = C;

        hipStream_t stream = h->stream;
        const int nz_sparse = (int)(h->sparse_thres * (double)m); // lu/solve_sparse.rs:24
        const char *what = updated ? "k_solve_upd_multi" : "k_solve_sparse_multi";
        if (build_lt) hipLaunchKernelGGL(k_build_lt, dim3(1), dim3(1024), 0, stream, h->dD, h->sw);
        // a failure behind this point may leave slots in the middle of a solve: the pool is dropped with it
        auto fail = [&](int code) {
            (void)hipStreamSynchronize(stream);
            if (code == BLU_ERROR_DEVICE) free_sparse_multi_pool(h);
            return code;
        };
        int64_t filled = 0; // entries of the result buffer in use
        Stage S;
        std::vector<long long> out;
        for (int64_t c0 = 0; c0 < nrhs; c0 += C) {
            const int64_t nc = std::min<int64_t>(C, nrhs - c0);
            // the chunk's right-hand sides, packed: beg[nc] | xrhs | cnt[nc] | irhs
            size_t tot = 0;
            for (int64_t s = 0; s < nc; s++)
                if (result[(size_t)(c0 + s)] == BLU_OK) tot += (size_t)(rhs_ptr[c0 + s + 1] - rhs_ptr[c0 + s]);
            S.restart();
            const auto aB = S.add<long long>((size_t)nc);
            const auto aX = S.add<double>(tot);
            const auto aC = S.add<int>((size_t)nc);
            const auto aI = S.add<int>(std::max<size_t>(tot, 1));
            const size_t total = S.bytes;
            S.host_front(total);
            {
                long long *beg = S.h(aB);
                double *sx = S.h(aX);
                int *cnt = S.h(aC), *si = S.h(aI);
                size_t put = 0;
                for (int64_t s = 0; s < nc; s++) {
                    const int64_t j = c0 + s, b = rhs_ptr[j], e = rhs_ptr[j + 1];
                    beg[s] = (long long)put;
                    if (result[(size_t)j] != BLU_OK) {
                        cnt[s] = -1;
                        continue;
                    }
                    cnt[s] = (int)(e - b);
                    for (int64_t q = b; q < e; q++) si[put + (size_t)(q - b)] = (int)irhs[q];
                    if (e > b) memcpy(sx + put, xrhs + b, (size_t)(e - b) * sizeof(double));
                    put += (size_t)(e - b);
                }
            }
            if (total > h->sm_stage_cap) {
                (void)hipStreamSynchronize(stream); // (the chunk before may still read it)
                dfree(h->sm_stage);
                h->sm_stage_cap = 0;
                if (!dalloc(h, &h->sm_stage, total)) {
                    (void)hipGetLastError();
                    return fail(BLU_ERROR_OUT_OF_MEMORY);
                }
                h->sm_stage_cap = total;
            }
            if (h->sm_marker > 0x7fffffff - 16) { // lu.rs:301-305: reset the marks before the marker overflows
                if (!hip_ok(h, hipMemsetAsync(h->sm_pool.marked, 0, (size_t)h->sm_slots * (size_t)m * sizeof(int), stream), "hipMemset"))
                    return fail(BLU_ERROR_DEVICE);
                h->sm_marker = 0;
            }
            S.dev = h->sm_stage; // (kept by the handle)
            if (!hip_ok(h, hipMemcpyAsync(S.dev, S.host.data(), total, hipMemcpyHostToDevice, stream), "h2d right-hand sides"))
                return fail(BLU_ERROR_DEVICE);
            const MultiRhs R{S.d(aB), S.d(aC), S.d(aI), S.d(aX)};
            if (updated)
                hipLaunchKernelGGL(k_solve_upd_multi, dim3((unsigned)nc), dim3(64), 0, stream, h->dD, h->sm_pool, h->sw, h->uw, R, tr, h->sm_marker,
                                   nz_sparse);
            else
                hipLaunchKernelGGL(k_solve_sparse_multi, dim3((unsigned)nc), dim3(64), 0, stream, h->dD, h->dO, h->sm_pool, h->sw, R, tr, h->sm_marker,
                                   nz_sparse);
            if (!hip_ok(h, hipStreamSynchronize(stream), what)) return fail(BLU_ERROR_DEVICE);
            h->sm_marker += 4;
            if (build_lt) {
                h->lt_for_nfact = h->nfactorize;
                build_lt = false;
            }
            out.resize((size_t)nc * 8);
            if (!hip_ok(h, hipMemcpy(out.data(), h->sm_pool.out, (size_t)nc * 8 * sizeof(long long), hipMemcpyDeviceToHost), "d2h counters"))
                return fail(BLU_ERROR_DEVICE);
            int64_t got = 0;
            for (int64_t s = 0; s < nc; s++) {
                const long long *o = out.data() + 8 * s;
                if (o[0] < 0 || o[0] > m) { // (never a valid state)
                    h->err = std::string(what) + ": slot counters out of range";
                    return fail(BLU_ERROR_DEVICE);
                }
                nz[(size_t)(c0 + s)] = o[0];
                branch[(size_t)(c0 + s)] = o[3];
                l_flops += o[1];
                u_flops += o[2];
                r_flops += o[4];
                got += o[0];
            }
            if (filled + got > h->sm_gcap) { // the earlier chunks' entries are kept
                const int64_t cap = std::max<int64_t>(filled + got, 2 * h->sm_gcap);
                if (!dgrow(h, &h->sm_gidx, (size_t)filled, (size_t)cap) || !dgrow(h, &h->sm_gval, (size_t)filled, (size_t)cap)) {
                    (void)hipGetLastError();
                    dfree(h->sm_gidx);
                    dfree(h->sm_gval);
                    h->sm_gcap = 0;
                    return fail(BLU_ERROR_OUT_OF_MEMORY);
                }
                h->sm_gcap = cap;
            }
            if (got > 0)
                hipLaunchKernelGGL(k_gather_lhs_multi, dim3((unsigned)nc), dim3(256), 0, stream, h->sm_pool, (long long)filled, h->sm_gidx, h->sm_gval);
            filled += got;
        }
        if (updated) hipLaunchKernelGGL(k_upd_add_flops, dim3(1), dim3(64), 0, stream, h->uw, l_flops, u_flops, r_flops);
        if (!hip_ok(h, hipStreamSynchronize(stream), "k_gather_lhs_multi")) return fail(BLU_ERROR_DEVICE);
        il.resize((size_t)filled);
        xv.resize((size_t)filled);
        if (filled > 0 && (!hip_ok(h, hipMemcpy(il.data(), h->sm_gidx, (size_t)filled * sizeof(int), hipMemcpyDeviceToHost), "d2h patterns") ||
                           !hip_ok(h, hipMemcpy(xv.data(), h->sm_gval, (size_t)filled * sizeof(double), hipMemcpyDeviceToHost), "d2h values")))
            return fail(BLU_ERROR_DEVICE);
    }

    // the call went through: the result, the caller's arrays and the counters, as after the single calls in order
    lhs_ptr[0] = 0;
    for (int64_t j = 0; j < nrhs; j++) lhs_ptr[j + 1] = lhs_ptr[j] + nz[(size_t)j];
    h->sm_ilhs.assign(il.begin(), il.end());
    h->sm_xlhs.swap(xv);
    h->sm_have = true;
    if (chunk > 0) h->sm_last_chunk = chunk;
    if (m > 0 && nvalid > 0) {
        h->sp_l_flops += l_flops;
        h->sp_u_flops += u_flops;
        for (int64_t j = nrhs - 1; j >= 0; j--)
            if (result[(size_t)j] == BLU_OK) {
                h->sp_branch = (int)branch[(size_t)j];
                break;
            }
        if (updated) { // the host mirror of what k_upd_add_flops did
            h->ust.status = UPD_OK;
            h->ust.l_flops += l_flops;
            h->ust.u_flops += u_flops;
            h->ust.r_flops += r_flops;
            h->ust.update_cost_numer += (double)r_flops;
        }
    }
    return batch_return(result, status);
}

extern "C" int blu_hip_get_sparse_multi(blu_hip *h, int64_t *ilhs, double *xlhs)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->sm_have) return BLU_ERROR_INVALID_CALL;
    const size_t n = h->sm_ilhs.size();
    if (n == 0) return BLU_OK;
    if (!ilhs || !xlhs) return BLU_ERROR_ARGUMENT_MISSING;
    memcpy(ilhs, h->sm_ilhs.data(), n * sizeof(int64_t));
    memcpy(xlhs, h->sm_xlhs.data(), n * sizeof(double));
    return BLU_OK;
}

// debug / test hook: byte limit of the pool of blu_hip_solve_sparse_multi (default -1: 1 GiB); a slot takes 48 m + 64
// bytes, so small values force the chunking at small shapes (below one slot: one at a time).  What is allocated is
// released, so the limit holds from the next call.
extern "C" int blu_hip_dbg_set_sparse_multi_ws_bytes(blu_hip *h, int64_t bytes)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    h->sm_ws_bytes = bytes;
    free_sparse_multi_pool(h);
    return BLU_OK;
}
// right-hand sides per chunk of the last blu_hip_solve_sparse_multi that reached its launches and succeeded (0: none yet)
extern "C" int64_t blu_hip_dbg_sparse_multi_last_chunk(const blu_hip *h) { return h ? h->sm_last_chunk : 0; }
