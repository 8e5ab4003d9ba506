// blu_solve_multi.inc -- blu_hip_solve_dense_multi (included by blu_hip.hip): blu_hip_solve_dense for many right-hand
// sides on ONE handle in one call.  Each right-hand side runs on one wave with a work vector of its own; the factors
// are shared:
//   k_build_lt               row-wise L of a fresh factorization, if a forward solve needs it and it does not exist yet
//                            (the same array ensure_lt builds, kept for later calls)
//   k_solve_dense_multi      fresh factorization (nupdate == 0): the sweeps of k_solve_dense, one workgroup per column
//   k_garbage_perm           updated factorization: the garbage permutation of the pivot sequence, once, on one wave
//   k_solve_dense_upd_multi  ... then the body of k_solve_dense_upd, one workgroup per column
// The columns go in chunks of C, launched back to back on the handle's stream, one synchronize at the end.  C is what
// keeps the work vectors (and, with host inputs, the staging block) within h->multi_ws_bytes.

static const int64_t kMultiWsBytes = (int64_t)1 << 30;

// doubles from one work vector to the next: the m + 2 a sweep may touch (what D.txrj provides), in whole 256-byte lines
static size_t multi_stride(const blu_hip *h) { return ((size_t)h->m + 2 + 31) & ~(size_t)31; }

static void free_multi(blu_hip *h)
{
    dfree(h->mws);
    dfree(h->mio);
    h->mws_cols = h->mio_cols = 0;
}

// work vectors (and staging block) for up to `want` columns at once; halved until the allocation succeeds
static int ensure_multi_ws(blu_hip *h, int64_t want, bool host_io, int64_t *got)
{
    const size_t stride = multi_stride(h);
    for (int64_t C = want; C >= 1; C /= 2) {
        bool ok = true;
        if (C > h->mws_cols) {
            dfree(h->mws);
            h->mws_cols = 0;
            ok = dalloc(h, &h->mws, (size_t)C * stride);
            if (ok) h->mws_cols = C;
        }
        if (ok && host_io && C > h->mio_cols) {
            dfree(h->mio);
            h->mio_cols = 0;
            ok = dalloc(h, &h->mio, (size_t)C * stride);
            if (ok) h->mio_cols = C;
        }
        if (ok) {
            *got = C;
            return BLU_OK;
        }
        (void)hipGetLastError();
    }
    return BLU_ERROR_OUT_OF_MEMORY;
}

// nc columns of m doubles between a host block (leading dimension ld) and the staging block (leading dimension stride)
static hipError_t multi_copy(blu_hip *h, double *dst, size_t dld, const double *src, size_t sld, int64_t nc, hipMemcpyKind kind)
{
    const size_t w = (size_t)h->m * sizeof(double);
    if (nc == 1) return hipMemcpyAsync(dst, src, w, kind, h->stream);
    return hipMemcpy2DAsync(dst, dld * sizeof(double), src, sld * sizeof(double), w, (size_t)nc, kind, h->stream);
}

extern "C" int blu_hip_solve_dense_multi(blu_hip *h, int64_t nrhs, const double *rhs, int64_t ldrhs, double *lhs, int64_t ldlhs, char trans,
                                         int inputs_on_device)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (h->nupdate < 0) return BLU_ERROR_INVALID_CALL; // solve_dense.rs:25-27
    if (!rhs || !lhs) return BLU_ERROR_ARGUMENT_MISSING;
    if (nrhs < 0 || (nrhs > 1 && (ldrhs < h->m || ldlhs < h->m))) return BLU_ERROR_INVALID_ARGUMENT;
    if (nrhs == 0 || h->m == 0) return BLU_OK;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    const int tr = (trans == 't' || trans == 'T') ? 1 : 0;
    const bool host_io = !inputs_on_device;
    const bool updated = h->nupdate > 0;
    const size_t stride = multi_stride(h);

    // what the solves need of the handle, as the single entry prepares it
    bool build_lt = false;
    if (updated) { // mutable U, row etas, pivot sequence (k_update.hip)
        int st = ensure_upd(h);
        if (st == BLU_OK) st = marker_room(h);
        if (st != BLU_OK) return st;
    } else if (!tr && h->lt_for_nfact != h->nfactorize) { // the forward L solve takes row dots (solve_dense.rs:79-86)
        const int st = ensure_lt_ws(h);
        if (st != BLU_OK) return st;
        build_lt = true;
    }

    // chunk size: the byte limit, then what can be allocated
    const int64_t limit = h->multi_ws_bytes >= 0 ? h->multi_ws_bytes : kMultiWsBytes;
    const int64_t per_col = (int64_t)(stride * sizeof(double)) * (host_io ? 2 : 1);
    int64_t C = std::min<int64_t>(nrhs, std::max<int64_t>(limit / per_col, 1));
    C = std::min<int64_t>(C, kIntMax); // (a grid dimension)
    const int st = ensure_multi_ws(h, C, host_io, &C);
    if (st != BLU_OK) return st;
    h->multi_last_chunk = C;

    hipStream_t stream = h->stream;
    if (build_lt) hipLaunchKernelGGL(k_build_lt, dim3(1), dim3(1024), 0, stream, h->dD, h->sw);
    if (updated) hipLaunchKernelGGL(k_garbage_perm, dim3(1), dim3(64), 0, stream, h->dD, h->sw, h->uw, h->marker);
    bool ok = true;
    for (int64_t c0 = 0; ok && c0 < nrhs; c0 += C) {
        const int64_t nc = std::min<int64_t>(C, nrhs - c0);
        const double *r = rhs + c0 * ldrhs;
        double *x = lhs + c0 * ldlhs;
        long long ldr = ldrhs, ldx = ldlhs;
        if (host_io) { // staged through the in-place block: one upload and one download per chunk
            ok = hip_ok(h, multi_copy(h, h->mio, stride, r, (size_t)ldrhs, nc, hipMemcpyHostToDevice), "h2d rhs block");
            if (!ok) break;
            r = x = h->mio;
            ldr = ldx = (long long)stride;
        }
        if (updated)
            hipLaunchKernelGGL(k_solve_dense_upd_multi, dim3((unsigned)nc), dim3(64), 0, stream, h->dD, h->sw, h->uw, r, ldr, x, ldx, h->mws,
                               (long long)stride, tr, h->marker);
        else
            hipLaunchKernelGGL(k_solve_dense_multi, dim3((unsigned)nc), dim3(64), 0, stream, h->dD, h->dO, r, ldr, x, ldx, h->mws, (long long)stride, tr,
                               h->sw.lt_ptr, h->sw.lt_idx, h->sw.lt_val);
        if (host_io) ok = hip_ok(h, multi_copy(h, lhs + c0 * ldlhs, (size_t)ldlhs, h->mio, stride, nc, hipMemcpyDeviceToHost), "d2h lhs block");
    }
    const bool synced = hip_ok(h, hipStreamSynchronize(stream), updated ? "k_solve_dense_upd_multi" : "k_solve_dense_multi");
    if (!ok || !synced) return BLU_ERROR_DEVICE;
    if (build_lt) h->lt_for_nfact = h->nfactorize;
    if (updated) h->marker += 4;
    return BLU_OK;
}

// debug / test hook: byte limit of the work vectors plus staging block of blu_hip_solve_dense_multi (default -1: 1 GiB);
// small values force the chunking at small shapes.  What is allocated is released, so the limit holds from the next call.
extern "C" int blu_hip_dbg_set_multi_ws_bytes(blu_hip *h, int64_t bytes)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    h->multi_ws_bytes = bytes;
    free_multi(h);
    return BLU_OK;
}
// columns per chunk of the last blu_hip_solve_dense_multi that reached its launches (0: none yet)
extern "C" int64_t blu_hip_dbg_multi_last_chunk(const blu_hip *h) { return h ? h->multi_last_chunk : 0; }
