// blu_matrix_batch.inc -- blu_hip_tableau_row_batch and blu_hip_price_batch (included by blu_hip.hip): what
// blu_hip_tableau_row / blu_hip_price (blu_matrix.inc) do, for many handles that hold ONE matrix (blu_hip_share_matrix) in
// one call.  Member k gets what the single entry gives on h[k]: status, the bits of every product, the solution when asked
// for, the counters and the state the solve leaves.
//   step one   the transposed solves of e_r[k]: the core of blu_hip_solve_sparse_batch (solve_sparse_batch_core), or with
//              prepare_update the core of the transposed blu_hip_solve_for_update_batch (solve_for_update_batch_core).  Each
//              member's compressed solution stays in its sw.ilhs / sw.xval / sw.out[0] on the device.
//   step two   on h[0]'s stream, per chunk of members: one hipMemsetAsync of the y tiles, one upload of the scatter
//              descriptors, one upload of the skip masks if any member of the chunk passes a skip, k_scatter_lhs_batch,
//              k_at_dot_batch, one synchronize, one download of the chunk's products into a host staging block.
//              blu_hip_price_batch uploads the y tiles, laid out on the host, instead of memset + descriptors + scatter.
// The y tiles (member-interleaved in groups of ATB_G, k_matrix.hip), the products, the masks and the descriptors of a
// chunk live in one device block that the shared matrix block keeps (MatShare::bt): grown when needed, freed with the
// last holder.  It stays within kMatrixBatchBytes; more members are worked in chunks of whole groups, and the chunk is
// halved when the allocation fails.  No result depends on the chunking, on n or on a member's position in the call.
// blu_hip_dbg_matrix_counts(h[0]) reports the launches, synchronizes, uploads and downloaded bytes of step two.

static const int64_t kMatrixBatchBytes = (int64_t)1 << 30;

static MatShare *mx_share_block(blu_hip *h); // (blu_matrix.inc)

struct MxBatchLayout {
    size_t y, out, mask, src, bytes;
};
// the block for `groups` groups (8 * groups members) of a matrix with m rows and ncol columns
static MxBatchLayout mx_batch_layout(size_t M, size_t N, size_t groups)
{
    MxBatchLayout L;
    L.y = 0;
    L.out = align_up(groups * M * ATB_G * sizeof(double));
    L.mask = align_up(L.out + groups * ATB_G * N * sizeof(double));
    L.src = align_up(L.mask + groups * N);
    L.bytes = L.src + groups * ATB_G * sizeof(ScatterSrc);
    return L;
}

// blu_hip_ratio_test_batch (blu_ratio.inc): the products of a chunk are not downloaded; k_ratio_pick_batch picks on them
// and stores each member's row into its kept-row buffer, and the records come down.  Indexed by member like hs.
struct MxRatio {
    const double *sigma;
    double pivtol, dualtol;
    blu_ratio_result *out;
};

// the pick of one chunk behind its k_at_dot_batch, on h0's stream: the descriptors (grown with the chunk, kept with the
// shared matrix) uploaded, then one workgroup per member; the records lie behind the descriptors.  false: failed
static bool mx_batch_pick(blu_hip *h0, blu_hip **hs, MatShare *S, const std::vector<int> &members, const double *dOut, size_t N, const MxRatio &rt,
                          std::vector<PickSrc> &ps) // (ps: host memory that lives until the synchronize)
{
    const size_t cn = members.size(), rec0 = align_up(cn * sizeof(PickSrc)), want = rec0 + cn * sizeof(blu_ratio_result);
    if (want > S->rt_cap) {
        dfree(S->rt);
        S->rt_cap = 0;
        if (!hip_ok(h0, hipMalloc((void **)&S->rt, want), "hipMalloc")) {
            (void)hipGetLastError();
            S->rt = nullptr;
            return false;
        }
        S->rt_cap = want;
    }
    ps.resize(cn);
    for (size_t s = 0; s < cn; s++) {
        blu_hip *h = hs[members[s]];
        ps[s] = PickSrc{h->du_d, h->du_kind, h->du_row, rt.sigma[members[s]]};
    }
    const bool ok = hip_ok(h0, hipMemcpyAsync(S->rt, ps.data(), cn * sizeof(PickSrc), hipMemcpyHostToDevice, h0->stream), "h2d pick descriptors");
    h0->mx_counts[2]++;
    if (!ok) return false;
    hipLaunchKernelGGL(k_ratio_pick_batch, dim3((unsigned)cn), dim3(PICK_THREADS_BATCH), 0, h0->stream, (const PickSrc *)S->rt, dOut, (int)N,
                       rt.pivtol, rt.dualtol, (RatioRec *)(S->rt + rec0));
    h0->mx_counts[0]++;
    return true;
}

// Step two for the members in `live` (all hold the matrix hm holds): member k's products into outs[k].  ys == NULL: y is
// scattered from the member's compressed solution on the device; else ys[k] is its dense y on the host.  Members a failed
// step takes with it get BLU_ERROR_DEVICE (BLU_ERROR_OUT_OF_MEMORY if the block of one group cannot be had).
// With rt (ys, skip and outs NULL) the masks come from the members' host mirrors of kind, and behind k_at_dot_batch the
// chunk goes on as described at MxRatio: one more upload (the pick descriptors), one more launch, 64 bytes per member down.
static void mx_batch_products(blu_hip *h0, blu_hip **hs, const std::vector<int> &live, const double *const *ys, const int64_t *const *skip,
                              double *const *outs, std::vector<int> &result, const MxRatio *rt = nullptr)
{
    if (live.empty()) return;
    blu_hip *hm = hs[live[0]];
    const size_t M = (size_t)hm->m, N = (size_t)hm->mx_ncol;
    if (N == 0) return;
    MatShare *S = mx_share_block(hm);
    const size_t total_groups = (live.size() + ATB_G - 1) / ATB_G;
    const size_t limit = (size_t)(S->bt_limit >= 0 ? S->bt_limit : kMatrixBatchBytes);
    size_t gc = std::min<size_t>(std::max<size_t>(limit / mx_batch_layout(M, N, 1).bytes, 1), std::min<size_t>(total_groups, 65535)); // (the grid: 65535 groups at most)
    while (gc > 1 && mx_batch_layout(M, N, gc).bytes > limit) gc--;
    while (mx_batch_layout(M, N, gc).bytes > S->bt_cap) { // grow the block; halve the chunk if the device refuses
        const size_t want = mx_batch_layout(M, N, gc).bytes;
        dfree(S->bt);
        S->bt_cap = 0;
        if (hip_ok(h0, hipMalloc((void **)&S->bt, want), "hipMalloc")) {
            S->bt_cap = want;
            break;
        }
        (void)hipGetLastError();
        S->bt = nullptr;
        if (gc == 1) {
            fail_members(h0, hs, live, result, BLU_ERROR_OUT_OF_MEMORY);
            return;
        }
        gc /= 2;
    }
    const MxBatchLayout L = mx_batch_layout(M, N, gc);
    double *dY = (double *)(S->bt + L.y), *dOut = (double *)(S->bt + L.out);
    unsigned char *dMask = (unsigned char *)(S->bt + L.mask);
    ScatterSrc *dSrc = (ScatterSrc *)(S->bt + L.src);
    const MatA A{hm->mv_ap, hm->mv_ai, hm->mv_ax};
    hipStream_t stream = h0->stream;
    const unsigned waves = (unsigned)((N + 63) / 64), per = ATD_THREADS / 64, nbx = (waves + per - 1) / per; // workgroups per group
    std::vector<double> tile, down;
    std::vector<unsigned char> mask;
    std::vector<ScatterSrc> src;
    std::vector<blu_ratio_result> recs;
    std::vector<PickSrc> ps;
    if (h0->mx_timing) h0->mx_kernel_s = 0.0;

    for (size_t c0 = 0; c0 < live.size(); c0 += gc * ATB_G) {
        const size_t cn = std::min(live.size() - c0, gc * ATB_G), groups = (cn + ATB_G - 1) / ATB_G;
        const std::vector<int> members(live.begin() + (long)c0, live.begin() + (long)(c0 + cn));
        bool ok = true, any_skip = false;
        if (ys) { // the y tiles laid out on the host (absent members of the last group: zero columns)
            tile.assign(groups * M * ATB_G, 0.0);
            for (size_t s = 0; s < cn; s++) {
                double *col = tile.data() + (s / ATB_G) * M * ATB_G + s % ATB_G;
                const double *y = ys[members[s]];
                for (size_t i = 0; i < M; i++) col[i * ATB_G] = y[i];
            }
            ok = hip_ok(h0, hipMemcpyAsync(dY, tile.data(), tile.size() * sizeof(double), hipMemcpyHostToDevice, stream), "h2d y tiles");
            h0->mx_counts[2]++;
        } else {
            src.resize(cn);
            for (size_t s = 0; s < cn; s++) {
                const SparseWs &W = hs[members[s]]->sw;
                src[s] = ScatterSrc{W.out, W.ilhs, W.xval};
            }
            ok = hip_ok(h0, hipMemsetAsync(dY, 0, groups * M * ATB_G * sizeof(double), stream), "hipMemset") &&
                 hip_ok(h0, hipMemcpyAsync(dSrc, src.data(), cn * sizeof(ScatterSrc), hipMemcpyHostToDevice, stream), "h2d scatter descriptors");
            h0->mx_counts[2]++;
        }
        for (size_t s = 0; skip && s < cn; s++) any_skip = any_skip || skip[members[s]];
        any_skip = any_skip || rt;
        if (ok && any_skip) { // bit t of mask[g * ncol + j]: member t of group g skips column j
            mask.assign(groups * N, 0);
            for (size_t s = 0; s < cn; s++) {
                const int64_t *sk = rt ? nullptr : skip[members[s]];
                const signed char *kd = rt ? hs[members[s]]->du_hkind.data() : nullptr;
                if (!sk && !kd) continue;
                unsigned char *row = mask.data() + (s / ATB_G) * N;
                const unsigned char bit = (unsigned char)(1u << (s % ATB_G));
                if (kd) { // (branch-free: ncol bytes per member, on the host, in every call)
                    for (size_t j = 0; j < N; j++) row[j] |= (unsigned char)(kd[j] == 0 ? bit : 0);
                    continue;
                }
                for (size_t j = 0; j < N; j++)
                    if (sk[j] != 0) row[j] |= bit;
            }
            ok = hip_ok(h0, hipMemcpyAsync(dMask, mask.data(), mask.size(), hipMemcpyHostToDevice, stream), "h2d skip masks");
            h0->mx_counts[2]++;
        }
        if (ok) {
            if (!ys) {
                hipLaunchKernelGGL(k_scatter_lhs_batch, dim3((unsigned)cn), dim3(256), 0, stream, dSrc, (int)M, dY);
                h0->mx_counts[0]++;
            }
            if (h0->mx_timing) (void)hipEventRecord(h0->ev[0], stream);
            hipLaunchKernelGGL(k_at_dot_batch, dim3(nbx * (unsigned)groups), dim3(ATD_THREADS), 0, stream, A, dY, any_skip ? dMask : nullptr,
                               (int)N, (int)M, (int)cn, (int)nbx, dOut);
            h0->mx_counts[0]++;
            if (h0->mx_timing) (void)hipEventRecord(h0->ev[1], stream);
            if (rt) ok = mx_batch_pick(h0, hs, S, members, dOut, N, *rt, ps);
            ok = ok && hip_ok(h0, hipStreamSynchronize(stream), rt ? "k_ratio_pick_batch" : "k_at_dot_batch");
            h0->mx_counts[1]++;
            if (h0->mx_timing && ok) {
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, h0->ev[0], h0->ev[1]) == hipSuccess) h0->mx_kernel_s += 1e-3 * (double)ms;
            }
        }
        if (ok && rt) {
            recs.resize(cn);
            ok = hip_ok(h0, hipMemcpy(recs.data(), S->rt + align_up(cn * sizeof(PickSrc)), cn * sizeof(blu_ratio_result), hipMemcpyDeviceToHost),
                        "d2h records");
        } else if (ok) {
            down.resize(cn * N);
            ok = hip_ok(h0, hipMemcpy(down.data(), dOut, cn * N * sizeof(double), hipMemcpyDeviceToHost), "d2h products");
        }
        if (!ok) { // this chunk and what is behind it
            fail_members(h0, hs, std::vector<int>(live.begin() + (long)c0, live.end()), result, BLU_ERROR_DEVICE);
            return;
        }
        if (rt) {
            h0->mx_counts[3] += (int64_t)(cn * sizeof(blu_ratio_result));
            for (size_t s = 0; s < cn; s++) {
                rt->out[members[s]] = recs[s];
                hs[members[s]]->du_row_valid = true;
            }
            continue;
        }
        h0->mx_counts[3] += (int64_t)(cn * N * sizeof(double));
        for (size_t s = 0; s < cn; s++) memcpy(outs[members[s]], down.data() + s * N, N * sizeof(double));
    }
}

// what both entries refuse as a whole behind their NULL checks: the handle list, then members with a set matrix that do
// not all hold the same one (the device pointer mv_ap tells)
static int mx_batch_refusal(blu_hip *const *hs, int n)
{
    if (const int st = batch_handles_refusal(hs, n); st != BLU_OK) return st;
    const long long *ap = nullptr;
    for (int k = 0; k < n; k++) {
        if (!hs[k]->mx_set) continue;
        if (ap && hs[k]->mv_ap != ap) return BLU_ERROR_INVALID_ARGUMENT;
        ap = hs[k]->mv_ap;
    }
    return BLU_OK;
}

// step one of blu_hip_tableau_row_batch and blu_hip_ratio_test_batch (blu_ratio.inc) for the members still pending in
// result: the batched transposed solves of e_r[k]; afterwards no member is pending
static void mx_batch_row_solves(blu_hip *h0, blu_hip **hs, int n, const int64_t *r, int prepare_update, int64_t *nzlhs, int64_t *const *ilhs,
                                double *const *lhs, std::vector<int> &result)
{
    const bool fetch = nzlhs && ilhs && lhs;
    std::vector<char> gather((size_t)n, 0);
    std::vector<uint64_t> ir((size_t)n);
    std::vector<const uint64_t *> pir((size_t)n);
    for (int k = 0; k < n; k++) {
        gather[(size_t)k] = (fetch && ilhs[k] && lhs[k]) ? 1 : 0;
        ir[(size_t)k] = (uint64_t)r[k];
        pir[(size_t)k] = &ir[(size_t)k];
    }
    if (prepare_update) { // blu_hip_solve_for_update(h, ., [r], ., 'T') with a solution
        solve_for_update_batch_core(h0, hs, n, nullptr, pir.data(), nullptr, nzlhs, ilhs, lhs, 1, std::vector<char>((size_t)n, 1), gather, result);
    } else { // blu_hip_solve_sparse(h, 1, [r], [1.0], ..., 'T')
        const double one = 1.0;
        const std::vector<int64_t> nz((size_t)n, 1);
        const std::vector<const double *> pxr((size_t)n, &one);
        solve_sparse_batch_core(h0, hs, n, nz.data(), pir.data(), pxr.data(), nzlhs, ilhs, lhs, 1, gather, result);
    }
    for (int k = 0; k < n; k++)
        if (result[k] == kPending) result[k] = BLU_ERROR_DEVICE;
}

extern "C" int blu_hip_tableau_row_batch(blu_hip **hs, int n, const int64_t *r, int prepare_update, const int64_t *const *skip,
                                         double *const *alpha, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, int *status)
{
    // refusals of the call as a whole: every status[k] carries the code, no handle is touched
    if (!hs || !r || !alpha || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (!hs[k] || (hs[k]->mx_set && hs[k]->mx_ncol > 0 && !alpha[k])) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (const int st = mx_batch_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    blu_hip *h0 = hs[0];
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);

    // per member, in the order of blu_hip_tableau_row: the matrix, then the refusals of its solve
    std::vector<int> result(n, kPending);
    for (int k = 0; k < n; k++)
        if (!hs[k]->mx_set) result[k] = BLU_ERROR_INVALID_CALL;
    mx_batch_row_solves(h0, hs, n, r, prepare_update, nzlhs, ilhs, lhs, result);

    // step two for the members whose solve ended well
    memset(h0->mx_counts, 0, sizeof h0->mx_counts);
    std::vector<int> live;
    for (int k = 0; k < n; k++)
        if (result[k] == BLU_OK) live.push_back(k);
    mx_batch_products(h0, hs, live, nullptr, skip, alpha, result);
    return batch_return(result, status);
}

extern "C" int blu_hip_price_batch(blu_hip **hs, int n, const double *const *y, const int64_t *const *skip, double *const *z, int *status)
{
    if (!hs || !y || !z || n < 0) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++) {
        if (!hs[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
        if (hs[k]->mx_set && ((hs[k]->m > 0 && !y[k]) || (hs[k]->mx_ncol > 0 && !z[k]))) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    }
    if (const int st = mx_batch_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st);
    blu_hip *h0 = hs[0];
    std::vector<int> result(n, kPending), live;
    for (int k = 0; k < n; k++) {
        if (!hs[k]->mx_set) {
            result[k] = BLU_ERROR_INVALID_CALL;
            continue;
        }
        result[k] = BLU_OK;
        if (hs[k]->m == 0) // (every column is empty)
            for (int64_t j = 0; j < hs[k]->mx_ncol; j++) z[k][j] = 0.0;
        else live.push_back(k);
    }
    memset(h0->mx_counts, 0, sizeof h0->mx_counts);
    if (!live.empty() && hs[live[0]]->mx_ncol > 0) {
        if (hipSetDevice(h0->device) != hipSuccess) fail_members(h0, hs, live, result, BLU_ERROR_DEVICE);
        else mx_batch_products(h0, hs, live, y, skip, z, result);
    }
    return batch_return(result, status);
}

// debug hook of the tests: the byte limit of the block of the batched products of h's matrix (< 0: the default), so that
// test sizes take two or more chunks; results do not depend on it
extern "C" int blu_hip_dbg_set_matrix_batch_bytes(blu_hip *h, int64_t bytes)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (!h->mx_set) return BLU_ERROR_INVALID_CALL;
    mx_share_block(h)->bt_limit = bytes;
    return BLU_OK;
}
