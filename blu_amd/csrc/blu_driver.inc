// blu_driver.inc -- the factorize driver (included by blu_hip.hip).
//
// factorize() (src/factorize.rs:34-182) + BLU::factorize's reallocation loop (src/blu.rs:95-118),
// for a BATCH of independent handles on one device: every kernel is launched once for the whole
// batch, one workgroup per handle; the host only steps in between launches to grow storage for the
// handles that asked for it (ST_NEED_*), exactly what BLU::factorize does on `Status::Reallocate`.
// A single blu_hip_factorize call is the batch of one.

#define ST_HOLD 9 // host-only: "this handle has finished the current phase, skip it in a re-launch"

__global__ void k_gather_scalars(DevLU *Ds, Scalars *out, int n)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) out[b] = *Ds[b].s;
}
__global__ void k_set_status(DevLU *Ds, const int *st, int n)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n && st[b] >= 0) Ds[b].s->status = st[b];
}
__global__ void k_reset_scalars(DevLU *Ds, const int *which, int n)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n && which[b]) { // (word by word through the pointer: a by-value Scalars built in the thread lived in scratch)
        Scalars *s = Ds[b].s;
        static_assert(sizeof(Scalars) % sizeof(unsigned long long) == 0, "Scalars is a whole number of 8-byte words");
        unsigned long long *w = (unsigned long long *)s;
        for (unsigned i = 0; i < sizeof(Scalars) / sizeof(unsigned long long); i++) w[i] = 0ull;
        s->status = ST_RUNNING;
        s->pivot_row = s->pivot_col = -1;
    }
}

// the descriptors of a batch go back to the handles' own slots (solve_dense, get_factors use those): one launch
__global__ void k_scatter_desc(const DevLU *sD, const FinishOut *sO, DevLU *const *dD, FinishOut *const *dO, int n)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < n) {
        *dD[b] = sD[b];
        *dO[b] = sO[b];
    }
}

struct BatchCtx {
    std::vector<blu_hip *> hs;
    int n = 0;
    DevLU *dD = nullptr;
    FinishOut *dO = nullptr;
    Scalars *dS = nullptr;
    int *dSt = nullptr;
    std::vector<int> st;     // status to write before the next launch (-1 = leave)
    std::vector<int> result; // API status per handle; kPending while in flight
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int block_pivot = 1024, block_other = 1024, block_stats = 256;
    bool owns_arrays = false;
    double t_pivot = 0, t_total = 0;
    double t_phase[6] = {0, 0, 0, 0, 0, 0}; // device time of k_prep, k_setup, k_finish, statistics; inside those: k_rows_grid, k_stats_tail (HIP events)
    hipEvent_t pe2[2] = {nullptr, nullptr};
    hipEvent_t pe[2] = {nullptr, nullptr};
    int relaunches = 0;
    int narrow_launches = 0; // launches of k_pivot_loop with 32-bit addressing (statistic 130)
    char *fill_scr = nullptr; // k_finish of a batch: scratch of fill_scr_bytes per workgroup for its fill through buckets (k_bucket.h)
    long long fill_scr_bytes = 0;
    void phase_begin() { (void)hipEventRecord(pe[0], stream); }
    void phase_end(int which) // call after the stream has been synchronized past the launch
    {
        (void)hipEventRecord(pe[1], stream);
        (void)hipEventSynchronize(pe[1]);
        float ms = 0;
        if (hipEventElapsedTime(&ms, pe[0], pe[1]) == hipSuccess) t_phase[which] += 1e-3 * ms;
    }
};

// A single factorize runs its O(nnz) phases chip-wide: cooperative launch of `grid_blocks` workgroups on the one
// matrix (GridScope, blu_dev.h).  Returns false if the launch was refused; the caller then takes the
// one-workgroup kernel (same body, BlockScope).
static bool launch_grid(BatchCtx &B, const void *fn, bool with_out)
{
    blu_hip *h = B.hs[0];
    if (B.n != 1 || h->grid_blocks <= 1) return false;
    if (hipMemsetAsync(h->gw, 0, sizeof(GridWs), B.stream) != hipSuccess) return false;
    void *a0 = (void *)B.dD, *a1 = (void *)B.dO, *a2 = (void *)h->gw;
    void *args3[3] = {&a0, &a1, &a2};
    void *args2[2] = {&a0, &a2};
    const hipError_t e = hipLaunchCooperativeKernel(fn, dim3(h->grid_blocks), dim3(1024), with_out ? args3 : args2, 0, B.stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        h->grid_blocks = 1; // refused once: stay with one workgroup
        return false;
    }
    return true;
}

static void batch_release(BatchCtx &B)
{
    // descriptors go back to the handles' own slots (solve_dense, get_factors): the batch slots are current (every
    // host-side change was uploaded to them), so one scatter launch does it for a batch
    bool scattered = false;
    if (B.n > 1 && B.owns_arrays && B.dD && B.dO) {
        std::vector<DevLU *> pd(B.n);
        std::vector<FinishOut *> po(B.n);
        for (int k = 0; k < B.n; k++) {
            pd[k] = B.hs[k]->dD;
            po[k] = B.hs[k]->dO;
        }
        DevLU **dpd = nullptr;
        FinishOut **dpo = nullptr;
        if (hipMalloc(&dpd, sizeof(DevLU *) * B.n) == hipSuccess && hipMalloc(&dpo, sizeof(FinishOut *) * B.n) == hipSuccess &&
            hipMemcpy(dpd, pd.data(), sizeof(DevLU *) * B.n, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dpo, po.data(), sizeof(FinishOut *) * B.n, hipMemcpyHostToDevice) == hipSuccess) {
            hipLaunchKernelGGL(k_scatter_desc, dim3((B.n + 63) / 64), dim3(64), 0, B.stream, B.dD, B.dO, dpd, dpo, B.n);
            scattered = hipStreamSynchronize(B.stream) == hipSuccess;
        }
        if (dpd) (void)hipFree(dpd);
        if (dpo) (void)hipFree(dpo);
    }
    for (int k = 0; k < B.n; k++) {
        blu_hip *h = B.hs[k];
        h->dslot = h->dD;
        h->oslot = h->dO;
        if (!scattered) {
            (void)hipMemcpy(h->dD, &h->D, sizeof(DevLU), hipMemcpyHostToDevice);
            (void)hipMemcpy(h->dO, &h->O, sizeof(FinishOut), hipMemcpyHostToDevice);
        }
        h->t_pivot = B.t_pivot;
        h->t_total = B.t_total;
        for (int q = 0; q < 6; q++) h->t_phase[q] = B.t_phase[q];
        h->relaunches = B.relaunches;
        h->narrow_launches = B.narrow_launches;
    }
    if (B.owns_arrays) {
        dfree(B.dD);
        dfree(B.dO);
    }
    dfree(B.dS);
    dfree(B.dSt);
    if (B.fill_scr) (void)hipFree(B.fill_scr);
    B.fill_scr = nullptr;
    for (int k = 0; k < 2; k++)
        if (B.pe[k]) (void)hipEventDestroy(B.pe[k]);
    for (int k = 0; k < 2; k++)
        if (B.pe2[k]) (void)hipEventDestroy(B.pe2[k]);
    if (B.n > 1) {
        if (B.stream) (void)hipStreamDestroy(B.stream);
        for (int k = 0; k < 4; k++)
            if (B.ev[k]) (void)hipEventDestroy(B.ev[k]);
    }
}

static bool batch_init(BatchCtx &B, blu_hip **hs, int n)
{
    B.n = n;
    B.hs.assign(hs, hs + n);
    B.st.assign(n, -1);
    B.result.assign(n, kPending);
    blu_hip *h0 = hs[0];
    B.block_pivot = h0->block_threads;
    if (n == 1) {
        B.dD = h0->dD;
        B.dO = h0->dO;
        B.stream = h0->stream;
        for (int k = 0; k < 4; k++) B.ev[k] = h0->ev[k];
    } else {
        B.owns_arrays = true;
        if (!dalloc(h0, &B.dD, n) || !dalloc(h0, &B.dO, n)) return false;
        if (!hip_ok(h0, hipStreamCreate(&B.stream), "hipStreamCreate")) return false;
        for (int k = 0; k < 4; k++)
            if (!hip_ok(h0, hipEventCreate(&B.ev[k]), "hipEventCreate")) return false;
        B.block_other = h0->batch_block_other;
        B.block_stats = h0->batch_block_stats;
    }
    if (!dalloc(h0, &B.dS, n) || !dalloc(h0, &B.dSt, n)) return false;
    for (int k = 0; k < 2; k++)
        if (!hip_ok(h0, hipEventCreate(&B.pe[k]), "hipEventCreate") || !hip_ok(h0, hipEventCreate(&B.pe2[k]), "hipEventCreate")) return false;
    for (int k = 0; k < n; k++) {
        hs[k]->dslot = B.dD + k;
        hs[k]->oslot = B.dO + k;
    }
    return true;
}

static bool batch_gather(BatchCtx &B)
{
    blu_hip *h0 = B.hs[0];
    hipLaunchKernelGGL(k_gather_scalars, dim3((B.n + 63) / 64), dim3(64), 0, B.stream, B.dD, B.dS, B.n);
    if (!hip_ok(h0, hipStreamSynchronize(B.stream), "kernel")) return false;
    std::vector<Scalars> S(B.n);
    if (!hip_ok(h0, hipMemcpy(S.data(), B.dS, sizeof(Scalars) * B.n, hipMemcpyDeviceToHost), "d2h scalars")) return false;
    for (int k = 0; k < B.n; k++) B.hs[k]->hs = S[k];
    return true;
}
static bool batch_apply_status(BatchCtx &B)
{
    blu_hip *h0 = B.hs[0];
    bool any = false;
    for (int k = 0; k < B.n; k++) any = any || B.st[k] >= 0;
    if (!any) return true;
    if (!hip_ok(h0, hipMemcpy(B.dSt, B.st.data(), sizeof(int) * B.n, hipMemcpyHostToDevice), "h2d status")) return false;
    hipLaunchKernelGGL(k_set_status, dim3((B.n + 63) / 64), dim3(64), 0, B.stream, B.dD, B.dSt, B.n);
    std::fill(B.st.begin(), B.st.end(), -1);
    return hip_ok(h0, hipStreamSynchronize(B.stream), "k_set_status");
}
static bool batch_reset_scalars(BatchCtx &B, const std::vector<int> &which)
{
    blu_hip *h0 = B.hs[0];
    if (!hip_ok(h0, hipMemcpy(B.dSt, which.data(), sizeof(int) * B.n, hipMemcpyHostToDevice), "h2d which")) return false;
    hipLaunchKernelGGL(k_reset_scalars, dim3((B.n + 63) / 64), dim3(64), 0, B.stream, B.dD, B.dSt, B.n);
    return hip_ok(h0, hipStreamSynchronize(B.stream), "k_reset_scalars");
}
static void fail_handle(BatchCtx &B, int k, int code, const char *what)
{
    blu_hip *h = B.hs[k];
    if (h->err.empty()) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: device status %d at kernel source line %d", what, h->hs.status, h->hs.err_line);
        h->err = buf;
    }
    B.result[k] = code;
}
static int oom_or_device(blu_hip *h)
{
    return h->err.find("hipMalloc") != std::string::npos ? BLU_ERROR_OUT_OF_MEMORY : BLU_ERROR_DEVICE;
}
// lu.reset() (lu.rs:329-359), the first thing every factorize call does (factorize.rs:44-47) whatever it returns: the
// statistics of the last factorization and of its updates read as a fresh LU's until this factorize succeeds.  (The
// device diagnostics of the last call stay: exit status and source line, statistics 57 / 58; fill paths, 119.)
static void reset_lu(blu_hip *h)
{
    const int status = h->hs.status, err_line = h->hs.err_line, fill_paths = h->hs.fill_paths;
    memset(&h->hs, 0, sizeof(Scalars));
    h->hs.status = status;
    h->hs.err_line = err_line;
    h->hs.fill_paths = fill_paths;
    h->nupdate = -1;               // invalidate the factorization (lu.rs:331)
    h->update_cost_denom = 1.0;    // (lu.rs:340)
    h->sp_l_flops = h->sp_u_flops = 0;
    h->upd_for_nfact = -1;         // nforrest, pivot_error, r_nz, r_flops, max_eta, update_cost_numer: 0 (lu.rs:332-346)
    h->lt_for_nfact = h->rows_for_nfact = -1; // row-wise copies of the old factors: never to be used again
}
// lu.update_cost_denom of a factorization that succeeded (factorize.rs:160-166)
static void set_factor_cost(blu_hip *h)
{
    const Scalars &s = h->hs;
    h->update_cost_denom = 250.0 * (0.04 * (double)h->m + 0.07 * (double)s.matrix_nz + 0.20 * (double)s.bump_nz +
                                    0.20 * (double)s.nsearch_pivot + 0.008 * (double)s.factor_flops);
}

// ---- phase 3+4: pivot loop (relaunched until every handle is done / stopped / failed), then read-out
// Workgroups of the O(nnz) kernels of a batch (k_prep, k_setup, k_finish: one workgroup works on one matrix at a time and
// takes the next when it is done).  MEASURED (C3 x 1536, 256-thread workgroups): these kernels get FASTER with fewer
// matrices in flight -- one per CU instead of 3-7: prep 0.241 -> 0.207 s, setup 0.218 -> 0.165 s, finish 0.53 -> 0.47 s
// (and slower with more: finish 0.645 s at 8 per CU).  Every matrix is ~150 MB of its own, touched by scattered
// 8-byte accesses: what is shared -- L2, the translation caches -- holds a few hundred such streams, not 1536.
// (k_stats is the opposite case, one dependent chain per wave: 0.75 s at 6 per CU, 1.6 s at one.)
static int batch_grid(const blu_hip *h0, int n)
{
    const int g = h0->batch_grid > 0 ? h0->batch_grid : h0->num_cus;
    return n < g ? n : g;
}

// dense work columns pivot_any needs in D.gwork: one per wave of the pivot kernel batch_pivot_and_finish will launch
// (k_pivot_loop: one per wave of its workgroup; the wave kernels: 1 or 2), and never fewer than the 9 columns of the
// statistics
static int pivot_work_columns(const BatchCtx &B)
{
    const bool workgroup_kernel = B.hs[0]->pivot_kernel == 0 && B.n == 1; // k_pivot_loop
    return std::max(9, workgroup_kernel ? B.block_pivot / 64 : 2);
}

static bool batch_pivot_and_finish(BatchCtx &B)
{
    blu_hip *h0 = B.hs[0];
    const int n = B.n;
    blu_hip *rows_built_for = nullptr; // the handle whose row-wise copies (k_rows_grid) were rebuilt by this call
    for (int iter = 0; iter < 400; iter++) {
        (void)hipEventRecord(B.ev[2], B.stream);
        // a batch: one wave per basis is the shape for as many bases as the registers allow (16 per CU); while the card holds
        // fewer than half of that -- bases of the 100k size: HBM capacity -- each gets two waves
        int which, regs = 4;
        if (h0->pivot_kernel == 3 || (h0->pivot_kernel == 0 && n > 1 && n <= h0->wave2_max)) {
            which = 3; // (every workgroup resident with the registers of three waves per SIMD: that variant)
            if (n <= h0->wave2_r3_max) {
                regs = 3;
                hipLaunchKernelGGL(k_pivot_loop_wave2_r3, dim3(n), dim3(128), 0, B.stream, B.dD, (int)h0->stop_at);
            } else {
                hipLaunchKernelGGL(k_pivot_loop_wave2, dim3(n), dim3(128), 0, B.stream, B.dD, (int)h0->stop_at);
            }
        } else if (h0->pivot_kernel == 1 || n > 1) {
            which = 1;
            if (n <= h0->wave_r3_max) {
                regs = 3;
                hipLaunchKernelGGL(k_pivot_loop_wave_r3, dim3(n), dim3(64), 0, B.stream, B.dD, (int)h0->stop_at);
            } else {
                hipLaunchKernelGGL(k_pivot_loop_wave, dim3(n), dim3(64), 0, B.stream, B.dD, (int)h0->stop_at);
            }
        } else {
            which = 0; // (one basis)
            h0->last_addr_wide = addr32_fits(h0) ? 0 : 1;
            if (h0->last_addr_wide) {
                hipLaunchKernelGGL(k_pivot_loop_w64, dim3(n), dim3(B.block_pivot), 0, B.stream, B.dD, (int)h0->stop_at);
            } else {
#ifdef BLU_EMU_BUILD
                g_emu_addr32_limit = h0->addr32_limit; // (what the asserting accessor checks)
#endif
                B.narrow_launches++;
                hipLaunchKernelGGL(k_pivot_loop, dim3(n), dim3(B.block_pivot), 0, B.stream, B.dD, (int)h0->stop_at);
            }
        }
        for (int k = 0; k < n; k++) B.hs[k]->last_pivot_kernel = which, B.hs[k]->last_pivot_regs = regs;
        (void)hipEventRecord(B.ev[3], B.stream);
        if (!batch_gather(B)) return false;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, B.ev[2], B.ev[3]);
        B.t_pivot += 1e-3 * ms;
        B.relaunches++;
        bool again = false;
        std::vector<int> creq(n, -1), cneed(n, 0); // arena compactions asked for: all of them in one launch below
        for (int k = 0; k < n; k++) {
            if (B.result[k] != kPending) continue;
            blu_hip *h = B.hs[k];
            const int st = h->hs.status;
            if (st == ST_DONE) continue;
            if (st == ST_STOPPED) {
                B.result[k] = BLU_STOPPED_STATUS;
                continue;
            }
            bool ok = true;
            if (st == ST_NEED_L) ok = grow_l(h, h->hs.need) && upload_desc(h);
            else if (st == ST_NEED_U) ok = grow_u(h, h->hs.need) && upload_desc(h);
            else if (st == ST_NEED_CW || st == ST_NEED_RW) {
                creq[k] = st == ST_NEED_RW ? 1 : 0;
                cneed[k] = h->hs.need;
            } else {
                fail_handle(B, k, BLU_ERROR_DEVICE, "pivot loop failed");
                continue;
            }
            if (!ok) {
                B.result[k] = oom_or_device(h);
                continue;
            }
            B.st[k] = ST_RUNNING;
            again = true;
        }
        {
            std::vector<char> cok;
            (void)compact_files(B.hs.data(), n, B.dD, B.stream, creq, cneed, cok);
            for (int k = 0; k < n; k++)
                if (creq[k] >= 0 && !cok[k]) {
                    B.result[k] = oom_or_device(B.hs[k]);
                    B.st[k] = -1;
                }
        }
        if (!again) break;
        if (!batch_apply_status(B)) return false;
        if (iter == 399) {
            for (int k = 0; k < n; k++)
                if (B.result[k] == kPending && B.hs[k]->hs.status != ST_DONE) fail_handle(B, k, BLU_ERROR_DEVICE, "too many relaunches");
        }
    }
    // build_factors + get_factors read-out on the device
    bool any = false;
    for (int k = 0; k < n; k++) {
        blu_hip *h = B.hs[k];
        if (B.result[k] != kPending || h->hs.status != ST_DONE) continue;
        if (!ensure_out(h, (int64_t)h->hs.lused + h->m, (int64_t)h->hs.uused + h->m, false)) {
            B.result[k] = BLU_ERROR_OUT_OF_MEMORY;
            B.st[k] = ST_ERROR;
            continue;
        }
        any = true;
    }
    { // the read-out descriptors of the whole batch in one copy
        std::vector<FinishOut> stage(n);
        for (int k = 0; k < n; k++) stage[k] = B.hs[k]->O;
        if (!hip_ok(h0, hipMemcpy(B.dO, stage.data(), sizeof(FinishOut) * n, hipMemcpyHostToDevice), "h2d read-out descriptors")) return false;
    }
    if (!batch_apply_status(B)) return false;
    if (any) {
        B.phase_begin();
        if (!launch_grid(B, (const void *)k_finish_grid, true)) {
            const int fb = n == 1 ? 1024 : B.block_other;
            const int win = (h0->lds_window_mode == 2 || (h0->lds_window_mode == 1 && n >= h0->num_cus)) ? h0->lds_window : 0;
            // the fill through buckets (k_bucket.h) keeps 20 bytes per entry of the stage-ordered U while a workgroup is on a
            // matrix: one scratch per WORKGROUP (not per basis: at C3 size 29 MB each, 7.4 GB for the 256 of a launch), for the
            // duration of this call; without it (no window, no memory) the fill takes its window sweeps
            if (win >= 16384 && fb <= 512 && !B.fill_scr) {
                long long per = 0;
                for (int k = 0; k < n; k++)
                    if (B.result[k] == kPending && B.hs[k]->hs.status == ST_DONE) per = std::max(per, 20LL * (((long long)B.hs[k]->hs.uused + 3) & ~3LL));
                per = (per + 255) & ~255LL;
                size_t free_b = 0, total_b = 0;
                if (per > 0 && hipMemGetInfo(&free_b, &total_b) == hipSuccess && (size_t)(per * batch_grid(h0, n)) + (1ull << 30) <= free_b &&
                    hipMalloc((void **)&B.fill_scr, (size_t)(per * batch_grid(h0, n))) == hipSuccess)
                    B.fill_scr_bytes = per;
                else
                    B.fill_scr = nullptr, (void)hipGetLastError();
            }
            if (fb <= 256) hipLaunchKernelGGL(k_finish<256>, dim3(batch_grid(h0, n)), dim3(fb), win, B.stream, B.dD, B.dO, n, win, B.fill_scr, B.fill_scr_bytes);
            else if (fb <= 512) hipLaunchKernelGGL(k_finish<512>, dim3(batch_grid(h0, n)), dim3(fb), win, B.stream, B.dD, B.dO, n, win, B.fill_scr, B.fill_scr_bytes);
            else hipLaunchKernelGGL(k_finish<1024>, dim3(batch_grid(h0, n)), dim3(fb), 0, B.stream, B.dD, B.dO, n, 0, (char *)nullptr, 0LL);
        }
        B.phase_end(2);
        B.phase_begin();
        // condest(L), condest(U), residual_test (factorize.rs:121-147)
        bool want_stats = false; // per handle (DevLU::skip_stats); the launch is skipped when nobody wants them
        for (int k = 0; k < n; k++) want_stats = want_stats || !B.hs[k]->skip_stats;
        // A single matrix: row-wise copies chip-wide, the four sweep chains on the chain pipeline (k_chain.h), then
        // the norms / residuals; a batch (or a device that refuses the launches): one workgroup per matrix.
        bool chained = false, continue_chained = true;
        blu_hip *h0 = B.hs[0];
        if (want_stats && n == 1 && h0->chain_ok && h0->grid_blocks > 1 &&
            ensure_rows_ws(h0, (int64_t)h0->hs.lused, (int64_t)h0->hs.uused) == BLU_OK) {
            (void)hipEventRecord(B.pe2[0], B.stream);
            if (launch_rows(h0, B.dD, B.stream)) {
                (void)hipEventRecord(B.pe2[1], B.stream);
                // (as after every cooperative launch of this file: the host waits for it before the next kernel goes to
                // the stream -- the chains read what k_rows_grid writes)
                (void)hipEventSynchronize(B.pe2[1]);
                rows_built_for = h0; // (lt_for_nfact / rows_for_nfact are set below, once the factorization stands)
                int *defect = &h0->gw->ctr[6];
                (void)hipMemsetAsync(defect, 0, sizeof(int), B.stream);
#ifdef BLU_STATS_DEBUG // diagnostic build: BLU_CHAIN_DEBUG = 1 stops after k_rows_grid, 2 after the chains (tools/stats_dbg.py)
                const char *dbg = getenv("BLU_CHAIN_DEBUG");
                const int dbg_level = dbg ? atoi(dbg) : 2;
#else
                const int dbg_level = 3;
#endif
                if (dbg_level >= 2)
                    hipLaunchKernelGGL(k_stats_chains, dim3(4), dim3(CHAIN_THREADS), sizeof(ChainLds), B.stream, B.dD, B.dO, rows_ws_of(h0), defect);
                hipEvent_t t0 = B.ev[2], t1 = B.ev[3];
                (void)hipEventRecord(t0, B.stream);
                int chain_defect = 0;
                if (dbg_level >= 3) {
                    (void)hipMemcpy(&chain_defect, defect, sizeof(int), hipMemcpyDeviceToHost); // (waits for the chains)
                    if (chain_defect == 0) {
                        hipLaunchKernelGGL(k_stats_tail_a, dim3(TAIL_BLOCKS), dim3(1024), 0, B.stream, B.dD, B.dO, h0->gw);
                        hipLaunchKernelGGL(k_stats_tail_b, dim3(1), dim3(1024), 0, B.stream, B.dD, B.dO, h0->gw);
                        // the work vectors of the chains and of the tail back to the all-zero state pivot_any expects
                        (void)hipMemsetAsync(h0->D.gwork, 0, 7 * ((size_t)h0->m + 1) * sizeof(double), B.stream);
                    }
                }
                (void)hipEventRecord(t1, B.stream);
                (void)hipEventSynchronize(t1);
                float ms = 0;
                if (hipEventElapsedTime(&ms, B.pe2[0], B.pe2[1]) == hipSuccess) B.t_phase[4] += 1e-3 * ms;
                if (hipEventElapsedTime(&ms, t0, t1) == hipSuccess) B.t_phase[5] += 1e-3 * ms;
                if (chain_defect) { // a bounded wait of the chain pipeline gave up: its work vectors are not to be used
                    h0->chain_defects++;
                    (void)hipMemset(h0->D.gwork, 0, (size_t)h0->gwork_cols * ((size_t)h0->m + 1) * sizeof(double)); // the all-zero state k_stats expects
                    continue_chained = false;
                }
                chained = continue_chained;
            }
        }
        if (want_stats && !chained) {
            if (n == 1 || B.block_stats > 256) {
                hipLaunchKernelGGL(k_stats, dim3(n), dim3(n == 1 ? 1024 : B.block_stats), 0, B.stream, B.dD, B.dO, 1);
            } else { // a batch: the chains at full residency, then the O(nnz) tail one workgroup per CU
                hipLaunchKernelGGL(k_stats, dim3(n), dim3(B.block_stats), 0, B.stream, B.dD, B.dO, 0);
                if (B.block_other == 512) hipLaunchKernelGGL(k_stats_tail<512>, dim3(batch_grid(h0, n)), dim3(512), 0, B.stream, B.dD, B.dO, n);
                else hipLaunchKernelGGL(k_stats_tail<256>, dim3(batch_grid(h0, n)), dim3(256), 0, B.stream, B.dD, B.dO, n);
            }
        }
        B.phase_end(3);
        if (!batch_gather(B)) return false;
    }
    (void)hipEventRecord(B.ev[1], B.stream);
    (void)hipEventSynchronize(B.ev[1]);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, B.ev[0], B.ev[1]);
    B.t_total = 1e-3 * ms;
    for (int k = 0; k < n; k++) {
        blu_hip *h = B.hs[k];
        if (B.result[k] != kPending) continue;
        if (h->hs.status != ST_DONE) {
            fail_handle(B, k, BLU_ERROR_DEVICE, "finish failed");
            continue;
        }
        h->nupdate = 0; // factorization successfully finished (factorize.rs:114-119)
        h->nfactorize++;
        set_factor_cost(h);
        if (rows_built_for == h) h->lt_for_nfact = h->rows_for_nfact = h->nfactorize; // the row-wise copies belong to THIS factorization
        B.result[k] = h->hs.rank < h->m ? BLU_WARNING_SINGULAR_MATRIX : BLU_OK;
    }
    return true;
}

// ---- phases 1+2: singletons, setup_bump; then the rest
static bool batch_factorize(BatchCtx &B)
{
    blu_hip *h0 = B.hs[0];
    const int n = B.n;
    (void)hipEventRecord(B.ev[0], B.stream);
    { // every slot must be valid (kernels index all of them): all descriptors staged on the host, ONE copy
        std::vector<DevLU> stage(n);
        const int gcols = pivot_work_columns(B);
        for (int k = 0; k < n; k++) {
            if (!ensure_gwork(B.hs[k], gcols)) return false;
            fill_desc(B.hs[k]);
            stage[k] = B.hs[k]->D;
        }
        if (!hip_ok(h0, hipMemcpy(B.dD, stage.data(), sizeof(DevLU) * n, hipMemcpyHostToDevice), "h2d descriptors")) return false;
    }
    {
        std::vector<int> which(n);
        for (int k = 0; k < n; k++) which[k] = B.result[k] == kPending;
        if (!batch_reset_scalars(B, which)) return false;
        for (int k = 0; k < n; k++) B.st[k] = which[k] ? -1 : ST_HOLD; // handles with nothing to do: skip in every launch
        if (!batch_apply_status(B)) return false;
    }
    // singletons (k_prep): re-run for the handles whose storage was too small
    for (int attempt = 0; attempt < 64; attempt++) {
        B.phase_begin();
        if (!launch_grid(B, (const void *)k_prep_grid, false)) {
            // (the LDS window of prep_body: only where a workgroup has the CU to itself -- the grid of a large batch)
            const int win = (h0->lds_window_mode == 2 || (h0->lds_window_mode == 1 && n >= h0->num_cus)) ? h0->lds_window : 0;
            if (B.block_other <= 256) hipLaunchKernelGGL(k_prep<256>, dim3(batch_grid(h0, n)), dim3(B.block_other), win, B.stream, B.dD, n, win);
            else if (B.block_other <= 512) hipLaunchKernelGGL(k_prep<512>, dim3(batch_grid(h0, n)), dim3(B.block_other), win, B.stream, B.dD, n, win);
            else hipLaunchKernelGGL(k_prep<1024>, dim3(batch_grid(h0, n)), dim3(B.block_other), 0, B.stream, B.dD, n, 0);
        }
        B.phase_end(0);
        if (!batch_gather(B)) return false;
        std::vector<int> redo(n, 0);
        bool again = false;
        for (int k = 0; k < n; k++) {
            if (B.result[k] != kPending) continue;
            blu_hip *h = B.hs[k];
            DevLU &D = h->D;
            const int st = h->hs.status;
            if (st == ST_RUNNING) {
                B.st[k] = ST_HOLD;
                continue;
            }
            if (st == ST_HOLD) continue;
            if (st == ST_INVALID_ARG) {
                B.result[k] = BLU_ERROR_INVALID_ARGUMENT;
                continue;
            }
            bool ok = true;
            if (st == ST_NEED_CW) { // packed copies of B too small
                const int64_t nn = std::min<int64_t>((int64_t)h->hs.need + 64, kIntMax);
                dfree(D.bc_idx); dfree(D.bc_val); dfree(D.bt_idx); dfree(D.bt_val);
                ok = dalloc(h, &D.bc_idx, nn) && dalloc(h, &D.bc_val, nn) && dalloc(h, &D.bt_idx, nn) && dalloc(h, &D.bt_val, nn);
                D.nzcap = (int)nn;
            } else if (st == ST_NEED_L || st == ST_NEED_U) {
                h->hs.lused = h->hs.uused = 0;
                ok = st == ST_NEED_L ? grow_l(h, h->hs.need) : grow_u(h, h->hs.need);
            } else {
                fail_handle(B, k, BLU_ERROR_DEVICE, "prep failed");
                continue;
            }
            if (!ok || !upload_desc(h)) {
                B.result[k] = oom_or_device(h);
                continue;
            }
            redo[k] = 1;
            again = true;
        }
        if (!batch_apply_status(B)) return false;
        if (!again) break;
        if (!batch_reset_scalars(B, redo)) return false;
    }
    for (int k = 0; k < n; k++) B.st[k] = (B.result[k] == kPending) ? ST_RUNNING : -1;
    if (!batch_apply_status(B)) return false;
    // setup_bump (k_setup); arenas are grown until the bump fits (setup_bump.rs:105-113)
    for (int attempt = 0; attempt < 64; attempt++) {
        B.phase_begin();
        if (!launch_grid(B, (const void *)k_setup_grid, false)) {
            // (the flag bitmaps of setup_body need 1 bit per line: 16 KB of LDS cover 130 000 lines, and any batch may have them)
            int mmax = 0;
            for (int k = 0; k < n; k++) mmax = std::max(mmax, (int)B.hs[k]->m);
            const int win = h0->lds_window_mode == 0 ? 0 : std::min(h0->lds_window, std::max(64, ((mmax + 64 + 31) / 32 * 4 + 15) & ~15));
            if (B.block_other <= 512) hipLaunchKernelGGL(k_setup<512>, dim3(batch_grid(h0, n)), dim3(B.block_other), win, B.stream, B.dD, n, win);
            else hipLaunchKernelGGL(k_setup<1024>, dim3(batch_grid(h0, n)), dim3(B.block_other), win, B.stream, B.dD, n, win);
        }
        B.phase_end(1);
        if (!batch_gather(B)) return false;
        bool again = false;
        for (int k = 0; k < n; k++) {
            if (B.result[k] != kPending) continue;
            blu_hip *h = B.hs[k];
            DevLU &D = h->D;
            const int st = h->hs.status;
            if (st == ST_RUNNING) {
                B.st[k] = ST_HOLD;
                continue;
            }
            if (st == ST_HOLD) continue;
            if (st == ST_NEED_CW || st == ST_NEED_RW) {
                const int64_t nn = grown(h, 2 * (int64_t)h->hs.need, 0);
                bool ok;
                if (st == ST_NEED_CW) {
                    dfree(D.cidx); dfree(D.cval);
                    ok = dalloc(h, &D.cidx, nn) && dalloc(h, &D.cval, nn);
                    D.carena_cap = (int)nn;
                } else {
                    dfree(D.ridx);
                    ok = dalloc(h, &D.ridx, nn);
                    D.rarena_cap = (int)nn;
                }
                if (!ok || !upload_desc(h)) {
                    B.result[k] = oom_or_device(h);
                    continue;
                }
                B.st[k] = ST_RUNNING;
                again = true;
                continue;
            }
            fail_handle(B, k, BLU_ERROR_DEVICE, "setup failed");
        }
        if (!batch_apply_status(B)) return false;
        if (!again) break;
    }
    for (int k = 0; k < n; k++) B.st[k] = (B.result[k] == kPending) ? ST_RUNNING : -1;
    if (!batch_apply_status(B)) return false;
    (void)h0;
    return batch_pivot_and_finish(B);
}

// common entry: inputs already on the device
static int factorize_batch_impl(blu_hip **hs, int n, const uint64_t *const *d_b_begin, const uint64_t *const *d_b_end,
                                const uint64_t *const *d_b_i, const double *const *d_b_x, const uint64_t *b_i_len, int *status)
{
    if (n <= 0) return BLU_OK;
    blu_hip *h0 = hs[0];
    // every early return reports itself in status[] too (refuse_all): a caller that looks at status[] alone must not
    // read "OK" for handles that were never worked on.  No member is NULL: both callers have refused that.
    // The factors every handle holds are invalid from here on, whatever happens next
    for (int k = 0; k < n; k++) reset_lu(hs[k]);
    if (hipSetDevice(h0->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);
    if (const int st = batch_handles_refusal(hs, n); st != BLU_OK) return refuse_all(status, n, st); // (twice = two workgroups on one DevLU)
    for (int k = 0; k < n; k++)
        if (b_i_len[k] > (uint64_t)kIntMax) return refuse_all(status, n, BLU_ERROR_INVALID_ARGUMENT); // 32-bit device indices
    BatchCtx B;
    if (!batch_init(B, hs, n)) {
        batch_release(B);
        return refuse_all(status, n, oom_or_device(h0));
    }
    for (int k = 0; k < n; k++) {
        blu_hip *h = hs[k];
        DevLU &D = h->D;
        h->err.clear();
        D.b_begin = (const unsigned long long *)d_b_begin[k];
        D.b_end = (const unsigned long long *)d_b_end[k];
        D.b_i = (const unsigned long long *)d_b_i[k];
        D.b_x = d_b_x[k];
        D.b_i_len = (long long)b_i_len[k];
        if (h->m == 0) { // nothing to do
            memset(&h->hs, 0, sizeof(Scalars));
            h->nupdate = 0;
            h->nfactorize++;
            set_factor_cost(h);
            B.result[k] = BLU_OK;
        }
    }
    bool any = false;
    for (int k = 0; k < n; k++) any = any || B.result[k] == kPending;
    bool ok = true;
    if (any) ok = batch_factorize(B);
    for (int k = 0; k < n; k++) // (kPending is negative too)
        if (B.result[k] < 0) reset_lu(hs[k]); // what the kernels counted before they refused B is not the reference's: it counts nothing (singletons.rs:119-259)
    int worst = batch_return(B.result, status);
    batch_release(B);
    if (!ok && worst >= 0) worst = BLU_ERROR_DEVICE;
    return worst;
}

static int factorize_device_impl(blu_hip *h, const uint64_t *d_b_begin, const uint64_t *d_b_end,
                                 const uint64_t *d_b_i, const double *d_b_x, uint64_t b_i_len)
{
    int st = BLU_ERROR_DEVICE;
    const int r = factorize_batch_impl(&h, 1, &d_b_begin, &d_b_end, &d_b_i, &d_b_x, &b_i_len, &st);
    (void)r;
    return st;
}

// continue a single stopped factorization (debug stepping)
static int continue_pivot_single(blu_hip *h)
{
    BatchCtx B;
    if (!batch_init(B, &h, 1)) {
        batch_release(B);
        return oom_or_device(h);
    }
    (void)hipEventRecord(B.ev[0], B.stream);
    const bool ok = h->gwork_cols >= pivot_work_columns(B) && batch_pivot_and_finish(B); // (a stopped factorize was started with them)
    int r = B.result[0];
    batch_release(B);
    if (!ok || r == kPending) return BLU_ERROR_DEVICE;
    return r;
}

extern "C" int blu_hip_factorize_device(blu_hip *h, const uint64_t *d_b_begin, const uint64_t *d_b_end,
                                        const uint64_t *d_b_i, const double *d_b_x, uint64_t b_i_len)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (h->m > 0 && (!d_b_begin || !d_b_end || (b_i_len && (!d_b_i || !d_b_x)))) return BLU_ERROR_ARGUMENT_MISSING;
    return factorize_device_impl(h, d_b_begin, d_b_end, d_b_i, d_b_x, b_i_len);
}

// copies the caller's host arrays of one handle into its owned device buffers
static int upload_inputs(blu_hip *h, const uint64_t *b_begin, const uint64_t *b_end, const uint64_t *b_i, const double *b_x,
                         uint64_t b_i_len)
{
    const size_t M = (size_t)h->m, NZ = (size_t)b_i_len;
    if ((int64_t)M > h->ob_mcap) {
        dfree(h->ob_begin); dfree(h->ob_end);
        if (!dalloc(h, &h->ob_begin, M) || !dalloc(h, &h->ob_end, M)) return BLU_ERROR_OUT_OF_MEMORY;
        h->ob_mcap = (int64_t)M;
    }
    if ((int64_t)NZ > h->ob_nzcap) {
        dfree(h->ob_i); dfree(h->ob_x);
        if (!dalloc(h, &h->ob_i, NZ) || !dalloc(h, &h->ob_x, NZ)) return BLU_ERROR_OUT_OF_MEMORY;
        h->ob_nzcap = (int64_t)NZ;
    }
    bool ok = true;
    if (M) ok = ok && hip_ok(h, hipMemcpy(h->ob_begin, b_begin, M * 8, hipMemcpyHostToDevice), "h2d b_begin");
    if (M) ok = ok && hip_ok(h, hipMemcpy(h->ob_end, b_end, M * 8, hipMemcpyHostToDevice), "h2d b_end");
    if (NZ) ok = ok && hip_ok(h, hipMemcpy(h->ob_i, b_i, NZ * 8, hipMemcpyHostToDevice), "h2d b_i");
    if (NZ) ok = ok && hip_ok(h, hipMemcpy(h->ob_x, b_x, NZ * 8, hipMemcpyHostToDevice), "h2d b_x");
    return ok ? BLU_OK : BLU_ERROR_DEVICE;
}

// BLU::factorize with host arrays: copy B to the device, then as above
extern "C" int blu_hip_factorize(blu_hip *h, const uint64_t *b_begin, const uint64_t *b_end,
                                 const uint64_t *b_i, const double *b_x, uint64_t b_i_len)
{
    if (!h) return BLU_ERROR_ARGUMENT_MISSING;
    if (h->m > 0 && (!b_begin || !b_end || (b_i_len && (!b_i || !b_x)))) return BLU_ERROR_ARGUMENT_MISSING;
    if (hipSetDevice(h->device) != hipSuccess) return BLU_ERROR_DEVICE;
    const int up = upload_inputs(h, b_begin, b_end, b_i, b_x, b_i_len);
    if (up != BLU_OK) return up;
    return factorize_device_impl(h, (const uint64_t *)h->ob_begin, (const uint64_t *)h->ob_end,
                                 (const uint64_t *)h->ob_i, h->ob_x, b_i_len);
}

// Batch of independent factorizations on one device, one workgroup per handle, all kernels launched
// once for the whole batch (SURVEY.md 8b "batch extension", 8e).
extern "C" int blu_hip_factorize_batch(blu_hip **hs, int n, const uint64_t *const *b_begin,
                                       const uint64_t *const *b_end, const uint64_t *const *b_i,
                                       const double *const *b_x, const uint64_t *b_i_len,
                                       int inputs_on_device, int *status)
{
    if (!hs || n < 0 || (n > 0 && (!b_begin || !b_end || !b_i || !b_x || !b_i_len))) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (n == 0) return BLU_OK;
    for (int k = 0; k < n; k++)
        if (!hs[k]) return refuse_all(status, n, BLU_ERROR_ARGUMENT_MISSING);
    if (inputs_on_device) return factorize_batch_impl(hs, n, b_begin, b_end, b_i, b_x, b_i_len, status);
    if (hipSetDevice(hs[0]->device) != hipSuccess) return refuse_all(status, n, BLU_ERROR_DEVICE);
    std::vector<const uint64_t *> pb(n), pe(n), pi(n);
    std::vector<const double *> px(n);
    for (int k = 0; k < n; k++) {
        const int up = upload_inputs(hs[k], b_begin[k], b_end[k], b_i[k], b_x[k], b_i_len[k]);
        if (up != BLU_OK) {
            for (int q = 0; q < n; q++) hs[q]->nupdate = -1; // nothing was factorized: no handle keeps stale factors
            return refuse_all(status, n, up);
        }
        pb[k] = (const uint64_t *)hs[k]->ob_begin;
        pe[k] = (const uint64_t *)hs[k]->ob_end;
        pi[k] = (const uint64_t *)hs[k]->ob_i;
        px[k] = hs[k]->ob_x;
    }
    return factorize_batch_impl(hs, n, pb.data(), pe.data(), pi.data(), px.data(), b_i_len, status);
}
