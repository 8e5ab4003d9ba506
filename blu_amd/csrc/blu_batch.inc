// blu_batch.inc -- what the batched entries of the C ABI share on the host (included by blu_hip.hip ahead of
// blu_driver.inc): blu_hip_factorize_batch, _solve_dense_batch, _solve_for_update_batch, _update_batch,
// _solve_sparse_batch, _solve_sparse_multi, _copy_batch, _share_matrix, _tableau_row_batch and _price_batch.
//   * a call is refused as a whole (refuse_all: every status[k] carries the code) or answers per member: result[k]
//     starts as kPending, and batch_return writes status[] and picks the return value;
//   * the handle list of a call (batch_handles_refusal), the members a failed launch takes with it (fail_members) and
//     the ones that go on (keep_pending);
//   * a staging block (Stage): the per-member descriptors and records of one launch, laid out on the host, uploaded in
//     one copy; stage_alloc / stage_run are the round around it for the entries that allocate the block per call.

static const int kPending = -12345; // result[k] of a member that is still in flight

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// a refusal of the call as a whole: every status[k] carries the code, no member is worked on
static int refuse_all(int *status, int n, int code)
{
    if (status)
        for (int k = 0; k < n; k++) status[k] = code;
    return code;
}

// the same handle twice = two waves on one factorization
static bool has_duplicate(std::vector<blu_hip *> hs)
{
    std::sort(hs.begin(), hs.end());
    return std::adjacent_find(hs.begin(), hs.end()) != hs.end();
}

// the refusals every entry over a list of handles shares; BLU_OK = go on
static int batch_handles_refusal(blu_hip *const *hs, int n)
{
    for (int k = 0; k < n; k++)
        if (!hs[k]) return BLU_ERROR_ARGUMENT_MISSING;
    for (int k = 0; k < n; k++)
        if (hs[k]->device != hs[0]->device) return BLU_ERROR_INVALID_ARGUMENT;
    return has_duplicate(std::vector<blu_hip *>(hs, hs + n)) ? BLU_ERROR_INVALID_ARGUMENT : BLU_OK;
}

// status[] and the return value: the most negative error if any member failed, else the largest status; a member
// nothing answered for is a device error
static int batch_return(const std::vector<int> &result, int *status)
{
    int worst_err = 0, worst_pos = BLU_OK;
    for (size_t k = 0; k < result.size(); k++) {
        const int r = result[k] == kPending ? BLU_ERROR_DEVICE : result[k];
        if (status) status[k] = r;
        if (r < 0) worst_err = std::min(worst_err, r);
        else worst_pos = std::max(worst_pos, r);
    }
    return worst_err < 0 ? worst_err : worst_pos;
}

// a launch on h0's stream failed: its members get the code and h0's error text
static void fail_members(blu_hip *h0, blu_hip **hs, const std::vector<int> &list, std::vector<int> &result, int code)
{
    for (int k : list) {
        if (hs[k] != h0) hs[k]->err = h0->err;
        result[k] = code;
    }
}

// the members of `list` that are still in flight
static void keep_pending(std::vector<int> &list, const std::vector<int> &result)
{
    list.erase(std::remove_if(list.begin(), list.end(), [&](int k) { return result[k] != kPending; }), list.end());
}

// One staging block: typed arrays at 256-byte-aligned offsets, in the order they are added.  `bytes` is the block on
// the device; `host` its front, which is what gets uploaded (arrays behind it are written by the kernels alone).
template <class T> struct StageArr {
    size_t off;
};
struct Stage {
    size_t bytes = 0;
    std::vector<char> host;
    char *dev = nullptr; // where the block lies on the device (not owned)
    template <class T> StageArr<T> add(size_t count)
    {
        const StageArr<T> a{align_up(bytes)};
        bytes = a.off + count * sizeof(T);
        return a;
    }
    void host_front(size_t n) { host.assign(n, 0); }
    void restart() { bytes = 0; } // lay out the next block; host_front reuses the allocation of the one before
    template <class T> T *h(StageArr<T> a) { return (T *)(host.data() + a.off); }
    template <class T> T *d(StageArr<T> a) const { return (T *)(dev + a.off); }
};

// the block on the device, for one call: BLU_OK or BLU_ERROR_OUT_OF_MEMORY ...
static int stage_alloc(blu_hip *h0, Stage &S)
{
    if (hip_ok(h0, hipMalloc((void **)&S.dev, S.bytes), "hipMalloc")) return BLU_OK;
    (void)hipGetLastError();
    return BLU_ERROR_OUT_OF_MEMORY;
}
// ... and its round on h0's stream: one upload, launch(stream), one synchronize, download() (false: failed), free
template <class Launch, class Download>
static int stage_run(blu_hip *h0, Stage &S, const char *what_upload, const char *what_kernel, Launch launch, Download download)
{
    hipStream_t stream = h0->stream;
    bool ok = hip_ok(h0, hipMemcpyAsync(S.dev, S.host.data(), S.host.size(), hipMemcpyHostToDevice, stream), what_upload);
    if (ok) {
        launch(stream);
        ok = hip_ok(h0, hipStreamSynchronize(stream), what_kernel) && download();
    }
    (void)hipFree(S.dev);
    S.dev = nullptr;
    return ok ? BLU_OK : BLU_ERROR_DEVICE;
}
