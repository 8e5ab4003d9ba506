// emu_replay.cpp -- replays a tape of C-ABI calls (include/blu_hip.h) against the library it is linked with and compares
// every result, bit for bit, with the one recorded on the tape.  Built by `make emu_replay` (against libblu_emu.so) and
// `make emu_replay_asan` (against libblu_emu_asan.so, itself compiled with -fsanitize=address, so the executable carries
// the sanitizer runtime and the kernels of the CPU emulation build run under AddressSanitizer without any preloading).
// tests/test_emu_cpu_solves.py writes the tape from the CPU oracle.
//
//   emu_replay TAPE          exit status 0: every call gave the recorded result; 1: first difference (named on stderr);
//                            2: unreadable tape
//
// Tape: 8-byte words in host byte order (int64, or the bits of a double).  word 0 = TAPE_MAGIC, then records
//   OP_NEW      m b_nz                                      a new handle (the previous one is freed)
//   OP_EXTRA    n                                           blu_hip_dbg_set_upd_extra(n): arena slack of the update path
//   OP_PARAM    key value(double) status
//   OP_FACT     nnz begin[m] end[m] b_i[nnz] b_x[nnz] status
//   OP_DENSE    trans rhs[m] status lhs[m]
//   OP_SPARSE   trans nzrhs irhs[nzrhs] xrhs[nzrhs] status nzlhs ilhs[nzlhs] lhs[m]      (nzlhs.. only if status == 0)
//   OP_FORUPD   trans nzrhs irhs[nzrhs] has_x xrhs[nzrhs if has_x] want status [nzlhs ilhs[nzlhs] lhs[m] if want and status == 0]
//   OP_UPDATE   xtbl(double) status
//   OP_STAT     key value(double)
//   OP_MULTI_WS bytes                                       blu_hip_dbg_set_multi_ws_bytes(bytes): chunking of the next record
//   OP_DENSE_MULTI trans nrhs ldrhs ldlhs rhs[nrhs * m] status lhs[nrhs * m]      blu_hip_solve_dense_multi with host blocks of
//               those leading dimensions, built here: NaN between m and ldrhs, and the lhs block ends with the last solution
//   OP_SPARSE_MULTI_WS bytes                                blu_hip_dbg_set_sparse_multi_ws_bytes(bytes): chunking of the next record
//   OP_SPARSE_MULTI trans nrhs rhs_ptr[nrhs + 1] irhs[tot] xrhs[tot] rc status[nrhs] lhs_ptr[nrhs + 1] ilhs[total] xlhs[total]
//               blu_hip_solve_sparse_multi with host arrays built here that end with their last entry (tot = rhs_ptr[nrhs],
//               total = lhs_ptr[nrhs]; rhs_ptr[0] = 0), then blu_hip_get_sparse_multi into arrays of exactly total entries
//   OP_SPARSE_MULTI_GET total ilhs[total] xlhs[total]       blu_hip_get_sparse_multi twice: the held result, both times
//   OP_MAXVOLUME_CHUNK n                                    blu_hip_dbg_set_maxvolume_chunk(n): candidates per chunk of the next passes
//   OP_MAXVOLUME ncol a_p[ncol + 1] a_i[nnz] a_x[nnz] basis[m] isbasic[ncol] volumetol(double) with_nupdate status nupdate
//               basis[m] isbasic[ncol]                      blu_hip_maxvolume with host arrays built here that end with their last
//               entry (nnz = a_p[ncol], a_p[0] = 0); with_nupdate == 0 passes a NULL p_nupdate and nupdate is not compared
//   OP_CLONE                                                the handle is replaced by its blu_hip_clone and the original freed: what
//               the clone still shares with the original is a use-after-free report from here on
//   OP_COPY_INTO b_nz                                       a new handle with that size hint receives blu_hip_copy_batch from the
//               current one (status BLU_OK expected), the original is freed and the tape continues on the copy
//   OP_SET_MATRIX ncol a_p[ncol + 1] a_i[nnz] a_x[nnz] status   blu_hip_set_matrix with host arrays built here that end with their
//               last entry (nnz = a_p[ncol], a_p[0] = 0); the records below use this ncol
//   OP_FACT_COLUMNS basis[m] status                         blu_hip_factorize_columns
//   OP_FORUPD_COLUMN j want status [nzlhs ilhs[nzlhs] lhs[m] if want and status == 0]      blu_hip_solve_for_update_column
//   OP_TABLEAU_ROW r prepare_update has_skip skip[ncol if has_skip] want status [alpha[ncol] [nzlhs ilhs[nzlhs] lhs[m] if want]
//               if status == 0]                             blu_hip_tableau_row into an alpha of exactly ncol entries
//   OP_PRICE has_skip skip[ncol if has_skip] y[m] status [z[ncol] if status == 0]          blu_hip_price
//   OP_SHARE_MATRIX n                                       n new handles receive blu_hip_copy_batch from the current one and then
//               blu_hip_share_matrix (every status BLU_OK expected); they replace the holders of an earlier record and are the
//               members 1..n of the two records below, the current handle being member 0
//   OP_TABLEAU_ROW_BATCH prepare_update bytes nmem {r has_skip skip[ncol if has_skip] want}[nmem] rc {status [alpha[ncol]
//               [nzlhs ilhs[nzlhs] lhs[m] if want] if status == 0}[nmem]      blu_hip_tableau_row_batch over the first nmem
//               members after blu_hip_dbg_set_matrix_batch_bytes(bytes), every alpha of exactly ncol entries
//   OP_PRICE_BATCH bytes nmem {has_skip skip[ncol if has_skip] y[m]}[nmem] rc {status [z[ncol] if status == 0]}[nmem]
//               blu_hip_price_batch likewise
//   OP_SET_DUALS d[ncol] kind[ncol] status                   blu_hip_set_duals with arrays of exactly ncol entries (kind one word each)
//   OP_RATIO_TEST r prepare_update sigma pivtol dualtol status [q ncand alpha_q d_q step bound row[ncol] if status == 0]
//               blu_hip_ratio_test, then blu_hip_get_ratio_row
//   OP_UPDATE_DUALS theta nset jset[nset] dset[nset] kset[nset] status [d[ncol] kind[ncol] if status == 0]
//               blu_hip_update_duals, then blu_hip_get_duals
//   OP_COPY_DUALS                                           blu_hip_copy_duals_batch from the current handle into the holders
//   OP_RATIO_TEST_BATCH bytes nmem {r sigma}[nmem] pivtol dualtol rc {status [record row[ncol] if status == 0]}[nmem]
//               blu_hip_ratio_test_batch over the first nmem members, then blu_hip_get_ratio_row of each
//   OP_UPDATE_DUALS_BATCH nmem {theta nset jset dset kset}[nmem] rc {status [d[ncol] kind[ncol] if status == 0]}[nmem]
//               blu_hip_update_duals_batch, then blu_hip_get_duals of each
//   OP_END
#include "../include/blu_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// the one debug hook of the library the update tapes need (blu_update.inc); not part of the product ABI
extern "C" int blu_hip_dbg_set_upd_extra(blu_hip *h, int64_t extra);
// ... and the one that sets the chunking of blu_hip_solve_dense_multi (blu_solve_multi.inc)
extern "C" int blu_hip_dbg_set_multi_ws_bytes(blu_hip *h, int64_t bytes);
// ... and of blu_hip_solve_sparse_multi (blu_solve_sparse_multi.inc)
extern "C" int blu_hip_dbg_set_sparse_multi_ws_bytes(blu_hip *h, int64_t bytes);
// ... and of blu_hip_maxvolume (blu_maxvolume.inc)
extern "C" int blu_hip_dbg_set_maxvolume_chunk(blu_hip *h, int64_t n);
// ... and of the batched products with a shared matrix (blu_matrix_batch.inc)
extern "C" int blu_hip_dbg_set_matrix_batch_bytes(blu_hip *h, int64_t bytes);

enum { OP_END = 0, OP_NEW, OP_EXTRA, OP_PARAM, OP_FACT, OP_DENSE, OP_SPARSE, OP_FORUPD, OP_UPDATE, OP_STAT, OP_MULTI_WS, OP_DENSE_MULTI,
       OP_SPARSE_MULTI_WS, OP_SPARSE_MULTI, OP_SPARSE_MULTI_GET, OP_MAXVOLUME, OP_MAXVOLUME_CHUNK, OP_CLONE, OP_COPY_INTO, OP_SET_MATRIX,
       OP_FACT_COLUMNS, OP_FORUPD_COLUMN, OP_TABLEAU_ROW, OP_PRICE, OP_SHARE_MATRIX, OP_TABLEAU_ROW_BATCH, OP_PRICE_BATCH,
       OP_SET_DUALS, OP_RATIO_TEST, OP_UPDATE_DUALS, OP_COPY_DUALS, OP_RATIO_TEST_BATCH, OP_UPDATE_DUALS_BATCH };
static const int64_t TAPE_MAGIC = 0x3145504154554c42LL; // "BLUTAPE1"
static const char *const OP_NAME[] = {"end", "new", "dbg_set_upd_extra", "set_param", "factorize", "solve_dense", "solve_sparse",
                                      "solve_for_update", "update", "get_stat", "dbg_set_multi_ws_bytes", "solve_dense_multi",
                                      "dbg_set_sparse_multi_ws_bytes", "solve_sparse_multi", "get_sparse_multi", "maxvolume",
                                      "dbg_set_maxvolume_chunk", "clone", "copy_batch", "set_matrix", "factorize_columns",
                                      "solve_for_update_column", "tableau_row", "price", "share_matrix", "tableau_row_batch",
                                      "price_batch", "set_duals", "ratio_test", "update_duals", "copy_duals_batch", "ratio_test_batch",
                                      "update_duals_batch"};

static std::vector<int64_t> tape;
static size_t pos = 0;
static long ncall = 0;
static int64_t op = 0;

static const int64_t *take(size_t n)
{
    if (n > tape.size() - pos) {
        fprintf(stderr, "emu_replay: tape ends inside call %ld (%s)\n", ncall, OP_NAME[op]);
        exit(2);
    }
    const int64_t *p = tape.data() + pos;
    pos += n;
    return p;
}
static int64_t word() { return *take(1); }
static double real()
{
    double x;
    memcpy(&x, take(1), 8);
    return x;
}
static void differ(const char *what, long k, const void *got, const void *want, bool is_double)
{
    fprintf(stderr, "emu_replay: call %ld (%s): %s", ncall, OP_NAME[op], what);
    if (k >= 0) fprintf(stderr, "[%ld]", k);
    if (is_double) {
        double g, w;
        memcpy(&g, got, 8);
        memcpy(&w, want, 8);
        fprintf(stderr, " is %.17g, the tape has %.17g\n", g, w);
    } else {
        int64_t g, w;
        memcpy(&g, got, 8);
        memcpy(&w, want, 8);
        fprintf(stderr, " is %lld, the tape has %lld\n", (long long)g, (long long)w);
    }
    exit(1);
}
static void same_int(const char *what, int64_t got, int64_t want)
{
    if (got != want) differ(what, -1, &got, &want, false);
}
static void same_words(const char *what, const void *got, const int64_t *want, size_t n, bool is_double)
{
    const char *g = (const char *)got;
    for (size_t k = 0; k < n; k++)
        if (memcmp(g + 8 * k, want + k, 8) != 0) differ(what, (long)k, g + 8 * k, want + k, is_double);
}
// the record of a ratio test, then the kept row of h
static void same_pick(blu_hip *h, const blu_ratio_result &R, size_t ncol)
{
    same_int("q", R.q, word());
    same_int("ncand", R.ncand, word());
    const double x[4] = {R.alpha_q, R.d_q, R.step, R.bound};
    same_words("record", x, take(4), 4, true);
    same_int("reserved", R.reserved[0] | R.reserved[1], 0);
    std::vector<double> row(ncol, -7.25e300);
    same_int("get_ratio_row", blu_hip_get_ratio_row(h, row.data()), BLU_OK);
    same_words("kept row", row.data(), take(ncol), ncol, true);
}
// d and kind of h
static void same_duals(blu_hip *h, size_t ncol)
{
    std::vector<double> d(ncol, -7.25e300);
    std::vector<int8_t> kind(ncol, 99);
    same_int("get_duals", blu_hip_get_duals(h, d.data(), kind.data()), BLU_OK);
    same_words("d", d.data(), take(ncol), ncol, true);
    const int64_t *tk = take(ncol);
    for (size_t j = 0; j < ncol; j++)
        if (kind[j] != tk[j]) {
            const int64_t g = kind[j];
            differ("kind", (long)j, &g, tk + j, false);
        }
}
struct DualSets { // the overrides of one dual step, arrays of exactly nset entries
    std::vector<int64_t> j;
    std::vector<double> d;
    std::vector<int8_t> k;
    void read()
    {
        const size_t n = (size_t)word();
        const int64_t *tj = take(n);
        j.assign(tj, tj + n);
        const double *td = (const double *)take(n);
        d.assign(td, td + n);
        const int64_t *tk = take(n);
        k.assign(tk, tk + n);
    }
};

// status, and for a solve that succeeded nzlhs, the pattern in order and the bits of the dense solution
static void same_solution(int status, int64_t m, int64_t nzlhs, const std::vector<int64_t> &ilhs, const std::vector<double> &lhs, bool want)
{
    same_int("status", status, word());
    if (status != BLU_OK || !want) return;
    same_int("nzlhs", nzlhs, word());
    same_words("ilhs", ilhs.data(), take((size_t)nzlhs), (size_t)nzlhs, false);
    same_words("lhs", lhs.data(), take((size_t)m), (size_t)m, true);
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: emu_replay TAPE\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    int64_t buf[4096];
    size_t n;
    while ((n = fread(buf, 8, 4096, f)) > 0) tape.insert(tape.end(), buf, buf + n);
    fclose(f);
    if (tape.empty() || tape[0] != TAPE_MAGIC) {
        fprintf(stderr, "emu_replay: %s is not a tape\n", argv[1]);
        return 2;
    }
    pos = 1;
    blu_hip *h = nullptr;
    int64_t m = 0;
    size_t ncol = 0; // of the last OP_SET_MATRIX
    std::vector<blu_hip *> holders; // of the last OP_SHARE_MATRIX
    for (;;) {
        op = word();
        if (op < OP_END || op > OP_UPDATE_DUALS_BATCH) {
            fprintf(stderr, "emu_replay: unknown record %lld after call %ld\n", (long long)op, ncall);
            return 2;
        }
        if (op == OP_END) break;
        ncall++;
        if (op != OP_NEW && !h) {
            fprintf(stderr, "emu_replay: call %ld (%s) before a handle exists\n", ncall, OP_NAME[op]);
            return 2;
        }
        switch (op) {
        case OP_NEW: {
            if (h) blu_hip_free(h);
            m = word();
            const int64_t b_nz = word();
            h = blu_hip_new(m, b_nz, 0);
            same_int("handle", h != nullptr, 1);
            break;
        }
        case OP_EXTRA:
            same_int("status", blu_hip_dbg_set_upd_extra(h, word()), BLU_OK);
            break;
        case OP_PARAM: {
            const int key = (int)word();
            const double value = real();
            same_int("status", blu_hip_set_param(h, key, value), word());
            break;
        }
        case OP_FACT: {
            const size_t nnz = (size_t)word();
            const uint64_t *bb = (const uint64_t *)take((size_t)m), *be = (const uint64_t *)take((size_t)m);
            const uint64_t *bi = (const uint64_t *)take(nnz);
            const double *bx = (const double *)take(nnz);
            same_int("status", blu_hip_factorize(h, bb, be, bi, bx, nnz), word());
            break;
        }
        case OP_DENSE: {
            const char trans = (char)word();
            const double *rhs = (const double *)take((size_t)m);
            std::vector<double> lhs((size_t)m, 0.0);
            const int st = blu_hip_solve_dense(h, rhs, lhs.data(), trans);
            same_int("status", st, word());
            if (st == BLU_OK) same_words("lhs", lhs.data(), take((size_t)m), (size_t)m, true);
            break;
        }
        case OP_SPARSE:
        case OP_FORUPD: {
            const char trans = (char)word();
            const int64_t nzrhs = word();
            const uint64_t *irhs = (const uint64_t *)take((size_t)nzrhs);
            const bool has_x = op == OP_SPARSE || word() != 0;
            const double *xrhs = has_x ? (const double *)take((size_t)nzrhs) : nullptr;
            const bool want = op == OP_SPARSE || word() != 0;
            std::vector<int64_t> ilhs((size_t)m, 0); // (exactly m: an entry written behind them is an AddressSanitizer report)
            std::vector<double> lhs((size_t)m, 0.0);
            int64_t nzlhs = 0;
            int st;
            if (op == OP_SPARSE)
                st = blu_hip_solve_sparse(h, nzrhs, irhs, xrhs, &nzlhs, ilhs.data(), lhs.data(), trans);
            else if (want)
                st = blu_hip_solve_for_update(h, nzrhs, irhs, xrhs, &nzlhs, ilhs.data(), lhs.data(), trans);
            else
                st = blu_hip_solve_for_update(h, nzrhs, irhs, xrhs, nullptr, nullptr, nullptr, trans);
            same_solution(st, m, nzlhs, ilhs, lhs, want);
            break;
        }
        case OP_UPDATE: {
            const double xtbl = real();
            same_int("status", blu_hip_update(h, xtbl), word());
            break;
        }
        case OP_MULTI_WS:
            same_int("status", blu_hip_dbg_set_multi_ws_bytes(h, word()), BLU_OK);
            break;
        case OP_DENSE_MULTI: {
            const char trans = (char)word();
            const size_t nrhs = (size_t)word(), ldr = (size_t)word(), ldl = (size_t)word(), M = (size_t)m;
            const double *rhs = (const double *)take(nrhs * M);
            // (exactly as long as the entry may touch: an access behind the last column is an AddressSanitizer report)
            std::vector<double> R(nrhs ? (nrhs - 1) * ldr + M : 0, __builtin_nan("")), X(nrhs ? (nrhs - 1) * ldl + M : 0, -7.25e300); // (= untouched)
            for (size_t j = 0; j < nrhs; j++) memcpy(R.data() + j * ldr, rhs + j * M, M * 8);
            const double untouched = -7.25e300;
            const int st = blu_hip_solve_dense_multi(h, (int64_t)nrhs, R.data(), (int64_t)ldr, X.data(), (int64_t)ldl, trans, 0);
            same_int("status", st, word());
            if (st != BLU_OK) break;
            const int64_t *want = take(nrhs * M);
            for (size_t j = 0; j < nrhs; j++) {
                same_words("lhs", X.data() + j * ldl, want + j * M, M, true);
                for (size_t k = M; k < ldl && j + 1 < nrhs; k++)
                    if (X[j * ldl + k] != untouched) differ("padding of lhs", (long)(j * ldl + k), &X[j * ldl + k], &untouched, true);
            }
            break;
        }
        case OP_SPARSE_MULTI_WS:
            same_int("status", blu_hip_dbg_set_sparse_multi_ws_bytes(h, word()), BLU_OK);
            break;
        case OP_SPARSE_MULTI: {
            const char trans = (char)word();
            const size_t nrhs = (size_t)word();
            const int64_t *p = take(nrhs + 1);
            const size_t tot = (size_t)p[nrhs];
            // (copies that end with their last entry: a read behind them is an AddressSanitizer report)
            std::vector<int64_t> rhs_ptr(p, p + nrhs + 1), lhs_ptr(nrhs + 1, -1);
            const uint64_t *ti = (const uint64_t *)take(tot);
            std::vector<uint64_t> irhs(ti, ti + tot);
            const double *tx = (const double *)take(tot);
            std::vector<double> xrhs(tx, tx + tot);
            std::vector<int> status(nrhs, -99);
            const int rc = blu_hip_solve_sparse_multi(h, (int64_t)nrhs, rhs_ptr.data(), tot ? irhs.data() : nullptr, tot ? xrhs.data() : nullptr,
                                                      trans, lhs_ptr.data(), status.data());
            same_int("return value", rc, word());
            const int64_t *ws = take(nrhs);
            for (size_t j = 0; j < nrhs; j++)
                if (status[j] != ws[j]) {
                    const int64_t got = status[j];
                    differ("status", (long)j, &got, ws + j, false);
                }
            same_words("lhs_ptr", lhs_ptr.data(), take(nrhs + 1), nrhs + 1, false);
            const size_t total = (size_t)lhs_ptr[nrhs];
            std::vector<int64_t> ilhs(total, -1); // (exactly total entries: a write behind them is an AddressSanitizer report)
            std::vector<double> xlhs(total, 0.0);
            same_int("get status", blu_hip_get_sparse_multi(h, total ? ilhs.data() : nullptr, total ? xlhs.data() : nullptr), BLU_OK);
            same_words("ilhs", ilhs.data(), take(total), total, false);
            same_words("xlhs", xlhs.data(), take(total), total, true);
            break;
        }
        case OP_SPARSE_MULTI_GET: {
            const size_t total = (size_t)word();
            const int64_t *wi = take(total), *wx = take(total);
            for (int rep = 0; rep < 2; rep++) {
                std::vector<int64_t> ilhs(total, -1);
                std::vector<double> xlhs(total, 0.0);
                same_int("get status", blu_hip_get_sparse_multi(h, total ? ilhs.data() : nullptr, total ? xlhs.data() : nullptr), BLU_OK);
                same_words("ilhs", ilhs.data(), wi, total, false);
                same_words("xlhs", xlhs.data(), wx, total, true);
            }
            break;
        }
        case OP_MAXVOLUME_CHUNK:
            same_int("status", blu_hip_dbg_set_maxvolume_chunk(h, word()), BLU_OK);
            break;
        case OP_MAXVOLUME: {
            const size_t ncol = (size_t)word(), M = (size_t)m;
            const uint64_t *p = (const uint64_t *)take(ncol + 1);
            const size_t nnz = (size_t)p[ncol];
            // (copies that end with their last entry: an access behind them is an AddressSanitizer report)
            std::vector<uint64_t> a_p(p, p + ncol + 1);
            const uint64_t *ti = (const uint64_t *)take(nnz);
            std::vector<uint64_t> a_i(ti, ti + nnz);
            const double *tx = (const double *)take(nnz);
            std::vector<double> a_x(tx, tx + nnz);
            const int64_t *tb = take(M);
            std::vector<int64_t> basis(tb, tb + M);
            const int64_t *tn = take(ncol);
            std::vector<int64_t> isbasic(tn, tn + ncol);
            const double volumetol = real();
            const bool with_nupdate = word() != 0;
            int64_t nupdate = -1;
            const int st = blu_hip_maxvolume(h, (int64_t)ncol, a_p.data(), nnz ? a_i.data() : nullptr, nnz ? a_x.data() : nullptr, basis.data(),
                                             isbasic.data(), volumetol, with_nupdate ? &nupdate : nullptr);
            same_int("status", st, word());
            const int64_t want_nupdate = word();
            if (with_nupdate) same_int("nupdate", nupdate, want_nupdate);
            same_words("basis", basis.data(), take(M), M, false);
            same_words("isbasic", isbasic.data(), take(ncol), ncol, false);
            break;
        }
        case OP_CLONE: {
            blu_hip *c = blu_hip_clone(h);
            same_int("clone", c != nullptr, 1);
            blu_hip_free(h);
            h = c;
            break;
        }
        case OP_COPY_INTO: {
            blu_hip *c = blu_hip_new(m, word(), 0);
            same_int("handle", c != nullptr, 1);
            int status = -99;
            same_int("return value", blu_hip_copy_batch(h, &c, 1, &status), BLU_OK);
            same_int("status", status, BLU_OK);
            blu_hip_free(h);
            h = c;
            break;
        }
        case OP_SET_MATRIX: {
            ncol = (size_t)word();
            const uint64_t *p = (const uint64_t *)take(ncol + 1);
            const size_t nnz = (size_t)p[ncol];
            // (copies that end with their last entry: an access behind them is an AddressSanitizer report)
            std::vector<uint64_t> a_p(p, p + ncol + 1);
            const uint64_t *ti = (const uint64_t *)take(nnz);
            std::vector<uint64_t> a_i(ti, ti + nnz);
            const double *tx = (const double *)take(nnz);
            std::vector<double> a_x(tx, tx + nnz);
            same_int("status", blu_hip_set_matrix(h, (int64_t)ncol, a_p.data(), nnz ? a_i.data() : nullptr, nnz ? a_x.data() : nullptr), word());
            break;
        }
        case OP_FACT_COLUMNS: {
            const int64_t *tb = take((size_t)m);
            std::vector<int64_t> basis(tb, tb + m);
            same_int("status", blu_hip_factorize_columns(h, basis.data()), word());
            break;
        }
        case OP_FORUPD_COLUMN: {
            const int64_t j = word();
            const bool want = word() != 0;
            std::vector<int64_t> ilhs((size_t)m, 0);
            std::vector<double> lhs((size_t)m, 0.0);
            int64_t nzlhs = 0;
            const int st = want ? blu_hip_solve_for_update_column(h, j, &nzlhs, ilhs.data(), lhs.data())
                                : blu_hip_solve_for_update_column(h, j, nullptr, nullptr, nullptr);
            same_solution(st, m, nzlhs, ilhs, lhs, want);
            break;
        }
        case OP_TABLEAU_ROW:
        case OP_PRICE: {
            const int64_t r = op == OP_TABLEAU_ROW ? word() : 0;
            const int prepare = op == OP_TABLEAU_ROW ? (int)word() : 0;
            const bool has_skip = word() != 0;
            const int64_t *ts = take(has_skip ? ncol : 0);
            std::vector<int64_t> skip(ts, ts + (has_skip ? ncol : 0));
            std::vector<double> out(ncol, -7.25e300); // (exactly ncol entries)
            if (op == OP_PRICE) {
                const double *ty = (const double *)take((size_t)m);
                std::vector<double> y(ty, ty + m);
                const int st = blu_hip_price(h, y.data(), has_skip ? skip.data() : nullptr, out.data());
                same_int("status", st, word());
                if (st == BLU_OK) same_words("z", out.data(), take(ncol), ncol, true);
                break;
            }
            const bool want = word() != 0;
            std::vector<int64_t> ilhs((size_t)m, 0);
            std::vector<double> lhs((size_t)m, 0.0);
            int64_t nzlhs = 0;
            const int st = blu_hip_tableau_row(h, r, prepare, has_skip ? skip.data() : nullptr, out.data(), want ? &nzlhs : nullptr,
                                               want ? ilhs.data() : nullptr, want ? lhs.data() : nullptr);
            same_int("status", st, word());
            if (st != BLU_OK) break;
            same_words("alpha", out.data(), take(ncol), ncol, true);
            if (want) {
                same_int("nzlhs", nzlhs, word());
                same_words("ilhs", ilhs.data(), take((size_t)nzlhs), (size_t)nzlhs, false);
                same_words("lhs", lhs.data(), take((size_t)m), (size_t)m, true);
            }
            break;
        }
        case OP_SHARE_MATRIX: {
            for (blu_hip *k : holders) blu_hip_free(k);
            holders.assign((size_t)word(), nullptr);
            for (blu_hip *&k : holders) {
                k = blu_hip_new(m, 1, 0);
                same_int("handle", k != nullptr, 1);
            }
            std::vector<int> status(holders.size(), -99);
            same_int("copy_batch", blu_hip_copy_batch(h, holders.data(), (int)holders.size(), status.data()), BLU_OK);
            same_int("return value", blu_hip_share_matrix(h, holders.data(), (int)holders.size(), status.data()), BLU_OK);
            for (int st : status) same_int("status", st, BLU_OK);
            same_int("holders", blu_hip_dbg_matrix_holders(h), (int64_t)holders.size() + 1);
            break;
        }
        case OP_TABLEAU_ROW_BATCH:
        case OP_PRICE_BATCH: {
            const bool rows = op == OP_TABLEAU_ROW_BATCH;
            const int prepare = rows ? (int)word() : 0;
            same_int("status", blu_hip_dbg_set_matrix_batch_bytes(h, word()), BLU_OK);
            const size_t nmem = (size_t)word(), M = (size_t)m;
            if (nmem > holders.size() + 1) {
                fprintf(stderr, "emu_replay: call %ld (%s) has more members than holders\n", ncall, OP_NAME[op]);
                return 2;
            }
            std::vector<blu_hip *> hs(1, h);
            hs.insert(hs.end(), holders.begin(), holders.begin() + (long)(nmem - 1));
            // (every host array of exactly the entries the call may touch)
            std::vector<int64_t> r(nmem, 0), nzlhs(nmem, 0);
            std::vector<char> want(nmem, 0);
            std::vector<std::vector<int64_t>> skip(nmem), ilhs(nmem);
            std::vector<std::vector<double>> y(nmem), out(nmem), lhs(nmem);
            std::vector<const int64_t *> pskip(nmem, nullptr);
            std::vector<const double *> py(nmem, nullptr);
            std::vector<double *> pout(nmem), plhs(nmem, nullptr);
            std::vector<int64_t *> pilhs(nmem, nullptr);
            bool any_want = false;
            for (size_t k = 0; k < nmem; k++) {
                if (rows) r[k] = word();
                if (word() != 0) {
                    const int64_t *ts = take(ncol);
                    skip[k].assign(ts, ts + ncol);
                    pskip[k] = skip[k].data();
                }
                if (rows) {
                    want[k] = word() != 0;
                    if (want[k]) {
                        ilhs[k].assign(M, 0);
                        lhs[k].assign(M, 0.0);
                        pilhs[k] = ilhs[k].data();
                        plhs[k] = lhs[k].data();
                        any_want = true;
                    }
                } else {
                    const double *ty = (const double *)take(M);
                    y[k].assign(ty, ty + M);
                    py[k] = y[k].data();
                }
                out[k].assign(ncol, -7.25e300);
                pout[k] = out[k].data();
            }
            std::vector<int> status(nmem, -99);
            const int rc = rows ? blu_hip_tableau_row_batch(hs.data(), (int)nmem, r.data(), prepare, pskip.data(), pout.data(),
                                                            any_want ? nzlhs.data() : nullptr, any_want ? pilhs.data() : nullptr,
                                                            any_want ? plhs.data() : nullptr, status.data())
                                : blu_hip_price_batch(hs.data(), (int)nmem, py.data(), pskip.data(), pout.data(), status.data());
            same_int("return value", rc, word());
            for (size_t k = 0; k < nmem; k++) {
                same_int("status", status[k], word());
                if (status[k] != BLU_OK) continue;
                same_words(rows ? "alpha" : "z", out[k].data(), take(ncol), ncol, true);
                if (!want[k]) continue;
                same_int("nzlhs", nzlhs[k], word());
                same_words("ilhs", ilhs[k].data(), take((size_t)nzlhs[k]), (size_t)nzlhs[k], false);
                same_words("lhs", lhs[k].data(), take(M), M, true);
            }
            break;
        }
        case OP_SET_DUALS: {
            const double *td = (const double *)take(ncol);
            const std::vector<double> d(td, td + ncol);
            const int64_t *tk = take(ncol);
            const std::vector<int8_t> kind(tk, tk + ncol);
            same_int("status", blu_hip_set_duals(h, d.data(), kind.data()), word());
            break;
        }
        case OP_RATIO_TEST: {
            const int64_t r = word();
            const int prepare = (int)word();
            const double sigma = real(), pivtol = real(), dualtol = real();
            blu_ratio_result R;
            const int status = blu_hip_ratio_test(h, r, prepare, sigma, pivtol, dualtol, &R, nullptr, nullptr, nullptr);
            same_int("status", status, word());
            if (status == BLU_OK) same_pick(h, R, ncol);
            break;
        }
        case OP_UPDATE_DUALS: {
            const double theta = real();
            DualSets S;
            S.read();
            const int status = blu_hip_update_duals(h, theta, (int64_t)S.j.size(), S.j.data(), S.d.data(), S.k.data());
            same_int("status", status, word());
            if (status == BLU_OK) same_duals(h, ncol);
            break;
        }
        case OP_COPY_DUALS: {
            std::vector<int> status(holders.size(), -99);
            same_int("return value", blu_hip_copy_duals_batch(h, holders.data(), (int)holders.size(), status.data()), BLU_OK);
            for (int st : status) same_int("status", st, BLU_OK);
            break;
        }
        case OP_RATIO_TEST_BATCH:
        case OP_UPDATE_DUALS_BATCH: {
            const bool pick = op == OP_RATIO_TEST_BATCH;
            if (pick) same_int("status", blu_hip_dbg_set_matrix_batch_bytes(h, word()), BLU_OK);
            const size_t nmem = (size_t)word();
            if (nmem > holders.size() + 1) {
                fprintf(stderr, "emu_replay: call %ld (%s) has more members than holders\n", ncall, OP_NAME[op]);
                return 2;
            }
            std::vector<blu_hip *> hs(1, h);
            hs.insert(hs.end(), holders.begin(), holders.begin() + (long)(nmem - 1));
            std::vector<int64_t> r(nmem, 0), ns(nmem, 0);
            std::vector<double> x(nmem, 0.0); // sigma or theta
            std::vector<DualSets> sets(nmem);
            std::vector<const int64_t *> pj(nmem);
            std::vector<const double *> pd(nmem);
            std::vector<const int8_t *> pk(nmem);
            for (size_t k = 0; k < nmem; k++) {
                if (pick) r[k] = word();
                x[k] = real();
                if (pick) continue;
                sets[k].read();
                ns[k] = (int64_t)sets[k].j.size();
                pj[k] = sets[k].j.data();
                pd[k] = sets[k].d.data();
                pk[k] = sets[k].k.data();
            }
            std::vector<blu_ratio_result> recs(nmem);
            std::vector<int> status(nmem, -99);
            int rc;
            if (pick) {
                const double pivtol = real(), dualtol = real();
                rc = blu_hip_ratio_test_batch(hs.data(), (int)nmem, r.data(), 0, x.data(), pivtol, dualtol, recs.data(), nullptr, nullptr, nullptr,
                                              status.data());
            } else {
                rc = blu_hip_update_duals_batch(hs.data(), (int)nmem, x.data(), ns.data(), pj.data(), pd.data(), pk.data(), status.data());
            }
            same_int("return value", rc, word());
            for (size_t k = 0; k < nmem; k++) {
                same_int("status", status[k], word());
                if (status[k] != BLU_OK) continue;
                if (pick) same_pick(hs[k], recs[k], ncol);
                else same_duals(hs[k], ncol);
            }
            break;
        }
        case OP_STAT: {
            const int key = (int)word();
            const double got = blu_hip_get_stat(h, key);
            char what[32];
            snprintf(what, sizeof what, "statistic %d", key);
            same_words(what, &got, take(1), 1, true);
            break;
        }
        }
    }
    for (blu_hip *k : holders) blu_hip_free(k);
    if (h) blu_hip_free(h);
    printf("REPLAY OK: %ld calls\n", ncall);
    return 0;
}
