/*
 * blu_hip.h -- C ABI of libblu_hip.so: MI355X (gfx950) implementation of the
 * factorize hot path of the `blu` crate (rwl/blu v0.2.1).
 *
 * This is the drop-in boundary.  Each entry point replaces one method of the
 * reference's object API (`struct BLU`, /root/reference/src/blu.rs) and is what
 * a Rust `extern "C"` block in the crate would bind.
 * Plain pointers and sizes only; every array argument is HOST memory owned by
 * the caller and borrowed for the duration of the call.  No exceptions or
 * aborts cross the boundary: every function returns a status.
 *
 * A handle is not thread-safe (the reference takes `&mut self` everywhere);
 * distinct handles are independent and may live on different devices.
 */
#ifndef BLU_HIP_H
#define BLU_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: enum Status, src/lib.rs:38-64 (numbers = upstream BASICLU) */
#define BLU_OK 0
#define BLU_REALLOCATE 1                /* never returned: handled inside, as BLU::factorize does (blu.rs:105-115) */
#define BLU_WARNING_SINGULAR_MATRIX 2   /* factorization valid, rank < m (factorize.rs:176-178) */
#define BLU_ERROR_INVALID_CALL (-2)
#define BLU_ERROR_ARGUMENT_MISSING (-3)
#define BLU_ERROR_INVALID_ARGUMENT (-4)
#define BLU_ERROR_MAXIMUM_UPDATES (-5)
#define BLU_ERROR_SINGULAR_UPDATE (-6)
#define BLU_ERROR_OUT_OF_MEMORY (-9)    /* blu.rs:46 doc: BLU_ERROR_OUT_OF_MEMORY */
#define BLU_ERROR_DEVICE (-100)         /* HIP runtime error / no gfx950 device / kernel trap */

/* ---- parameters: public fields of struct LU, src/lu/lu.rs:11-66, defaults lu.rs:249-259 */
enum blu_param {
    BLU_PARAM_DROPTOL = 0,      /* 1e-20 */
    BLU_PARAM_ABSTOL = 1,       /* 1e-14 */
    BLU_PARAM_RELTOL = 2,       /* 0.1   */
    BLU_PARAM_NZBIAS = 3,       /* Option<usize>: default Some(1); pass -1 for None */
    BLU_PARAM_MAXSEARCH = 4,    /* 3     */
    BLU_PARAM_PAD = 5,          /* 4     */
    BLU_PARAM_STRETCH = 6,      /* 0.3   */
    BLU_PARAM_COMPRESS_THRES = 7, /* 0.5 */
    BLU_PARAM_SPARSE_THRES = 8, /* 0.05  */
    BLU_PARAM_SEARCH_ROWS = 9,  /* 0 (lu.rs:259; the doc comment lu.rs:63-66 says 1, the code says 0) */
    BLU_PARAM_REALLOC_FACTOR = 10 /* BLU.realloc_factor, blu.rs:68: 1.5 */
};

/* ---- statistics: getters of struct LU, src/lu/lu.rs:398-684 */
enum blu_stat {
    BLU_STAT_M = 0,
    BLU_STAT_NUPDATE = 1,        /* -1 = None (no valid factorization) */
    BLU_STAT_NFACTORIZE = 2,
    BLU_STAT_L_NZ = 3,           /* lu.rs:466 */
    BLU_STAT_U_NZ = 4,           /* lu.rs:471 */
    BLU_STAT_MIN_PIVOT = 5,
    BLU_STAT_MAX_PIVOT = 6,
    BLU_STAT_CONDEST_L = 7,
    BLU_STAT_CONDEST_U = 8,
    BLU_STAT_NORM_L = 9,
    BLU_STAT_NORM_U = 10,
    BLU_STAT_NORMEST_L_INV = 11,
    BLU_STAT_NORMEST_U_INV = 12,
    BLU_STAT_ONENORM = 13,
    BLU_STAT_INFNORM = 14,
    BLU_STAT_RESIDUAL_TEST = 15,
    BLU_STAT_MATRIX_NZ = 16,     /* lu.rs:619 */
    BLU_STAT_RANK = 17,
    BLU_STAT_BUMP_SIZE = 18,
    BLU_STAT_BUMP_NZ = 19,
    BLU_STAT_NSEARCH_PIVOT = 20,
    BLU_STAT_NEXPAND = 21,       /* layout dependent: not part of the parity contract */
    BLU_STAT_NGARBAGE = 22,      /* layout dependent: not part of the parity contract */
    BLU_STAT_FACTOR_FLOPS = 23,  /* lu.rs:658 */
    BLU_STAT_TIME_FACTORIZE = 24,
    /* 25-27: device seconds of the last factorize: singleton phase (k_prep); Markowitz search and elimination run inside
     * one persistent kernel, whose time is split only by the diagnostic build with phase counters (otherwise
     * TIME_SEARCH_PIVOT = 0 and TIME_ELIM_PIVOT = the whole pivot kernel) */
    BLU_STAT_TIME_SINGLETONS = 25,
    BLU_STAT_TIME_SEARCH_PIVOT = 26,
    BLU_STAT_TIME_ELIM_PIVOT = 27,
    BLU_STAT_UPDATE_COST_DENOM = 28, /* factorize.rs:160-166 */
    BLU_STAT_RANKDEF = 29,
    BLU_STAT_L_MEM = 30,
    BLU_STAT_U_MEM = 31,
    BLU_STAT_W_MEM = 32,
    BLU_STAT_L_FLOPS = 33,       /* lu.l_flops, accumulated by solve_sparse (lu/solve_sparse.rs:356) */
    BLU_STAT_U_FLOPS = 34,       /* lu.u_flops (:357) */
    BLU_STAT_NFORREST = 35,      /* lu.nforrest: Forrest-Tomlin updates since the last factorize (lu.rs:92) */
    BLU_STAT_PIVOT_ERROR = 36,   /* lu.pivot_error of the last update (update.rs:942) */
    BLU_STAT_R_NZ = 37,          /* lu.r_nz: nonzeros in the row eta file */
    BLU_STAT_R_FLOPS = 38,       /* lu.r_flops (lu/solve_sparse.rs:358) */
    BLU_STAT_MAX_ETA = 39,       /* lu.max_eta */
    /* device-side extras (no reference counterpart) */
    BLU_STAT_DEV_TIME_PIVOT_LOOP = 40,  /* seconds, hipEvent, last factorize */
    BLU_STAT_DEV_TIME_TOTAL = 41,       /* seconds, hipEvent, all kernels of last factorize */
    BLU_STAT_DEV_RELAUNCHES = 42,       /* pivot-loop kernel launches of last factorize */
    /* 44..47: device seconds of k_prep / k_setup / k_finish / the statistics tail of the last factorize;
     * 108, 109: inside the statistics of a single factorize, k_rows_grid and k_stats_tail_a+b (diagnostic keys
     * without enum names, as 50..58 and 60..107 of the diagnostic build) */
    BLU_STAT_NSYMPERM_TOTAL = 48,       /* lu.nsymperm_total: updates done by a symmetric permutation alone */
    BLU_STAT_NFORREST_TOTAL = 49,       /* lu.nforrest_total */
    BLU_STAT_DEV_NUNSYMPERM_TOTAL = 59, /* updates done by an unsymmetric permutation (update.rs:794-814); no getter in the reference */
    BLU_STAT_UPDATE_COST = 124          /* LU::update_cost() = update_cost_numer / update_cost_denom (lu.rs:324-326) */
};

typedef struct blu_hip blu_hip; /* opaque: owns all device + host state (= struct LU + struct BLU) */

/* BLU::new(m, b_nz) -- src/blu.rs:61, LU::new src/lu/lu.rs:243.
 * `device` = HIP device ordinal.  Returns NULL on bad argument, missing gfx950
 * device or allocation failure. */
blu_hip *blu_hip_new(int64_t m, int64_t b_nz, int device);
void blu_hip_free(blu_hip *h);

/* public parameter fields of LU / BLU -- src/lu/lu.rs:11-66, src/blu.rs:18-20 */
int blu_hip_set_param(blu_hip *h, int key, double value);
double blu_hip_get_param(const blu_hip *h, int key);
/* getters -- src/lu/lu.rs:398-684 */
double blu_hip_get_stat(const blu_hip *h, int key);

/* BLU::factorize(&mut self, b_begin, b_end, b_i, b_x) -- src/blu.rs:95-118,
 * factorize() src/factorize.rs:34-182.  Column j of B holds
 * b_i[b_begin[j]..b_end[j]], b_x[...]; b_begin/b_end may overlap (CSC colptr,
 * colptr+1).  b_i_len = length of b_i and b_x (needed to size the upload; the
 * Rust slices carry it).  Returns BLU_OK, BLU_WARNING_SINGULAR_MATRIX,
 * BLU_ERROR_INVALID_ARGUMENT (src/lu/singletons.rs:122-201), or a device error. */
int blu_hip_factorize(blu_hip *h, const uint64_t *b_begin, const uint64_t *b_end,
                      const uint64_t *b_i, const double *b_x, uint64_t b_i_len);

/* Same, with B already resident in device memory (hipMalloc'ed on the handle's
 * device).  This is the entry bench.py times: inputs in HBM when the clock starts. */
int blu_hip_factorize_device(blu_hip *h, const uint64_t *d_b_begin, const uint64_t *d_b_end,
                             const uint64_t *d_b_i, const double *d_b_x, uint64_t b_i_len);

/* BLU::get_factors -- src/blu.rs:139, get_factors() src/get_factors.rs:48-180.
 * Any NULL pointer skips that output (all three of an L or U triple must be
 * non-NULL for the triple to be written, get_factors.rs:73,122).
 * Sizes: rowperm[m], colperm[m], l_colptr[m+1], l_rowidx/l_value[m+l_nz],
 * u_colptr[m+1], u_rowidx/u_value[m+u_nz]. */
int blu_hip_get_factors(blu_hip *h, int64_t *rowperm, int64_t *colperm,
                        int64_t *l_colptr, int64_t *l_rowidx, double *l_value,
                        int64_t *u_colptr, int64_t *u_rowidx, double *u_value);

/* BLU::solve_dense -- src/blu.rs:182, src/lu/solve_dense.rs:7-120.
 * rhs and lhs may be the same array (solve_dense.rs doc, lines 14-16). */
int blu_hip_solve_dense(blu_hip *h, const double *rhs, double *lhs, char trans);

/* solve_sparse -- src/solve_sparse.rs:36-68 (BLU::solve_sparse, src/blu.rs:207, keeps the same three
 * outputs inside the object), lu/solve_sparse.rs:11-360 with solve_symbolic.rs, dfs.rs and
 * solve_triangular.rs.  Right-hand side in compressed form: irhs[0..nzrhs) (no duplicates),
 * xrhs[0..nzrhs).  `lhs` (m doubles) must be all zero on entry, as the reference requires
 * (solve_sparse.rs:23-24); on return the solution is scattered into it, *p_nzlhs is its number of
 * nonzeros and ilhs[0..*p_nzlhs) their indices IN THE REFERENCE'S ORDER (the topological order its
 * depth-first searches produce, or pivot order when the sequential branch runs; parameters
 * BLU_PARAM_SPARSE_THRES and BLU_PARAM_DROPTOL decide as in the reference).  ilhs must have room for m.
 * Returns BLU_ERROR_INVALID_CALL without a valid factorization, BLU_ERROR_INVALID_ARGUMENT for
 * nzrhs < 0, nzrhs > m or an index out of range.  Works on fresh and on updated factorizations. */
int blu_hip_solve_sparse(blu_hip *h, int64_t nzrhs, const uint64_t *irhs, const double *xrhs,
                         int64_t *p_nzlhs, int64_t *ilhs, double *lhs, char trans);

/* solve_for_update -- src/solve_for_update.rs:73-119 (BLU::solve_for_update, src/blu.rs:257-288, keeps the
 * outputs inside the object), lu/solve_for_update.rs:12-455.  Prepares an update of the factorization:
 *   trans 't'/'T': the column to be REPLACED is irhs[0] (nzrhs, xrhs and irhs[1..] are not read); computes and
 *                  stores the row eta (partial solve with U').
 *   otherwise:     irhs[0..nzrhs) / xrhs[0..nzrhs) (no duplicates) is the column to be INSERTED; computes and
 *                  stores the spike (solve with L and the row etas).
 * If p_nzlhs, ilhs and lhs are all non-NULL the solution of the system is completed and returned as by
 * blu_hip_solve_sparse (lhs all zero on entry); otherwise only the update is prepared.  Returns
 * BLU_ERROR_INVALID_CALL without a valid factorization, BLU_ERROR_MAXIMUM_UPDATES after m Forrest-Tomlin
 * updates, BLU_ERROR_INVALID_ARGUMENT for indices out of range, BLU_ERROR_ARGUMENT_MISSING for a forward
 * solve without xrhs.  Status::Reallocate is handled inside, as BLU::solve_for_update does.
 * The reference's own code is defective on this path; what is implemented is the
 * algorithm it documents (blu_amd/csrc/k_update.hip, repairs listed in oracle/orc_update.c). */
int blu_hip_solve_for_update(blu_hip *h, int64_t nzrhs, const uint64_t *irhs, const double *xrhs,
                             int64_t *p_nzlhs, int64_t *ilhs, double *lhs, char trans);

/* update -- src/update.rs:49-55 (BLU::update, src/blu.rs:319-335), lu/update.rs:388-959: replaces the column
 * named by the last transposed blu_hip_solve_for_update by the column given to the last forward one
 * (Forrest-Tomlin update, or a pure permutation update when the spiked U is still permuted triangular).
 * xtbl = element jpivot of the forward solution (stability monitor only: BLU_STAT_PIVOT_ERROR).  Returns
 * BLU_ERROR_INVALID_CALL unless both solves were done, BLU_ERROR_SINGULAR_UPDATE if the new pivot is zero or
 * below abstol (the old factorization stays valid).  Afterwards BLU_STAT_NUPDATE is one higher,
 * blu_hip_get_factors answers BLU_ERROR_INVALID_CALL (get_factors.rs:59) and the solves work on the updated
 * factorization. */
int blu_hip_update(blu_hip *h, double xtbl);

/* Batch extension (no reference counterpart; the reference's only parallel
 * axis is independent BLU objects).  Factorizes n handles that
 * live on the same device concurrently: every kernel is launched once for the batch, the pivot loop with ONE WAVE
 * per handle (k_pivot_loop_wave; throughput grows with n up to 16 handles per CU, 4096 per MI355X) -- with TWO waves
 * per handle while n is at most half of that (k_pivot_loop_wave2: large bases, where HBM capacity limits n).  Matrix k is
 * given by the k-th pointers.  status[k] receives the per-handle status (also when the call as a whole
 * is refused: then every status[k] carries the refusal and no handle keeps usable factors).  The same
 * handle may not appear twice and all handles must live on one device (BLU_ERROR_INVALID_ARGUMENT).
 * Parameters and blu_hip_set_skip_stats are honoured per handle; the workgroup size of the batch
 * (a debug knob) is taken from h[0].  Device memory: besides what the handles own, a call of at least one handle per
 * CU borrows, for its duration, 20 bytes per U entry of its largest member for every CU (7.4 GB for bases of the
 * 100k size) when that leaves at least 1 GB free; without it the same results take a little longer. */
int blu_hip_factorize_batch(blu_hip **h, int n,
                            const uint64_t *const *b_begin, const uint64_t *const *b_end,
                            const uint64_t *const *b_i, const double *const *b_x,
                            const uint64_t *b_i_len, int inputs_on_device, int *status);

/* Batch extension: blu_hip_solve_dense for n handles on one device in one call, bit-identical per member to
 * blu_hip_solve_dense on the same handle and right-hand side.  rhs[k] / lhs[k] hold m_k doubles of member k (members
 * may differ in m); with inputs_on_device != 0 they are device pointers on the handles' device, else host arrays.
 * rhs[k] == lhs[k] is allowed; the arrays of two different members must not overlap.  trans applies to every member
 * ('t' / 'T' transposed, anything else forward).  Each system runs on ONE wave (k_solve_dense_batch for a fresh
 * factorization, k_solve_dense_upd_batch after updates): one launch per kind and one synchronize for the call, no copy
 * per member with device inputs (host inputs are staged through each handle's own solve buffers).
 * status[k]: BLU_OK (also for m == 0), BLU_ERROR_INVALID_CALL for a handle without a valid factorization,
 * BLU_ERROR_OUT_OF_MEMORY if its workspace could not be allocated, BLU_ERROR_DEVICE; the other members are solved
 * regardless.  Refused as a whole, every status[k] carrying the refusal and no handle changed: NULL arrays, handles or
 * per-member pointers, n < 0 (BLU_ERROR_ARGUMENT_MISSING), the same handle twice or handles on different devices
 * (BLU_ERROR_INVALID_ARGUMENT).  n == 0 returns BLU_OK.  Returns the most negative member status, else the largest.
 * Device memory: a forward solve of a fresh factorization builds its row-wise L (k_build_lt_batch) as
 * blu_hip_solve_dense does, 8 bytes per row plus 12 bytes per L entry per handle, kept for later solves of the same
 * factorization; host inputs add the handle's 16 bytes per row of solve buffers; for its duration the call borrows
 * under 1 KB per member for the gathered descriptors. */
int blu_hip_solve_dense_batch(blu_hip **h, int n, const double *const *rhs, double *const *lhs, char trans,
                              int inputs_on_device, int *status);

/* Several right-hand sides on ONE handle: blu_hip_solve_dense for nrhs right-hand sides in one call, column j bit-identical
 * to blu_hip_solve_dense(h, rhs_j, lhs_j, trans), on fresh (rank-deficient included) and on updated factorizations.
 * Right-hand side j is rhs[j*ldrhs .. j*ldrhs+m), solution j goes to lhs[j*ldlhs .. j*ldlhs+m); what lies between m and
 * a leading dimension is neither read nor written.  rhs == lhs with ldrhs == ldlhs is allowed (in place); otherwise the
 * two blocks must not overlap.  With inputs_on_device != 0 both are device pointers on the handle's device, else host
 * arrays.  Each right-hand side runs on ONE wave with a work vector of its own, the factors are shared
 * (k_solve_dense_multi; after updates k_garbage_perm once, then k_solve_dense_upd_multi).  Afterwards the handle is as
 * after ONE blu_hip_solve_dense call: the row-wise L a forward solve built is kept, after updates the pivot sequence
 * is compacted once and the marker advanced once, and later solve_sparse / solve_for_update / update calls continue
 * exactly as they would have.
 * Checked in this order: NULL h BLU_ERROR_ARGUMENT_MISSING; no valid factorization BLU_ERROR_INVALID_CALL; NULL rhs or
 * lhs BLU_ERROR_ARGUMENT_MISSING; nrhs < 0, or ldrhs < m or ldlhs < m when nrhs > 1, BLU_ERROR_INVALID_ARGUMENT;
 * nrhs == 0 or m == 0 BLU_OK with nothing written.  BLU_ERROR_OUT_OF_MEMORY if not even one work vector can be
 * allocated (the handle stays usable), BLU_ERROR_DEVICE.
 * Device memory: the handle keeps one work vector of m + 2 doubles, rounded up to a multiple of 32, per right-hand side in
 * flight, and with host inputs a staging block of the same shape (one upload and one download per chunk); the two
 * together stay within 1 GiB: more right-hand sides than that holds are worked in chunks, launched back to back with one
 * synchronize at the end (halved further if the allocation fails).  Freed with the handle. */
int blu_hip_solve_dense_multi(blu_hip *h, int64_t nrhs, const double *rhs, int64_t ldrhs, double *lhs, int64_t ldlhs,
                              char trans, int inputs_on_device);

/* Batch extension: blu_hip_solve_for_update and blu_hip_update for n handles on one device in one call.  Member k gets
 * exactly what blu_hip_solve_for_update(h[k], nzrhs[k], irhs[k], xrhs[k], &nzlhs[k], ilhs[k], lhs[k], trans) /
 * blu_hip_update(h[k], xtbl[k]) gives: status, pattern in the same order, the bits of the values, every statistic and
 * the handle's later behaviour.  trans applies to every member; for a transposed call nzrhs and xrhs may be NULL and
 * only irhs[k][0] is read.  If nzlhs, ilhs and lhs are all NULL only the updates are prepared; if they are given, a
 * member whose ilhs[k] or lhs[k] is NULL is prepared without a solution (lhs[k] all zero on entry otherwise).
 * Each member runs on ONE wave, the members in one launch (k_solve_upd_batch / k_update_batch); a round of the call
 * costs one upload, one launch, one synchronize and one download whatever n is; members whose kernel asks for storage
 * are grown and launched again alone.  The first call after a factorization builds the row-wise L and the update
 * workspace of the members that lack them in one launch each (k_build_lt_batch, k_upd_init_batch).
 * Refused as a whole, every status[k] carrying the code and no handle touched: NULL h, irhs, a NULL handle or irhs[k],
 * a forward call with nzrhs, xrhs or an xrhs[k] NULL, NULL xtbl, n < 0 (BLU_ERROR_ARGUMENT_MISSING); the same handle
 * twice or handles on different devices (BLU_ERROR_INVALID_ARGUMENT).  n == 0 returns BLU_OK.  Everything else is per
 * member with the code of the single entry (BLU_ERROR_INVALID_CALL, BLU_ERROR_INVALID_ARGUMENT,
 * BLU_ERROR_MAXIMUM_UPDATES, BLU_ERROR_SINGULAR_UPDATE, BLU_ERROR_OUT_OF_MEMORY, BLU_ERROR_DEVICE) and the other
 * members run regardless.  status may be NULL.  Returns the most negative member status, else the largest. */
int blu_hip_solve_for_update_batch(blu_hip **h, int n, const int64_t *nzrhs, const uint64_t *const *irhs,
                                   const double *const *xrhs, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs,
                                   char trans, int *status);
int blu_hip_update_batch(blu_hip **h, int n, const double *xtbl, int *status);

/* Batch extension: blu_hip_solve_sparse for n handles on one device in one call.  Member k gets exactly what
 * blu_hip_solve_sparse(h[k], nzrhs[k], irhs[k], xrhs[k], &nzlhs[k], ilhs[k], lhs[k], trans) gives: status, nzlhs, the
 * pattern in the reference's order, the bits of the values, BLU_STAT_L_FLOPS / U_FLOPS / R_FLOPS, the branch taken and
 * the handle's later behaviour (marker, all-zero work vectors, the row-wise L kept for later calls).  lhs[k] is all
 * zero on entry, as for the single call; trans applies to every member.  Each member runs on ONE wave, the members of
 * a kind in one launch (k_solve_sparse_batch for a fresh factorization, k_solve_upd_batch after updates), and the call
 * costs, whatever n is: one upload (descriptors and every right-hand side, packed), the launches, one synchronize, one
 * download of the counters, one gather launch (k_gather_lhs_batch) and one download of the gathered solutions, which
 * the host scatters into lhs[k] / ilhs[k].  A transposed call builds the row-wise L of the fresh members that lack it
 * in one launch first (k_build_lt_batch).  The kernels keep 24 KB of LDS per member in flight, so about 6 members per
 * CU run at once and the rest follow inside the same launch.
 * Refused as a whole, every status[k] carrying the code and no handle touched: NULL h, nzrhs, nzlhs, ilhs, lhs, a NULL
 * handle, ilhs[k] or lhs[k], n < 0, NULL irhs / xrhs or a NULL irhs[k] / xrhs[k] of a member with nzrhs[k] > 0
 * (BLU_ERROR_ARGUMENT_MISSING); the same handle twice or handles on different devices (BLU_ERROR_INVALID_ARGUMENT).
 * n == 0 returns BLU_OK and writes nothing.  Everything else is per member, checked in the order of the single entry,
 * and the other members run regardless: BLU_ERROR_INVALID_CALL without a valid factorization,
 * BLU_ERROR_INVALID_ARGUMENT for nzrhs[k] < 0, nzrhs[k] > m or an index out of range, BLU_OK with nzlhs[k] = 0 for
 * m == 0, BLU_ERROR_OUT_OF_MEMORY, BLU_ERROR_DEVICE.  status may be NULL.  Returns the most negative member status,
 * else the largest.  Several SPARSE right-hand sides for ONE handle: blu_hip_solve_sparse_multi below (dense ones:
 * blu_hip_solve_dense_multi). */
int blu_hip_solve_sparse_batch(blu_hip **h, int n, const int64_t *nzrhs, const uint64_t *const *irhs,
                               const double *const *xrhs, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs,
                               char trans, int *status);

/* Several SPARSE right-hand sides on ONE handle: blu_hip_solve_sparse for nrhs right-hand sides in one call.  Right-hand
 * side j is irhs / xrhs[rhs_ptr[j] .. rhs_ptr[j+1]) (compressed columns: rhs_ptr has nrhs + 1 non-decreasing entries, no
 * index twice inside a column).  Right-hand side j gets exactly what blu_hip_solve_sparse(h, nz_j, irhs_j, xrhs_j, ...,
 * trans) gives on the same handle: status, number of nonzeros, the pattern in the reference's order and the bits of
 * the values -- on fresh (rank-deficient included) and on updated factorizations, both systems, and on both branches of
 * the second triangular solve, chosen per right-hand side by BLU_PARAM_SPARSE_THRES.
 * The call writes lhs_ptr[0 .. nrhs]: lhs_ptr[0] = 0, solution j has lhs_ptr[j+1] - lhs_ptr[j] nonzeros.  The compressed
 * solutions stay in the handle (on the host) until the next blu_hip_solve_sparse_multi or blu_hip_free;
 * blu_hip_get_sparse_multi copies them into ilhs / xlhs of lhs_ptr[nrhs] entries each, any number of times: solution j
 * in [lhs_ptr[j], lhs_ptr[j+1]), the indices blu_hip_solve_sparse leaves in ilhs[0 .. nzlhs) and the values lhs[ilhs[n]].
 * No capacity has to be guessed and no solve is ever repeated because a buffer was too small.
 * status may be NULL; status[j] is BLU_OK, or BLU_ERROR_INVALID_ARGUMENT for a column of more than m entries or with an
 * index out of range: that column gets an empty solution and counts nothing, the others are solved regardless.  Returns
 * the most negative status, else the largest.
 * Checked in this order, and a call refused as a whole touches nothing (lhs_ptr, status, the held result, the counters,
 * the handle): NULL h BLU_ERROR_ARGUMENT_MISSING; no valid factorization BLU_ERROR_INVALID_CALL; NULL rhs_ptr or lhs_ptr
 * BLU_ERROR_ARGUMENT_MISSING; NULL irhs or xrhs while rhs_ptr[nrhs] > rhs_ptr[0] BLU_ERROR_ARGUMENT_MISSING; nrhs < 0, a
 * negative rhs_ptr[0] or a decreasing rhs_ptr BLU_ERROR_INVALID_ARGUMENT; nrhs == 0 BLU_OK with an empty result held;
 * m == 0 every solution empty.  Failures of the call itself come after these checks and fail it as a whole, with
 * lhs_ptr, status, the counters and the result held before left as they were: BLU_ERROR_OUT_OF_MEMORY if not even one
 * workspace, the staging block or the result buffer can be allocated (the handle stays usable), BLU_ERROR_DEVICE for a
 * failed HIP call.  The solves on updated factors cannot ask for storage or meet a broken invariant in this mode and do
 * not write the shared status word, so no right-hand side can report such a state on its own: the one impossible state
 * the host can see, a solution count outside 0 .. m, is BLU_ERROR_DEVICE for the WHOLE call (the workspaces are dropped
 * and allocated again by the next call), not for that right-hand side alone.
 * Afterwards the handle is as after the nrhs single calls in order, wherever that can be observed: BLU_STAT_L_FLOPS,
 * U_FLOPS, R_FLOPS and BLU_STAT_UPDATE_COST have grown by the sums over the solved right-hand sides (added once, behind
 * the waves), the branch statistic is that of the last solved one, the row-wise L a transposed call built is kept, a
 * pending blu_hip_solve_for_update (spike, row eta) is untouched -- a multi call between the two solve_for_update calls
 * and blu_hip_update leaves the update exactly as it would have been --, the handle's own sparse workspace is not
 * touched and later calls continue with the bits they would have had.
 * Each right-hand side runs on ONE wave with a workspace of its own, the factors shared (k_solve_sparse_multi; after
 * updates k_solve_upd_multi, which reads the mutable U, the etas and the pivot sequence and leaves the shared update
 * state to k_upd_add_flops, one lane, once).  The kernels keep 24 KB of LDS per wave, so about 6 per CU run at once and
 * the rest follow inside the same launch.
 * Device memory: the handle keeps a pool of workspaces, 48 bytes per row plus 64 bytes each, within 1 GiB and at most
 * 8192 of them; more right-hand sides are worked in chunks, one after the other (halved further if the allocation
 * fails).  The pool has a marker of its own.  Freed with the handle.
 * Cost, per chunk: one upload (all its right-hand sides, packed; the workspaces are addressed by slot number, so there
 * are no descriptors to send), one solve launch, one synchronize, one download of the counters, one gather launch
 * (k_gather_lhs_multi).  The counters size the result buffer, so the host waits for a chunk's solves before it starts
 * the next chunk: chunks run one after the other, not back to back.  For the call: one synchronize and the download of the gathered solutions (indices and values,
 * one copy each), and the one-off k_build_lt when a transposed call on a fresh handle lacks the row-wise L.  Nothing is
 * copied or synchronized per right-hand side. */
int blu_hip_solve_sparse_multi(blu_hip *h, int64_t nrhs, const int64_t *rhs_ptr, const uint64_t *irhs, const double *xrhs,
                               char trans, int64_t *lhs_ptr, int *status);
/* BLU_ERROR_INVALID_CALL if no result of blu_hip_solve_sparse_multi is held; BLU_ERROR_ARGUMENT_MISSING for a NULL handle,
 * or for NULL arrays while the held total is above 0. */
int blu_hip_get_sparse_multi(blu_hip *h, int64_t *ilhs, double *xlhs);

/* maxvolume -- src/maxvolume.rs:64-224: one pass over the columns of the rectangular A (compressed columns a_p[ncol + 1],
 * a_i, a_x; ncol >= m), which pivots every non-basic column into the basis that grows |det B| by more than volumetol.
 * basis[m] holds the column indices of the start basis and isbasic[ncol] is nonzero exactly for them; both are updated in
 * place.  *p_nupdate (may be NULL) gets the number of basis changes; a caller repeats the pass until it is 0.
 * The pass is, decision for decision, the reference's loop over blu_hip_factorize, blu_hip_solve_for_update (forward with
 * the solution, then transposed) and blu_hip_update on this handle, with its refactorization rule (eta file full, pivot
 * error above 1e-8, BLU_STAT_UPDATE_COST above 1): the same status, *p_nupdate, basis and isbasic -- also after a pass
 * that ends early with an error --, and afterwards the same statistics (NUPDATE, NFACTORIZE, NFORREST, PIVOT_ERROR,
 * L / U / R_FLOPS, R_NZ, U_NZ, MAX_ETA, UPDATE_COST, the permutation totals, the branch statistic) and the same bits from
 * every later call -- with one exception: the loop's last forward blu_hip_solve_for_update, of a column that was not
 * taken, leaves a pending spike behind, so that a transposed blu_hip_solve_for_update and blu_hip_update right after the
 * loop would insert that column; the pass prices without storing spikes, and there blu_hip_update answers
 * BLU_ERROR_INVALID_CALL until the caller has made a forward blu_hip_solve_for_update of its own.
 * Checked before anything is touched: NULL h, a_p, basis or isbasic BLU_ERROR_ARGUMENT_MISSING; ncol < 0 or a decreasing
 * a_p BLU_ERROR_INVALID_ARGUMENT; NULL a_i or a_x while A has entries BLU_ERROR_ARGUMENT_MISSING; a basis[i] outside
 * [0, ncol) BLU_ERROR_INVALID_ARGUMENT; volumetol < 1.0 BLU_ERROR_INVALID_ARGUMENT with *p_nupdate = 0.
 * A candidate column with an index >= m or more than m entries ends the pass with BLU_ERROR_INVALID_ARGUMENT when its
 * turn comes; BLU_WARNING_SINGULAR_MATRIX or an error of a factorization, a solve or the update ends it with that status.
 * A is uploaded once per pass into buffers the handle keeps (20 bytes per entry).  The candidates are priced in chunks,
 * one wave each on the workspace pool of blu_hip_solve_sparse_multi (k_price_multi), and one wave picks the first
 * candidate taken or refused and counts those in front of it (k_price_pick): per chunk one small upload, two launches,
 * one synchronize and a 64-byte download.  A candidate that is taken is solved again through the single path, which
 * stores the spike; what was priced behind it is priced again against the new factors. */
int blu_hip_maxvolume(blu_hip *h, int64_t ncol, const uint64_t *a_p, const uint64_t *a_i, const double *a_x,
                      int64_t *basis, int64_t *isbasic, double volumetol, int64_t *p_nupdate);

/* The resident constraint matrix (no reference counterpart): the rectangular A of a simplex or branch-and-bound code is
 * uploaded once and stays on the device, and the products of an iteration with it -- the pivot row
 * alpha_r = A' (B^-T e_r), the pricing vector z = A' y -- are made there, next to the solves.
 *
 * blu_hip_set_matrix makes A resident and validated: ncol compressed columns, offsets relative to a_p[0] as in
 * blu_hip_maxvolume; ncol < m and ncol == 0 are allowed; no valid factorization is needed.  Checked in this order before
 * anything is touched, the previous matrix staying in place: NULL h or a_p BLU_ERROR_ARGUMENT_MISSING; ncol < 0 or above
 * INT_MAX, a decreasing a_p, more than INT_MAX entries BLU_ERROR_INVALID_ARGUMENT; NULL a_i or a_x while A has entries
 * BLU_ERROR_ARGUMENT_MISSING; any row index >= m BLU_ERROR_INVALID_ARGUMENT -- which is what lets the product kernel gather
 * y[a_i[q]] without a bound test.  BLU_ERROR_OUT_OF_MEMORY or BLU_ERROR_DEVICE behind these checks leave no matrix set.
 * The matrix lives in the buffers of blu_hip_maxvolume (20 bytes per entry) plus 8 m + 9 ncol bytes and a host copy of the
 * offsets.  It is the handle's own, like the other pools: it survives blu_hip_factorize, blu_hip_update, the solves and
 * blu_hip_copy_batch in either role, is not copied into a destination, and a destination keeps its own.
 * blu_hip_maxvolume overwrites the buffers with a matrix whose row indices nobody checked: after it the four entries
 * below answer BLU_ERROR_INVALID_CALL until the next blu_hip_set_matrix. */
int blu_hip_set_matrix(blu_hip *h, int64_t ncol, const uint64_t *a_p, const uint64_t *a_i, const double *a_x);
/* blu_hip_factorize of A[:, basis[0..m)] from the resident matrix with an m-sized upload: the status, factors,
 * statistics and later behaviour, bit for bit, of blu_hip_factorize given the gathered columns.  NULL h or basis
 * BLU_ERROR_ARGUMENT_MISSING; no matrix set BLU_ERROR_INVALID_CALL; a basis[i] outside [0, ncol)
 * BLU_ERROR_INVALID_ARGUMENT with the handle untouched. */
int blu_hip_factorize_columns(blu_hip *h, const int64_t *basis);
/* The forward blu_hip_solve_for_update of column j of the resident matrix, nothing uploaded: the status, stored spike,
 * solution, pattern order, bits and counters of blu_hip_solve_for_update(h, n_j, a_i_j, a_x_j, ..., 'N') with its checks in
 * their order; BLU_ERROR_INVALID_CALL without a set matrix comes first among the call-state checks, and j outside
 * [0, ncol) is BLU_ERROR_INVALID_ARGUMENT where that call refuses an index.  p_nzlhs, ilhs, lhs as there (all three or
 * no solution). */
int blu_hip_solve_for_update_column(blu_hip *h, int64_t j, int64_t *p_nzlhs, int64_t *ilhs, double *lhs);
/* Row r of B^-1 A: alpha[j] = column j of A dotted with y = B^-T e_r, for all ncol columns.
 * Step one is the transposed solve of e_r exactly as its single entry makes it -- prepare_update == 0:
 * blu_hip_solve_sparse(h, 1, [r], [1.0], ..., 'T'); otherwise the transposed blu_hip_solve_for_update(h, ., [r], ., ..., 'T')
 * with a solution, the leaving row of a dual simplex iteration, which stores the row eta -- with the same refusals in the
 * same order, flop counters, marker and later behaviour of the handle.  If p_nzlhs, ilhs and lhs are all non-NULL they are
 * filled as by that call (lhs all zero on entry); otherwise the solution is not downloaded.
 * Step two stays on the device: y (m doubles the handle keeps) is cleared, k_scatter_lhs writes the compressed solution
 * into it with the count read on the device, k_at_dot writes every alpha[j], and the ncol doubles are downloaded.
 * skip may be NULL; otherwise skip[j] != 0 (a caller passes its isbasic) gives alpha[j] = +0.0 and column j is not read.
 * The summation order is fixed (n = length of column j, t_q = a_x[q] * y[a_i[q]] rounded once, no fma, no term left out
 * for being zero): n <= 64: s = +0.0, then s = s + t_q in storage order; n > 64: 64 partial sums p[l] = +0.0, then
 * p[l] = p[l] + t_q for q - a_p[j] = l, l + 64, l + 128, ..., then for w = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + w] for
 * l < w; the result is p[0].  It does not depend on ncol, on skip or on where the column falls in the launch.
 * Additional refusals, in front of those of the solve: no matrix set BLU_ERROR_INVALID_CALL, then NULL alpha while
 * ncol > 0 BLU_ERROR_ARGUMENT_MISSING.  A failure of step two (BLU_ERROR_DEVICE) leaves the handle as after the solve.
 * Cost: what its single solve costs, plus one memset, two launches, one synchronize and one download of 8 ncol bytes, plus
 * the upload of ncol bytes when skip is given; launches and synchronizes do not depend on ncol (ncol == 0: the solve
 * alone). */
int blu_hip_tableau_row(blu_hip *h, int64_t r, int prepare_update, const int64_t *skip, double *alpha, int64_t *p_nzlhs,
                        int64_t *ilhs, double *lhs);
/* z[j] = column j of the resident matrix dotted with the dense host vector y[0..m) (for the reduced costs d = c - A' y
 * with y = blu_hip_solve_dense(c_B, 'T')): the kernel, the summation order and the skip of blu_hip_tableau_row.  Needs a
 * set matrix (else BLU_ERROR_INVALID_CALL) but no factorization, and changes nothing observable on the handle.  NULL h,
 * NULL y while m > 0 or NULL z while ncol > 0: BLU_ERROR_ARGUMENT_MISSING.  m == 0 gives every z[j] = +0.0.
 * Cost: the upload of y, of skip when given, one launch, one synchronize, one download. */
int blu_hip_price(blu_hip *h, const double *y, const int64_t *skip, double *z);
/* The last blu_hip_price, or the part of the last blu_hip_tableau_row behind its solve: out[0] kernel launches,
 * [1] synchronizes, [2] host-to-device copies, [3] bytes downloaded. */
int blu_hip_dbg_matrix_counts(const blu_hip *h, int64_t out[4]);

/* Shared matrix, batched rows (no reference counterpart): the nodes a branch-and-bound code forks with blu_hip_copy_batch
 * all work on one A.  blu_hip_share_matrix lets them hold one copy of it, and the two batch entries make the pivot rows and
 * the pricing of all of them in one call.
 *
 * After blu_hip_share_matrix every dst[k] holds the matrix src holds: blu_hip_factorize_columns,
 * blu_hip_solve_for_update_column, blu_hip_tableau_row, blu_hip_price and the two batch entries answer on dst[k] exactly as
 * on a handle that had called blu_hip_set_matrix with the same arrays.  The device arrays of A and the host offsets exist
 * once, in a reference-counted block; no device copy of A is made and nothing is launched.  Each destination gets the
 * 8 m + 9 ncol bytes blu_hip_set_matrix allocates besides A; BLU_ERROR_OUT_OF_MEMORY there is that member's status, it is
 * left without a matrix, and the others are shared regardless.  A destination that has a matrix, its own or a shared one,
 * releases it first.  A holder leaves the block through blu_hip_free, through blu_hip_set_matrix (it gets a new matrix of
 * its own) or through blu_hip_maxvolume (it answers BLU_ERROR_INVALID_CALL to the matrix entries afterwards, as any
 * handle); the other holders keep the matrix, src being a holder like the others, and the last one frees the arrays.
 * blu_hip_copy_batch in either role disturbs no holder and copies no matrix.
 * Refused as a whole, every status[k] carrying the code and nothing touched: NULL src, dst or dst[k], or n < 0,
 * BLU_ERROR_ARGUMENT_MISSING; src without a set matrix BLU_ERROR_INVALID_CALL; src among the destinations, a destination
 * twice, on another device or with another m BLU_ERROR_INVALID_ARGUMENT.  n == 0 returns BLU_OK; status may be NULL; the
 * return value is that of the other batch entries. */
int blu_hip_share_matrix(blu_hip *src, blu_hip **dst, int n, int *status);
/* handles that hold h's matrix, h included; 0 when none is set */
int blu_hip_dbg_matrix_holders(const blu_hip *h);
/* what tells one resident matrix from another: equal for the holders of one matrix, NULL when none is set */
const void *blu_hip_dbg_matrix_id(const blu_hip *h);
/* blu_hip_tableau_row(h[k], r[k], prepare_update, skip[k], alpha[k], ...) for n handles that hold one matrix, in one call:
 * member k gets the status, the bits of every alpha[k][j] in the summation order above, +0.0 for skipped columns, the
 * solution when asked for, the flop counters, the marker, the stored row eta and every later call of that single entry.
 * prepare_update applies to every member.  skip may be NULL, and so may any skip[k].  If nzlhs, ilhs and lhs are all given,
 * a member whose ilhs[k] and lhs[k] are non-NULL gets its solution (lhs[k] all zero on entry); otherwise it is not
 * downloaded.  Fresh and updated members may be mixed.
 * Step one is the batched transposed solve of its kind (blu_hip_solve_sparse_batch, blu_hip_solve_for_update_batch), the
 * solutions staying on the device.  Step two, per chunk of members: the y vectors are scattered into tiles that interleave
 * the members in groups of 8 (Y[i * 8 + t] for row i and member t), and one kernel reads every column of A once per group
 * and keeps eight sums, each with the chain of additions of blu_hip_tableau_row; the products are downloaded in one copy.
 * No result depends on the group size, on n, on a member's position or on the chunking.
 * Refused as a whole: NULL h, r, alpha or h[k], NULL alpha[k] of a member with a matrix of ncol > 0, or n < 0,
 * BLU_ERROR_ARGUMENT_MISSING; the same handle twice, two devices, or members with a set matrix that do not all hold the
 * same one BLU_ERROR_INVALID_ARGUMENT (one unshared handle with n == 1 is fine).  n == 0 returns BLU_OK.
 * Per member, in the order of the single entry, the others running regardless: BLU_ERROR_INVALID_CALL without a matrix,
 * the refusals of its solve, BLU_ERROR_OUT_OF_MEMORY, BLU_ERROR_DEVICE; a failure of step two leaves the members as after
 * their solves.
 * Cost behind the solves, per chunk: one memset, one upload of descriptors, one of the skip masks if any member skips, two
 * launches, one synchronize, one download of 8 ncol bytes per member -- none of them per member.  The device block of the
 * tiles, products and masks is kept with the shared matrix, stays within 1 GiB and is freed with the last holder. */
int blu_hip_tableau_row_batch(blu_hip **h, int n, const int64_t *r, int prepare_update, const int64_t *const *skip,
                              double *const *alpha, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, int *status);
/* blu_hip_price(h[k], y[k], skip[k], z[k]) for n handles that hold one matrix, in one call: the y tiles are laid out on
 * the host and uploaded, then the kernel, the download and the refusals of blu_hip_tableau_row_batch (NULL y[k] while
 * m > 0 or NULL z[k] while ncol > 0: BLU_ERROR_ARGUMENT_MISSING).  Changes nothing observable on the handles. */
int blu_hip_price_batch(blu_hip **h, int n, const double *const *y, const int64_t *const *skip, double *const *z, int *status);
/* debug: the byte limit of the device block of the batched products of h's matrix (< 0: the default), so that small calls
 * take several chunks; BLU_ERROR_INVALID_CALL without a set matrix.  After a batch call blu_hip_dbg_matrix_counts(h[0])
 * reports its part behind the solves, summed over the chunks. */
int blu_hip_dbg_set_matrix_batch_bytes(blu_hip *h, int64_t bytes);

/* Ratio test on the device (no reference counterpart): the reduced costs d[ncol] and the bound status kind[ncol] of the
 * columns of the resident matrix stay on the device, the dual ratio test picks the entering column there from the pivot
 * row, and the dual step d -= theta * alpha_r is made from the row the handle kept.  With
 * blu_hip_solve_for_update_column and blu_hip_update a dual simplex iteration downloads 64 bytes plus the FTRAN solution.
 *
 * kind[j]: 0 no candidate (basic, fixed), +1 at its lower bound, -1 at its upper bound, 2 free.  The state -- d, kind and
 * the kept row, 17 ncol device bytes, with a host mirror of kind -- is the handle's own and no part of what
 * blu_hip_copy_batch copies.  It is allocated at the first blu_hip_set_duals and dropped by blu_hip_set_matrix, by being a
 * destination of blu_hip_share_matrix and by blu_hip_maxvolume; then the entries below answer BLU_ERROR_INVALID_CALL until
 * the next blu_hip_set_duals.  blu_hip_tableau_row and blu_hip_price do not disturb the kept row.
 *
 * The selection rule, for sigma (exactly +1.0 or -1.0) and finite pivtol >= 0, dualtol >= 0 -- anything else is
 * BLU_ERROR_INVALID_ARGUMENT before anything is touched.  alpha is the tableau row with alpha[j] = +0.0 where
 * kind[j] == 0 (those columns are not read), a = |alpha|, s = sigma * alpha.  Column j is a candidate if kind == 1 and
 * s > pivtol, or kind == -1 and s < -pivtol, or kind == 2 and a > pivtol; its bound_j = (|d_j| + dualtol) / a_j (the sum
 * rounded once, then the quotient) and step_j = |d_j| / a_j; a NaN bound_j makes it no candidate, and a NaN alpha[j]
 * fails every comparison.  ncand counts the candidates.  None: q = -1 and every floating result +0.0.  Otherwise
 * theta = min bound_j, and q is, among the candidates with step_j <= theta, the one with the largest a_j, the smallest j
 * among equal a_j.  A minimum and a maximum of a total order: no bit depends on launch geometry, n or chunking. */
typedef struct blu_ratio_result {
    int64_t q;      /* the entering column, -1: none */
    int64_t ncand;
    double alpha_q;
    double d_q;
    double step;    /* step_q */
    double bound;   /* theta */
    int64_t reserved[2];
} blu_ratio_result;
/* Uploads d[0..ncol) and / or kind[0..ncol); a NULL pointer keeps the previous content, the first call after a drop needs
 * both (else BLU_ERROR_ARGUMENT_MISSING).  NULL h BLU_ERROR_ARGUMENT_MISSING; no matrix set BLU_ERROR_INVALID_CALL; a
 * kind[j] outside {0, 1, -1, 2} BLU_ERROR_INVALID_ARGUMENT before anything is touched.  ncol == 0 is fine.  A kept row
 * stays valid. */
int blu_hip_set_duals(blu_hip *h, const double *d, const int8_t *kind);
/* Downloads d and / or kind (NULL: not wanted).  BLU_ERROR_INVALID_CALL without duals. */
int blu_hip_get_duals(blu_hip *h, double *d, int8_t *kind);
/* Downloads the kept row: the alpha of the last blu_hip_ratio_test(_batch) that answered BLU_OK on this handle, +0.0 where
 * kind was 0.  BLU_ERROR_INVALID_CALL without duals or without a valid kept row; NULL alpha while ncol > 0
 * BLU_ERROR_ARGUMENT_MISSING. */
int blu_hip_get_ratio_row(blu_hip *h, double *alpha);
/* The pivot row r and the selection rule on it.  Step one is the solve of blu_hip_tableau_row(h, r, prepare_update, ...)
 * through the same code: its refusals in its order, flop counters, marker, stored row eta, optional download of the
 * solution.  Step two stays on the device: y cleared, k_scatter_lhs, k_at_dot with kind == 0 as the skip straight into the
 * kept-row buffer, k_ratio_pick, one synchronize, one download of the 64-byte record into *out
 * (blu_hip_dbg_matrix_counts: 3 launches, 1 synchronize, 0 uploads, 64 bytes).
 * Refusals in front of the solve, in this order: NULL h BLU_ERROR_ARGUMENT_MISSING; no matrix, then no duals
 * BLU_ERROR_INVALID_CALL; NULL out BLU_ERROR_ARGUMENT_MISSING; the argument checks of the selection rule.  A refusal,
 * the solve's own included, leaves the kept row as it was.  Behind the solve the kept row is replaced: valid when the call
 * answers BLU_OK (q == -1 included), invalid when step two fails (BLU_ERROR_DEVICE), the handle being as after the solve.
 * ncol == 0 makes the solve alone and answers q = -1. */
int blu_hip_ratio_test(blu_hip *h, int64_t r, int prepare_update, double sigma, double pivtol, double dualtol, blu_ratio_result *out,
                       int64_t *p_nzlhs, int64_t *ilhs, double *lhs);
/* The dual step d[j] = d[j] - theta * row[j] for every j with kind[j] != 0 (the product rounded once, then the difference;
 * row is the kept row), then the nset overrides d[jset[t]] = dset[t], kind[jset[t]] = kset[t] -- the entering and the
 * leaving column of a pivot.  NULL h, or NULL jset, dset or kset while nset > 0, BLU_ERROR_ARGUMENT_MISSING; no duals or no
 * valid kept row (also with theta == 0.0) BLU_ERROR_INVALID_CALL; nset < 0, an index twice or outside [0, ncol), a kset
 * outside {0, 1, -1, 2} BLU_ERROR_INVALID_ARGUMENT, nothing touched.  Cost: at most one upload (the overrides), at most
 * two launches, one synchronize, nothing downloaded.  The kept row stays valid. */
int blu_hip_update_duals(blu_hip *h, double theta, int64_t nset, const int64_t *jset, const double *dset, const int8_t *kset);
/* d and kind of src into every dst[k], device to device: one upload of the destination table, one launch and one
 * synchronize whatever n is.  The kept row is not copied; a destination keeps its own.  Refused as a whole as
 * blu_hip_share_matrix refuses (src without duals: BLU_ERROR_INVALID_CALL).  Per member: a dst[k] that does not hold
 * src's matrix BLU_ERROR_INVALID_CALL, BLU_ERROR_OUT_OF_MEMORY; the others are served regardless. */
int blu_hip_copy_duals_batch(blu_hip *src, blu_hip **dst, int n, int *status);
/* blu_hip_ratio_test(h[k], r[k], prepare_update, sigma[k], pivtol, dualtol, &out[k], ...) for n handles that hold one
 * matrix, in one call: member k gets the status, the record, the kept row, the solution, the statistics and the later
 * behaviour of the single entry.  Refused as a whole as blu_hip_tableau_row_batch refuses (NULL h, r, sigma or out
 * BLU_ERROR_ARGUMENT_MISSING; a bad pivtol or dualtol BLU_ERROR_INVALID_ARGUMENT).  Per member, in this order: no matrix,
 * then no duals BLU_ERROR_INVALID_CALL; a bad sigma[k] BLU_ERROR_INVALID_ARGUMENT; then the refusals of its solve; out[k]
 * of such a member is not written.  Step one is the batched solve of blu_hip_tableau_row_batch.  Step two, per chunk: the
 * tiles and k_at_dot_batch as there, the skip masks built from the host mirrors of kind, then k_ratio_pick_batch, one
 * workgroup per member, which also stores the member's row into its kept-row buffer; one synchronize, one download of
 * 64 bytes per member (blu_hip_dbg_matrix_counts(h[0]) per chunk: 3 launches, 1 synchronize, 3 uploads, 64 bytes per
 * member -- independent of n and ncol). */
int blu_hip_ratio_test_batch(blu_hip **h, int n, const int64_t *r, int prepare_update, const double *sigma, double pivtol, double dualtol,
                             blu_ratio_result *out, int64_t *nzlhs, int64_t *const *ilhs, double *const *lhs, int *status);
/* blu_hip_update_duals(h[k], theta[k], nset[k], jset[k], dset[k], kset[k]) per member; nset may be NULL (no overrides).
 * Refused as a whole: NULL h, theta or h[k], n < 0 BLU_ERROR_ARGUMENT_MISSING; the same handle twice, two devices or
 * members that do not hold one matrix BLU_ERROR_INVALID_ARGUMENT.  Per member the refusals of the single entry.  Cost: one
 * packed upload (the steps and the overrides of all members), at most two launches, one synchronize. */
int blu_hip_update_duals_batch(blu_hip **h, int n, const double *theta, const int64_t *nset, const int64_t *const *jset,
                               const double *const *dset, const int8_t *const *kset, int *status);

/* Copying a handle (no reference counterpart): the complete logical state of src goes into the n handles dst[0..n) of
 * the same m on the same device, so that many handles hold one factorization -- fresh or updated, a pending
 * blu_hip_solve_for_update included -- and the batch entries above can continue from it, each member its own way.
 * After a successful copy dst[k] is observably src: every blu_hip_get_param key, every blu_hip_get_stat key 0..124 (flop
 * counters, totals, UPDATE_COST, NFACTORIZE, the timing keys, L_MEM / U_MEM / W_MEM) and blu_hip_set_skip_stats answer as
 * on src, and every later call on dst[k] -- get_factors, the solves, solve_for_update, update, maxvolume, the batch entries,
 * factorize -- returns the status, the pattern order and the bits the same call on src would have returned.  A pending
 * update continues where src stands: blu_hip_update(dst[k], xtbl) right after the copy is valid when both solves had been
 * made on src.  Afterwards src and every dst[k] are independent; src itself is unchanged (statistics, the caches it has
 * built, its marker, a held blu_hip_solve_sparse_multi result).  Not part of the state, and the destination's own before
 * and after: debug knobs, environment-read settings, the workspace pools (solve_dense_multi, solve_sparse_multi, the
 * resident A of maxvolume) and the sparse workspace with its marker.  A blu_hip_solve_sparse_multi result dst[k] held is
 * dropped (blu_hip_get_sparse_multi: BLU_ERROR_INVALID_CALL until the next multi call).  A source without a valid
 * factorization (BLU_STAT_NUPDATE -1) makes every destination invalid in the same way; m == 0 copies the host state
 * and launches nothing.
 * Refused as a whole, every status[k] carrying the code and no handle touched: NULL src, dst or dst[k], n < 0
 * (BLU_ERROR_ARGUMENT_MISSING); src among the destinations, a destination twice, on another device or with another m
 * (BLU_ERROR_INVALID_ARGUMENT).  n == 0 returns BLU_OK.  Per member: BLU_ERROR_OUT_OF_MEMORY for a destination whose
 * storage could not be grown -- it is left without a valid factorization (NUPDATE -1) but usable -- and the other members
 * are copied regardless.  status may be NULL.  Returns the most negative member status, else the largest.
 * Storage: what dst[k] has allocated is reused where it holds at least the capacity of src's array, and allocated anew
 * with src's capacity otherwise; the capacity dst[k] then works with is src's, so it asks for storage exactly when src
 * would.  A second copy into the same destination allocates nothing.  src keeps a staging block of under 1 KB per
 * destination plus 4 KB.
 * Cost, whatever n is: one upload (segment table, destination pointers, the destinations' descriptors), one launch of
 * k_copy_fanout and one synchronize.  Only live extents are copied; the source is read once per group of up to 64
 * destinations.  The row-wise L and the sorted U rows are not copied: dst[k] rebuilds them, with the same bits, at
 * the first solve that needs them. */
int blu_hip_copy_batch(blu_hip *src, blu_hip **dst, int n, int *status);
/* blu_hip_new(m, src's b_nz, src's device) and blu_hip_copy_batch into it; NULL on any failure. */
blu_hip *blu_hip_clone(blu_hip *src);
/* The last blu_hip_copy_batch with this source: out[0] kernel launches, [1] synchronizes, [2] host-to-device copies,
 * [3] device allocations made, [4] bytes of state read per destination, [5] bytes written to all destinations. */
int blu_hip_dbg_copy_counts(const blu_hip *src, int64_t out[6]);

/* factorize() ends with the statistics tail of src/factorize.rs:121-147 (condest(L), condest(U),
 * residual_test; getters BLU_STAT_CONDEST_* .. BLU_STAT_RESIDUAL_TEST).  It is a chain of 8 triangular
 * sweeps (~17 % of the factorize time at 100k); a caller that never reads those getters can switch
 * it off (on != 0): the keys then return 0.  Default: computed, as the reference does. */
int blu_hip_set_skip_stats(blu_hip *h, int on);

/* Synthetic LP basis used by the benchmark and the tests (host utility, no device
 * work): CSC out, colptr[m+1], rowidx/value[<= m*k].  Returns nnz. */
int64_t blu_hip_gen_lp_basis(int64_t m, int64_t k, int64_t bw, double tri_frac, double offscale,
                             uint64_t seed, uint64_t *colptr, uint64_t *rowidx, double *value);

/* Library/device introspection */
const char *blu_hip_version(void);
int blu_hip_device_count(void);
/* Text of the last HIP/runtime error seen by this handle ("" if none). */
const char *blu_hip_last_error(const blu_hip *h);

#ifdef __cplusplus
}
#endif
#endif
