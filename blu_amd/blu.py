"""Python host-side mirror of the reference's object API (`struct BLU`, src/blu.rs) on top of the
C ABI of libblu_hip.so (include/blu_hip.h).

The reference's host language is Rust; there is no Rust toolchain in this image, so the layer a
Rust caller would use (`extern "C"` block) is exercised from Python through ctypes
with the same method names, argument meaning and error behaviour:

    BLU(m, b_nz)                                   BLU::new                 blu.rs:61
    .factorize(b_begin, b_end, b_i, b_x)           BLU::factorize           blu.rs:95
    .get_factors()                                 BLU::get_factors         blu.rs:139
    .solve_dense(rhs, trans)                       BLU::solve_dense         blu.rs:182
    .solve_dense_multi(rhs, trans)                 solve_dense for many right-hand sides on one handle in one call
    .solve_sparse_multi(irhs_list, xrhs_list)      solve_sparse for many right-hand sides on one handle in one call
    .get_sparse_multi(total)                       the compressed solutions the last solve_sparse_multi left in the handle
    .maxvolume(ncol, a_p, a_i, a_x, basis, isbasic, volumetol)   maxvolume, src/maxvolume.rs:64 (one pass, in the library)
    .set_matrix(ncol, a_p, a_i, a_x)               the rectangular A resident on the device (blu_hip_set_matrix), then
    .factorize_columns(basis)                      ... factorize A[:, basis] with an m-sized upload
    .solve_for_update_column(j)                    ... the forward solve_for_update of column j, nothing uploaded
    .tableau_row(r, prepare_update, skip)          ... row r of B^-1 A: the transposed solve and A' y on the device
    .price(y, skip)                                ... z = A' y for a dense y
    solve_dense_batch(handles, rhs, trans)         solve_dense for many handles in one call (batch extension)
    solve_for_update_batch(handles, irhs, xrhs)    solve_for_update for many handles in one call (batch extension)
    update_batch(handles, xtbl)                    update for many handles in one call (batch extension)
    solve_sparse_batch(handles, irhs, xrhs)        solve_sparse for many handles in one call (batch extension)
    .clone()                                       a new BLU holding this one's complete state (blu_hip_clone)
    copy_batch(src, dsts)                          the state of one handle copied into many in one launch (batch extension)
    .set_param / .stat                             pub fields / getters     lu.rs:11-66, 398-684

There is NO CPU fallback: if the shared library is missing, or no gfx950 device is visible, this
module raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import keys as K

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("BLU_HIP_LIB") or os.path.join(_HERE, "libblu_hip.so")  # BLU_HIP_LIB: diagnostic builds
_LIB = None

_i64p = C.POINTER(C.c_int64)
_u64p = C.POINTER(C.c_uint64)
_f64p = C.POINTER(C.c_double)

STOPPED = 100  # debug stepping only

EXPORTS = [
    "blu_hip_new", "blu_hip_free", "blu_hip_set_param", "blu_hip_get_param", "blu_hip_get_stat",
    "blu_hip_factorize", "blu_hip_factorize_device", "blu_hip_get_factors", "blu_hip_solve_dense",
    "blu_hip_factorize_batch", "blu_hip_version", "blu_hip_device_count", "blu_hip_last_error",
    "blu_hip_solve_sparse", "blu_hip_solve_for_update", "blu_hip_update", "blu_hip_set_skip_stats", "blu_hip_gen_lp_basis",
    "blu_hip_solve_dense_batch", "blu_hip_solve_for_update_batch", "blu_hip_update_batch",
    "blu_hip_solve_sparse_batch", "blu_hip_solve_dense_multi",
    "blu_hip_solve_sparse_multi", "blu_hip_get_sparse_multi", "blu_hip_maxvolume",
    "blu_hip_copy_batch", "blu_hip_clone",
    "blu_hip_set_matrix", "blu_hip_factorize_columns", "blu_hip_solve_for_update_column", "blu_hip_tableau_row", "blu_hip_price",
    "blu_hip_set_duals", "blu_hip_get_duals", "blu_hip_get_ratio_row", "blu_hip_ratio_test", "blu_hip_update_duals",
    "blu_hip_copy_duals_batch", "blu_hip_ratio_test_batch", "blu_hip_update_duals_batch",
]


class BluError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__("blu_hip status %d %s" % (status, msg))
        self.status = status


SELFCHECK_LIB_PATH = os.path.join(_HERE, "libblu_hip_ewcheck.so")


def build_library(verbose=False, selfcheck=False):
    """Compile libblu_hip.so for gfx950 with hipcc (works without a GPU).

    selfcheck=True builds libblu_hip_ewcheck.so instead: the same library with -DBLU_EWCHECK, in which the pivot loop
    compares every early / speculative search of the next pivot with the ordinary search (candidates, count, key,
    staged entries) and raises ST_ERROR on the first difference.  Select it with BLU_HIP_LIB=<path> (diagnostic)."""
    target = "../libblu_hip_ewcheck.so" if selfcheck else "../libblu_hip.so"
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), target]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return SELFCHECK_LIB_PATH if selfcheck else _LIB_PATH


def lib():
    """Load libblu_hip.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError("libblu_hip.so not built: run blu_amd.build_library() / __graft_entry__.build()")
        L = C.CDLL(_LIB_PATH)
        L.blu_hip_new.restype = C.c_void_p
        L.blu_hip_new.argtypes = [C.c_int64, C.c_int64, C.c_int]
        L.blu_hip_free.argtypes = [C.c_void_p]
        L.blu_hip_set_param.argtypes = [C.c_void_p, C.c_int, C.c_double]
        L.blu_hip_get_param.restype = C.c_double
        L.blu_hip_get_param.argtypes = [C.c_void_p, C.c_int]
        L.blu_hip_get_stat.restype = C.c_double
        L.blu_hip_get_stat.argtypes = [C.c_void_p, C.c_int]
        L.blu_hip_factorize.argtypes = [C.c_void_p, _u64p, _u64p, _u64p, _f64p, C.c_uint64]
        L.blu_hip_factorize_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.blu_hip_get_factors.argtypes = [C.c_void_p] + [C.c_void_p] * 8
        L.blu_hip_solve_dense.argtypes = [C.c_void_p, _f64p, _f64p, C.c_char]
        L.blu_hip_solve_sparse.argtypes = [C.c_void_p, C.c_int64, _u64p, _f64p, C.c_void_p, C.c_void_p, _f64p, C.c_char]
        L.blu_hip_solve_for_update.argtypes = [C.c_void_p, C.c_int64, _u64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char]
        L.blu_hip_update.argtypes = [C.c_void_p, C.c_double]
        L.blu_hip_version.restype = C.c_char_p
        L.blu_hip_last_error.restype = C.c_char_p
        L.blu_hip_last_error.argtypes = [C.c_void_p]
        L.blu_hip_gen_lp_basis.restype = C.c_int64
        L.blu_hip_gen_lp_basis.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_uint64, _u64p, _u64p, _f64p]
        L.blu_hip_dbg_set_stop.argtypes = [C.c_void_p, C.c_int64]
        L.blu_hip_dbg_set_block.argtypes = [C.c_void_p, C.c_int]
        L.blu_hip_dbg_continue.argtypes = [C.c_void_p, C.c_int64]
        L.blu_hip_dbg_count.restype = C.c_int64
        L.blu_hip_dbg_count.argtypes = [C.c_void_p, C.c_int]
        L.blu_hip_dbg_active_state.argtypes = [C.c_void_p] + [C.c_void_p] * 12
        L.blu_hip_dbg_partial_lu.argtypes = [C.c_void_p] + [C.c_void_p] * 6
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(t)


def gen_lp_basis(m, k, bw, tri_frac, seed, offscale=1.0):
    """Synthetic LP basis (host utility inside libblu_hip.so). Returns CSC (colptr, rowidx, values)."""
    colptr = np.zeros(m + 1, dtype=np.uint64)
    n = max(1, m * max(k, 1))
    rowidx = np.zeros(n, dtype=np.uint64)
    value = np.zeros(n, dtype=np.float64)
    nnz = lib().blu_hip_gen_lp_basis(m, k, bw, float(tri_frac), float(offscale), seed,
                                     _p(colptr, _u64p), _p(rowidx, _u64p), _p(value, _f64p))
    return colptr, rowidx[:nnz].copy(), value[:nnz].copy()


def factorize_batch(handles, mats=None, device_ptrs=None, block=None):
    """Factorize len(handles) independent bases concurrently on one GPU (one workgroup per basis).

    mats: list of host matrices, each a CSC triple (colptr, rowidx, values) or, as BLU.factorize takes it, a quadruple
    (b_begin, b_end, b_i, b_x): column j is b_i[b_begin[j]..b_end[j]), b_x[...] (columns gathered from a larger
    matrix, in any order and with gaps between them), or
    device_ptrs: list of (p_begin, p_end, p_i, p_x, nnz_len) raw device pointers (inputs already in HBM).
    block: accepted for the callers that pass it and ignored (the pivot kernels of a batch have fixed workgroup sizes).
    Returns the list of per-handle statuses (reference Status numbering)."""
    n = len(handles)
    L = lib()
    L.blu_hip_factorize_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_int, C.c_void_p]
    hs = (C.c_void_p * n)(*[h._h for h in handles])
    pb, pe, pi, px = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    ln = (C.c_uint64 * n)()
    keep = []
    if device_ptrs is not None:
        for k, (b, e, i, x, nn) in enumerate(device_ptrs):
            pb[k], pe[k], pi[k], px[k], ln[k] = b, e, i, x, int(nn)
        on_dev = 1
    else:
        for k, mat in enumerate(mats):
            if len(mat) == 3:
                cp, ri, v = mat
                cp = np.ascontiguousarray(cp, dtype=np.uint64)
                bb, be = cp[:-1], cp[1:]
            else:
                bb, be, ri, v = mat
                bb = np.ascontiguousarray(bb, dtype=np.uint64)
                be = np.ascontiguousarray(be, dtype=np.uint64)
                cp = None
                if len(bb) != handles[k].m or len(be) != handles[k].m or len(ri) != len(v):
                    raise ValueError("factorize_batch: member %d: b_begin / b_end need m entries, b_i / b_x equal lengths" % k)
            ri = np.ascontiguousarray(ri, dtype=np.uint64)
            v = np.ascontiguousarray(v, dtype=np.float64)
            keep.append((cp, bb, be, ri, v))
            pb[k], pe[k], pi[k], px[k], ln[k] = bb.ctypes.data, be.ctypes.data, ri.ctypes.data, v.ctypes.data, len(ri)
        on_dev = 0
    UNTOUCHED = -12345
    st = (C.c_int * n)(*([UNTOUCHED] * n))
    rc = L.blu_hip_factorize_batch(hs, n, pb, pe, pi, px, ln, on_dev, st)
    out = [int(s) for s in st]
    if rc < 0 and any(s == UNTOUCHED for s in out):  # refused before any handle was worked on
        raise BluError(rc, handles[0].last_error())
    if rc in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY) and all(s >= 0 for s in out):
        raise BluError(rc, handles[0].last_error())
    for h, s in zip(handles, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error())
    return out


def solve_dense_batch(handles, rhs=None, trans="N", device_ptrs=None):
    """solve_dense for len(handles) handles of one device in one call (one wave per system; bit-identical per member to
    BLU.solve_dense on the same handle and right-hand side).

    rhs: list of 1-D host arrays, rhs[k] with handles[k].m entries (or an (n, m) array when every m is equal).
        Returns (solutions, statuses): the list of solutions (float64 arrays; a member that was not solved gets zeros)
        and the per-member statuses.
    device_ptrs: list of (p_rhs, p_lhs) raw device pointers of m float64 each (e.g. torch tensors' data_ptr()); p_rhs ==
        p_lhs is allowed.  Returns the statuses alone.
    A refused call raises BluError, as does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member; ERROR_INVALID_CALL of a
    member without a valid factorization is only reported in its status."""
    n = len(handles)
    L = lib()
    L.blu_hip_solve_dense_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_char, C.c_int, C.c_void_p]
    hs = (C.c_void_p * max(n, 1))(*[h._h for h in handles])
    pr, pl = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    sols = None
    if device_ptrs is not None:
        if len(device_ptrs) != n:
            raise ValueError("solve_dense_batch: one (p_rhs, p_lhs) pair per handle")
        for k, (r, l) in enumerate(device_ptrs):
            pr[k], pl[k] = int(r), int(l)
        on_dev = 1
    else:
        if rhs is None or len(rhs) != n:
            raise ValueError("solve_dense_batch: one right-hand side per handle")
        rs = [np.ascontiguousarray(rhs[k], dtype=np.float64) for k in range(n)]
        for k, (r, h) in enumerate(zip(rs, handles)):
            if r.shape != (h.m,):
                raise ValueError("solve_dense_batch: member %d: right-hand side needs m = %d entries" % (k, h.m))
        sols = [np.zeros(h.m) for h in handles]
        for k in range(n):
            pr[k], pl[k] = rs[k].ctypes.data or 8, sols[k].ctypes.data or 8  # (m == 0: any non-NULL pointer)
        on_dev = 0
    UNTOUCHED = -12345
    st = (C.c_int * max(n, 1))(*([UNTOUCHED] * max(n, 1)))
    rc = L.blu_hip_solve_dense_batch(hs, n, pr, pl, trans.encode()[0:1], on_dev, st)
    out = [int(s) for s in st][:n]
    if rc in (K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT):  # (codes only a refusal of the whole call returns)
        raise BluError(rc, "solve_dense_batch refused")
    for h, s in zip(handles, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error())
    return out if sols is None else (sols, out)


def _refused(rc, handles, what):
    """A refusal of a whole update-batch call raises; ERROR_INVALID_ARGUMENT is also a member's status (an index out of
    range), so it counts as a refusal only for what the call refuses with it: a handle twice, or two devices."""
    if rc == K.ERROR_ARGUMENT_MISSING or (rc == K.ERROR_INVALID_ARGUMENT and (
            len({h._h for h in handles}) != len(handles) or len({h.device for h in handles}) > 1)):
        raise BluError(rc, what + " refused")


def solve_for_update_batch(handles, irhs, xrhs=None, trans="N", want_solution=True):
    """BLU.solve_for_update for len(handles) handles of one device in one call (one wave per member; per member the
    status, pattern, values and statistics of the single call, bit for bit).

    irhs[k] / xrhs[k]: member k's arguments as BLU.solve_for_update takes them; trans applies to every member (xrhs may be
    None for 'T').  With want_solution each handle's previous solution is cleared and the new one left in h.lhs /
    h.ilhs[0..h.nzlhs), as BLU.solve_for_update does.  Returns the per-member statuses.  A refused call raises BluError, as
    does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member; the other codes are only reported in the member's status."""
    n = len(handles)
    if len(irhs) != n or (xrhs is not None and len(xrhs) != n):
        raise ValueError("solve_for_update_batch: one right-hand side per handle")
    L = lib()
    L.blu_hip_solve_for_update_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_char, C.c_void_p]
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in handles])
    irs = [np.ascontiguousarray(a, dtype=np.uint64) for a in irhs]
    xrs = None if xrhs is None else [np.ascontiguousarray(a, dtype=np.float64) for a in xrhs]
    nzr = (C.c_int64 * N)(*[len(a) for a in irs])
    pi, px, pil, pl = (C.c_void_p * N)(), (C.c_void_p * N)(), (C.c_void_p * N)(), (C.c_void_p * N)()
    for k, h in enumerate(handles):
        h._clear_lhs()
        pi[k] = irs[k].ctypes.data or 8  # (an empty column: any non-NULL pointer)
        if xrs is not None:
            px[k] = xrs[k].ctypes.data or 8
        pil[k], pl[k] = h.ilhs.ctypes.data, h.lhs.ctypes.data
    nzl = (C.c_int64 * N)()
    st = (C.c_int * N)()
    rc = L.blu_hip_solve_for_update_batch(hs, n, nzr, pi, None if xrs is None else px, nzl if want_solution else None,
                                          pil if want_solution else None, pl if want_solution else None, trans.encode()[0:1], st)
    _refused(rc, handles, "solve_for_update_batch")
    out = [int(s) for s in st][:n]
    for k, (h, s) in enumerate(zip(handles, out)):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error())
        if s == K.OK and want_solution:
            h.nzlhs = int(nzl[k])
    return out


def update_batch(handles, xtbl):
    """BLU.update for len(handles) handles of one device in one call: xtbl[k] for handles[k].  Returns the per-member
    statuses; errors are raised as by solve_for_update_batch."""
    n = len(handles)
    if len(xtbl) != n:
        raise ValueError("update_batch: one xtbl per handle")
    L = lib()
    L.blu_hip_update_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in handles])
    xt = (C.c_double * N)(*[float(x) for x in xtbl])
    st = (C.c_int * N)()
    rc = L.blu_hip_update_batch(hs, n, xt, st)
    _refused(rc, handles, "update_batch")
    out = [int(s) for s in st][:n]
    for h, s in zip(handles, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error())
    return out


def solve_sparse_batch(handles, irhs, xrhs, trans="N"):
    """BLU.solve_sparse for len(handles) handles of one device in one call (one wave per member; per member the status,
    pattern, values and flop counters of the single call, bit for bit).

    irhs[k] / xrhs[k]: member k's sparse right-hand side; trans applies to every member.  Each handle's previous solution
    is cleared and the new one left in h.lhs / h.ilhs[0..h.nzlhs), as BLU.solve_sparse does.  Returns the per-member
    statuses.  A refused call raises BluError, as does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member; the other codes
    are only reported in the member's status."""
    n = len(handles)
    if len(irhs) != n or len(xrhs) != n:
        raise ValueError("solve_sparse_batch: one right-hand side per handle")
    L = lib()
    L.blu_hip_solve_sparse_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_char, C.c_void_p]
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in handles])
    irs = [np.ascontiguousarray(a, dtype=np.uint64) for a in irhs]
    xrs = [np.ascontiguousarray(a, dtype=np.float64) for a in xrhs]
    for k in range(n):
        if irs[k].shape != xrs[k].shape or irs[k].ndim != 1:
            raise ValueError("solve_sparse_batch: member %d: irhs and xrhs need equal lengths" % k)
    nzr = (C.c_int64 * N)(*[len(a) for a in irs])
    pi, px, pil, pl = (C.c_void_p * N)(), (C.c_void_p * N)(), (C.c_void_p * N)(), (C.c_void_p * N)()
    for k, h in enumerate(handles):
        h._clear_lhs()
        pi[k], px[k] = irs[k].ctypes.data or None, xrs[k].ctypes.data or None  # (an empty right-hand side may pass NULL)
        pil[k], pl[k] = h.ilhs.ctypes.data, h.lhs.ctypes.data or 8  # (m == 0: any non-NULL pointer)
    nzl = (C.c_int64 * N)()
    st = (C.c_int * N)()
    rc = L.blu_hip_solve_sparse_batch(hs, n, nzr, pi, px, nzl, pil, pl, trans.encode()[0:1], st)
    _refused(rc, handles, "solve_sparse_batch")
    out = [int(s) for s in st][:n]
    for k, (h, s) in enumerate(zip(handles, out)):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error())
        if s == K.OK:
            h.nzlhs = int(nzl[k])
    return out


def copy_batch(src, dsts):
    """The complete logical state of `src` copied into every handle of `dsts` (same m, same device) in one launch: each
    is afterwards observably src -- parameters, statistics, a pending solve_for_update, the bits of every later call -- and
    independent of it.  The Python-side solution of a destination (lhs / ilhs / nzlhs) is cleared.  Returns the per-member
    statuses.  A refused call raises BluError, as does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member."""
    n = len(dsts)
    L = lib()
    L.blu_hip_copy_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in dsts])
    st = (C.c_int * N)()
    rc = L.blu_hip_copy_batch(src._h, hs, n, st)
    if rc in (K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT):  # (codes only a refusal of the whole call returns)
        raise BluError(rc, "copy_batch refused")
    out = [int(s) for s in st][:n]
    for h, s in zip(dsts, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error() or src.last_error())
        h.lhs = h.ilhs = None
        h.nzlhs = 0
    return out


def share_matrix(src, dsts):
    """Every handle of `dsts` (same m, same device) holds the resident matrix `src` holds afterwards
    (blu_hip_share_matrix): one copy of A on the device for all of them, no device copy and no launch.  A destination that
    has a matrix lets go of it first.  Returns the per-member statuses.  A refused call raises BluError, as does
    ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member."""
    n = len(dsts)
    L = lib()
    L.blu_hip_share_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in dsts])
    st = (C.c_int * N)()
    rc = L.blu_hip_share_matrix(src._h, hs, n, st)
    if rc in (K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT, K.ERROR_INVALID_CALL):  # (only a refusal of the whole call)
        raise BluError(rc, "share_matrix refused")
    out = [int(s) for s in st][:n]
    for h, s in zip(dsts, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error() or src.last_error())
        h._ncol = getattr(src, "_ncol", 0)
    return out


def _matrix_batch_refused(rc, handles, what):
    """ERROR_INVALID_ARGUMENT is also a member's status (a row out of range): it is a refusal of the whole call for a
    handle twice, two devices, or members that do not hold one matrix -- then every member carries it."""
    if rc == K.ERROR_ARGUMENT_MISSING:
        raise BluError(rc, what + " refused")
    _refused(rc, handles, what)
    L = lib()
    L.blu_hip_dbg_matrix_id.restype = C.c_void_p
    L.blu_hip_dbg_matrix_id.argtypes = [C.c_void_p]
    if rc == K.ERROR_INVALID_ARGUMENT and len({L.blu_hip_dbg_matrix_id(h._h) for h in handles} - {None}) > 1:
        raise BluError(rc, what + " refused: the handles do not hold one matrix")


def _skip_pointers(handles, skips, what):
    """(array of pointers or None, the arrays kept alive)"""
    n = len(handles)
    if skips is None:
        return None, []
    if len(skips) != n:
        raise ValueError(what + ": one skip (or None) per handle")
    keep = [h._skip(s, what) for h, s in zip(handles, skips)]
    ps = (C.c_void_p * max(n, 1))()
    for k, sk in enumerate(keep):
        ps[k] = None if sk is None else sk.ctypes.data or 8
    return ps, keep


def tableau_row_batch(handles, rows, prepare_update=False, skips=None, want_solution=False):
    """BLU.tableau_row(rows[k], prepare_update, skips[k]) for len(handles) handles that hold one matrix (share_matrix) in
    one call: per member the status, the bits of alpha, the solution and the statistics of the single call.  skips may be
    None, and so may any skips[k].  With want_solution each handle's previous solution is cleared and the new one left in
    h.lhs / h.ilhs[0..h.nzlhs).  Returns (statuses, alphas).  A refused call raises BluError, as does ERROR_DEVICE or
    ERROR_OUT_OF_MEMORY of a member; the other codes are only reported in the member's status."""
    n = len(handles)
    if len(rows) != n:
        raise ValueError("tableau_row_batch: one row per handle")
    L = lib()
    L.blu_hip_tableau_row_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in handles])
    rr = (C.c_int64 * N)(*[int(r) for r in rows])
    alphas = [np.zeros(getattr(h, "_ncol", 0)) for h in handles]
    pa, pil, pl = (C.c_void_p * N)(), (C.c_void_p * N)(), (C.c_void_p * N)()
    ps, keep = _skip_pointers(handles, skips, "tableau_row_batch")
    for k, h in enumerate(handles):
        pa[k] = alphas[k].ctypes.data or 8
        if want_solution:
            h._clear_lhs()
            pil[k], pl[k] = h.ilhs.ctypes.data, h.lhs.ctypes.data or 8
    nzl = (C.c_int64 * N)()
    st = (C.c_int * N)()
    rc = L.blu_hip_tableau_row_batch(hs, n, rr, int(bool(prepare_update)), ps, pa, nzl if want_solution else None,
                                     pil if want_solution else None, pl if want_solution else None, st)
    _matrix_batch_refused(rc, handles, "tableau_row_batch")
    out = [int(s) for s in st][:n]
    for k, (h, s) in enumerate(zip(handles, out)):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error() or handles[0].last_error())
        if s == K.OK and want_solution:
            h.nzlhs = int(nzl[k])
    del keep
    return out, alphas


def price_batch(handles, ys, skips=None):
    """BLU.price(ys[k], skips[k]) for len(handles) handles that hold one matrix in one call: (statuses, zs), z[k] with
    the bits of the single call.  A member without a matrix gets ERROR_INVALID_CALL.  A refused call raises BluError, as
    does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member."""
    n = len(handles)
    if len(ys) != n:
        raise ValueError("price_batch: one y per handle")
    yy = [np.ascontiguousarray(y, dtype=np.float64) for y in ys]
    for h, y in zip(handles, yy):
        if y.shape != (h.m,):
            raise ValueError("price_batch: y needs m = %d entries" % h.m)
    L = lib()
    L.blu_hip_price_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in handles])
    zs = [np.zeros(getattr(h, "_ncol", 0)) for h in handles]
    py, pz = (C.c_void_p * N)(), (C.c_void_p * N)()
    ps, keep = _skip_pointers(handles, skips, "price_batch")
    for k in range(n):
        py[k], pz[k] = yy[k].ctypes.data or 8, zs[k].ctypes.data or 8
    st = (C.c_int * N)()
    rc = L.blu_hip_price_batch(hs, n, py, ps, pz, st)
    out = [int(s) for s in st][:n]
    if rc in (K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT):  # (codes only a refusal of the whole call returns)
        raise BluError(rc, "price_batch refused")
    for h, s in zip(handles, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error() or handles[0].last_error())
    del keep
    return out, zs


class RatioResult(C.Structure):
    """blu_ratio_result (include/blu_hip.h)"""
    _fields_ = [("q", C.c_int64), ("ncand", C.c_int64), ("alpha_q", C.c_double), ("d_q", C.c_double), ("step", C.c_double),
                ("bound", C.c_double), ("reserved", C.c_int64 * 2)]

    def as_tuple(self):
        """(q, ncand, alpha_q, d_q, step, bound)"""
        return (int(self.q), int(self.ncand), float(self.alpha_q), float(self.d_q), float(self.step), float(self.bound))


def copy_duals_batch(src, dsts):
    """d and kind of `src` (BLU.set_duals) into every handle of `dsts` that holds src's matrix, device to device in one
    launch; the kept row is not copied.  Returns the per-member statuses (ERROR_INVALID_CALL: another matrix or none).  A
    refused call raises BluError, as does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member."""
    n = len(dsts)
    L = lib()
    L.blu_hip_copy_duals_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in dsts])
    st = (C.c_int * N)()
    rc = L.blu_hip_copy_duals_batch(src._h, hs, n, st)
    out = [int(s) for s in st][:n]
    if rc in (K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_ARGUMENT) or (rc == K.ERROR_INVALID_CALL and out == [rc] * n):
        raise BluError(rc, "copy_duals_batch refused")
    for h, s in zip(dsts, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error() or src.last_error())
    return out


def ratio_test_batch(handles, rows, sigmas, pivtol, dualtol, prepare_update=False, want_solution=False):
    """BLU.ratio_test(rows[k], sigmas[k], pivtol, dualtol, prepare_update) for len(handles) handles that hold one matrix in
    one call: per member the status, the record, the kept row, the solution and the statistics of the single call.
    Returns (statuses, records) with records[k] = (q, ncand, alpha_q, d_q, step, bound), None where the status is not OK.
    A refused call raises BluError, as does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member."""
    n = len(handles)
    if len(rows) != n or len(sigmas) != n:
        raise ValueError("ratio_test_batch: one row and one sigma per handle")
    L = lib()
    L.blu_hip_ratio_test_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 5
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in handles])
    rr = (C.c_int64 * N)(*[int(r) for r in rows])
    sg = (C.c_double * N)(*[float(s) for s in sigmas])
    recs = (RatioResult * N)()
    pil, pl = (C.c_void_p * N)(), (C.c_void_p * N)()
    if want_solution:
        for k, h in enumerate(handles):
            h._clear_lhs()
            pil[k], pl[k] = h.ilhs.ctypes.data, h.lhs.ctypes.data or 8
    nzl = (C.c_int64 * N)()
    st = (C.c_int * N)()
    rc = L.blu_hip_ratio_test_batch(hs, n, rr, int(bool(prepare_update)), sg, float(pivtol), float(dualtol), recs,
                                    nzl if want_solution else None, pil if want_solution else None, pl if want_solution else None, st)
    out = [int(s) for s in st][:n]
    if rc == K.ERROR_INVALID_ARGUMENT and not all(np.isfinite(t) and t >= 0 for t in (float(pivtol), float(dualtol))):
        raise BluError(rc, "ratio_test_batch refused: pivtol and dualtol are finite and not negative")
    _matrix_batch_refused(rc, handles, "ratio_test_batch")
    for k, (h, s) in enumerate(zip(handles, out)):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error() or handles[0].last_error())
        if s == K.OK and want_solution:
            h.nzlhs = int(nzl[k])
    return out, [recs[k].as_tuple() if out[k] == K.OK else None for k in range(n)]


def update_duals_batch(handles, thetas, sets=None):
    """BLU.update_duals(thetas[k], *sets[k]) per member in one call; sets[k] is (jset, dset, kset) or None.  Returns the
    per-member statuses.  A refused call raises BluError, as does ERROR_DEVICE or ERROR_OUT_OF_MEMORY of a member."""
    n = len(handles)
    if len(thetas) != n or (sets is not None and len(sets) != n):
        raise ValueError("update_duals_batch: one theta (and one set or None) per handle")
    L = lib()
    L.blu_hip_update_duals_batch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    N = max(n, 1)
    hs = (C.c_void_p * N)(*[h._h for h in handles])
    th = (C.c_double * N)(*[float(t) for t in thetas])
    ns = (C.c_int64 * N)()
    pj, pd, pk = (C.c_void_p * N)(), (C.c_void_p * N)(), (C.c_void_p * N)()
    keep = []
    for k in range(n):
        if sets is None or sets[k] is None:
            continue
        j, d, kd = _dual_sets(*sets[k])
        keep.append((j, d, kd))
        ns[k] = len(j)
        pj[k], pd[k], pk[k] = j.ctypes.data or 8, d.ctypes.data or 8, kd.ctypes.data or 8
    st = (C.c_int * N)()
    rc = L.blu_hip_update_duals_batch(hs, n, th, ns, pj, pd, pk, st)
    _matrix_batch_refused(rc, handles, "update_duals_batch")
    out = [int(s) for s in st][:n]
    for h, s in zip(handles, out):
        if s in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(s, h.last_error() or handles[0].last_error())
    del keep
    return out


def _dual_sets(jset, dset, kset):
    j = np.ascontiguousarray(jset, dtype=np.int64)
    d = np.ascontiguousarray(dset, dtype=np.float64)
    kd = np.ascontiguousarray(kset, dtype=np.int8)
    if not (len(j) == len(d) == len(kd)):
        raise ValueError("update_duals: jset, dset and kset need one length")
    return j, d, kd


class BLU:
    """`struct BLU` (src/blu.rs:9-20) backed by the HIP implementation."""

    def __init__(self, m, b_nz, device=0):
        self.m = int(m)
        self.device = int(device)
        self.lhs = self.ilhs = None  # BLU.lhs / BLU.ilhs / BLU.nzlhs (blu.rs:12-17): solve_sparse results
        self.nzlhs = 0
        self._h = lib().blu_hip_new(int(m), int(b_nz), int(device))
        if not self._h:
            raise BluError(K.ERROR_DEVICE, "blu_hip_new failed (no gfx950 device, bad argument or out of memory)")

    def close(self):
        if getattr(self, "_h", None):
            lib().blu_hip_free(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def clone(self):
        """A new BLU with the complete logical state of this one (blu_hip_clone: blu_hip_new with this handle's size hint
        and device, then the copy).  lhs / ilhs / nzlhs are not carried over."""
        L = lib()
        L.blu_hip_clone.restype = C.c_void_p
        L.blu_hip_clone.argtypes = [C.c_void_p]
        h = L.blu_hip_clone(self._h)
        if not h:
            raise BluError(K.ERROR_DEVICE, "blu_hip_clone failed (out of memory or device error) " + self.last_error())
        c = BLU.__new__(BLU)
        c.m = self.m
        c.device = self.device
        c.lhs = c.ilhs = None
        c.nzlhs = 0
        c._h = h
        return c

    def dbg_copy_counts(self):
        """The last copy_batch / clone with this handle as the source: (kernel launches, synchronizes, host-to-device
        copies, device allocations made, bytes of state read per destination, bytes written to all destinations)."""
        out = (C.c_int64 * 6)()
        lib().blu_hip_dbg_copy_counts.argtypes = [C.c_void_p, C.c_void_p]
        lib().blu_hip_dbg_copy_counts(self._h, out)
        return tuple(int(x) for x in out)

    # --- parameters / statistics (lu.rs public fields and getters) -------------------------------
    def set_param(self, key, value):
        st = lib().blu_hip_set_param(self._h, int(key), float(value))
        if st != K.OK:
            raise BluError(st)

    def get_param(self, key):
        return lib().blu_hip_get_param(self._h, int(key))

    def stat(self, key):
        return lib().blu_hip_get_stat(self._h, int(key))

    def last_error(self):
        return lib().blu_hip_last_error(self._h).decode()

    # --- BLU::factorize (blu.rs:95) ----------------------------------------------------------------
    def factorize(self, b_begin, b_end, b_i, b_x):
        """Returns the status (OK / WARNING_SINGULAR_MATRIX / ERROR_INVALID_ARGUMENT ...), as the reference's
        Result<(), Status> does; device failures raise."""
        bb = np.ascontiguousarray(b_begin, dtype=np.uint64)
        be = np.ascontiguousarray(b_end, dtype=np.uint64)
        bi = np.ascontiguousarray(b_i, dtype=np.uint64)
        bx = np.ascontiguousarray(b_x, dtype=np.float64)
        if len(bb) != self.m or len(be) != self.m or len(bi) != len(bx):
            return K.ERROR_INVALID_ARGUMENT
        st = lib().blu_hip_factorize(self._h, _p(bb, _u64p), _p(be, _u64p), _p(bi, _u64p), _p(bx, _f64p), len(bi))
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    def factorize_device(self, d_begin, d_end, d_i, d_x, nnz_len):
        """Same with B already in device memory (raw device pointers as ints)."""
        st = lib().blu_hip_factorize_device(self._h, d_begin, d_end, d_i, d_x, int(nnz_len))
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    # --- BLU::get_factors (blu.rs:139) -------------------------------------------------------------
    def get_factors(self):
        m = self.m
        l_nz = int(self.stat(K.STAT_L_NZ))
        u_nz = int(self.stat(K.STAT_U_NZ))
        out = dict(
            rowperm=np.zeros(m, np.int64), colperm=np.zeros(m, np.int64),
            l_colptr=np.zeros(m + 1, np.int64), l_rowidx=np.zeros(m + l_nz, np.int64), l_value=np.zeros(m + l_nz),
            u_colptr=np.zeros(m + 1, np.int64), u_rowidx=np.zeros(m + u_nz, np.int64), u_value=np.zeros(m + u_nz),
        )
        st = lib().blu_hip_get_factors(self._h, *[out[k].ctypes.data for k in
                                                  ("rowperm", "colperm", "l_colptr", "l_rowidx", "l_value",
                                                   "u_colptr", "u_rowidx", "u_value")])
        if st != K.OK:
            raise BluError(st, self.last_error())
        return out

    # --- BLU::solve_dense (blu.rs:182) -------------------------------------------------------------
    def solve_dense(self, rhs, trans="N"):
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        lhs = np.zeros(self.m)
        st = lib().blu_hip_solve_dense(self._h, _p(rhs, _f64p), _p(lhs, _f64p), trans.encode()[0:1])
        if st != K.OK:
            raise BluError(st, self.last_error())
        return lhs

    def solve_dense_multi(self, rhs=None, trans="N", device_ptrs=None):
        """solve_dense for many right-hand sides on this handle in one call (one wave per right-hand side, the factors
        shared; every solution bit-identical to solve_dense on the same right-hand side).

        rhs: (nrhs, m) host array, row j the j-th right-hand side.  Returns the (nrhs, m) solutions.
        device_ptrs: (p_rhs, ldrhs, p_lhs, ldlhs, nrhs) raw device pointers (e.g. torch tensors' data_ptr()) and leading
            dimensions in doubles: right-hand side j at p_rhs + 8*j*ldrhs, solution j at p_lhs + 8*j*ldlhs; p_rhs == p_lhs
            with equal leading dimensions is allowed.  Returns nothing.
        Errors raise BluError, as solve_dense does."""
        L = lib()
        L.blu_hip_solve_dense_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_char, C.c_int]
        tr = trans.encode()[0:1]
        if device_ptrs is not None:
            p_rhs, ldrhs, p_lhs, ldlhs, nrhs = device_ptrs
            st = L.blu_hip_solve_dense_multi(self._h, int(nrhs), int(p_rhs), int(ldrhs), int(p_lhs), int(ldlhs), tr, 1)
            if st != K.OK:
                raise BluError(st, self.last_error())
            return None
        r = np.ascontiguousarray(rhs, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != self.m:
            raise ValueError("solve_dense_multi: rhs needs the shape (nrhs, m = %d)" % self.m)
        lhs = np.zeros(r.shape)
        st = L.blu_hip_solve_dense_multi(self._h, r.shape[0], r.ctypes.data or 8, self.m, lhs.ctypes.data or 8, self.m, tr, 0)
        if st != K.OK:
            raise BluError(st, self.last_error())
        return lhs

    # --- BLU::solve_sparse (blu.rs:207) ------------------------------------------------------------
    def solve_sparse(self, irhs, xrhs, trans="N"):
        """Sparse right-hand side irhs/xrhs -> solution.  As in the reference the result stays in the
        object: self.lhs (dense, m), self.ilhs[0..self.nzlhs) the pattern in the reference's order.
        The previous solution is cleared first (lu_clear_lhs, blu.rs:380-395).  Returns the status."""
        m = self.m
        if self.lhs is None:
            self.lhs = np.zeros(m)
            self.ilhs = np.zeros(max(1, m), np.int64)
            self.nzlhs = 0
        if self.nzlhs:
            if self.nzlhs <= int(self.get_param(K.PARAM_SPARSE_THRES) * m):
                self.lhs[self.ilhs[:self.nzlhs]] = 0.0
            else:
                self.lhs[:] = 0.0
            self.nzlhs = 0
        ir = np.ascontiguousarray(irhs, dtype=np.uint64)
        xr = np.ascontiguousarray(xrhs, dtype=np.float64)
        nz = C.c_int64(0)
        st = lib().blu_hip_solve_sparse(self._h, len(ir), _p(ir, _u64p), _p(xr, _f64p), C.byref(nz),
                                        self.ilhs.ctypes.data, _p(self.lhs, _f64p), trans.encode()[0:1])
        if st == K.OK:
            self.nzlhs = int(nz.value)
        elif st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    def solve_sparse_multi(self, irhs_list, xrhs_list, trans="N"):
        """solve_sparse for many sparse right-hand sides on this handle in one call (one wave per right-hand side with a
        workspace of its own, the factors shared; per right-hand side the status, pattern order, values and flop counters of
        solve_sparse, bit for bit).

        irhs_list[j] / xrhs_list[j]: right-hand side j.  Returns (statuses, solutions) with solutions[j] = (ilhs_j, xlhs_j):
        the pattern in the reference's order and the values at those indices (empty for a right-hand side that was refused
        with ERROR_INVALID_ARGUMENT).  self.lhs / self.ilhs / self.nzlhs are not touched.  A call refused as a whole,
        ERROR_DEVICE or ERROR_OUT_OF_MEMORY raise BluError."""
        n = len(irhs_list)
        if len(xrhs_list) != n:
            raise ValueError("solve_sparse_multi: one xrhs per irhs")
        irs = [np.ascontiguousarray(a, dtype=np.uint64) for a in irhs_list]
        xrs = [np.ascontiguousarray(a, dtype=np.float64) for a in xrhs_list]
        for j in range(n):
            if irs[j].shape != xrs[j].shape or irs[j].ndim != 1:
                raise ValueError("solve_sparse_multi: right-hand side %d: irhs and xrhs need equal lengths" % j)
        ptr = np.zeros(n + 1, np.int64)
        ptr[1:] = np.cumsum([len(a) for a in irs])
        ir = np.concatenate(irs) if n else np.zeros(0, np.uint64)
        xr = np.concatenate(xrs) if n else np.zeros(0)
        lp = np.zeros(n + 1, np.int64)
        st = np.zeros(max(n, 1), np.int32)
        L = lib()
        L.blu_hip_solve_sparse_multi.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char, C.c_void_p, C.c_void_p]
        rc = L.blu_hip_solve_sparse_multi(self._h, n, ptr.ctypes.data, ir.ctypes.data if len(ir) else None, xr.ctypes.data if len(xr) else None,
                                          trans.encode()[0:1], lp.ctypes.data, st.ctypes.data)
        sts = [int(s) for s in st[:n]]
        if rc < 0 and (rc in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY) or not any(s == rc for s in sts)):
            raise BluError(rc, self.last_error())
        il, xl = self.get_sparse_multi(int(lp[n]))
        return sts, [(il[lp[j]:lp[j + 1]], xl[lp[j]:lp[j + 1]]) for j in range(n)]

    def get_sparse_multi(self, total):
        """The compressed solutions of the last solve_sparse_multi: (ilhs, xlhs) of `total` = lhs_ptr[nrhs] entries each.
        May be called any number of times; raises BluError(ERROR_INVALID_CALL) if no result is held."""
        il, xl = np.zeros(total, np.int64), np.zeros(total)
        L = lib()
        L.blu_hip_get_sparse_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        st = L.blu_hip_get_sparse_multi(self._h, il.ctypes.data if total else None, xl.ctypes.data if total else None)
        if st != K.OK:
            raise BluError(st, self.last_error())
        return il, xl

    def _clear_lhs(self):
        m = self.m
        if self.lhs is None:
            self.lhs = np.zeros(m)
            self.ilhs = np.zeros(max(1, m), np.int64)
            self.nzlhs = 0
        if self.nzlhs:  # lu_clear_lhs, blu.rs:380-395
            if self.nzlhs <= int(self.get_param(K.PARAM_SPARSE_THRES) * m):
                self.lhs[self.ilhs[:self.nzlhs]] = 0.0
            else:
                self.lhs[:] = 0.0
            self.nzlhs = 0

    # --- BLU::solve_for_update (blu.rs:257) --------------------------------------------------------
    def solve_for_update(self, irhs, xrhs=None, trans="N", want_solution=True):
        """Prepare an update.  trans 'T': irhs[0] is the column to be replaced; otherwise irhs/xrhs is the column
        to be inserted.  With want_solution the solution of the system is left in self.lhs / self.ilhs[0..nzlhs)
        as by solve_sparse.  Returns the status."""
        self._clear_lhs()
        ir = np.ascontiguousarray(irhs, dtype=np.uint64)
        xr = None if xrhs is None else np.ascontiguousarray(xrhs, dtype=np.float64)
        nz = C.c_int64(0)
        if want_solution:
            st = lib().blu_hip_solve_for_update(self._h, len(ir), _p(ir, _u64p), None if xr is None else xr.ctypes.data,
                                                C.addressof(nz), self.ilhs.ctypes.data, self.lhs.ctypes.data, trans.encode()[0:1])
        else:
            st = lib().blu_hip_solve_for_update(self._h, len(ir), _p(ir, _u64p), None if xr is None else xr.ctypes.data,
                                                None, None, None, trans.encode()[0:1])
        if st == K.OK and want_solution:
            self.nzlhs = int(nz.value)
        elif st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    # --- BLU::update (blu.rs:319) ------------------------------------------------------------------
    def update(self, xtbl):
        st = lib().blu_hip_update(self._h, float(xtbl))
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    # --- maxvolume (maxvolume.rs:64) ----------------------------------------------------------------
    def maxvolume(self, ncol, a_p, a_i, a_x, basis, isbasic, volumetol):
        """One pass of maxvolume inside the library (blu_hip_maxvolume): the decisions, results and statistics of the loop
        blu_amd.maxvolume(self, ...) over the single entries, with the candidate columns priced in chunks on the device.
        basis (m entries) and isbasic (ncol entries) are updated in place, lists and arrays alike.  Returns
        (status, nupdate); ERROR_DEVICE and ERROR_OUT_OF_MEMORY raise."""
        ap = np.ascontiguousarray(a_p, dtype=np.uint64)
        ai = np.ascontiguousarray(a_i, dtype=np.uint64)
        ax = np.ascontiguousarray(a_x, dtype=np.float64)
        ncol = int(ncol)
        if len(ap) != ncol + 1 or len(basis) != self.m or len(isbasic) != ncol or len(ai) != len(ax) or (ncol >= 0 and len(ai) < int(ap[-1])):
            raise ValueError("maxvolume: a_p needs ncol + 1 entries, basis m, isbasic ncol, a_i / a_x a_p[ncol]")
        b = np.array(basis, dtype=np.int64)
        ib = np.array(isbasic, dtype=np.int64)
        nup = C.c_int64(0)
        L = lib()
        L.blu_hip_maxvolume.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5 + [C.c_double, C.c_void_p]
        st = L.blu_hip_maxvolume(self._h, ncol, ap.ctypes.data, ai.ctypes.data if len(ai) else None, ax.ctypes.data if len(ax) else None,
                                 b.ctypes.data or 8, ib.ctypes.data or 8, float(volumetol), C.addressof(nup))
        basis[:] = b.tolist() if isinstance(basis, list) else b
        isbasic[:] = ib.tolist() if isinstance(isbasic, list) else ib
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st, int(nup.value)

    def dbg_set_maxvolume_chunk(self, n):
        """Candidates per chunk of maxvolume (n <= 0: the policy); results do not depend on it."""
        lib().blu_hip_dbg_set_maxvolume_chunk.argtypes = [C.c_void_p, C.c_int64]
        lib().blu_hip_dbg_set_maxvolume_chunk(self._h, int(n))

    def dbg_maxvolume_counts(self):
        """The last maxvolume pass: (chunks launched, candidates priced, candidates discarded behind a hit, hits)."""
        out = (C.c_int64 * 4)()
        lib().blu_hip_dbg_maxvolume_counts.argtypes = [C.c_void_p, C.c_void_p]
        lib().blu_hip_dbg_maxvolume_counts(self._h, out)
        return tuple(int(x) for x in out)

    # --- the resident constraint matrix (blu_matrix.inc) -------------------------------------------------
    def set_matrix(self, ncol, a_p, a_i, a_x):
        """Make the rectangular A (ncol compressed columns, every row index below m) resident on the device.  Returns the
        status; ERROR_DEVICE and ERROR_OUT_OF_MEMORY raise."""
        ap = np.ascontiguousarray(a_p, dtype=np.uint64)
        ai = np.ascontiguousarray(a_i, dtype=np.uint64)
        ax = np.ascontiguousarray(a_x, dtype=np.float64)
        ncol = int(ncol)
        if len(ap) != ncol + 1 or len(ai) != len(ax) or (ncol >= 0 and len(ai) < int(ap[-1])):
            raise ValueError("set_matrix: a_p needs ncol + 1 entries, a_i / a_x a_p[ncol]")
        L = lib()
        L.blu_hip_set_matrix.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        st = L.blu_hip_set_matrix(self._h, ncol, ap.ctypes.data, ai.ctypes.data if len(ai) else None, ax.ctypes.data if len(ax) else None)
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        if st == K.OK:
            self._ncol = ncol
        return st

    def factorize_columns(self, basis):
        """factorize of A[:, basis] from the resident matrix (m column indices).  Returns the status as factorize does."""
        b = np.ascontiguousarray(basis, dtype=np.int64)
        if len(b) != self.m:
            return K.ERROR_INVALID_ARGUMENT
        L = lib()
        L.blu_hip_factorize_columns.argtypes = [C.c_void_p, C.c_void_p]
        st = L.blu_hip_factorize_columns(self._h, b.ctypes.data or 8)
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    def solve_for_update_column(self, j, want_solution=True):
        """solve_for_update(a_i_j, a_x_j, 'N') of column j of the resident matrix; the solution as there."""
        self._clear_lhs()
        nz = C.c_int64(0)
        L = lib()
        L.blu_hip_solve_for_update_column.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        if want_solution:
            st = L.blu_hip_solve_for_update_column(self._h, int(j), C.addressof(nz), self.ilhs.ctypes.data, self.lhs.ctypes.data or 8)
        else:
            st = L.blu_hip_solve_for_update_column(self._h, int(j), None, None, None)
        if st == K.OK and want_solution:
            self.nzlhs = int(nz.value)
        elif st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    def _skip(self, skip, what):
        if skip is None:
            return None
        sk = np.ascontiguousarray(skip, dtype=np.int64)
        if len(sk) != getattr(self, "_ncol", -1):
            raise ValueError(what + ": skip needs ncol entries")
        return sk

    def tableau_row(self, r, prepare_update=False, skip=None, want_solution=False):
        """Row r of B^-1 A for the resident matrix: (status, alpha) with alpha[j] = A[:, j] . (B^-T e_r), +0.0 where
        skip[j] != 0.  The transposed solve is solve_sparse([r], [1.0], 'T'), or with prepare_update the transposed
        solve_for_update([r]); with want_solution its solution is left in self.lhs / self.ilhs[0..nzlhs) as the solves
        leave it."""
        ncol = getattr(self, "_ncol", 0)
        alpha = np.zeros(ncol)
        sk = self._skip(skip, "tableau_row")
        nz = C.c_int64(0)
        L = lib()
        L.blu_hip_tableau_row.argtypes = [C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 5
        if want_solution:
            self._clear_lhs()
            st = L.blu_hip_tableau_row(self._h, int(r), int(bool(prepare_update)), None if sk is None else sk.ctypes.data or 8,
                                       alpha.ctypes.data or 8, C.addressof(nz), self.ilhs.ctypes.data, self.lhs.ctypes.data or 8)
        else:
            st = L.blu_hip_tableau_row(self._h, int(r), int(bool(prepare_update)), None if sk is None else sk.ctypes.data or 8,
                                       alpha.ctypes.data or 8, None, None, None)
        if st == K.OK and want_solution:
            self.nzlhs = int(nz.value)
        elif st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st, alpha

    def price(self, y, skip=None):
        """z[j] = A[:, j] . y for the resident matrix and a dense y of m entries; +0.0 where skip[j] != 0.  Errors raise."""
        yy = np.ascontiguousarray(y, dtype=np.float64)
        if yy.shape != (self.m,):
            raise ValueError("price: y needs m = %d entries" % self.m)
        z = np.zeros(getattr(self, "_ncol", 0))
        sk = self._skip(skip, "price")
        L = lib()
        L.blu_hip_price.argtypes = [C.c_void_p] + [C.c_void_p] * 3
        st = L.blu_hip_price(self._h, yy.ctypes.data or 8, None if sk is None else sk.ctypes.data or 8, z.ctypes.data or 8)
        if st != K.OK:
            raise BluError(st, self.last_error())
        return z

    # --- the ratio test on the device (blu_ratio.inc) -----------------------------------------------------
    def set_duals(self, d=None, kind=None):
        """Upload the reduced costs d and / or the bound status kind (0 no candidate, 1 at lower, -1 at upper, 2 free) of the
        ncol columns of the resident matrix; None keeps the previous content, the first call needs both.  Returns the
        status; ERROR_DEVICE and ERROR_OUT_OF_MEMORY raise."""
        ncol = getattr(self, "_ncol", 0)
        dd = None if d is None else np.ascontiguousarray(d, dtype=np.float64)
        kk = None if kind is None else np.ascontiguousarray(kind, dtype=np.int8)
        for a in (dd, kk):
            if a is not None and a.shape != (ncol,):
                raise ValueError("set_duals: d and kind need ncol entries")
        L = lib()
        L.blu_hip_set_duals.argtypes = [C.c_void_p] * 3
        st = L.blu_hip_set_duals(self._h, None if dd is None else dd.ctypes.data or 8, None if kk is None else kk.ctypes.data or 8)
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    def get_duals(self):
        """(status, d, kind) as the device holds them"""
        ncol = getattr(self, "_ncol", 0)
        d, kind = np.zeros(ncol), np.zeros(ncol, np.int8)
        L = lib()
        L.blu_hip_get_duals.argtypes = [C.c_void_p] * 3
        st = L.blu_hip_get_duals(self._h, d.ctypes.data or 8, kind.ctypes.data or 8)
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st, d, kind

    def ratio_row(self):
        """(status, alpha): the row the last successful ratio test on this handle kept, +0.0 where kind was 0"""
        alpha = np.zeros(getattr(self, "_ncol", 0))
        L = lib()
        L.blu_hip_get_ratio_row.argtypes = [C.c_void_p] * 2
        st = L.blu_hip_get_ratio_row(self._h, alpha.ctypes.data or 8)
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st, alpha

    def ratio_test(self, r, sigma, pivtol, dualtol, prepare_update=False, want_solution=False):
        """The dual ratio test on row r of B^-1 A, on the device: the transposed solve of tableau_row(r, prepare_update),
        the row into the kept-row buffer, and the selection rule of include/blu_hip.h over it and the resident d and
        kind.  Returns (status, (q, ncand, alpha_q, d_q, step, bound)), the record None unless the status is OK; 64 bytes
        are downloaded, plus the solution with want_solution."""
        rec = RatioResult()
        nz = C.c_int64(0)
        L = lib()
        L.blu_hip_ratio_test.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 4
        if want_solution:
            self._clear_lhs()
            st = L.blu_hip_ratio_test(self._h, int(r), int(bool(prepare_update)), float(sigma), float(pivtol), float(dualtol),
                                      C.addressof(rec), C.addressof(nz), self.ilhs.ctypes.data, self.lhs.ctypes.data or 8)
        else:
            st = L.blu_hip_ratio_test(self._h, int(r), int(bool(prepare_update)), float(sigma), float(pivtol), float(dualtol),
                                      C.addressof(rec), None, None, None)
        if st == K.OK and want_solution:
            self.nzlhs = int(nz.value)
        elif st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st, rec.as_tuple() if st == K.OK else None

    def update_duals(self, theta, jset=(), dset=(), kset=()):
        """The dual step d[j] -= theta * row[j] where kind[j] != 0, row being the kept row, then the overrides
        d[jset[t]] = dset[t], kind[jset[t]] = kset[t].  Returns the status."""
        j, d, kd = _dual_sets(jset, dset, kset)
        L = lib()
        L.blu_hip_update_duals.argtypes = [C.c_void_p, C.c_double, C.c_int64] + [C.c_void_p] * 3
        st = L.blu_hip_update_duals(self._h, float(theta), len(j), j.ctypes.data or 8, d.ctypes.data or 8, kd.ctypes.data or 8)
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    def dbg_matrix_counts(self):
        """The last price, or the last tableau_row behind its solve: (kernel launches, synchronizes, host-to-device
        copies, bytes downloaded)."""
        out = (C.c_int64 * 4)()
        lib().blu_hip_dbg_matrix_counts.argtypes = [C.c_void_p, C.c_void_p]
        lib().blu_hip_dbg_matrix_counts(self._h, out)
        return tuple(int(x) for x in out)

    def dbg_matrix_holders(self):
        """Handles that hold this handle's matrix, itself included (share_matrix); 0 when none is set."""
        lib().blu_hip_dbg_matrix_holders.argtypes = [C.c_void_p]
        return int(lib().blu_hip_dbg_matrix_holders(self._h))

    def dbg_set_matrix_batch_bytes(self, n):
        """Byte limit of the device block of tableau_row_batch / price_batch for this handle's matrix (n < 0: the
        default), so that small calls take several chunks; results do not depend on it."""
        lib().blu_hip_dbg_set_matrix_batch_bytes.argtypes = [C.c_void_p, C.c_int64]
        return int(lib().blu_hip_dbg_set_matrix_batch_bytes(self._h, int(n)))

    def dbg_set_matrix_timing(self, on=True):
        """Bracket the product kernel of tableau_row / price with two events (off by default)."""
        lib().blu_hip_dbg_set_matrix_timing.argtypes = [C.c_void_p, C.c_int]
        lib().blu_hip_dbg_set_matrix_timing(self._h, int(bool(on)))

    def dbg_matrix_kernel_seconds(self):
        """Device seconds of the product kernel in the last tableau_row / price made with dbg_set_matrix_timing."""
        lib().blu_hip_dbg_matrix_kernel_seconds.restype = C.c_double
        lib().blu_hip_dbg_matrix_kernel_seconds.argtypes = [C.c_void_p]
        return float(lib().blu_hip_dbg_matrix_kernel_seconds(self._h))

    # --- test hooks (step-wise comparison with the oracle) -------------------------------------------
    def dbg_set_stop(self, n):
        lib().blu_hip_dbg_set_stop(self._h, int(n))

    def dbg_set_block(self, threads):
        st = lib().blu_hip_dbg_set_block(self._h, int(threads))
        if st != K.OK:
            raise BluError(st)

    def set_skip_stats(self, on=True):
        """Skip the statistics tail of factorize() (condest, residual_test); default: computed, as the reference."""
        lib().blu_hip_set_skip_stats.argtypes = [C.c_void_p, C.c_int]
        lib().blu_hip_set_skip_stats(self._h, int(bool(on)))

    def dbg_set_upd_extra(self, n):
        """Arena slack of the update path (entries); small values force the host-side growth loop."""
        lib().blu_hip_dbg_set_upd_extra.argtypes = [C.c_void_p, C.c_int64]
        lib().blu_hip_dbg_set_upd_extra(self._h, int(n))

    def dbg_upd_grows(self):
        """Storage requests of the update kernels this handle has answered so far."""
        lib().blu_hip_dbg_upd_grows.restype = C.c_int64
        lib().blu_hip_dbg_upd_grows.argtypes = [C.c_void_p]
        return int(lib().blu_hip_dbg_upd_grows(self._h))

    def dbg_set_multi_ws_bytes(self, n):
        """Byte limit of the work vectors plus staging block of solve_dense_multi (-1: the default, 1 GiB); small values
        force the chunking at small shapes."""
        lib().blu_hip_dbg_set_multi_ws_bytes.argtypes = [C.c_void_p, C.c_int64]
        lib().blu_hip_dbg_set_multi_ws_bytes(self._h, int(n))

    def dbg_multi_last_chunk(self):
        """Right-hand sides per chunk of the last solve_dense_multi."""
        lib().blu_hip_dbg_multi_last_chunk.restype = C.c_int64
        lib().blu_hip_dbg_multi_last_chunk.argtypes = [C.c_void_p]
        return int(lib().blu_hip_dbg_multi_last_chunk(self._h))

    def dbg_set_sparse_multi_ws_bytes(self, n):
        """Byte limit of the workspace pool of solve_sparse_multi (-1: the default, 1 GiB; a slot takes 48 m + 64 bytes);
        small values force the chunking at small shapes."""
        lib().blu_hip_dbg_set_sparse_multi_ws_bytes.argtypes = [C.c_void_p, C.c_int64]
        lib().blu_hip_dbg_set_sparse_multi_ws_bytes(self._h, int(n))

    def dbg_sparse_multi_last_chunk(self):
        """Right-hand sides per chunk of the last solve_sparse_multi."""
        lib().blu_hip_dbg_sparse_multi_last_chunk.restype = C.c_int64
        lib().blu_hip_dbg_sparse_multi_last_chunk.argtypes = [C.c_void_p]
        return int(lib().blu_hip_dbg_sparse_multi_last_chunk(self._h))

    def dbg_set_grid_blocks(self, n):
        """Workgroups of the chip-wide O(nnz) phases of a single factorize (1 = one workgroup, as inside a batch)."""
        lib().blu_hip_dbg_set_grid_blocks.argtypes = [C.c_void_p, C.c_int]
        st = lib().blu_hip_dbg_set_grid_blocks(self._h, int(n))
        if st != K.OK:
            raise BluError(st)

    def dbg_set_pivot_kernel(self, which):
        """0 = default (one basis: k_pivot_loop; batch: k_pivot_loop_wave2 while every workgroup is resident, else
        k_pivot_loop_wave), 1 = one wave per matrix, 3 = two waves per matrix; any other value raises INVALID_ARGUMENT"""
        lib().blu_hip_dbg_set_pivot_kernel.argtypes = [C.c_void_p, C.c_int]
        st = lib().blu_hip_dbg_set_pivot_kernel(self._h, int(which))
        if st != K.OK:
            raise BluError(st, "dbg_set_pivot_kernel")

    def dbg_set_no_fast(self, on=True):
        """Run the general pivot paths only (k_pivot_fast.hip off): A/B of the two implementations."""
        lib().blu_hip_dbg_set_no_fast.argtypes = [C.c_void_p, C.c_int]
        lib().blu_hip_dbg_set_no_fast(self._h, int(bool(on)))

    def dbg_continue(self, stop_at):
        st = lib().blu_hip_dbg_continue(self._h, int(stop_at))
        if st in (K.ERROR_DEVICE, K.ERROR_OUT_OF_MEMORY):
            raise BluError(st, self.last_error())
        return st

    def dbg_active_state(self):
        m = self.m
        ncol = lib().blu_hip_dbg_count(self._h, 0)
        nrow = lib().blu_hip_dbg_count(self._h, 1)
        s = dict(
            colptr=np.zeros(m + 1, np.int64), colidx=np.zeros(max(1, ncol), np.int64), colval=np.zeros(max(1, ncol)),
            rowptr=np.zeros(m + 1, np.int64), rowidx=np.zeros(max(1, nrow), np.int64),
            colmax=np.zeros(m), pinv=np.zeros(m, np.int64), qinv=np.zeros(m, np.int64),
            col_flink=np.zeros(2 * m + 2, np.int64), col_blink=np.zeros(2 * m + 2, np.int64),
            row_flink=np.zeros(2 * m + 2, np.int64), row_blink=np.zeros(2 * m + 2, np.int64),
        )
        st = lib().blu_hip_dbg_active_state(self._h, *[s[k].ctypes.data for k in
                                                       ("colptr", "colidx", "colval", "rowptr", "rowidx", "colmax",
                                                        "pinv", "qinv", "col_flink", "col_blink", "row_flink", "row_blink")])
        if st != K.OK:
            raise BluError(st, self.last_error())
        s["colidx"], s["colval"], s["rowidx"] = s["colidx"][:ncol], s["colval"][:ncol], s["rowidx"][:nrow]
        return s

    def dbg_partial_lu(self):
        nl = lib().blu_hip_dbg_count(self._h, 2)
        nu = lib().blu_hip_dbg_count(self._h, 3)
        rank = int(self.stat(K.STAT_RANK))
        s = dict(lptr=np.zeros(rank + 1, np.int64), lidx=np.zeros(max(1, nl), np.int64), lval=np.zeros(max(1, nl)),
                 uptr=np.zeros(rank + 1, np.int64), uidx=np.zeros(max(1, nu), np.int64), uval=np.zeros(max(1, nu)))
        st = lib().blu_hip_dbg_partial_lu(self._h, *[s[k].ctypes.data for k in ("lptr", "lidx", "lval", "uptr", "uidx", "uval")])
        if st != K.OK:
            raise BluError(st, self.last_error())
        s["lidx"], s["lval"], s["uidx"], s["uval"] = s["lidx"][:nl], s["lval"][:nl], s["uidx"][:nu], s["uval"][:nu]
        return s
