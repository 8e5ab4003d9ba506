"""Shared by the tests of the shared matrix and its batched products (blu_hip_share_matrix, _tableau_row_batch,
_price_batch): the drivers that run a set of handles through the batch entries beside clones driven by the single entries
and beside the summation order of the contract (tests/util_matrix.at_dot) -- equalities of bits only.  The library is the
one blu_amd loads: the emulation build in the child processes of tests/test_emu_cpu_matrix_batch.py, the default one in
tests/test_gpu_matrix_batch.py."""
import ctypes as C

import numpy as np

import blu_amd
from blu_amd import keys as K
from tests import util_matrix as MX
from tests import util_maxvolume as MV

INVARG, MISS, INVCALL = K.ERROR_INVALID_ARGUMENT, K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_CALL
GROUP_SIZES = (1, 7, 8, 9, 17)  # both sides of the group size of k_at_dot_batch, and more than two groups


def new_root(name):
    """(m, ncol, a, root with A set and the start basis factorized, basis, isbasic)"""
    m, ncol, a = MX.MATRICES[name]()
    g = blu_amd.BLU(m, len(a[1]))
    assert g.set_matrix(ncol, *a) == K.OK
    basis, isbasic = MV.start(m, ncol)
    assert g.factorize_columns(basis) == K.OK
    return m, ncol, a, g, basis, isbasic


def fork(h, n=1):
    """n copies of h (copy_batch) that hold h's matrix (share_matrix)"""
    out = [blu_amd.BLU(h.m, 8) for _ in range(n)]
    assert blu_amd.copy_batch(h, out) == [K.OK] * n
    assert blu_amd.share_matrix(h, out) == [K.OK] * n
    return out


def close_all(hs):
    for h in hs:
        h.close()


def sub_matrix(a, ncol):
    """another matrix: a without its last five columns"""
    return ncol - 5, (a[0][:ncol - 4], a[1], a[2])


def answers(h, a, m, ncol, basis, isbasic):
    """what the entries that read the matrix answer on h, from a fresh factorization of the start basis on: the factors,
    the spike of the last column with entries, a tableau row, a price, and the two batch entries with n == 1"""
    j = max(c for c in range(ncol) if a[0][c + 1] > a[0][c])
    y = MX.price_vectors(m)[0]
    out = [h.factorize_columns(basis)]
    f = h.get_factors()
    out += [f[k] for k in sorted(f)]
    out += [h.solve_for_update_column(j)] + list(MX.solution(h))
    st, alpha = h.tableau_row(m // 2, False, isbasic, want_solution=True)
    out += [st, alpha] + list(MX.solution(h))
    out.append(h.price(y, None))
    sts, al = blu_amd.tableau_row_batch([h], [1], False, [isbasic], want_solution=True)
    out += [sts[0], al[0]] + list(MX.solution(h))
    sts, zs = blu_amd.price_batch([h], [y], [isbasic])
    out += [sts[0], zs[0]]
    return out


def same_answers(x, y, what):
    assert len(x) == len(y), what
    for k, (u, v) in enumerate(zip(x, y)):
        if isinstance(u, np.ndarray) and u.dtype == np.float64:
            assert MX.same_bits(u, v), (what, k)
        else:
            assert np.array_equal(u, v), (what, k)


def matrix_entries(h, m, ncol):
    """the statuses of the entries that need a matrix, through the C ABI (a refusal does not raise)"""
    L = blu_amd.lib()
    L.blu_hip_factorize_columns.argtypes = [C.c_void_p, C.c_void_p]
    L.blu_hip_solve_for_update_column.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3
    L.blu_hip_tableau_row.argtypes = [C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 5
    L.blu_hip_price.argtypes = [C.c_void_p] * 4
    b = np.arange(m, dtype=np.int64)
    y, al = np.zeros(max(m, 1)), np.zeros(max(ncol, 1))
    return [L.blu_hip_factorize_columns(h._h, b.ctypes.data), L.blu_hip_solve_for_update_column(h._h, 0, None, None, None),
            L.blu_hip_tableau_row(h._h, 0, 0, None, al.ctypes.data, None, None, None), L.blu_hip_price(h._h, y.ctypes.data, None, al.ctypes.data)]


def check_sharing(name):
    m, ncol, a, g, basis, isbasic = new_root(name)
    twin = blu_amd.BLU(m, len(a[1]))  # called set_matrix itself
    assert twin.set_matrix(ncol, *a) == K.OK
    y = MX.price_vectors(m)[0]
    z_full = MX.at_dot(a[0], a[1], a[2], y)
    ncol2, a2 = sub_matrix(a, ncol)
    z_sub = MX.at_dot(a2[0], a2[1], a2[2], y)
    kids = [blu_amd.BLU(m, 8) for _ in range(9)]
    assert blu_amd.copy_batch(g, kids) == [K.OK] * 9
    assert all(k.dbg_matrix_holders() == 0 for k in kids) and g.dbg_matrix_holders() == 1 and twin.dbg_matrix_holders() == 1
    assert blu_amd.share_matrix(g, kids) == [K.OK] * 9
    assert [h.dbg_matrix_holders() for h in [g] + kids] == [10] * 10
    want = answers(twin, a, m, ncol, basis, isbasic)
    same_answers(answers(g, a, m, ncol, basis, isbasic), want, "root")
    for k, h in enumerate(kids):
        same_answers(answers(h, a, m, ncol, basis, isbasic), want, ("child", k))

    # ---- the root is freed: the children go on
    g.close()
    assert [h.dbg_matrix_holders() for h in kids] == [9] * 9
    same_answers(answers(kids[8], a, m, ncol, basis, isbasic), want, "child after the root was freed")

    # ---- set_matrix on one holder: a matrix of its own, the others keep the old one
    assert kids[0].set_matrix(ncol2, *a2) == K.OK
    assert kids[0].dbg_matrix_holders() == 1 and [h.dbg_matrix_holders() for h in kids[1:]] == [8] * 8
    assert MX.same_bits(kids[0].price(y), z_sub)
    t2 = blu_amd.BLU(m, len(a[1]))
    assert t2.set_matrix(ncol2, *a2) == K.OK
    same_answers(answers(kids[0], a2, m, ncol2, basis, isbasic[:ncol2]), answers(t2, a2, m, ncol2, basis, isbasic[:ncol2]), "child with a new matrix")
    same_answers(answers(kids[1], a, m, ncol, basis, isbasic), want, "child beside a set_matrix")

    # ---- maxvolume on one holder: it loses the matrix, the others are untouched
    b2, i2 = MV.start(m, ncol)
    assert kids[1].maxvolume(ncol, a[0], a[1], a[2], b2, i2, 1e300)[0] == K.OK  # (a pass that takes no candidate)
    assert matrix_entries(kids[1], m, ncol) == [INVCALL] * 4
    assert kids[1].dbg_matrix_holders() == 0 and [h.dbg_matrix_holders() for h in kids[2:]] == [7] * 7
    same_answers(answers(kids[2], a, m, ncol, basis, isbasic), want, "child beside a maxvolume")

    # ---- sharing into a handle that has a matrix of its own, a shared one, or the buffers maxvolume left
    assert blu_amd.share_matrix(kids[2], [kids[0], kids[1]]) == [K.OK] * 2
    assert [h.dbg_matrix_holders() for h in kids] == [9] * 9
    (x,) = fork(t2)  # holds t2's matrix
    assert t2.dbg_matrix_holders() == x.dbg_matrix_holders() == 2
    assert blu_amd.share_matrix(kids[8], [x, kids[3]]) == [K.OK] * 2  # (kids[3] holds it already)
    assert t2.dbg_matrix_holders() == 1 and [h.dbg_matrix_holders() for h in kids + [x]] == [10] * 10
    assert MX.same_bits(t2.price(y), z_sub)
    for h in (kids[0], kids[1], x):
        same_answers(answers(h, a, m, ncol, basis, isbasic), want, "shared into a handle that had a matrix")

    # ---- copy_batch in either role disturbs no holder and copies no matrix
    plain = blu_amd.BLU(m, 8)
    assert blu_amd.copy_batch(kids[4], [kids[5], plain]) == [K.OK] * 2
    assert plain.dbg_matrix_holders() == 0 and matrix_entries(plain, m, ncol) == [INVCALL] * 4
    assert [h.dbg_matrix_holders() for h in kids + [x]] == [10] * 10
    same_answers(answers(kids[5], a, m, ncol, basis, isbasic), want, "a copy_batch destination keeps the shared matrix")
    same_answers(answers(kids[4], a, m, ncol, basis, isbasic), want, "a copy_batch source keeps the shared matrix")

    # ---- refusals as a whole: every status carries the code, nothing is touched
    L = blu_amd.lib()
    SHARE = L.blu_hip_share_matrix
    SHARE.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    other_m = blu_amd.BLU(m + 1, 8)

    def refused(src, dsts, code, n=None):
        arr = (C.c_void_p * max(len(dsts), 1))(*[None if h is None else h._h for h in dsts])
        st = (C.c_int * max(len(dsts), 1))(*([77] * max(len(dsts), 1)))
        before = [h.dbg_matrix_holders() for h in kids + [x, t2, plain]]
        assert SHARE(None if src is None else src._h, arr, len(dsts) if n is None else n, st) == code
        if n is None:
            assert list(st)[:len(dsts)] == [code] * len(dsts), (code, list(st))
        assert [h.dbg_matrix_holders() for h in kids + [x, t2, plain]] == before, code
        assert MX.same_bits(t2.price(y), z_sub) and MX.same_bits(kids[6].price(y), z_full), code

    refused(None, [t2], MISS)
    refused(kids[6], [t2, None], MISS)
    refused(kids[6], [t2], MISS, n=-1)
    assert SHARE(kids[6]._h, None, 1, None) == MISS
    refused(plain, [t2], INVCALL)
    refused(kids[6], [t2, kids[6]], INVARG)
    refused(kids[6], [t2, plain, t2], INVARG)
    refused(kids[6], [t2, other_m], INVARG)
    arr = (C.c_void_p * 1)(t2._h)
    assert SHARE(kids[6]._h, arr, 0, None) == K.OK and t2.dbg_matrix_holders() == 1  # n == 0
    assert SHARE(kids[6]._h, arr, 1, None) == K.OK and t2.dbg_matrix_holders() == 11  # status may be NULL
    for bad in (lambda: blu_amd.share_matrix(plain, [other_m]), lambda: blu_amd.share_matrix(kids[6], [kids[6]])):
        try:
            bad()
        except blu_amd.BluError:
            continue
        raise AssertionError("a refused share_matrix raises")
    close_all(kids + [x, t2, plain, other_m, twin])


def members_at_different_points(name, n):
    """n holders of one matrix, clones of one root taken after 0, 1, 2 and 3 updates made through util_matrix.update_pair,
    each with the isbasic of its point: (m, ncol, a, members, isbasics, keep)"""
    m, ncol, a, g, basis, isbasic = new_root(name)
    s = blu_amd.BLU(m, len(a[1]))
    assert s.factorize(*MX.gathered(a, basis)) == K.OK
    members, isb = [None] * n, [None] * n
    for stage in range(4):
        ks = [k for k in range(n) if k % 4 == stage]
        if not ks:
            break
        if stage:
            MX.update_pair(g, s, a, basis, isbasic, 1, ("stage", stage))
        for k, h in zip(ks, fork(g, len(ks))):
            members[k], isb[k] = h, list(isbasic)
    s.close()
    return m, ncol, a, members, isb, g


def skips_of(mode, isb):
    if mode == "none":
        return None
    if mode == "isbasic":
        return isb
    return [None if k % 3 == 0 else ([1] * len(sk) if k % 3 == 1 else sk) for k, sk in enumerate(isb)]  # mixed per member


def forward_solves(hs, a, isb):
    """a pending forward solve_for_update on every handle: the spike of its last nonbasic column with entries; returns
    the leaving rows and pivots (util_matrix.pick_leaving)"""
    ncol = len(a[0]) - 1
    rows, xtbl = [], []
    for h, sk in zip(hs, isb):
        j = max(c for c in range(ncol) if not sk[c] and a[0][c + 1] > a[0][c])
        assert h.solve_for_update_column(j) == K.OK
        p, x = MX.pick_leaving(h)
        rows.append(p)
        xtbl.append(x)
    return rows, xtbl


def rows_of_call(a, m, hs, isb, prep):
    """the rows of one call: with prep the forward solves on hs first and the leaving rows they pick (with the pivots)"""
    if prep:
        return forward_solves(hs, a, isb)
    return [(3 * k + 1) % m for k in range(len(hs))], None


def check_one_call(a, m, members, isb, mode, prep, want):
    """one tableau_row_batch over forks of `members` beside the single tableau_row on a second set of forks; with prep the
    forward solves first and update_batch / update afterwards.  Returns the alphas and the counts of the call."""
    n = len(members)
    B = [fork(h)[0] for h in members]
    S = [fork(h)[0] for h in members]
    rows, xtbl = rows_of_call(a, m, B, isb, prep)
    assert rows_of_call(a, m, S, isb, prep) == (rows, xtbl)
    skips = skips_of(mode, isb)
    sts, al = blu_amd.tableau_row_batch(B, rows, prep, skips, want_solution=want)
    counts = B[0].dbg_matrix_counts()
    for k in range(n):
        what = (mode, prep, want, "member", k)
        sk = None if skips is None else skips[k]
        st, single = S[k].tableau_row(rows[k], prep, sk, want_solution=True)
        assert sts[k] == st == K.OK, (what, sts[k], st)
        assert MX.same_bits(al[k], single), (what, "the single entry", np.flatnonzero(al[k] != single)[:5])
        assert MX.same_bits(al[k], MX.at_dot(a[0], a[1], a[2], S[k].lhs, sk)), (what, "at_dot of the single solve's y")
        if sk is not None:
            assert not np.any(al[k].view(np.uint64)[np.asarray(sk) != 0]), (what, "skipped entries are +0.0")
        if want:
            assert MX.same_solution(MX.solution(B[k]), MX.solution(S[k])), (what, "solution")
        for key in MX.FLOPS:
            assert B[k].stat(key) == S[k].stat(key), (what, "statistic", key)
    if prep:
        assert blu_amd.update_batch(B, xtbl) == [h.update(x) for h, x in zip(S, xtbl)]
    for k in range(n):
        MX.same_handles(B[k], S[k], a, (mode, prep, want, "afterwards", k))
    close_all(B + S)
    return al, counts


def call_again(a, m, members, isb, mode, prep, order, chunk_bytes):
    """the same call on fresh forks, the handle list in another order or the chunk limit forced: (alphas in member
    order, counts)"""
    n = len(members)
    B = [fork(h)[0] for h in members]
    rows, _ = rows_of_call(a, m, B, isb, prep)
    skips = skips_of(mode, isb)
    assert B[0].dbg_set_matrix_batch_bytes(chunk_bytes) == K.OK
    sts, al = blu_amd.tableau_row_batch([B[k] for k in order], [rows[k] for k in order], prep,
                                        None if skips is None else [skips[k] for k in order])
    counts = B[order[0]].dbg_matrix_counts()
    assert B[0].dbg_set_matrix_batch_bytes(-1) == K.OK
    assert sts == [K.OK] * n
    alphas = [None] * n
    for pos, k in enumerate(order):
        alphas[k] = al[pos]
    close_all(B)
    return alphas, counts


def check_rows(name, n, modes=("none", "isbasic", "mixed")):
    m, ncol, a, members, isb, g = members_at_different_points(name, n)
    assert members[0].dbg_matrix_holders() == n + 1
    perm = list(np.random.default_rng(n).permutation(n))
    for prep in (False, True):
        for mode in modes:
            want = mode != "isbasic"
            al, counts = check_one_call(a, m, members, isb, mode, prep, want)
            groups_skip = mode != "none" and (mode == "isbasic" or n > 1)
            assert counts == (2, 1, 1 + (1 if groups_skip else 0), 8 * n * ncol), (mode, prep, counts)
            if mode != "mixed":
                continue
            al2, _ = call_again(a, m, members, isb, mode, prep, perm, -1)
            al3, counts = call_again(a, m, members, isb, mode, prep, list(range(n)), 1)  # one group per chunk
            chunks = (n + 7) // 8
            assert counts[:2] == (2 * chunks, chunks) and counts[3] == 8 * n * ncol, counts
            for k in range(n):
                assert MX.same_bits(al[k], al2[k]), ("permuted", prep, k)
                assert MX.same_bits(al[k], al3[k]), ("chunked", prep, k)
    close_all(members + [g])


def check_rows_rank_deficient(name="M0"):
    """a member factorized on a basis with a column twice beside regular members: the batch gives what the single entry
    gives, whatever that is"""
    m, ncol, a, g, basis, isbasic = new_root(name)
    d = fork(g)[0]
    twice = list(basis)
    twice[1] = twice[0]
    st = d.factorize_columns(twice)
    assert st != K.OK  # (the factorization reports the deficiency)
    hs = fork(g, 3) + [d]
    singles = [fork(h)[0] for h in hs]
    rows = [1, 0, m - 1, 1]
    sts, al = blu_amd.tableau_row_batch(hs, rows, False, None, want_solution=True)
    for k, s in enumerate(singles):
        st1, single = s.tableau_row(rows[k], False, None, want_solution=True)
        assert sts[k] == st1 and MX.same_bits(al[k], single), ("rank-deficient", k, sts[k], st1)
        if st1 == K.OK:
            assert MX.same_solution(MX.solution(hs[k]), MX.solution(s)), k
            MX.same_handles(hs[k], s, a, ("rank-deficient", k))
    close_all(hs + singles + [g])


def check_rows_bad_members(name):
    """an out-of-range row, a member without a factorization, one without a matrix: each its own status, the others their
    rows; then the refusals of the call as a whole"""
    m, ncol, a, g, basis, isbasic = new_root(name)
    for prep in (False, True):
        good = fork(g, 9)
        nofact = blu_amd.BLU(m, 8)
        assert blu_amd.share_matrix(g, [nofact]) == [K.OK]
        nomat = g.clone()
        hs = good[:3] + [nofact] + good[3:6] + [nomat] + good[6:]
        rows = [(5 * k + 2) % m for k in range(len(hs))]
        rows[1] = m
        rows[9] = -1
        S = [fork(h)[0] if h.dbg_matrix_holders() else h.clone() for h in hs]
        sts, al = blu_amd.tableau_row_batch(hs, rows, prep, [isbasic if h.dbg_matrix_holders() else None for h in hs], want_solution=True)
        for k, s in enumerate(S):
            st, single = s.tableau_row(rows[k], prep, isbasic if s.dbg_matrix_holders() else None, want_solution=True)
            assert sts[k] == st, (prep, k, sts[k], st)
            if st == K.OK:
                assert MX.same_bits(al[k], single), (prep, k)
                assert MX.same_solution(MX.solution(hs[k]), MX.solution(s)), (prep, k)
        assert [sts[k] for k in (1, 3, 7, 9)] == [INVARG, INVCALL, INVCALL, INVARG] and sts.count(K.OK) == len(hs) - 4, sts
        for k in (0, 2, 4, 10):
            MX.same_handles(hs[k], S[k], a, ("beside refused members", prep, k))
        close_all(hs + S)

    # ---- refused as a whole
    L = blu_amd.lib()
    ROWS, PRICE = L.blu_hip_tableau_row_batch, L.blu_hip_price_batch
    ROWS.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    PRICE.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
    k1, k2 = fork(g, 2)
    own = blu_amd.BLU(m, len(a[1]))  # the same arrays, but a matrix of its own
    assert own.set_matrix(ncol, *a) == K.OK and own.factorize_columns(basis) == K.OK
    y = MX.price_vectors(m)[0]
    z_full = MX.at_dot(a[0], a[1], a[2], y)
    stats = [[h.stat(key) for key in MV.STATS] for h in (k1, k2, own)]

    def call(hs, code, n=None, r=True, alpha=True, null_alpha=None, ys=True, what="rows"):
        N = len(hs)
        arr = (C.c_void_p * N)(*[None if h is None else h._h for h in hs])
        rr = (C.c_int64 * N)(*([0] * N))
        outs = [np.zeros(ncol) for _ in range(N)]
        pa = (C.c_void_p * N)(*[None if k == null_alpha else o.ctypes.data for k, o in enumerate(outs)])
        py = (C.c_void_p * N)(*[y.ctypes.data] * N)
        st = (C.c_int * N)(*([77] * N))
        cnt = N if n is None else n
        if what == "rows":
            rc = ROWS(arr, cnt, rr if r else None, 0, None, pa if alpha else None, None, None, None, st)
        else:
            rc = PRICE(arr, cnt, py if ys else None, None, pa if alpha else None, st)
        assert rc == code, (what, rc, code)
        if n is None:
            assert list(st) == [code] * N, (what, code, list(st))
        assert [[h.stat(key) for key in MV.STATS] for h in (k1, k2, own)] == stats, (what, code)

    for what in ("rows", "price"):
        call([k1, None], MISS, what=what)
        call([k1, k2], MISS, n=-1, what=what)
        call([k1, k2], MISS, alpha=False, what=what)
        call([k1, k2], MISS, null_alpha=1, what=what)
        call([k1, k2, k1], INVARG, what=what)
        call([k1, own], INVARG, what=what)  # two matrices
        call([k1, k2], K.OK, n=0, what=what)
    call([k1, k2], MISS, r=False)
    call([k1, k2], MISS, ys=False, what="price")
    assert ROWS(None, 1, None, 0, None, None, None, None, None, None) == MISS and PRICE(None, 1, None, None, None, None) == MISS
    # one unshared handle is fine
    sts, al = blu_amd.tableau_row_batch([own], [2], False, [isbasic])
    st, single = k1.tableau_row(2, False, isbasic)
    assert sts == [K.OK] and st == K.OK and MX.same_bits(al[0], single)
    sts, zs = blu_amd.price_batch([own], [y])
    assert sts == [K.OK] and MX.same_bits(zs[0], z_full) and own.dbg_matrix_holders() == 1
    for bad in (lambda: blu_amd.tableau_row_batch([k1, own], [0, 0]), lambda: blu_amd.price_batch([k1, own], [y, y]),
                lambda: blu_amd.tableau_row_batch([k1, k1], [0, 0])):
        try:
            bad()
        except blu_amd.BluError:
            continue
        raise AssertionError("a refused batch call raises")
    close_all([k1, k2, own, g])


def check_pricing():
    """price_batch against at_dot for the vectors of util_matrix.price_vectors and a NaN, skips mixed per member; nothing
    observable changes; the counts of both entries do not depend on n within a chunk nor on the matrix"""
    seen = {}
    for name in ("M0", "M1"):
        m, ncol, a, g, basis, isbasic = new_root(name)
        hs = [g] + fork(g, 16)
        nofact = blu_amd.BLU(m, 8)  # pricing needs no factorization
        assert blu_amd.share_matrix(g, [nofact]) == [K.OK]
        hs.append(nofact)
        n = len(hs)
        y, z = MX.price_vectors(m)
        ys = [(y if k % 2 else z) * (1.0 + k) for k in range(n)]
        ys[5] = ys[5].copy()
        ys[5][m // 2] = np.nan
        skips = skips_of("mixed", [isbasic] * n)
        before = [[h.stat(key) for key in MV.STATS] for h in hs]
        for sk in (None, skips, [isbasic] * n):
            sts, zs = blu_amd.price_batch(hs, ys, sk)
            assert sts == [K.OK] * n
            for k in range(n):
                want = MX.at_dot(a[0], a[1], a[2], ys[k], None if sk is None else sk[k])
                if k == 5:
                    assert np.array_equal(zs[k], want, equal_nan=True), (name, "price with a NaN", sk is None)
                    assert sk is None or sk[k] is None or not np.any(zs[k].view(np.uint64)[np.asarray(sk[k]) != 0])
                else:
                    assert MX.same_bits(zs[k], want), (name, "price", k, sk is None)
                    assert MX.same_bits(zs[k], hs[k].price(ys[k], None if sk is None else sk[k])), (name, "the single entry", k)
        after = [[h.stat(key) for key in MV.STATS] for h in hs]
        assert np.array_equal(before, after, equal_nan=True), name
        # the same bits in three chunks and in another order
        ref = blu_amd.price_batch(hs, ys, skips)[1]
        assert g.dbg_set_matrix_batch_bytes(1) == K.OK
        perm = list(np.random.default_rng(3).permutation(n))
        sts, zs = blu_amd.price_batch([hs[k] for k in perm], [ys[k] for k in perm], [skips[k] for k in perm])
        uploads = sum(1 + any(skips[k] is not None for k in perm[c:c + 8]) for c in range(0, n, 8))  # y tiles, masks if any
        assert hs[perm[0]].dbg_matrix_counts() == (3, 3, uploads, 8 * n * ncol)
        assert g.dbg_set_matrix_batch_bytes(-1) == K.OK
        for pos, k in enumerate(perm):
            assert np.array_equal(zs[pos].view(np.uint64), ref[k].view(np.uint64)), (name, "chunked and permuted", k)
        # the cost of the part behind the solves
        fact = hs[:-1]
        for cnt in GROUP_SIZES:
            for with_skip in (False, True):
                sk = [isbasic] * cnt if with_skip else None
                blu_amd.price_batch(fact[:cnt], ys[:cnt], sk)
                c = fact[0].dbg_matrix_counts()
                assert c == (1, 1, 1 + with_skip, 8 * cnt * ncol), (name, "price", cnt, c)
                assert blu_amd.tableau_row_batch(fact[:cnt], [1] * cnt, False, sk)[0] == [K.OK] * cnt
                r = fact[0].dbg_matrix_counts()
                assert r == (2, 1, 1 + with_skip, 8 * cnt * ncol), (name, "rows", cnt, r)
                seen.setdefault((cnt, with_skip), []).append((c[:3], r[:3]))
        close_all(hs)
    assert all(len(v) == 2 and v[0] == v[1] for v in seen.values()), seen  # the same for both matrices
