"""Shared by the tests of the ratio test on the device (blu_hip_set_duals, _get_duals, _get_ratio_row, _ratio_test,
_update_duals, _copy_duals_batch, _ratio_test_batch, _update_duals_batch): the selection rule and the dual step of the
contract restated in numpy (ratio_pick, duals_step -- they are the specification), the matrices, the cases, and the drivers
that run handles through the new entries beside clones driven by the existing single entries.  Equalities of bits and of
integers only.  The library is the one blu_amd loads: the emulation build in the child processes of
tests/test_emu_cpu_ratio.py, the default one in tests/test_gpu_ratio.py."""
import ctypes as C

import numpy as np

import blu_amd
from blu_amd import keys as K
from tests import util_matrix as MX
from tests import util_matrix_batch as MB
from tests import util_maxvolume as MV

INVARG, MISS, INVCALL = K.ERROR_INVALID_ARGUMENT, K.ERROR_ARGUMENT_MISSING, K.ERROR_INVALID_CALL
NONE = (-1, 0, 0.0, 0.0, 0.0, 0.0)


def ratio_pick(alpha, d, kind, sigma, pivtol, dualtol, details=False):
    """The selection rule: (q, ncand, alpha_q, d_q, step_q, theta).  alpha is the tableau row; where kind == 0 it counts as
    +0.0.  With details also the candidate mask, the pool mask, step and a."""
    kind = np.asarray(kind, np.int64)
    d = np.asarray(d, np.float64)
    alpha = np.where(kind == 0, 0.0, np.asarray(alpha, np.float64))
    with np.errstate(all="ignore"):
        a = np.abs(alpha)
        s = np.float64(sigma) * alpha
        cand = ((kind == 1) & (s > pivtol)) | ((kind == -1) & (s < -pivtol)) | ((kind == 2) & (a > pivtol))
        bound = (np.abs(d) + np.float64(dualtol)) / a
        step = np.abs(d) / a
        cand = cand & ~np.isnan(bound)
        ncand = int(cand.sum())
        pool = np.zeros(len(a), bool)
        rec = NONE
        if ncand:
            theta = bound[cand].min()
            pool = cand & (step <= theta)
            assert pool.any()  # (rounding is monotone: the minimizer of the bound is in it)
            q = int(np.flatnonzero(pool & (a == a[pool].max()))[0])
            rec = (q, ncand, float(alpha[q]), float(d[q]), float(step[q]), float(theta))
    return (rec, cand, pool, step, a) if details else rec


def duals_step(d, kind, row, theta, jset=(), dset=(), kset=()):
    """The dual step: d[j] - theta * row[j] where kind[j] != 0 (the product rounded once, then the difference), then the
    overrides.  Returns (d, kind)."""
    d, kind = np.array(d, np.float64), np.array(kind, np.int8)
    nz = kind != 0
    with np.errstate(all="ignore"):
        t = np.float64(theta) * np.asarray(row, np.float64)[nz]
        d[nz] = d[nz] - t
    for j, x, k in zip(jset, dset, kset):
        d[j], kind[j] = x, k
    return d, kind


def same_record(x, y):
    return x is not None and y is not None and x[:2] == y[:2] and MX.same_bits(x[2:], y[2:])


def m2():
    """util_matrix.m1() plus 800 columns: appended column t copies column 200 + t % 131, negated when (t // 131) % 2 == 1.
    ncol = 1131 is more than any workgroup size and no multiple of 64; the copies are exact twins of short and long
    (> 64 entries) columns, so their alpha are bit-equal or bit-negated and ties on |alpha| exist by construction."""
    m, ncol, (a_p, a_i, a_x) = MX.m1()
    p, i, x = [int(v) for v in a_p], [a_i], [a_x]
    for t in range(800):
        src = 200 + t % 131
        b, e = int(a_p[src]), int(a_p[src + 1])
        i.append(a_i[b:e])
        x.append(-a_x[b:e] if (t // 131) % 2 == 1 else a_x[b:e])
        p.append(p[-1] + e - b)
    return m, ncol + 800, (np.array(p, np.uint64), np.concatenate(i), np.concatenate(x))


def twins_hold(name, alpha):
    """the appended columns' alpha are the bits of their originals, or those negated"""
    if name != "M2":
        return
    for t in range(800):
        want = alpha[200 + t % 131]
        if want == 0.0:  # (a sum that starts at +0.0 has no -0.0 for a twin)
            assert alpha[331 + t] == 0.0, ("twin", t)
            continue
        assert MX.same_bits(alpha[331 + t], -want if (t // 131) % 2 == 1 else want), ("twin", t)


MATRICES = {"M0": MX.m0, "M2": m2}
STRIDES = (256, 1024)  # the workgroups of the batched and of the single pick


def new_root(name):
    m, ncol, a = MATRICES[name]()
    g = blu_amd.BLU(m, len(a[1]))
    assert g.set_matrix(ncol, *a) == K.OK
    basis, isbasic = MV.start(m, ncol)
    assert g.factorize_columns(basis) == K.OK
    return m, ncol, a, g, basis, isbasic


def full_row(h, a, r, prep=False):
    """the reference alpha of row r (nothing skipped): at_dot of a clone's solve_sparse([r], [1.0], 'T') solution -- with
    prep of its transposed solve_for_update([r]), the solve a ratio test with prepare_update makes; also the clone, which
    then stands where a handle stands after the solve of a ratio test"""
    c = h.clone()
    assert (c.solve_for_update([r], None, "T", True) if prep else c.solve_sparse([r], [1.0], "T")) == K.OK
    return MX.at_dot(a[0], a[1], a[2], c.lhs), c


def find_row(h, a, m, ncol, start=0):
    """a row whose alpha has entries at column ncol - 1 and at six columns or more, both signs among them"""
    ci, _ = MX.column(a, ncol - 1)
    first = [int(i) for i in ci]
    for r in first[start % len(first):] + first[:start % len(first)] + [(start + k) % m for k in range(m)]:
        alpha, c = full_row(h, a, r)
        c.close()
        nz = np.flatnonzero(alpha)
        if alpha[ncol - 1] != 0.0 and len(nz) >= 6 and (alpha > 0).sum() >= 3 and (alpha < 0).sum() >= 3:
            return r, alpha
    raise AssertionError("no row fits the cases")


def cases(name, alpha, seed=0):
    """[(label, d, kind, sigma, pivtol, dualtol)] for a row with the reference alpha; every case asserts on the restatement
    that it shows its property, so none is vacuous.  (a) to (h) as the tests' docstrings list them."""
    ncol = len(alpha)
    rng = np.random.default_rng(seed)
    a = np.abs(alpha)
    by_sign = np.where(alpha > 0, 1, np.where(alpha < 0, -1, 0)).astype(np.int8)  # with sigma = +1 every nonzero is a candidate
    out = []

    def add(label, d, kind, sigma=1.0, pivtol=0.0, dualtol=0.0):
        out.append((label, np.array(d, np.float64), np.array(kind, np.int8), sigma, pivtol, dualtol))
        return ratio_pick(alpha, d, kind, sigma, pivtol, dualtol, details=True)

    # (a) a unique minimum ratio
    d_a = rng.uniform(1.0, 2.0, ncol) * a
    rec_a, cand, pool, step, _ = add("a unique", d_a, by_sign)
    assert rec_a[0] >= 0 and pool.sum() == 1 and (step[cand] == step[cand].min()).sum() == 1
    # (b) equal ratios decided by |alpha|: step == 2.0 exactly (without the appended twins)
    k_b = by_sign.copy()
    k_b[331:] = 0
    rec, cand, pool, step, aa = add("b by size", 2.0 * a, k_b)
    assert cand.sum() >= 3 and np.all(step[cand] == 2.0) and np.array_equal(pool, cand) and (aa[pool] == aa[pool].max()).sum() == 1
    # (c) equal ratio and equal |alpha|: the smallest index (the twins)
    if name == "M2":
        k_c = by_sign.copy()
        k_c[:331] = 0  # (only appended columns: every column has a copy 262 behind it or before it)
        rec, cand, pool, step, aa = add("c twins", 2.0 * a, k_c)
        tie = np.flatnonzero(pool & (aa == aa[pool].max()))
        assert len(tie) >= 2 and rec[0] == tie[0] and np.all(step[cand] == 2.0)
    # (d) no candidate
    rec, *_ = add("d all kind 0", d_a, np.zeros(ncol, np.int8))
    assert rec == NONE
    rec, *_ = add("d pivtol above all", d_a, by_sign, pivtol=2.0 * a.max())
    assert rec == NONE
    # (e) a dualtol that changes the winner
    nz = np.flatnonzero(alpha)
    j1, j2 = nz[np.argmin(a[nz])], nz[np.argmax(a[nz])]
    assert a[j1] < a[j2] and a[j1] <= 1000.0
    d_e = 1e3 * a
    d_e[j1], d_e[j2] = 0.0, 1e-9 * a[j2]
    rec0, *_ = add("e dualtol 0", d_e, by_sign)
    rec1, *_ = add("e dualtol", d_e, by_sign, dualtol=1e-6)
    assert rec0[0] == j1 and rec1[0] == j2
    # (f) the winner in the first stride, in the last partial stride, at column ncol - 1
    last = max(((ncol - 1) // s) * s for s in STRIDES if s < ncol) if ncol > min(STRIDES) else 0
    mid = last + int(np.argmax(a[last:ncol - 1]))
    for label, j in (("f first stride", int(nz[0])), ("f last stride", mid), ("f last column", ncol - 1)):
        assert alpha[j] != 0.0 and (label != "f first stride" or j < min(STRIDES)), (label, j)
        d_f = 5.0 * a
        d_f[j] = 0.0
        rec, *_ = add(label, d_f, by_sign)
        assert rec[0] == j
    # (g) both signs of sigma, all four kinds
    k_g = np.zeros(ncol, np.int8)
    for idx in (np.flatnonzero(alpha > 0), np.flatnonzero(alpha < 0)):
        k_g[idx[0::3]], k_g[idx[1::3]], k_g[idx[2::3]] = 1, -1, 2
    k_g[np.flatnonzero(alpha > 0)[2]] = 0  # (a column with an entry that is no candidate for its kind)
    d_g = rng.standard_normal(ncol)
    for sigma in (1.0, -1.0):
        rec, cand, *_ = add("g sigma %+d" % sigma, d_g, k_g, sigma=sigma, pivtol=1e-12, dualtol=1e-9)
        assert all((cand & (k_g == k)).any() for k in (1, -1, 2)) and not cand[k_g == 0].any() and (~cand & (k_g == 1)).any()
    # (h) a NaN in d on the column that would otherwise win
    d_h = d_a.copy()
    d_h[rec_a[0]] = np.nan
    rec, *_ = add("h NaN", d_h, by_sign)
    assert rec[0] not in (-1, rec_a[0]) and rec[1] == rec_a[1] - 1
    return out


def pick_of(alpha, case):
    _, d, kind, sigma, pivtol, dualtol = case
    return ratio_pick(alpha, d, kind, sigma, pivtol, dualtol)


def kept(alpha, kind):
    return np.where(np.asarray(kind) == 0, 0.0, alpha)


def update_through_ratio_test(g, s, a, basis, isbasic, nupdates, what):
    """nupdates basis changes: g through ratio_test(p, prepare_update) + solve_for_update_column(q) + update +
    update_duals, the twin s through the existing single entries; every piece is compared on the way"""
    m, ncol = g.m, len(a[0]) - 1
    done = 0
    for p in range(m):
        if done == nupdates:
            break
        alpha, c = full_row(g, a, p, prep=True)
        c.close()
        nonbasic = np.asarray(isbasic) == 0
        if np.abs(alpha[nonbasic]).max() < 0.05:
            continue
        kind = np.where(nonbasic, np.where(alpha >= 0, 1, -1), 0).astype(np.int8)
        d = 2.0 * np.abs(alpha) + 1.0 * (alpha == 0)
        assert g.set_duals(d, kind) == K.OK
        want = ratio_pick(alpha, d, kind, 1.0, 1e-9, 0.0)
        st, rec = g.ratio_test(p, 1.0, 1e-9, 0.0, prepare_update=True, want_solution=True)
        assert st == s.solve_for_update([p], None, "T", True) == K.OK, (what, p, st)
        assert g.dbg_matrix_counts() == (3, 1, 0, 64), (what, g.dbg_matrix_counts())
        assert MX.same_solution(MX.solution(g), MX.solution(s)), (what, "row solve", p)
        assert same_record(rec, want), (what, "record", p, rec, want)
        st, row = g.ratio_row()
        assert st == K.OK and MX.same_bits(row, kept(alpha, kind)), (what, "kept row", p)
        q = rec[0]
        assert g.solve_for_update_column(q) == s.solve_for_update(*MX.column(a, q), "N", True) == K.OK, (what, q)
        assert MX.same_solution(MX.solution(g), MX.solution(s)), (what, "spike solve", q)
        xtbl = float(g.lhs[p])
        assert g.update(xtbl) == s.update(xtbl) == K.OK, (what, "update", q, p)
        theta, leave = rec[4], basis[p]
        assert g.update_duals(theta, [q, leave], [0.0, -theta], [0, 1]) == K.OK
        st, d1, k1 = g.get_duals()
        d2, k2 = duals_step(d, kind, row, theta, [q, leave], [0.0, -theta], [0, 1])
        assert st == K.OK and MX.same_bits(d1, d2) and np.array_equal(k1, k2), (what, "dual step", p)
        isbasic[leave], isbasic[q], basis[p] = 0, 1, q
        done += 1
    assert done == nupdates, (what, done)
    MX.same_handles(g, s, a, what)


def check_single(name, nupdates):
    """the single entry on a fresh factorization (nupdates == 0) or after updates made through it"""
    m, ncol, a, g, basis, isbasic = new_root(name)
    s = blu_amd.BLU(m, len(a[1]))
    assert s.factorize(*MX.gathered(a, basis)) == K.OK
    update_through_ratio_test(g, s, a, basis, isbasic, nupdates, (name, nupdates))
    r, alpha = find_row(g, a, m, ncol)
    twins_hold(name, alpha)
    labels = set()
    for ci, case in enumerate(cases(name, alpha, seed=nupdates)):
        label, d, kind, sigma, pivtol, dualtol = case
        what = (name, nupdates, label)
        labels.add(label[0])
        # d and kind go up together, or one after the other
        if ci % 2:
            assert g.set_duals(d, None) == K.OK and g.set_duals(None, kind) == K.OK
        else:
            assert g.set_duals(d, kind) == K.OK
        (t,) = MB.fork(g)
        c = g.clone()
        st, rec = g.ratio_test(r, sigma, pivtol, dualtol, want_solution=True)
        assert st == c.solve_sparse([r], [1.0], "T") == s.solve_sparse([r], [1.0], "T") == K.OK, what
        assert g.dbg_matrix_counts() == (3, 1, 0, 64), (what, g.dbg_matrix_counts())
        assert same_record(rec, pick_of(alpha, case)), (what, rec, pick_of(alpha, case))
        assert MX.same_solution(MX.solution(g), MX.solution(c)), (what, "solution")
        for key in MX.FLOPS:
            assert g.stat(key) == c.stat(key), (what, "statistic", key)
        st, row = g.ratio_row()
        st2, al = t.tableau_row(r, False, (kind == 0).astype(np.int64))
        assert st == st2 == K.OK and MX.same_bits(row, al) and MX.same_bits(row, kept(alpha, kind)), (what, "kept row")
        # tableau_row and price write mx_out: the kept row stays
        assert g.tableau_row((r + 1) % m)[0] == s.solve_sparse([(r + 1) % m], [1.0], "T") == K.OK
        g.price(MX.price_vectors(m)[0])
        assert MX.same_bits(g.ratio_row()[1], row), (what, "kept row behind tableau_row and price")
        # the dual step from the kept row
        theta = rec[4] if rec[0] >= 0 else 0.25
        sets = ([rec[0], ncol - 1], [0.0, -1.5], [0, 2]) if rec[0] not in (-1, ncol - 1) else ([], [], [])
        assert g.update_duals(theta, *sets) == K.OK, what
        st, d1, k1 = g.get_duals()
        d2, k2 = duals_step(d, kind, row, theta, *sets)
        assert st == K.OK and np.array_equal(d1.view(np.uint64), d2.view(np.uint64)) and np.array_equal(k1, k2), (what, "dual step")
        MB.close_all([t, c])
    assert labels == set("abcdefgh" if name == "M2" else "abdefgh"), labels
    MX.same_handles(g, s, a, (name, nupdates, "afterwards"))
    MB.close_all([g, s])


def members_at_different_points(name, n):
    """n holders of one matrix, clones of one root after 0, 1, 2 and 3 updates (util_matrix.update_pair): (m, ncol, a,
    members, root)"""
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
        for k, h in zip(ks, MB.fork(g, len(ks))):
            members[k], isb[k] = h, list(isbasic)
    s.close()
    return m, ncol, a, members, isb, g


def batch_call(members, rows, cs, order=None, chunk_bytes=-1, prep=False, want=False):
    """set_duals of member k's case, then one ratio_test_batch in the given order: (statuses, records, kept rows, counts)
    in member order"""
    n = len(members)
    order = list(range(n)) if order is None else order
    for h, c in zip(members, cs):
        assert h.set_duals(c[1], c[2]) == K.OK
    assert members[0].dbg_set_matrix_batch_bytes(chunk_bytes) == K.OK
    sts, recs = blu_amd.ratio_test_batch([members[k] for k in order], [rows[k] for k in order], [cs[k][3] for k in order], cs[0][4], cs[0][5],
                                         prepare_update=prep, want_solution=want)
    counts = members[order[0]].dbg_matrix_counts()
    assert members[0].dbg_set_matrix_batch_bytes(-1) == K.OK
    s2, r2 = [None] * n, [None] * n
    for pos, k in enumerate(order):
        s2[k], r2[k] = sts[pos], recs[pos]
    return s2, r2, [h.ratio_row()[1] for h in members], counts


def check_batch(name, n):
    m, ncol, a, members, isb, g = members_at_different_points(name, n)
    rows, alphas, lists = [], [], []
    for k, h in enumerate(members):
        r, alpha = find_row(h, a, m, ncol, start=3 * k + 1)
        twins_hold(name, alpha)
        rows.append(r)
        alphas.append(alpha)
        lists.append(cases(name, alpha, seed=k))
    ncase = len(lists[0])
    # pivtol and dualtol belong to the call: member k takes case (ci + k) % ncase with the tolerances of case ci, and the
    # restatement says what that gives (the properties are asserted where a member runs a case with its own tolerances)
    seen = set()
    for ci in range(ncase):
        tol = lists[0][ci][4:]
        cs = [lists[k][(ci + k) % ncase][:4] + tol for k in range(n)]
        seen |= {c[0][0] for c in cs if c[0] == lists[0][ci][0]}
        singles = []
        if ci == 0:  # d and kind through copy_duals_batch, then set_duals on some; beside the single entry on forks
            assert g.set_duals(cs[0][1], cs[0][2]) == K.OK
            assert blu_amd.copy_duals_batch(g, members) == [K.OK] * n
            for h in members:
                st, d1, k1 = h.get_duals()
                assert st == K.OK and MX.same_bits(d1, cs[0][1]) and np.array_equal(k1, cs[0][2])
                assert h.ratio_row()[0] == INVCALL  # (the kept row is not copied)
            singles = [MB.fork(h)[0] for h in members]
            assert blu_amd.copy_duals_batch(g, singles) == [K.OK] * n
            for h, c in zip(singles, cs):
                assert h.set_duals(c[1], c[2]) == K.OK
        sts, recs, rws, counts = batch_call(members, rows, cs, want=(ci == 0))
        assert sts == [K.OK] * n and counts == (3, 1, 3, 64 * n), (ci, sts, counts)
        for k in range(n):
            what = (name, n, ci, "member", k, cs[k][0])
            assert same_record(recs[k], pick_of(alphas[k], cs[k])), (what, recs[k], pick_of(alphas[k], cs[k]))
            assert MX.same_bits(rws[k], kept(alphas[k], cs[k][2])), (what, "kept row")
        for k, s in enumerate(singles):
            st, rec = s.ratio_test(rows[k], cs[k][3], *tol, want_solution=True)
            assert st == K.OK and same_record(rec, recs[k]), (k, "the single entry")
            assert MX.same_bits(s.ratio_row()[1], rws[k]) and MX.same_solution(MX.solution(s), MX.solution(members[k])), (k, "single")
            for key in MX.FLOPS:
                assert s.stat(key) == members[k].stat(key), (k, "statistic", key)
        if ci == 1:  # the same call permuted, and in chunks of one group
            perm = list(np.random.default_rng(n).permutation(n))
            _, recs2, rws2, _ = batch_call(members, rows, cs, order=perm)
            _, recs3, rws3, counts = batch_call(members, rows, cs, chunk_bytes=1)
            chunks = (n + 7) // 8
            assert counts == (3 * chunks, chunks, 3 * chunks, 64 * n), counts
            for k in range(n):
                assert same_record(recs[k], recs2[k]) and same_record(recs[k], recs3[k]), ("permuted / chunked", k)
                assert MX.same_bits(rws[k], rws2[k]) and MX.same_bits(rws[k], rws3[k]), ("permuted / chunked rows", k)
        MB.close_all(singles)
    assert seen == set("abcdefgh" if name == "M2" else "abdefgh"), seen

    # ---- an iteration: forward solves, ratio_test_batch with prepare_update, update_batch, update_duals_batch, beside forks
    # driven by the single entries
    S = [MB.fork(h)[0] for h in members]
    prows, xtbl = MB.forward_solves(members, a, isb)
    assert MB.forward_solves(S, a, isb) == (prows, xtbl)
    cs = []
    for k, h in enumerate(members):
        c = h.clone()
        assert c.solve_for_update([prows[k]], None, "T", True) == K.OK
        al = MX.at_dot(a[0], a[1], a[2], c.lhs)
        c.close()
        nonbasic = np.asarray(isb[k]) == 0
        kind = np.where(nonbasic, np.where(al >= 0, 1, -1), 0).astype(np.int8)
        cs.append(("iteration", 2.0 * np.abs(al) + 1.0 * (al == 0), kind, 1.0 if k % 2 else -1.0, 1e-9, 1e-7))
        alphas[k] = al
    for h, c in zip(S, cs):
        assert h.set_duals(c[1], c[2]) == K.OK
    sts, recs, rws, counts = batch_call(members, prows, cs, prep=True, want=True)
    assert sts == [K.OK] * n and counts == (3, 1, 3, 64 * n), (sts, counts)
    thetas, sets = [], []
    for k, s in enumerate(S):
        st, rec = s.ratio_test(prows[k], cs[k][3], 1e-9, 1e-7, prepare_update=True, want_solution=True)
        assert st == K.OK and same_record(rec, recs[k]) and same_record(rec, pick_of(alphas[k], cs[k])), ("iteration", k, rec, recs[k])
        assert MX.same_solution(MX.solution(s), MX.solution(members[k])), ("iteration", k)
        thetas.append(rec[4] if rec[0] >= 0 else 0.0)
        sets.append(None if rec[0] < 0 or k % 3 == 0 else ([rec[0]], [-0.0], [0]))
    assert blu_amd.update_batch(members, xtbl) == [h.update(x) for h, x in zip(S, xtbl)]
    assert blu_amd.update_duals_batch(members, thetas, sets) == [K.OK] * n
    for k, s in enumerate(S):
        one = sets[k] or ([], [], [])
        assert s.update_duals(thetas[k], *one) == K.OK
        st, d1, k1 = members[k].get_duals()
        _, d2, k2 = s.get_duals()
        d3, k3 = duals_step(cs[k][1], cs[k][2], rws[k], thetas[k], *one)
        assert st == K.OK and MX.same_bits(d1, d2) and MX.same_bits(d1, d3) and np.array_equal(k1, k2) and np.array_equal(k1, k3), ("dual step", k)
        MX.same_handles(members[k], s, a, ("iteration afterwards", k))
    MB.close_all(members + S + [g])


def check_bad_members(name):
    """members without a matrix, without duals, with an out-of-range row, without a factorization, with a bad sigma: each
    its own status, the others their records"""
    m, ncol, a, g, basis, isbasic = new_root(name)
    r, alpha = find_row(g, a, m, ncol)
    case = cases(name, alpha)[0]
    assert g.set_duals(case[1], case[2]) == K.OK
    for prep in (False, True):
        good = MB.fork(g, 6)
        nomat = g.clone()
        noduals = MB.fork(g)[0]
        nofact = blu_amd.BLU(m, 8)
        assert blu_amd.share_matrix(g, [nofact]) == [K.OK]
        hs = [good[0], nomat, good[1], noduals, good[2], good[3], nofact, good[4], good[5]]
        assert blu_amd.copy_duals_batch(g, hs) == [K.OK, INVCALL] + [K.OK] * 7
        (noduals2,) = MB.fork(g)
        hs[3].close()
        hs[3] = noduals2
        rows = [r] * len(hs)
        rows[4] = m
        sig = [1.0] * len(hs)
        sig[7] = 0.5
        if prep:
            for h in (good[0], good[1], good[3], good[5]):
                assert h.solve_for_update_column(ncol - 1) == K.OK
        ref = good[2].clone()  # (good[2] has no pending forward solve, and its row is refused)
        assert (ref.solve_for_update([r], None, "T", True) if prep else ref.solve_sparse([r], [1.0], "T")) == K.OK
        alpha = MX.at_dot(a[0], a[1], a[2], ref.lhs)
        ref.close()
        sts, recs = blu_amd.ratio_test_batch(hs, rows, sig, 0.0, 0.0, prepare_update=prep)
        assert sts == [K.OK, INVCALL, K.OK, INVCALL, INVARG, K.OK, INVCALL, INVARG, K.OK], (prep, sts)
        for k in (0, 2, 5, 8):
            assert same_record(recs[k], pick_of(alpha, case)), (prep, k, recs[k], pick_of(alpha, case))
        assert blu_amd.update_duals_batch(hs, [0.5] * len(hs)) == [K.OK, INVCALL, K.OK, INVCALL, INVCALL, K.OK, INVCALL, INVCALL, K.OK]
        want = duals_step(case[1], case[2], kept(alpha, case[2]), 0.5)[0]
        assert MX.same_bits(hs[0].get_duals()[1], want) and MX.same_bits(hs[4].get_duals()[1], case[1])
        # a member's own bad overrides
        bad = [None, None, ([0, 0], [1.0, 2.0], [0, 0]), None, None, ([ncol], [1.0], [0]), None, None, ([1], [1.0], [3])]
        assert blu_amd.update_duals_batch(hs, [0.0] * len(hs), bad) == [K.OK, INVCALL, INVARG, INVCALL, INVCALL, INVARG, INVCALL, INVCALL, INVARG]
        assert MX.same_bits(hs[2].get_duals()[1], want), "a refused member is not touched"
        MB.close_all(hs)
    g.close()


def check_refusals_and_lifetime(name):
    m, ncol, a, g, basis, isbasic = new_root(name)
    r, alpha = find_row(g, a, m, ncol)
    case = cases(name, alpha)[0]
    _, d, kind, sigma, pivtol, dualtol = case
    L = blu_amd.lib()
    RT, UD, SD, GR = L.blu_hip_ratio_test, L.blu_hip_update_duals, L.blu_hip_set_duals, L.blu_hip_get_ratio_row
    RT.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_double] + [C.c_void_p] * 4
    UD.argtypes = [C.c_void_p, C.c_double, C.c_int64] + [C.c_void_p] * 3
    SD.argtypes = [C.c_void_p] * 3
    GR.argtypes = [C.c_void_p] * 2
    rec = blu_amd.blu.RatioResult()
    out = C.addressof(rec)
    row = np.zeros(ncol)

    def entries(h):
        """the statuses of the entries that need duals"""
        return [h.get_duals()[0], h.ratio_row()[0], RT(h._h, r, 0, 1.0, 0.0, 0.0, out, None, None, None), UD(h._h, 0.0, 0, None, None, None)]

    # ---- before the first set_duals, and its own refusals
    assert entries(g) == [INVCALL] * 4
    nomat = g.clone()
    assert SD(nomat._h, d.ctypes.data, kind.ctypes.data) == INVCALL and SD(None, d.ctypes.data, kind.ctypes.data) == MISS
    assert SD(g._h, d.ctypes.data, None) == MISS and SD(g._h, None, kind.ctypes.data) == MISS  # (the first call needs both)
    badk = kind.copy()
    badk[ncol // 2] = 3
    assert SD(g._h, d.ctypes.data, badk.ctypes.data) == INVARG and entries(g) == [INVCALL] * 4
    assert g.set_duals(d, kind) == K.OK
    assert entries(g)[:2] == [K.OK, INVCALL]  # (no kept row yet; the ratio test of entries() then made one)
    assert SD(g._h, None, badk.ctypes.data) == INVARG and np.array_equal(g.get_duals()[2], kind)

    # ---- ratio_test: refusals in front of the solve leave everything alone
    want = pick_of(alpha, case)
    st, got = g.ratio_test(r, sigma, pivtol, dualtol)
    assert st == K.OK and same_record(got, want)
    keep = g.ratio_row()[1]
    stats = [g.stat(key) for key in MV.STATS]
    nan, inf = float("nan"), float("inf")
    assert RT(None, r, 0, 1.0, 0.0, 0.0, out, None, None, None) == MISS
    assert RT(nomat._h, r, 0, 1.0, 0.0, 0.0, out, None, None, None) == INVCALL
    assert RT(g._h, r, 0, 1.0, 0.0, 0.0, None, None, None, None) == MISS
    for sg, pt, dt in ((0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (nan, 0.0, 0.0), (1.0, -1.0, 0.0), (1.0, 0.0, -1e-9), (1.0, nan, 0.0), (1.0, 0.0, inf),
                       (-1.0, inf, 0.0)):
        assert RT(g._h, r, 0, sg, pt, dt, out, None, None, None) == INVARG, (sg, pt, dt)
    assert RT(g._h, m, 0, 1.0, 0.0, 0.0, out, None, None, None) == INVARG and RT(g._h, -1, 1, 1.0, 0.0, 0.0, out, None, None, None) == INVARG
    assert [g.stat(key) for key in MV.STATS] == stats and MX.same_bits(g.ratio_row()[1], keep)
    # ---- update_duals
    j2 = np.array([1, 1], np.int64)
    jo = np.array([ncol], np.int64)
    jn = np.array([-1], np.int64)
    x2 = np.zeros(2)
    k2 = np.zeros(2, np.int8)
    k3 = np.array([0, 5], np.int8)
    j01 = np.array([0, 1], np.int64)
    assert UD(None, 0.0, 0, None, None, None) == MISS and UD(g._h, 0.0, 1, None, x2.ctypes.data, k2.ctypes.data) == MISS
    assert UD(g._h, 0.0, -1, None, None, None) == INVARG
    assert UD(g._h, 0.0, 2, j2.ctypes.data, x2.ctypes.data, k2.ctypes.data) == INVARG
    assert UD(g._h, 0.0, 1, jo.ctypes.data, x2.ctypes.data, k2.ctypes.data) == INVARG
    assert UD(g._h, 0.0, 1, jn.ctypes.data, x2.ctypes.data, k2.ctypes.data) == INVARG
    assert UD(g._h, 0.0, 2, j01.ctypes.data, x2.ctypes.data, k3.ctypes.data) == INVARG
    st, d1, k1 = g.get_duals()
    assert MX.same_bits(d1, d) and np.array_equal(k1, kind), "refused steps touch nothing"
    assert g.update_duals(0.0) == K.OK and g.update_duals(0.0) == K.OK  # (the kept row stays valid)
    d0 = duals_step(d, kind, keep, 0.0)[0]
    assert MX.same_bits(g.get_duals()[1], d0)

    # ---- the batch entries refused as a whole
    RB, UB, CB = L.blu_hip_ratio_test_batch, L.blu_hip_update_duals_batch, L.blu_hip_copy_duals_batch
    RB.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double] + [C.c_void_p] * 5
    UB.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6
    CB.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    k1h, k2h = MB.fork(g, 2)
    assert blu_amd.copy_duals_batch(g, [k1h, k2h]) == [K.OK] * 2
    own = blu_amd.BLU(m, len(a[1]))
    assert own.set_matrix(ncol, *a) == K.OK and own.factorize_columns(basis) == K.OK and own.set_duals(d, kind) == K.OK
    other_m = blu_amd.BLU(m + 1, 8)
    watched = (g, k1h, k2h, own)
    stats = [[h.stat(key) for key in MV.STATS] for h in watched]

    def whole(fn, hs, code, n=None, **kw):
        N = len(hs)
        arr = (C.c_void_p * N)(*[None if h is None else h._h for h in hs])
        st = (C.c_int * N)(*([77] * N))
        cnt = N if n is None else n
        rr = (C.c_int64 * N)(*([r] * N))
        sg = (C.c_double * N)(*([1.0] * N))
        recs = (blu_amd.blu.RatioResult * N)()
        th = (C.c_double * N)()
        if fn == "ratio":
            rc = RB(arr, cnt, rr if kw.get("r", True) else None, 0, sg if kw.get("sigma", True) else None, kw.get("pivtol", 0.0),
                    kw.get("dualtol", 0.0), recs if kw.get("out", True) else None, None, None, None, st)
        elif fn == "step":
            rc = UB(arr, cnt, th if kw.get("theta", True) else None, None, None, None, None, st)
        else:
            rc = CB(kw["src"]._h if kw.get("src") else None, arr, cnt, st)
        assert rc == code, (fn, rc, code, kw)
        if n is None:
            assert list(st) == [code] * N, (fn, code, list(st))
        assert [[h.stat(key) for key in MV.STATS] for h in watched] == stats, (fn, code)
        for h in watched:
            assert MX.same_bits(h.get_duals()[1], d0 if h is g else d), (fn, code)

    for fn in ("ratio", "step"):
        whole(fn, [k1h, None], MISS)
        whole(fn, [k1h, k2h], MISS, n=-1)
        whole(fn, [k1h, k2h, k1h], INVARG)
        whole(fn, [k1h, own], INVARG)  # two matrices
        whole(fn, [k1h, k2h], K.OK, n=0)
    whole("ratio", [k1h, k2h], MISS, r=False)
    whole("ratio", [k1h, k2h], MISS, sigma=False)
    whole("ratio", [k1h, k2h], MISS, out=False)
    whole("ratio", [k1h, k2h], INVARG, pivtol=-1.0)
    whole("ratio", [k1h, k2h], INVARG, dualtol=nan)
    whole("step", [k1h, k2h], MISS, theta=False)
    assert RB(None, 1, None, 0, None, 0.0, 0.0, None, None, None, None, None) == MISS and UB(None, 1, None, None, None, None, None, None) == MISS
    whole("copy", [k1h], MISS)  # NULL src
    whole("copy", [k1h, None], MISS, src=g)
    whole("copy", [k1h], MISS, n=-1, src=g)
    whole("copy", [k1h], INVCALL, src=nomat)
    whole("copy", [k1h, g], INVARG, src=g)
    whole("copy", [k1h, k2h, k1h], INVARG, src=g)
    whole("copy", [k1h, other_m], INVARG, src=g)
    whole("copy", [k1h], K.OK, n=0, src=g)
    assert blu_amd.copy_duals_batch(g, [k1h, own, nomat]) == [K.OK, INVCALL, INVCALL]  # (another matrix, none)
    assert MX.same_bits(k1h.get_duals()[1], d0) and MX.same_bits(own.get_duals()[1], d)
    for bad in (lambda: blu_amd.ratio_test_batch([k1h, own], [r, r], [1.0, 1.0], 0.0, 0.0), lambda: blu_amd.copy_duals_batch(nomat, [k1h]),
                lambda: blu_amd.ratio_test_batch([k1h], [r], [1.0], -1.0, 0.0), lambda: blu_amd.update_duals_batch([k1h, k1h], [0.0, 0.0])):
        try:
            bad()
        except blu_amd.BluError:
            continue
        raise AssertionError("a refused batch call raises")

    # ---- the lifetime of the state
    assert k1h.ratio_test(r, sigma, pivtol, dualtol)[0] == K.OK and k2h.ratio_test(r, sigma, pivtol, dualtol)[0] == K.OK
    plain = blu_amd.BLU(m, 8)
    assert blu_amd.copy_batch(k1h, [k2h, plain]) == [K.OK] * 2  # copy_batch in either role: the duals and kept rows stay, none is copied
    assert entries(plain) == [INVCALL] * 4
    for h in (k1h, k2h):
        st, dd, kk = h.get_duals()
        assert st == K.OK and MX.same_bits(dd, d0 if h is k1h else d) and MX.same_bits(h.ratio_row()[1], keep)
    assert k1h.factorize_columns(basis) == K.OK and MX.same_bits(k1h.ratio_row()[1], keep) and k1h.update_duals(0.0) == K.OK  # factorize_columns: stays
    assert blu_amd.share_matrix(own, [k2h]) == [K.OK] and entries(k2h)[:2] == [INVCALL] * 2 and entries(own)[0] == K.OK  # a destination: dropped
    assert k2h.set_duals(d, kind) == K.OK and k2h.ratio_row()[0] == INVCALL and same_record(k2h.ratio_test(r, sigma, pivtol, dualtol)[1], want)
    assert own.set_matrix(ncol, *a) == K.OK and entries(own)[:2] == [INVCALL] * 2  # set_matrix: dropped
    b2, i2 = MV.start(m, ncol)
    assert k1h.maxvolume(ncol, a[0], a[1], a[2], b2, i2, 1e300)[0] == K.OK and entries(k1h) == [INVCALL] * 4  # maxvolume: dropped
    assert g.get_duals()[0] == K.OK and MX.same_bits(g.ratio_row()[1], keep)  # the other holders are untouched
    MB.close_all([g, k1h, k2h, own, other_m, plain, nomat])

    # ---- ncol == 0: the solve alone, q = -1
    e = blu_amd.BLU(m, len(a[1]))
    assert e.set_matrix(0, np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0)) == K.OK
    assert e.factorize(*MX.gathered(a, basis)) == K.OK and e.set_duals(np.zeros(0), np.zeros(0, np.int8)) == K.OK
    st, got = e.ratio_test(1, 1.0, 0.0, 0.0, want_solution=True)
    assert st == K.OK and got == NONE and e.nzlhs > 0 and e.dbg_matrix_counts() == (0, 0, 0, 0)
    assert e.update_duals(1.0) == K.OK and e.ratio_row()[0] == K.OK and e.get_duals()[0] == K.OK
    sts, recs = blu_amd.ratio_test_batch([e], [1], [-1.0], 0.0, 0.0)
    assert sts == [K.OK] and recs == [NONE] and blu_amd.update_duals_batch([e], [1.0]) == [K.OK]
    e.close()
