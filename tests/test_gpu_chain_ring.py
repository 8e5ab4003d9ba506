"""The ring of chain waves (k_chain.h): a triangular sweep of the statistics tail and of solve_dense is walked by several
waves, which hand each step's result over through the LDS window and a tag.  Run with -m gpu on an MI355X.

Every case checks, bit for bit: every statistic bench.py dumps and solve_dense 'N' / 'T' against the CPU oracle and against
the library's own one-workgroup kernels (BLU_HIP_NO_CHAIN=1); statistic 108 > 0 (the chain path ran) and statistic 126 == 0
(no bounded wait of the chain pipeline gave up).  The inputs are the smallest at which a ring can go wrong: fewer steps than
ring waves and the edges of the blocks of 32 steps and of the step ring of 256; every distance 1..11 from a step to its
nearest producer in all four line sets (so the boundary between the early and the late part of a step is crossed for any ring
of up to 8 waves), asserted from the oracle's factors before anything runs on the GPU; lines of more than 16 and of more than
64 entries and more steps than the window of 2048 results; a pure chain; no dependency at all; a second factorize on the same
handle."""
import numpy as np
import pytest
import scipy.sparse as sp

from blu_amd import keys as K
from tests import util

pytestmark = pytest.mark.gpu

CH_FAR = 320  # k_chain.h: a producer this many steps back is added by the helpers
STAT_KEYS = [K.STAT_RANK, K.STAT_MATRIX_NZ, K.STAT_BUMP_SIZE, K.STAT_BUMP_NZ, K.STAT_L_NZ, K.STAT_U_NZ, K.STAT_NSEARCH_PIVOT,
             K.STAT_FACTOR_FLOPS, K.STAT_RANKDEF, 50, 51, 52, 53, 54, 55, 56, K.STAT_MIN_PIVOT, K.STAT_MAX_PIVOT,
             K.STAT_CONDEST_L, K.STAT_CONDEST_U, K.STAT_NORM_L, K.STAT_NORM_U, K.STAT_NORMEST_L_INV,
             K.STAT_NORMEST_U_INV, K.STAT_ONENORM, K.STAT_INFNORM, K.STAT_RESIDUAL_TEST]  # the list bench.py dumps
SMALL_M = (1, 2, 3, 5, 7, 31, 32, 33, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def blu():
    import blu_amd
    if blu_amd.lib().blu_hip_device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return blu_amd


def _bits(x):
    return np.float64(x).view(np.int64)


def _handles(blu, monkeypatch, m, nz):
    """A handle on the chain pipeline and one on the one-workgroup kernels (the switch is read when a handle is made)."""
    a = blu.BLU(m, nz)
    monkeypatch.setenv("BLU_HIP_NO_CHAIN", "1")
    b = blu.BLU(m, nz)
    monkeypatch.delenv("BLU_HIP_NO_CHAIN")
    return a, b


def _check(a, b, o, so, cp, ri, v, where, defects_before=0):
    """Factorize on both handles and compare them with the oracle `o` (already factorized, status `so`) and with each other."""
    m = len(cp) - 1
    assert a.factorize(cp[:-1], cp[1:], ri, v) == so == K.OK, where
    assert b.factorize(cp[:-1], cp[1:], ri, v) == K.OK, where
    assert a.stat(108) > 0.0 and b.stat(108) == 0.0, where  # k_rows_grid, hence the chains, ran for the first handle only
    assert a.stat(126) == defects_before, (where, a.stat(126))  # no bounded wait gave up
    for key in STAT_KEYS:
        x, y, z = a.stat(key), o.stat(key), b.stat(key)
        assert _bits(x) == _bits(y), (where, "oracle", key, x, y)
        assert _bits(x) == _bits(z), (where, "one workgroup", key, x, z)
    rng = np.random.default_rng(11)
    rhs = rng.standard_normal(m)
    for trans in "NT":
        x = a.solve_dense(rhs, trans)
        assert np.array_equal(x, o.solve_dense(rhs, trans)), (where, trans, "oracle")
        assert np.array_equal(x, b.solve_dense(rhs, trans)), (where, trans, "one workgroup")
    assert a.stat(126) == defects_before, (where, a.stat(126))


def _line_sets(f, m):
    """The four line sets of the sweeps from get_factors (pivot coordinates).  For each: per step the distance to the nearest
    and to the farthest producer (0: the step is empty) and the number of entries."""
    out = {}
    L = sp.csc_matrix((f["l_value"], f["l_rowidx"], f["l_colptr"]), shape=(m, m)).tocoo()
    U = sp.csc_matrix((f["u_value"], f["u_rowidx"], f["u_colptr"]), shape=(m, m)).tocoo()
    for name, M, lower in (("L", L, True), ("U", U, False)):
        off = M.row != M.col
        r, c = M.row[off], M.col[off]
        d = (r - c) if lower else (c - r)
        assert np.all(d > 0)
        for by, g in (("column", c), ("row", r)):
            near = np.full(m, np.iinfo(np.int64).max)
            far = np.zeros(m, np.int64)
            np.minimum.at(near, g, d)
            np.maximum.at(far, g, d)
            n = np.bincount(g, minlength=m)
            near[n == 0] = 0
            out["%s by %s" % (name, by)] = (near, far, n)
    return out


def test_fewer_steps_than_ring_waves_and_block_edges(blu, oracle, monkeypatch):
    skipped = []
    for m in SMALL_M:
        cp, ri, v = oracle.gen_lp_basis(m, 4, 4, 0.5, 1, 0.3)
        o, so = util.oracle_factorize(oracle, cp, ri, v)
        if so != K.OK:
            skipped.append((m, so))
            continue
        a, b = _handles(blu, monkeypatch, m, len(ri))
        _check(a, b, o, so, cp, ri, v, "m=%d" % m)
    print("not OK in the oracle:", skipped)
    assert len(skipped) <= 2, skipped


def test_every_hand_over_distance(blu, oracle, monkeypatch):
    m = 2000
    cp, ri, v = oracle.gen_lp_basis(m, 8, 8, 0.5, 7, 0.3)
    o, so = util.oracle_factorize(oracle, cp, ri, v)
    assert so == K.OK
    for name, (near, far, n) in _line_sets(o.get_factors(), m).items():
        hist = np.bincount(near[near < 16], minlength=16)
        print(name, "nearest producer 0 (empty), 1..15 back:", hist.tolist(), "nearest >= %d back:" % CH_FAR, int((near >= CH_FAR).sum()),
              "longest line", int(n.max()))
        assert np.all(hist[1:12] > 0), (name, hist)
        assert hist[0] > 0 and (far >= CH_FAR).any(), name  # empty steps, and terms the helpers add
        assert n.max() <= 64, (name, n.max())
    a, b = _handles(blu, monkeypatch, m, len(ri))
    _check(a, b, o, so, cp, ri, v, "m=2000")


@pytest.mark.parametrize("spec", [(6000, 8, 8, 0.5, 3, 0.3), (1000, 8, 8, 0.0, 7, 0.3)], ids=lambda s: "m%d" % s[0])
def test_long_lines_and_a_wrapping_window(blu, oracle, monkeypatch, spec):
    m = spec[0]
    cp, ri, v = oracle.gen_lp_basis(*spec)
    o, so = util.oracle_factorize(oracle, cp, ri, v)
    assert so == K.OK
    sets = _line_sets(o.get_factors(), m)
    longest = max(int(n.max()) for _, _, n in sets.values())
    print(spec, {name: (int(n.max()), int((near >= CH_FAR).sum())) for name, (near, far, n) in sets.items()})
    assert longest > 64  # a line the ring waves take from global memory
    assert any(((n >= 17) & (n <= 64)).any() for _, _, n in sets.values())  # a staged line too long for the sum by rows of 16 lanes
    if m == 6000:
        assert m > 2048 and all((near >= CH_FAR).any() for name, (near, far, n) in sets.items() if name[0] == "U")
    a, b = _handles(blu, monkeypatch, m, len(ri))
    _check(a, b, o, so, cp, ri, v, spec)


def _bidiagonal(m):
    # B = I + superdiagonal of ones: column j holds rows j - 1 and j
    cp = np.concatenate(([0], np.arange(1, 2 * m, 2))).astype(np.uint64)
    ri = np.concatenate([[j - 1, j] if j else [0] for j in range(m)]).astype(np.uint64)
    return cp, ri, np.ones(len(ri))


def _diagonal(m):
    return np.arange(m + 1, dtype=np.uint64), np.arange(m, dtype=np.uint64), 1.0 + 0.25 * (np.arange(m) % 7)


def test_a_pure_chain(blu, oracle, monkeypatch):
    m = 2300
    cp, ri, v = _bidiagonal(m)
    o, so = util.oracle_factorize(oracle, cp, ri, v)
    near, far, n = _line_sets(o.get_factors(), m)["U by column"]
    # one term per step, from its predecessor (all steps but the first and the two ends of the oracle's pivot order)
    assert (near == 1).sum() >= m - 3 and n.max() == 1
    a, b = _handles(blu, monkeypatch, m, len(ri))
    _check(a, b, o, so, cp, ri, v, "bidiagonal")


def test_a_diagonal_basis(blu, oracle, monkeypatch):
    m = 300
    cp, ri, v = _diagonal(m)
    o, so = util.oracle_factorize(oracle, cp, ri, v)
    assert all(n.max() == 0 for _, _, n in _line_sets(o.get_factors(), m).values())  # every step is empty
    a, b = _handles(blu, monkeypatch, m, len(ri))
    _check(a, b, o, so, cp, ri, v, "diagonal")


def test_refactorize_on_the_same_handle(blu, oracle, monkeypatch):
    """Tags and progress counters are set up per sweep: a second, different basis on the same handles."""
    m = 700
    bases = [oracle.gen_lp_basis(m, 8, 8, 0.5, 5, 0.3), _bidiagonal(m), oracle.gen_lp_basis(m, 6, 6, 0.3, 9, 0.5)]
    a, b = _handles(blu, monkeypatch, m, max(len(ri) for _, ri, _ in bases))
    for i, (cp, ri, v) in enumerate(bases):
        o, so = util.oracle_factorize(oracle, cp, ri, v)
        _check(a, b, o, so, cp, ri, v, "basis %d" % i)
