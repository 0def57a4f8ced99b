"""The layer report without a device: the numpy / oracle restatement of its arithmetic contract
(tests/report_ref.py, DESIGN.md §3 "Layer report") pinned to the reference's recorded numbers, the
chain of the stacking trick checked against exact rational arithmetic, and the C entries'
argument checks (quantizer.py:296-306 in Gram form)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import report_ref as rr
from conftest import load_golden
from oracle import oracle as orc

E_ARG, E_WORKSPACE = 1, 5
F32, F16, BF16, I8 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def atq():
    """examples.py:15-45 example 1 on the oracle's fitted grids: (W, X, G, Ŵ_itf, Ŵ_aga)."""
    g = load_golden("examples_atq")
    W, X = g["W"], g["X"].reshape(-1, g["X"].shape[-1])
    a0, m0, T0 = orc.ternary_init(W)
    a1, m1, T1, _ = orc.iterative_ternary_fitting(W, a0, m0, T0)
    a2, m2 = orc.activation_aware_grid_alignment(W, T1, X)
    return g, W, X, orc.gram(X), (a1, m1, T1), (a2, m2, T1)


def test_restatement_matches_reference_numbers(atq):
    """The restated totals lie within the derived bound of the float64 value of the same f32 D and
    G, and so do the reference's recorded floats (err_itf, out_err_itf, out_err_aga): the same bound
    again.  Observed: out_err_itf restated 806559.8125 / exact 806559.7551 / recorded 806559.75,
    out_err_aga 806687.1875 / 806687.2399 / 806687.1875 (bound 2.5e3, 3.1e-3 relative); err_itf
    24838.12695 / 24838.12574 / 24838.125 (bound 0.12)."""
    g, W, X, G, itf, aga = atq
    m = W.shape[1]
    for (a, mu, T), key in ((itf, "out_err_itf"), (aga, "out_err_aga")):
        rep = rr.report(W, a, mu, T, m, None, G, reference=False)
        D = rep["D"]
        assert np.array_equal(D, W - (a * T + mu))  # the reference's own W - W_c
        ex, exact, bound = float(rep["totals"][1]), rr.exact_total(D, G), rr.error_bound(D, G)
        rec = float(g[key])
        print(f"{key}: restated {ex!r} exact {exact!r} recorded {rec!r} bound {bound:.3e} "
              f"(rel {bound / exact:.2e}); |restated-exact| {abs(ex - exact):.3e} "
              f"|restated-recorded| {abs(ex - rec):.3e}")
        assert abs(ex - exact) <= bound
        assert abs(rec - exact) <= bound
        assert ex == pytest.approx(rec, rel=1e-5)  # test_metrics_cpu.py's tolerance holds too
    a, mu, T = itf
    rep = rr.report(W, a, mu, T, m)
    D = rep["D"].astype(np.float64)
    ew, exact = float(rep["totals"][0]), float((D * D).sum())
    n = W.shape[0]
    bound = (-(-m // 32) + -(-n // 32) + 16) * 2.0 ** -23 * exact
    rec = float(g["err_itf"])
    print(f"err_itf: restated {ew!r} exact {exact!r} recorded {rec!r} bound {bound:.3e}")
    assert abs(ew - exact) <= bound and abs(rec - exact) <= bound
    assert ew == pytest.approx(rec, rel=1e-5)


def rn_f32(x: Fraction) -> Fraction:
    """Round-to-nearest-even of an exact rational to float32 (no overflow in these tests)."""
    if x == 0:
        return x
    e = math.floor(math.log2(abs(x)))
    while Fraction(2) ** e > abs(x):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(x):
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = x / ulp
    f = math.floor(q)
    r = q - f
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2):
        f += 1
    return f * ulp


def test_chain_is_exact_fmaf_chain(atq):
    """P = A G from oracle.gram on [Aᵀ | G] is the k-ascending fmaf chain from +0: a few entries
    against exact rational arithmetic with one rounding per step."""
    _, W, X, G, itf, _ = atq
    a, mu, T = itf
    D = rr.residual(W, a, mu, T, W.shape[1])
    P = rr.chain_product(D, G)
    n, m = D.shape
    for i, j in ((0, 0), (n - 1, m - 1), (n // 2, 3), (1, m // 2)):
        acc = Fraction(0)
        for k in range(m):
            acc = rn_f32(acc + Fraction(float(D[i, k])) * Fraction(float(G[k, j])))
        assert float(acc) == float(P[i, j]), (i, j)


def test_rowtree_shape_is_fixed():
    """ROWTREE is the 32-chunk halving tree with ascending chunk sums -- spelled out once more
    elementwise, on lengths around the chunk edges."""
    rng = np.random.default_rng(5)
    for L in (1, 31, 32, 33, 70):
        v = (rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L)).astype(np.float32)
        p = np.zeros(-(-L // 32) * 32, np.float32)
        p[:L] = v
        s = np.float32(0)
        for c in range(len(p) // 32):
            w = list(p[32 * c:32 * c + 32])
            h = 16
            while h:
                w = [np.float32(w[j] + w[j + h]) for j in range(h)]
                h //= 2
            s = np.float32(s + w[0])
        assert rr.rowtree(v) == s


def test_block_table_follows_positions():
    perm = np.array([4, 0, 3, 1, 2], np.int64)
    assert list(rr.block_of_column(5, 2, perm)) == [0, 1, 2, 1, 0]
    assert list(rr.block_of_column(5, 8, perm)) == [0] * 5  # b >= m: one block


def test_report_entries_without_device(pt2q):
    lib = pt2q._lib.lib()
    for s in ("pt2q_quadform_rows", "pt2q_quadform_rows_workspace_bytes", "pt2q_layer_report",
              "pt2q_layer_report_workspace_bytes"):
        assert hasattr(lib, s)
    sizes = [(1, 1), (33, 31), (130, 257), (4096, 4096), (4096, 11008), (11008, 11008)]
    prev = (0, 0, 0)
    for n, m in sizes:
        cur = (lib.pt2q_quadform_rows_workspace_bytes(n, m), lib.pt2q_layer_report_workspace_bytes(n, m, 0),
               lib.pt2q_layer_report_workspace_bytes(n, m, 1))
        assert all(c > 0 for c in cur) and all(c >= p for c, p in zip(cur, prev))
        assert cur[2] >= cur[1]
        prev = cur
    assert lib.pt2q_layer_report_workspace_bytes(0, 8, 0) == 0
    assert lib.pt2q_quadform_rows_workspace_bytes(8, 0) == 0
    p = ctypes.c_void_p(4096)
    big = 1 << 40

    def rep(W=p, wdt=F32, ldw=64, n=16, m=64, b=32, alpha=p, mu=p, T=p, tdt=I8, ldt=64, G=p, ldg=64, flags=1,
            ws=p, wsb=big):
        return lib.pt2q_layer_report(W, wdt, ldw, n, m, b, alpha, mu, T, tdt, ldt, None, G, ldg, flags, p, p, p, p,
                                     ws, wsb, None)
    for bad in (dict(n=0), dict(m=0), dict(b=0), dict(n=-1), dict(W=None), dict(T=None), dict(alpha=None),
                dict(mu=None), dict(ldw=63), dict(ldt=63), dict(ldg=63), dict(wdt=I8), dict(wdt=7), dict(tdt=F16),
                dict(flags=2)):
        assert rep(**bad) == E_ARG, bad
    need = lib.pt2q_layer_report_workspace_bytes(16, 64, 1)
    assert rep(wsb=need - 1) == E_WORKSPACE
    assert rep(ws=None) == E_WORKSPACE

    def qf(A=p, adt=F32, lda=64, rows=16, m=64, G=p, ldg=64, ws=p, wsb=big):
        return lib.pt2q_quadform_rows(A, adt, lda, rows, m, G, ldg, p, p, ws, wsb, None)
    for bad in (dict(rows=0), dict(m=0), dict(A=None), dict(G=None), dict(lda=63), dict(ldg=63), dict(adt=I8)):
        assert qf(**bad) == E_ARG, bad
    assert qf(wsb=lib.pt2q_quadform_rows_workspace_bytes(16, 64) - 1) == E_WORKSPACE
