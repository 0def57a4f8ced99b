"""tests/breakdown_cases.py on the CPU: the oracle alone establishes every expectation of
test_gpu_breakdown.py (planted pivots give k + 1, emergent ones lie in (N, m], healthy items and tiny
pivots give 0 and a NaN-free inverse), and the pivots reach the launches they are there for (by
factoring_step, a walk over ragged_cases.chol_schedule)."""
import numpy as np
import pytest

import breakdown_cases as bc
import ragged_cases as rc
from oracle import oracle as orc


# ------------------------------------------------------------------ the oracle on every case

@pytest.mark.parametrize("m,k", bc.PLANTED_CASES)
def test_planted_pivot(m, k):
    H = bc.planted(m, k)
    assert H[k, k] == 0.0 and np.array_equal(H, H.T)
    assert bc.oracle_info(H) == k + 1


@pytest.mark.parametrize("m", bc.REUSE_M)
def test_planted_base_is_healthy(m):
    assert bc.oracle_info(bc.healthy(m)) == 0
    Hinv = bc.healthy_inverse(m)
    assert np.isfinite(Hinv).all() and np.array_equal(Hinv, Hinv.T)


@pytest.mark.slow
@pytest.mark.parametrize("k", bc.LOOKAHEAD_K)
def test_lookahead_planted_pivot(k):
    H = bc.lookahead_planted(k)
    assert H.shape == (bc.LOOKAHEAD_M, bc.LOOKAHEAD_M) and H[k, k] == -1.0
    assert bc.oracle_info(H) == k + 1


@pytest.mark.parametrize("N,m", bc.EMERGENT)
def test_emergent_pivot_is_a_cancellation(N, m):
    """No diagonal entry is non-positive on input and the first N pivots hold: the breakdown comes
    out of the chains."""
    H, info = bc.emergent(N, m)
    assert N < m and (np.diag(H) > 0).all()
    assert N < info <= m, info


def test_emergent_pivots_depend_on_rounding():
    """In exact arithmetic every one of them would fail at pivot N + 1; in fp32 some hold one longer."""
    late = [bc.emergent(N, m)[1] - (N + 1) for N, m in bc.EMERGENT]
    assert min(late) == 0 and max(late) > 0, late


@pytest.mark.parametrize("name", sorted(bc.SPECIAL))
def test_special_cases(name):
    H = bc.special_case(name)
    assert np.array_equal(H, H.T, equal_nan=True)
    assert bc.oracle_info(H) == bc.SPECIAL[name]


def test_special_case_inputs():
    H = bc.special_case("first_wins")
    assert H[70, 70] == H[130, 130] == -1.0 and bc.factoring_step(576, 70) != bc.factoring_step(576, 130)
    assert np.signbit(bc.special_case("minus_zero")[70, 70]) and not np.signbit(bc.special_case("plus_zero")[70, 70])
    # pivot 100 of the cancellation case is an exact zero reached in the chain, not on input
    H = bc.special_case("cancel_to_zero")
    assert (np.diag(H) == 1.0).all()
    for name in ("nan_diag", "nan_offdiag", "inf_offdiag", "neg_inf_diag", "pos_inf_diag"):
        assert not np.isfinite(bc.special_case(name)).all()


@pytest.mark.parametrize("name", sorted(bc.TINY))
def test_tiny_pivots_are_no_breakdowns(name):
    v = bc.TINY[name]
    H, U, Hinv = bc.tiny_case(name)
    assert v > 0 and H[70, 70] == v and bc.oracle_info(H) == 0
    # the correctly rounded square root of the (sub)normal pivot
    assert U[70, 70] == np.float32(np.sqrt(np.float64(v))) and U[70, 70] > 0
    assert not np.isnan(Hinv).any()
    subnormal = v < np.finfo(np.float32).tiny
    assert np.isposinf(Hinv[70, 70]) == subnormal
    rest = np.delete(np.delete(Hinv, 70, 0), 70, 1)
    assert np.array_equal(rest, np.eye(127, dtype=np.float32))
    assert {n for n, x in bc.TINY.items() if x < np.finfo(np.float32).tiny} == {"1e-40", "denorm_min"}


@pytest.mark.parametrize("m", bc.BATCH_M)
def test_batch_items(m):
    Gs, Hs, infos, Hinvs = bc.batch_case(m)
    assert infos == [want for _, _, want in bc.BATCH_ITEMS]
    for z, (N, neg, want) in enumerate(bc.BATCH_ITEMS):
        if want == 0:
            assert N > m and not np.isnan(Hinvs[z]).any()
        elif neg is not None:
            assert want == neg + 1 and Gs[z][neg, neg] < 0 and N > m
        else:
            assert N < want <= m  # rank-deficient: a cancellation breakdown
    # the failing items sit at other places than "item 1", on both chunk positions
    failing = [z for z, i in enumerate(infos) if i]
    assert failing == [1, 2, 3, 5]
    for chunk in bc.BATCH_CHUNKS:
        assert {z % chunk for z in failing} >= {1, 2, 3}
    assert 4 in bc.BATCH_CHUNKS and 3 % 4 == 3 and 5 % 4 == 1  # last of a call; item 1 of the next


def test_layer_cases():
    n, m, N, bs = bc.LAYER
    W, X, info, ref = bc.layer_case()
    assert (N, m) in bc.EMERGENT and N < info <= m and bs < m
    H, _ = orc.prepare_hessian(orc.gram(X), N, 0.0)
    assert bc.oracle_info(H) == info
    assert ref["spd"] and ref["alpha"].shape == (n, rc.ceil_div(m, bs))
    assert set(np.unique(ref["T"])) == {-1, 0, 1} and np.isfinite(ref["alpha"]).all()
    n, m, N, b = bc.PER_CHANNEL
    W, X, info, ref = bc.per_channel_case()
    assert b >= m and not rc.needs_inverse(m, b) and N < info <= m  # a Hessian that would break down
    assert ref["alpha"].shape == (n, 1) and np.array_equal(ref["perm"], np.arange(m))


# ------------------------------------------------------------------ the launches the pivots reach

def _steps(m, ks, batch=1):
    return {k: bc.factoring_step(m, k, batch) for k in ks}


def test_planted_pivots_reach_both_factoring_kernels():
    per_m = {m: _steps(m, ks) for m, (_, ks) in bc.PLANTED.items()}
    kernels = {m: {s.kernel for s in st.values()} for m, st in per_m.items()}
    assert kernels[100] == kernels[576] == {"diag", "fused"}
    assert kernels[333] == {"diag"}  # m % 4: the strip update is the generic pair, never the fused factor
    assert set().union(*kernels.values()) == {"diag", "fused"}
    # both panel-solve kernels: one lane per column for whole blocks of 16-byte rows, four otherwise
    assert {s.solve for s in per_m[576].values()} == {"lane"}
    assert {s.solve for s in per_m[333].values()} == {"lpr"}
    assert {s.solve for s in per_m[100].values()} == {"lane", "lpr"}
    # m = 100: the ragged 36-block is factored inside the strip-update launch
    assert per_m[100][64] == per_m[100][99] == bc.Step("fused", "lpr", "strip", 0, 0, 64, 36)
    assert per_m[100][0] == per_m[100][63] == bc.Step("diag", "lane", "start", 0, 0, 0, 64)
    # m = 333: a ragged last block of 13; the block at 256 sits behind a sub-panel term
    assert per_m[333][320] == per_m[333][332] == bc.Step("diag", "lpr", "strip", 0, 0, 320, 13)
    assert per_m[333][256].after == "subpanel" and per_m[333][255].after == "strip"
    # every block of every width is hit at its first or last pivot somewhere
    for m, st in per_m.items():
        assert {s.p0 for s in st.values()} >= {0, (m - 1) // 64 * 64}


def test_planted_pivots_reach_subpanel_and_panel_boundaries():
    st = _steps(576, bc.PLANTED[576][1])
    assert 576 % 4 == 0
    for k in (256, 257):  # the first block of the second sub-panel: its own launch after the rank-256 terms
        assert st[k] == bc.Step("diag", "lane", "subpanel", 0, 0, 256, 64)
    for k in (512, 513, 575):  # the block behind the 512-row panel's terms
        assert st[k] == bc.Step("diag", "lane", "panel", 0, 0, 512, 64)
    for k in (64, 65, 127, 128, 191, 255, 511):  # inside a sub-panel: the fused factor
        assert st[k].kernel == "fused" and st[k].after == "strip", k
    assert st[0].after == "start" and st[63].kernel == "diag"
    # first and last pivot of a block on both sides of every boundary
    assert {63, 64, 255, 256, 511, 512} <= set(st)


def test_lookahead_pivots_lie_behind_forks():
    m = bc.LOOKAHEAD_M
    assert m > 6144
    a, b = (bc.factoring_step(m, k) for k in bc.LOOKAHEAD_K)
    assert (a.forks, a.joins) == (1, 0) and (b.forks, b.joins) == (2, 1)
    assert a.kernel == b.kernel == "fused" and a.solve == b.solve == "lane"
    assert (a.p0, b.p0) == (576, 1088)
    # the widths below the look-ahead, and a batch at this width, never fork
    assert all(bc.factoring_step(mm, mm - 1).forks == 0 for mm in (576, 1100, 6144))
    assert bc.factoring_step(m, 1100, batch=2).forks == 0
    # side-stream work is still owed when the pivot fails: later panels exist
    assert bc.factoring_step(m, m - 1).forks > b.forks


def test_batch_items_land_on_different_steps():
    batch = len(bc.BATCH_ITEMS)
    for b in (batch, 4, 2):
        s2, s3 = bc.factoring_step(320, 70, b), bc.factoring_step(320, 256, b)
        assert (s2.kernel, s3.kernel) == ("fused", "diag") and s3.after == "subpanel"
        assert {bc.factoring_step(333, k, b).kernel for k in (70, 256)} == {"diag"}
    # the emergent items: pivot 200 (0-based) in the fused launch at 320, 151 likewise
    assert bc.factoring_step(320, 200, batch).kernel == bc.factoring_step(320, 151, 2).kernel == "fused"


def test_emergent_pivots_and_steps():
    seen = set()
    for N, m in bc.EMERGENT:
        s = bc.factoring_step(m, bc.emergent(N, m)[1] - 1)
        seen.add((s.kernel, s.solve))
    assert ("fused", "lane") in seen and ("diag", "lpr") in seen  # 577 % 4 != 0
