"""The Cholesky breakdown word on the GPU, as an integer against the CPU oracle: info_dev = 0, or
k + 1 for the first non-positive pivot (include/pt2q.h), through pt2q_cholesky_inverse,
pt2q_hessian_inverse_batched (one word per item) and pt2q_quantize_layer.  The cases of
tests/breakdown_cases.py, which tests/test_breakdown_cases_cpu.py shows to reach both factoring
kernels (chol_diag_kernel, and rank_update2_kernel's fused factor), both panel-solve kernels, a
sub-panel and a panel boundary, a ragged last block, the look-ahead's side stream, and batch items
on both chunk positions.  After a breakdown Hinv is undefined and is not read; where the
factorisation succeeds it is the oracle's, bit for bit.  No tolerances."""
import numpy as np
import pytest
import torch

import breakdown_cases as bc
from test_gpu_parity import bits_equal, cuda, host
from test_gpu_strides import ACT, SSR, LoopOut, env

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x5A5A5A5A  # info_dev before every call: the call itself must zero the word


def _info_word(count=1):
    return torch.full((count,), SENTINEL, dtype=torch.int32, device=DEV)


def _inverse(pt2q, H, ws=None):
    """pt2q_cholesky_inverse on a packed H (numpy or device) -> (info, Hinv on the device); the
    return code must be PT2Q_OK whatever the word says."""
    L, lib, st = env(pt2q)
    Hd = H if isinstance(H, torch.Tensor) else cuda(H)
    m = Hd.shape[0]
    Hinv = torch.empty_like(Hd)
    info = _info_word()
    if ws is None:
        ws = L.workspace(lib.pt2q_cholesky_workspace_bytes(m), DEV)
    rc = lib.pt2q_cholesky_inverse(L.ptr(Hd), m, m, L.ptr(Hinv), m, L.ptr(ws), ws.numel(), L.ptr(info), st)
    assert rc == L.PT2Q_OK
    return int(info.item()), Hinv


# ------------------------------------------------------------------ pt2q_cholesky_inverse

@pytest.mark.parametrize("m,k", bc.PLANTED_CASES)
def test_planted_pivot(pt2q, m, k):
    """H[k][k] = 0 on a damped Hessian.  m = 100: 64 + a ragged 36 factored inside the strip-update
    launch; m = 333: every block by chol_diag_kernel and the four-lane panel kernel, last block 13;
    m = 576: the fused factor inside sub-panels, chol_diag_kernel behind the sub-panel term (256) and
    the panel term (512); first and last pivots of the blocks on both sides."""
    H = bc.planted(m, k)
    want = bc.oracle_info(H)
    assert want == k + 1
    assert _inverse(pt2q, H)[0] == want


@pytest.mark.parametrize("k", bc.LOOKAHEAD_K)
def test_planted_pivot_behind_the_lookahead(pt2q, k):
    """m = 6400: the pivot fails in a block behind the first fork (600), or behind a join and the
    second fork (1100), while the side stream still owes the later rows their terms."""
    H = bc.lookahead_planted(k)
    want = bc.oracle_info(H)
    assert want == k + 1
    assert _inverse(pt2q, H)[0] == want


@pytest.mark.parametrize("N,m", bc.EMERGENT)
def test_emergent_pivot(pt2q, N, m):
    """An undamped Gram of N < m rows: the pivot that fails comes out of the chains' last bits."""
    H, want = bc.emergent(N, m)
    assert N < want <= m
    assert _inverse(pt2q, H)[0] == want


@pytest.mark.parametrize("name", sorted(bc.SPECIAL))
def test_special_cases(pt2q, name):
    """First-wins (two negative pivots, the later one in a later block), a pivot that cancels to an
    exact zero, +0 and -0 pivots, and non-finite entries (only the word is defined for those:
    +inf on the diagonal is no breakdown)."""
    H = bc.special_case(name)
    want = bc.oracle_info(H)
    assert want == bc.SPECIAL[name]
    assert _inverse(pt2q, H)[0] == want


@pytest.mark.parametrize("name", sorted(bc.TINY))
def test_tiny_positive_pivot_is_no_breakdown(pt2q, name):
    """FLT_MIN and two subnormals as a pivot of the second block (which goes through the rank-64
    strip update and the fused factor): info = 0 and Hinv the oracle's bits, +inf at (70, 70) for
    the subnormals included."""
    H, U, ref = bc.tiny_case(name)
    info, Hinv = _inverse(pt2q, H)
    assert info == 0
    got = host(Hinv)
    assert not np.isnan(got).any()
    assert bits_equal(got, ref)


@pytest.mark.parametrize("m", bc.REUSE_M)
def test_healthy_call_after_a_breakdown(pt2q, m):
    """One breakdown call, then a healthy H of the same m on the same workspace and stream."""
    L, lib, st = env(pt2q)
    ws = L.workspace(lib.pt2q_cholesky_workspace_bytes(m), DEV)
    k = bc.REUSE[m]
    assert _inverse(pt2q, bc.planted(m, k), ws)[0] == k + 1
    info, Hinv = _inverse(pt2q, bc.healthy(m), ws)
    assert info == 0
    assert bits_equal(host(Hinv), bc.healthy_inverse(m))


def test_healthy_call_after_a_breakdown_behind_the_lookahead(pt2q):
    """m = 6400: the side stream's fork / join events after a failed factorisation.  The healthy
    result before the breakdown call (tied to the oracle by test_hessian_cholesky_inverse_bitexact)
    must come back afterwards, bit for bit."""
    L, lib, st = env(pt2q)
    m, k = bc.LOOKAHEAD_M, bc.LOOKAHEAD_K[1]
    ws = L.workspace(lib.pt2q_cholesky_workspace_bytes(m), DEV)
    H0 = cuda(bc.lookahead_healthy())
    info, want = _inverse(pt2q, H0, ws)
    assert info == 0
    assert _inverse(pt2q, bc.lookahead_planted(k), ws)[0] == k + 1
    info, got = _inverse(pt2q, H0, ws)
    assert info == 0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------ pt2q_hessian_inverse_batched

@pytest.mark.parametrize("chunk", bc.BATCH_CHUNKS)
@pytest.mark.parametrize("m", bc.BATCH_M)
def test_batched_items_report_their_own_pivots(pt2q, m, chunk):
    """Six items, four of them failing at different pivots (planted and emergent; at m = 320 in both
    factoring kernels), two healthy: every word is the oracle's, the healthy items equal the
    per-item call and the oracle.  chunk = 4: item 3 ends the first launch sequence, item 5 is
    item 1 of the second."""
    L, lib, st = env(pt2q)
    Gs, Hs, infos, Hinvs = bc.batch_case(m)
    assert infos == [want for _, _, want in bc.BATCH_ITEMS]
    G = cuda(np.stack(Gs))
    Hinv, info = pt2q.engine.hessian_inverse_batched(G, bc.BATCH_NSAMPLES, 0.0, info=_info_word(len(Gs)), chunk=chunk)
    assert host(info).tolist() == infos
    for z, want in enumerate(infos):
        H, _ = pt2q.prepare_hessian(G[z], bc.BATCH_NSAMPLES, 0.0)
        assert bits_equal(host(H), Hs[z]), z
        one_info, one = _inverse(pt2q, H)
        assert one_info == want, z
        if want == 0:
            assert bits_equal(host(Hinv[z]), host(one)), z
            assert bits_equal(host(Hinv[z]), Hinvs[z]), z


# ------------------------------------------------------------------ pt2q_quantize_layer

def test_fused_layer_reports_the_pivot(pt2q):
    """The whole-layer entry on N = 200 < m = 320 rows: undamped, outputs.info is the oracle's pivot
    of the undamped Hessian; damped, it is 0 and the layer is the oracle's.  No stall either time."""
    n, m, N, bs = bc.LAYER
    W, X, want, ref = bc.layer_case()
    Wd, Xd = cuda(W), cuda(X)
    out = pt2q.engine.quantize_layer(Wd, Xd, block_size=bs, use_ssr=True, percdamp=0.0, check_spd=False)
    assert int(out.info.item()) == want != 0
    assert int(out.status.reshape(-1)[0].item()) == 0
    out = pt2q.engine.quantize_layer(Wd, Xd, block_size=bs, use_ssr=True, percdamp=0.01, check_spd=False)
    assert int(out.info.item()) == 0
    assert int(out.status.reshape(-1)[0].item()) == 0
    np.testing.assert_array_equal(host(out.perm), ref["perm"])
    np.testing.assert_array_equal(host(out.T), ref["T"])
    assert bits_equal(host(out.alpha), ref["alpha"]) and bits_equal(host(out.mu), ref["mu"])
    np.testing.assert_array_equal(host(out.iters), ref["iters"])


def test_per_channel_layer_skips_the_factorisation(pt2q):
    """b >= m: one block reads no H⁻¹, so pt2q_quantize_layer skips the factorisation and reports
    success -- info_dev, preset to a sentinel, is 0 although this Hessian would break down."""
    L, lib, st = env(pt2q)
    n, m, N, b = bc.PER_CHANNEL
    W, X, would, ref = bc.per_channel_case()
    assert would != 0
    Wd, Xd = cuda(W), cuda(X)
    out = LoopOut(n, m, 1)
    info = _info_word()
    ws = L.workspace(lib.pt2q_layer_workspace_bytes(n, m, b, SSR | ACT), DEV)
    rc = lib.pt2q_quantize_layer(L.ptr(Wd), 0, m, n, m, L.ptr(Xd), 0, N, m, b, SSR | ACT, 0.0, 100, out.alpha.p,
                                 out.mu.p, out.T.p, 3, out.perm.p, out.iters.p, L.ptr(info), L.ptr(ws), ws.numel(), st)
    assert rc == L.PT2Q_OK
    L.check_status(ws, "pt2q_quantize_layer")
    assert int(info.item()) == 0
    out.check(ref)
