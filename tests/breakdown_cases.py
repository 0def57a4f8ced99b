"""The Cholesky breakdown word (include/pt2q.h: info_dev = 0, or k + 1 for the first non-positive
pivot) on every factorisation path -- a plain helper, not a conftest.

The diagonal blocks are factored in two places, both through chol_diag.hpp's diag_factor and its
first-wins report: chol_diag_kernel (chol.hip: the first block of every 256-row sub-panel, and every
block when the strip update is not the rank-<=128 kernel) and rank_update2_kernel (gemm.hip: the next
block inside the strip-update launch).  This module holds

  * the case tables of tests/test_gpu_breakdown.py -- matrices whose first failing pivot k is known,
    planted on the diagonal or emerging from cancellation -- with the builders of H / G and the
    CPU-oracle expectations (orc.cholesky_upper returns the same k + 1 under the same fmaf chains), and
  * factoring_step(m, k, batch): which launch factors the block that holds pivot k and what precedes
    it, read off ragged_cases.chol_schedule, so that tests/test_breakdown_cases_cpu.py can check,
    without a GPU, that the pivots reach both kernels, a sub-panel and a panel boundary, a ragged last
    block and the look-ahead's side stream.

Every expectation is an integer or a bit pattern; there are no tolerances."""
import collections
import functools

import numpy as np

import ragged_cases as rc
import synth
from oracle import oracle as orc

NB, SP = rc.NB, rc.SP

# ------------------------------------------------------------------ which launch factors pivot k

Step = collections.namedtuple("Step", "kernel solve after forks joins p0 nb")
Step.__doc__ = """kernel: "diag" (chol_diag_kernel) or "fused" (rank_update2_kernel's RuDiag); solve: the
panel-solve kernel of the block ("lane" / "lpr"); after: what was launched since the previous block --
"start", "strip", "subpanel" (the rank-256 launch_big pair) or "panel" (the rank-CP launch_big terms);
forks / joins: side-stream forks and joins issued before the block; p0, nb: the block."""


def factoring_step(m, k, batch=1):
    """The step of pt2q_launch_cholesky_inverse that factors the diagonal block holding pivot k
    (0-based), by a walk over ragged_cases.chol_schedule(m, batch).  Blocks start at multiples of NB
    (sub-panels and panels are whole blocks; only the matrix's last block is ragged), a block the
    strip update did not factor has its own ("diag", ...) entry, a sub-panel's terms are a pair of
    "big" entries of K = SP and a panel's a pair of K = CP -- or two pairs, the second on the side
    stream behind a fork (which the next panel boundary joins before its own terms)."""
    assert 0 <= k < m
    want, j = k // NB, -1
    own, since, forks, joins, pending = False, [], 0, 0, False
    for step, kind, d in rc.chol_schedule(m, batch):
        if step == "diag":
            own = True
        elif step == "strip":
            since.append(("strip", kind))
        elif step == "big":
            since.append(("big", d["K"]))
        elif step == "block":
            j += 1
            bigs = [K for s, K in since if s == "big"]
            if bigs and bigs[0] != SP:  # a panel boundary
                assert len(bigs) in (2, 4) and len(set(bigs)) == 1 and bigs[0] in (512, 1024), bigs
                joins += pending
                pending = len(bigs) == 4
                forks += pending
            if j == want:
                after = "start" if not since else "strip" if not bigs else "subpanel" if bigs[0] == SP else "panel"
                # the schedule's own rule: a block has its own factor launch unless the strip update
                # before it was the rank-<=128 kernel
                assert own == (since != [("strip", "rank_update2")])
                assert d == min(NB, m - want * NB)
                return Step("diag" if own else "fused", kind, after, forks, joins, want * NB, d)
            own, since = False, []
    raise AssertionError((m, k))


# ------------------------------------------------------------------ case tables

# planted: H = prepare_hessian(gram(activations(seed, N, m)), N, 0.01) with H[k][k] = 0.0 -> info = k + 1
PLANTED = {
    100: (160, (0, 63, 64, 99)),                     # 64 + a ragged 36, fused with dnb = 36
    333: (400, (0, 64, 255, 256, 320, 332)),         # m % 4: every block by chol_diag_kernel, last block 13
    576: (700, (0, 63, 64, 65, 127, 128, 191, 255, 256, 257, 511, 512, 513, 575)),  # a panel boundary at 512
}
PLANTED_CASES = [(m, k) for m, (_, ks) in PLANTED.items() for k in ks]
# a healthy H of the same m after a breakdown call: m -> the pivot of that call (100: the fused ragged
# block; 333: behind the sub-panel term; 576: the fused factor)
REUSE = {100: 64, 333: 256, 576: 128}
REUSE_M = tuple(REUSE)

# the look-ahead (m > 6144): the cheap SPD matrix of test_gpu_strides._inverse_ref with H[k][k] = -1;
# 600 lies behind the first fork, 1100 behind a join and the second fork.  No late pivots at this
# width: the oracle stops at the pivot.
LOOKAHEAD_M = 6400
LOOKAHEAD_K = (600, 1100)

# emergent: H = prepare_hessian(G, N, 0.0) of an undamped rank-deficient Gram (N < m), seed 7 + m; the
# pivot is the oracle's, N < info <= m (a cancellation breakdown, decided by the last bits).
EMERGENT = [(100, 300), (200, 320), (130, 577), (600, 1100)]   # (N, m)

# name -> info the oracle must give (test_breakdown_cases_cpu.py); built by special_case(name)
SPECIAL = {
    "first_wins": 71,      # m = 576, H[130][130] = H[70][70] = -1
    "cancel_to_zero": 101, # I_128 with H[3][100] = H[100][3] = 1: pivot 100 is exactly 1 - 1 * 1 = 0
    "plus_zero": 71,       # I_128 with H[70][70] = +0.0
    "minus_zero": 71,      # ... = -0.0
    # non-finite H on the m = 576 base: only info is defined
    "nan_diag": 201,       # NaN at (200, 200)
    "nan_offdiag": 301,    # NaN at (10, 300), mirrored
    "inf_offdiag": 301,    # +inf at (10, 300), mirrored
    "neg_inf_diag": 91,    # -inf at (90, 90)
    "pos_inf_diag": 0,     # +inf at (90, 90): sqrt(inf) = inf, the row becomes 0 -- no breakdown
}

# tiny positive pivots that are no breakdowns: I_128 with H[70][70] = the value; info = 0 and Hinv
# the oracle's bits (Hinv[70][70] = +inf for the two subnormals)
TINY = {"flt_min": np.float32(np.finfo(np.float32).tiny), "1e-40": np.float32(1e-40),
        "denorm_min": np.float32(1.4e-45)}

# batch (through G: the batched entry damps inside the call): percdamp = 0.0 and nsamples = 4096 for the
# whole call, item z from activations(100 + m + z, N_z, m); (N_z, negated diagonal entry of G, info)
BATCH_M = (320, 333)
BATCH_NSAMPLES = 4096
BATCH_ITEMS = [(400, None, 0), (200, None, 201), (400, 70, 71), (400, 256, 257), (450, None, 0), (150, None, 152)]
BATCH_CHUNKS = (32, 4)   # chunk 4: item 3 ends the first call, items 4 and 5 are items 0 and 1 of the second

# the fused layer: (n, m, N, block size); X is the (200, 320) emergent case's activations
LAYER = (64, 320, 200, 128)
# per-channel (b >= m): the factorisation is skipped by contract and info reports success
PER_CHANNEL = (64, 576, 200, 1024)


# ------------------------------------------------------------------ builders

@functools.lru_cache(maxsize=None)
def _base(m):
    N = PLANTED[m][0]
    H, _ = orc.prepare_hessian(orc.gram(synth.activations(31 + m, N, m)), N, 0.01)
    H.setflags(write=False)
    return H


def healthy(m):
    """The damped Hessian the planted cases of width m start from."""
    return _base(m).copy()


def planted(m, k):
    H = _base(m).copy()
    H[k, k] = 0.0
    return H


@functools.lru_cache(maxsize=None)
def healthy_inverse(m):
    Hinv, spd = orc.cholesky_inverse(_base(m))
    assert spd
    return Hinv


@functools.lru_cache(maxsize=1)
def lookahead_base():
    m = LOOKAHEAD_M
    orc.set_threads(16)
    H = (orc.gram(synth.activations(961 + m, 128, m)) / np.float32(128) + np.eye(m, dtype=np.float32))
    H = H.astype(np.float32)
    H.setflags(write=False)
    return H


def lookahead_healthy():
    return lookahead_base().copy()


def lookahead_planted(k):
    H = lookahead_base().copy()
    H[k, k] = -1.0
    return H


@functools.lru_cache(maxsize=None)
def emergent_x(N, m):
    return synth.activations(7 + m, N, m)


@functools.lru_cache(maxsize=None)
def emergent(N, m):
    """-> (H, info): the undamped Hessian of N < m rows and the oracle's first failing pivot."""
    H, _ = orc.prepare_hessian(orc.gram(emergent_x(N, m)), N, 0.0)
    return H, oracle_info(H)


def _eye(k=None, v=None):
    H = np.eye(128, dtype=np.float32)
    if k is not None:
        H[k, k] = v
    return H


def special_case(name):
    if name == "cancel_to_zero":
        H = _eye()
        H[3, 100] = H[100, 3] = 1.0
        return H
    if name in ("plus_zero", "minus_zero"):
        return _eye(70, np.float32(0.0) if name == "plus_zero" else np.float32(-0.0))
    H = _base(576).copy()
    if name == "first_wins":
        H[130, 130] = H[70, 70] = -1.0
    elif name == "nan_diag":
        H[200, 200] = np.nan
    elif name == "nan_offdiag":
        H[10, 300] = H[300, 10] = np.nan
    elif name == "inf_offdiag":
        H[10, 300] = H[300, 10] = np.inf
    elif name == "neg_inf_diag":
        H[90, 90] = -np.inf
    elif name == "pos_inf_diag":
        H[90, 90] = np.inf
    else:
        raise KeyError(name)
    return H


@functools.lru_cache(maxsize=None)
def tiny_case(name):
    """-> (H, U, Hinv) of the oracle; the factorisation must succeed."""
    H = _eye(70, TINY[name])
    U, info = orc.cholesky_upper(H)
    assert info == 0
    Hinv, spd = orc.cholesky_inverse(H)
    assert spd
    return H, U, Hinv


def oracle_info(H):
    return orc.cholesky_upper(H)[1]


@functools.lru_cache(maxsize=None)
def batch_case(m):
    """-> (Gs, Hs, infos, Hinvs): raw Grams, the oracle's undamped Hessians over BATCH_NSAMPLES, its
    pivots, and its inverses of the healthy items (None for the others)."""
    Gs, Hs, infos, Hinvs = [], [], [], []
    for z, (N, neg, _) in enumerate(BATCH_ITEMS):
        G = orc.gram(synth.activations(100 + m + z, N, m))
        if neg is not None:
            G[neg, neg] = -G[neg, neg]
        H, damp = orc.prepare_hessian(G, BATCH_NSAMPLES, 0.0)
        assert damp == 0.0
        info = oracle_info(H)
        Gs.append(G); Hs.append(H); infos.append(info)
        Hinvs.append(orc.cholesky_inverse(H)[0] if info == 0 else None)
    return Gs, Hs, infos, Hinvs


@functools.lru_cache(maxsize=None)
def layer_case():
    """-> (W, X, info at percdamp 0, oracle layer at percdamp 0.01)."""
    n, m, N, bs = LAYER
    W, X = synth.weights(7 + n, n, m), emergent_x(N, m)
    return W, X, emergent(N, m)[1], orc.quantize_layer_m(W, X, block_size=bs, use_ssr=True, percdamp=0.01)


@functools.lru_cache(maxsize=None)
def per_channel_case():
    """-> (W, X, the oracle's pivot of the Hessian the call skips, oracle block loop): one block, so
    H⁻¹ is never read (the zeros stand for it)."""
    n, m, N, b = PER_CHANNEL
    W, X = synth.weights(7 + n, n, m), emergent_x(N, m)
    G = orc.gram(X)
    H, _ = orc.prepare_hessian(G, N, 0.0)
    return W, X, oracle_info(H), orc.quantize_blocks(W, G, np.zeros((m, m), np.float32), b, True, 1)
