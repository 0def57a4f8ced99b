"""CPU restatement of the layer report's arithmetic contract (DESIGN.md §3 "Layer report") from
existing oracle entries and numpy float32 -- a plain helper for the report tests, not a conftest.

  residual   D_ic = RN(W_ic - RN(RN(alpha_ik t_ic) + mu_ik)), k the block of column c's position
  chain      P = A G, every entry the k-ascending fmaf chain from +0 (oracle.gram on [Aᵀ | G])
  ROWTREE    32-wide chunks (+0 past the end), halving tree per chunk, chunks added ascending from +0
"""
import numpy as np

from oracle import oracle as orc

F = np.float32


def block_of_column(m, b, perm=None):
    """blockof[c] = p // bb for the position p with perm[p] = c (b, B clamped as pt2q_dequantize)."""
    bb = b if b < m else m
    pos = np.arange(m) if perm is None else np.asarray(perm, np.int64)
    blockof = np.zeros(m, np.int64)
    blockof[pos] = np.arange(m) // bb
    return blockof


def dequantized(alpha, mu, T, b, perm=None):
    alpha, mu = np.asarray(alpha, F), np.asarray(mu, F)
    k = block_of_column(T.shape[1], b, perm)
    return (alpha[:, k] * np.asarray(T).astype(F)).astype(F) + mu[:, k]


def residual(W, alpha, mu, T, b, perm=None):
    """W must already be the exact fp32 upcast of the layer's weights."""
    D = np.asarray(W, F) - dequantized(alpha, mu, T, b, perm)
    assert D.dtype == F
    return D


def chain_product(A, G):
    """P[i][j] = fmaf chain over k ascending of A[i][k] * G[k][j], from +0."""
    A, G = np.ascontiguousarray(A, F), np.ascontiguousarray(G, F)
    n = A.shape[0]
    return orc.gram(np.ascontiguousarray(np.hstack([A.T, G])))[:n, n:]


def rowtree(R):
    """ROWTREE along the last axis of a float32 array."""
    R = np.asarray(R, F)
    L = R.shape[-1]
    nch = -(-L // 32)
    v = np.zeros(R.shape[:-1] + (nch * 32,), F)
    v[..., :L] = R
    v = v.reshape(R.shape[:-1] + (nch, 32))
    h = 16
    while h >= 1:
        v = v[..., :h] + v[..., h:2 * h]
        h //= 2
    v = v[..., 0]
    s = np.zeros(R.shape[:-1], F)
    for c in range(nch):
        s = s + v[..., c]
    assert s.dtype == F
    return s


def quadform(A, G):
    """q[i] = ROWTREE_j RN(P_ij a_ij), P = A G the chain."""
    A = np.asarray(A, F)
    return rowtree(chain_product(A, G) * A)


def report(W, alpha, mu, T, b, perm=None, G=None, reference=True):
    """{"ew", "ex", "ey", "totals"} as pt2q_layer_report writes them (None where not computed;
    totals 0 there)."""
    W = np.asarray(W, F)
    D = residual(W, alpha, mu, T, b, perm)
    n = W.shape[0]
    ew = rowtree(D * D)
    ex = ey = None
    if G is not None:
        if reference:  # one chain product for both, as the kernel's one launch
            q = quadform(np.vstack([D, W]), G)
            ex, ey = q[:n], q[n:]
        else:
            ex = quadform(D, G)
    z = F(0)
    totals = np.array([rowtree(ew), rowtree(ex) if ex is not None else z,
                       rowtree(ey) if ey is not None else z], F)
    return {"ew": ew, "ex": ex, "ey": ey, "totals": totals, "D": D}


def error_bound(D, G, nrows=None):
    """The derived bound on |computed - exact| of the total Σ_i d_i G d_iᵀ for f32 D and G:
    (m + ceil(m/32) + ceil(n/32) + 16) 2^-23 Σ_i |d_i| |G| |d_i|ᵀ  (gamma_m of the chain, one
    rounding of the product, the depths of the two trees, doubled for higher-order terms)."""
    D64, G64 = np.abs(np.asarray(D, np.float64)), np.abs(np.asarray(G, np.float64))
    n, m = D64.shape
    mag = float(((D64 @ G64) * D64).sum())
    return (m + -(-m // 32) + -(-n // 32) + 16) * 2.0 ** -23 * mag


def exact_total(D, G):
    D64, G64 = np.asarray(D, np.float64), np.asarray(G, np.float64)
    return float(((D64 @ G64) * D64).sum())
