"""CPU restatement of the fused ternary decode kernel's arithmetic contract
in numpy float32 -- a plain helper for the decode tests, not a conftest.

  positions  p = 128 kb + 16 g + 8 h + j, P = m padded to 128; code c[i][p] = T[i][perm[p]]
             (compat: T[i][p]), gather[p] = perm[p] (compat: perm[perm[p]]), -1 / code 0 for p >= m
             (tl_pack_kernel, tl_gather_index_kernel); byte 32 kb + 16 h + 2 g + j/4 of a packed row
             holds code + 1 at bits 2 (j % 4)
  operands   w = RN_TX(mu + c alpha) with the fp32 alpha, mu of block min(p / bse, B - 1)
             (bse = bs if bs < m else P), xs = x[gather[p]] or +0
  piece      q = 2 kb + h: its 64 positions, g then j ascending; lane l owns q = l, l + 64, ...
  chain      acc = RN_f32(acc + w xs) from +0 (the product is exact, so this is fmaf)
  fold       v = v + v[lane ^ s], s = 32, 16, 8, 4, 2, 1;  y = RN_TY(v + bias)

alpha, mu and bias are the fp32 values the kernel is given (TernaryLinear hands it its 16-bit
buffers widened; round16 below does that rounding)."""
import numpy as np
import torch

F = np.float32


def round16(a, dtype):
    """fp32 -> dtype ("fp16" | "bf16") -> fp32, round to nearest even."""
    a = np.array(a, dtype=F, order="C")  # a copy: torch wants a writable array
    if dtype == "fp16":
        return a.astype(np.float16).astype(F)
    return torch.from_numpy(a).bfloat16().float().numpy()


def positions(m):
    return -(-m // 128) * 128


def piece_positions(P):
    """pos[q][16-bit slot 8 g + j] = 128 (q // 2) + 16 g + 8 (q % 2) + j."""
    q = np.arange(P // 64)[:, None, None]
    g = np.arange(8)[None, :, None]
    j = np.arange(8)[None, None, :]
    return (128 * (q // 2) + 16 * g + 8 * (q % 2) + j).reshape(P // 64, 64)


def pack(T, perm, compat):
    """(c, gather): codes at positions (int8 n x P) and the gather index (int32 P)."""
    T = np.asarray(T, np.int8)
    perm = np.asarray(perm, np.int64)
    n, m = T.shape
    P = positions(m)
    c = np.zeros((n, P), np.int8)
    c[:, :m] = T[:, :m] if compat else T[:, perm]
    gather = np.full(P, -1, np.int32)
    gather[:m] = perm[perm] if compat else perm
    return c, gather


def packed_bytes(c):
    """The n x P/4 bytes pt2q_ternary_pack writes for position codes c."""
    n, P = c.shape
    b = np.arange(P // 4)
    kb, h, g, j0 = b // 32, (b % 32) // 16, (b % 16) // 2, (b % 2) * 4
    out = np.zeros((n, P // 4), np.uint8)
    for s in range(4):
        p = 128 * kb + 16 * g + 8 * h + j0 + s
        out |= ((c[:, p] + 1).astype(np.uint8) << (2 * s)).astype(np.uint8)
    return out


def operands(x, alpha, mu, T, perm, bs, dtype, compat):
    """(w, xs): the rounded weights n x P and the gathered activations tokens x P, fp32."""
    x = round16(np.atleast_2d(x), dtype)
    alpha, mu = np.asarray(alpha, F), np.asarray(mu, F)
    c, gather = pack(T, perm, compat)
    n, P = c.shape
    m = np.asarray(T).shape[1]
    B = alpha.shape[1]
    bse = bs if bs < m else P
    blk = np.minimum(np.arange(P) // bse, B - 1)
    # the three weights of every (row, block): RN_TX(mu - alpha), RN_TX(mu), RN_TX(mu + alpha)
    tab = round16(np.stack([mu - alpha, mu, mu + alpha], axis=2), dtype).reshape(n, 3 * B)
    w = np.take_along_axis(tab, 3 * blk[None, :] + (c.astype(np.int64) + 1), axis=1)
    xs = np.where(gather >= 0, x[:, np.maximum(gather, 0)], F(0)).astype(F)
    return w, xs


def fold(x, alpha, mu, T, perm, bs, dtype, compat=False, check_exact=False):
    """v (tokens x n, fp32): the folded sum of DOT64P before the bias add and the output rounding.
    check_exact: also assert that every product is exact in fp32."""
    w, xs = operands(x, alpha, mu, T, perm, bs, dtype, compat)
    n, P = w.shape
    tokens = xs.shape[0]
    pos = piece_positions(P)
    npieces = P // 64
    nround = -(-npieces // 64)
    # seq[step][lane]: the lane's positions in chain order (-1: no piece)
    seq = np.full((nround * 64, 64), -1, np.int64)
    for k in range(nround):
        own = np.arange(64 * k, min(64 * (k + 1), npieces))
        seq[64 * k:64 * (k + 1), own - 64 * k] = pos[own].T
    valid = seq >= 0
    sq = np.maximum(seq, 0)
    xl = np.where(valid[..., None], xs.T[sq], F(0)).astype(F)  # steps x 64 x tokens
    v = np.zeros((tokens, n), F)
    lanes = np.arange(64)
    wt = np.ascontiguousarray(w.T)  # P x n
    for r0 in range(0, n, 1024):
        wl = np.where(valid[..., None], wt[:, r0:r0 + 1024][sq], F(0)).astype(F)  # steps x 64 x rows
        acc = np.zeros((64, tokens, wl.shape[2]), F)
        for s in range(seq.shape[0]):
            prod = wl[s][:, None, :] * xl[s][:, :, None]
            if check_exact:
                p64 = wl[s][:, None, :].astype(np.float64) * xl[s][:, :, None].astype(np.float64)
                assert np.array_equal(prod.astype(np.float64), p64)
            acc += prod  # fp32 add of the exact product: fmaf
        assert acc.dtype == F
        for s in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ s]
        v[:, r0:r0 + 1024] = acc[0]
    return v


def finish(v, bias, dtype, out_dtype=None):
    """y = RN_TY(v + bias): one fp32 add (none without bias), one rounding (none for "fp32")."""
    y = np.asarray(v, F)
    if bias is not None:
        y = y + np.asarray(bias, F)[None, :]
    assert y.dtype == F
    return y.copy() if out_dtype == "fp32" else round16(y, dtype)


def decode(x, alpha, mu, T, perm, bias, bs, dtype, compat=False, out_dtype=None, check_exact=False):
    """y (tokens x n, float32 holding the out_dtype values) by DOT64P.  out_dtype: None (= dtype)
    or "fp32"."""
    return finish(fold(x, alpha, mu, T, perm, bs, dtype, compat, check_exact), bias, dtype, out_dtype)


# (n, m, bs, tokens, dtype): what the decode tests run (tests/test_ternary_decode_cpu.py,
# tests/test_gpu_ternary_decode.py)
SHAPES = [(33, 100, 16, 2, "fp16"),        # 2 pieces, 62 idle lanes; 16-position tables; block clamp; ragged n
          (40, 1030, 64, 8, "bf16"),       # the clamp on a ragged m
          (96, 1100, 128, 3, "fp16"),      # ragged m with a 128 block
          (70, 520, 520, 5, "bf16"),       # per-channel
          (130, 8320, 128, 8, "fp16"),     # 130 pieces: lanes 0 and 1 own a third piece
          (4096, 4096, 128, 1, "fp16"),    # the workload's own shape
          (4096, 11008, 128, 4, "bf16")]   # the wide workload shape


def make_case(n, m, bs, tokens, dtype, seed=None):
    """Random layer and activations in the value ranges of tests/test_gpu_ternary.py, scales, bias
    and x already rounded to dtype (what TernaryLinear hands the kernel)."""
    import synth
    rng = np.random.default_rng(n + m + tokens if seed is None else seed)
    B = -(-m // bs)
    case = {"n": n, "m": m, "bs": bs, "tokens": tokens, "dtype": dtype,
            "T": rng.integers(-1, 2, size=(n, m)).astype(np.int8),
            "alpha": round16(rng.random((n, B)) * 0.05 + 0.005, dtype),
            "mu": round16(rng.standard_normal((n, B)) * 0.002, dtype),
            "perm": rng.permutation(m).astype(np.int64),
            "bias": round16(rng.standard_normal(n) * 0.1, dtype),
            "x": round16(synth.activations(7 + tokens, tokens, m), dtype)}
    return case


_FOLD = {}


def reference(case, bias=True, out_dtype=None, compat=False):
    """decode() of a make_case case; the fold is computed once per (case, compat) and shared."""
    key = (case["n"], case["m"], case["bs"], case["tokens"], case["dtype"], compat)
    if key not in _FOLD:
        v = fold(case["x"], case["alpha"], case["mu"], case["T"], case["perm"], case["bs"], case["dtype"], compat)
        v.setflags(write=False)
        _FOLD[key] = v
    return finish(_FOLD[key], case["bias"] if bias else None, case["dtype"], out_dtype)
