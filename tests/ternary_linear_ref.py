"""CPU helpers for the bit-exact tests of the MFMA ternary linear path (csrc/ternary_linear.hip:
tl_gemm_kernel<BF16, NT> + tl_reduce_kernel, tl_prefill_kernel) -- a plain helper, not a conftest.

The path accumulates in fp32 in an order that depends on the kernel, the K split and the MFMA, so
on random data it can only be held to a tolerance.  exact_case builds data on which that order
cannot matter: every operand is a small multiple of a power of two, so every product and every
partial sum, in any order, is an integer number of 1/64 below 2**20 in magnitude and hence exact
in fp32.  Any summation order, any K split and either 16-bit type must then give the same bits,
and exact_reference computes them in integers.

  T      in {-1, 0, 1}; rows 0, 1, 2 are all 0, all +1, all -1 (when n >= 3)
  alpha  a/16, a in 1..7; mu b/16, b in -4..4: drawn per (row, block), so a wrong row or block shows
  x      k/4, k in -8..8;  bias k/4, k in -32..32;  perm random
  weight (a c + b)/16, |a c + b| <= 11: four significant bits, exact in fp16 and in bf16

weight_tx is the dense weight of the contract (the kernel's header comment, oracle.ternary_weight's
docstring) for either 16-bit type, for scales that do need the TX rounding.  launch_path restates
the launcher's dispatch so that the tests can say, and check, which kernel a shape reaches."""
import functools

import numpy as np
import torch

from oracle import oracle as orc

F = np.float32
UNITS = 64            # one unit = 1/64 = (x step 1/4) * (weight step 1/16)
EXACT_BOUND = 2 ** 20  # |any partial sum| in units: 4 bits to spare below fp32's 2**24


def round16(a, dtype):
    """fp32 -> dtype ("fp16" | "bf16") -> fp32, round to nearest even."""
    a = np.array(a, dtype=F, order="C")
    if dtype == "fp16":
        return a.astype(np.float16).astype(F)
    return torch.from_numpy(a).bfloat16().float().numpy()


def nblocks(m, bs):
    return -(-m // bs)


def exact_case(n, m, bs, tokens, seed):
    """Exactly summable layer and activations (module docstring).  The *_int arrays are the integer
    numerators; alpha, mu, bias and x are the float32 values (exact in fp16 and bf16)."""
    rng = np.random.default_rng(seed)
    B = nblocks(m, bs)
    T = rng.integers(-1, 2, size=(n, m)).astype(np.int8)
    if n >= 3:
        T[0], T[1], T[2] = 0, 1, -1
    c = {"n": n, "m": m, "bs": bs, "tokens": tokens, "seed": seed, "T": T,
         "alpha_int": rng.integers(1, 8, size=(n, B)), "mu_int": rng.integers(-4, 5, size=(n, B)),
         "x_int": rng.integers(-8, 9, size=(tokens, m)), "bias_int": rng.integers(-32, 33, size=n),
         "perm": rng.permutation(m).astype(np.int64)}
    c["alpha"] = (c["alpha_int"] / 16).astype(F)
    c["mu"] = (c["mu_int"] / 16).astype(F)
    c["x"] = (c["x_int"] / 4).astype(F)
    c["bias"] = (c["bias_int"] / 4).astype(F)
    for k in ("alpha", "mu", "x", "bias"):
        assert np.array_equal(round16(c[k], "fp16"), c[k]) and np.array_equal(round16(c[k], "bf16"), c[k]), k
    return c


def weight_int(case, compat):
    """16 x the dense weight, int64, placed exactly as oracle.ternary_weight places it (its fp16
    values are exact on this data, so they serve bf16 as well)."""
    W = orc.ternary_weight(case["alpha"], case["mu"], case["T"], case["perm"], case["bs"], compat)
    W16 = W.astype(np.float64) * 16
    Wi = np.rint(W16).astype(np.int64)
    assert np.array_equal(Wi, W16) and np.abs(Wi).max() <= 11
    return Wi


@functools.lru_cache(maxsize=None)
def _units(n, m, bs, tokens, seed, compat):
    case = exact_case(n, m, bs, tokens, seed)
    Wi = weight_int(case, compat)
    xi = case["x_int"].astype(np.int64)
    # the bound that makes the data order-free: no partial sum of any subset of the terms of an
    # output, bias included, can reach 2**20 units
    worst = (np.abs(xi) @ np.abs(Wi).T).max() + 16 * np.abs(case["bias_int"]).max()
    assert worst < EXACT_BOUND, (worst, EXACT_BOUND)
    u = xi @ Wi.T
    u.setflags(write=False)
    return u


def exact_units(case, compat, bias):
    """The expected outputs as int64 numbers of 1/64 (x k/4 times weight w/16; a bias k/4 is 16 k)."""
    u = _units(case["n"], case["m"], case["bs"], case["tokens"], case["seed"], bool(compat))
    if bias:
        u = u + 16 * case["bias_int"].astype(np.int64)[None, :]
    assert np.abs(u).max() < EXACT_BOUND
    return u


def exact_reference(case, compat, bias=True, out="fp32"):
    """The expected output of an exact_case layer (tokens x n, float32 holding the values).
    out: "fp32", or "fp16" / "bf16" for an output in x's type ("tx"): the exact value rounded once,
    to nearest even, as the kernel's (TY) conversion rounds it."""
    y = (exact_units(case, compat, bias).astype(np.float64) / UNITS).astype(F)
    if out == "fp32":
        return y
    t = torch.from_numpy(y).to(torch.float16 if out == "fp16" else torch.bfloat16)
    return t.float().numpy()


def weight_tx(alpha, mu, T, perm, bs, compat, dtype):
    """Wd of the contract, n x m float32 holding the `dtype` values ("fp16" | "bf16"): alpha and mu
    rounded to dtype, alpha c + mu formed in fp32 and rounded to dtype, placed as
    oracle.ternary_weight places it (compat: contiguous blocks of T and the double permutation)."""
    if dtype == "fp16":
        return orc.ternary_weight(alpha, mu, T, perm, bs, compat)
    a, mm = round16(alpha, "bf16"), round16(mu, "bf16")
    T = np.asarray(T).astype(F)
    perm = np.asarray(perm, np.int64)
    n, m = T.shape
    b = bs if bs < m else m
    W = np.zeros((n, m), F)
    for k in range(a.shape[1]):
        s, e = k * b, min((k + 1) * b, m)
        cols = np.arange(s, e) if compat else perm[s:e]
        W[:, cols] = round16(a[:, k:k + 1] * T[:, cols] + mm[:, k:k + 1], "bf16")
    if compat:
        inv = np.argsort(perm)
        W = W[:, inv[inv]]
    return W


def launch_path(n, m, bs, tokens):
    """What pt2q_ternary_linear launches: ("prefill", 1, [P/128]) or ("gemm<NT>", splits, the
    128-position blocks of every split), by the launcher's rules and tl_plan."""
    P = -(-m // 128) * 128
    nkb = P // 128
    bse = bs if bs < m else P
    if tokens >= 256 and bse % 128 == 0:
        return "prefill", 1, [nkb]
    tile = 128 if tokens >= 512 else (64 if tokens >= 128 else 32)
    tiles = -(-n // 128) * -(-tokens // tile)
    splits = 1
    while splits < 16 and tiles * splits < 512 and nkb // (splits * 2) >= 2:
        splits *= 2
    kchunk = -(-nkb // splits)
    splits = -(-nkb // kchunk)
    NT = 4 if tokens >= 512 else (2 if tokens >= 128 else 1)
    return f"gemm<{NT}>", splits, [min(kchunk, nkb - z * kchunk) for z in range(splits)]


# 3a, exact GEMM: (n, m, bs, tokens, compat of the fp16 run; the bf16 run takes the other mode).
# Paths by launch_path; tests/test_ternary_linear_ref_cpu.py checks that the list covers what it
# claims to.  Blocks per split in brackets.
GEMM_SHAPES = [
    # --- K-split kernel, NT = 1 (tokens < 128)
    (1, 100, 16, 1, False),       # one split [1]; 16-position tables, 100 % 16 != 0; n = 1
    (40, 100, 128, 5, True),      # per-channel (bs >= m) on the K-split kernel
    (127, 200, 48, 31, True),     # [2]; the table switches inside a 128-position block
    (128, 1100, 80, 32, False),   # [3, 3, 3]; one full 32-token tile
    (129, 640, 192, 33, True),    # uneven [3, 2]; a second token tile of one row
    (200, 1600, 128, 127, False),  # [4, 4, 4, 1]
    (127, 130, 130, 33, False),   # per-channel, P = 256
    # --- K-split kernel, NT = 2 (tokens 128..255, or ..511 with bs % 128 != 0)
    (256, 2100, 128, 128, True),  # [3, 3, 3, 3, 3, 2]
    (257, 1100, 128, 129, False),
    (300, 640, 128, 255, True),
    (256, 1600, 192, 200, False),
    (129, 1100, 64, 256, True),   # 1100 % 64 != 0
    (40, 200, 48, 300, False),
    (200, 2100, 48, 511, True),   # ceil(P / bs) = 46 > B = 44: the last feature's padding scales lie past alpha
    (1, 640, 64, 511, False),
    # --- K-split kernel, NT = 4 (tokens >= 512, bs < m, bs % 128 != 0)
    (129, 640, 64, 512, False),
    (300, 100, 16, 513, True),
    (128, 1600, 16, 645, False),
    (257, 200, 16, 512, True),
    (1, 2100, 64, 513, True),
    (200, 200, 80, 645, False),
    (127, 1100, 64, 645, True),
    # --- prefill kernel (tokens >= 256 and (bs >= m or bs % 128 == 0))
    (1, 100, 128, 256, False),    # per-channel, P = 128: two stages, no second block fetch
    (127, 200, 128, 257, True),   # P = 256: one block fetch ahead; scale block 1 is ragged
    (128, 1100, 384, 383, False),  # 384-wide blocks, 1100 % 384 != 0
    (129, 384, 128, 384, True),
    (200, 1100, 256, 385, False),
    (256, 1100, 384, 513, True),  # exactly one 256-feature workgroup
    (257, 200, 256, 256, False),  # per-channel; a second workgroup of one feature
    (300, 1100, 128, 257, True),
    (129, 1100, 1100, 256, True),  # per-channel over 9 blocks
    (256, 100, 128, 384, True),
    (200, 384, 256, 300, False),  # 384 % 256 != 0
]

# 3c, scale arrays with a guard: ceil(P / bs) > B, so a padding position's p / bs is past the row
GUARD_SHAPES = [(40, 100, 16, 5), (40, 100, 16, 130), (40, 200, 48, 5), (40, 200, 48, 130)]

# 3d, stale pack
STALE_SHAPE = (40, 200, 64, 7)


def case_seed(n, m, bs, tokens):
    return 1000003 * n + 1009 * m + 31 * bs + tokens
