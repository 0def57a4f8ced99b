"""The helpers of the bit-exact MFMA ternary linear tests (tests/ternary_linear_ref.py) on the CPU:
the integer reference against the oracle and a float64 product, weight_tx against the oracle on
the reference's fixtures, the exactness bound at every shape the GPU tests use, and that the shape
list reaches every kernel instantiation, tile edge and block size it is there for."""
import numpy as np
import pytest

import ternary_linear_ref as ref
from conftest import load_golden
from oracle import oracle as orc

SMALL = [(5, 100, 16, 3), (40, 200, 48, 9), (33, 640, 192, 17), (7, 130, 130, 4), (20, 1100, 128, 33)]


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("n,m,bs,tokens", SMALL)
def test_exact_reference_equals_oracle_fp16(n, m, bs, tokens, compat):
    """On exactly summable data the oracle's float64 sum rounded to fp16 is the exact value rounded
    once: the integer reference must give the same bits, with and without bias."""
    c = ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens))
    for bias in (True, False):
        yo = orc.ternary_linear(c["x"], c["alpha"], c["mu"], c["T"], c["perm"], c["bias"] if bias else None,
                                bs, compat=compat)
        assert yo.dtype == np.float16
        y = ref.exact_reference(c, compat, bias, out="fp16")
        assert np.array_equal(y.astype(np.float16).view(np.uint16), yo.view(np.uint16))


@pytest.mark.parametrize("compat", [False, True])
@pytest.mark.parametrize("n,m,bs,tokens", SMALL)
def test_exact_reference_equals_float64_product(n, m, bs, tokens, compat):
    c = ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens))
    for dtype in ("fp16", "bf16"):
        W = ref.weight_tx(c["alpha"], c["mu"], c["T"], c["perm"], bs, compat, dtype).astype(np.float64)
        y64 = c["x"].astype(np.float64) @ W.T
        assert np.array_equal(ref.exact_reference(c, compat, bias=False).astype(np.float64), y64)
        y64 = y64 + c["bias"].astype(np.float64)
        assert np.array_equal(ref.exact_reference(c, compat, bias=True).astype(np.float64), y64)


def test_exact_case_layout():
    c = ref.exact_case(6, 200, 48, 4, 11)
    assert c["alpha"].shape == c["mu"].shape == (6, 5)
    assert (c["T"][0] == 0).all() and (c["T"][1] == 1).all() and (c["T"][2] == -1).all()
    assert set(np.unique(c["T"])) <= {-1, 0, 1}
    assert c["alpha_int"].min() >= 1 and c["alpha_int"].max() <= 7 and np.abs(c["mu_int"]).max() <= 4
    assert np.abs(c["x_int"]).max() <= 8 and np.abs(c["bias_int"]).max() <= 32
    assert np.array_equal(np.sort(c["perm"]), np.arange(200))
    # rows of constant codes: weight = mu, mu + alpha, mu - alpha of the column's block
    Wi = ref.weight_int(c, compat=False)
    blk = np.empty(200, np.int64)
    blk[c["perm"]] = np.arange(200) // 48
    assert np.array_equal(Wi[0], c["mu_int"][0][blk])
    assert np.array_equal(Wi[1], (c["mu_int"][1] + c["alpha_int"][1])[blk])
    assert np.array_equal(Wi[2], (c["mu_int"][2] - c["alpha_int"][2])[blk])


@pytest.mark.parametrize("name", ["ternary_linear_384x512", "ternary_linear_200x1000_pc"])
def test_weight_tx_fp16_is_the_oracle_weight(name):
    g = load_golden(name)
    bs = int(g["block_size"])
    for compat in (False, True):
        W = ref.weight_tx(g["alpha"], g["mu"], g["T"], g["perm"], bs, compat, "fp16")
        assert np.array_equal(W, orc.ternary_weight(g["alpha"], g["mu"], g["T"], g["perm"], bs, compat))
        # bf16: the same placement (the two weights agree to bf16's rounding of the fp32 value)
        Wb = ref.weight_tx(g["alpha"], g["mu"], g["T"], g["perm"], bs, compat, "bf16")
        assert np.array_equal(Wb, ref.round16(Wb, "bf16"))
        a, mm = ref.round16(g["alpha"], "bf16"), ref.round16(g["mu"], "bf16")
        full = orc.ternary_weight(a, mm, g["T"], g["perm"], bs, compat, dtype=np.float32)
        assert np.array_equal(Wb, ref.round16(full, "bf16"))


@pytest.mark.parametrize("n,m,bs,tokens", [s[:4] for s in ref.GEMM_SHAPES] + ref.GUARD_SHAPES + [ref.STALE_SHAPE])
def test_exactness_bound_holds(n, m, bs, tokens):
    """exact_units asserts |any partial sum| < 2**20 units; here for every GPU shape, both modes."""
    c = ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens))
    for compat in (False, True):
        u = ref.exact_units(c, compat, bias=True)
        assert u.dtype == np.int64 and np.abs(u).max() < ref.EXACT_BOUND
        y = ref.exact_reference(c, compat, True)
        assert np.array_equal(y.astype(np.float64) * ref.UNITS, u)  # fp32 holds the value exactly


def test_launch_path_examples():
    """The dispatch restated in launch_path, at the cases the launcher's comments name."""
    assert ref.launch_path(1000, 1100, 128, 300) == ("prefill", 1, [9])
    assert ref.launch_path(1000, 1100, 128, 255)[0] == "gemm<2>"
    assert ref.launch_path(40, 100, 16, 5) == ("gemm<1>", 1, [1])
    assert ref.launch_path(40, 200, 48, 130) == ("gemm<2>", 1, [2])
    assert ref.launch_path(129, 640, 64, 512) == ("gemm<4>", 2, [3, 2])
    assert ref.launch_path(128, 1100, 80, 32) == ("gemm<1>", 3, [3, 3, 3])
    assert ref.launch_path(200, 1600, 128, 127) == ("gemm<1>", 4, [4, 4, 4, 1])
    assert ref.launch_path(256, 2100, 128, 128) == ("gemm<2>", 6, [3, 3, 3, 3, 3, 2])
    assert ref.launch_path(600, 640, 640, 513)[0] == "prefill"   # per-channel
    assert ref.launch_path(600, 640, 64, 513)[0] == "gemm<4>"


def test_pack_is_dropped_when_buffers_can_change(pt2q):
    """TernaryLinear._packed is derived from the buffers: a state-dict load and every _apply, on the
    module or on a parent, must drop it (host logic only: CPU buffers, a stand-in pack)."""
    import torch
    mk = lambda: pt2q.TernaryLinear(32, 4, 16, dtype=torch.float16, device="cpu")  # noqa: E731
    other = mk()
    other.alpha.fill_(0.5)
    for act in (lambda l, p: l.load_state_dict(other.state_dict()), lambda l, p: p.load_state_dict(
                torch.nn.Sequential(other).state_dict()), lambda l, p: l.bfloat16(), lambda l, p: p.half(),
                lambda l, p: l.to("cpu"), lambda l, p: p.float()):
        lay = mk()
        parent = torch.nn.Sequential(lay)
        lay._packed = ("stale",)
        act(lay, parent)
        assert lay._packed is None
    lay = mk()
    lay.load_state_dict(other.state_dict())
    assert torch.equal(lay.alpha, other.alpha)
    assert lay.bfloat16().dtype == torch.bfloat16


def test_gemm_shapes_cover_what_they_claim():
    runs = []  # (kernel, dtype, compat, n, m, bs, tokens)
    for n, m, bs, tokens, c16 in ref.GEMM_SHAPES:
        assert n <= 300 and m <= 2100
        k = ref.launch_path(n, m, bs, tokens)[0]
        runs += [(k, "fp16", c16, n, m, bs, tokens), (k, "bf16", not c16, n, m, bs, tokens)]
    assert 40 <= len(runs) <= 70
    kernels = ("gemm<1>", "gemm<2>", "gemm<4>", "prefill")
    for k in kernels:  # every instantiation with both compat modes
        for dt in ("fp16", "bf16"):
            assert {r[2] for r in runs if r[0] == k and r[1] == dt} == {False, True}, (k, dt)

    def have(kern, **kw):
        idx = {"n": 3, "m": 4, "bs": 5, "tokens": 6}
        sel = [r for r in runs if r[0] in kern and all(r[idx[a]] == v for a, v in kw.items())]
        return {r[1] for r in sel} == {"fp16", "bf16"}

    for t in (1, 31, 32, 33, 127):
        assert have(("gemm<1>",), tokens=t), t
    for t in (128, 129, 255):
        assert have(("gemm<2>",), tokens=t, bs=128), t
    for t in (256, 300, 511):
        assert any(have(("gemm<2>",), tokens=t, bs=b) for b in (64, 48)), t
    assert all(any(have(("gemm<2>",), tokens=t, bs=b) for t in (256, 300, 511)) for b in (64, 48))
    for t in (512, 513, 645):
        assert any(have(("gemm<4>",), tokens=t, bs=b) for b in (64, 16)), t
    assert all(any(have(("gemm<4>",), tokens=t, bs=b) for t in (512, 513, 645)) for b in (64, 16))
    gemm = kernels[:3]
    for m_ in (100, 200, 640, 1100, 1600, 2100):
        assert have(gemm, m=m_), m_
    split_sets = {tuple(ref.launch_path(*s[:4])[2]) for s in ref.GEMM_SHAPES if ref.launch_path(*s[:4])[0] != "prefill"}
    assert {(1,), (2,), (3, 2), (3, 3, 3), (4, 4, 4, 1), (3, 3, 3, 3, 3, 2)} <= split_sets
    for t in (256, 257, 383, 384, 385, 513):
        assert have(("prefill",), tokens=t), t
    for m_ in (100, 200, 384, 1100):
        assert have(("prefill",), m=m_), m_
    for b in (128, 256, 384):
        assert any(r[0] == "prefill" and r[5] == b and b < r[4] for r in runs), b
    assert any(r[0] == "prefill" and r[5] >= r[4] for r in runs)
    for n_ in (1, 127, 128, 129, 200, 256, 257, 300):
        assert have(gemm, n=n_) and have(("prefill",), n=n_), n_
    for b in (16, 48, 64, 80, 192):
        assert any(r[0] in gemm and r[5] == b and r[4] % b != 0 and b < r[4] for r in runs), b
    for s in ref.GUARD_SHAPES:  # the block index of a padding position is past the row's scales
        n, m, bs, tokens = s
        assert ref.launch_path(*s)[0] in ("gemm<1>", "gemm<2>")
        assert -(-(-(-m // 128) * 128) // bs) > ref.nblocks(m, bs)
