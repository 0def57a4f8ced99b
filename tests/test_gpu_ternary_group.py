"""The grouped decode entry (pt2q_ternary_decode_group, csrc/ternary_decode.hip): a PLAIN
group against pt2q_ternary_decode on each member alone and the DOT64P restatement, the SWIGLU
epilogue against the numpy restatement of contract SWIGLU16 (tests/ternary_group_ref.py), bit for
bit; TernaryGatedMLP and fuse_gated_mlp on top of them."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ternary_decode_ref as ref
import ternary_group_ref as gref
from test_gpu_parity import cuda, host
from test_gpu_ternary_decode import TDT

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-3, 2e-3  # tests/test_gpu_ternary.py
E_ARG, E_UNSUPPORTED = 1, 3
# (m, bs, tokens, dtype) of ref.SHAPES[0], [1], [3], [4]: idle lanes, 16-position tables and the
# block clamp; a ragged m; per-channel; a third piece on lanes 0 and 1
SHAPES = [(100, 16, 2, "fp16"), (1030, 64, 8, "bf16"), (520, 520, 5, "bf16"), (8320, 128, 8, "fp16")]
assert [(s[1],) + s[2:] for s in (ref.SHAPES[0], ref.SHAPES[1], ref.SHAPES[3], ref.SHAPES[4])] == SHAPES
ROWS = (33, 40, 7, 130)  # unequal member rows: ragged against the 8 rows of a workgroup
_MEMBERS = {}


class Member:
    """A ref.make_case layer of its own seed (so its T and perm differ from its neighbours') on the
    x every case of (m, tokens) shares, with its device buffers and its DOT64P fold."""

    def __init__(self, pt2q, n, m, bs, tokens, dtype, seed):
        self.c = c = ref.make_case(n, m, bs, tokens, dtype, seed=seed)
        self.n, self.bs, self.dtype = n, bs, dtype
        lay = pt2q.TernaryLinear(m, n, bs, bias=True, dtype=TDT[dtype], decode="fused")
        lay.set_quantized_params(cuda(c["alpha"]), cuda(c["mu"]), cuda(c["T"]), cuda(c["perm"]), cuda(c["bias"]))
        lay._prepare()
        self.layer = lay
        self.pack = lay._packed
        self.x = cuda(c["x"]).to(TDT[dtype])
        assert np.array_equal(host(self.x.float()), c["x"]) and np.array_equal(host(self.pack[4]), c["bias"])
        self._fold = None

    def tup(self, bias=True):
        return self.pack if bias else self.pack[:4] + (None,)

    def fold(self):
        if self._fold is None:
            c = self.c
            self._fold = ref.fold(c["x"], c["alpha"], c["mu"], c["T"], c["perm"], c["bs"], c["dtype"])
            self._fold.setflags(write=False)
        return self._fold

    def want(self, bias=True, out_dtype=None):
        return ref.finish(self.fold(), self.c["bias"] if bias else None, self.dtype, out_dtype)

    def alone(self, pt2q, x=None, bias=True, out_dtype=None):
        p = self.pack
        return pt2q.ternary_decode(self.x if x is None else x, p[0], p[1], p[2], p[3], self.bs,
                                   p[4] if bias else None, out_dtype=out_dtype)


def member(pt2q, n, m, bs, tokens, dtype, seed):
    key = (n, m, bs, tokens, dtype, seed)
    if key not in _MEMBERS:
        _MEMBERS[key] = Member(pt2q, n, m, bs, tokens, dtype, seed)
    return _MEMBERS[key]


def group(pt2q, m, bs, tokens, dtype, count=4):
    ms = [member(pt2q, ROWS[z], m, bs, tokens, dtype, 1000 + z) for z in range(count)]
    assert all(np.array_equal(a.c["x"], ms[0].c["x"]) for a in ms)
    assert count < 2 or not np.array_equal(ms[0].c["perm"], ms[1].c["perm"])
    return ms


def pair(pt2q, n, m, bs, tokens, dtype):
    """Gate and up of one width on one x, different seeds."""
    return member(pt2q, n, m, bs, tokens, dtype, 2000), member(pt2q, n, m, bs, tokens, dtype, 2001)


def want_swiglu(gm, um, bias=True):
    return gref.swiglu(gm.want(bias), um.want(bias), gm.dtype)


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("m,bs,tokens,dtype", SHAPES)
def test_plain_group_is_the_members_alone(pt2q, m, bs, tokens, dtype, count):
    ms = group(pt2q, m, bs, tokens, dtype, count)
    x = ms[0].x
    for f32out in (False, True):
        odt = torch.float32 if f32out else None
        # every member with bias, none with bias, and member 1 (member 0 of a single) without
        for nobias in (set(), set(range(count)), {min(1, count - 1)}):
            ys = pt2q.ternary_decode_group(x, [a.tup(z not in nobias) for z, a in enumerate(ms)], out_dtype=odt,
                                           block_size=bs)
            assert len(ys) == count
            for z, (a, y) in enumerate(zip(ms, ys)):
                assert y.dtype == (torch.float32 if f32out else TDT[dtype]) and tuple(y.shape) == (tokens, a.n)
                assert torch.equal(y, a.alone(pt2q, bias=z not in nobias, out_dtype=odt)), (z, nobias, f32out)
                assert np.array_equal(host(y.float()), a.want(z not in nobias, "fp32" if f32out else None))
    # modules as members, packed on demand
    ys = pt2q.ternary_decode_group(x, [a.layer for a in ms])
    assert all(torch.equal(y, a.alone(pt2q)) for a, y in zip(ms, ys))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n,m,bs,tokens,dtype", [ref.SHAPES[i] for i in (0, 1, 3, 4)])
def test_swiglu_bit_exact_vs_restatement(pt2q, n, m, bs, tokens, dtype, bias):
    gm, um = pair(pt2q, n, m, bs, tokens, dtype)
    h = pt2q.ternary_decode_swiglu(gm.x, gm.tup(bias), um.tup(bias), block_size=bs)
    assert h.dtype == TDT[dtype] and tuple(h.shape) == (tokens, n)
    assert np.array_equal(host(h.float()), want_swiglu(gm, um, bias))
    # and from the device's own separate outputs
    g, u = gm.alone(pt2q, bias=bias), um.alone(pt2q, bias=bias)
    assert np.array_equal(host(h.float()), gref.swiglu(host(g.float()), host(u.float()), dtype))
    if bias:
        assert torch.equal(h, pt2q.ternary_decode_swiglu(gm.x, gm.layer, um.layer))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_activation_over_every_16bit_gate_value(pt2q, dtype):
    """m = 64, one token, all-zero codes and mu = 0, so v = +0 and g is the gate bias: one row per
    finite 16-bit value.  With the up bias 1.0, h = s; with random 16-bit up biases the product
    and its rounding.  A flushed subnormal, a fused multiply-add or an approximate division
    anywhere in the chain shows here."""
    gb = gref.finite16(dtype)
    n, m = gb.size, 64
    rng = np.random.default_rng(64)
    ub = gref.finite16(dtype)[rng.integers(0, n, size=n)]
    zero = torch.zeros((n, 1), dtype=torch.float32, device="cuda")
    lay = pt2q.TernaryLinear(m, n, m, bias=True, dtype=TDT[dtype], decode="fused")
    lay._prepare()  # T = 0, identity perm
    codes, gather = lay._packed[:2]
    x = cuda(ref.round16(rng.standard_normal((1, m)), dtype)).to(TDT[dtype])
    v = np.zeros((1, n), np.float32)
    g = ref.finish(v, gb, dtype)
    assert np.array_equal(g[0], gb)
    for upbias in (np.ones(n, np.float32), ub):
        gate, up = (codes, gather, zero, zero, cuda(gb)), (codes, gather, zero, zero, cuda(upbias))
        h = host(pt2q.ternary_decode_swiglu(x, gate, up, block_size=m).float())
        want = gref.swiglu(g, ref.finish(v, upbias, dtype), dtype)
        bad = np.flatnonzero((h != want)[0] & ~(np.isnan(h) & np.isnan(want))[0])
        assert bad.size == 0, (gb[bad][:8], upbias[bad][:8], h[0][bad][:8], want[0][bad][:8])
        assert np.array_equal(np.signbit(h), np.signbit(want))


@pytest.mark.parametrize("m,bs,dtype", [(1030, 64, "bf16"), (8320, 128, "fp16")])
def test_token_invariance(pt2q, m, bs, dtype):
    """Row t of a T-token call equals the 1-token call on that row, whatever T (and so whatever
    token grouping the launcher picks), for the plain group and for SwiGLU."""
    ms = group(pt2q, m, bs, 8, dtype, 3)
    gm, um = pair(pt2q, 40, m, bs, 8, dtype)
    x = ms[0].x
    assert torch.equal(x, gm.x)
    plain = lambda xv: pt2q.ternary_decode_group(xv, [a.tup() for a in ms], block_size=bs)  # noqa: E731
    swi = lambda xv: pt2q.ternary_decode_swiglu(xv, gm.tup(), um.tup(), block_size=bs)  # noqa: E731
    p1 = [torch.cat(ys) for ys in zip(*[plain(x[t:t + 1]) for t in range(8)])]
    s1 = torch.cat([swi(x[t:t + 1]) for t in range(8)])
    assert np.array_equal(host(s1.float()), want_swiglu(gm, um))
    for T in (1, 2, 3, 5, 8):
        for xv, sl in ((x[:T], slice(0, T)), (x[8 - T:], slice(8 - T, 8))):
            assert all(torch.equal(y, w[sl]) for y, w in zip(plain(xv), p1)), T
            assert torch.equal(swi(xv), s1[sl]), T


@pytest.mark.parametrize("m,bs,tokens,dtype", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_strides_and_alignment(pt2q, m, bs, tokens, dtype):
    """x a column slice (ldx > m, base 2 bytes off 16-byte alignment), outputs with ldy > n whose
    padding keeps its sentinel, one member's gather 4 bytes off 16-byte alignment."""
    ms = group(pt2q, m, bs, tokens, dtype, 3)
    gm, um = pair(pt2q, 40, m, bs, tokens, dtype)
    dev = ms[0].x.device
    buf = torch.zeros((tokens, m + 11), dtype=TDT[dtype], device=dev)
    buf[:, 1:1 + m] = ms[0].x
    xv = buf[:, 1:1 + m]
    assert xv.data_ptr() % 16 == 2 and xv.stride(0) > m

    def off4(t):  # the same gather, 4 bytes off
        gbuf = torch.empty(t.numel() + 1, dtype=torch.int32, device=dev)
        gbuf[1:] = t
        assert gbuf[1:].data_ptr() % 16 == 4
        return gbuf[1:]
    tups = [a.tup() for a in ms]
    tups[1] = (tups[1][0], off4(tups[1][1])) + tups[1][2:]
    for odt in (TDT[dtype], torch.float32):
        ybufs = [torch.full((tokens, a.n + 5), -77.0, dtype=odt, device=dev) for a in ms]
        pt2q.ternary_decode_group(xv, tups, out_dtype=odt, outs=[b[:, :a.n] for a, b in zip(ms, ybufs)], block_size=bs)
        for a, b in zip(ms, ybufs):
            assert np.array_equal(host(b[:, :a.n].float()), a.want(out_dtype="fp32" if odt == torch.float32 else None))
            assert bool((b[:, a.n:] == -77.0).all())
    hbuf = torch.full((tokens, 40 + 5), -77.0, dtype=TDT[dtype], device=dev)
    up = um.tup()
    pt2q.ternary_decode_swiglu(xv, gm.tup(), (up[0], off4(up[1])) + up[2:], out=hbuf[:, :40], block_size=bs)
    assert np.array_equal(host(hbuf[:, :40].float()), want_swiglu(gm, um))
    assert bool((hbuf[:, 40:] == -77.0).all())


def test_wide_plain_group(pt2q):
    """m = 28672 (seven rounds of pieces): one token's activations need more than 64 KiB of LDS."""
    ms = [member(pt2q, 24, 28672, 128, 1, "fp16", 3000 + z) for z in range(2)]
    ys = pt2q.ternary_decode_group(ms[0].x, [a.tup() for a in ms], block_size=128)
    for a, y in zip(ms, ys):
        assert np.array_equal(host(y.float()), a.want())


def _raw_swiglu(pt2q, x, gm, um, out, bs):
    """The C entry itself, SWIGLU, returning its status."""
    L = pt2q._lib
    tokens, m = x.shape
    arr = lambda ts: L.ptr_array(ts)  # noqa: E731
    ia = lambda vs: (ctypes.c_int * len(vs))(*vs)  # noqa: E731
    ns, Bs, ldy = ia([gm.n, um.n]), ia([gm.pack[2].shape[1], um.pack[2].shape[1]]), (ctypes.c_int64 * 1)(out.stride(0))
    keep = [arr([gm.pack[i], um.pack[i]]) for i in range(5)] + [arr([out])]
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    rc = L.lib().pt2q_ternary_decode_group(L.ptr(x), L.dtype_code(x), tokens, x.stride(0), m, 2, vp(ns), keep[0][0],
                                           keep[1][0], keep[2][0], keep[3][0], vp(Bs), bs, keep[4][0], keep[5][0],
                                           L.dtype_code(out), vp(ldy), L.DECODE_SWIGLU, L.stream_of(x.device))
    torch.cuda.synchronize()
    return rc


def test_swiglu_widest_layer_and_the_first_refused(pt2q):
    """Two gathered copies and the staged row: m = 20480 is the widest a token fits 128 KiB with
    (5 rounds: 80 KiB + 40 KiB); m = 20481 takes a sixth round and is refused, nothing written."""
    gm, um = pair(pt2q, 24, 20480, 128, 1, "bf16")
    h = pt2q.ternary_decode_swiglu(gm.x, gm.tup(), um.tup(), block_size=128)
    assert np.array_equal(host(h.float()), want_swiglu(gm, um))
    m = 20481
    lays = []
    for _ in range(2):
        lay = pt2q.TernaryLinear(m, 24, 128, bias=True, dtype=torch.bfloat16, decode="fused")
        lay._prepare()
        lays.append(lay)
    x = torch.ones((1, m), dtype=torch.bfloat16, device="cuda")
    out = torch.full((1, 24), -77.0, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(pt2q._lib.Pt2qError, match="status 3"):
        pt2q.ternary_decode_swiglu(x, lays[0], lays[1], out=out)
    torch.cuda.synchronize()
    assert bool((out == -77.0).all())
    # the plain group takes the same layers
    ys = pt2q.ternary_decode_group(x, lays)
    assert all(bool((y == 0).all()) for y in ys)  # T = 0, mu = 0, bias = 0


def test_argument_errors_launch_nothing(pt2q):
    L = pt2q._lib
    m, bs, tokens, dtype = SHAPES[1]
    ms = group(pt2q, m, bs, tokens, dtype, 4) + [member(pt2q, 33, m, bs, tokens, dtype, 1004)]
    x = ms[0].x
    B = ms[0].pack[2].shape[1]

    def call(count=2, epilogue=L.DECODE_PLAIN, rows=None, ydtype=None, ntok=tokens, mm=m, Bv=B, idx=(0, 1, 2, 3, 4),
             null=None, ldx=None):
        sel = [ms[i] for i in idx]
        nmem = len(sel)
        rows = [a.n for a in sel] if rows is None else rows
        ydt = TDT[dtype] if ydtype is None else ydtype
        outs = [torch.full((8, 140), -77.0, dtype=ydt, device=x.device) for _ in sel]
        keep = [L.ptr_array([None if null == (f, z) else a.pack[f] for z, a in enumerate(sel)]) for f in range(5)]
        keep.append(L.ptr_array(outs))
        ns, Bs = (ctypes.c_int * nmem)(*rows), (ctypes.c_int * nmem)(*([Bv] * nmem))
        ldy = (ctypes.c_int64 * nmem)(*([140] * nmem))
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
        rc = L.lib().pt2q_ternary_decode_group(L.ptr(x), L.dtype_code(x), ntok, mm if ldx is None else ldx, mm, count,
                                               vp(ns), keep[0][0], keep[1][0], keep[2][0], keep[3][0], vp(Bs), bs,
                                               keep[4][0], keep[5][0], L._DT[ydt], vp(ldy), epilogue,
                                               L.stream_of(x.device))
        torch.cuda.synchronize()
        assert all(bool((o == -77.0).all()) for o in outs) or rc == 0
        return rc

    assert call(count=2) == 0 and call(count=4) == 0  # the harness itself is a valid call
    assert call(count=2, epilogue=L.DECODE_SWIGLU, idx=(0, 4)) == 0
    assert call(count=0) == E_ARG and call(count=5) == E_ARG and call(count=-1) == E_ARG
    assert call(count=1, epilogue=L.DECODE_SWIGLU, idx=(0, 4)) == E_ARG
    assert call(count=3, epilogue=L.DECODE_SWIGLU, idx=(0, 4, 0)) == E_ARG
    assert call(count=2, epilogue=L.DECODE_SWIGLU, idx=(0, 1)) == E_ARG  # n[0] != n[1]
    assert call(count=2, epilogue=L.DECODE_SWIGLU, idx=(0, 4), ydtype=torch.float32) == E_ARG
    assert call(count=2, epilogue=2) == E_ARG
    # per member, the rules of pt2q_ternary_decode
    assert call(count=2, rows=[33, 0]) == E_ARG
    assert call(count=2, null=(0, 1)) == E_ARG and call(count=3, null=(1, 2)) == E_ARG  # codes, gather
    assert call(count=2, Bv=B - 1) == E_ARG
    assert call(count=2, ldx=m - 1) == E_ARG
    assert call(count=2, ydtype=torch.bfloat16 if dtype == "fp16" else torch.float16) == E_ARG
    assert call(count=2, null=(4, 1)) == 0  # a null bias entry is no error
    assert call(count=2, ntok=9) == E_UNSUPPORTED
    assert call(count=2, mm=32769, Bv=-(-32769 // bs)) == E_UNSUPPORTED
    # through Python: the same refusals as exceptions
    with pytest.raises(L.Pt2qError):
        pt2q.ternary_decode_group(x, [a.layer for a in ms])  # five members
    with pytest.raises(L.Pt2qError):
        pt2q.ternary_decode_swiglu(x, ms[0].layer, ms[1].layer)  # unequal rows
    with pytest.raises(L.Pt2qError):
        pt2q.ternary_decode_group(x.cpu(), [ms[0].layer])


# ---- TernaryGatedMLP / fuse_gated_mlp ----

HID, INTER, MBS = 256, 384, 128


@pytest.fixture
def mlp_cap8(pt2q, monkeypatch):
    """The fused MLP path for every token count the library takes (the shipped
    mlp_decode_max_tokens is the measured crossover, which may be lower)."""
    monkeypatch.setattr(pt2q.ternary, "mlp_decode_max_tokens", pt2q._lib.lib().pt2q_ternary_decode_max_tokens())


def _mlp(pt2q, dtype="fp16"):
    gm, um = pair(pt2q, INTER, HID, MBS, 8, dtype)
    dm = member(pt2q, HID, INTER, MBS, 8, dtype, 2002)
    return pt2q.TernaryGatedMLP(gm.layer, um.layer, dm.layer), gm, um, dm


def _unfused(mlp, x):
    return mlp.down_proj(F.silu(mlp.gate_proj(x)) * mlp.up_proj(x))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_gated_mlp_fused_forward(pt2q, mlp_cap8, dtype):
    mlp, gm, um, dm = _mlp(pt2q, dtype)
    assert [k for k, _ in mlp.named_children()] == ["gate_proj", "up_proj", "down_proj"]
    x1 = gm.x[:1]
    y = mlp(x1)
    h = pt2q.ternary_decode_swiglu(x1, gm.layer, um.layer)
    assert np.array_equal(host(h.float()), want_swiglu(gm, um)[:1])
    assert torch.equal(y, pt2q.ternary_decode(h, *dm.pack[:4], MBS, dm.pack[4]))
    # against the unfused composition: the two differ only where SWIGLU16's s and torch's SiLU
    # round differently
    np.testing.assert_allclose(host(y.float()), host(_unfused(mlp, x1).float()), rtol=RTOL, atol=ATOL)
    # a leading batch dimension flattens into tokens
    y4 = mlp(gm.x[:4].reshape(2, 2, HID))
    assert tuple(y4.shape) == (2, 2, HID) and torch.equal(y4[0, :1], y)
    h4 = pt2q.ternary_decode_swiglu(gm.x[:4], gm.layer, um.layer)
    assert torch.equal(y4.reshape(4, HID), pt2q.ternary_decode(h4, *dm.pack[:4], MBS, dm.pack[4]))


def test_gated_mlp_above_the_crossover_and_in_mfma_mode(pt2q):
    """As shipped: more tokens than mlp_decode_max_tokens, and any call once a child is switched to
    decode="mfma", are exactly the children's own calls."""
    mlp, gm, um, dm = _mlp(pt2q)
    k = pt2q.ternary.mlp_decode_max_tokens
    assert 0 <= k <= pt2q._lib.lib().pt2q_ternary_decode_max_tokens()
    x = gm.x[:k + 1]
    assert torch.equal(mlp(x), _unfused(mlp, x))
    if k >= 1:
        h = pt2q.ternary_decode_swiglu(x[:k], gm.layer, um.layer)
        assert torch.equal(mlp(x[:k]), pt2q.ternary_decode(h, *dm.pack[:4], MBS, dm.pack[4]))
    try:
        assert pt2q.set_decode(mlp, "mfma") is mlp and mlp.gate_proj.decode == "mfma"
        assert torch.equal(mlp(x[:1]), _unfused(mlp, x[:1]))
    finally:
        pt2q.set_decode(mlp, "fused")
    with pytest.raises(pt2q._lib.Pt2qError):
        pt2q.TernaryGatedMLP(gm.layer, dm.layer, dm.layer)


def test_gated_mlp_graph_capture_replays_eager_bits(pt2q, mlp_cap8):
    """The 1-token fused forward (two launches on one stream, a plain chain) captured into a graph."""
    mlp, gm, um, dm = _mlp(pt2q)
    x1 = gm.x[:1].clone()
    eager = mlp(x1).clone()  # eager warm-up: loads the kernels before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = mlp(x1)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


def _ternary_llama(pt2q, hidden_act="silu"):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=384, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=4, max_position_embeddings=256,
                                   hidden_act=hidden_act)  # tests/test_gpu_calibration.py
    torch.manual_seed(0)
    model = transformers.LlamaForCausalLM(cfg).cuda().eval()
    g = torch.Generator().manual_seed(5)
    params = {}
    for name, mod in model.named_modules():
        if isinstance(mod, torch.nn.Linear) and ".layers." in name:
            n, m = mod.out_features, mod.in_features
            B = -(-m // 128)
            params[name] = {"alpha": (torch.rand((n, B), generator=g) * 0.05 + 0.005).half(),
                            "mu": (torch.randn((n, B), generator=g) * 0.002).half(),
                            "T": torch.randint(-1, 2, (n, m), generator=g, dtype=torch.int8),
                            "perm": torch.randperm(m, generator=g)}
    pt2q.replace_linear_with_ternary(model, params, block_size=128, decode="fused")
    return model, params


def test_fuse_gated_mlp_on_a_llama(pt2q, mlp_cap8, tmp_path):
    model, params = _ternary_llama(pt2q)
    keys = list(model.state_dict().keys())
    attn_types = [type(l.self_attn) for l in model.model.layers]
    mlp0 = model.model.layers[0].mlp
    x = torch.randn((1, 256), generator=torch.Generator().manual_seed(6)).cuda().half()
    y_before = mlp0(x)
    assert pt2q.fuse_gated_mlp(model) is model
    for lay, at in zip(model.model.layers, attn_types):
        assert isinstance(lay.mlp, pt2q.TernaryGatedMLP) and type(lay.self_attn) is at
        assert all(isinstance(getattr(lay.self_attn, k), pt2q.TernaryLinear) for k in ("q_proj", "k_proj", "v_proj", "o_proj"))
    assert model.model.layers[0].mlp.gate_proj is mlp0.gate_proj
    assert list(model.state_dict().keys()) == keys
    y = model.model.layers[0].mlp(x)
    np.testing.assert_allclose(host(y.float()), host(y_before.float()), rtol=RTOL, atol=ATOL)
    assert pt2q.fuse_gated_mlp(model) is model  # idempotent
    # save / load round trip on the fused model
    path = str(tmp_path / "fused.pt")
    pt2q.save_quantized_model(model, path, {k: {kk: vv.cpu() for kk, vv in v.items()} for k, v in params.items()})
    fresh, _ = _ternary_llama(pt2q)
    for mod in fresh.modules():
        if isinstance(mod, pt2q.TernaryLinear):
            mod.T.zero_()
    pt2q.fuse_gated_mlp(fresh)
    fresh, qp = pt2q.load_quantized_model(fresh, path)
    assert set(qp) == set(params)
    assert torch.equal(fresh.model.layers[0].mlp(x), y)
    # set_decode reaches the children of the fused module
    pt2q.set_decode(model, "mfma")
    assert all(l.mlp.up_proj.decode == "mfma" for l in model.model.layers)


def test_fuse_gated_mlp_leaves_a_gelu_mlp(pt2q):
    model, _ = _ternary_llama(pt2q, hidden_act="gelu")
    types = [type(l.mlp) for l in model.model.layers]
    pt2q.fuse_gated_mlp(model)
    assert [type(l.mlp) for l in model.model.layers] == types
    assert not any(isinstance(m, pt2q.TernaryGatedMLP) for m in model.modules())
