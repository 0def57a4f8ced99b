"""The RMSNorm prologue and the residual epilogue of the decode kernel (pt2q_ternary_decode_fused)
and the stand-alone pt2q_rmsnorm (csrc/ternary_decode.hip): bit for bit against the numpy
restatement of contracts RMSNORM16 and RESADD16 (tests/ternary_norm_ref.py) composed with DOT64P
and SWIGLU16, and against the unfused calls on the device; TernaryMLPBlock on top of them."""
import ctypes

import numpy as np
import pytest
import torch

import ternary_decode_ref as ref
import ternary_group_ref as gref
import ternary_norm_ref as nref
import test_gpu_ternary_group as G
from test_gpu_parity import cuda, host
from test_gpu_ternary_decode import TDT

pytestmark = pytest.mark.gpu

E_ARG = 1
EPS = 1e-5
SHAPES = G.SHAPES  # (m, bs, tokens, dtype) of ref.SHAPES[0], [1], [3], [4]
PAIR_ROWS = {s[1]: s[0] for s in ref.SHAPES[:5]}  # the rows ref.SHAPES gives each m
_NORMED, _WANT = {}, {}


def normed(a):
    """(weight on the device, RMSNORM16 of the member's x by the restatement), per (m, tokens, dtype)."""
    c = a.c
    key = (c["m"], c["tokens"], c["dtype"])
    if key not in _NORMED:
        w = nref.make_inputs(1, c["m"], c["dtype"], seed=c["m"])[1]
        xn = nref.rmsnorm(c["x"], w, EPS, c["dtype"])
        xn.setflags(write=False)
        _NORMED[key] = (cuda(w).to(TDT[c["dtype"]]), xn)
    return _NORMED[key]


def want_norm(a, bias=True):
    """DOT64P on the restated norm of the member's x."""
    if id(a) not in _WANT:
        c = a.c
        v = ref.fold(normed(a)[1], c["alpha"], c["mu"], c["T"], c["perm"], c["bs"], c["dtype"])
        v.setflags(write=False)
        _WANT[id(a)] = (a, v)  # keeps `a` alive, so the id stays its own
    return ref.finish(_WANT[id(a)][1], a.c["bias"] if bias else None, a.dtype)


def one(pt2q, a, x, bias=True, **kw):
    p = a.tup(bias)
    return pt2q.ternary_decode(x, p[0], p[1], p[2], p[3], a.bs, p[4], **kw)


def residual_for(a, tokens, seed):
    r = ref.round16(np.random.default_rng(seed).standard_normal((tokens, a.n)) * 0.5, a.dtype)
    return r, cuda(r).to(TDT[a.dtype])


# ---- pt2q_rmsnorm ----

@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("tokens,m", [(2, 100), (8, 1030), (5, 520), (8, 8320), (19, 1030)])
def test_rms_norm_bit_exact(pt2q, tokens, m, dtype):
    x, w = nref.make_inputs(tokens, m, dtype, seed=tokens * m)
    want = nref.rmsnorm(x, w, EPS, dtype)
    xd, wd = cuda(x).to(TDT[dtype]), cuda(w).to(TDT[dtype])
    y = pt2q.rms_norm(xd, wd, EPS)
    assert y.dtype == TDT[dtype] and np.array_equal(host(y.float()), want)
    # a padded row stride and a base one element off, in and out; the padding keeps its sentinel
    xb = torch.zeros((tokens, m + 9), dtype=TDT[dtype], device=xd.device)
    xb[:, 1:1 + m] = xd
    yb = torch.full((tokens, m + 5), -77.0, dtype=TDT[dtype], device=xd.device)
    assert xb[:, 1:1 + m].data_ptr() % 4 == 2
    assert pt2q.rms_norm(xb[:, 1:1 + m], wd, EPS, out=yb[:, 1:1 + m]).data_ptr() == yb[:, 1:1 + m].data_ptr()
    assert np.array_equal(host(yb[:, 1:1 + m].float()), want)
    assert bool((yb[:, :1] == -77.0).all()) and bool((yb[:, 1 + m:] == -77.0).all())
    # out= aliasing x
    xv = xb[:, 1:1 + m]
    pt2q.rms_norm(xv, wd, EPS, out=xv)
    assert np.array_equal(host(xv.float()), want) and bool((xb[:, 1 + m:] == 0).all())
    # more dimensions, contiguous
    if tokens == 8:
        assert torch.equal(pt2q.rms_norm(xd.reshape(2, 4, m), wd, EPS), y.reshape(2, 4, m))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_rms_norm_square_root_and_division(pt2q, dtype):
    """4096 rows of 64 elements whose scales run over 2^-12 .. 2^12: thousands of distinct
    v = mean + eps, so an approximate square root or reciprocal shows."""
    rows, m = 4096, 64
    rng = np.random.default_rng(4096)
    sc = 2.0 ** (-12.0 + 24.0 * np.arange(rows) / (rows - 1))
    x = ref.round16(rng.standard_normal((rows, m)) * sc[:, None], dtype)
    w = ref.round16(1.0 + rng.uniform(-0.5, 0.5, size=m), dtype)
    xd, wd = cuda(x).to(TDT[dtype]), cuda(w).to(TDT[dtype])
    for eps in (0.0, 1e-6, 1e-5):
        assert np.unique(nref.scale(x, eps)).size > 3000
        assert np.array_equal(host(pt2q.rms_norm(xd, wd, eps).float()), nref.rmsnorm(x, w, eps, dtype)), eps


# ---- the prologue and the epilogue ----

@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("m,bs,tokens,dtype", SHAPES)
def test_norm_prologue(pt2q, m, bs, tokens, dtype, bias):
    ms = G.group(pt2q, m, bs, tokens, dtype, 4)
    gm, um = G.pair(pt2q, PAIR_ROWS[m], m, bs, tokens, dtype)
    x = ms[0].x
    assert torch.equal(x, gm.x)
    w, xn = normed(ms[0])
    norm = (w, EPS)
    xnd = pt2q.rms_norm(x, w, EPS)
    assert np.array_equal(host(xnd.float()), xn)
    # the single linear, 16-bit and fp32 output
    y = one(pt2q, ms[0], x, bias, norm=norm)
    assert torch.equal(y, one(pt2q, ms[0], xnd, bias)) and np.array_equal(host(y.float()), want_norm(ms[0], bias))
    assert torch.equal(one(pt2q, ms[0], x, bias, norm=norm, out_dtype=torch.float32),
                       one(pt2q, ms[0], xnd, bias, out_dtype=torch.float32))
    # PLAIN groups of unequal rows
    for count in (1, 2, 3, 4):
        ys = pt2q.ternary_decode_group(x, [a.tup(bias) for a in ms[:count]], block_size=bs, norm=norm)
        for a, y in zip(ms, ys):
            assert torch.equal(y, one(pt2q, a, xnd, bias)), count
            assert np.array_equal(host(y.float()), want_norm(a, bias)), count
    # SWIGLU
    h = pt2q.ternary_decode_swiglu(x, gm.tup(bias), um.tup(bias), block_size=bs, norm=norm)
    assert torch.equal(h, pt2q.ternary_decode_swiglu(xnd, gm.tup(bias), um.tup(bias), block_size=bs))
    assert np.array_equal(host(h.float()), gref.swiglu(want_norm(gm, bias), want_norm(um, bias), dtype))
    if bias:  # modules as members
        assert torch.equal(h, pt2q.ternary_decode_swiglu(x, gm.layer, um.layer, norm=norm))
    assert torch.equal(x, ms[0].x) and np.array_equal(host(x.float()), ms[0].c["x"])  # x itself is not written


@pytest.mark.parametrize("m,bs,tokens,dtype", SHAPES)
def test_residual_epilogue(pt2q, m, bs, tokens, dtype):
    ms = G.group(pt2q, m, bs, tokens, dtype, 3)
    x = ms[0].x
    res = [residual_for(a, tokens, 50 + z) for z, a in enumerate(ms)]
    # the single linear
    a, (rn, rd) = ms[0], res[0]
    y = one(pt2q, a, x, residual=rd)
    assert torch.equal(y, rd + a.alone(pt2q)) and np.array_equal(host(y.float()), nref.resadd(a.want(), rn, dtype))
    out = rd.clone()
    assert one(pt2q, a, x, out=out, residual=out) is out and torch.equal(out, y)  # in place
    assert torch.equal(one(pt2q, a, x, bias=False, residual=rd), rd + a.alone(pt2q, bias=False))
    # the group: member 1 without a residual, member 2's in a padded buffer (ldr > n)
    pad = torch.full((tokens, ms[2].n + 7), -77.0, dtype=TDT[dtype], device=x.device)
    pad[:, 3:3 + ms[2].n] = res[2][1]
    rs = [res[0][1], None, pad[:, 3:3 + ms[2].n]]
    ys = pt2q.ternary_decode_group(x, [b.tup() for b in ms], block_size=bs, residuals=rs)
    for z, (b, y) in enumerate(zip(ms, ys)):
        alone = b.alone(pt2q)
        assert torch.equal(y, alone if rs[z] is None else rs[z] + alone), z
        assert np.array_equal(host(y.float()), b.want() if rs[z] is None else nref.resadd(b.want(), res[z][0], dtype)), z
    # in place: hidden += ..., one member's output still in its padded buffer
    outs = [res[0][1].clone(), res[1][1].clone(), pad[:, 3:3 + ms[2].n]]
    back = pt2q.ternary_decode_group(x, [b.tup() for b in ms], block_size=bs, outs=outs, residuals=outs)
    assert all(o is b for o, b in zip(outs, back))
    assert torch.equal(outs[0], ys[0]) and torch.equal(outs[1], res[1][1] + ms[1].alone(pt2q)) and torch.equal(outs[2], ys[2])
    assert bool((pad[:, :3] == -77.0).all()) and bool((pad[:, 3 + ms[2].n:] == -77.0).all())


@pytest.mark.parametrize("m,bs,tokens,dtype", [SHAPES[0], SHAPES[3]])
def test_norm_and_residual_together(pt2q, m, bs, tokens, dtype):
    ms = G.group(pt2q, m, bs, tokens, dtype, 3)
    x = ms[0].x
    w = normed(ms[0])[0]
    res = [residual_for(a, tokens, 70 + z) for z, a in enumerate(ms)]
    xnd = pt2q.rms_norm(x, w, EPS)
    y = one(pt2q, ms[0], x, norm=(w, EPS), residual=res[0][1])
    assert torch.equal(y, res[0][1] + one(pt2q, ms[0], xnd))
    assert np.array_equal(host(y.float()), nref.resadd(want_norm(ms[0]), res[0][0], dtype))
    ys = pt2q.ternary_decode_group(x, [a.tup() for a in ms], block_size=bs, norm=(w, EPS),
                                   residuals=[r[1] for r in res])
    for a, y, (rn, rd) in zip(ms, ys, res):
        assert torch.equal(y, rd + one(pt2q, a, xnd))
        assert np.array_equal(host(y.float()), nref.resadd(want_norm(a), rn, dtype))


@pytest.mark.parametrize("m,bs,dtype", [(1030, 64, "bf16"), (8320, 128, "fp16")])
def test_token_invariance(pt2q, m, bs, dtype):
    """Token t of a T-token call has the bits of the 1-token call on row t alone, norm and residual
    both on: the sums of a row's squares do not depend on its neighbours or on the token grouping."""
    ms = G.group(pt2q, m, bs, 8, dtype, 3)
    gm, um = G.pair(pt2q, 40, m, bs, 8, dtype)
    x = ms[0].x
    w = normed(ms[0])[0]
    res = [residual_for(a, 8, 90 + z)[1] for z, a in enumerate(ms)]
    plain = lambda sl: pt2q.ternary_decode_group(x[sl], [a.tup() for a in ms], block_size=bs, norm=(w, EPS),  # noqa: E731
                                                 residuals=[r[sl] for r in res])
    single = lambda sl: one(pt2q, ms[0], x[sl], norm=(w, EPS), residual=res[0][sl])  # noqa: E731
    swi = lambda sl: pt2q.ternary_decode_swiglu(x[sl], gm.tup(), um.tup(), block_size=bs, norm=(w, EPS))  # noqa: E731
    rows = [slice(t, t + 1) for t in range(8)]
    p1 = [torch.cat(ys) for ys in zip(*[plain(sl) for sl in rows])]
    s1 = torch.cat([swi(sl) for sl in rows])
    assert np.array_equal(host(s1.float()), gref.swiglu(want_norm(gm), want_norm(um), dtype))
    assert torch.equal(p1[0], torch.cat([single(sl) for sl in rows]))
    for T in (2, 3, 5, 8):
        for sl in (slice(0, T), slice(8 - T, 8)):
            assert all(torch.equal(y, v[sl]) for y, v in zip(plain(sl), p1)), T
            assert torch.equal(single(sl), p1[0][sl]) and torch.equal(swi(sl), s1[sl]), T


def test_widest_layers_with_the_norm(pt2q):
    """The prologue adds no LDS: the widest layers the kernel takes still launch with it (PLAIN
    m = 32768: 128 KiB for one token; SWIGLU m = 20480), and m = 4096 with four tokens still has
    its four tokens in one workgroup's 64 KiB (TG = 4)."""
    a = G.member(pt2q, 16, 32768, 128, 1, "fp16", 3100)
    w = normed(a)[0]
    assert np.array_equal(host(one(pt2q, a, a.x, norm=(w, EPS)).float()), want_norm(a))
    gm, um = (G.member(pt2q, 16, 20480, 128, 1, "bf16", 3101 + z) for z in range(2))
    w = normed(gm)[0]
    h = pt2q.ternary_decode_swiglu(gm.x, gm.tup(), um.tup(), block_size=128, norm=(w, EPS))
    assert np.array_equal(host(h.float()), gref.swiglu(want_norm(gm), want_norm(um), "bf16"))
    b = G.member(pt2q, 16, 4096, 128, 4, "bf16", 3103)
    w = normed(b)[0]
    res = residual_for(b, 4, 3104)
    y = one(pt2q, b, b.x, norm=(w, EPS), residual=res[1])
    assert np.array_equal(host(y.float()), nref.resadd(want_norm(b), res[0], "bf16"))


def test_argument_errors_launch_nothing(pt2q):
    L = pt2q._lib
    m, bs, tokens, dtype = SHAPES[1]
    ms = G.group(pt2q, m, bs, tokens, dtype, 2) + [G.member(pt2q, 33, m, bs, tokens, dtype, 1004)]
    x = ms[0].x
    w = normed(ms[0])[0]
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def call(idx=(0, 1), epilogue=L.DECODE_PLAIN, ydtype=None, weight=None, eps=EPS, res=(True, True), ldr=140):
        sel = [ms[i] for i in idx]
        ydt = TDT[dtype] if ydtype is None else ydtype
        outs = [torch.full((8, 140), -77.0, dtype=ydt, device=x.device) for _ in sel]
        rbuf = [torch.full((8, 140), 1.0, dtype=ydt, device=x.device) if r else None for r in res]
        keep = [L.ptr_array([a.pack[f] for a in sel]) for f in range(5)] + [L.ptr_array(outs), L.ptr_array(rbuf)]
        ns = (ctypes.c_int * 2)(*[a.n for a in sel])
        Bs = (ctypes.c_int * 2)(*[a.pack[2].shape[1] for a in sel])
        ldy, ldrs = (ctypes.c_int64 * 2)(140, 140), (ctypes.c_int64 * 2)(140, ldr)
        rc = L.lib().pt2q_ternary_decode_fused(
            L.ptr(x), L.dtype_code(x), tokens, m, m, 2, vp(ns), keep[0][0], keep[1][0], keep[2][0], keep[3][0], vp(Bs), bs,
            keep[4][0], keep[5][0], L._DT[ydt], vp(ldy), epilogue, L.ptr(weight), eps,
            keep[6][0] if any(res) else None, vp(ldrs), L.stream_of(x.device))
        torch.cuda.synchronize()
        assert rc == 0 or all(bool((o == -77.0).all()) for o in outs)
        return rc

    assert call() == 0 and call(weight=w) == 0 and call(res=(False, True), weight=w) == 0  # the harness is valid
    assert call(epilogue=L.DECODE_SWIGLU, idx=(0, 2), res=(False, False), weight=w) == 0
    assert call(ydtype=torch.float32) == E_ARG and call(ydtype=torch.float32, res=(False, True)) == E_ARG
    assert call(ydtype=torch.float32, res=(False, False), weight=w) == 0  # the norm alone takes an fp32 output
    assert call(epilogue=L.DECODE_SWIGLU, idx=(0, 2), res=(True, False)) == E_ARG
    assert call(ldr=ms[1].n - 1) == E_ARG and call(ldr=ms[1].n) == 0
    for eps in (-1e-6, float("nan"), float("inf")):
        assert call(weight=w, eps=eps) == E_ARG, eps
    assert call(weight=None, eps=float("nan"), res=(False, False)) == 0  # no norm: eps is not looked at
    assert call(weight=w, eps=0.0) == 0

    # pt2q_rmsnorm
    def rms(xp=x, wp=w, eps=EPS, ldx=m, ldy=m, null_y=False):
        y = torch.full((tokens, m), -77.0, dtype=TDT[dtype], device=x.device)
        rc = L.lib().pt2q_rmsnorm(L.ptr(xp), L.dtype_code(x), tokens, ldx, m, L.ptr(wp), eps, None if null_y else L.ptr(y),
                                  ldy, L.stream_of(x.device))
        torch.cuda.synchronize()
        assert rc == 0 or bool((y == -77.0).all())
        return rc

    assert rms() == 0
    assert rms(wp=None) == E_ARG and rms(xp=None) == E_ARG and rms(null_y=True) == E_ARG
    assert rms(eps=-1.0) == E_ARG and rms(eps=float("nan")) == E_ARG
    assert rms(ldx=m - 1) == E_ARG and rms(ldy=m - 1) == E_ARG
    # through Python: the same refusals as exceptions
    a = ms[0]
    with pytest.raises(L.Pt2qError):
        one(pt2q, a, x, out_dtype=torch.float32, residual=torch.zeros((tokens, a.n), dtype=torch.float32, device=x.device))
    with pytest.raises(L.Pt2qError):
        one(pt2q, a, x, norm=(w, -1.0))
    with pytest.raises(L.Pt2qError):
        one(pt2q, a, x, norm=(w[:-1], EPS))
    with pytest.raises(L.Pt2qError):
        one(pt2q, a, x, residual=torch.zeros((tokens, a.n + 1), dtype=TDT[dtype], device=x.device))
    with pytest.raises(L.Pt2qError):
        pt2q.rms_norm(x, w.float(), EPS)


def test_fused_entry_without_extras_is_the_plain_call(pt2q):
    """A group of one through pt2q_ternary_decode_fused with no norm and no residual: the bits of
    pt2q_ternary_decode."""
    m, bs, tokens, dtype = SHAPES[1]
    a = G.group(pt2q, m, bs, tokens, dtype, 1)[0]
    out = torch.empty((tokens, a.n), dtype=TDT[dtype], device=a.x.device)
    pt2q.ternary._decode_group(a.x, [a.pack], bs, [out], pt2q._lib.DECODE_PLAIN, "pt2q_ternary_decode_fused",
                               None, [None], "test")
    assert torch.equal(out, a.alone(pt2q))


# ---- TernaryMLPBlock ----

@pytest.fixture
def block_cap8(pt2q, monkeypatch):
    """The two-launch block, and the two-launch MLP it is compared with, for every token count the
    library takes (the shipped caps are the measured crossovers, which may be lower)."""
    cap = pt2q._lib.lib().pt2q_ternary_decode_max_tokens()
    monkeypatch.setattr(pt2q.ternary, "block_decode_max_tokens", cap)
    monkeypatch.setattr(pt2q.ternary, "mlp_decode_max_tokens", cap)


def _block(pt2q, dtype="fp16"):
    mlp, gm, um, dm = G._mlp(pt2q, dtype)
    w = normed(gm)[0]
    return pt2q.TernaryMLPBlock(w, EPS, mlp), mlp, gm, w


def _spy(pt2q, monkeypatch):
    """Records whether ternary_decode_swiglu was called with the norm prologue."""
    seen = []
    real = pt2q.ternary.ternary_decode_swiglu

    def swiglu(*a, **kw):
        seen.append(kw.get("norm") is not None)
        return real(*a, **kw)
    monkeypatch.setattr(pt2q.ternary, "ternary_decode_swiglu", swiglu)
    return seen


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_mlp_block_fused_forward(pt2q, block_cap8, monkeypatch, dtype):
    blk, mlp, gm, w = _block(pt2q, dtype)
    seen = _spy(pt2q, monkeypatch)
    for T in (1, 3, 8):
        h = gm.x[:T]
        del seen[:]
        y = blk(h)
        assert seen == [True]  # one SwiGLU launch, with the norm in it
        assert y.dtype == h.dtype and torch.equal(y, h + mlp(pt2q.rms_norm(h, w, EPS)))
        assert torch.equal(h, gm.x[:T])  # the input is not the output
    y4 = blk(gm.x[:4].reshape(2, 2, G.HID))
    assert tuple(y4.shape) == (2, 2, G.HID) and torch.equal(y4.reshape(4, G.HID), blk(gm.x[:4]))
    # and the pieces by the restatements: RMSNORM16, then DOT64P and SWIGLU16, DOT64P, RESADD16
    gm_, um_ = G.pair(pt2q, G.INTER, G.HID, G.MBS, 8, dtype)
    dm_ = G.member(pt2q, G.HID, G.INTER, G.MBS, 8, dtype, 2002)
    a = gref.swiglu(want_norm(gm_), want_norm(um_), dtype)
    c = dm_.c
    d = ref.finish(ref.fold(a, c["alpha"], c["mu"], c["T"], c["perm"], c["bs"], dtype), c["bias"], dtype)
    assert np.array_equal(host(blk(gm.x).float()), nref.resadd(d, gm.c["x"], dtype))


def test_mlp_block_above_the_cap_and_in_mfma_mode(pt2q, monkeypatch):
    """As shipped: more tokens than block_decode_max_tokens, and any call once a projection is
    switched to decode="mfma", are rms_norm, the MLP and torch's add."""
    blk, mlp, gm, w = _block(pt2q)
    seen = _spy(pt2q, monkeypatch)
    assert 0 <= pt2q.ternary.block_decode_max_tokens <= pt2q._lib.lib().pt2q_ternary_decode_max_tokens()
    k = min(pt2q.ternary.block_decode_max_tokens, pt2q.ternary.mlp_decode_max_tokens)  # the block follows its MLP
    h = gm.x[:k + 1]
    assert torch.equal(blk(h), h + mlp(pt2q.rms_norm(h, w, EPS))) and True not in seen
    if k >= 1:
        del seen[:]
        blk(h[:k])
        assert seen == [True]
    monkeypatch.setattr(pt2q.ternary, "block_decode_max_tokens", 8)
    monkeypatch.setattr(pt2q.ternary, "mlp_decode_max_tokens", 1)
    del seen[:]
    assert torch.equal(blk(gm.x[:2]), gm.x[:2] + mlp(pt2q.rms_norm(gm.x[:2], w, EPS))) and True not in seen
    try:
        pt2q.set_decode(blk, "mfma")
        del seen[:]
        assert torch.equal(blk(h[:1]), h[:1] + mlp(pt2q.rms_norm(h[:1], w, EPS))) and seen == []
    finally:
        pt2q.set_decode(blk, "fused")
    with pytest.raises(pt2q._lib.Pt2qError):
        pt2q.TernaryMLPBlock(w[:-1], EPS, mlp)
    with pytest.raises(pt2q._lib.Pt2qError):
        pt2q.TernaryMLPBlock(w, EPS, mlp.down_proj)


def test_mlp_block_graph_capture_replays_eager_bits(pt2q, block_cap8):
    blk, mlp, gm, w = _block(pt2q)
    h = gm.x[:1].clone()
    eager = blk(h).clone()  # eager warm-up: loads the kernels before capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = blk(h)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)


def test_mlp_block_state_dict_round_trip(pt2q, block_cap8):
    blk, mlp, gm, w = _block(pt2q)
    sd = blk.state_dict()
    assert "norm_weight" in sd and "mlp.gate_proj.T" in sd and "mlp.down_proj.alpha" in sd
    y = blk(gm.x[:2])
    kids = [pt2q.TernaryLinear(l.in_features, l.out_features, l.block_size, bias=True, dtype=l.dtype, decode="fused")
            for l in (mlp.gate_proj, mlp.up_proj, mlp.down_proj)]
    fresh = pt2q.TernaryMLPBlock(torch.zeros_like(w), EPS, pt2q.TernaryGatedMLP(*kids))
    assert not torch.equal(fresh(gm.x[:2]), y)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.norm_weight, w) and torch.equal(fresh(gm.x[:2]), y)
