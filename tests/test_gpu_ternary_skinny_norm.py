"""pt2q_ternary_skinny_fused (csrc/ternary_skinny.hip): the RMSNorm prologue in the gather launch and the
residual epilogue where y is converted, through the norm= / residual(s)= keywords of ternary_skinny,
ternary_skinny_group and ternary_skinny_swiglu, and TernaryMLPBlock over decode="skinny" children.

The reference is the composition of entries the other test files pin to their numpy restatements:
rms_norm (RMSNORM16), the plain skinny calls, torch's 16-bit add (RESADD16).  Bit for bit, no tolerance.

The shapes are tests/ternary_skinny_cases.py's: NORM_SHAPES and NORM_SWIGLU on rows of m <= 2100, and
NORM_LONG (a PLAIN group of two on m = 10240) and NORM_RES_LONG (norm and residual, one member, m =
14336, 64 tokens) for the norm prologue's 512 threads on rows of 20 and 28 elements per thread, in front
of K slices of 5 and 7 blocks."""
import ctypes

import numpy as np
import pytest
import torch

import stream_cases as sc
import ternary_linear_ref as ref
import ternary_norm_ref as nref
from test_gpu_stream_order import cycles_per_ms, test_entry_on_a_delayed_stream as _delayed_stream  # noqa: F401
from test_gpu_ternary_skinny import TDT, _layer
from ternary_skinny_cases import NORM_LONG, NORM_RES_LONG, NORM_SHAPES as SHAPES, NORM_SWIGLU as SWIGLU, PLAIN
from test_gpu_ternary_skinny_group import _ints, _lone, _members, _x

pytestmark = pytest.mark.gpu

EPS = 1e-5
DTYPES = ["fp16", "bf16"]
E_ARG, E_UNSUPPORTED = 1, 3
# Stream order (appended at collection, as the two skinny test files do): PLAIN with norm and
# residuals, 17 tokens, two K slices per member.
GN, GM, GTOK = 384, 512, 17


def _sc_make(seed):
    d = {"nw": sc.t(nref.make_inputs(1, GM, "fp16", seed)[1], sc.f16)}
    for z in "01":
        d.update(sc.tern(seed + 10 * int(z), GN, GM, 128, GTOK, sc.f16, z))
        d["res" + z] = sc.acts(seed + 3 + int(z), GTOK, GN, sc.f16)
    return d


def _sc_call(c):
    a = lambda k: c.arr(k + "0", k + "1")  # noqa: E731
    return c.L.pt2q_ternary_skinny_fused(
        c.p("x"), sc.F16, GTOK, GM, GM, 2, c.ints([GN, GN]), a("codes"), a("gather"), a("alpha"), a("mu"),
        c.ints([GM // 128] * 2), 128, a("bias"), a("y"), sc.F16, c.ints([GN, GN], ctypes.c_int64), 0, c.p("nw"), EPS,
        a("res"), c.ints([GN, GN], ctypes.c_int64), c.p("ws"), c.nbytes("ws"), c.st)


sc.case("ternary-skinny-fused", "pt2q_ternary_skinny_fused", _sc_make, _sc_call, ("y0", "y1"),
        "test_gpu_ternary_skinny_norm.py::test_norm_and_residual", out={"y" + z: ((GTOK, GN), sc.f16) for z in "01"},
        ws={"ws": lambda L: L.pt2q_ternary_skinny_group_workspace_bytes(GTOK, GM, 2, _ints([GN, GN]), 0)},
        index=sc.tern_index(GM, ("0", "1")))
sc.BY_ID[sc.CASES[-1].id] = sc.CASES[-1]


def test_stream_order(pt2q, cycles_per_ms):  # noqa: F811
    _delayed_stream(pt2q, cycles_per_ms, sc.BY_ID["ternary-skinny-fused"])


def _setup(pt2q, m, bs, tokens, ns, dtype):
    cases, lays, x_int = _members(pt2q, m, bs, tokens, ns, dtype)
    x = _x(x_int, dtype, 0.37)
    w = torch.from_numpy(nref.make_inputs(1, m, dtype, seed=m)[1]).to(x.device).to(TDT[dtype])
    return cases, lays, x, w


def _off1(t, fill=0.0):  # t in a buffer with a padded leading dimension, its base one element off
    buf = torch.full((t.shape[0], t.shape[1] + 6), fill, dtype=t.dtype, device=t.device)
    buf[:, 1:1 + t.shape[1]] = t
    return buf[:, 1:1 + t.shape[1]]


def _res(y, seed):
    g = torch.Generator(device=y.device).manual_seed(seed)
    return (torch.randn(y.shape, device=y.device, generator=g) * 0.5).to(y.dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,bs,tokens,ns", SHAPES + [NORM_LONG])
def test_norm_plain_group(pt2q, m, bs, tokens, ns, dtype):
    _, lays, x, w = _setup(pt2q, m, bs, tokens, ns, dtype)
    if m == 640:  # ldx > m and a base that is only 2-byte aligned
        x = _off1(x)
        assert x.data_ptr() % 4 == 2 and x.stride(0) > m
    keep = x.clone()
    xn = pt2q.rms_norm(x, w, EPS)
    for ydt in (TDT[dtype], torch.float32):
        ys = pt2q.ternary_skinny_group(x, lays, out_dtype=ydt, norm=(w, EPS))
        for z, (lay, y) in enumerate(zip(lays, ys)):
            assert torch.equal(y, pt2q.ternary_skinny(xn, *lay._packed[:4], lay.block_size, lay._packed[4], out_dtype=ydt)), z
    y0 = pt2q.ternary_skinny(x, *lays[0]._packed[:4], lays[0].block_size, lays[0]._packed[4], norm=(w, EPS))
    assert torch.equal(y0, _lone(pt2q, lays[0], xn)) and torch.equal(x, keep)  # x itself is not written


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,bs,tokens,n", SWIGLU)
def test_norm_swiglu(pt2q, m, bs, tokens, n, dtype):
    _, lays, x, w = _setup(pt2q, m, bs, tokens, (n, n), dtype)
    h = pt2q.ternary_skinny_swiglu(x, *lays, norm=(w, EPS))
    assert torch.equal(h, pt2q.ternary_skinny_swiglu(pt2q.rms_norm(x, w, EPS), *lays))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,bs,tokens,ns", SHAPES + [(512, 128, 3, (65,))])
def test_residual_plain_group(pt2q, m, bs, tokens, ns, dtype):
    """Member 0: residual and y with a padded leading dimension and an unaligned base; 1: none; others: residual is out."""
    _, lays, x, _ = _setup(pt2q, m, bs, tokens, ns, dtype)
    alone = [_lone(pt2q, lay, x) for lay in lays]
    rs = [_res(y, 60 + z) for z, y in enumerate(alone)]
    outs = [_off1(torch.empty_like(alone[0]), -77.0)] + [r.clone() for r in rs[1:]]
    given = [_off1(rs[0])] + [None if z == 1 else o for z, o in enumerate(outs)][1:]
    back = pt2q.ternary_skinny_group(x, lays, outs=outs, residuals=given)
    for z, (y, r, a) in enumerate(zip(back, rs, alone)):
        assert y is outs[z] and torch.equal(y, a if z == 1 else r + a), z
    pad = outs[0]._base
    assert bool((pad[:, :1] == -77.0).all()) and bool((pad[:, 1 + alone[0].shape[1]:] == -77.0).all())
    y0 = pt2q.ternary_skinny(x, *lays[0]._packed[:4], lays[0].block_size, lays[0]._packed[4], residual=rs[0])
    assert torch.equal(y0, rs[0] + alone[0])


def _norm_and_residual(pt2q, shape, dtype):
    _, lays, x, w = _setup(pt2q, *shape, dtype)
    xn = pt2q.rms_norm(x, w, EPS)
    rs = [_res(_lone(pt2q, lay, x), 80 + z) for z, lay in enumerate(lays)]
    for lay, y, r in zip(lays, pt2q.ternary_skinny_group(x, lays, norm=(w, EPS), residuals=rs), rs):
        assert torch.equal(y, r + _lone(pt2q, lay, xn))


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_and_residual(pt2q, dtype):
    _norm_and_residual(pt2q, PLAIN[1], dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_norm_and_residual_long_rows(pt2q, dtype):
    """One member, m = 14336, 64 tokens: 28 elements per thread of the norm, then 16 slices of 7 blocks."""
    _norm_and_residual(pt2q, NORM_RES_LONG, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_float64(pt2q, dtype):
    """Against dequantised weights · rmsnorm64(x) + bias + residual: no further than the unfused composition."""
    m, bs, tokens = PLAIN[1][:3]
    cases, lays, x, w = _setup(pt2q, m, bs, tokens, (65,), dtype)
    c, lay = cases[0], lays[0]
    r = _res(_lone(pt2q, lay, x), 90)
    W = ref.weight_tx(c["alpha"], c["mu"], c["T"], c["perm"], bs, False, dtype).astype(np.float64)
    f64 = lambda t: t.float().cpu().numpy().astype(np.float64)  # noqa: E731
    want = nref.rmsnorm64(f64(x), f64(w), EPS) @ W.T + c["bias"].astype(np.float64) + f64(r)
    fused = pt2q.ternary_skinny(x, *lay._packed[:4], bs, lay._packed[4], norm=(w, EPS), residual=r)
    unfused = r + _lone(pt2q, lay, pt2q.rms_norm(x, w, EPS))
    errs = [np.abs(f64(y) - want).max() for y in (fused, unfused)]
    assert errs[0] <= errs[1]


def _fused(pt2q, x, lays, ys, epilogue=0, weight=None, eps=EPS, res=None, ldr=True):
    L = pt2q._lib  # the C entry on the layers' packed operands: its status
    arrs = [L.ptr_array([lay._packed[i] for lay in lays]) for i in range(5)] + [L.ptr_array(ys), L.ptr_array(res or [None])]
    m, ns = lays[0].in_features, [lay.out_features for lay in lays]
    nbytes = L.lib().pt2q_ternary_skinny_group_workspace_bytes(x.shape[0], m, len(lays), _ints(ns), epilogue)
    ws = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=x.device)
    ldrs = _ints(ldr, ctypes.c_int64) if isinstance(ldr, list) else _ints([y.shape[1] for y in ys], ctypes.c_int64) if ldr else None
    rc = L.lib().pt2q_ternary_skinny_fused(
        L.ptr(x), L.dtype_code(x), x.shape[0], x.stride(0), m, len(lays), _ints(ns), arrs[0][0], arrs[1][0], arrs[2][0],
        arrs[3][0], _ints([lay._packed[2].shape[1] for lay in lays]), lays[0].block_size, arrs[4][0], arrs[5][0],
        L.dtype_code(ys[0]), _ints([y.shape[1] for y in ys], ctypes.c_int64), epilogue, L.ptr(weight), eps,
        arrs[6][0] if res else None, ldrs, L.ptr(ws), ws.numel(), L.stream_of(x.device))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_and_the_entry_without_extras(pt2q, dtype):
    _, lays, x, w = _setup(pt2q, 640, 128, 17, (65, 65), dtype)
    new = lambda ydt=TDT[dtype], k=2: [torch.full((17, 65), 7.0, dtype=ydt, device=x.device) for _ in range(k)]  # noqa: E731
    rs = new()
    ys = new()  # both extras NULL: the plain entries' bits
    assert _fused(pt2q, x, lays, ys) == 0 and all(torch.equal(y, v) for y, v in zip(ys, pt2q.ternary_skinny_group(x, lays)))
    assert _fused(pt2q, x, lays[:1], ys[:1]) == 0 and torch.equal(ys[0], _lone(pt2q, lays[0], x))
    assert _fused(pt2q, x, lays, new(), weight=w, res=rs) == 0 and _fused(pt2q, x, lays, new(torch.float32), weight=w) == 0
    assert _fused(pt2q, x, lays, new(), weight=None, eps=float("nan")) == 0  # no norm: eps is not looked at
    refused = [dict(weight=w, eps=e) for e in (-1e-6, float("inf"), float("nan"))] + [
        dict(ys=new(torch.float32), res=new(torch.float32)), dict(ys=new(k=1), epilogue=1, res=rs[:1]),
        dict(res=[None, rs[1]], ldr=False), dict(res=rs, ldr=[65, 64])]
    for kw in refused:
        ys = kw.pop("ys", None) or new()
        assert _fused(pt2q, x, lays, ys, **kw) == E_ARG, kw
        assert all(bool((y == 7.0).all()) for y in ys), kw
    wide = _layer(pt2q, ref.exact_case(8, 32769, 128, 2, 5), dtype, False)  # one column past the LDS image
    xw, y = torch.ones((2, 32769), dtype=TDT[dtype], device=x.device), torch.full((2, 8), 7.0, dtype=TDT[dtype], device=x.device)
    assert _fused(pt2q, xw, [wide], [y], weight=xw[0]) == E_UNSUPPORTED and bool((y == 7.0).all())
    assert _fused(pt2q, xw, [wide], [y]) == 0  # only the norm is capped
    for kw in (dict(norm=(w[:-1], EPS)), dict(residuals=[rs[0][:, :-1], None])):
        with pytest.raises(pt2q._lib.Pt2qError):
            pt2q.ternary_skinny_group(x, lays, **kw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_mlp_block_over_skinny_children(pt2q, monkeypatch, dtype):
    cap = pt2q._lib.lib().pt2q_ternary_skinny_max_tokens()
    for name in ("skinny_max_tokens", "skinny_mlp_max_tokens", "skinny_block_max_tokens"):
        monkeypatch.setattr(pt2q.ternary, name, cap)  # the shipped caps are measured crossovers, which may be lower
    hid, inter, bs = 256, 130, 128
    gate, up, down = (_layer(pt2q, ref.exact_case(n, m, bs, cap + 1, seed), dtype, False)
                      for seed, (n, m) in enumerate(((inter, hid), (inter, hid), (hid, inter))))
    mlp = pt2q.TernaryGatedMLP(gate, up, down)
    h = _x(ref.exact_case(inter, hid, bs, cap + 1, 9)["x_int"], dtype, 0.37)
    w = torch.from_numpy(nref.make_inputs(1, hid, dtype, seed=hid)[1]).to(h.device).to(TDT[dtype])
    blk = pt2q.TernaryMLPBlock(w, EPS, mlp)
    seen, real = [], pt2q.ternary.ternary_skinny_swiglu

    def swiglu(*a, **kw):
        seen.append(kw.get("norm") is not None)
        return real(*a, **kw)
    monkeypatch.setattr(pt2q.ternary, "ternary_skinny_swiglu", swiglu)
    for tokens, fused in ((2, True), (cap, True), (cap + 1, False), (1, False)):
        del seen[:]
        y = blk(h[:tokens])
        assert (True in seen) == fused, tokens
        assert torch.equal(y, h[:tokens] + mlp(pt2q.rms_norm(h[:tokens], w, EPS))), tokens
