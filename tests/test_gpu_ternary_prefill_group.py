"""pt2q_ternary_prefill_group (csrc/ternary_prefill.hip: 1..4 linears on the same x in one gather and one
GEMM launch on the prefill kernel's body; SWIGLU in the 512-thread pair kernel), through
ternary_prefill_group, ternary_prefill_swiglu and TernaryGatedMLP(prefill="fused").

Exact data (tests/ternary_linear_ref.py) with one x for all members: member 0's x_int, every member's
expected output in integers.  |x_int| <= 8 and |16 w| <= 11, so no partial sum of an output passes
88 m + 512 units of 1/64, which _want asserts to be below 2**20: any order gives the same fp32 bits, and a
mismatch is a wrong operand."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_cases as sc
import ternary_linear_ref as ref
from ternary_group_ref import swiglu
from test_gpu_parity import cuda
from test_gpu_stream_order import cycles_per_ms, test_entry_on_a_delayed_stream as _delayed_stream  # noqa: F401
from test_gpu_ternary_skinny import TDT, _layer

pytestmark = pytest.mark.gpu

# The stream-order case of the entry (appended at collection, as tests/test_gpu_ternary_skinny_group.py does):
# SWIGLU, two feature tiles and two token tiles.
GN, GM, GTOK = 384, 512, 130


def _sc_make(seed):
    d = {}
    for z in "01":
        d.update(sc.tern(seed + 10 * int(z), GN, GM, 128, GTOK, sc.f16, z))
    return d


def _sc_call(c):
    a = lambda k: c.arr(k + "0", k + "1")  # noqa: E731
    return c.L.pt2q_ternary_prefill_group(
        c.p("x"), sc.F16, GTOK, GM, GM, 2, c.ints([GN, GN]), a("codes"), a("gather"), a("alpha"), a("mu"),
        c.ints([GM // 128] * 2), 128, a("bias"), c.arr("y"), sc.F16, c.ints([GN], ctypes.c_int64), 1, c.p("ws"),
        c.nbytes("ws"), c.st)


sc.case("ternary-prefill-group-swiglu", "pt2q_ternary_prefill_group", _sc_make, _sc_call, ("y",),
        "test_gpu_ternary_prefill_group.py::test_swiglu_exact", out={"y": ((GTOK, GN), sc.f16)},
        ws={"ws": lambda L: L.pt2q_ternary_prefill_group_workspace_bytes(GTOK, GM, 2)},
        index=sc.tern_index(GM, ("0", "1")))
sc.BY_ID[sc.CASES[-1].id] = sc.CASES[-1]


def test_stream_order(pt2q, cycles_per_ms):  # noqa: F811
    _delayed_stream(pt2q, cycles_per_ms, sc.BY_ID["ternary-prefill-group-swiglu"])

# (m, bs, tokens, ns)
PLAIN = [
    (128, 128, 100, (40,)),                # one block, two stages, no next fetch; ragged token tile
    (200, 256, 129, (130, 257)),           # padding positions, per-channel; second token tile of one row
    (640, 128, 257, (256, 300, 40, 513)),  # ring wraps, block slots alternate; member tiles at and across 256
    (512, 256, 128, (33, 33)),             # a scale block spans two packed blocks
]
# (m, bs, tokens, n)
SWIGLU = [(128, 128, 100, 130), (200, 256, 129, 256), (640, 128, 257, 300), (512, 256, 128, 513)]


def _ints(v, ty=ctypes.c_int):
    return ctypes.cast((ty * len(v))(*v), ctypes.c_void_p)


def _members(pt2q, m, bs, tokens, ns, dtype, compat=False):
    """Exact-data layers (decode="mfma") of ns features on m columns and the x_int they all read (member 0's)."""
    cases = [ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens) + z) for z, n in enumerate(ns)]
    return cases, [_layer(pt2q, c, dtype, compat, "mfma") for c in cases], cases[0]["x_int"].astype(np.int64)


def _want(c, x_int, compat, bias, out):
    """Member c's expected output on x_int, float32 holding `out` ("fp32" | "fp16" | "bf16") values."""
    assert 88 * c["m"] + 512 < ref.EXACT_BOUND
    u = x_int @ ref.weight_int(c, compat).T + (16 * c["bias_int"].astype(np.int64)[None, :] if bias else 0)
    y = (u / ref.UNITS).astype(np.float32)
    return y if out == "fp32" else ref.round16(y, out)


def _x(x_int, dtype, scale=1.0):
    return (cuda((x_int / 4).astype(np.float32)) * scale).to(TDT[dtype])


def _eq(y, want):
    return torch.equal(y.float().cpu(), torch.from_numpy(np.asarray(want, np.float32)))


def _nobias(lay):
    return lay._packed[:4] + (None,)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("m,bs,tokens,ns", PLAIN)
def test_plain_group_exact(pt2q, m, bs, tokens, ns, dtype):
    compat = dtype == "bf16"
    cases, lays, x_int = _members(pt2q, m, bs, tokens, ns, dtype, compat)
    packs = [lay._packed if z else _nobias(lay) for z, lay in enumerate(lays)]  # member 0 without its bias
    wants = [_want(c, x_int, compat, z > 0, "fp32") for z, c in enumerate(cases)]  # exact in fp32
    for ydt, out in ((TDT[dtype], dtype), (torch.float32, "fp32")):
        ys = pt2q.ternary_prefill_group(_x(x_int, dtype), packs, out_dtype=ydt, block_size=bs)
        for z, (w, y) in enumerate(zip(wants, ys)):
            assert _eq(y, w if out == "fp32" else ref.round16(w, out)), (z, out)


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("tokens", [256, 300])
def test_plain_group_is_the_lone_call(pt2q, tokens, count):
    """Not exactly summable (x scaled by 0.37): only the prefill kernel's own chain gives its bits."""
    m, bs, _, ns = PLAIN[2]
    _, lays, x_int = _members(pt2q, m, bs, tokens, ns[:count], "fp16")
    x = _x(x_int, "fp16", 0.37)
    for lay, y in zip(lays, pt2q.ternary_prefill_group(x, lays)):
        assert torch.equal(y, lay(x))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("m,bs,tokens,n", SWIGLU)
def test_swiglu_exact(pt2q, m, bs, tokens, n, dtype):
    compat = dtype == "bf16"
    cases, lays, x_int = _members(pt2q, m, bs, tokens, (n, n), dtype, compat)
    for bias in (True, False):
        g, u = (_want(c, x_int, compat, bias, dtype) for c in cases)
        h = pt2q.ternary_prefill_swiglu(_x(x_int, dtype), *[lay._packed if bias else _nobias(lay) for lay in lays],
                                        block_size=bs)
        assert _eq(h, swiglu(g, u, dtype)), bias


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_swiglu_of_the_lone_outputs(pt2q, dtype):
    m, bs, _, n = SWIGLU[2]
    _, lays, x_int = _members(pt2q, m, bs, 256, (n, n), dtype)
    x = _x(x_int, dtype, 0.37)
    g, u = (lay(x).float().cpu().numpy() for lay in lays)
    hs = [pt2q.ternary_prefill_swiglu(x, *lays) for _ in range(8)]
    assert _eq(hs[0], swiglu(g, u, dtype))
    assert all(torch.equal(h, hs[0]) for h in hs[1:])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_random_against_float64(pt2q, dtype):
    """Scales in the range of real layers, x ~ N(0, 1) in TX, fp32 y.  The bound allows one unit in the
    last place (2^-24 relative, doubled to 2^-23 for the rounding of the sum itself) per accumulation step
    in any order: m products and the bias, against the sum of magnitudes."""
    m, bs, tokens, ns = PLAIN[2]
    rng = np.random.default_rng(m)
    B = ref.nblocks(m, bs)
    x = ref.round16(rng.standard_normal((tokens, m)), dtype)
    cs = [{"n": n, "m": m, "bs": bs, "T": rng.integers(-1, 2, size=(n, m)).astype(np.int8),
           "alpha": ref.round16(rng.random((n, B)) * 0.05 + 0.005, dtype),
           "mu": ref.round16(rng.standard_normal((n, B)) * 0.002, dtype),
           "perm": rng.permutation(m).astype(np.int64), "bias": ref.round16(rng.standard_normal(n) * 0.1, dtype)}
          for n in ns]
    ys = pt2q.ternary_prefill_group(cuda(x).to(TDT[dtype]), [_layer(pt2q, c, dtype, False, "mfma") for c in cs],
                                    out_dtype=torch.float32)
    for c, y in zip(cs, ys):
        W = ref.weight_tx(c["alpha"], c["mu"], c["T"], c["perm"], bs, False, dtype).astype(np.float64)
        want = x.astype(np.float64) @ W.T + c["bias"]
        bound = (m + 1) * 2.0 ** -23 * (np.abs(x).astype(np.float64) @ np.abs(W).T + np.abs(c["bias"]))
        err = np.abs(y.cpu().numpy().astype(np.float64) - want)
        print(f"n = {c['n']}: max err / bound = {(err / bound).max():.3e}")
        assert (err <= bound).all()


def _raw(pt2q, x, lays, ys, epilogue, ws, ws_bytes):
    """The C entry on the layers' packed operands: its status, with the caller's outputs and workspace."""
    L = pt2q._lib
    arrs = [L.ptr_array([lay._packed[i] for lay in lays]) for i in range(5)] + [L.ptr_array(ys)]
    m = lays[0].in_features
    return L.lib().pt2q_ternary_prefill_group(
        L.ptr(x), L.dtype_code(x), x.shape[0], m, m, len(lays), _ints([lay.out_features for lay in lays]),
        arrs[0][0], arrs[1][0], arrs[2][0], arrs[3][0], _ints([lay._packed[2].shape[1] for lay in lays]),
        lays[0].block_size, arrs[4][0], arrs[5][0], L.dtype_code(ys[0]), _ints([y.shape[1] for y in ys], ctypes.c_int64),
        epilogue, L.ptr(ws), ws_bytes, L.stream_of(x.device))


def test_workspace_hygiene(pt2q):
    m, bs, tokens, n = SWIGLU[2]
    cases, lays, x_int = _members(pt2q, m, bs, tokens, (n, n), "fp16")
    x = _x(x_int, "fp16")
    nbytes = pt2q._lib.lib().pt2q_ternary_prefill_group_workspace_bytes(tokens, m, 2)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=x.device)
    g, u = (_want(c, x_int, False, True, "fp16") for c in cases)
    for _ in range(2):  # PLAIN then SWIGLU on one workspace
        ys = [torch.empty((tokens, n), dtype=torch.float16, device=x.device) for _ in range(2)]
        assert _raw(pt2q, x, lays, ys, 0, ws, nbytes) == 0
        assert _eq(ys[0], g) and _eq(ys[1], u)
        assert _raw(pt2q, x, lays, ys[:1], 1, ws, nbytes) == 0
        assert _eq(ys[0], swiglu(g, u, "fp16"))


@pytest.mark.parametrize("bs,ns,epilogue,ydt,short,status", [
    (64, (40, 40), 0, torch.float16, 0, 3),       # PT2Q_E_UNSUPPORTED: bs < m, no multiple of 128
    (256, (40, 40), 0, torch.float16, 1, 5),      # PT2Q_E_WORKSPACE: one byte short
    (256, (40,) * 5, 0, torch.float16, 0, 1),     # PT2Q_E_ARG from here on: count 5
    (256, (40,) * 3, 1, torch.float16, 0, 1),     # SWIGLU with count 3
    (256, (40, 33), 1, torch.float16, 0, 1),      # SWIGLU with n[0] != n[1]
    (256, (40, 40), 1, torch.float32, 0, 1),      # SWIGLU with f32 y
])
def test_refused_calls_leave_y_alone(pt2q, bs, ns, epilogue, ydt, short, status):
    tokens, m = 65, 200
    _, lays, x_int = _members(pt2q, m, bs, tokens, ns, "fp16")
    x = _x(x_int, "fp16")
    nbytes = pt2q._lib.lib().pt2q_ternary_prefill_group_workspace_bytes(tokens, m, min(len(ns), 4))
    ws = torch.zeros(2 * nbytes, dtype=torch.uint8, device=x.device)
    ys = [torch.full((tokens, n), 7.0, dtype=ydt, device=x.device) for n in ns]
    assert _raw(pt2q, x, lays, ys, epilogue, ws, nbytes - 1 if short else 2 * nbytes) == status
    torch.cuda.synchronize()
    assert all(bool((y == 7.0).all()) for y in ys)


def test_module_routing(pt2q, monkeypatch):
    monkeypatch.setattr(pt2q.ternary, "prefill_mlp_min_tokens", 256)
    hid, inter = 256, 130
    x = _x(ref.exact_case(inter, hid, 128, 256, 9)["x_int"], "fp16", 0.37)

    def mlps(bs):
        gate, up, down = (_layer(pt2q, ref.exact_case(n, m, bs, 256, seed), "fp16", False, "mfma")
                          for seed, (n, m) in enumerate(((inter, hid), (inter, hid), (hid, inter))))
        return (gate, up, down), pt2q.TernaryGatedMLP(gate, up, down, prefill="fused"), \
            pt2q.TernaryGatedMLP(gate, up, down)

    def kids(p, v):
        return p[2](F.silu(p[0](v)) * p[1](v))
    p, fused, children = mlps(128)
    assert children.prefill == "children"
    assert torch.equal(fused(x), p[2](pt2q.ternary_prefill_swiglu(x, p[0], p[1])))
    assert torch.equal(fused(x[:255]), kids(p, x[:255]))
    assert torch.equal(children(x), kids(p, x))
    p, fused, _ = mlps(64)  # a block size the entry refuses: the children
    assert torch.equal(fused(x), kids(p, x))


def test_graph_replay(pt2q):
    """One SWIGLU call (gather, pair GEMM) captured once and replayed on three x written into the captured
    buffer: the eager bits."""
    m, bs, tokens, n = SWIGLU[2]
    _, lays, x_int = _members(pt2q, m, bs, tokens, (n, n), "fp16")
    xs = [_x(x_int, "fp16", s) for s in (0.37, 0.61, 1.0)]
    eager = [pt2q.ternary_prefill_swiglu(x, *lays).clone() for x in xs]
    assert not torch.equal(eager[0], eager[1])
    xg = torch.zeros_like(xs[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hg = pt2q.ternary_prefill_swiglu(xg, *lays)
    for x, want in zip(xs, eager):
        xg.copy_(x)
        graph.replay()
        assert torch.equal(hg, want)
