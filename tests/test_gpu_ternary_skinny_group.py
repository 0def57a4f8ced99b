"""pt2q_ternary_skinny_group (csrc/ternary_skinny.hip: 1..4 linears on the same x in one gather and one
GEMM launch; SWIGLU where the K-split partials are summed), through ternary_skinny_group,
ternary_skinny_swiglu and TernaryGatedMLP over decode="skinny" children.

Exact data (tests/ternary_linear_ref.py) with one x for all members: member 0's x_int, every member's
expected output in integers.  |x_int| <= 8 and |16 w| <= 11, so no partial sum of an output passes
88 m + 512 units of 1/64, which _want asserts to be below 2**20: any order gives the same fp32 bits.

The shapes are tests/ternary_skinny_cases.py's.  PLAIN and SWIGLU: ragged edges, scale-block edges, every
NT, on K slices of 1..3 blocks.  PLAIN_LONG: a 256-tile member of 2 splits (4-block slices, 6 MiB of
partial tiles) beside a 2-tile member of 4 splits in one launch, so the first member's tiles see
workgroups of slices they do not have.  SWIGLU_LONG: 5-block slices and 32 tickets per tile.
test_ternary_skinny_cases_cpu.py holds the tables to those plans."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_cases as sc
import ternary_linear_ref as ref
from ternary_group_ref import swiglu
from ternary_skinny_cases import PLAIN, PLAIN_LONG, SWIGLU, SWIGLU_LONG
from test_gpu_parity import cuda
from test_gpu_stream_order import cycles_per_ms, test_entry_on_a_delayed_stream as _delayed_stream  # noqa: F401
from test_gpu_ternary_skinny import TDT, _layer

pytestmark = pytest.mark.gpu

# The stream-order case of the entry (appended at collection, as tests/test_gpu_ternary_skinny.py does):
# SWIGLU, 17 tokens, two K slices per member, so every call rewrites the shared counters and the partials.
GN, GM, GTOK = 384, 512, 17


def _sc_make(seed):
    d = {}
    for z in "01":
        d.update(sc.tern(seed + 10 * int(z), GN, GM, 128, GTOK, sc.f16, z))
    return d


def _sc_call(c):
    a = lambda k: c.arr(k + "0", k + "1")  # noqa: E731
    return c.L.pt2q_ternary_skinny_group(
        c.p("x"), sc.F16, GTOK, GM, GM, 2, c.ints([GN, GN]), a("codes"), a("gather"), a("alpha"), a("mu"),
        c.ints([GM // 128] * 2), 128, a("bias"), c.arr("y"), sc.F16, c.ints([GN], ctypes.c_int64), 1, c.p("ws"),
        c.nbytes("ws"), c.st)


sc.case("ternary-skinny-group-swiglu", "pt2q_ternary_skinny_group", _sc_make, _sc_call, ("y",),
        "test_gpu_ternary_skinny_group.py::test_swiglu_exact", out={"y": ((GTOK, GN), sc.f16)},
        ws={"ws": lambda L: L.pt2q_ternary_skinny_group_workspace_bytes(GTOK, GM, 2, _ints([GN, GN]), 1)},
        index=sc.tern_index(GM, ("0", "1")))
sc.BY_ID[sc.CASES[-1].id] = sc.CASES[-1]


def test_stream_order(pt2q, cycles_per_ms):  # noqa: F811
    _delayed_stream(pt2q, cycles_per_ms, sc.BY_ID["ternary-skinny-group-swiglu"])


def _ints(v, ty=ctypes.c_int):
    return ctypes.cast((ty * len(v))(*v), ctypes.c_void_p)


def _members(pt2q, m, bs, tokens, ns, dtype, compat=False):
    """Exact-data layers of ns features on m columns and the x_int they all read (member 0's)."""
    cases = [ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens) + z) for z, n in enumerate(ns)]
    return cases, [_layer(pt2q, c, dtype, compat) for c in cases], cases[0]["x_int"].astype(np.int64)


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


def _lone(pt2q, lay, x):
    return pt2q.ternary_skinny(x, *lay._packed[:4], lay.block_size, lay._packed[4])


def _nobias(lay):
    return lay._packed[:4] + (None,)


@pytest.mark.parametrize("m,bs,tokens,ns,dtype", [s + (d,) for s in PLAIN for d in ("fp16", "bf16")
                                                  if d == "fp16" or s[3][0] != 32705] + PLAIN_LONG)
def test_plain_group_exact(pt2q, m, bs, tokens, ns, dtype):
    compat = dtype == "bf16"
    cases, lays, x_int = _members(pt2q, m, bs, tokens, ns, dtype, compat)
    packs = [lay._packed if z else _nobias(lay) for z, lay in enumerate(lays)]  # member 0 without its bias
    wants = [_want(c, x_int, compat, z > 0, "fp32") for z, c in enumerate(cases)]  # exact in fp32
    for ydt, out in ((TDT[dtype], dtype), (torch.float32, "fp32")):
        ys = pt2q.ternary_skinny_group(_x(x_int, dtype), packs, out_dtype=ydt, block_size=bs)
        for z, (w, y) in enumerate(zip(wants, ys)):
            assert _eq(y, w if out == "fp32" else ref.round16(w, out)), (z, out)


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("m,bs,tokens,ns", [PLAIN[1], PLAIN[2][:3] + ((40, 130, 63, 129),)])
def test_plain_group_is_the_members_alone(pt2q, m, bs, tokens, ns, count):
    """Not exactly summable (x scaled by 0.37): only the lone call's own split and order give its bits."""
    _, lays, x_int = _members(pt2q, m, bs, tokens, ns[:count], "fp16")
    x = _x(x_int, "fp16", 0.37)
    for lay, y in zip(lays, pt2q.ternary_skinny_group(x, lays)):
        assert torch.equal(y, _lone(pt2q, lay, x))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("m,bs,tokens,n", SWIGLU + SWIGLU_LONG)
def test_swiglu_exact(pt2q, m, bs, tokens, n, dtype):
    compat = dtype == "bf16"
    cases, lays, x_int = _members(pt2q, m, bs, tokens, (n, n), dtype, compat)
    for bias in (True, False):
        g, u = (_want(c, x_int, compat, bias, dtype) for c in cases)
        h = pt2q.ternary_skinny_swiglu(_x(x_int, dtype), *[lay._packed if bias else _nobias(lay) for lay in lays],
                                       block_size=bs)
        assert _eq(h, swiglu(g, u, dtype)), bias


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("m,bs,tokens,n", SWIGLU[1:3])
def test_swiglu_of_the_lone_outputs(pt2q, m, bs, tokens, n, dtype):
    _, lays, x_int = _members(pt2q, m, bs, tokens, (n, n), dtype)
    x = _x(x_int, dtype, 0.37)
    g, u = (_lone(pt2q, lay, x).float().cpu().numpy() for lay in lays)
    hs = [pt2q.ternary_skinny_swiglu(x, *lays) for _ in range(8)]
    assert _eq(hs[0], swiglu(g, u, dtype))
    assert all(torch.equal(h, hs[0]) for h in hs[1:])


def _raw(pt2q, x, lays, ys, epilogue, ws, ws_bytes, tokens=None):
    """The C entry on the layers' packed operands: its status, with the caller's outputs and workspace."""
    L = pt2q._lib
    arrs = [L.ptr_array([lay._packed[i] for lay in lays]) for i in range(5)] + [L.ptr_array(ys)]
    m = lays[0].in_features
    return L.lib().pt2q_ternary_skinny_group(
        L.ptr(x), L.dtype_code(x), x.shape[0] if tokens is None else tokens, m, m, len(lays),
        _ints([lay.out_features for lay in lays]), arrs[0][0], arrs[1][0], arrs[2][0], arrs[3][0],
        _ints([lay._packed[2].shape[1] for lay in lays]), lays[0].block_size, arrs[4][0], arrs[5][0],
        L.dtype_code(ys[0]), _ints([y.shape[1] for y in ys], ctypes.c_int64), epilogue, L.ptr(ws), ws_bytes,
        L.stream_of(x.device))


def test_workspace_hygiene(pt2q):
    m, bs, tokens, n = SWIGLU[2]
    cases, lays, x_int = _members(pt2q, m, bs, tokens, (n, n), "fp16")
    x = _x(x_int, "fp16")
    sizes = [pt2q._lib.lib().pt2q_ternary_skinny_group_workspace_bytes(tokens, m, 2, _ints([n, n]), e) for e in (0, 1)]
    ws = torch.full((max(sizes),), 0xFF, dtype=torch.uint8, device=x.device)
    g, u = (_want(c, x_int, False, True, "fp16") for c in cases)
    for _ in range(2):  # PLAIN then SWIGLU on one workspace: each finds the other's counters and partials
        ys = [torch.empty((tokens, n), dtype=torch.float16, device=x.device) for _ in range(2)]
        assert _raw(pt2q, x, lays, ys, 0, ws, sizes[0]) == 0
        assert _eq(ys[0], g) and _eq(ys[1], u)
        assert _raw(pt2q, x, lays, ys[:1], 1, ws, sizes[1]) == 0
        assert _eq(ys[0], swiglu(g, u, "fp16"))


@pytest.mark.parametrize("tokens,ns,epilogue,ydt,short,status", [
    (65, (40, 40), 0, torch.float16, 0, 3),       # PT2Q_E_UNSUPPORTED
    (64, (40, 40), 0, torch.float16, 1, 5),       # PT2Q_E_WORKSPACE: one byte short
    (64, (40,) * 5, 0, torch.float16, 0, 1),      # PT2Q_E_ARG from here on: count 5
    (64, (40,) * 3, 1, torch.float16, 0, 1),      # SWIGLU with count 3
    (64, (40, 33), 1, torch.float16, 0, 1),       # SWIGLU with n[0] != n[1]
    (64, (40, 40), 1, torch.float32, 0, 1),       # SWIGLU with f32 y
])
def test_refused_calls_leave_y_alone(pt2q, tokens, ns, epilogue, ydt, short, status):
    _, lays, x_int = _members(pt2q, 200, 64, 65, ns, "fp16")
    x = _x(x_int, "fp16")
    nbytes = pt2q._lib.lib().pt2q_ternary_skinny_group_workspace_bytes(64, 200, 2, _ints([40, 40]), 0)
    ws = torch.zeros(4 * nbytes, dtype=torch.uint8, device=x.device)
    ys = [torch.full((65, n), 7.0, dtype=ydt, device=x.device) for n in ns]
    assert _raw(pt2q, x, lays, ys, epilogue, ws, nbytes - 1 if short else 4 * nbytes, tokens) == status
    torch.cuda.synchronize()
    assert all(bool((y == 7.0).all()) for y in ys)


def test_module_routing(pt2q, monkeypatch):
    monkeypatch.setattr(pt2q.ternary, "skinny_max_tokens", 64)
    monkeypatch.setattr(pt2q.ternary, "skinny_mlp_max_tokens", 64)
    hid, inter, bs = 256, 130, 128
    gate, up, down = (_layer(pt2q, ref.exact_case(n, m, bs, 65, seed), "fp16", False)
                      for seed, (n, m) in enumerate(((inter, hid), (inter, hid), (hid, inter))))
    mlp = pt2q.TernaryGatedMLP(gate, up, down)
    x = _x(ref.exact_case(inter, hid, bs, 65, 9)["x_int"], "fp16", 0.37)

    def kids(v):
        return down(F.silu(gate(v)) * up(v))
    for tokens in (2, 64):
        assert torch.equal(mlp(x[:tokens]), _lone(pt2q, down, pt2q.ternary_skinny_swiglu(x[:tokens], gate, up)))
    assert torch.equal(mlp(x), kids(x))          # 65 tokens: past the cap
    assert torch.equal(mlp(x[:1]), kids(x[:1]))  # 1 token: unchanged
    up.decode = "mfma"
    assert torch.equal(mlp(x[:2]), kids(x[:2]))
