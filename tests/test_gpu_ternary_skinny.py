"""pt2q_ternary_skinny (csrc/ternary_skinny.hip: 16x16x32 MFMA, x through an LDS ring, the K-split
reduced inside the launch) for 2..64 tokens, through ternary_skinny and TernaryLinear(decode="skinny").

  1. exact GEMM   exactly summable data (tests/ternary_linear_ref.py): any split, order or tile must
                  give the integer reference's bits; no tolerance
  2. workspace    a workspace full of 0xFF bytes, and one a previous call left behind, change nothing;
                  problem A, problem B, A again through one workspace, each exact
  3. random data  against float64 within one ulp per accumulation step; eight calls, one result
  4. graph        a captured decode="skinny" call replayed on rewritten x equals the eager bits
  5. routing      which kernel a decode="skinny" module reaches for 1, 2, 64 and 65 tokens
  6. arguments    refused calls return their status and leave y alone

The shapes are tests/ternary_skinny_cases.py's: SHAPES for the ragged edges, the scale-block edges and
every NT, on K slices of 1..3 blocks; LONG and WIDE for slices of 4..7 blocks, which overwrite and lap
the 3-slot LDS ring, for 16 splits by the clamp, and for many feature tiles, where the split is the
workgroup target's and the partial tiles outgrow an XCD's L2.  test_ternary_skinny_cases_cpu.py holds
the tables to those plans."""
import numpy as np
import pytest
import torch

import stream_cases as sc
import ternary_linear_ref as ref
from ternary_skinny_cases import LONG, SHAPES, WIDE
from test_gpu_parity import cuda
from test_gpu_stream_order import cycles_per_ms, test_entry_on_a_delayed_stream as _delayed_stream  # noqa: F401

pytestmark = pytest.mark.gpu

# The stream-order case of the new entry (tests/stream_cases.py's table; appended from here, at
# collection, so the header-coverage test of a suite run finds it).  17 tokens: two token tiles
# and two K slices, so every call rewrites the tile counters and the partials.
TSN, TSM, TSTOK = 384, 512, 17
sc.case("ternary-skinny", "pt2q_ternary_skinny", lambda seed: sc.tern(seed, TSN, TSM, 128, TSTOK, sc.f16),
        lambda c: c.L.pt2q_ternary_skinny(c.p("x"), sc.F16, TSTOK, TSM, TSN, TSM, c.p("codes"), c.p("gather"),
                                          c.p("alpha"), c.p("mu"), TSM // 128, 128, c.p("bias"), c.p("y"), sc.F16, TSN,
                                          c.p("ws"), c.nbytes("ws"), c.st),
        ("y",), "test_gpu_ternary_skinny.py::test_exact_gemm", out={"y": ((TSTOK, TSN), sc.f16)},
        ws={"ws": lambda L: L.pt2q_ternary_skinny_workspace_bytes(TSTOK, TSN, TSM)}, index=sc.tern_index(TSM))
sc.BY_ID[sc.CASES[-1].id] = sc.CASES[-1]


def test_stream_order(pt2q, cycles_per_ms):  # noqa: F811
    """tests/test_gpu_stream_order.py's check (delayed side streams, decoy buffers) on the case above."""
    _delayed_stream(pt2q, cycles_per_ms, sc.CASES[-1])

TDT = {"fp16": torch.float16, "bf16": torch.bfloat16}
GUARD = 64  # fp32 elements of NaN before and after a guarded array


def _layer(pt2q, c, dtype, compat, decode="skinny"):
    lay = pt2q.TernaryLinear(c["m"], c["n"], c["bs"], bias=True, dtype=TDT[dtype], compat=compat, decode=decode)
    lay.set_quantized_params(cuda(c["alpha"]), cuda(c["mu"]), cuda(c["T"]), cuda(c["perm"]), cuda(c["bias"]))
    lay._prepare()
    return lay


def _guarded(t):
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), dtype=torch.float32, device=t.device)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _skinny(pt2q, lay, x, ydt, bias):
    codes, gather, a32, m32, b32 = lay._packed
    return pt2q.ternary_skinny(x, codes, gather, a32, m32, lay.block_size, b32 if bias else None, out_dtype=ydt)


def _raw(pt2q, lay, x, y, ws, ws_bytes, tokens=None):
    """The C entry on the layer's packed operands: its status, with the caller's y and workspace."""
    L = pt2q._lib
    codes, gather, a32, m32, b32 = lay._packed
    n, m = lay.out_features, lay.in_features
    return L.lib().pt2q_ternary_skinny(
        L.ptr(x), L.dtype_code(x), x.shape[0] if tokens is None else tokens, m, n, m, L.ptr(codes), L.ptr(gather),
        L.ptr(a32), L.ptr(m32), a32.shape[1], lay.block_size, L.ptr(b32), L.ptr(y), L.dtype_code(y), n, L.ptr(ws),
        ws_bytes, L.stream_of(x.device))


def _same(y, want):
    got = y.float().cpu()
    return torch.equal(got, torch.from_numpy(want)) and bool(torch.isfinite(got).all())


def _case(n, m, bs, tokens, compat16, dtype):
    compat = compat16 if dtype == "fp16" else not compat16
    return ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens)), compat


def _exact_gemm(pt2q, monkeypatch, n, m, bs, tokens, compat16, dtype):
    monkeypatch.setattr(pt2q.ternary, "skinny_max_tokens", 64)
    c, compat = _case(n, m, bs, tokens, compat16, dtype)
    lay = _layer(pt2q, c, dtype, compat)
    if (n, m) == (40, 2100):  # scales and bias inside NaN-filled buffers: nothing past an array reaches y
        codes, gather, a32, m32, b32 = lay._packed
        lay._packed = (codes, gather, _guarded(a32), _guarded(m32), _guarded(b32))
    x = cuda(c["x"]).to(TDT[dtype])
    assert _same(lay(x), ref.exact_reference(c, compat, True, dtype))
    for bias in (True, False):
        assert _same(_skinny(pt2q, lay, x, TDT[dtype], bias), ref.exact_reference(c, compat, bias, dtype)), bias
        assert _same(_skinny(pt2q, lay, x, torch.float32, bias), ref.exact_reference(c, compat, bias)), bias


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("n,m,bs,tokens,compat16", SHAPES + LONG)
def test_exact_gemm(pt2q, monkeypatch, n, m, bs, tokens, compat16, dtype):
    _exact_gemm(pt2q, monkeypatch, n, m, bs, tokens, compat16, dtype)


@pytest.mark.parametrize("n,m,bs,tokens,compat16,dtype", WIDE)
def test_exact_gemm_many_tiles(pt2q, monkeypatch, n, m, bs, tokens, compat16, dtype):
    """256, 171 and 512 feature tiles: 2 and 3 splits because the workgroup target asks for no more
    (4-block slices, 6 MiB of partial tiles at the first), and the direct store after a 7-block slice."""
    _exact_gemm(pt2q, monkeypatch, n, m, bs, tokens, compat16, dtype)


@pytest.mark.parametrize("shape", [SHAPES[5], SHAPES[4]])
def test_workspace_hygiene(pt2q, shape):
    c, compat = _case(*shape, "fp16")
    lay = _layer(pt2q, c, "fp16", compat)
    x = cuda(c["x"]).half()
    nbytes = pt2q._lib.lib().pt2q_ternary_skinny_workspace_bytes(c["tokens"], c["n"], c["m"])
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=x.device)
    want = ref.exact_reference(c, compat, True)
    for _ in range(2):  # the second call finds the first one's counters and partials
        y = torch.empty((c["tokens"], c["n"]), dtype=torch.float32, device=x.device)
        assert _raw(pt2q, lay, x, y, ws, nbytes) == 0
        assert _same(y, want)


@pytest.mark.parametrize("shape,dtype", [(LONG[3], "fp16"), (WIDE[0][:5], WIDE[0][5])])
def test_workspace_reuse_across_problems(pt2q, shape, dtype):
    """A, B, A through one workspace, B the same shapes from another seed (the decoy rule of DESIGN.md
    §6.4: valid operands everywhere, no poison).  A call that reads a partial tile, a counter or an
    x_sel row its own launches have not written yet finds the other problem's, and its bits are wrong.
    Seven-block slices with 16 partials per tile, and the 6 MiB of partials of 256 tiles."""
    n, m, bs, tokens = shape[:4]
    a, compat = _case(*shape, dtype)
    b = ref.exact_case(n, m, bs, tokens, a["seed"] + 1)
    lays = [_layer(pt2q, c, dtype, compat) for c in (a, b)]
    wants = [ref.exact_reference(c, compat, True) for c in (a, b)]
    assert (wants[0] != wants[1]).mean() > 0.9
    nbytes = pt2q._lib.lib().pt2q_ternary_skinny_workspace_bytes(tokens, n, m)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    for k in (0, 1, 0):
        x = cuda([a, b][k]["x"]).to(TDT[dtype])
        y = torch.empty((tokens, n), dtype=torch.float32, device=x.device)
        assert _raw(pt2q, lays[k], x, y, ws, nbytes) == 0
        assert _same(y, wants[k]), k


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("n,m,bs,tokens", [(130, 2100, 128, 33), (65, 640, 192, 17), (65, 13824, 128, 33),
                                           (16321, 1024, 128, 48)])
def test_random_against_float64(pt2q, n, m, bs, tokens, dtype):
    """Scales in the range of real layers, x ~ N(0, 1) in TX.  The bound allows one unit in the last
    place (2^-24 relative, doubled to 2^-23 for the rounding of the sum itself) per accumulation
    step in any order: m products, up to 16 partials, the bias, against the sum of magnitudes."""
    rng = np.random.default_rng(n + m)
    B = ref.nblocks(m, bs)
    c = {"n": n, "m": m, "bs": bs, "T": rng.integers(-1, 2, size=(n, m)).astype(np.int8),
         "alpha": ref.round16(rng.random((n, B)) * 0.05 + 0.005, dtype),
         "mu": ref.round16(rng.standard_normal((n, B)) * 0.002, dtype),
         "perm": rng.permutation(m).astype(np.int64), "bias": ref.round16(rng.standard_normal(n) * 0.1, dtype)}
    x = ref.round16(rng.standard_normal((tokens, m)), dtype)
    W = ref.weight_tx(c["alpha"], c["mu"], c["T"], c["perm"], bs, False, dtype).astype(np.float64)
    want = x.astype(np.float64) @ W.T + c["bias"]
    bound = (m + 18) * 2.0 ** -23 * (np.abs(x).astype(np.float64) @ np.abs(W).T + np.abs(c["bias"]))
    lay = _layer(pt2q, c, dtype, False)
    xd = cuda(x).to(TDT[dtype])
    ys = [_skinny(pt2q, lay, xd, torch.float32, True) for _ in range(8)]
    err = np.abs(ys[0].cpu().numpy().astype(np.float64) - want)
    print(f"max err / bound = {(err / bound).max():.3e}")
    assert (err <= bound).all()
    assert all(torch.equal(y, ys[0]) for y in ys[1:])


def test_graph_replay(pt2q, monkeypatch):
    """One decode="skinny" layer call (gather, then the GEMM with its tickets: 16 splits of 7 blocks,
    NT 4) captured once and replayed on three x written into the captured buffer: the eager bits."""
    monkeypatch.setattr(pt2q.ternary, "skinny_max_tokens", 64)
    c, compat = _case(*LONG[3], "fp16")
    lay = _layer(pt2q, c, "fp16", compat)
    xs = [(cuda(c["x"]) * s).half() for s in (0.37, 0.61, 1.0)]
    eager = [lay(x).clone() for x in xs]
    assert _same(eager[2], ref.exact_reference(c, compat, True, "fp16"))
    assert not torch.equal(eager[0], eager[1])
    xg = torch.zeros_like(xs[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yg = lay(xg)
    for x, want in zip(xs, eager):
        xg.copy_(x)
        graph.replay()
        assert torch.equal(yg, want)


def test_routing(pt2q, monkeypatch):
    monkeypatch.setattr(pt2q.ternary, "skinny_max_tokens", 64)
    n, m, bs = 130, 640, 128
    c = ref.exact_case(n, m, bs, 65, 7)
    lays = {mode: _layer(pt2q, c, "fp16", False, mode) for mode in ("skinny", "fused", "mfma")}
    x = (cuda(c["x"]) * 0.37).half()  # not exactly summable: the paths differ in the last bits
    for tokens in (2, 64):
        assert torch.equal(lays["skinny"](x[:tokens]), _skinny(pt2q, lays["skinny"], x[:tokens], torch.float16, True))
    assert torch.equal(lays["skinny"](x[:1]), lays["fused"](x[:1]))
    assert torch.equal(lays["skinny"](x), lays["mfma"](x))
    assert lays["skinny"](x[:0]).shape == (0, n)
    assert pt2q.set_decode(torch.nn.Sequential(lays["mfma"]), "skinny")[0].decode == "skinny"
    with pytest.raises(ValueError):
        pt2q.TernaryLinear(m, n, bs, decode="bogus")


def test_refused_calls_leave_y_alone(pt2q):
    L = pt2q._lib
    c = ref.exact_case(40, 200, 64, 65, 3)
    lay = _layer(pt2q, c, "fp16", False)
    x = cuda(c["x"]).half()
    assert L.lib().pt2q_ternary_skinny_max_tokens() == 64
    nbytes = L.lib().pt2q_ternary_skinny_workspace_bytes(64, 40, 200)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
    for tokens, ydt, wsb, status in ((65, torch.float16, nbytes, 3),      # PT2Q_E_UNSUPPORTED
                                     (64, torch.float16, nbytes - 1, 5),  # PT2Q_E_WORKSPACE
                                     (64, torch.bfloat16, nbytes, 1)):    # PT2Q_E_ARG
        y = torch.full((65, 40), 7.0, dtype=ydt, device=x.device)
        assert _raw(pt2q, lay, x, y, ws, wsb, tokens) == status
        torch.cuda.synchronize()
        assert bool((y == 7.0).all())
