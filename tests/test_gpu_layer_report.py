"""pt2q_layer_report / pt2q_quadform_rows on the GPU against the numpy / oracle restatement of the
contract (tests/report_ref.py, DESIGN.md §3 "Layer report"): ew, ex, ey and totals are BIT-EQUAL to
it in every case; the comparisons with float64 values and with the reference's recorded numbers use
the derived bound (report_ref.error_bound)."""
import copy
import functools
import importlib

import numpy as np
import pytest
import torch

import report_ref as rr
from conftest import layer_inputs, load_golden, round16
from oracle import oracle as orc
from test_gpu_strides import Pad, ins_ok, outs_ok, vec

pytestmark = pytest.mark.gpu

DEV = "cuda"
REF = 0x1
# (n, m, b): one element; inside one tile; one past the 128 / 256 tile edges with a ragged last
# block and chunk; ragged everything; one block (B = 1) twice; several K stages plus a ragged one
CASES = [(1, 1, 128), (33, 31, 128), (130, 257, 128), (100, 300, 128), (64, 512, 512), (300, 640, 640),
         (260, 1100, 128)]
SMALL = CASES[1:4]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def case(n, m, b, wdtype="fp32", with_perm=True):
    """Random inputs and their restated report (computed once per case, shared, never modified)."""
    rng = np.random.default_rng(1000 * n + m + (7 if wdtype != "fp32" else 0) + (0 if with_perm else 3))
    W = rng.standard_normal((n, m)).astype(np.float32)
    if wdtype != "fp32":
        W = round16(W, wdtype)
    B = -(-m // b) if b < m else 1
    alpha = (0.5 + rng.random((n, B))).astype(np.float32)
    mu = (0.1 * rng.standard_normal((n, B))).astype(np.float32)
    T = rng.integers(-1, 2, (n, m)).astype(np.int8)
    perm = rng.permutation(m).astype(np.int64) if with_perm else None
    G = rng.standard_normal((m, m)).astype(np.float32)  # read as stored: no symmetry is assumed
    ref = rr.report(W, alpha, mu, T, b, perm, G, reference=True)
    for v in (W, alpha, mu, T, G) + ((perm,) if with_perm else ()):
        v.setflags(write=False)
    return dict(W=W, alpha=alpha, mu=mu, T=T, perm=perm, G=G, ref=ref, b=b)


def torch_w(W, wdtype):
    t = torch.from_numpy(np.array(W))
    return {"fp32": t, "fp16": t.half(), "bf16": t.bfloat16()}[wdtype].to(DEV)


def run_report(pt2q, c, wdtype="fp32", t_float=False, flags=REF, use_g=True):
    """pt2q_layer_report through the C ABI on contiguous device tensors -> host arrays."""
    lib, L = pt2q._lib, pt2q._lib.lib()
    W = torch_w(c["W"], wdtype)
    n, m = W.shape
    T = torch.from_numpy(np.array(c["T"])).to(DEV)
    T = T.float() if t_float else T
    alpha, mu = (torch.from_numpy(np.array(c[k])).to(DEV) for k in ("alpha", "mu"))
    perm = torch.from_numpy(np.array(c["perm"])).to(DEV) if c["perm"] is not None else None
    G = torch.from_numpy(np.array(c["G"])).to(DEV) if use_g else None
    out = torch.full((3, n), float("nan"), device=DEV)
    totals = torch.full((3,), float("nan"), device=DEV)
    ws = lib.workspace(L.pt2q_layer_report_workspace_bytes(n, m, flags), DEV)
    rc = L.pt2q_layer_report(lib.ptr(W), lib.dtype_code(W), m, n, m, c["b"], lib.ptr(alpha), lib.ptr(mu), lib.ptr(T),
                             lib.dtype_code(T), m, lib.ptr(perm), lib.ptr(G), m, flags, lib.ptr(out[0]),
                             lib.ptr(out[1]), lib.ptr(out[2]), lib.ptr(totals), lib.ptr(ws), ws.numel(),
                             lib.stream_of(torch.device(DEV)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert int(lib.status_view(ws).item()) == 0
    o = out.cpu().numpy()
    return o[0], o[1], o[2], totals.cpu().numpy()


def check_against(ref, got, ex=True, ey=True):
    ew_, ex_, ey_, tot = got
    assert same_bits(ew_, ref["ew"])
    want = [ref["totals"][0], np.float32(0), np.float32(0)]
    if ex:
        assert same_bits(ex_, ref["ex"])
        want[1] = ref["totals"][1]
    else:
        assert np.isnan(ex_).all()  # not computed: left alone
    if ey:
        assert same_bits(ey_, ref["ey"])
        want[2] = ref["totals"][2]
    else:
        assert np.isnan(ey_).all()
    assert same_bits(tot, np.array(want, np.float32))


@pytest.mark.parametrize("n,m,b", CASES)
def test_random_cases_bit_equal(pt2q, n, m, b):
    """W fp32 with a random perm: int8 and fp32 codes, PT2Q_REPORT_REF on and off, G = NULL."""
    c = case(n, m, b)
    check_against(c["ref"], run_report(pt2q, c))
    check_against(c["ref"], run_report(pt2q, c, t_float=True))
    check_against(c["ref"], run_report(pt2q, c, flags=0), ey=False)
    check_against(c["ref"], run_report(pt2q, c, use_g=False), ex=False, ey=False)


@pytest.mark.parametrize("n,m,b", SMALL)
@pytest.mark.parametrize("wdtype", ["fp16", "bf16"])
def test_16bit_weights_bit_equal(pt2q, n, m, b, wdtype):
    c = case(n, m, b, wdtype)
    check_against(c["ref"], run_report(pt2q, c, wdtype))


@pytest.mark.parametrize("n,m,b", SMALL)
def test_null_perm_is_identity(pt2q, n, m, b):
    c = case(n, m, b, with_perm=False)
    check_against(c["ref"], run_report(pt2q, c))


@pytest.mark.parametrize("n,m,b,ldw,ldt,ldg,lead", [
    (130, 257, 128, 259, 261, 263, 0),   # odd leading dimensions
    (130, 257, 128, 260, 264, 260, 1),   # 16-byte leading dimensions, every base one element off
    (130, 257, 128, 259, 261, 263, 1),   # both
    (100, 300, 128, 301, 303, 304, 0),   # G padded but 16-byte addressable: its 16-byte DMA path
])
def test_padded_and_offset_operands(pt2q, n, m, b, ldw, ldt, ldg, lead):
    """ldw, ldt, ldg padded (odd or not) and / or every base offset by one element (a G that is
    not 16-byte addressable takes the 4-byte DMA path; W / T the scalar loads they always use):
    results bit-equal, sentinel pads and guards of the outputs intact, inputs unchanged."""
    c = case(n, m, b)
    lib, L = pt2q._lib, pt2q._lib.lib()
    f32, i8 = torch.float32, torch.int8
    W = Pad((n, m), ldw, f32, np.array(c["W"]), lead=lead)
    T = Pad((n, m), ldt, i8, np.array(c["T"]), lead=lead)
    G = Pad((m, m), ldg, f32, np.array(c["G"]), lead=lead)
    B = c["alpha"].shape[1]
    alpha, mu = Pad((n, B), B, f32, np.array(c["alpha"])), Pad((n, B), B, f32, np.array(c["mu"]))
    perm = vec(m, torch.int64, np.array(c["perm"]))
    ew, ex, ey = (vec(n, f32, out=True, lead=lead) for _ in range(3))
    tot = vec(3, f32, out=True, lead=lead)
    ws = lib.workspace(L.pt2q_layer_report_workspace_bytes(n, m, REF), DEV)
    rc = L.pt2q_layer_report(W.p, 0, ldw, n, m, b, alpha.p, mu.p, T.p, 3, ldt, perm.p, G.p, ldg, REF, ew.p, ex.p,
                             ey.p, tot.p, lib.ptr(ws), ws.numel(), lib.stream_of(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    ref = c["ref"]
    assert same_bits(ew.win()[0], ref["ew"]) and same_bits(ex.win()[0], ref["ex"])
    assert same_bits(ey.win()[0], ref["ey"]) and same_bits(tot.win()[0], ref["totals"])
    assert outs_ok(ew, ex, ey, tot)
    assert ins_ok(W, T, G, alpha, mu, perm)
    # pt2q_quadform_rows on the same padded W and G
    q, t1 = vec(n, f32, out=True, lead=lead), vec(1, f32, out=True, lead=lead)
    ws = lib.workspace(L.pt2q_quadform_rows_workspace_bytes(n, m), DEV)
    rc = L.pt2q_quadform_rows(W.p, 0, ldw, n, m, G.p, ldg, q.p, t1.p, lib.ptr(ws), ws.numel(),
                              lib.stream_of(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    assert same_bits(q.win()[0], ref["ey"]) and same_bits(t1.win()[0], ref["totals"][2:3])
    assert outs_ok(q, t1) and ins_ok(W, G)


def test_real_layer(pt2q):
    """engine.quantize_layer on layer_m_384x300_n200 (SSR perm, ragged last block), then the report
    from its outputs and its Gram: bit-equal to the restatement; relative_output_error in (0, 1);
    output_error within the derived bound of the float64 ‖(W - Ŵ) Xᵀ‖² formed from X itself -- the
    bound of the f32 D and G plus the f32 Gram's own gamma_N: N 2^-23 Σ_i |d_i| (|X|ᵀ|X|) |d_i|ᵀ."""
    g = load_golden("layer_m_384x300_n200")
    W, X = layer_inputs(g)
    Wd, Xd = torch.from_numpy(W).to(DEV), torch.from_numpy(X).to(DEV)
    out = pt2q.quantize_layer(Wd, Xd)
    G = pt2q.gram(Xd)
    rep = pt2q.layer_report(Wd, out, G, 128)
    alpha, mu, T, perm = (t.cpu().numpy() for t in (out.alpha, out.mu, out.T, out.perm))
    assert not np.array_equal(perm, np.arange(len(perm)))
    ref = rr.report(W, alpha, mu, T, 128, perm, G.cpu().numpy())
    for k in ("ew", "ex", "ey"):
        assert same_bits(getattr(rep, k).cpu().numpy(), ref[k]), k
    assert same_bits(rep.totals.cpu().numpy(), ref["totals"])
    assert rep.weight_error == float(ref["totals"][0]) and rep.output_error == float(ref["totals"][1])
    assert rep.reference_energy == float(ref["totals"][2])
    assert 0.0 < rep.relative_output_error < 1.0
    assert rep.relative_output_error == rep.output_error / rep.reference_energy
    D64, X64 = ref["D"].astype(np.float64), X.astype(np.float64)
    exact = float(((D64 @ X64.T) ** 2).sum())
    aD, aX = np.abs(D64), np.abs(X64)
    bound = rr.error_bound(ref["D"], G.cpu().numpy()) + X.shape[0] * 2.0 ** -23 * float(((aD @ aX.T) ** 2).sum())
    print(f"output_error {rep.output_error!r} exact {exact!r} bound {bound:.3e}")
    assert abs(rep.output_error - exact) <= bound
    # a tuple in place of the LayerOutput, and no reference energy
    rep2 = pt2q.layer_report(Wd, (out.alpha, out.mu, out.T, out.perm), G, 128, reference=False)
    assert rep2.ey is None and rep2.relative_output_error is None and rep2.output_error == rep.output_error


def test_examples_atq_public_calls(pt2q):
    """compute_output_error_from_gram (CPU tensors in, a float out) against the reference's two
    recorded numbers and against compute_output_error(W, W_c, X) (the torch path on X), each within
    the derived bound."""
    g = load_golden("examples_atq")
    W, X = g["W"], g["X"].reshape(-1, g["X"].shape[-1])
    a0, m0, T0 = orc.ternary_init(W)
    a1, m1, T1, _ = orc.iterative_ternary_fitting(W, a0, m0, T0)
    a2, m2 = orc.activation_aware_grid_alignment(W, T1, X)
    Wt, Xt = torch.from_numpy(W), torch.from_numpy(X)
    G = pt2q.gram(Xt.to(DEV)).cpu()
    assert same_bits(G.numpy(), orc.gram(X))
    for (a, mu), key in (((a1, m1), "out_err_itf"), ((a2, m2), "out_err_aga")):
        Wc = a * T1 + mu
        got = pt2q.compute_output_error_from_gram(Wt, torch.from_numpy(Wc), G)
        D = W - Wc
        assert got == float(rr.rowtree(rr.quadform(D, G.numpy())))  # the contract's bits
        bound = rr.error_bound(D, G.numpy())
        via_x = pt2q.compute_output_error(Wt, torch.from_numpy(Wc), Xt)
        print(f"{key}: from Gram {got!r} via X {via_x!r} recorded {float(g[key])!r} bound {bound:.3e}")
        assert abs(got - float(g[key])) <= 2 * bound
        assert abs(got - via_x) <= 2 * bound


def test_special_values_and_geometry(pt2q):
    n, m, b = 130, 257, 128
    c = dict(case(n, m, b))
    W, G = np.array(c["W"]), np.array(c["G"])
    W[5] = rr.dequantized(c["alpha"], c["mu"], c["T"], b, c["perm"])[5]  # a zero residual row
    G[9, :] = 0.0
    G[:, 9] = 0.0
    c.update(W=W, G=G, ref=rr.report(W, c["alpha"], c["mu"], c["T"], b, c["perm"], G))
    got = run_report(pt2q, c)
    check_against(c["ref"], got)
    assert got[0][5] == 0.0 and got[1][5] == 0.0 and got[2][5] != 0.0
    again = run_report(pt2q, c)
    assert all(same_bits(x, y) for x, y in zip(got, again))  # run to run
    # the first 64 rows alone: the tree does not depend on n or on the grid
    c64 = dict(c, W=W[:64], alpha=c["alpha"][:64], mu=c["mu"][:64], T=c["T"][:64])
    part = run_report(pt2q, c64)
    for k in range(3):
        assert same_bits(part[k], got[k][:64])
    # quadform_rows(W, G) is the report's ey
    q = pt2q.engine.quadform_rows(torch.from_numpy(W).to(DEV), torch.from_numpy(G).to(DEV))
    assert same_bits(q.cpu().numpy(), got[2])
    assert same_bits(pt2q.quadform_rows(torch.from_numpy(W), torch.from_numpy(G)).numpy(), got[2])


class Decoderish(torch.nn.Module):
    """A decoder-like module: q/k/v read one tensor, gate/up another, o and down their own."""

    def __init__(self, d=256, inter=384):
        super().__init__()
        lin = torch.nn.Linear
        self.q, self.k, self.v, self.o = (lin(d, d, bias=False) for _ in range(4))
        self.gate, self.up, self.down = lin(d, inter, bias=False), lin(d, inter, bias=False), lin(inter, d, bias=False)

    def forward(self, x):
        h = x + self.o(torch.tanh(self.q(x)) * self.k(x) + self.v(x))
        return h + self.down(torch.nn.functional.silu(self.gate(h)) * self.up(h))


@pytest.mark.parametrize("schedule", ["grams-first", "lanes"])
def test_model_loop_reports(pt2q, schedule):
    """quantize_decoder_layer with the report on and off: params and written-back weights are
    bit-identical, and every linear's report equals a stand-alone layer_report on its original
    weight, its fp32 grids and the Gram of its group's concatenated inputs."""
    eng = pt2q.engine
    sharding = importlib.import_module(pt2q.__name__ + ".sharding")
    torch.manual_seed(3)
    base = Decoderish().to(DEV)
    samples = [torch.randn(40, 256, device=DEV) for _ in range(3)]
    dev = torch.device(DEV, torch.cuda.current_device())

    def run(report):
        layer = copy.deepcopy(base)
        pipe = eng.UnitPipeline(dev, 128, True, 0.01)
        gf = sharding.GramsFirst(pipe, dev) if schedule == "grams-first" else None

        def fwd(cap):
            for s in samples:
                layer(s)
                cap.next_pass()
        res = pt2q.quantize_decoder_layer(layer, fwd, 128, True, 0.01, 0, "correct", dev,
                                          None if gf is not None else pipe, gf, report=report)
        return layer, res

    l0, r0 = run(None)
    reports = {}
    l1, r1 = run(reports)
    assert sorted(r0) == sorted(r1) and len(r1) == 7
    for name in r0:
        for k in ("alpha", "mu", "T", "perm"):
            assert torch.equal(r0[name][k], r1[name][k]), (name, k)
    for (k0, p0), (k1, p1) in zip(l0.state_dict().items(), l1.state_dict().items()):
        assert k0 == k1 and torch.equal(p0, p1), k0
    # the groups' inputs on the original weights
    inputs = {}
    hooks = [mod.register_forward_hook(lambda md, inp, out, nm=nm: inputs.setdefault(nm, []).append(inp[0].detach()))
             for nm, mod in base.named_children()]
    with torch.no_grad():
        for s in samples:
            base(s)
    for h in hooks:
        h.remove()
    assert sorted(reports) == sorted(r1)
    for nm, mod in base.named_children():
        X = torch.cat(inputs[nm])
        p = r1[f"layer_0.{nm}"]
        alone = pt2q.layer_report(mod.weight.data, (p["alpha"], p["mu"], p["T"], p["perm"]), pt2q.gram(X), 128)
        assert reports[f"layer_0.{nm}"] == alone.as_dict(X.shape[0]), nm
        assert 0.0 < reports[f"layer_0.{nm}"]["relative_output_error"] < 1.0


def test_unit_and_gptq_reports(pt2q):
    """quantize_unit(report=True) attaches to each output the stand-alone report on the unit's
    Gram and changes no output; GPTQ.error_report() reports against the object's raw Σ XᵀX."""
    torch.manual_seed(11)
    X = torch.randn(200, 256, device=DEV)
    Ws = [torch.randn(96, 256, device=DEV), torch.randn(64, 256, device=DEV)]
    plain = pt2q.quantize_unit(Ws, X)
    outs = pt2q.quantize_unit(Ws, X, report=True)
    G = pt2q.gram(X)
    for W, o, p in zip(Ws, outs, plain):
        assert p.report is None
        for k in ("alpha", "mu", "T", "perm"):
            assert torch.equal(getattr(o, k), getattr(p, k)), k
        alone = pt2q.layer_report(W, o, G, 128)
        assert o.report.as_dict() == alone.as_dict() and 0.0 < o.report.relative_output_error < 1.0
    with pytest.raises(ValueError):
        pt2q.quantize_unit(Ws, X, report=True, defer=True)
    lin = torch.nn.Linear(256, 96, bias=False).to(DEV)
    q = pt2q.GPTQ(lin, block_size=128)
    with pytest.raises(RuntimeError):
        q.error_report()
    q.add_batch(X[:120])
    q.add_batch(X[120:])
    alpha, mu, T, perm = q.quantize()
    rep = q.error_report()
    D = (lin.weight.data - q.get_quantized_weight()).double()
    exact = float(((D @ X.double().T) ** 2).sum())
    Dn = D.float().cpu().numpy()
    bound = rr.error_bound(Dn, q.H.cpu().numpy()) + 2 * X.shape[0] * 2.0 ** -23 * float(
        ((D.abs() @ X.double().abs().T) ** 2).sum())  # + the accumulated Gram's own rounding
    assert abs(rep.output_error - exact) <= bound
    assert rep.weight_error == pytest.approx(float((D ** 2).sum()), rel=1e-5)
    assert 0.0 < rep.relative_output_error < 1.0


class TinyLM(torch.nn.Module):
    """Embedding + two decoder-like layers under .model.layers (the llama layout)."""

    def __init__(self):
        super().__init__()
        self.model = torch.nn.Module()
        self.model.embed = torch.nn.Embedding(64, 256)
        self.model.layers = torch.nn.ModuleList([Decoderish(), Decoderish()])

    def forward(self, ids, use_cache=False):
        x = self.model.embed(ids)
        for layer in self.model.layers:
            x = layer(x)
        return x


def test_model_quantizer_reports(pt2q):
    """PT2LLMQuantizer.quantize(report=True) fills layer_reports for every linear (host floats,
    nsamples = captured rows) and returns what report=False returns."""
    torch.manual_seed(5)
    base = TinyLM().to(DEV)
    samples = [torch.randint(0, 64, (1, 48)) for _ in range(3)]
    got = {}
    for rep in (False, True):
        q = pt2q.PT2LLMQuantizer(copy.deepcopy(base), None, "llama", block_size=128)
        got[rep] = (q.quantize(samples, writeback="correct", report=rep), q.layer_reports)
    res0, reps0 = got[False]
    res1, reps1 = got[True]
    assert reps0 == {} and sorted(reps1) == sorted(res1) and len(res1) == 14
    for name in res0:
        for k in ("alpha", "mu", "T", "perm"):
            assert torch.equal(res0[name][k], res1[name][k]), (name, k)
        r = reps1[name]
        assert r["nsamples"] == 3 * 48 and all(isinstance(r[k], float) for k in r if k != "nsamples")
        assert r["weight_error"] > 0 and 0.0 < r["relative_output_error"] < 1.0
        assert r["relative_output_error"] == r["output_error"] / r["reference_energy"]
