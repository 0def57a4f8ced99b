"""Ragged widths (m % 4 != 0) and row counts (n % 4 != 0) on the GPU, bit for bit against the CPU
oracle: the shapes of tests/ragged_cases.py, which tests/test_ragged_cases_cpu.py shows to reach the
launchers' fallbacks -- the four-lane Cholesky block step, gemmx's refusal and the non-vector chain
GEMMs on odd strides (ld = m, batch items m * m floats apart), the scalar damping pass, the
unfused w-bar kernels with the generic similarity kernel, the block loop without the EF kernel,
its w-bar hand-off or the 16-byte ATQ stage, the wide per-channel kernel on rows the streamed
kernel refuses, and GramsFirst steps that mix grouped, per-channel and lone loops.  No tolerances."""
import importlib

import numpy as np
import pytest
import torch

import ragged_cases as rc
import synth
from oracle import oracle as orc
from test_gpu_parity import bits_equal, cuda, host, oracle_gram

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ids(c):
    return "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


def _assert_layer(out, ref):
    np.testing.assert_array_equal(host(out.perm), ref["perm"])
    np.testing.assert_array_equal(host(out.T), ref["T"])
    assert bits_equal(host(out.alpha), ref["alpha"])
    assert bits_equal(host(out.mu), ref["mu"])
    np.testing.assert_array_equal(host(out.iters), ref["iters"])


def _same(a, b, what=None):
    for f in ("alpha", "mu", "T", "perm"):
        x, y = (a[f] if isinstance(a, dict) else getattr(a, f)), (b[f] if isinstance(b, dict) else getattr(b, f))
        assert bits_equal(host(x), host(y)), (what, f)


# ------------------------------------------------------------------ Hessian inverse

@pytest.mark.parametrize("m", rc.INVERSE_M)
def test_inverse_odd_width(pt2q, m):
    """prepare_hessian (scalar form) + cholesky_inverse with ld = m odd: 65 one whole block then a
    1-wide one; 130 / 323 the other residues; 257 a rank-256 sub-panel update with a 1-row target;
    1001 two 512-panels; 1537 the lauum's 84 upper tiles, which gemmx refuses."""
    orc.set_threads(16)
    G, N, (Hr, dr), (Hinv_r, spd_r) = rc.inverse_case(m)
    H, damp = pt2q.prepare_hessian(cuda(G), N, 0.01)
    assert bits_equal(host(H), Hr) and np.float32(host(damp)[0]) == np.float32(dr)
    Hinv, spd = pt2q.cholesky_inverse(H)
    assert spd and spd_r
    assert bits_equal(host(Hinv), Hinv_r)


@pytest.mark.parametrize("m,batch,chunk", rc.BATCHED_INVERSE)
def test_inverse_batched_odd_item_stride(pt2q, m, batch, chunk):
    """hessian_inverse_batched with items m * m floats apart (m odd: 4-byte aligned item bases;
    chunk 2 of 3 starts its second launch sequence at such a base): every positive definite item
    equals the per-item call and the oracle; the negated item reports its own pivot."""
    orc.set_threads(16)
    N = m + 50
    Gs = [rc.inverse_case(m)[0]] + [orc.gram(synth.activations(rc.case_seed(m, 8, z), N, m)) for z in range(1, batch)]
    Gs[1] = -Gs[1]  # damping a negative definite Gram: breakdown at the first pivot
    G = cuda(np.stack(Gs))
    Hinv, info = pt2q.engine.hessian_inverse_batched(G, N, 0.01, chunk=chunk)
    info = host(info)
    for z in range(batch):
        Hr, _ = orc.prepare_hessian(Gs[z], N, 0.01)
        if z == 1:
            assert info[z] == orc.cholesky_upper(Hr)[1] != 0
            continue
        assert info[z] == 0, (z, info[z])
        H, _ = pt2q.prepare_hessian(G[z], N, 0.01)
        want, spd = pt2q.cholesky_inverse(H)
        assert spd and bits_equal(host(Hinv[z]), host(want)), z
        want_r, spd_r = orc.cholesky_inverse(Hr)
        assert spd_r and bits_equal(host(Hinv[z]), want_r), z


# ------------------------------------------------------------------ Gram

@pytest.mark.parametrize("N,m,dt", rc.GRAM, ids=_ids)
def test_gram_odd_width(pt2q, N, m, dt):
    """m odd: 16-bit rows start on 2-byte boundaries (register-staged operands; 4101: the split
    persistent Gram), fp32 rows on 4-byte ones; then accumulate (gptq.py add_batch)."""
    orc.set_threads(16)
    Xd = rc.to_dtype(synth.activations(rc.case_seed(N, m, 9), N, m), dt).to(DEV)
    G = pt2q.gram(Xd)
    ref = oracle_gram(Xd)
    assert bits_equal(host(G), ref)
    G2 = pt2q.gram(Xd[: N // 2], G.clone(), accumulate=True)
    assert bits_equal(host(G2), ref + oracle_gram(Xd[: N // 2]))


# ------------------------------------------------------------------ SSR

@pytest.mark.parametrize("n,m,b", rc.SSR)
def test_ssr_ragged_rows(pt2q, n, m, b):
    """n % 4 != 0 (and n > 16384): w-bar by the partial kernel and sumfinal, or sum + final above
    12288 rows, then the generic similarity kernel; rem a proper subset in arbitrary order, W with
    exact ties (duplicated columns) and an all-zero column."""
    W, rem, sim_r, blk_r, newrem_r = rc.ssr_case(n, m, b)
    Wd, remd = cuda(W), cuda(rem)
    sim = pt2q.compute_column_similarity_to_mean(Wd, remd)
    assert bits_equal(host(sim), sim_r)
    blk, newrem = pt2q.select_next_block_ssr(Wd, remd, b)
    np.testing.assert_array_equal(host(blk), blk_r)
    np.testing.assert_array_equal(host(newrem), newrem_r)


# ------------------------------------------------------------------ error feedback entry

@pytest.mark.parametrize("n,m,bs", rc.EF)
def test_error_feedback_entry_odd_shapes(pt2q, n, m, bs):
    """pt2q_error_feedback with n, m odd: bs = 50 the EF kernel (coefficient rows padded to a
    multiple of 4), bs = 150 > 128 the generic GEMM with the row gather."""
    W, blk, rem, E, Hinv, ref = rc.ef_case(n, m, bs)
    Wd = cuda(W)
    pt2q.error_feedback(Wd, cuda(blk), cuda(rem), cuda(E), cuda(Hinv))
    assert bits_equal(host(Wd), ref)
    assert bits_equal(host(Wd)[:, blk], W[:, blk])


# ------------------------------------------------------------------ whole layers

@pytest.mark.parametrize("case", rc.LAYER_M + rc.LAYER_M_ROWS, ids=_ids)
def test_layer_m_ragged(pt2q, case):
    """quantize_layer (variant M) with m % 4 != 0 and n % 4 != 0: scalar damping, the odd-stride
    inverse, scalar transposes, unfused w-bar, no EF kernel (coefficient rows of m floats) and no
    w-bar hand-off, no 16-byte ATQ stage; 16-bit cases: 16-bit activations, the gram16 arithmetic.
    m = 384 with n = 203: the EF kernel without its w-bar hand-off, beside the unfused w-bar."""
    n, m, N, bs, ssr, dt = case
    orc.set_threads(16)
    W, X, ref = rc.layer_m_case(*case)
    out = pt2q.quantize_layer(W.to(DEV), X.to(DEV), block_size=bs, use_ssr=ssr)
    assert out.spd and ref["spd"]
    _assert_layer(out, ref)
    if case == rc.LAYER_M_F32_CODES:  # T requested as fp32: the code transpose's int8 -> f32 form
        outf = pt2q.quantize_layer(W.to(DEV), X.to(DEV), block_size=bs, use_ssr=ssr, t_dtype=torch.float32)
        assert outf.T.dtype == torch.float32
        _assert_layer(outf, ref)


@pytest.mark.parametrize("case", rc.PER_CHANNEL, ids=_ids)
def test_per_channel_wide_ragged(pt2q, case):
    """Per-channel (one block, m > 512) rows the streamed kernel refuses ((m * E) % 16 != 0): the
    wide kernel on the caller's row-major W (bf16 at m = 515: rows on 2-byte boundaries), as a
    whole layer and as the block loop with S1 / d formed here and given."""
    n, m, N, bs, dt = case
    orc.set_threads(16)
    W, X, ref = rc.layer_m_case(n, m, N, bs, True, dt)
    Wd, Xd = W.to(DEV), X.to(DEV)
    _assert_layer(pt2q.quantize_layer(Wd, Xd, block_size=bs, use_ssr=True), ref)
    G = pt2q.gram(Xd)
    _assert_layer(pt2q.quantize_blocks(Wd, G, None, bs, True), ref)
    s1d = pt2q.engine.s1_from_gram_batched(G[None])
    _assert_layer(pt2q.quantize_blocks(Wd, G, None, bs, True, s1d=s1d[0]), ref)


@pytest.mark.parametrize("case", rc.LAYER_G, ids=_ids)
def test_layer_g_ragged(pt2q, case):
    """Variant G (GPTQ.add_batch / quantize) at 67 x 203: bs = 64 with SSR; bs = 150: the H_bb
    product of blocks wider than 128 columns (150-wide, odd ld); bs = 203: one block."""
    n, m, N, bs, ssr = case
    W, X, ref = rc.layer_g_case(*case)
    lin = torch.nn.Linear(m, n, bias=False).to(DEV)
    lin.weight.data = cuda(W)
    gq = pt2q.GPTQ(lin, bs, 0.01)
    for c in np.array_split(X, 2):
        gq.add_batch(cuda(c))
    alpha, mu, T, perm = gq.quantize(use_ssr=ssr)
    assert ref["spd"]
    np.testing.assert_array_equal(host(perm), ref["perm"])
    np.testing.assert_array_equal(host(T), ref["T"])
    assert bits_equal(host(alpha), ref["alpha"]) and bits_equal(host(mu), ref["mu"])


def test_layer_graph_replay_ragged(pt2q):
    """The hipGraph-captured ragged layer replays to the eager result (and the oracle's)."""
    n, m, N, bs, ssr, dt = rc.GRAPH_LAYER
    W, X, ref = rc.layer_m_case(*rc.GRAPH_LAYER)
    Wd, Xd = W.to(DEV), X.to(DEV)
    eager = pt2q.quantize_layer(Wd, Xd, block_size=bs, use_ssr=ssr)
    lg = pt2q.LayerGraph(Wd, Xd, block_size=bs, use_ssr=ssr)
    out = lg.replay()
    torch.cuda.synchronize()
    assert lg.spd()
    _same(out, eager)
    assert bits_equal(host(out.iters), host(eager.iters))
    _assert_layer(out, ref)
    W2 = rc.to_dtype(synth.weights(rc.case_seed(n, m, 10), n, m), dt)  # new inputs in place
    Wd.copy_(W2.to(DEV))
    out = lg.replay()
    torch.cuda.synchronize()
    _same(out, pt2q.quantize_layer(Wd, Xd, block_size=bs, use_ssr=ssr))


# ------------------------------------------------------------------ GramsFirst with refused shapes

def _gf_units():
    units, data = [], {}
    for i, (m, dt, ns, N) in enumerate(rc.GF_UNITS):
        X = rc.to_dtype(synth.activations(rc.case_seed(N, m, 11, i), N, m), dt).to(DEV)
        Ws = {f"p{k}": rc.to_dtype(synth.weights(rc.case_seed(n, m, 12, i, k), n, m), dt).to(DEV)
              for k, n in enumerate(ns)}
        units.append((f"u{i}", [(f"p{k}", n, m) for k, n in enumerate(ns)], N))
        data[f"u{i}"] = (X, Ws)
    return units, data


_GF_WANT = {}


def _gf_want(pt2q, bs):
    """quantize_unit per unit, once per block size."""
    if bs not in _GF_WANT:
        units, data = _gf_units()
        _GF_WANT[bs] = {name: pt2q.quantize_unit([data[name][1][p] for p, _, _ in lins], data[name][0],
                                                 block_size=bs, use_ssr=True) for name, lins, _ in units}
    return _GF_WANT[bs]


@pytest.mark.parametrize("batched,group", rc.GF_MODES)
@pytest.mark.parametrize("bs", rc.GF_BLOCK_SIZES)
def test_grams_first_refused_shapes(pt2q, bs, batched, group):
    """quantize_units_sharded over units the batched / grouped entries refuse beside one they take:
    m = 333 (16-bit: per-item Grams; m % 4: lone loops), m = 512 (grouped at bs = 128), m = 515
    bf16 (bs = 1024: per-channel with S1 / d formed, never upper-only), m = 333 fp32.  Equal to
    quantize_unit per unit; a second step over the same slots equals the first."""
    sharding = importlib.import_module("pt2q.sharding")
    eng = pt2q.engine
    units, data = _gf_units()
    pipe = pt2q.UnitPipeline(DEV, bs, True, lanes=3)
    gf = sharding.GramsFirst(pipe, DEV, batched=batched, group=group)
    res, mine = sharding.quantize_units_sharded(units, lambda u: data[u[0]], block_size=bs, pack=False,
                                                grams_first=gf)
    # what each unit took: the helper's predicates agree with the engine's, and the step's state shows it
    for (m, dt, ns, N), (name, lins, _) in zip(rc.GF_UNITS, units):
        X = data[name][0]
        assert eng.gram_batched_supported(X) == rc.gram_batched_supported(dt, m) == (m == 512 or dt == "fp32")
        grp = gf.groups[(m, N)]
        assert (grp["Hinv"] is not None) == (batched and bs < m)
        assert (grp.get("S1d") is not None) == rc.gf_s1d(m, bs, batched) == (batched and bs == 1024 and m == 515)
        assert grp["upper"] == rc.gf_upper(m, bs, dt, batched) is False  # never upper-only here (515 % 4)
        for n in ns:
            assert eng.group_supported(n, m, bs) == rc.group_supported(n, m, bs) == (m == 512 and bs == 128)
    if gf.grouped:
        assert bool(gf.gws) == (bs == 128)                                  # the 512-wide unit's group
        assert any(k[0] != "pc" for k in gf.ows)                            # lone ("one") loops ran
        assert any(k[0] == "pc" for k in gf.ows) == (bs == 1024)            # the 515-wide per-channel group
    res2, _ = sharding.quantize_units_sharded(units, lambda u: data[u[0]], block_size=bs, pack=False,
                                              grams_first=gf)
    want = _gf_want(pt2q, bs)
    assert sorted(mine) == list(range(len(units)))
    for name, lins, _ in units:
        for (p, _, _), r in zip(lins, want[name]):
            _same(res[f"{name}.{p}"], r, (name, p))
            _same(res2[f"{name}.{p}"], res[f"{name}.{p}"], (name, p, "second step"))
