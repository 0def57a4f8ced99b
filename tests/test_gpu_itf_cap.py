"""The ITF iteration cap (max_iter, quantizer.py:25,162) on the GPU, bit for bit against the CPU oracle:
the cases of tests/itf_cap_cases.py, which tests/test_itf_cap_cases_cpu.py shows to bite (every cap
below a case's natural count k changes the oracle's bits, and at the cap some waves have stopped on
their own while others are cut).  Each case runs at the caps {0, 1, 2, 3, k - 1, k, k + 1} through
the three device loops -- row_itf (the narrow stage and block kernels), wide_itf (the wide stage and
block kernels) and pc_rows (the streamed and register-resident per-channel kernels) -- with the
iteration counts they reduce (iters_part + atq_finish_kernel, atomicMax) and the all-zero-block
repair beside capped neighbours; then max_iter through the fused layer, its captured graph, and the
Python plumbing that carries it.  No tolerances."""
import importlib

import numpy as np
import pytest
import torch

import itf_cap_cases as ic
import ragged_cases as rc
import synth
from oracle import oracle as orc
from test_gpu_parity import bits_equal, cuda, host

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_ARG = 1


def _ids(c):
    return "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


def _assert_atq(got, ref, what):
    """(alpha, mu, T) of the class surface against the oracle's (alpha, mu, T, iters)."""
    a, m, T = got
    assert np.array_equal(host(T), ref[2]), what
    assert bits_equal(host(a), ref[0]) and bits_equal(host(m), ref[1]), what


def _assert_layer(out, ref, what=None):
    np.testing.assert_array_equal(host(out.perm), ref["perm"], err_msg=str(what))
    np.testing.assert_array_equal(host(out.T), ref["T"], err_msg=str(what))
    assert bits_equal(host(out.alpha), ref["alpha"]), what
    assert bits_equal(host(out.mu), ref["mu"]), what
    np.testing.assert_array_equal(host(out.iters), ref["iters"], err_msg=str(what))


def _assert_pc(out, ref, what):
    """A one-block LayerOutput against the oracle's (alpha, mu, T, iters)."""
    a, mu, T, it = ref
    assert np.array_equal(host(out.T).astype(np.float32), T), what
    assert bits_equal(host(out.alpha), a) and bits_equal(host(out.mu), mu), what
    assert host(out.iters).tolist() == [it], (what, host(out.iters), it)
    np.testing.assert_array_equal(host(out.perm), np.arange(T.shape[1]), err_msg=str(what))


def _same(a, b, what=None, iters=True):
    for f in ("alpha", "mu", "T", "perm") + (("iters",) if iters else ()):
        x, y = (a[f] if isinstance(a, dict) else getattr(a, f)), (b[f] if isinstance(b, dict) else getattr(b, f))
        assert bits_equal(host(x), host(y)), (what, f)


# ------------------------------------------------------------------ stage entry

@pytest.mark.parametrize("case", ic.STAGE, ids=_ids)
def test_stage_entry_at_the_cap(pt2q, case):
    """AsymmetricTernaryQuantizer(max_iter=c): iterative_ternary_fitting from the init (the stage
    kernels' general-T entry form, also on a caller's T that is not ternary) and quantize without
    and with X (the AGA after a capped ITF).  67 x 128: every lane full; 67 x 100: a partial last
    16-column group; 33 x 16; 37 x 640 and 5 x 1100: the wide stage kernel."""
    n, b = case
    W, X, S1, d = ic.stage_inputs(n, b)
    k = ic.stage_k(n, b)
    Wd, Xd = cuda(W), cuda(X)
    a0, m0, T0 = orc.ternary_init(W)
    Tg = (synth.centered24(ic.seed(4, n, b), n * b).reshape(n, b) % 5 - 2).astype(np.float32)  # in -2 .. 2
    for c in ic.caps(k):
        q = pt2q.AsymmetricTernaryQuantizer(max_iter=c)
        ref = ic.stage_ref(n, b, c, False)
        assert ref[3] == min(c, k)
        _assert_atq(q.iterative_ternary_fitting(Wd, cuda(a0), cuda(m0), cuda(T0)), ref, ("itf", c))
        assert int(q.last_itf_iters.item()) == ref[3], ("itf", c)
        rg = orc.iterative_ternary_fitting(W, a0, m0, Tg, max_iter=c)
        _assert_atq(q.iterative_ternary_fitting(Wd, cuda(a0), cuda(m0), cuda(Tg)), rg, ("itf, general T", c))
        assert int(q.last_itf_iters.item()) == rg[3], ("itf, general T", c)
        _assert_atq(q.quantize(Wd), ref, ("quantize", c))
        assert int(q.last_itf_iters.item()) == ref[3], ("quantize", c)
        _assert_atq(q.quantize(Wd, Xd), ic.stage_ref(n, b, c, True), ("quantize, X", c))
        assert int(q.last_itf_iters.item()) == ref[3], ("quantize, X", c)


# ------------------------------------------------------------------ block loop

@pytest.mark.parametrize("aga", [True, False], ids=["aga", "noaga"])
@pytest.mark.parametrize("case", ic.BLOCKS, ids=_ids)
def test_block_loop_at_the_cap(pt2q, case, aga):
    """quantize_blocks with Hinv and SSR: the error feedback carries a capped block's result into
    the next block's input.  64 x 384: the 16-byte staged rows; 67 x 300: the per-element rows and a
    44-column last block; 48 x 1600 at 640: the wide kernel, then a 320-column block.  Every block's
    iteration count is compared.  noaga: the grid ITF leaves reaches the outputs (and the error
    term) as it is, so the cut at k - 1 shows in alpha and mu."""
    n, m, bs = case
    W, G, Hinv = ic.blocks_inputs(n, m)
    Wd, Gd, Hd = cuda(W), cuda(G), cuda(Hinv)
    L = pt2q._lib
    for c in ic.caps(ic.blocks_k(n, m, bs, aga=aga)):
        out = pt2q.quantize_blocks(Wd, Gd if aga else None, Hd, bs, True, L.AGA_ACT if aga else L.AGA_NONE, max_iter=c)
        _assert_layer(out, ic.blocks_ref(n, m, bs, c, aga), c)


# ------------------------------------------------------------------ per-channel

def _pc_call(pt2q, Wd, m, s1d, G, aga, c, t_dtype):
    L = pt2q._lib
    if not aga:
        return pt2q.quantize_blocks(Wd, None, None, m, True, L.AGA_NONE, max_iter=c, t_dtype=t_dtype)
    if m <= 512:  # the narrow block kernel forms S1 / d from the Gram
        return pt2q.quantize_blocks(Wd, G, None, m, True, L.AGA_ACT, max_iter=c, t_dtype=t_dtype)
    return pt2q.quantize_blocks(Wd, None, None, m, True, L.AGA_ACT, max_iter=c, t_dtype=t_dtype, s1d=s1d)


@pytest.mark.parametrize("t_dtype", ic.CODE_TYPES, ids=["i8", "f32"])
@pytest.mark.parametrize("case", ic.PER_CHANNEL, ids=_ids)
def test_per_channel_at_the_cap(pt2q, case, t_dtype):
    """One block of every column (b >= m), both code types.  64 x 256: the narrow kernel (NS = 16);
    40 x 1100 fp32 and 40 x 1104 fp16: the streamed atq_pc_kernel; 40 x 1100 fp16 and 24 x 1001
    fp32 (rows that are no whole 16-byte pieces): atq_wide_block_kernel on the row-major W;
    24 x 5120 bf16: the register-resident atq_pcr_kernel."""
    n, m, dt = case
    W, Wf, S1, d, G = ic.pc_inputs(n, m, dt)
    assert ("pc:atq_pcr" in ic.pc_paths(n, m, dt)) == (m == ic.PCR_M)
    Wd, s1d = W.to(DEV), cuda(ic.s1d_of(S1, d))
    Gd = cuda(G) if G is not None else None
    k = ic.pc_k(n, m, dt)
    for aga in (True, False):
        for c in ic.caps(k):
            _assert_pc(_pc_call(pt2q, Wd, m, s1d, Gd, aga, c, t_dtype), ic.pc_ref(n, m, dt, c, aga), (aga, c))


# ------------------------------------------------------------------ grouped entries

@pytest.mark.parametrize("aga", [True, False], ids=["aga", "noaga"])
def test_blocks_group_at_the_cap(pt2q, aga):
    """quantize_blocks_group, three 64 x 256 linears at 128: per linear the oracle's block loop at
    the same cap, at every cap of every member (their natural counts differ)."""
    count, n, m, bs = ic.GROUP_BLOCKS
    tags = [11 + 2 * z for z in range(count)]
    ins = [ic.blocks_inputs(n, m, t) for t in tags]
    Ws, Gs, Hs = ([cuda(x[j]) for x in ins] for j in range(3))
    L = pt2q._lib
    assert pt2q.engine.group_supported(n, m, bs, L.FLAG_SSR | (L.AGA_ACT if aga else L.AGA_NONE))
    for c in sorted(set().union(*[ic.caps(ic.blocks_k(n, m, bs, t, aga)) for t in tags])):
        outs = pt2q.engine.quantize_blocks_group(Ws, Gs if aga else None, Hs, bs, True,
                                                 L.AGA_ACT if aga else L.AGA_NONE, max_iter=c)
        for z, t in enumerate(tags):
            _assert_layer(outs[z], ic.blocks_ref(n, m, bs, c, aga, t), (c, z))


@pytest.mark.parametrize("case", ic.PC_GROUPS, ids=lambda c: "%d-%s" % c[1:])
def test_perchannel_group_at_the_cap(pt2q, case):
    """quantize_perchannel_group over 24, 9 and 16 rows, the middle member an all-zero W: the
    repair gives it alpha = mu = 0 and iters = 0 while its neighbours stop at the cap; every member
    equals the oracle and its own quantize_blocks call at the same cap.  1100 fp32: the streamed
    kernel's grouped grid; 1100 fp16: a wide-kernel launch per member; 5120 bf16: the
    register-resident kernel; each followed by the group's repair launch."""
    ns, m, dt = case
    members = ic.pc_group_members(ns, m, dt)
    ins = [ic.pc_inputs(n, m, dt, tag, zero) for n, tag, zero in members]
    Wds = [x[0].to(DEV) for x in ins]
    s1d = cuda(ic.s1d_of(ins[0][2], ins[0][3]))
    eng, L = pt2q.engine, pt2q._lib
    ks = [ic.pc_k(n, m, dt, tag) for n, tag, zero in members if not zero]
    for t_dtype in ic.CODE_TYPES:
        for c in sorted(set().union(*[ic.caps(k) for k in ks])):
            outs = eng.quantize_perchannel_group(Wds, [s1d] * len(Wds), max_iter=c, t_dtype=t_dtype)
            for z, (n, tag, zero) in enumerate(members):
                _assert_pc(outs[z], ic.pc_ref(n, m, dt, c, True, tag, zero), (c, z))
                own = pt2q.quantize_blocks(Wds[z], None, None, m, True, L.AGA_ACT, max_iter=c, t_dtype=t_dtype, s1d=s1d)
                _same(outs[z], own, (c, z))
                if zero:
                    assert not host(outs[z].alpha).any() and not host(outs[z].mu).any() and not host(outs[z].T).any()
                    assert host(outs[z].iters).tolist() == [0]
                else:
                    assert host(outs[z].iters).tolist() == [min(c, ic.pc_k(n, m, dt, tag))]
        outs = eng.quantize_perchannel_group(Wds, None, max_iter=2, t_dtype=t_dtype)  # no AGA
        for z, (n, tag, zero) in enumerate(members):
            _assert_pc(outs[z], ic.pc_ref(n, m, dt, 2, False, tag, zero), ("no AGA", z))


# ------------------------------------------------------------------ fused layer, captured graph

def test_quantize_layer_at_the_cap(pt2q):
    n, m, N, bs = ic.LAYER
    W, X, ref = ic.layer_case()
    out = pt2q.quantize_layer(cuda(W), cuda(X), block_size=bs, use_ssr=True, max_iter=ic.LAYER_CAP)
    assert out.spd and ref["spd"]
    _assert_layer(out, ref)
    assert host(out.iters).tolist() == [ic.LAYER_CAP] * rc.ceil_div(m, bs)
    _assert_layer(pt2q.quantize_layer(cuda(W), cuda(X), block_size=bs, use_ssr=True), ic.layer_case(ic.UNCAPPED)[2])


def test_layer_graph_at_the_cap(pt2q):
    """LayerGraph(max_iter=2): the replay equals the eager bits and the oracle's, and again after W
    changed in place."""
    n, m, N, bs = ic.LAYER
    W, X, ref = ic.layer_case()
    Wd, Xd = cuda(W), cuda(X)
    eager = pt2q.quantize_layer(Wd, Xd, block_size=bs, use_ssr=True, max_iter=ic.LAYER_CAP)
    lg = pt2q.LayerGraph(Wd, Xd, block_size=bs, use_ssr=True, max_iter=ic.LAYER_CAP)
    out = lg.replay()
    torch.cuda.synchronize()
    assert lg.spd()
    _same(out, eager)
    _assert_layer(out, ref)
    W2 = ic.weights(21, n, m, easy=True)
    Wd.copy_(cuda(W2))
    out = lg.replay()
    torch.cuda.synchronize()
    assert lg.spd()
    _same(out, pt2q.quantize_layer(Wd, Xd, block_size=bs, use_ssr=True, max_iter=ic.LAYER_CAP))
    _assert_layer(out, orc.quantize_layer_m(W2, X, block_size=bs, use_ssr=True, max_iter=ic.LAYER_CAP))
    assert not bits_equal(host(out.alpha), ref["alpha"])


# ------------------------------------------------------------------ plumbing

def _plumb_units(bs):
    units, data = [], {}
    for i, (m, dt, ns, N) in enumerate(ic.PLUMB[bs]):
        X = rc.to_dtype(ic.activations(30 + i, N, m), dt).to(DEV)
        Ws = {f"p{k}": rc.to_dtype(ic.weights(40 + 10 * i + k, n, m), dt).to(DEV) for k, n in enumerate(ns)}
        units.append((f"u{i}", [(f"p{k}", n, m) for k, n in enumerate(ns)], N))
        data[f"u{i}"] = (X, Ws)
    return units, data


@pytest.mark.parametrize("bs", sorted(ic.PLUMB))
def test_plumbing_carries_the_cap(pt2q, bs):
    """max_iter = 2 through UnitPipeline(lanes=3), a GramsFirst step (grouped, and group=1),
    quantize_shared and quantize_layer_split (world 1): linear for linear the bits of
    quantize_layer(..., max_iter=2), which are not those of the default 100 -- a dropped argument
    shows.  bs = 128: grouped and lone block loops; bs = 2048: the per-channel group."""
    sharding = importlib.import_module("pt2q.sharding")
    cap = ic.LAYER_CAP
    units, data = _plumb_units(bs)
    want = {}
    for name, lins, N in units:
        X, Ws = data[name]
        for p, n, m in lins:
            want[f"{name}.{p}"] = pt2q.quantize_layer(Ws[p], X, bs, True, max_iter=cap)
            full = pt2q.quantize_layer(Ws[p], X, bs, True)
            assert (host(want[f"{name}.{p}"].iters) == cap).all() and (host(full.iters) > cap).all()
            assert not bits_equal(host(want[f"{name}.{p}"].alpha), host(full.alpha))

    def check(outs_by_name, what, iters=True):
        assert sorted(outs_by_name) == sorted(want), what
        for key, o in outs_by_name.items():
            _same(o, want[key], (what, key), iters=iters)

    pipe = pt2q.UnitPipeline(DEV, bs, True, max_iter=cap, lanes=3)
    runs = [(name, lins, pipe.run([data[name][1][p] for p, _, _ in lins], data[name][0])) for name, lins, _ in units]
    check({f"{name}.{p}": o for name, lins, run in runs for (p, _, _), o in zip(lins, run.finish())}, "UnitPipeline")
    for group in (16, 1):
        gf = sharding.GramsFirst(pt2q.UnitPipeline(DEV, bs, True, max_iter=cap, lanes=3), DEV, batched=True, group=group)
        res, mine = sharding.quantize_units_sharded(units, lambda u: data[u[0]], block_size=bs, pack=False, grams_first=gf)
        assert sorted(mine) == list(range(len(units))) and gf.grouped == (group > 1)
        check(res, ("GramsFirst", group), iters=False)
    shared, split = {}, {}
    for name, lins, N in units:
        X, Ws = data[name]
        Wl = [Ws[p] for p, _, _ in lins]
        for (p, _, _), o, s in zip(lins, pt2q.quantize_shared(Wl, pt2q.gram(X), N, bs, True, max_iter=cap),
                                   sharding.quantize_layer_split(Wl, X, block_size=bs, use_ssr=True, max_iter=cap)):
            shared[f"{name}.{p}"], split[f"{name}.{p}"] = o, s
    check(shared, "quantize_shared")
    check(split, "quantize_layer_split")


def test_pinv_fallbacks_carry_the_cap(pt2q):
    """The three re-runs after a Cholesky breakdown (main.py:140-141: pinv of the damped Hessian,
    then the block loops again) keep the cap: quantize_unit's and a grouped GramsFirst step's on a
    negated Gram, quantize_layer's on activations with a zero column and no damping -- each equal
    to quantize_blocks at max_iter = 2 with the same pinv.  Block 0 sees no error feedback, so its
    count is the cap, where the default run's is above it."""
    sharding = importlib.import_module("pt2q.sharding")
    cap, bs = ic.LAYER_CAP, 128
    m, dt, ns, N = ic.PLUMB[bs][0]
    X = rc.to_dtype(ic.activations(60, N, m), dt).to(DEV)
    Wl = [rc.to_dtype(ic.weights(61 + k, n, m), dt).to(DEV) for k, n in enumerate(ns)]

    def want_for(G, percdamp):
        Hinv = torch.linalg.pinv(pt2q.prepare_hessian(G, N, percdamp)[0])
        outs = [pt2q.quantize_blocks(W, G, Hinv, bs, True, max_iter=cap) for W in Wl]
        for W, o in zip(Wl, outs):
            assert host(o.iters)[0] == cap < host(pt2q.quantize_blocks(W, G, Hinv, bs, True).iters)[0]
        return outs

    Gneg = -pt2q.gram(X)
    want = want_for(Gneg, 0.01)
    got = pt2q.quantize_unit(Wl, G=Gneg, nsamples=N, block_size=bs, max_iter=cap)
    assert [o.spd for o in got] == [False] * len(Wl)
    for o, r in zip(got, want):
        _same(o, r, "quantize_unit")
    gf = sharding.GramsFirst(pt2q.UnitPipeline(DEV, bs, True, max_iter=cap, lanes=2), DEV, batched=True, group=16)
    gf.begin([(0, m, N)])
    gf.gram(0, X)
    gf.flush()
    g, z = gf.slot[0]
    gf.groups[g]["G"][z].neg_()
    gf.inverses()
    got = gf.tails([(0, Wl, N)])[0].finish()
    gf.check()
    assert gf.grouped and [o.spd for o in got] == [False] * len(Wl)
    for o, r in zip(got, want):
        _same(o, r, "GramsFirst")
    X0 = X.clone()
    X0[:, 5] = 0.0  # a zero input column and percdamp 0: H is singular (the layer_m_notspd fixture's way)
    want = want_for(pt2q.gram(X0), 0.0)
    for W, r in zip(Wl, want):
        o = pt2q.quantize_layer(W, X0, bs, True, percdamp=0.0, max_iter=cap)
        assert not o.spd
        _same(o, r, "quantize_layer")


# ------------------------------------------------------------------ status codes

def test_negative_cap_is_refused_and_writes_nothing(pt2q):
    """max_iter = -1: PT2Q_E_ARG from all five C entries (the cases of
    test_itf_cap_cases_cpu.py, here on device buffers), every output still the sentinel it was
    filled with; the same calls with max_iter = 0 run, so the cap alone is what was refused.  The
    Python surface raises."""
    lib, L = pt2q._lib.lib(), pt2q._lib
    n, m, b, N, count, wide = (ic.NEG[k] for k in ("n", "m", "b", "N", "count", "wide"))
    flags = L.FLAG_SSR | L.AGA_ACT
    X = cuda(ic.activations(50, N, m))
    keep = {"W": cuda(ic.weights(51, n, m)), "X": X, "G": pt2q.gram(X),
            "Hinv": torch.eye(m, dtype=torch.float32, device=DEV).contiguous()}
    outs = {}

    def sentinel(key, nbytes=1 << 16):
        outs[key] = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
        return outs[key].data_ptr()
    ws_bytes = 4096 + max(lib.pt2q_layer_workspace_bytes(n, m, b, flags), lib.pt2q_blocks_workspace_bytes(n, m, b, flags),
                          lib.pt2q_quantize_blocks_group_workspace_bytes(count, n, m, b, flags),
                          lib.pt2q_quantize_perchannel_group_workspace_bytes(count))
    ws = L.workspace(ws_bytes, DEV)
    bufs = {k: v.data_ptr() for k, v in keep.items()}
    bufs.update({k: sentinel(k) for k in ("alpha", "mu", "T", "Tf", "perm", "iters", "info")})
    bufs.update(ws=ws.data_ptr(), ws_bytes=ws.numel())
    for z in range(count):
        keep[f"W{z}"], keep[f"Ww{z}"] = cuda(ic.weights(52 + z, n, m)), cuda(ic.weights(54 + z, n, wide))
    bufs.update(Wz=[keep[f"W{z}"].data_ptr() for z in range(count)], Wwz=[keep[f"Ww{z}"].data_ptr() for z in range(count)],
                Gz=[bufs["G"]] * count, Hz=[bufs["Hinv"]] * count)
    for k in ("az", "mz", "Tz", "pz", "iz", "Twz", "pwz"):
        bufs[k] = [sentinel(f"{k}{z}") for z in range(count)]
    calls, arrays = ic.negative_cap_calls(lib, bufs)
    assert len(calls) == 5
    for name, call in calls.items():
        assert call(-1) == E_ARG, name
    torch.cuda.synchronize()
    for key, t in outs.items():
        assert bool((t == 0x5A).all()), key
    for name, call in calls.items():  # every other argument is valid: the same calls run at max_iter = 0
        assert call(0) == L.PT2Q_OK, name
    torch.cuda.synchronize()
    for key in ("alpha", "mu", "T", "Tf", "perm", "az0", "mz1", "Tz0", "pz1", "Twz0", "pwz1"):
        assert not bool((outs[key] == 0x5A).all()), key
    with pytest.raises(L.Pt2qError):
        pt2q.AsymmetricTernaryQuantizer(max_iter=-1).quantize(keep["W"])
    with pytest.raises(L.Pt2qError):
        pt2q.quantize_layer(keep["W"], X, b, True, max_iter=-1)
    with pytest.raises(L.Pt2qError):
        pt2q.quantize_blocks(keep["W"], keep["G"], keep["Hinv"], b, True, max_iter=-1)
