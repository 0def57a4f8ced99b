"""One case per host-side launch sequence of every stream-taking entry of include/pt2q.h -- a plain
helper, not a conftest.

tests/test_gpu_stream_order.py runs every case on a delayed, non-default stream over buffers that
hold a decoy problem before and after the call; tests/test_stream_cases_cpu.py checks, without a
GPU, that the table covers the header and that the decoys can show a stale read.  This module
imports neither torch.cuda nor the library: a case only describes its buffers and its call.

A case gives
  entry    the pt2q.h function,
  make     make(seed) -> {name: CPU tensor}: every device input (and "h_*": host scalars the call
           passes by value, e.g. pt2q_fill_synthetic's seed).  The decoy of a case is make() with
           another seed: same shapes and dtypes, other values,
  out      {name: (shape, dtype)}: pure outputs and caller-owned scratch, allocated zeroed,
  ws       {name: bytes(L)}: workspaces, sized by the library's own *_workspace_bytes,
  call     call(c) -> status or [statuses]: the argument list(s) from a Ctx (device pointers by
           buffer name, pointer arrays, the stream),
  outputs  the buffers a test compares (pure outputs and in-out inputs),
  status   workspaces whose first int is the entry's status word (pt2q.h PT2Q_STATUS_BYTES),
  index    {input: kind} for inputs a kernel uses as an index, a count or a code: ("range", lo, hi)
           or ("codes2",) (four 2-bit codes <= 2 per byte).  A decoy of such an input is a valid
           value of its kind -- never poison: an ordering bug must show as wrong bits only,
  oracle   optional, where it is cheap: oracle(inputs) -> {output: array} from oracle/ or the
           *_ref restatements,
  pinned   the existing test that ties this entry at this shape or launch form to the oracle (the
           default-stream bits are the reference where `oracle` is None).

To add a case for a new entry: write its make() from synth (values) and numpy (valid indices) so
that another seed changes every buffer, list its outputs, name the test that pins its bits, and
append it to CASES; test_stream_cases_cpu.py fails until every `void* stream` entry of the header
has one.  Keep a case below ~500 launches: a full hardware queue must never be what makes the
host wait."""
import ctypes
import os
import re

import numpy as np
import torch

import ragged_cases as rc
import synth
import ternary_decode_ref as tdr
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pt2q.h")
REAL_SEED, DECOY_SEED = 4100, 5200
F32, F16, BF16, I8 = 0, 1, 2, 3
SSR, S1_GIVEN, ACT, HESS = 0x1, 0x2, 0x10, 0x20
f32, f16, bf16 = torch.float32, torch.float16, torch.bfloat16
i8, u8, i32, i64 = torch.int8, torch.uint8, torch.int32, torch.int64
CODE = {f32: F32, f16: F16, bf16: BF16, i8: I8}


def stream_entries(path=HEADER):
    """The functions of pt2q.h whose last parameter is `void* stream`."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(pt2q_\w+)\s*\([^;{]*?\bvoid\s*\*\s*stream\s*\)\s*;", text)))


class Ctx:
    """What a case's call() sees: one buffer set, the host scalars, the library and a stream."""

    def __init__(self, L, bufs, host, stream):
        self.L, self.t, self.host, self.st = L, bufs, host, ctypes.c_void_p(stream)
        self.arrays = []  # (ctypes array, buffer names): the host pointer arrays of this call

    def p(self, name, offset=0):
        return ctypes.c_void_p(self.t[name].data_ptr() + offset)

    def nbytes(self, name):
        return self.t[name].numel() * self.t[name].element_size()

    def arr(self, *names):
        a = (ctypes.c_void_p * len(names))(*[self.t[k].data_ptr() for k in names])
        self.arrays.append((a, names))
        return ctypes.cast(a, ctypes.c_void_p)

    def ints(self, vals, ty=ctypes.c_int):
        a = (ty * len(vals))(*vals)
        self.arrays.append((a, ()))  # kept alive; not a pointer array
        return ctypes.cast(a, ctypes.c_void_p)

    def h(self, name):
        return self.host["h_" + name]


class Case:
    def __init__(self, id, entry, make, call, outputs, pinned, out=None, ws=None, status=(), index=None,
                 oracle=None):
        self.id, self.entry, self.make, self.call, self.outputs, self.pinned = id, entry, make, call, outputs, pinned
        self.out, self.ws, self.status, self.index, self.oracle = out or {}, ws or {}, status, index or {}, oracle

    def __repr__(self):
        return self.id


CASES = []


def case(*a, **k):
    CASES.append(Case(*a, **k))


# ------------------------------------------------------------------ input builders

def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x if dtype is None else x.to(dtype)


def acts(seed, N, m, dtype=f32):
    return t(synth.activations(seed, N, m), dtype)


def wts(seed, n, m, dtype=f32):
    return t(synth.weights(seed, n, m), dtype)


def sym(A):
    return (np.triu(A) + np.triu(A, 1).T).astype(np.float32)


def raw_gram(seed, m, N):
    """A symmetric positive semi-definite fp32 matrix: XᵀX of N synthetic rows (numpy; an input
    like any other -- the entries under test do not care how their Gram was summed)."""
    X = synth.activations(seed, N, m)
    return sym(X.T @ X)


def damped(G, N):
    H = G / np.float32(N)
    return sym(H + np.float32(0.01) * np.mean(np.diag(H)) * np.eye(len(G), dtype=np.float32))


def spd(seed, m):
    """A cheap well-conditioned SPD matrix: a rank-128 Gram plus the identity (as
    test_gpu_strides._inverse_ref)."""
    X = synth.activations(seed, 128, m)
    return sym(X.T @ X / np.float32(128) + np.eye(m, dtype=np.float32))


def inverse(H):
    return sym(np.linalg.inv(H.astype(np.float64)))


def s1d_of(G):
    S1 = G.sum(axis=1, dtype=np.float32)
    return np.concatenate([S1, [S1.sum(dtype=np.float32)]]).astype(np.float32)


def loop_out(n, m, B, z=""):
    return {"alpha" + z: ((n, B), f32), "mu" + z: ((n, B), f32), "T" + z: ((n, m), i8), "perm" + z: ((m,), i64),
            "iters" + z: ((B,), i32)}


LOOP = ("alpha", "mu", "T", "perm", "iters")


# ------------------------------------------------------------------ pt2q_gram

def _gram_f32(mode):
    def make(seed):
        d = {"X": acts(seed, 70, 100)}
        if mode:
            d["X0"] = acts(seed + 1, 16, 100)          # (the rows G already holds; not an argument)
            d["G"] = t(orc.gram(d["X0"].numpy()))
        return d

    def oracle(i):
        GX = orc.gram(i["X"].numpy())
        if mode == 0:
            return {"G": GX}
        if mode == 1:
            return {"G": (i["G"].numpy() + GX).astype(np.float32)}
        return {"G": orc.gram(np.concatenate([i["X0"].numpy(), i["X"].numpy()]))}
    case("gram-f32-acc%d" % mode, "pt2q_gram", make,
         lambda c: c.L.pt2q_gram(c.p("X"), F32, 70, 100, 100, c.p("G"), 100, mode, None, 0, c.st),
         ("G",), "test_gpu_strides.py::test_gram_f32", out={} if mode else {"G": ((100, 100), f32)}, oracle=oracle)


for _mode in (0, 1, 2):
    _gram_f32(_mode)

case("gram-f16-streamk", "pt2q_gram", lambda seed: {"X": acts(seed, 40, 4096, f16)},
     lambda c: c.L.pt2q_gram(c.p("X"), F16, 40, 4096, 4096, c.p("G"), 4096, 0, c.p("ws"), c.nbytes("ws"), c.st),
     ("G",), "test_gpu_strides.py::test_gram16_split", out={"G": ((4096, 4096), f32)},
     ws={"ws": lambda L: L.pt2q_gram_workspace_bytes(4096)}, status=("ws",))


def _gram_batched(id, fn, dt, m, N, batch, pinned):
    names = ["X%d" % z for z in range(batch)]
    case(id, fn, lambda seed: {k: acts(seed + z, N, m, dt) for z, k in enumerate(names)},
         lambda c: getattr(c.L, fn)(batch, c.arr(*names), CODE[dt], N, m, m, c.p("G"), c.st),
         ("G",), pinned, out={"G": ((batch, m, m), f32)})


_gram_batched("gram-batched-f16", "pt2q_gram_batched", f16, 256, 72, 3, "test_gpu_strides.py::test_gram16_batched_padded")
_gram_batched("gram-batched-f32", "pt2q_gram_batched", f32, 100, 70, 2, "test_gpu_strides.py::test_gram_f32_batched_padded")
_gram_batched("gram-batched-upper-bf16", "pt2q_gram_batched_upper", bf16, 256, 72, 2,
              "test_gpu_strides.py::test_gram16_batched_padded")

# ------------------------------------------------------------------ Hessian, Cholesky inverse


def _prepare(m):
    N = m + 50

    def oracle(i):
        H, damp = orc.prepare_hessian(i["G"].numpy(), N, 0.01)
        return {"H": H, "damp": np.array([damp], np.float32)}
    case("prepare-hessian-%s" % rc.prepare_hessian_form(m), "pt2q_prepare_hessian",
         lambda seed: {"G": t(raw_gram(seed, m, N))},
         lambda c: c.L.pt2q_prepare_hessian(c.p("G"), m, m, N, 0.01, c.p("H"), m, c.p("damp"), c.st),
         ("H", "damp"), "test_gpu_strides.py::test_prepare_hessian", out={"H": ((m, m), f32), "damp": ((1,), f32)},
         oracle=oracle)


_prepare(100)   # fill4
_prepare(65)    # fill
assert {rc.prepare_hessian_form(100), rc.prepare_hessian_form(65)} == {"fill4", "fill"}

CHOL_AHEAD_M = 6208  # m > 6144 and more than two 512-row panels: the side stream of chol.hip


def chol_make(m):
    return lambda seed: {"H": t(spd(seed, m))}


def chol_call(m):
    return lambda c: c.L.pt2q_cholesky_inverse(c.p("H"), m, m, c.p("Hinv"), m, c.p("ws"), c.nbytes("ws"), c.p("info"),
                                               c.st)


def chol_out(m):
    return {"Hinv": ((m, m), f32), "info": ((1,), i32)}


def chol_ws(m):
    return {"ws": lambda L: L.pt2q_cholesky_workspace_bytes(m)}


def _chol_oracle(i):
    Hinv, spd_ = orc.cholesky_inverse(i["H"].numpy())
    return {"Hinv": Hinv, "info": np.array([0 if spd_ else 1], np.int32)}


for _m in (80, 700, 2200, CHOL_AHEAD_M):
    case("cholesky-inverse-%d" % _m, "pt2q_cholesky_inverse", chol_make(_m), chol_call(_m), ("Hinv", "info"),
         "test_gpu_parity.py::test_hessian_cholesky_inverse_bitexact", out=chol_out(_m), ws=chol_ws(_m),
         oracle=_chol_oracle if _m == 80 else None)


def _inverse_batched(m, batch, chunk):
    N, c = m + 50, min(chunk, batch)
    isz = m * m * 4

    def call(x):
        return [x.L.pt2q_hessian_inverse_batched(x.p("G", z0 * isz), m, min(c, batch - z0), N, 0.01, x.p("H"),
                                                 x.p("Hinv", z0 * isz), x.p("ws"), x.nbytes("ws"), x.p("info", 4 * z0),
                                                 x.st) for z0 in range(0, batch, c)]
    case("inverse-batched-%dx%d-chunk%d" % (m, batch, c), "pt2q_hessian_inverse_batched",
         lambda seed: {"G": t(np.stack([raw_gram(seed + z, m, N) for z in range(batch)]))}, call, ("Hinv", "info"),
         "test_gpu_parity.py::test_hessian_inverse_batched_equals_per_item",
         out={"H": ((c, m, m), f32), "Hinv": ((batch, m, m), f32), "info": ((batch,), i32)},
         ws={"ws": lambda L: L.pt2q_hessian_inverse_batched_workspace_bytes(m, c)})


_inverse_batched(131, 3, 32)
_inverse_batched(384, 4, 3)

# ------------------------------------------------------------------ block loops


def loop_inputs(seed, n, m, dt=f32):
    """W, the raw Gram of m + 60 rows, its damped Hessian and (numpy) inverse."""
    G = raw_gram(seed + 1, m, m + 60)
    H = damped(G, m + 60)
    return {"W": wts(seed, n, m, dt), "G": t(G), "H": t(H), "Hinv": t(inverse(H))}


def _blocks(id, n, m, b, flags, pinned, with_oracle):
    B = rc.ceil_div(m, b)
    A = {ACT: "G", HESS: "H", 0: None}[flags & 0x30]

    def make(seed):
        d = loop_inputs(seed, n, m)
        return {k: d[k] for k in ("W", "Hinv") + ((A,) if A else ())}

    def call(c):
        return c.L.pt2q_quantize_blocks(c.p("W"), F32, m, n, m, b, flags, c.p(A) if A else None, m, c.p("Hinv"), m,
                                        100, c.p("alpha"), c.p("mu"), c.p("T"), I8, c.p("perm"), c.p("iters"),
                                        c.p("ws"), c.nbytes("ws"), c.st)

    def oracle(i):
        r = orc.quantize_blocks(i["W"].numpy(), i[A].numpy() if A else None, i["Hinv"].numpy(), b, True,
                                {ACT: 1, HESS: 2, 0: 0}[flags & 0x30])
        return {k: r[k] for k in LOOP}
    case(id, "pt2q_quantize_blocks", make, call, LOOP, pinned, out=loop_out(n, m, B),
         ws={"ws": lambda L: L.pt2q_blocks_workspace_bytes(n, m, b, flags)}, status=("ws",),
         oracle=oracle if with_oracle else None)


_blocks("blocks-act", 203, 333, 128, SSR | ACT, "test_gpu_ragged.py::test_layer_m_ragged", True)
_blocks("blocks-hess", 203, 333, 128, SSR | HESS, "test_gpu_ragged.py::test_layer_g_ragged", True)
_blocks("blocks-none", 203, 333, 128, SSR, "test_gpu_itf_cap.py::test_block_loop_at_the_cap", True)
_blocks("blocks-wide", 384, 640, 256, SSR | ACT, "test_gpu_parity.py::test_gptq_wide_blocks_vs_oracle", False)

PC_N, PC_M = 70, 520


def _pc_make(seed):
    return {"W": wts(seed, PC_N, PC_M, bf16), "S1d": t(s1d_of(raw_gram(seed + 1, PC_M, 300)))}


case("blocks-per-channel-s1-given", "pt2q_quantize_blocks", _pc_make,
     lambda c: c.L.pt2q_quantize_blocks(c.p("W"), BF16, PC_M, PC_N, PC_M, PC_M, SSR | ACT | S1_GIVEN, c.p("S1d"), PC_M,
                                        None, 0, 100, c.p("alpha"), c.p("mu"), c.p("T"), I8, c.p("perm"),
                                        c.p("iters"), c.p("ws"), c.nbytes("ws"), c.st),
     LOOP, "test_gpu_strides.py::test_quantize_blocks_per_channel", out=loop_out(PC_N, PC_M, 1),
     ws={"ws": lambda L: L.pt2q_blocks_workspace_bytes(PC_N, PC_M, PC_M, SSR | ACT | S1_GIVEN)}, status=("ws",))


def _blocks_group(n, m, b, count):
    B, flags = m // b, SSR | ACT
    zs = [str(z) for z in range(count)]

    def make(seed):
        d = {}
        for z in zs:
            x = loop_inputs(seed + 10 * int(z), n, m)
            d.update({"W" + z: x["W"], "G" + z: x["G"], "Hinv" + z: x["Hinv"]})
        return d

    def call(c):
        a = lambda k: c.arr(*[k + z for z in zs])  # noqa: E731
        return c.L.pt2q_quantize_blocks_group(count, a("W"), F32, m, n, m, b, flags, a("G"), m, a("Hinv"), m, 100,
                                              a("alpha"), a("mu"), a("T"), I8, a("perm"), a("iters"), c.p("ws"),
                                              c.nbytes("ws"), c.st)
    out = {}
    for z in zs:
        out.update(loop_out(n, m, B, z))
    case("blocks-group-%dx%dx%d" % (count, n, m), "pt2q_quantize_blocks_group", make, call,
         tuple(k + z for z in zs for k in LOOP), "test_gpu_parity.py::test_blocks_group_equals_per_linear", out=out,
         ws={"ws": lambda L: L.pt2q_quantize_blocks_group_workspace_bytes(count, n, m, b, flags)}, status=("ws",))


_blocks_group(256, 512, 128, 3)
PCG_NS = (70, 36)


def _pcg_make(seed):
    d = {"W%d" % z: wts(seed + z, n, PC_M, bf16) for z, n in enumerate(PCG_NS)}
    d["S1d"] = t(s1d_of(raw_gram(seed + 7, PC_M, 300)))
    return d


def _pcg_call(c):
    zs = [str(z) for z in range(len(PCG_NS))]
    a = lambda k: c.arr(*[k + z for z in zs])  # noqa: E731
    return c.L.pt2q_quantize_perchannel_group(len(PCG_NS), a("W"), BF16, PC_M, c.ints(PCG_NS), PC_M,
                                              c.arr(*["S1d"] * len(PCG_NS)), 100, a("alpha"), a("mu"), a("T"), I8,
                                              a("perm"), a("iters"), c.p("ws"), c.nbytes("ws"), c.st)


_o = {}
for _z, _n in enumerate(PCG_NS):
    _o.update(loop_out(_n, PC_M, 1, str(_z)))
case("perchannel-group", "pt2q_quantize_perchannel_group", _pcg_make, _pcg_call,
     tuple(k + str(z) for z in range(len(PCG_NS)) for k in LOOP),
     "test_gpu_strides.py::test_quantize_perchannel_group", out=_o,
     ws={"ws": lambda L: L.pt2q_quantize_perchannel_group_workspace_bytes(len(PCG_NS))}, status=("ws",))

LN, LM, LNN, LB = rc.GRAPH_LAYER[:4]
case("quantize-layer", "pt2q_quantize_layer",
     lambda seed: {"W": wts(seed, LN, LM), "X": acts(seed + 1, LNN, LM)},
     lambda c: c.L.pt2q_quantize_layer(c.p("W"), F32, LM, LN, LM, c.p("X"), F32, LNN, LM, LB, SSR | ACT, 0.01, 100,
                                       c.p("alpha"), c.p("mu"), c.p("T"), I8, c.p("perm"), c.p("iters"), c.p("info"),
                                       c.p("ws"), c.nbytes("ws"), c.st),
     LOOP + ("info",), "test_gpu_ragged.py::test_layer_graph_replay_ragged",
     out=dict(loop_out(LN, LM, rc.ceil_div(LM, LB)), info=((1,), i32)),
     ws={"ws": lambda L: L.pt2q_layer_workspace_bytes(LN, LM, LB, SSR | ACT)}, status=("ws",))

# ------------------------------------------------------------------ pt2q_atq_stage

STAGE_NAMES = ("init", "grid", "round", "itf", "aga", "full")
STAGE_IN = {0: (), 1: ("T",), 2: ("alpha", "mu"), 3: ("alpha", "mu", "T"), 4: ("T", "S1", "d"), 5: ("S1", "d")}
STAGE_OUT = {0: ("alpha", "mu", "T"), 1: ("alpha", "mu"), 2: ("T",), 3: ("alpha", "mu", "T", "iters"),
             4: ("alpha", "mu"), 5: ("alpha", "mu", "T", "iters")}


def _stage(mode, n, b, pinned):
    shapes = {"alpha": ((n,), f32), "mu": ((n,), f32), "T": ((n, b), f32), "iters": ((1,), i32)}

    def make(seed):
        W = synth.weights(seed, n, b)
        a, mu, T = orc.ternary_init(W)
        S1, d = orc.s1_from_x(synth.activations(seed + 1, 24, b))
        full = {"alpha": t(a[:, 0]), "mu": t(mu[:, 0]), "T": t(T, f32), "S1": t(S1), "d": t(np.array([d], np.float32))}
        return dict({"W": t(W)}, **{k: full[k] for k in STAGE_IN[mode]})

    def call(c):
        opt = lambda k: c.p(k) if k in c.t else None  # noqa: E731
        return c.L.pt2q_atq_stage(mode, c.p("W"), b, n, b, c.p("alpha"), c.p("mu"), c.p("T"), b, opt("S1"), opt("d"),
                                  100, c.p("iters") if mode in (3, 5) else None, c.p("ws"), c.nbytes("ws"), c.st)

    def full_oracle(i):
        W = i["W"].numpy()
        a, mu, T = orc.ternary_init(W)
        a, mu, T, it = orc.iterative_ternary_fitting(W, a, mu, T, 100)
        a, mu = orc.activation_aware_grid_alignment(W, T, S1=i["S1"].numpy(), d=np.float32(i["d"].numpy()[0]))
        return {"alpha": a[:, 0], "mu": mu[:, 0], "T": T, "iters": np.array([it], np.int32)}
    case("atq-stage-%s-%dx%d" % (STAGE_NAMES[mode], n, b), "pt2q_atq_stage", make, call, STAGE_OUT[mode], pinned,
         out={k: v for k, v in shapes.items() if k not in STAGE_IN[mode]}, ws={"ws": lambda L: 256},
         oracle=full_oracle if mode == 5 else None)


for _mode in range(6):
    _stage(_mode, 64, 128, "test_gpu_parity.py::test_atq_stages_vs_oracle_and_reference")
_stage(5, 64, 777, "test_gpu_strides.py::test_atq_stage_full")

# ------------------------------------------------------------------ S1 / d
S1_M = 520


def _s1_oracle(S):
    S1 = orc.rowsum_seq(S)
    return np.concatenate([S1, orc.rowsum_seq(S1[None, :])]).astype(np.float32)


case("s1-from-gram", "pt2q_s1_from_gram", lambda seed: {"S": t(raw_gram(seed, S1_M, 24))},
     lambda c: c.L.pt2q_s1_from_gram(c.p("S"), S1_M, S1_M, c.p("S1"), c.p("d"), c.st), ("S1", "d"),
     "test_gpu_strides.py::test_s1_from_gram", out={"S1": ((S1_M,), f32), "d": ((1,), f32)},
     oracle=lambda i: {"S1": _s1_oracle(i["S"].numpy())[:S1_M], "d": _s1_oracle(i["S"].numpy())[S1_M:]})
for _fn, _pin in (("pt2q_s1_from_gram_batched", "test_gpu_strides.py::test_s1_from_gram"),
                  ("pt2q_s1_from_upper_batched", "test_gpu_strides.py::test_s1_from_upper")):
    case(_fn[5:].replace("_", "-"), _fn,
         lambda seed: {"S": t(np.stack([raw_gram(seed + z, S1_M, 24) for z in range(2)]))},
         lambda c, fn=_fn: getattr(c.L, fn)(c.p("S"), S1_M, S1_M, 2, S1_M * S1_M, c.p("S1d"), c.st), ("S1d",), _pin,
         out={"S1d": ((2, S1_M + 1), f32)},
         oracle=lambda i: {"S1d": np.stack([_s1_oracle(S) for S in i["S"].numpy()])})

# ------------------------------------------------------------------ SSR
SN, SM, SB = 256, 700, 128


def _ssr_make(seed):
    cols = np.arange(SM, dtype=np.int64)
    return {"W": wts(seed, SN, SM), "rem": t(cols[(cols % 13) != (4 if seed == REAL_SEED else 7)])}


SR = int(_ssr_make(REAL_SEED)["rem"].numel())


def _ssr_oracle(i):
    W, rem = i["W"].numpy(), i["rem"].numpy()
    blk, new = orc.select_next_block_ssr(W, rem, SB)
    return {"blk": blk, "newrem": new, "sim": orc.ssr_similarity(W, rem)}


case("ssr-select", "pt2q_ssr_select", _ssr_make,
     lambda c: c.L.pt2q_ssr_select(c.p("W"), SM, SN, SM, c.p("rem"), SR, SB, c.p("blk"), c.p("newrem"), c.p("sim"),
                                   c.p("ws"), c.nbytes("ws"), c.st),
     ("blk", "newrem", "sim"), "test_gpu_strides.py::test_ssr_select",
     out={"blk": ((SB,), i64), "newrem": ((SR - SB,), i64), "sim": ((SR,), f32)},
     ws={"ws": lambda L: L.pt2q_ssr_workspace_bytes(SN, SM)}, status=("ws",), index={"rem": ("range", 0, SM)},
     oracle=_ssr_oracle)
case("cosine-similarity", "pt2q_cosine_similarity", lambda seed: {"W": wts(seed, 100, 130)},
     lambda c: c.L.pt2q_cosine_similarity(c.p("W"), F32, 130, 100, 130, c.p("S"), 130, c.p("ws"), c.nbytes("ws"), c.st),
     ("S",), "test_gpu_static_reorder.py::test_bit_exact_against_restatement", out={"S": ((130, 130), f32)},
     ws={"ws": lambda L: L.pt2q_cosine_similarity_workspace_bytes(100, 130)}, status=("ws",))


def _cos(seed, n, m):
    W = synth.weights(seed, n, m)
    Wn = W / np.maximum(np.sqrt((W * W).sum(0)), 1e-8)
    return sym(Wn.T @ Wn)


case("ssr-static-order", "pt2q_ssr_static_order", lambda seed: {"S": t(_cos(seed, 100, 130))},
     lambda c: c.L.pt2q_ssr_static_order(c.p("S"), 130, 130, c.p("perm"), c.p("inv"), c.p("ws"), c.nbytes("ws"), c.st),
     ("perm", "inv"), "test_gpu_static_reorder.py::test_bit_exact_against_restatement",
     out={"perm": ((130,), i64), "inv": ((130,), i64)},
     ws={"ws": lambda L: L.pt2q_ssr_static_order_workspace_bytes(130)}, status=("ws",))

# ------------------------------------------------------------------ layer report
RN, RM, RB = 33, 31, 128   # test_gpu_layer_report.SMALL[0]


def _report_make(seed):
    rng = np.random.default_rng(seed)
    return {"W": wts(seed, RN, RM), "alpha": t(rng.random((RN, 1)) * 0.05 + 0.005, f32),
            "mu": t(rng.standard_normal((RN, 1)) * 0.002, f32), "T": t(rng.integers(-1, 2, (RN, RM)), i8),
            "perm": t(rng.permutation(RM).astype(np.int64)), "G": t(raw_gram(seed + 1, RM, 64))}


case("quadform-rows", "pt2q_quadform_rows", lambda seed: {"A": wts(seed, RN, RM), "G": t(raw_gram(seed + 1, RM, 64))},
     lambda c: c.L.pt2q_quadform_rows(c.p("A"), F32, RM, RN, RM, c.p("G"), RM, c.p("q"), c.p("total"), c.p("ws"),
                                      c.nbytes("ws"), c.st),
     ("q", "total"), "test_gpu_layer_report.py::test_random_cases_bit_equal", out={"q": ((RN,), f32), "total": ((1,), f32)},
     ws={"ws": lambda L: L.pt2q_quadform_rows_workspace_bytes(RN, RM)}, status=("ws",))
case("layer-report", "pt2q_layer_report", _report_make,
     lambda c: c.L.pt2q_layer_report(c.p("W"), F32, RM, RN, RM, RB, c.p("alpha"), c.p("mu"), c.p("T"), I8, RM,
                                     c.p("perm"), c.p("G"), RM, 0x1, c.p("ew"), c.p("ex"), c.p("ey"), c.p("totals"),
                                     c.p("ws"), c.nbytes("ws"), c.st),
     ("ew", "ex", "ey", "totals"), "test_gpu_layer_report.py::test_random_cases_bit_equal",
     out={"ew": ((RN,), f32), "ex": ((RN,), f32), "ey": ((RN,), f32), "totals": ((3,), f32)},
     ws={"ws": lambda L: L.pt2q_layer_report_workspace_bytes(RN, RM, 0x1)}, status=("ws",),
     index={"perm": ("range", 0, RM), "T": ("range", -1, 2)})

# ------------------------------------------------------------------ error feedback, dequantize
EN, EM = rc.EF[0][:2]


def _ef(bs):
    def make(seed):
        cols = np.random.default_rng(seed).permutation(EM).astype(np.int64)
        H = damped(raw_gram(seed + 2, EM, 2 * EM), 2 * EM)
        return {"W": wts(seed, EN, EM), "blk": t(cols[:bs]), "rem": t(cols[bs:]),
                "E": t(synth.weights(seed + 1, EN, bs) * np.float32(0.1)), "Hinv": t(inverse(H))}
    case("error-feedback-bs%d" % bs, "pt2q_error_feedback", make,
         lambda c: c.L.pt2q_error_feedback(c.p("W"), EM, EN, EM, c.p("blk"), bs, c.p("rem"), EM - bs, c.p("E"), bs,
                                           c.p("Hinv"), EM, c.p("ws"), c.nbytes("ws"), c.st),
         ("W",), "test_gpu_ragged.py::test_error_feedback_entry_odd_shapes",
         ws={"ws": lambda L: L.pt2q_error_feedback_workspace_bytes(EN, EM, bs)},
         index={"blk": ("range", 0, EM), "rem": ("range", 0, EM)},
         oracle=lambda i: {"W": orc.error_feedback(*[i[k].numpy() for k in ("W", "blk", "rem", "E", "Hinv")])})


_ef(50)
_ef(128)
DN, DM, DB = 67, 203, 64


def _deq_make(seed):
    rng = np.random.default_rng(seed)
    B = rc.ceil_div(DM, DB)
    return {"alpha": t(rng.random((DN, B)) * 0.05 + 0.005, f32), "mu": t(rng.standard_normal((DN, B)) * 0.002, f32),
            "T": t(rng.integers(-1, 2, (DN, DM)), i8), "perm": t(rng.permutation(DM).astype(np.int64))}


case("dequantize", "pt2q_dequantize", _deq_make,
     lambda c: c.L.pt2q_dequantize(c.p("alpha"), c.p("mu"), c.p("T"), I8, c.p("perm"), DN, DM, DB, c.p("out"), c.st),
     ("out",), "test_gpu_ternary.py::test_correct_forward_matches_reconstruction", out={"out": ((DN, DM), f32)},
     index={"perm": ("range", 0, DM), "T": ("range", -1, 2)})

# ------------------------------------------------------------------ packing, partial sums, synthetic fill
NCODES = 1001


def _codes(seed, count):
    return np.random.default_rng(seed).integers(-1, 2, count).astype(np.int8)


def _pack4(T):
    c = np.zeros(rc.round_up(len(T), 4), np.uint8)
    c[:len(T)] = T + 1
    c = c.reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


case("pack-ternary", "pt2q_pack_ternary", lambda seed: {"T": t(_codes(seed, NCODES))},
     lambda c: c.L.pt2q_pack_ternary(c.p("T"), NCODES, c.p("packed"), c.st), ("packed",),
     "test_gpu_parity.py::test_pack_unpack_matches_reference_layout", out={"packed": ((rc.ceil_div(NCODES, 4),), u8)},
     index={"T": ("range", -1, 2)})
case("unpack-ternary", "pt2q_unpack_ternary", lambda seed: {"packed": t(_pack4(_codes(seed, NCODES)))},
     lambda c: c.L.pt2q_unpack_ternary(c.p("packed"), NCODES, c.p("T"), c.st), ("T",),
     "test_gpu_parity.py::test_pack_unpack_matches_reference_layout", out={"T": ((NCODES,), i8)},
     index={"packed": ("codes2",)},
     oracle=lambda i: {"T": ((i["packed"].numpy()[:, None] >> np.arange(0, 8, 2)) & 3).reshape(-1)[:NCODES].astype(np.int8) - 1})
case("sum-partials", "pt2q_sum_partials", lambda seed: {"parts": wts(seed, 3, 1000)},
     lambda c: c.L.pt2q_sum_partials(c.p("parts"), 1000, 3, 1000, c.p("out"), c.st), ("out",),
     "test_gpu_strides.py::test_sum_partials_strided", out={"out": ((1000,), f32)},
     oracle=lambda i: {"out": orc.sum_partials(list(i["parts"].numpy()))})
FILL = (7, 130)
case("fill-synthetic", "pt2q_fill_synthetic", lambda seed: {"h_seed": seed},
     lambda c: c.L.pt2q_fill_synthetic(c.p("out"), FILL[0] * FILL[1], c.h("seed"), float(synth.scale_for_std(0.02)),
                                       FILL[1], 0, 0.0, c.st),
     ("out",), "test_gpu_parity.py::test_fill_synthetic_matches_numpy", out={"out": (FILL, f32)},
     oracle=lambda i: {"out": synth.weights(i["h_seed"], *FILL)})

# ------------------------------------------------------------------ ternary inference


def tern(seed, n, m, bs, tokens, dt, z=""):
    """A packed ternary layer and its activations (tests/ternary_decode_ref.make_case's value
    ranges; the packed codes and the gather index are tdr.pack's: valid whatever the seed)."""
    dn = "fp16" if dt == f16 else "bf16"
    rng = np.random.default_rng(seed)
    B = rc.ceil_div(m, bs)
    T, perm = rng.integers(-1, 2, (n, m)).astype(np.int8), rng.permutation(m).astype(np.int64)
    c, gather = tdr.pack(T, perm, False)
    return {"x": acts(seed + 1, tokens, m, dt), "codes" + z: t(tdr.packed_bytes(c)), "gather" + z: t(gather),
            "alpha" + z: t(tdr.round16(rng.random((n, B)) * 0.05 + 0.005, dn), f32),
            "mu" + z: t(tdr.round16(rng.standard_normal((n, B)) * 0.002, dn), f32),
            "bias" + z: t(tdr.round16(rng.standard_normal(n) * 0.1, dn), f32)}


def tern_index(m, zs=("",)):
    d = {}
    for z in zs:
        d.update({"codes" + z: ("codes2",), "gather" + z: ("range", -1, m)})
    return d


def _tpack(mode):
    n, m = 40, 200
    P = tdr.positions(m)

    def make(seed):
        rng = np.random.default_rng(seed)
        return {"T": t(rng.integers(-1, 2, (n, m)), i8), "perm": t(rng.permutation(m).astype(np.int64))}

    def oracle(i):
        c, g = tdr.pack(i["T"].numpy(), i["perm"].numpy(), bool(mode))
        return {"codes": tdr.packed_bytes(c), "gather": g}
    case("ternary-pack-mode%d" % mode, "pt2q_ternary_pack", make,
         lambda c: c.L.pt2q_ternary_pack(c.p("T"), m, n, m, c.p("perm"), mode, c.p("codes"), c.p("gather"), c.st),
         ("codes", "gather"), "test_gpu_ternary_decode.py::test_pack_matches_restated_layout",
         out={"codes": ((n, P // 4), u8), "gather": ((P,), i32)},
         index={"T": ("range", -1, 2), "perm": ("range", 0, m)}, oracle=oracle)


_tpack(0)
_tpack(1)
TLN, TLM, TLBS, TLTOK = 384, 512, 128, 5
case("ternary-linear", "pt2q_ternary_linear", lambda seed: tern(seed, TLN, TLM, TLBS, TLTOK, f16),
     lambda c: c.L.pt2q_ternary_linear(c.p("x"), F16, TLTOK, TLM, TLN, TLM, c.p("codes"), c.p("gather"), c.p("alpha"),
                                       c.p("mu"), TLM // TLBS, TLBS, c.p("bias"), c.p("y"), F16, TLN, c.p("ws"),
                                       c.nbytes("ws"), c.st),
     ("y",), "test_gpu_ternary_linear_exact.py::test_exact_gemm",
     out={"y": ((TLTOK, TLN), f16)}, ws={"ws": lambda L: L.pt2q_ternary_linear_workspace_bytes(TLTOK, TLN, TLM)},
     index=tern_index(TLM))


def _decode(n, m, bs, tokens, dt):
    case("ternary-decode-%dtok" % tokens, "pt2q_ternary_decode", lambda seed: tern(seed, n, m, bs, tokens, dt),
         lambda c: c.L.pt2q_ternary_decode(c.p("x"), CODE[dt], tokens, m, n, m, c.p("codes"), c.p("gather"),
                                           c.p("alpha"), c.p("mu"), rc.ceil_div(m, bs), bs, c.p("bias"), c.p("y"),
                                           CODE[dt], n, c.st),
         ("y",), "test_gpu_ternary_decode.py::test_bit_exact_vs_restatement", out={"y": ((tokens, n), dt)},
         index=tern_index(m))


_decode(33, 100, 16, 1, f16)
_decode(40, 1030, 64, 8, bf16)


def _group(id, entry, ns, m, bs, tokens, dt, epilogue, pinned, fused=False):
    zs = [str(z) for z in range(len(ns))]
    ys = zs[:1] if epilogue else zs
    B = rc.ceil_div(m, bs)

    def make(seed):
        d = {}
        for z, n in zip(zs, ns):
            d.update(tern(seed + 10 * int(z), n, m, bs, tokens, dt, z))
        d["x"] = acts(seed + 1, tokens, m, dt)
        if fused:
            d["nw"] = t(1.0 + synth.weights(seed + 2, 1, m)[0] * np.float32(5.0), dt)
            for z, n in zip(ys, ns):
                d["res" + z] = acts(seed + 3 + int(z), tokens, n, dt)
        return d

    def call(c):
        a = lambda k, names=zs: c.arr(*[k + z for z in names])  # noqa: E731
        args = (c.p("x"), CODE[dt], tokens, m, m, len(ns), c.ints(ns), a("codes"), a("gather"), a("alpha"), a("mu"),
                c.ints([B] * len(ns)), bs, a("bias"), a("y", ys), CODE[dt], c.ints([ns[int(z)] for z in ys], ctypes.c_int64),
                epilogue)
        if not fused:
            return c.L.pt2q_ternary_decode_group(*args, c.st)
        return c.L.pt2q_ternary_decode_fused(*args, c.p("nw"), 1e-5, a("res", ys),
                                             c.ints([ns[int(z)] for z in ys], ctypes.c_int64), c.st)
    case(id, entry, make, call, tuple("y" + z for z in ys), pinned,
         out={"y" + z: ((tokens, ns[int(z)]), dt) for z in ys}, index=tern_index(m, zs))


_group("decode-group-plain3", "pt2q_ternary_decode_group", (40, 33, 24), 200, 64, 3, f16, 0,
       "test_gpu_ternary_group.py::test_plain_group_is_the_members_alone")
_group("decode-group-swiglu", "pt2q_ternary_decode_group", (40, 40), 200, 64, 2, bf16, 1,
       "test_gpu_ternary_group.py::test_swiglu_bit_exact_vs_restatement")
_group("decode-fused-norm-residual", "pt2q_ternary_decode_fused", (40, 33), 200, 64, 2, f16, 0,
       "test_gpu_ternary_norm.py::test_norm_and_residual_together", fused=True)
NT, NM = 3, 1030
case("rmsnorm", "pt2q_rmsnorm",
     lambda seed: {"x": acts(seed, NT, NM, bf16), "w": t(1.0 + synth.weights(seed + 1, 1, NM)[0] * np.float32(5.0), bf16)},
     lambda c: c.L.pt2q_rmsnorm(c.p("x"), BF16, NT, NM, NM, c.p("w"), 1e-5, c.p("y"), NM, c.st), ("y",),
     "test_gpu_ternary_norm.py::test_rms_norm_bit_exact", out={"y": ((NT, NM), bf16)})

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
