"""The C ABI (include/pt2q.h) with padded leading dimensions and unaligned base pointers.

The Python bindings always pass contiguous, freshly allocated tensors, so ld == cols and every
base is 256-byte aligned.  Here every entry that takes an `ld*` argument is called directly
(pt2q._lib.lib().pt2q_*) on operands that live inside one flat guarded buffer:

    [ guard | lead elements | rows x ld (the logical rows x cols window in its first columns) | guard ]

filled with a sentinel (inputs: a NaN with a recognisable payload, so padding that reaches a
result shows in it; outputs: a fixed bit pattern no kernel produces).  Every case asserts that
  1. the rows x cols window of every output is bit-identical to the CPU oracle run on the
     contiguous logical arrays (ternary inference: the tolerance of test_gpu_ternary.py),
  2. every pad column, lead element and guard element of every output still holds its sentinel,
  3. the input buffers are unchanged.
Variants: (a) ld padded and still vector-aligned (the fast path reads padded rows), (b) odd ld,
(c) base offset by one element with an aligned ld, (d) input and output lds varied independently.
Each docstring names the kernel path the launch code takes for each variant."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import synth
from oracle import oracle as orc
from test_gpu_parity import bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 4096  # least number of elements before and after the operand (>= 4 KiB for every type)
E_UNSUPPORTED = 3
F16, BF16 = torch.float16, torch.bfloat16
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def sentinel(dtype, out):
    """Bit pattern (as a signed integer of the element's width) that fills pads and guards."""
    if dtype == torch.float32:
        return 0x7FA5C3E1 if out else 0x7FC0BEEF  # out: a non-canonical pattern; in: quiet NaN, payload BEEF
    if dtype == F16:
        return 0x7EEF  # fp16 NaN
    if dtype == BF16:
        return 0x7FEF  # bf16 NaN
    if dtype in (torch.int8, torch.uint8):
        return 0x55    # outside {-1, 0, 1}
    return -0x5A5A5A5B  # int32 / int64: a fixed negative value


class Pad:
    """A (batch x) rows x cols operand with leading dimension ld (and item stride istride),
    `lead` elements after a guard inside one flat sentinel-filled device buffer."""

    def __init__(self, shape, ld, dtype, data=None, lead=0, istride=None, out=False):
        batch, rows, cols = shape if len(shape) == 3 else (1,) + tuple(shape)
        assert ld >= cols
        istride = rows * ld if istride is None else istride
        span = (batch - 1) * istride + rows * ld
        self.dtype, self.sent = dtype, sentinel(dtype, out)
        # (16 elements per row: a kernel that took another operand's ld for this one stays inside)
        guard = max(GUARD, 16 * rows * batch)
        self.ibuf = torch.full((guard + lead + span + guard,), self.sent, dtype=_INT[dtype.itemsize], device=DEV)
        self.buf = self.ibuf.view(dtype)
        self.geom = ((batch, rows, cols), (istride, ld, 1), guard + lead)
        self.batched = len(shape) == 3
        v = self.buf.as_strided(*self.geom)
        if data is not None:
            t = torch.as_tensor(data)
            assert t.dtype == dtype, (t.dtype, dtype)
            v.copy_(t.reshape(batch, rows, cols).to(DEV))
        self.view = v if self.batched else v[0]
        self.ptr = self.view.data_ptr()
        self.snap = self.ibuf.clone()

    @property
    def p(self):
        return ctypes.c_void_p(self.ptr)

    def item_ptr(self, z):
        return self.buf.as_strided(*self.geom)[z].data_ptr()

    def win(self):
        """The logical window on the host (numpy; bf16 as a torch CPU tensor)."""
        t = self.view.cpu()
        return t if self.dtype == BF16 else t.numpy()

    def iwin(self):
        """The window's raw bits (integer tensor, device)."""
        v = self.ibuf.as_strided(*self.geom)
        return v if self.batched else v[0]

    def pads_intact(self):
        c = self.ibuf.clone()
        c.as_strided(*self.geom).fill_(self.sent)
        return bool((c == self.sent).all())

    def untouched(self):
        return torch.equal(self.ibuf, self.snap)


def vec(n, dtype, data=None, out=False, lead=0):
    return Pad((1, n), n, dtype, data=data, lead=lead, out=out)


def outs_ok(*pads):
    return all(p.pads_intact() for p in pads)


def ins_ok(*pads):
    return all(p.untouched() for p in pads)


def parr(ptrs):
    """A host array of device pointers (the grouped entries' pointer-array arguments)."""
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def env(pt2q):
    L = pt2q._lib
    return L, L.lib(), L.stream_of(torch.device("cuda", torch.cuda.current_device()))


def to16(a, dt):
    """fp32 numpy -> (device payload, oracle operand) of a 16-bit type."""
    if dt == F16:
        h = a.astype(np.float16)
        return torch.from_numpy(h), h
    t = torch.from_numpy(np.ascontiguousarray(a)).bfloat16()
    return t, t


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


# ------------------------------------------------------------------ pt2q_gram

@functools.lru_cache(maxsize=None)
def _gram_f32_ref():
    X0, X = synth.activations(901, 16, 100), synth.activations(902, 70, 100)
    G0, GX = orc.gram(X0), orc.gram(X)
    return X, G0, {0: GX, 1: (G0 + GX).astype(np.float32), 2: orc.gram(np.concatenate([X0, X]))}


@pytest.mark.parametrize("ldx,ldg,lead", [(104, 104, 0), (101, 101, 0), (104, 104, 1), (104, 101, 0),
                                          (101, 108, 0)])
def test_gram_f32(pt2q, ldx, ldg, lead):
    """N = 70, m = 100, every accumulate mode (pt2q_launch_gram -> pt2q_launch_gemm -> launch_dt:
    one 128-tile, so gemm_kernel<64, 64, float, VEC>).  VEC (vec_ok: 16-byte X, ldx % 4, m % 4) and
    the 16-byte C stores (cvec: 16-byte G, ldg % 4) are chosen independently:
    (104, 104): VEC loads + cvec stores over padded rows; (101, 101): scalar loads and stores;
    lead = 1 (4-byte aligned X and G): scalar both; (104, 101): VEC loads, scalar stores;
    (101, 108): scalar loads, cvec stores.  Modes 1 / 2 read the old G window (pads are NaN)."""
    L, lib, st = env(pt2q)
    Xh, G0, refs = _gram_f32_ref()
    X = Pad(Xh.shape, ldx, torch.float32, f32(Xh), lead)
    for mode in (0, 1, 2):
        G = Pad((100, 100), ldg, torch.float32, f32(G0) if mode else None, lead, out=True)
        L.check(lib.pt2q_gram(X.p, 0, 70, 100, ldx, G.p, ldg, mode, None, 0, st), "pt2q_gram")
        assert bits_equal(G.win(), refs[mode]), mode
        assert outs_ok(G) and ins_ok(X), mode


@functools.lru_cache(maxsize=None)
def _gram16_small_ref(dt, m):
    X0, X = synth.activations(911, 16, m), synth.activations(912 + m, 77, m)
    (d0, o0), (d1, o1) = to16(X0, dt), to16(X, dt)
    G0, GX = orc.gram16(o0), orc.gram16(o1)
    return d1, G0, {0: GX, 1: (G0 + GX).astype(np.float32), 2: orc.gram16(o1, G=G0)}


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("m,ldx,ldg,lead", [(136, 144, 140, 0), (136, 139, 137, 0), (136, 144, 140, 1),
                                            (136, 144, 137, 0), (136, 139, 140, 0), (130, 136, 136, 0)])
def test_gram16_small(pt2q, dt, m, ldx, ldg, lead):
    """N = 77 (a ragged last MFMA group), no workspace: pt2q_launch_gram16 without the split, one
    gram16x_kernel<BF16, DMA> workgroup per tile.  DMA (LDS-DMA staging: 16-byte X, ldx % 8,
    m % 8) and vec4 (float4 mirror stores: 16-byte G, ldg % 4):
    m = 136, (144, 140): DMA + vec4; (139, 137): register-staged + scalar mirror; lead = 1 (2-byte
    aligned X, 4-byte aligned G): register-staged + scalar; (144, 137): DMA + scalar mirror;
    (139, 140): register-staged + vec4; m = 130 with ldx = 136: an aligned ld, but m % 8 != 0 keeps
    the register-staged path.  All three accumulate modes (mode 2 continues a 16-row batch)."""
    L, lib, st = env(pt2q)
    Xd, G0, refs = _gram16_small_ref(dt, m)
    X = Pad((77, m), ldx, dt, Xd, lead)
    for mode in (0, 1, 2):
        G = Pad((m, m), ldg, torch.float32, f32(G0) if mode else None, lead, out=True)
        L.check(lib.pt2q_gram(X.p, L.dtype_code(X.buf), 77, m, ldx, G.p, ldg, mode, None, 0, st), "pt2q_gram")
        assert bits_equal(G.win(), refs[mode]), mode
        assert outs_ok(G) and ins_ok(X), mode


@functools.lru_cache(maxsize=None)
def _gram16_split_ref():
    orc.set_threads(16)
    Xd, Xo = to16(synth.activations(921, 40, 4096), F16)
    ref = orc.gram16(Xo)
    return Xd, ref, orc.gram16(Xo[:8]), orc.gram16(Xo[8:], G=orc.gram16(Xo[:8]))


@pytest.mark.parametrize("ldx,ldg,lead", [(4104, 4100, 0), (4104, 4097, 0), (4099, 4100, 0), (4104, 4100, 1)])
def test_gram16_split(pt2q, ldx, ldg, lead):
    """m = 4096, N = 40, fp16, workspace given: gx_ntile(4096) = 272 tiles >= one per CU, so the
    balanced split of gram16x_kernel runs (136 256-wide tiles are fewer than the two waves the
    256 x 256 kernel wants).  (4104, 4100): DMA staging + vec4 mirror stores; (4104, 4097): the
    split and the DMA stay (neither reads ldg), the mirror stores turn scalar; (4099, 4100):
    register-staged operands; lead = 1: register-staged and scalar stores.  The status word must
    stay zero (no stalled hand-off).  Then accumulate = 2 on the last 32 rows from the Gram of the
    first 8 (the split stays in CHAIN_POS mode: every piece first loads its tile of G through ldg)
    must give the same bits as the one-launch Gram."""
    L, lib, st = env(pt2q)
    Xd, ref, ref8, ref_cont = _gram16_split_ref()
    X = Pad((40, 4096), ldx, F16, Xd, lead)
    G = Pad((4096, 4096), ldg, torch.float32, None, lead, out=True)
    ws = L.workspace(lib.pt2q_gram_workspace_bytes(4096), DEV)
    L.check(lib.pt2q_gram(X.p, 1, 40, 4096, ldx, G.p, ldg, 0, L.ptr(ws), ws.numel(), st), "pt2q_gram")
    L.check_status(ws, "pt2q_gram")
    assert bits_equal(G.win(), ref)
    assert outs_ok(G) and ins_ok(X)
    assert bits_equal(ref_cont, ref)  # (the oracle's own continue guarantee: 8-row first batch)
    G.view.copy_(f32(ref8).to(DEV))
    X8 = ctypes.c_void_p(X.ptr + 8 * ldx * 2)
    L.check(lib.pt2q_gram(X8, 1, 32, 4096, ldx, G.p, ldg, 2, L.ptr(ws), ws.numel(), st), "pt2q_gram")
    L.check_status(ws, "pt2q_gram")
    assert bits_equal(G.win(), ref_cont)
    assert outs_ok(G) and ins_ok(X)


def test_gram16_wide_tiles_padded(pt2q):
    """m = 8192, N = 40, bf16, workspace, ldx = 8200, ldg = 8196: 528 tiles of 256 x 256 are two
    waves of 256 workgroups, so gram16w_kernel runs (gram16.hip: split && dma && m % 256 == 0 &&
    ntw >= 2 NG R && 16-byte G && ldg % 4 == 0).  Compared with the oracle on sampled column
    blocks; the whole window must be symmetric and the pads intact."""
    from test_gpu_configs import sample_cols
    L, lib, st = env(pt2q)
    m, N, ldx, ldg = 8192, 40, 8200, 8196
    Xd, _ = to16(synth.activations(931, N, m), BF16)
    X = Pad((N, m), ldx, BF16, Xd)
    G = Pad((m, m), ldg, torch.float32, None, out=True)
    ws = L.workspace(lib.pt2q_gram_workspace_bytes(m), DEV)
    L.check(lib.pt2q_gram(X.p, 2, N, m, ldx, G.p, ldg, 0, L.ptr(ws), ws.numel(), st), "pt2q_gram")
    L.check_status(ws, "pt2q_gram")
    assert torch.equal(G.iwin(), G.iwin().T)
    orc.set_threads(16)
    S = sample_cols(m)
    St = torch.from_numpy(S).to(DEV)
    got = G.view[St][:, St].cpu().numpy()
    assert bits_equal(got, orc.gram16(Xd[:, torch.from_numpy(S)].contiguous()))
    assert outs_ok(G) and ins_ok(X)


# ------------------------------------------------------------------ pt2q_gram_batched[_upper]

@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("upper", [False, True])
def test_gram16_batched_padded(pt2q, dt, upper):
    """m = 256, N = 72, two items, ldx = 264 (a multiple of 8, 16-byte aligned X[z]):
    gram16b_kernel, one 256 x 256 tile per item reading padded rows.  Each item bit-equal to the
    oracle's 16-bit Gram; _upper leaves the strictly lower part of G as it was.  ldx = 260 and an
    X[z] offset by one element are refused (PT2Q_E_UNSUPPORTED) before any launch: G untouched."""
    L, lib, st = env(pt2q)
    m, N = 256, 72
    fn = lib.pt2q_gram_batched_upper if upper else lib.pt2q_gram_batched
    hosts = [to16(synth.activations(941 + z, N, m), dt) for z in range(2)]
    Xs = [Pad((N, m), 264, dt, h[0]) for h in hosts]
    G = Pad((2, m, m), m, torch.float32, None, out=True)
    arr, keep = parr([x.ptr for x in Xs])
    L.check(fn(2, arr, L.dtype_code(Xs[0].buf), N, m, 264, G.p, st), "pt2q_gram_batched")
    got, bits = G.win(), G.iwin().cpu().numpy()
    for z in range(2):
        ref = orc.gram16(hosts[z][1])
        if upper:
            iu = np.triu_indices(m)
            assert bits_equal(got[z][iu], ref[iu]), z
            assert (bits[z][np.tril_indices(m, -1)] == G.sent).all(), z
        else:
            assert bits_equal(got[z], ref), z
    assert outs_ok(G) and ins_ok(*Xs)
    # refused operands: nothing may be launched
    G2 = Pad((2, m, m), m, torch.float32, None, out=True)
    X260 = [Pad((N, m), 260, dt, h[0]) for h in hosts]
    arr, keep = parr([x.ptr for x in X260])
    assert fn(2, arr, L.dtype_code(Xs[0].buf), N, m, 260, G2.p, st) == E_UNSUPPORTED
    Xoff = [Xs[0], Pad((N, m), 264, dt, hosts[1][0], lead=1)]
    arr, keep = parr([x.ptr for x in Xoff])
    assert fn(2, arr, L.dtype_code(Xs[0].buf), N, m, 264, G2.p, st) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert G2.untouched()


@pytest.mark.parametrize("ldx,lead", [(104, 0), (101, 0), (104, 1)])
def test_gram_f32_batched_padded(pt2q, ldx, lead):
    """fp32 items, m = 100, N = 70, batch 2 ("any m" in pt2q.h).  ldx = 104 with aligned bases:
    gemmx_gram_kernel (LDS-DMA, reads padded rows); ldx = 101 or a 4-byte aligned base:
    pt2q_launch_gemmx_gram refuses and pt2q_launch_gram_f32_batched falls back to
    gram_f32_batched_kernel<64, 64, VEC = false> -- a working scalar path, bit-identical."""
    L, lib, st = env(pt2q)
    m, N = 100, 70
    hosts = [synth.activations(951 + z, N, m) for z in range(2)]
    Xs = [Pad((N, m), ldx, torch.float32, f32(h), lead if z == 1 else 0) for z, h in enumerate(hosts)]
    G = Pad((2, m, m), m, torch.float32, None, out=True)
    arr, keep = parr([x.ptr for x in Xs])
    L.check(lib.pt2q_gram_batched(2, arr, 0, N, m, ldx, G.p, st), "pt2q_gram_batched")
    got = G.win()
    for z in range(2):
        assert bits_equal(got[z], orc.gram(hosts[z])), z
    assert outs_ok(G) and ins_ok(*Xs)


# ------------------------------------------------------------------ Hessian, Cholesky inverse

@functools.lru_cache(maxsize=None)
def _hessian_ref(m):
    orc.set_threads(16)
    N = m + 60
    G = orc.gram(synth.activations(961 + m, N, m))
    H, damp = orc.prepare_hessian(G, N, 0.01)
    return N, G, H, damp


@pytest.mark.parametrize("m", [100, 64])
@pytest.mark.parametrize("dg,dh,lead", [(4, 4, 0), (1, 1, 0), (4, 4, 1), (4, 1, 0), (1, 8, 0)])
def test_prepare_hessian(pt2q, m, dg, dh, lead):
    """ldg = m + dg, ldh = m + dh.  With damp_dev: hess_diag_damp_kernel, then hess_fill4_kernel
    when m, ldg, ldh are multiples of 4 and G, H 16-byte aligned -- (4, 4) -- else
    hess_fill_kernel: (1, 1), lead = 1, (4, 1), (1, 8).  damp_dev = NULL (documented nullable):
    the hess_scale_kernel + hess_damp_kernel pair that otherwise runs only for m > 12288."""
    L, lib, st = env(pt2q)
    N, Gh, Href, dref = _hessian_ref(m)
    G = Pad((m, m), m + dg, torch.float32, f32(Gh), lead)
    for with_damp in (True, False):
        H = Pad((m, m), m + dh, torch.float32, None, lead, out=True)
        damp = vec(1, torch.float32, out=True)
        L.check(lib.pt2q_prepare_hessian(G.p, m + dg, m, N, 0.01, H.p, m + dh, damp.p if with_damp else None, st),
                "pt2q_prepare_hessian")
        assert bits_equal(H.win(), Href), with_damp
        if with_damp:
            assert np.float32(damp.win()[0, 0]) == np.float32(dref)
        else:
            assert damp.untouched()
        assert outs_ok(H, damp) and ins_ok(G), with_damp


@functools.lru_cache(maxsize=None)
def _inverse_ref(m):
    if m > 1000:  # a cheap well-conditioned SPD matrix: a rank-128 Gram plus the identity
        orc.set_threads(16)
        H = (orc.gram(synth.activations(961 + m, 128, m)) / np.float32(128) + np.eye(m, dtype=np.float32))
        H = H.astype(np.float32)
    else:
        H = _hessian_ref(m)[2]
    Hinv, spd = orc.cholesky_inverse(H)
    assert spd
    return H, Hinv


def _cholesky_case(pt2q, m, ldh, ldhi, lead):
    L, lib, st = env(pt2q)
    Hh, ref = _inverse_ref(m)
    H = Pad((m, m), ldh, torch.float32, f32(Hh), lead)
    Hinv = Pad((m, m), ldhi, torch.float32, None, lead, out=True)
    info = vec(1, torch.int32, out=True)
    ws = L.workspace(lib.pt2q_cholesky_workspace_bytes(m), DEV)
    L.check(lib.pt2q_cholesky_inverse(H.p, ldh, m, Hinv.p, ldhi, L.ptr(ws), ws.numel(), info.p, st),
            "pt2q_cholesky_inverse")
    assert int(info.win()[0, 0]) == 0
    assert bits_equal(Hinv.win(), ref)
    assert outs_ok(Hinv, info) and ins_ok(H)


@pytest.mark.parametrize("m", [100, 384])
@pytest.mark.parametrize("dh,dhi,lead", [(4, 4, 0), (1, 1, 0), (4, 4, 1), (4, 1, 0), (1, 8, 0)])
def test_cholesky_inverse(pt2q, m, dh, dhi, lead):
    """ldh = m + dh feeds copy_upper_kernel only (scalar; U and Ui are packed in the workspace).
    ldhi = m + dhi is the ldc of the final Ui Uiᵀ product: at these m launch_big has fewer than 64
    tiles, so it is gemm_kernel<64, 64, float, VEC = true> (Ui is aligned) whose C stores are
    16-byte (cvec) for (., 4), (., 8) and scalar for an odd ldhi or lead = 1.  m = 100: one ragged
    block; m = 384: six 64-blocks with rank-64 strip updates and a sub-panel term."""
    _cholesky_case(pt2q, m, m + dh, m + dhi, lead)


@pytest.mark.parametrize("dhi", [4, 1])
def test_cholesky_inverse_gemmx_product(pt2q, dhi):
    """m = 1536: 72 upper 128-tiles, so launch_big sends the final Ui Uiᵀ product to gemmx_kernel
    when ldhi % 4 == 0 and Hinv is 16-byte aligned (ldhi = m + 4: padded C rows), and off it to
    gemm_kernel for ldhi = m + 1.  ldh = m + 4."""
    _cholesky_case(pt2q, 1536, 1540, 1536 + dhi, 0)


def test_cholesky_breakdown_padded(pt2q):
    """test_cholesky_breakdown_reports_and_falls_back's matrix (identity, H[37][37] = -1) with
    ldh = 84, ldhi = 81: info_dev = k + 1 = 38; Hinv is undefined but its pads must survive."""
    L, lib, st = env(pt2q)
    Hh = np.eye(80, dtype=np.float32)
    Hh[37, 37] = -1.0
    H = Pad((80, 80), 84, torch.float32, f32(Hh))
    Hinv = Pad((80, 80), 81, torch.float32, None, out=True)
    info = vec(1, torch.int32, out=True)
    ws = L.workspace(lib.pt2q_cholesky_workspace_bytes(80), DEV)
    L.check(lib.pt2q_cholesky_inverse(H.p, 84, 80, Hinv.p, 81, L.ptr(ws), ws.numel(), info.p, st),
            "pt2q_cholesky_inverse")
    assert int(info.win()[0, 0]) == 38
    assert outs_ok(Hinv, info) and ins_ok(H)


# ------------------------------------------------------------------ S1 = S·1, d = 1ᵀS1

@functools.lru_cache(maxsize=None)
def _s1_ref(m, z):
    """A Gram and its S1 / d: orc.rowsum_seq on the Gram (the l-ascending row sums and the
    j-ascending total), cross-checked on the host against orc.s1_from_x on the activations."""
    orc.set_threads(16)
    X = synth.activations(971 + m + z, 24, m)
    G = orc.gram(X)
    S1 = orc.rowsum_seq(G)
    d = orc.rowsum_seq(S1[None, :])[0]
    S1x, dx = orc.s1_from_x(X)
    assert bits_equal(S1, S1x) and np.float32(d) == np.float32(dx)
    return G, np.concatenate([S1, [d]]).astype(np.float32)


@pytest.mark.parametrize("m,dl,ds,lead", [
    (516, 4, 8, 0),    # s1_ring_kernel
    (516, 1, 8, 0),    # s1_rows_kernel (lds % 4)
    (516, 4, 5, 0),    # s1_rows_kernel (item stride % 4)
    (516, 4, 8, 1),    # s1_rows_kernel (4-byte aligned base)
    (518, 4, 6, 0),    # s1_rows_kernel (m % 4)
    (300, 4, 8, 0), (300, 1, 3, 1),    # s1_row_wg_kernel
    (100, 4, 8, 0), (100, 1, 3, 1)])   # s1_fused_kernel
def test_s1_from_gram(pt2q, m, dl, ds, lead):
    """pt2q_s1_from_gram_batched on two Grams with lds = m + dl and item_stride = lds m + ds (the
    gap between the items is NaN), then pt2q_s1_from_gram on item 1 alone.  Batched paths
    (pt2q_launch_s1, S1_GRAMS; grid.y = item) as annotated on the cases: m > 512 takes
    s1_ring_kernel only with m, lds, item_stride multiples of 4 and a 16-byte base, else
    s1_rows_kernel; 128 < m <= 512: s1_row_wg_kernel; m <= 128: s1_fused_kernel.  The single entry
    (S1_BLOCK): s1_rows_kernel / s1_row_wg_kernel / s1_fused_kernel by m alone."""
    L, lib, st = env(pt2q)
    lds = m + dl
    istride = lds * m + ds
    refs = [_s1_ref(m, z) for z in range(2)]
    S = Pad((2, m, m), lds, torch.float32, f32(np.stack([r[0] for r in refs])), lead, istride)
    S1d = Pad((2, m + 1), m + 1, torch.float32, None, out=True)
    L.check(lib.pt2q_s1_from_gram_batched(S.p, lds, m, 2, istride, S1d.p, st), "pt2q_s1_from_gram_batched")
    got = S1d.win()
    for z in range(2):
        assert bits_equal(got[z], refs[z][1]), z
    S1, d = vec(m, torch.float32, out=True), vec(1, torch.float32, out=True)
    L.check(lib.pt2q_s1_from_gram(ctypes.c_void_p(S.item_ptr(1)), lds, m, S1.p, d.p, st), "pt2q_s1_from_gram")
    assert bits_equal(S1.win()[0], refs[1][1][:m]) and bits_equal(d.win()[0], refs[1][1][m:])
    assert outs_ok(S1d, S1, d) and ins_ok(S)


def test_s1_from_upper(pt2q):
    """pt2q_s1_from_upper_batched, m = 516, lds = 520, item_stride = lds m + 8, two items whose
    strictly lower triangles are NaN (s1_upper_ring_kernel must take those entries from the upper
    triangle).  An odd lds, an odd item stride and a 4-byte aligned base are refused
    (PT2Q_E_UNSUPPORTED) with S1d untouched."""
    L, lib, st = env(pt2q)
    m, lds = 516, 520
    istride = lds * m + 8
    refs = [_s1_ref(m, z) for z in range(2)]
    S = Pad((2, m, m), lds, torch.float32, f32(np.stack([r[0] for r in refs])), 0, istride)
    lo = torch.tril(torch.ones(m, m, dtype=torch.bool, device=DEV), -1)
    S.iwin()[lo.expand(2, m, m)] = S.sent
    S.snap = S.ibuf.clone()
    S1d = Pad((2, m + 1), m + 1, torch.float32, None, out=True)
    L.check(lib.pt2q_s1_from_upper_batched(S.p, lds, m, 2, istride, S1d.p, st), "pt2q_s1_from_upper_batched")
    got = S1d.win()
    for z in range(2):
        assert bits_equal(got[z], refs[z][1]), z
    assert outs_ok(S1d) and ins_ok(S)
    out2 = Pad((2, m + 1), m + 1, torch.float32, None, out=True)
    for ld2, is2, lead in ((517, 517 * m + 7, 0), (520, 520 * m + 5, 0), (520, 520 * m + 8, 1)):
        S2 = Pad((2, m, m), ld2, torch.float32, None, lead, is2)
        assert lib.pt2q_s1_from_upper_batched(S2.p, ld2, m, 2, is2, out2.p, st) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert out2.untouched()


# ------------------------------------------------------------------ pt2q_atq_stage

STAGE_ITF, STAGE_FULL = 3, 5


@functools.lru_cache(maxsize=None)
def _atq_ref(n, b):
    orc.set_threads(16)
    W = synth.weights(981 + b, n, b)
    X = synth.activations(982 + b, 96, b)
    S1, d = orc.s1_from_x(X)
    return W, S1, np.float32(d), orc.atq_quantize(W, X), orc.atq_quantize(W)


@pytest.mark.parametrize("n,b", [(70, 128), (64, 777)])
@pytest.mark.parametrize("dw,dt_,lead", [(4, 4, 0), (1, 1, 0), (4, 4, 1), (4, 1, 0), (1, 8, 0)])
def test_atq_stage_full(pt2q, n, b, dw, dt_, lead):
    """PT2Q_STAGE_FULL with S1 / d (init + ITF + AGA) and without (S1 = NULL), ldw = b + dw,
    ldt = b + dt_.  b = 128: atq_stage_kernel<8>, two passes (dispatch_ns); b = 777 > 512:
    atq_wide_stage_kernel, two passes, one lane per row.  Neither launch chooses a kernel by
    alignment: every variant runs the same kernel with per-element row addressing through
    ldw / ldt, so a stride mix-up shows as NaN (pads) in alpha / mu / T."""
    L, lib, st = env(pt2q)
    Wh, S1h, dh, ref_x, ref_0 = _atq_ref(n, b)
    W = Pad((n, b), b + dw, torch.float32, f32(Wh), lead)
    S1, d = vec(b, torch.float32, f32(S1h)), vec(1, torch.float32, f32(np.array([dh])))
    for aga, (ra, rm, rT, rit) in ((True, ref_x), (False, ref_0)):
        a, mu = vec(n, torch.float32, out=True), vec(n, torch.float32, out=True)
        T = Pad((n, b), b + dt_, torch.float32, None, lead, out=True)
        it = vec(1, torch.int32, out=True)
        ws = L.workspace(256, DEV)
        L.check(lib.pt2q_atq_stage(STAGE_FULL, W.p, b + dw, n, b, a.p, mu.p, T.p, b + dt_, S1.p if aga else None,
                                   d.p if aga else None, 100, it.p, L.ptr(ws), ws.numel(), st), "pt2q_atq_stage")
        assert bits_equal(a.win()[0], ra[:, 0]) and bits_equal(mu.win()[0], rm[:, 0]), aga
        assert np.array_equal(T.win(), rT) and int(it.win()[0, 0]) == rit, aga
        assert outs_ok(a, mu, T, it) and ins_ok(W, S1, d), aga


@pytest.mark.parametrize("n,b,dw,dt_", [(70, 128, 4, 8), (70, 128, 1, 3), (64, 777, 3, 1)])
def test_atq_stage_itf_reads_padded_t(pt2q, n, b, dw, dt_):
    """PT2Q_STAGE_ITF: T is an input (the init codes) read through ldt = b + dt_ by
    count_zero_rows_kernel and by the ITF kernel (atq_stage_kernel<8> / atq_wide_stage_kernel),
    then overwritten in place; alpha / mu are in-out."""
    L, lib, st = env(pt2q)
    Wh = _atq_ref(n, b)[0]
    a0, m0, T0 = orc.ternary_init(Wh)
    ra, rm, rT, rit = orc.iterative_ternary_fitting(Wh, a0, m0, T0)
    W = Pad((n, b), b + dw, torch.float32, f32(Wh))
    a, mu = vec(n, torch.float32, f32(a0[:, 0]), out=True), vec(n, torch.float32, f32(m0[:, 0]), out=True)
    T = Pad((n, b), b + dt_, torch.float32, f32(T0), out=True)
    it = vec(1, torch.int32, out=True)
    ws = L.workspace(256, DEV)
    L.check(lib.pt2q_atq_stage(STAGE_ITF, W.p, b + dw, n, b, a.p, mu.p, T.p, b + dt_, None, None, 100, it.p,
                               L.ptr(ws), ws.numel(), st), "pt2q_atq_stage")
    assert bits_equal(a.win()[0], ra[:, 0]) and bits_equal(mu.win()[0], rm[:, 0])
    assert np.array_equal(T.win(), rT) and int(it.win()[0, 0]) == rit
    assert outs_ok(a, mu, T, it) and ins_ok(W)


# ------------------------------------------------------------------ pt2q_ssr_select

@pytest.mark.parametrize("subset", [False, True])
@pytest.mark.parametrize("ldw,lead", [(704, 0), (701, 0), (704, 1)])
def test_ssr_select(pt2q, subset, ldw, lead):
    """n = 256, m = 700, b = 128; rem = every column, or a subset.  The caller's ldw is read by
    one kernel only: transpose_kernel<float, float> (fp32 W has no vector transpose), which
    writes the feature-major workspace copy; the similarity and top-k kernels then run on that
    copy whatever the caller's alignment (fused w-bar, ssr_sim_kernel<16>)."""
    L, lib, st = env(pt2q)
    n, m, b = 256, 700, 128
    Wh = synth.weights(991, n, m)
    rem = np.arange(m, dtype=np.int64)
    if subset:
        rem = rem[(rem % 13) != 4]
    r = len(rem)
    rblk, rnew = orc.select_next_block_ssr(Wh, rem, b)
    rsim = orc.ssr_similarity(Wh, rem)
    W = Pad((n, m), ldw, torch.float32, f32(Wh), lead)
    remd = vec(r, torch.int64, torch.from_numpy(rem))
    blk, new = vec(b, torch.int64, out=True), vec(r - b, torch.int64, out=True)
    sim = vec(r, torch.float32, out=True)
    ws = L.workspace(lib.pt2q_ssr_workspace_bytes(n, m), DEV)
    L.check(lib.pt2q_ssr_select(W.p, ldw, n, m, remd.p, r, b, blk.p, new.p, sim.p, L.ptr(ws), ws.numel(), st),
            "pt2q_ssr_select")
    L.check_status(ws, "pt2q_ssr_select")
    assert np.array_equal(blk.win()[0], rblk) and np.array_equal(new.win()[0], rnew)
    assert bits_equal(sim.win()[0], rsim)
    assert outs_ok(blk, new, sim) and ins_ok(W, remd)


def test_ssr_select_last_block(pt2q):
    """r = 100 <= b = 128 with ldw = 701: blk is rem itself, in order, whatever W holds (no
    similarity launch when sim is NULL); newrem and an unpassed sim buffer stay untouched, and
    the padded W is still transposed into the workspace without being modified."""
    L, lib, st = env(pt2q)
    n, m, b = 256, 700, 128
    rem = np.arange(m, dtype=np.int64)[3::7]
    r = len(rem)
    W = Pad((n, m), 701, torch.float32, f32(synth.weights(991, n, m)))
    remd = vec(r, torch.int64, torch.from_numpy(rem))
    blk, new, sim = vec(r, torch.int64, out=True), vec(8, torch.int64, out=True), vec(r, torch.float32, out=True)
    ws = L.workspace(lib.pt2q_ssr_workspace_bytes(n, m), DEV)
    L.check(lib.pt2q_ssr_select(W.p, 701, n, m, remd.p, r, b, blk.p, new.p, None, L.ptr(ws), ws.numel(), st),
            "pt2q_ssr_select")
    L.check_status(ws, "pt2q_ssr_select")
    assert np.array_equal(blk.win()[0], rem)
    assert outs_ok(blk) and new.untouched() and sim.untouched() and ins_ok(W, remd)


# ------------------------------------------------------------------ pt2q_error_feedback

@functools.lru_cache(maxsize=None)
def _ef_ref():
    n, m, bs = 132, 330, 100
    rng = np.random.default_rng(n + m)
    W = synth.weights(700 + n, n, m)
    cols = rng.permutation(m)
    blk, rem = cols[:bs].astype(np.int64), cols[bs:].astype(np.int64)
    E = synth.weights(701 + n, n, bs) * np.float32(0.1)
    H, _ = orc.prepare_hessian(orc.gram(synth.activations(702 + m, 2 * m, m)), 2 * m)
    Hinv, spd = orc.cholesky_inverse(H)
    assert spd
    return W, blk, rem, E, Hinv, orc.error_feedback(W, blk, rem, E, Hinv)


@pytest.mark.parametrize("ldw,lde,ldhi,lead", [(336, 104, 340, 0), (331, 101, 333, 0), (336, 104, 340, 1),
                                               (331, 104, 340, 0), (336, 101, 333, 0)])
def test_error_feedback(pt2q, ldw, lde, ldhi, lead):
    """(n, m, bs) = (132, 330, 100), W updated in place.  The caller's ldw / lde are read by
    transpose_kernel<float, float> (into the feature-major workspace copies) and ldw again by the
    transpose back; ldhi by ef_coeff_kernel (scalar gathers Hinv[blk_k][rem_e]).  The update itself
    (pt2q_launch_ef, ef.hip) runs on the workspace copies, whose alignment does not depend on the
    caller.  W's pads and its block columns must be untouched."""
    L, lib, st = env(pt2q)
    n, m, bs = 132, 330, 100
    Wh, blkh, remh, Eh, Hh, ref = _ef_ref()
    W = Pad((n, m), ldw, torch.float32, f32(Wh), lead, out=True)
    E = Pad((n, bs), lde, torch.float32, f32(Eh), lead)
    Hinv = Pad((m, m), ldhi, torch.float32, f32(Hh), lead)
    blk, rem = vec(bs, torch.int64, torch.from_numpy(blkh)), vec(m - bs, torch.int64, torch.from_numpy(remh))
    ws = L.workspace(lib.pt2q_error_feedback_workspace_bytes(n, m, bs), DEV)
    L.check(lib.pt2q_error_feedback(W.p, ldw, n, m, blk.p, bs, rem.p, m - bs, E.p, lde, Hinv.p, ldhi, L.ptr(ws),
                                    ws.numel(), st), "pt2q_error_feedback")
    got = W.win()
    assert bits_equal(got, ref)
    assert bits_equal(got[:, blkh], Wh[:, blkh])
    assert outs_ok(W) and ins_ok(E, Hinv, blk, rem)


# ------------------------------------------------------------------ block loops

SSR, S1_GIVEN, ACT, HESS = 0x1, 0x2, 0x10, 0x20


@functools.lru_cache(maxsize=None)
def _loop_inputs(m, N, seed):
    """Raw Gram, damped Hessian and inverse of fp32 activations (oracle)."""
    orc.set_threads(16)
    G = orc.gram(synth.activations(seed, N, m))
    H, _ = orc.prepare_hessian(G, N, 0.01)
    Hinv, spd = orc.cholesky_inverse(H)
    assert spd
    return G, H, Hinv


class LoopOut:
    """The packed outputs of a block loop (no leading dimensions), each guarded; lead offsets the
    bases of alpha, mu and T (T by one byte: the code transposes' 16-byte path needs an aligned T)."""

    def __init__(self, n, m, B, lead=0):
        self.alpha = Pad((n, B), B, torch.float32, None, lead, out=True)
        self.mu = Pad((n, B), B, torch.float32, None, lead, out=True)
        self.T = Pad((n, m), m, torch.int8, None, lead, out=True)
        self.perm = vec(m, torch.int64, out=True)
        self.iters = vec(B, torch.int32, out=True)

    def check(self, ref):
        assert np.array_equal(self.perm.win()[0], ref["perm"])
        assert np.array_equal(self.T.win(), ref["T"])
        assert bits_equal(self.alpha.win(), ref["alpha"]) and bits_equal(self.mu.win(), ref["mu"])
        assert np.array_equal(self.iters.win()[0], ref["iters"])
        assert outs_ok(self.alpha, self.mu, self.T, self.perm, self.iters)


def _wpad(Wh, dt, ldw, lead=0):
    """W (fp32 numpy) as a padded device operand of type dt, and the fp32 values the oracle takes."""
    if dt == torch.float32:
        return Pad(Wh.shape, ldw, dt, f32(Wh), lead), Wh
    d, _ = to16(Wh, dt)
    return Pad(Wh.shape, ldw, dt, d, lead), d.float().numpy()


@functools.lru_cache(maxsize=None)
def _blocks_ref(dt):
    G, _, Hinv = _loop_inputs(384, 500, 1001)
    Wo = _wpad(synth.weights(1002, 128, 384), dt, 384)[1]
    return orc.quantize_blocks(Wo, G, Hinv, 128, True, 1)


@pytest.mark.parametrize("dt,ldw,lda,ldhi,lead", [
    (torch.float32, 388, 392, 396, 0), (torch.float32, 385, 387, 389, 0), (torch.float32, 388, 392, 396, 1),
    (F16, 392, 388, 396, 0), (F16, 387, 385, 389, 0), (F16, 392, 388, 396, 1)])
def test_quantize_blocks(pt2q, dt, ldw, lda, ldhi, lead):
    """n = 128, m = 384, b = 128, SSR + variant M, three different leading dimensions.  ldw is read
    by the setup transpose: fp32 W -> transpose_kernel<float, float> whatever the alignment; fp16 W
    -> transpose16_kernel<_Float16> for ldw = 392 (ldw % 8, 16-byte base) and the scalar
    transpose_kernel<_Float16, float> for ldw = 387 or lead = 1.  lda is read by the S1 / d
    workgroups inside atq_block_kernel (blocks <= 128 columns) and ldhi by its EF coefficient
    workgroups, both by scalar gathers.  Everything else runs on the workspace copies; the codes
    come back through transpose_i8x16_kernel, or transpose_kernel<int8_t, int8_t> when T's base is
    not 16-byte aligned (lead = 1 offsets the outputs too)."""
    L, lib, st = env(pt2q)
    n, m, b = 128, 384, 128
    G, _, Hinvh = _loop_inputs(m, 500, 1001)
    W, _ = _wpad(synth.weights(1002, n, m), dt, ldw, lead)
    A = Pad((m, m), lda, torch.float32, f32(G), lead)
    Hinv = Pad((m, m), ldhi, torch.float32, f32(Hinvh), lead)
    out = LoopOut(n, m, 3, lead)
    ws = L.workspace(lib.pt2q_blocks_workspace_bytes(n, m, b, SSR | ACT), DEV)
    L.check(lib.pt2q_quantize_blocks(W.p, L.dtype_code(W.buf), ldw, n, m, b, SSR | ACT, A.p, lda, Hinv.p, ldhi, 100,
                                     out.alpha.p, out.mu.p, out.T.p, 3, out.perm.p, out.iters.p, L.ptr(ws),
                                     ws.numel(), st), "pt2q_quantize_blocks")
    L.check_status(ws, "pt2q_quantize_blocks")
    out.check(_blocks_ref(dt))
    assert ins_ok(W, A, Hinv)


@pytest.mark.parametrize("ldw,lda,ldhi,lead", [(304, 308, 312, 0), (301, 303, 305, 0), (304, 308, 312, 1)])
def test_quantize_blocks_variant_g(pt2q, ldw, lda, ldhi, lead):
    """Variant G (PT2Q_AGA_HESS), n = 64, m = 300, b = 100: A is the damped Hessian, read through
    lda by s1_hess_block_kernel (gathers H[blk][blk] into LDS by scalar loads); Hinv through ldhi
    by the EF coefficient workgroups of atq_block_kernel; W through ldw by transpose_kernel."""
    L, lib, st = env(pt2q)
    n, m, b = 64, 300, 100
    _, Hh, Hinvh = _loop_inputs(m, 400, 1011)
    Wh = synth.weights(1012, n, m)
    ref = orc.quantize_blocks(Wh, Hh, Hinvh, b, True, 2)
    W = Pad((n, m), ldw, torch.float32, f32(Wh), lead)
    A = Pad((m, m), lda, torch.float32, f32(Hh), lead)
    Hinv = Pad((m, m), ldhi, torch.float32, f32(Hinvh), lead)
    out = LoopOut(n, m, 3, lead)
    ws = L.workspace(lib.pt2q_blocks_workspace_bytes(n, m, b, SSR | HESS), DEV)
    L.check(lib.pt2q_quantize_blocks(W.p, 0, ldw, n, m, b, SSR | HESS, A.p, lda, Hinv.p, ldhi, 100, out.alpha.p,
                                     out.mu.p, out.T.p, 3, out.perm.p, out.iters.p, L.ptr(ws), ws.numel(), st),
            "pt2q_quantize_blocks")
    L.check_status(ws, "pt2q_quantize_blocks")
    out.check(ref)
    assert ins_ok(W, A, Hinv)


@functools.lru_cache(maxsize=None)
def _pc_ref(n, seed):
    """Per-channel (one block) oracle result for an n x 520 bf16 linear."""
    m = 520
    G = _loop_inputs(m, 300, 1021)[0]
    Wo = _wpad(synth.weights(seed, n, m), BF16, m)[1]
    return orc.quantize_blocks(Wo, G, np.zeros((m, m), np.float32), m, True, 1)


def _pc_s1d(m):
    G = _loop_inputs(m, 300, 1021)[0]
    S1 = orc.rowsum_seq(G)
    return np.concatenate([S1, orc.rowsum_seq(S1[None, :])]).astype(np.float32)


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("ldw,lda,lead,olead", [(528, 524, 0, 0), (523, 521, 0, 0), (528, 524, 1, 0),
                                                (528, 524, 0, 1)])
def test_quantize_blocks_per_channel(pt2q, given, ldw, lda, lead, olead):
    """Per-channel (b = m = 520 > 512), n = 70, bf16 W read in place through ldw, Hinv = NULL.
    ldw = 528 (1056-byte rows, 16-byte base): the atq_pc row kernels (pt2q_atq_pc_supported);
    ldw = 523 or lead = 1: atq_wide_block_kernel<LayRM<uint16_t, int8_t>>.  Without
    PT2Q_FLAG_S1_GIVEN, A is the raw Gram read through lda by s1_rows_kernel (pt2q_launch_s1,
    m > 512); with it, A is S1 then d (m + 1 floats).  olead = 1: the atq_pc kernels writing
    alpha, mu and T (ld m) at bases offset by one element."""
    L, lib, st = env(pt2q)
    n, m = 70, 520
    G = _loop_inputs(m, 300, 1021)[0]
    W, _ = _wpad(synth.weights(1022, n, m), BF16, ldw, lead)
    A = vec(m + 1, torch.float32, f32(_pc_s1d(m)), lead=lead) if given else Pad((m, m), lda, torch.float32, f32(G), lead)
    out = LoopOut(n, m, 1, olead)
    flags = SSR | ACT | (S1_GIVEN if given else 0)
    ws = L.workspace(lib.pt2q_blocks_workspace_bytes(n, m, m, flags), DEV)
    L.check(lib.pt2q_quantize_blocks(W.p, 2, ldw, n, m, m, flags, A.p, lda, None, 0, 100, out.alpha.p, out.mu.p,
                                     out.T.p, 3, out.perm.p, out.iters.p, L.ptr(ws), ws.numel(), st),
            "pt2q_quantize_blocks")
    L.check_status(ws, "pt2q_quantize_blocks")
    out.check(_pc_ref(n, 1022))
    assert ins_ok(W, A)


@pytest.mark.parametrize("ldw,lda,ldhi", [(392, 388, 396), (387, 385, 389)])
def test_quantize_blocks_group(pt2q, ldw, lda, ldhi):
    """pt2q_quantize_blocks_group, two fp16 linears of 128 x 384, b = 128, each with its own Gram
    and inverse, padded ldw / lda / ldhi: transpose16_kernel (ldw = 392) or the scalar transpose
    (387) per linear, then the grouped launches (grid.z = linear) whose S1 / d and EF coefficient
    workgroups gather through lda / ldhi.  Each linear equals the oracle."""
    L, lib, st = env(pt2q)
    n, m, b = 128, 384, 128
    ins, outs, refs = [], [], []
    for z in range(2):
        G, _, Hinvh = _loop_inputs(m, 500 + 64 * z, 1031 + z)
        W, Wo = _wpad(synth.weights(1041 + z, n, m), F16, ldw)
        ins.append((W, Pad((m, m), lda, torch.float32, f32(G)), Pad((m, m), ldhi, torch.float32, f32(Hinvh))))
        outs.append(LoopOut(n, m, 3))
        refs.append(orc.quantize_blocks(Wo, G, Hinvh, b, True, 1))
    arrs = [parr(x) for x in ([i[0].ptr for i in ins], [i[1].ptr for i in ins], [i[2].ptr for i in ins],
                              [o.alpha.ptr for o in outs], [o.mu.ptr for o in outs], [o.T.ptr for o in outs],
                              [o.perm.ptr for o in outs], [o.iters.ptr for o in outs])]
    p = [a[0] for a in arrs]
    ws = L.workspace(lib.pt2q_quantize_blocks_group_workspace_bytes(2, n, m, b, SSR | ACT), DEV)
    L.check(lib.pt2q_quantize_blocks_group(2, p[0], 1, ldw, n, m, b, SSR | ACT, p[1], lda, p[2], ldhi, 100, p[3],
                                           p[4], p[5], 3, p[6], p[7], L.ptr(ws), ws.numel(), st),
            "pt2q_quantize_blocks_group")
    L.check_status(ws, "pt2q_quantize_blocks_group")
    for z in range(2):
        outs[z].check(refs[z])
        assert ins_ok(*ins[z]), z


@pytest.mark.parametrize("ldw", [528, 523])
def test_quantize_perchannel_group(pt2q, ldw):
    """pt2q_quantize_perchannel_group, m = 520, n = [70, 36], bf16, S1 / d given.  ldw = 528: every
    linear passes pt2q_atq_pc_supported, one pt2q_launch_atq_pc_group launch; ldw = 523: one
    atq_wide_block_kernel<LayRM> launch per linear.  Then the grouped zero-row repair."""
    L, lib, st = env(pt2q)
    m, ns = 520, [70, 36]
    s1d = vec(m + 1, torch.float32, f32(_pc_s1d(m)))
    Ws = [_wpad(synth.weights(1022 + z, n, m), BF16, ldw)[0] for z, n in enumerate(ns)]
    outs = [LoopOut(n, m, 1) for n in ns]
    arrs = [parr(x) for x in ([w.ptr for w in Ws], [s1d.ptr] * 2, [o.alpha.ptr for o in outs],
                              [o.mu.ptr for o in outs], [o.T.ptr for o in outs], [o.perm.ptr for o in outs],
                              [o.iters.ptr for o in outs])]
    p = [a[0] for a in arrs]
    narr = (ctypes.c_int * 2)(*ns)
    ws = L.workspace(lib.pt2q_quantize_perchannel_group_workspace_bytes(2), DEV)
    L.check(lib.pt2q_quantize_perchannel_group(2, p[0], 2, ldw, ctypes.cast(narr, ctypes.c_void_p), m, p[1], 100,
                                               p[2], p[3], p[4], 3, p[5], p[6], L.ptr(ws), ws.numel(), st),
            "pt2q_quantize_perchannel_group")
    L.check_status(ws, "pt2q_quantize_perchannel_group")
    for z, n in enumerate(ns):
        outs[z].check(_pc_ref(n, 1022 + z))
    assert ins_ok(s1d, *Ws)


@pytest.mark.parametrize("ldw,ldx,lead", [(260, 264, 0), (257, 259, 0), (260, 264, 1)])
def test_quantize_layer(pt2q, ldw, ldx, lead):
    """pt2q_quantize_layer, n = 128, m = 256, N = 200, b = 128, fp32 W, fp16 X.  ldx feeds the
    Gram (gram16x_kernel, no split at 6 tiles: DMA staging for ldx = 264, register-staged for
    ldx = 259 or lead = 1); ldw the setup transpose (transpose_kernel<float, float>).  Everything
    after them runs on packed workspace matrices."""
    L, lib, st = env(pt2q)
    n, m, N, b = 128, 256, 200, 128
    Wh = synth.weights(1051, n, m)
    Xd, Xo = to16(synth.activations(1052, N, m), F16)
    ref = _layer_ref()
    W = Pad((n, m), ldw, torch.float32, f32(Wh), lead)
    X = Pad((N, m), ldx, F16, Xd, lead)
    out = LoopOut(n, m, 2)
    info = vec(1, torch.int32, out=True)
    ws = L.workspace(lib.pt2q_layer_workspace_bytes(n, m, b, SSR | ACT), DEV)
    L.check(lib.pt2q_quantize_layer(W.p, 0, ldw, n, m, X.p, 1, N, ldx, b, SSR | ACT, 0.01, 100, out.alpha.p,
                                    out.mu.p, out.T.p, 3, out.perm.p, out.iters.p, info.p, L.ptr(ws), ws.numel(),
                                    st), "pt2q_quantize_layer")
    L.check_status(ws, "pt2q_quantize_layer")
    assert int(info.win()[0, 0]) == 0 and outs_ok(info)
    out.check(ref)
    assert ins_ok(W, X)


@functools.lru_cache(maxsize=None)
def _layer_ref():
    orc.set_threads(16)
    return orc.quantize_layer_m(synth.weights(1051, 128, 256), to16(synth.activations(1052, 200, 256), F16)[1])


# ------------------------------------------------------------------ ternary inference

def _tl_reference(x, alpha, mu, T, perm, bias, bs, dt):
    """test_gpu_ternary.py::test_shapes_vs_oracle's reference and tolerance."""
    n, m = T.shape
    if dt == F16:
        yo = orc.ternary_linear(x, alpha, mu, T, perm, bias, bs, compat=False).astype(np.float32)
        return yo, 2e-3, 2e-3 * max(1.0, np.sqrt(m / 512))
    B = alpha.shape[1]
    a16 = torch.from_numpy(alpha).bfloat16().float().numpy()
    m16 = torch.from_numpy(mu).bfloat16().float().numpy()
    W = np.zeros((n, m), np.float32)
    for k in range(B):
        cols = perm[k * bs:(k + 1) * bs]
        W[:, cols] = torch.from_numpy(a16[:, k:k + 1] * T[:, cols].astype(np.float32)
                                      + m16[:, k:k + 1]).bfloat16().float().numpy()
    xb = torch.from_numpy(x).bfloat16().double().numpy()
    y = xb @ W.astype(np.float64).T
    if bias is not None:
        y = y + torch.from_numpy(bias).bfloat16().double().numpy()
    return torch.from_numpy(y.astype(np.float32)).bfloat16().float().numpy(), 1.6e-2, 1e-2


@pytest.mark.parametrize("dt", [F16, BF16])
@pytest.mark.parametrize("tokens", [1, 5, 256])
@pytest.mark.parametrize("ldt,ldx,dy,lead", [(400, 392, 8, 0), (385, 387, 3, 0), (400, 392, 8, 1)])
def test_ternary_pack_and_linear(pt2q, dt, tokens, ldt, ldx, dy, lead):
    """n = 200, m = 384, bs = 128.  pt2q_ternary_pack reads T through ldt (tl_pack_kernel, one byte
    of four codes per thread, scalar loads); pt2q_ternary_linear reads x through ldx in
    tl_gather_x_kernel (scalar gather into the packed workspace copy) and writes y through
    ldy = n + dy in tl_reduce_kernel (tokens < 256: tl_gemm_kernel<BF16, 1> with K split, then the
    reduce; tokens = 256: tl_prefill_kernel, which stores y through ldy itself) -- none of them
    chooses a path by alignment.  y in xdtype and in fp32, with a bias and
    with bias = NULL; the pads of y, codes and gather must be intact."""
    L, lib, st = env(pt2q)
    n, m, bs = 200, 384, 128
    rng = np.random.default_rng(n + m + tokens)
    Th = rng.integers(-1, 2, size=(n, m)).astype(np.int8)
    alpha = (rng.random((n, 3)) * 0.05 + 0.005).astype(np.float32)
    mu = (rng.standard_normal((n, 3)) * 0.002).astype(np.float32)
    permh = rng.permutation(m).astype(np.int64)
    biash = (rng.standard_normal(n) * 0.1).astype(np.float32)
    xh = synth.activations(7 + tokens, tokens, m)
    T = Pad((n, m), ldt, torch.int8, torch.from_numpy(Th), lead)
    perm = vec(m, torch.int64, torch.from_numpy(permh))
    P = int(lib.pt2q_ternary_linear_positions(m))
    codes = Pad((n, P // 4), P // 4, torch.uint8, None, out=True)
    gather = vec(P, torch.int32, out=True)
    L.check(lib.pt2q_ternary_pack(T.p, ldt, n, m, perm.p, 0, codes.p, gather.p, st), "pt2q_ternary_pack")
    assert outs_ok(codes, gather) and ins_ok(T, perm)
    codes.snap, gather.snap = codes.ibuf.clone(), gather.ibuf.clone()  # inputs from here on
    # scales and bias as TernaryLinear stores them: rounded to the layer dtype, widened to fp32
    a32, m32 = vec(n * 3, torch.float32, f32(alpha).to(dt).float()), vec(n * 3, torch.float32, f32(mu).to(dt).float())
    b32 = vec(n, torch.float32, f32(biash).to(dt).float())
    x = Pad((tokens, m), ldx, dt, to16(xh, dt)[0], lead)
    code = L.dtype_code(x.buf)
    ws = L.workspace(lib.pt2q_ternary_linear_workspace_bytes(tokens, n, m), DEV)
    for ydt in (dt, torch.float32):
        for bias in (biash, None):
            yo, rtol, atol = _tl_reference(xh, alpha, mu, Th, permh, bias, bs, dt)
            y = Pad((tokens, n), n + dy, ydt, None, lead, out=True)
            L.check(lib.pt2q_ternary_linear(x.p, code, tokens, ldx, n, m, codes.p, gather.p, a32.p, m32.p, 3, bs,
                                            b32.p if bias is not None else None, y.p, L.dtype_code(y.buf), n + dy,
                                            L.ptr(ws), ws.numel(), st), "pt2q_ternary_linear")
            np.testing.assert_allclose(y.view.float().cpu().numpy(), yo, rtol=rtol, atol=atol)
            assert outs_ok(y), (ydt, bias is None)
    assert ins_ok(x, codes, gather, a32, m32, b32)


# ------------------------------------------------------------------ pt2q_sum_partials

@pytest.mark.parametrize("nparts", [3, 10])
def test_sum_partials_strided(pt2q, nparts):
    """count = 1000, stride = 1008 (NaN gaps between the parts), out = parts[0] (documented) and a
    separate out: sum_parts_kernel<8>, float4 per thread; 10 parts take two launches, the second
    continuing the fold from out.  stride % 4 != 0 or a 4-byte aligned out are refused
    (PT2Q_E_UNSUPPORTED) with out untouched."""
    L, lib, st = env(pt2q)
    count, stride = 1000, 1008
    parts_h = [synth.weights(1061 + p, 1, count)[0] for p in range(nparts)]
    ref = orc.sum_partials(parts_h)
    stack = f32(np.stack(parts_h))
    P = Pad((nparts, count), stride, torch.float32, stack)
    out = vec(count, torch.float32, out=True)
    L.check(lib.pt2q_sum_partials(P.p, stride, nparts, count, out.p, st), "pt2q_sum_partials")
    assert bits_equal(out.win()[0], ref)
    assert outs_ok(out) and ins_ok(P)
    Q = Pad((nparts, count), stride, torch.float32, stack, out=True)  # in place: out = parts[0]
    L.check(lib.pt2q_sum_partials(Q.p, stride, nparts, count, Q.p, st), "pt2q_sum_partials")
    got = Q.win()
    assert bits_equal(got[0], ref) and bits_equal(got[1:], np.stack(parts_h)[1:])
    assert outs_ok(Q)
    bad = vec(count, torch.float32, out=True, lead=1)
    Podd = Pad((nparts, count), 1001, torch.float32, stack)
    assert lib.pt2q_sum_partials(Podd.p, 1001, nparts, count, out.p, st) == E_UNSUPPORTED
    assert lib.pt2q_sum_partials(P.p, stride, nparts, count, bad.p, st) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bad.untouched() and bits_equal(out.win()[0], ref)
