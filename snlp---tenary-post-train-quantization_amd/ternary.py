"""Ternary inference layer on MI355X — the reference's TernaryLinear (model.py:17-127),
replace_linear_with_ternary (model.py:174-225) and save/load (utils.py:288-304).

Buffers and their state_dict names are the reference's (T int8, alpha, mu, perm, inv_perm, bias),
so checkpoints move between the two.  The forward pass is the libpt2q kernel
pt2q_ternary_linear (csrc/ternary_linear.hip): 2-bit packed codes dequantised in registers into
f16/bf16 MFMA operands; decode="fused" sends calls of 1..decode_max_tokens tokens to the
single-launch kernel pt2q_ternary_decode (csrc/ternary_decode.hip) instead; linears that read the
same x go through pt2q_ternary_decode_group (the same kernel) in one launch, a gated MLP's gate
and up projection with the SwiGLU activation as its epilogue (TernaryGatedMLP, fuse_gated_mlp);
the decode calls take an RMSNorm as prologue and a residual add as epilogue inside the same launch
(norm=, residual=, pt2q_ternary_decode_fused; rms_norm; TernaryMLPBlock).
Two semantics:

  compat=False (default)  y = x · Ŵᵀ + b with the correct reconstruction of gptq.py:201-230
                          (block k of alpha/mu belongs to columns perm[k·bs:(k+1)·bs]).
  compat=True             exactly what the reference forward computes: contiguous blocks of T
                          and a double permutation (model.py:75-110).
"""
import ctypes
import os
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


DECODE_MODES = ("mfma", "fused")
# Largest token count a decode="fused" layer sends to pt2q_ternary_decode.  The library takes up to
# pt2q_ternary_decode_max_tokens() = 8, but profiles/ternary_decode_timing.txt has the fused call
# below the MFMA path at every measured shape and dtype only for 1 token (2 tokens lose by 0.19 us
# at 4096 x 11008 bf16, 4 and 8 at most shapes), so that is the crossover used.
# A caller whose shapes do better may raise it, up to the library's cap.
DECODE_CROSSOVER_TOKENS = 1
decode_max_tokens = min(int(_lib.lib().pt2q_ternary_decode_max_tokens()), DECODE_CROSSOVER_TOKENS)
# Largest token count a TernaryGatedMLP whose children are decode="fused" sends to the SwiGLU
# kernel and ternary_decode(down_proj); above it the children are called one by one.
# profiles/ternary_mlp_timing.txt has the fused module below three decode calls plus torch's silu and
# mul by 7.8-11.2 us at 1 token at every measured shape and dtype; at 2 tokens and above it loses at
# hidden 5120 (two gathered copies of x leave LDS for one token per workgroup there), so the
# crossover is 1.  A caller whose shapes do better may raise it, up to the cap.
MLP_DECODE_CROSSOVER_TOKENS = 1
mlp_decode_max_tokens = min(int(_lib.lib().pt2q_ternary_decode_max_tokens()), MLP_DECODE_CROSSOVER_TOKENS)
# Largest token count a TernaryMLPBlock whose projections are decode="fused" runs in two launches
# (norm prologue, residual epilogue); above it the block is rms_norm, the TernaryGatedMLP and
# torch's add.  profiles/ternary_block_timing.txt has the two launches below that four-launch form
# by 3.3-6.6 us at 1, 2 and 4 tokens at every measured shape and dtype and level with it or behind
# at 8 (-0.5 .. +1.4 us), so the crossover is 4.  The table's four-launch form has
# the TernaryGatedMLP on its own two-launch path, so the block also stays within
# mlp_decode_max_tokens: above that the MLP goes through its children, which the table does not
# cover, and the block follows it.  A caller whose shapes do better may raise both, up to the cap.
BLOCK_DECODE_CROSSOVER_TOKENS = 4
block_decode_max_tokens = min(int(_lib.lib().pt2q_ternary_decode_max_tokens()), BLOCK_DECODE_CROSSOVER_TOKENS)


def _check_mode(decode):
    if decode not in DECODE_MODES:
        raise ValueError(f"decode must be one of {DECODE_MODES}, got {decode!r}")
    return decode


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pt2q_rmsnorm: the Llama RMSNorm weight * (x.float() * rsqrt(mean(x²) + eps)).to(x.dtype) over
    the last dimension, bit-defined by contract RMSNORM16 (not torch's bits: its
    reduction order and rsqrt differ).  x: fp16/bf16, tokens x m with unit column stride (any row
    stride and base) or contiguous with more dimensions; weight: m elements of x's dtype; any
    number of tokens; out: an optional tensor of x's shape and dtype to write into, which may be
    x.  The norm= keyword of the decode calls computes the same bits inside their launch."""
    what = "rms_norm"
    _lib.require_device(x)
    m = x.shape[-1] if x.dim() else 0
    weight = _check_norm(x, (weight, eps), what)[0]
    if x.dim() != 2 and not x.is_contiguous() or x.dim() == 2 and x.stride(1) != 1:
        raise _lib.Pt2qError(f"{what}: x must be tokens x m with unit column stride, or contiguous")
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    elif out.shape != x.shape or out.dtype != x.dtype or not out.is_cuda or \
            (out.stride(1) != 1 if out.dim() == 2 else not out.is_contiguous()):
        raise _lib.Pt2qError(f"{what}: out must have x's shape and dtype, with unit column stride or contiguous")
    x2, o2 = (x, out) if x.dim() == 2 else (x.view(-1, m), out.view(-1, m))
    tokens = x2.shape[0]
    if tokens:
        _lib.check(_lib.lib().pt2q_rmsnorm(
            _lib.ptr(x2), _lib.dtype_code(x2), tokens, x2.stride(0) if tokens > 1 else m, m, _lib.ptr(weight), float(eps),
            _lib.ptr(o2), o2.stride(0) if tokens > 1 else m, _lib.stream_of(x.device)), "pt2q_rmsnorm")
    return out


def _check_norm(x, norm, what):
    """(weight, eps) of a norm= keyword after its checks."""
    weight, eps = norm
    _lib.require_device(weight)
    if x.dtype not in (torch.float16, torch.bfloat16) or x.dim() < 1 or weight.dtype != x.dtype or \
            weight.dim() != 1 or weight.numel() != x.shape[-1]:
        raise _lib.Pt2qError(f"{what}: the norm weight has x's dtype (fp16 / bf16) and its m elements")
    return weight.contiguous(), float(eps)


def ternary_decode(x: torch.Tensor, codes: torch.Tensor, gather: torch.Tensor, alpha: torch.Tensor,
                   mu: torch.Tensor, block_size: int, bias: Optional[torch.Tensor] = None,
                   out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None,
                   norm=None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pt2q_ternary_decode: y = x · Ŵᵀ (+ bias) for 1..8 tokens in one launch, bit-defined (DESIGN.md
    §3 DOT64P).  x: tokens x m fp16/bf16 with unit column stride (any row stride and base); codes
    (n x P/4 uint8) and gather (P int32) from pt2q_ternary_pack; alpha, mu: n x B fp32; bias: n fp32
    or None; out_dtype: x's dtype (default) or torch.float32; out: an optional tokens x n tensor of
    that dtype with unit column stride to write into.  norm=(weight, eps): the layer reads
    rms_norm(x, weight, eps), computed inside the launch; residual: a tokens x n tensor of x's
    dtype added to the result as torch adds 16-bit tensors (RESADD16), which may be `out` itself.
    With either the call is pt2q_ternary_decode_fused, still one launch."""
    what = "ternary_decode"
    packs, bs = _group_members(x, [(codes, gather, alpha, mu, bias)], block_size, what)
    codes, gather, alpha, mu, bias = packs[0]
    tokens, m = x.shape
    n, B = alpha.shape
    out = _check_out(out, tokens, n, x.dtype if out_dtype is None else out_dtype, x.device, what)
    if norm is not None or residual is not None:
        if tokens:
            _decode_group(x, packs, bs, [out], _lib.DECODE_PLAIN, "pt2q_ternary_decode_fused", norm, [residual], what)
        return out
    if tokens == 0:
        return out
    ldx = x.stride(0) if tokens > 1 else m
    ldy = out.stride(0) if tokens > 1 else n
    _lib.check(_lib.lib().pt2q_ternary_decode(
        _lib.ptr(x), _lib.dtype_code(x), tokens, ldx, n, m, _lib.ptr(codes), _lib.ptr(gather),
        _lib.ptr(alpha), _lib.ptr(mu), B, bs, _lib.ptr(bias), _lib.ptr(out),
        _lib.dtype_code(out), ldy, _lib.stream_of(x.device)), "pt2q_ternary_decode")
    return out


def _group_members(x, members, block_size, what):
    """The (codes, gather, alpha, mu, bias) tuples of `members` (TernaryLinear, packed on demand, or
    such tuples with `block_size`) after the checks every decode call makes, and their block size."""
    if not 1 <= len(members) <= _lib.DECODE_GROUP_MAX:
        raise _lib.Pt2qError(f"{what}: 1..{_lib.DECODE_GROUP_MAX} members, got {len(members)}")
    _lib.require_device(x)
    if x.dim() != 2 or x.stride(1) != 1:
        raise _lib.Pt2qError(f"{what}: x must be tokens x m with unit column stride")
    m = x.shape[1]
    P = int(_lib.lib().pt2q_ternary_linear_positions(m))
    packs = []
    for mem in members:
        if isinstance(mem, TernaryLinear):
            if mem._packed is None:
                mem._prepare()
            if block_size is not None and block_size != mem.block_size:
                raise _lib.Pt2qError(f"{what}: the members share one block size")
            block_size = mem.block_size
            if mem.in_features != m or mem.dtype != x.dtype:
                raise _lib.Pt2qError(f"{what}: the members read x ({m} columns of {x.dtype})")
            mem = mem._packed
        codes, gather, alpha, mu, bias = mem
        for t in (codes, gather, alpha, mu):
            _lib.require_device(t)
        if alpha.dtype != torch.float32 or mu.dtype != torch.float32 or alpha.shape != mu.shape or alpha.dim() != 2 or \
                (bias is not None and bias.dtype != torch.float32):
            raise _lib.Pt2qError(f"{what}: alpha, mu (n x B) and bias are fp32")
        if codes.dtype != torch.uint8 or gather.dtype != torch.int32:
            raise _lib.Pt2qError(f"{what}: codes uint8 and gather int32, as pt2q_ternary_pack writes them")
        n = alpha.shape[0]
        if tuple(codes.shape) != (n, P // 4) or gather.numel() != P or (bias is not None and bias.numel() != n):
            raise _lib.Pt2qError(f"{what}: codes / gather / bias do not match x and alpha")
        packs.append((codes.contiguous(), gather.contiguous(), alpha.contiguous(), mu.contiguous(),
                      None if bias is None else bias.contiguous()))
    if block_size is None:
        raise _lib.Pt2qError(f"{what}: block_size is needed with packed tuples")
    return packs, int(block_size)


def _decode_group(x, packs, block_size, outs, epilogue, what, norm=None, residuals=None, caller=None):
    """pt2q_ternary_decode_group, or with norm (weight, eps) or residuals (one tensor or None per
    out) pt2q_ternary_decode_fused."""
    tokens, m = x.shape
    count = len(packs)
    ns = (ctypes.c_int * count)(*[p[2].shape[0] for p in packs])
    Bs = (ctypes.c_int * count)(*[p[2].shape[1] for p in packs])
    ld = lambda ts: (ctypes.c_int64 * len(ts))(*[0 if t is None else t.stride(0) if tokens > 1 else t.shape[1] for t in ts])  # noqa: E731
    ldys = ld(outs)
    arrs = [_lib.ptr_array([p[i] for p in packs]) for i in range(5)] + [_lib.ptr_array(outs)]
    as_p = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    args = (_lib.ptr(x), _lib.dtype_code(x), tokens, x.stride(0) if tokens > 1 else m, m, count, as_p(ns),
            arrs[0][0], arrs[1][0], arrs[2][0], arrs[3][0], as_p(Bs), block_size, arrs[4][0], arrs[5][0],
            _lib.dtype_code(outs[0]), as_p(ldys), epilogue)
    if norm is None and residuals is None:
        _lib.check(_lib.lib().pt2q_ternary_decode_group(*args, _lib.stream_of(x.device)), what)
        return
    weight, eps = (None, 0.0) if norm is None else _check_norm(x, norm, caller)
    residuals = [None] * len(outs) if residuals is None else list(residuals)
    if len(residuals) != len(outs):
        raise _lib.Pt2qError(f"{caller}: one residual (or None) per output")
    for r, o in zip(residuals, outs):
        if r is not None and (not isinstance(r, torch.Tensor) or not r.is_cuda or r.shape != o.shape or
                              r.dtype != o.dtype or r.stride(1) != 1):
            raise _lib.Pt2qError(f"{caller}: a residual has its output's shape and dtype, with unit column stride")
    res, ldrs = _lib.ptr_array(residuals), ld(residuals)
    _lib.check(_lib.lib().pt2q_ternary_decode_fused(*args, _lib.ptr(weight), eps, res[0], as_p(ldrs),
                                                    _lib.stream_of(x.device)), what)


def _check_out(out, tokens, n, dtype, device, what):
    if out is None:
        return torch.empty((tokens, n), dtype=dtype, device=device)
    if tuple(out.shape) != (tokens, n) or out.dtype != dtype or out.stride(1) != 1 or not out.is_cuda:
        raise _lib.Pt2qError(f"{what}: out must be tokens x n of the output dtype with unit column stride")
    return out


def ternary_decode_group(x: torch.Tensor, members, out_dtype: Optional[torch.dtype] = None, outs=None,
                         block_size: Optional[int] = None, norm=None, residuals=None):
    """pt2q_ternary_decode_group, PLAIN: 1..4 ternary linears on the same x (1..8 tokens) in one
    launch -- the q/k/v projections of a host that owns its attention code.  members: TernaryLinear
    modules (packed on demand) or (codes, gather, alpha, mu, bias) tuples as ternary_decode takes
    them, then with block_size.  Returns one tokens x n tensor per member (out_dtype: x's dtype or
    torch.float32; outs: optional tensors to write into), each bit-equal to ternary_decode on that
    member alone.  norm=(weight, eps) and residuals (one tensor or None per member) as in
    ternary_decode: input_layernorm and q/k/v in one launch."""
    what = "ternary_decode_group"
    packs, bs = _group_members(x, members, block_size, what)
    tokens = x.shape[0]
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if outs is not None and len(outs) != len(packs):
        raise _lib.Pt2qError(f"{what}: one out per member")
    outs = [_check_out(None if outs is None else outs[z], tokens, p[2].shape[0], out_dtype, x.device, what)
            for z, p in enumerate(packs)]
    if tokens and norm is None and residuals is None:
        _decode_group(x, packs, bs, outs, _lib.DECODE_PLAIN, "pt2q_ternary_decode_group")
    elif tokens:
        _decode_group(x, packs, bs, outs, _lib.DECODE_PLAIN, "pt2q_ternary_decode_fused", norm, residuals, what)
    return outs


def ternary_decode_swiglu(x: torch.Tensor, gate, up, out: Optional[torch.Tensor] = None,
                          block_size: Optional[int] = None, norm=None) -> torch.Tensor:
    """pt2q_ternary_decode_group, SWIGLU: h = silu(gate(x)) * up(x) for 1..8 tokens in one launch,
    bit-defined by contract SWIGLU16 from the outputs the two separate
    ternary_decode calls would give.  gate, up: members as in ternary_decode_group, equal widths;
    h has x's dtype.  norm=(weight, eps) as in ternary_decode: post_attention_layernorm, gate, up
    and the activation in one launch."""
    what = "ternary_decode_swiglu"
    packs, bs = _group_members(x, [gate, up], block_size, what)
    if packs[0][2].shape[0] != packs[1][2].shape[0]:
        raise _lib.Pt2qError(f"{what}: gate and up have the same number of rows")
    out = _check_out(out, x.shape[0], packs[0][2].shape[0], x.dtype, x.device, what)
    if x.shape[0] and norm is None:
        _decode_group(x, packs, bs, [out], _lib.DECODE_SWIGLU, "pt2q_ternary_decode_group")
    elif x.shape[0]:
        _decode_group(x, packs, bs, [out], _lib.DECODE_SWIGLU, "pt2q_ternary_decode_fused", norm, None, what)
    return out


class TernaryLinear(nn.Module):
    """model.py:17-127.  decode="fused": forwards of 1..decode_max_tokens tokens run the
    single-launch kernel (ternary_decode); every other call, and decode="mfma", the MFMA path."""

    def __init__(self, in_features: int, out_features: int, block_size: int = 128,
                 bias: bool = True, dtype: torch.dtype = torch.float16, compat: bool = False,
                 device=None, decode: str = "mfma"):
        super().__init__()
        self.decode = _check_mode(decode)
        if dtype not in (torch.float16, torch.bfloat16):
            raise _lib.Pt2qError("TernaryLinear runs fp16/bf16 activations on the f16/bf16 MFMA "
                                 f"(got {dtype})")
        device = torch.device(device) if device is not None else torch.device("cuda")
        self.in_features = in_features
        self.out_features = out_features
        self.block_size = block_size
        self.compat = compat
        num_blocks = (in_features + block_size - 1) // block_size
        self.register_buffer("T", torch.zeros(out_features, in_features, dtype=torch.int8, device=device))
        self.register_buffer("alpha", torch.ones(out_features, num_blocks, dtype=dtype, device=device))
        self.register_buffer("mu", torch.zeros(out_features, num_blocks, dtype=dtype, device=device))
        self.register_buffer("perm", torch.arange(in_features, dtype=torch.long, device=device))
        self.register_buffer("inv_perm", torch.arange(in_features, dtype=torch.long, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=dtype, device=device))
        else:
            self.bias = None
        self._packed = None

    @property
    def dtype(self):
        return self.alpha.dtype

    # _packed (codes, fp32 scales, bias) is derived from the buffers: drop it wherever they can
    # change underneath it -- a state-dict load (on this module or a parent) and every _apply
    # (.half(), .bfloat16(), .to(), .cuda() on this module or a parent); the next forward repacks.
    def _load_from_state_dict(self, *args, **kwargs):
        self._packed = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _apply(self, *args, **kwargs):
        self._packed = None
        return super()._apply(*args, **kwargs)

    def set_quantized_params(self, alpha: torch.Tensor, mu: torch.Tensor, T: torch.Tensor,
                             perm: torch.Tensor, bias: Optional[torch.Tensor] = None):
        """model.py:59-73, then packs the codes for the kernel."""
        self.T.copy_(T.to(torch.int8))
        self.alpha.copy_(alpha)
        self.mu.copy_(mu)
        self.perm.copy_(perm)
        self.inv_perm.copy_(torch.argsort(self.perm))
        if bias is not None and self.bias is not None:
            self.bias.copy_(bias)
        self._packed = None

    def _prepare(self):
        _lib.require_device(self.T)
        n, m = self.out_features, self.in_features
        dev = self.T.device
        P = int(_lib.lib().pt2q_ternary_linear_positions(m))
        codes = torch.empty((n, P // 4), dtype=torch.uint8, device=dev)
        gather = torch.empty(P, dtype=torch.int32, device=dev)
        st = _lib.stream_of(dev)
        _lib.check(_lib.lib().pt2q_ternary_pack(_lib.ptr(self.T.contiguous()), m, n, m,
                                                _lib.ptr(self.perm.contiguous()), int(self.compat),
                                                _lib.ptr(codes), _lib.ptr(gather), st),
                   "pt2q_ternary_pack")
        # scales as the reference stores them (alpha's dtype), widened exactly to fp32
        self._packed = (codes, gather, self.alpha.float().contiguous(), self.mu.float().contiguous(),
                        None if self.bias is None else self.bias.float().contiguous())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """model.py:75-95 (compat) or x·Ŵᵀ + b (default), on the ternary MFMA kernel."""
        if self._packed is None:
            self._prepare()
        codes, gather, a32, m32, b32 = self._packed
        _lib.require_device(x)
        shape = x.shape
        xt = x.reshape(-1, self.in_features).to(self.dtype).contiguous()
        tokens = xt.shape[0]
        n, m = self.out_features, self.in_features
        y = torch.empty((tokens, n), dtype=self.dtype, device=x.device)
        if tokens == 0:
            return y.reshape(*shape[:-1], n)
        if self.decode == "fused" and tokens <= decode_max_tokens:
            ternary_decode(xt, codes, gather, a32, m32, self.block_size, b32, out=y)
            return y.reshape(*shape[:-1], n)
        ws = _lib.workspace(_lib.lib().pt2q_ternary_linear_workspace_bytes(tokens, n, m), x.device)
        B = a32.shape[1]
        _lib.check(_lib.lib().pt2q_ternary_linear(
            _lib.ptr(xt), _lib.dtype_code(xt), tokens, m, n, m, _lib.ptr(codes), _lib.ptr(gather),
            _lib.ptr(a32), _lib.ptr(m32), B, self.block_size, _lib.ptr(b32), _lib.ptr(y),
            _lib.dtype_code(y), n, _lib.ptr(ws), ws.numel(), _lib.stream_of(x.device)),
            "pt2q_ternary_linear")
        return y.reshape(*shape[:-1], n)

    def _dequantize(self) -> torch.Tensor:
        """model.py:97-110 as written (contiguous blocks of T; meaningful when perm = identity)."""
        W = torch.zeros(self.out_features, self.in_features, device=self.T.device, dtype=self.alpha.dtype)
        for b in range(self.alpha.shape[1]):
            s, e = b * self.block_size, min((b + 1) * self.block_size, self.in_features)
            W[:, s:e] = self.alpha[:, b:b + 1] * self.T[:, s:e].to(self.alpha.dtype) + self.mu[:, b:b + 1]
        return W

    def memory_footprint(self) -> int:
        """model.py:112-127 (bytes, reference accounting: int8 T, 2-byte scales)."""
        bias_bytes = self.bias.numel() * 2 if self.bias is not None else 0
        return (self.T.numel() + self.alpha.numel() * 2 + self.mu.numel() * 2 +
                self.perm.numel() * 8 + bias_bytes)

    def packed_footprint(self) -> int:
        """Bytes the kernel actually reads per call: 2-bit codes + fp32 scales (+ bias)."""
        if self._packed is None:
            self._prepare()
        codes, gather, a32, m32, b32 = self._packed
        return (codes.numel() + gather.numel() * 4 + a32.numel() * 4 + m32.numel() * 4 +
                (b32.numel() * 4 if b32 is not None else 0))


class TernaryGatedMLP(nn.Module):
    """down_proj(silu(gate_proj(x)) * up_proj(x)) over three TernaryLinear children (the names, and
    so the state_dict keys, of a Llama MLP).  With all three at decode="fused", forwards of
    1..mlp_decode_max_tokens tokens take two launches -- ternary_decode_swiglu, then
    ternary_decode on down_proj -- in place of three launches and two elementwise kernels; every
    other call goes through the children exactly as the unfused MLP does."""

    def __init__(self, gate_proj: TernaryLinear, up_proj: TernaryLinear, down_proj: TernaryLinear):
        super().__init__()
        if not _gated_mlp_matches(gate_proj, up_proj, down_proj):
            raise _lib.Pt2qError("TernaryGatedMLP: gate_proj and up_proj are TernaryLinear of one shape, dtype and "
                                 "block size, and down_proj reads their width in that dtype")
        self.gate_proj, self.up_proj, self.down_proj = gate_proj, up_proj, down_proj

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        gate, up, down = self.gate_proj, self.up_proj, self.down_proj
        if gate.decode == up.decode == down.decode == "fused":
            xt = x.reshape(-1, gate.in_features).to(gate.dtype).contiguous()
            if 0 < xt.shape[0] <= mlp_decode_max_tokens:
                if down._packed is None:
                    down._prepare()
                h = ternary_decode_swiglu(xt, gate, up)
                codes, gather, a32, m32, b32 = down._packed
                y = ternary_decode(h, codes, gather, a32, m32, down.block_size, b32)
                return y.reshape(*x.shape[:-1], down.out_features)
        return down(F.silu(gate(x)) * up(x))


class TernaryMLPBlock(nn.Module):
    """forward(h) = h + mlp(rms_norm(h, norm_weight, eps)): the MLP half of a pre-norm decoder layer
    over a TernaryGatedMLP.  With all three projections at decode="fused", h in their dtype and
    1..min(block_decode_max_tokens, mlp_decode_max_tokens) tokens it takes two launches --
    ternary_decode_swiglu with the norm as prologue, then ternary_decode on down_proj with h as
    residual -- in place of four (rms_norm, SwiGLU, down_proj, torch's add), with the same bits;
    every other call is the formula above over the same modules.
    norm_weight (hidden elements of the projections' dtype) is a buffer: state_dict key
    "norm_weight", beside the children's keys under "mlp."."""

    def __init__(self, norm_weight: torch.Tensor, eps: float, mlp: TernaryGatedMLP):
        super().__init__()
        if not isinstance(mlp, TernaryGatedMLP) or mlp.down_proj.out_features != mlp.gate_proj.in_features:
            raise _lib.Pt2qError("TernaryMLPBlock: mlp is a TernaryGatedMLP whose down_proj returns to the hidden width")
        if norm_weight.dim() != 1 or norm_weight.numel() != mlp.gate_proj.in_features or \
                norm_weight.dtype != mlp.gate_proj.dtype:
            raise _lib.Pt2qError("TernaryMLPBlock: norm_weight has the hidden width and the projections' dtype")
        self.register_buffer("norm_weight", norm_weight.detach().clone().to(mlp.gate_proj.T.device))
        self.eps = float(eps)
        self.mlp = mlp

    def forward(self, h: torch.Tensor) -> torch.Tensor:
        gate, up, down = self.mlp.gate_proj, self.mlp.up_proj, self.mlp.down_proj
        hidden = gate.in_features
        if gate.decode == up.decode == down.decode == "fused" and h.dtype == gate.dtype == self.norm_weight.dtype:
            ht = h.reshape(-1, hidden).contiguous()
            if 0 < ht.shape[0] <= min(block_decode_max_tokens, mlp_decode_max_tokens):
                if down._packed is None:
                    down._prepare()
                a = ternary_decode_swiglu(ht, gate, up, norm=(self.norm_weight, self.eps))
                codes, gather, a32, m32, b32 = down._packed
                y = ternary_decode(a, codes, gather, a32, m32, down.block_size, b32, residual=ht)
                return y.reshape(h.shape)
        return h + self.mlp(rms_norm(h.contiguous(), self.norm_weight.to(h.dtype), self.eps))


def _gated_mlp_matches(gate, up, down) -> bool:
    return all(isinstance(l, TernaryLinear) for l in (gate, up, down)) and \
        gate.in_features == up.in_features and gate.out_features == up.out_features == down.in_features and \
        gate.dtype == up.dtype == down.dtype and gate.block_size == up.block_size


_SILU_PROBE = (-20.0, -3.0, -1.0, -0.5, 0.0, 0.25, 1.0, 2.5, 8.0, 30.0)


def _computes_silu(act_fn) -> bool:
    """Whether act_fn gives F.silu's values on a fixed small CPU tensor (nn.SiLU, a functional
    silu, transformers' SiLU class; a GELU does not)."""
    if not callable(act_fn):
        return False
    p = torch.tensor(_SILU_PROBE, dtype=torch.float32)
    try:
        with torch.no_grad():
            r = act_fn(p.clone())
    except Exception:
        return False
    return isinstance(r, torch.Tensor) and r.shape == p.shape and torch.equal(r, F.silu(p))


def fuse_gated_mlp(model: nn.Module) -> nn.Module:
    """Replace every gated MLP of `model` by a TernaryGatedMLP over the same children: a module
    whose children are TernaryLinear gate_proj, up_proj and down_proj of matching dtypes, widths
    and block sizes (plus at most its act_fn), with no tensors of its own and an act_fn that
    computes SiLU.  Everything else -- attention, an MLP with another activation -- is left as it
    is; state_dict keys do not change."""
    for parent in list(model.modules()):
        for name, mod in list(parent.named_children()):
            kids = dict(mod.named_children())
            if isinstance(mod, TernaryGatedMLP) or not set(kids) - {"act_fn"} == {"gate_proj", "up_proj", "down_proj"}:
                continue
            if list(mod.parameters(recurse=False)) or list(mod.buffers(recurse=False)):
                continue
            gate, up, down = kids["gate_proj"], kids["up_proj"], kids["down_proj"]
            if _gated_mlp_matches(gate, up, down) and _computes_silu(getattr(mod, "act_fn", None)):
                setattr(parent, name, TernaryGatedMLP(gate, up, down))
    return model


def replace_linear_with_ternary(model: nn.Module, quantized_params: Dict[str, Dict[str, torch.Tensor]],
                                block_size: int = 128, compat: bool = False,
                                decode: str = "mfma") -> nn.Module:
    """model.py:174-225: swap each quantised nn.Linear for a TernaryLinear (decode: its keyword)."""
    for name, params in quantized_params.items():
        parts = name.split(".")
        parent = model
        for part in parts[:-1]:
            parent = getattr(parent, part)
        orig = getattr(parent, parts[-1])
        dt = params["alpha"].dtype if params["alpha"].dtype in (torch.float16, torch.bfloat16) \
            else torch.float16
        layer = TernaryLinear(orig.in_features, orig.out_features, block_size,
                              bias=orig.bias is not None, dtype=dt, compat=compat,
                              device=orig.weight.device, decode=decode)
        layer.set_quantized_params(params["alpha"], params["mu"], params["T"], params["perm"],
                                   orig.bias.data if orig.bias is not None else None)
        setattr(parent, parts[-1], layer)
        del orig
    return model


def set_decode(model: nn.Module, mode: str) -> nn.Module:
    """Switch every TernaryLinear of `model` to decode="mfma" or "fused"."""
    _check_mode(mode)
    for mod in model.modules():
        if isinstance(mod, TernaryLinear):
            mod.decode = mode
    return model


def compute_bits_per_weight(model: nn.Module, include_scales: bool = True) -> float:
    """utils.py:251-285: average bits per weight over the ternary layers of `model` -- log2(3)
    rounded to 1.58 bits per code plus 16 bits per alpha / mu entry; 16.0 when the model has no
    ternary layer (the reference finds none after its own CLI run).  Host
    arithmetic on buffer sizes only."""
    total_params = 0
    total_bits = 0.0
    for _, module in model.named_modules():
        if hasattr(module, "T"):  # TernaryLinear (the reference's duck test)
            nw = module.T.numel()
            total_params += nw
            total_bits += nw * 1.58
            if include_scales:
                total_bits += (module.alpha.numel() + module.mu.numel()) * 16
    if total_params == 0:
        return 16.0
    return total_bits / total_params


def save_quantized_model(model: nn.Module, save_path: str,
                         quantized_params: Dict[str, Dict[str, torch.Tensor]]):
    """utils.py:288-296 (same file layout)."""
    torch.save({"model_state_dict": model.state_dict(), "quantized_params": quantized_params},
               save_path)


def load_quantized_model(model: nn.Module, load_path: str):
    """utils.py:299-304, with the safe loader (tensors and dicts only)."""
    ckpt = torch.load(load_path, map_location="cpu", weights_only=True)
    model.load_state_dict(ckpt["model_state_dict"])  # (every TernaryLinear drops its pack on load)
    return model, ckpt.get("quantized_params", {})
