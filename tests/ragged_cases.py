"""Ragged widths (m % 4 != 0) and row counts (n % 4 != 0) of the calibration path -- a plain
helper, not a conftest.

The launchers of csrc/ switch kernels on divisibility conditions: 16-byte aligned rows, whole
vectors, whole 64-blocks.  This module holds

  * the case lists of tests/test_gpu_ragged.py -- the smallest shapes that still take each
    fallback -- with their inputs and CPU-oracle references (computed once, cached), and
  * a restatement in Python of the launch predicates those shapes are there to flip: each
    function returns the names of the kernels / forms the launch code takes, so that
    tests/test_ragged_cases_cpu.py can check, without a GPU, that every fallback is reached.

Workspaces are carved at 256-byte boundaries and the Python bindings pass fresh contiguous
tensors, so every base pointer is taken as 16-byte aligned unless an argument says otherwise;
offsets are counted in floats from such a base."""
import functools

import numpy as np
import torch

import synth
from oracle import oracle as orc

NB, SP = 64, 256          # chol.hip: block and sub-panel rows
SUMN_LDS_MAX = 12288      # common.hpp
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}


def ceil_div(a, b):
    return -(-a // b)


def round_up(a, b):
    return ceil_div(a, b) * b


# ------------------------------------------------------------------ case lists

INVERSE_M = [65, 130, 257, 323, 1001, 1537]                     # N = m + 50
BATCHED_INVERSE = [(131, 3, 32), (131, 3, 2), (1001, 2, 32)]    # (m, batch, chunk)
GRAM = [(77, 131, "fp32"), (77, 131, "fp16"), (77, 131, "bf16"), (300, 4101, "fp16")]  # (N, m, dtype)
SSR = [(203, 333, 128), (4099, 300, 128), (12291, 260, 128), (16388, 260, 128)]       # (n, m, b)
EF = [(67, 203, 50), (67, 203, 150)]                            # (n, m, bs)
LAYER_M = [(203, 333, 450, 128, True, "fp32"), (131, 257, 300, 64, True, "fp32"),
           (70, 1001, 1100, 128, False, "fp32"), (202, 330, 450, 128, True, "fp16"),
           (202, 330, 450, 128, True, "bf16")]                  # (n, m, N, bs, ssr, dtype)
# n % 4 != 0 alone (m a multiple of 128): the EF kernel runs, but without the w-bar hand-off, beside
# the unfused w-bar; 16-bit weights lose the tile transpose to the odd row count
LAYER_M_ROWS = [(203, 384, 450, 128, True, "fp32"), (203, 384, 450, 128, True, "fp16")]
LAYER_M_F32_CODES = LAYER_M[0]                                  # also run with T requested as fp32
PER_CHANNEL = [(61, 515, 600, 1024, "fp32"), (61, 515, 600, 1024, "bf16"), (61, 518, 600, 1024, "fp16")]
LAYER_G = [(67, 203, 300, 64, True), (67, 203, 300, 150, True), (67, 203, 300, 203, True)]  # (n, m, N, bs, ssr)
GRAPH_LAYER = (203, 333, 450, 128, True, "fp32")
# GramsFirst units (m, dtype, row counts of the unit's linears, N)
GF_UNITS = [(333, "fp16", (203, 128), 450), (512, "fp16", (384,), 640), (515, "bf16", (61,), 600),
            (333, "fp32", (70,), 400)]
GF_BLOCK_SIZES = [128, 1024]
GF_MODES = [(True, 16), (True, 1), (False, 1)]                  # (batched, group)


# ------------------------------------------------------------------ launch predicates

def chol_block_step(m, nb):
    """chol.hip factor(): the one-lane-per-column kernel for whole blocks of 16-byte rows."""
    return "lane" if nb == NB and m % 4 == 0 else "lpr"


def _desc(M, N, K, a, b, c, ld, upper=False, batch=1):
    return {"M": M, "N": N, "K": K, "A": a, "B": b, "C": c, "ld": ld, "upper": upper, "batch": batch}


def _trailing(ld, p0, nb, r0, rows, c0, cols, upper, batch):
    return _desc(rows, cols, nb, p0 * ld + r0, p0 * ld + c0, r0 * ld + c0, ld, upper, batch)


def _trtri(ld, j0, K, c1, cols, nk, batch):
    return _desc(cols, nk, K, j0 * ld + c1, j0 * ld, c1 * ld, ld, False, batch)


def gemm_vec(g):
    """gemm.hip vec_ok, f32 K-major operands: 16-byte rows, whole vectors, aligned items."""
    ok = all(g[x] % 4 == 0 for x in ("A", "B", "ld", "M", "N"))
    return ok and (g["batch"] <= 1 or (g["ld"] * g["ld"]) % 4 == 0)


def gemmx_ok(g):
    """gemmx.hip pt2q_launch_gemmx: aligned operands and C, lds and M, N multiples of 4."""
    return all(g[x] % 4 == 0 for x in ("A", "B", "C", "ld", "M", "N"))


def launch_big(g):
    """chol.hip launch_big: (asks gemmx, kernel taken)."""
    tiles = ceil_div(g["M"], 128) * ceil_div(g["N"], 128) // (2 if g["upper"] else 1) * max(g["batch"], 1)
    asks = tiles >= 64 and g["K"] >= 128
    if asks and gemmx_ok(g):
        return asks, "gemmx"
    return asks, "gemm_vec" if gemm_vec(g) else "gemm_novec"


def strip_update(g0, g1):
    """gemm.hip pt2q_launch_gemm2: the rank-<=128 kernel (which also factors the next diagonal
    block) or the generic pair."""
    def ru_ok(g):
        return g["M"] <= 0 or g["N"] <= 0 or (g["K"] <= 128 and gemmx_ok(g))
    if ru_ok(g0) and ru_ok(g1):
        return "rank_update2"
    live = [g for g in (g0, g1) if g["M"] > 0 and g["N"] > 0]
    return "gemm2_vec" if all(gemm_vec(g) for g in live) else "gemm2_novec"


def chol_schedule(m, batch=1):
    """The launches of pt2q_launch_cholesky_inverse for width m as (step, kernel, detail) tuples:
    ("block", lane|lpr, nb), ("diag", "chol_diag", nb) where the strip update did not factor the
    block, ("strip", ...), ("big", gemmx|gemm_vec|gemm_novec, {"asks", "M", "N", "K"})."""
    ld = m
    out = []
    ahead = m > 6144 and batch == 1
    CP = 1024 if (m > 6144 and not ahead) else 512
    side = ahead and m > 2 * CP
    factored = False

    def big(g):
        asks, k = launch_big(g)
        out.append(("big", k, {"asks": asks, "M": g["M"], "N": g["N"], "K": g["K"]}))

    for P0 in range(0, m, CP):
        Pend = m if m - P0 < CP else P0 + CP
        for Q0 in range(P0, Pend, SP):
            Qend = Pend if Pend - Q0 < SP else Q0 + SP
            p0 = Q0
            while p0 < Qend:
                nb = min(NB, Qend - p0)
                if not factored:
                    out.append(("diag", "chol_diag", nb))
                out.append(("block", chol_block_step(m, nb), nb))
                factored = False
                p1 = p0 + nb
                if p1 >= Qend:
                    break
                k = strip_update(_trailing(ld, p0, nb, p1, Qend - p1, p1, m - p1, False, batch),
                                 _trtri(ld, p0, nb, p1, Qend - p1, p1, batch))
                out.append(("strip", k, nb))
                factored = k == "rank_update2"
                p0 += NB
            if Qend >= Pend:
                break
            K = Qend - Q0
            big(_trailing(ld, Q0, K, Qend, Pend - Qend, Qend, m - Qend, False, batch))
            big(_trtri(ld, Q0, K, Qend, Pend - Qend, Qend, batch))
        if Pend >= m:
            break
        K, rest = Pend - P0, m - Pend
        Pend2 = min(m, Pend + CP) if side else m
        big(_trailing(ld, P0, K, Pend, Pend2 - Pend, Pend, rest, not Pend2 < m, batch))
        big(_trtri(ld, P0, K, Pend, Pend2 - Pend, Pend, batch))
        if Pend2 < m:
            big(_trailing(ld, P0, K, Pend2, m - Pend2, Pend2, m - Pend2, True, 1))
            big(_trtri(ld, P0, K, Pend2, m - Pend2, Pend, 1))
    big(_desc(m, m, m, 0, 0, 0, ld, True, batch))  # lauum
    return out


def prepare_hessian_form(m, base_floats=0):
    """misc.hip pt2q_launch_prepare_hessian with packed m x m operands (ld = item stride / m = m)."""
    if m > SUMN_LDS_MAX:
        return "scale+damp"
    return "fill4" if m % 4 == 0 and base_floats % 4 == 0 else "fill"


def ssr_kernels(n, fusable=True, ldw=None):
    """ssr.hip pt2q_launch_ssr_similarity on the feature-major copy (ldw = round_up(n, 64) unless
    given): the w-bar kernels, then the similarity kernel."""
    ldw = round_up(n, 64) if ldw is None else ldw
    v4 = n % 4 == 0 and ldw % 4 == 0
    if fusable and n <= 16384 and v4:
        names = ["wbar_fused"]
    else:
        names = ["wbar_partial"] + (["wbar_sumfinal"] if n <= SUMN_LDS_MAX else ["wbar_sum", "wbar_final"])
    if v4 and 4096 < n <= 16384:
        names.append("sim_split<%d>" % ceil_div(n, 4096))
    else:
        names.append("sim<0>" if not v4 else "sim<16>" if n <= 4096 else "sim<48>" if n <= 12288 else "sim<0>")
    return names


def ef_wbar_ok(n):
    """api.hip ef_wbar_ok on the block loop's own Wt (ldw = round_up(n, 64), aligned)."""
    return n <= 16384 and n % 4 == 0


def ef_kernel(bs, ldk):
    """ef.hip pt2q_launch_ef on aligned workspaces: the EF kernel for blocks of <= 128 columns whose
    coefficient rows (ldk floats) are 16-byte aligned, else the generic GEMM (GEMM_SUB, row gather)."""
    return "ef2" if 0 < bs <= 128 and ldk % 4 == 0 else "gemm_sub"


def ef_entry_kernel(n, m, bs):
    """pt2q_error_feedback: its coefficient rows are padded to round_up(m, 4)."""
    return ef_kernel(bs, round_up(m, 4))


def atq_block_vec(n, b):
    """atq.hip pt2q_launch_atq_block: the 16-byte staged rows (full 128-column blocks, n % 16 == 0)."""
    return b == 128 and n % 16 == 0


def atq_pc_supported(dtype, m, ldw=None):
    """atq_pc.hip pt2q_atq_pc_supported for an aligned W with ldw = m unless given."""
    ldw = m if ldw is None else ldw
    E = 4 if dtype == "fp32" else 2
    if (ldw * E) % 16 or (m * E) % 16 or m <= 512:
        return False
    stage = 4 * (512 * E + 16 * E)
    return 2 * (stage + ceil_div(m, 512) * 64 * 8) <= 160 * 1024


def transpose_to_f32_fast(dtype, rows, cols, lds=None, ldd=None):
    """misc.hip pt2q_launch_transpose_to_f32: the 16-bit 64 x 64 tile kernel."""
    lds = cols if lds is None else lds
    ldd = round_up(rows, 64) if ldd is None else ldd
    return dtype in ("fp16", "bf16") and cols % 8 == 0 and rows % 4 == 0 and lds % 8 == 0 and ldd % 4 == 0


def transpose_i8_fast(rows, cols, lds, ldd, i8=True):
    """misc.hip pt2q_launch_transpose_i8: the 16-bytes-per-lane kernel."""
    return i8 and rows % 16 == 0 and cols % 16 == 0 and lds % 16 == 0 and ldd % 16 == 0


def gram_batched_supported(dtype, m):
    """engine.gram_batched_supported for contiguous, aligned activations."""
    return True if dtype == "fp32" else m % 256 == 0 and m % 8 == 0


def group_supported(n, m, b, variant_g=False):
    """api.hip group_ok (pt2q_quantize_blocks_group_supported), variant M unless variant_g."""
    return (n > 0 and m > 0 and 0 < b <= 128 and b < m < 65536 and not variant_g and n <= 16384
            and n % 4 == 0 and m % 4 == 0 and m * round_up(n, 64) * 4 < 0x80000000)


def perchannel_group_supported(m):
    return m > 512


def needs_inverse(m, bs):
    return bs < m


def gf_s1d(m, bs, batched):
    """GramsFirst.begin: per-channel groups wider than 512 get S1 / d formed once per Gram."""
    return batched and not needs_inverse(m, bs) and m > 512


def gf_upper(m, bs, dtype, batched):
    """GramsFirst.flush: upper-only Grams for per-channel 16-bit groups whose every slot went
    through the batched Gram."""
    return gf_s1d(m, bs, batched) and dtype in ("fp16", "bf16") and m % 4 == 0 and gram_batched_supported(dtype, m)


def gf_class(n, m, bs, batched):
    """GramsFirst.tails: the class a linear joins."""
    if group_supported(n, m, bs):
        return "group"
    if gf_s1d(m, bs, batched) and perchannel_group_supported(m):
        return "pc"
    return "one"


def block_loop_paths(n, m, bs, ssr, dtype, variant_g=False, codes_i8=True):
    """The forms run_blocks takes for one linear (api.hip), as a set of names."""
    B = ceil_div(m, bs) if bs < m else 1
    names = set()
    if B == 1 and m > 512 and not variant_g:
        names.add("pc:atq_pc" if atq_pc_supported(dtype, m) else "pc:atq_wide_rm")
        return names
    names.add("to_f32:" + ("tile16" if transpose_to_f32_fast(dtype, n, m) else "scalar"))
    ldw = round_up(n, 64)
    r, pre = m, False
    for _ in range(B):
        b = min(r, bs)
        nr = r - b
        if ssr and r > bs:
            names.update("ssr:" + k for k in ssr_kernels(n))
            if pre:
                names.add("ssr:wbar_from_ef")
        if variant_g and b > 128:
            names.add("hess_wide")
        names.add("atq:wide" if b > 512 else "atq:vec16" if atq_block_vec(n, b) else "atq:rows")
        if nr > 0:
            k = ef_kernel(b, m)
            names.add("ef:" + k)
            want = ssr and nr > bs and ef_wbar_ok(n)
            names.add("ef_wbar:" + ("on" if want and k == "ef2" else "off"))
            pre = want and k == "ef2"
        r = nr
    names.add("i8T:" + ("x16" if transpose_i8_fast(m, n, ldw, m, codes_i8) else "scalar"))
    return names


def layer_paths(n, m, N, bs, ssr, dtype):
    """pt2q_quantize_layer (variant M): damping form, the inverse's kernels, the block loop's forms."""
    names = {"hess:" + prepare_hessian_form(m)}
    if needs_inverse(m, bs):
        for step, k, _ in chol_schedule(m):
            names.add(step + ":" + k)
    return names | block_loop_paths(n, m, bs, ssr, dtype)


# ------------------------------------------------------------------ inputs and oracle references

def to_dtype(a, dtype):
    """fp32 numpy -> CPU torch tensor of the case's dtype (one rounding to nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DT[dtype])


def oracle_x(t):
    """A CPU activation tensor as the oracle takes it (fp32 / fp16 numpy, bf16 torch)."""
    return t if t.dtype == torch.bfloat16 else t.numpy()


def case_seed(*shape):
    return 7000 + sum((i + 1) * 131 * int(v) for i, v in enumerate(shape)) % 100000


@functools.lru_cache(maxsize=None)
def inverse_case(m):
    """-> (G, N, (Hr, damp), (Hinv, spd)) for the damped Hessian inverse of width m."""
    N = m + 50
    G = orc.gram(synth.activations(case_seed(m, 1), N, m))
    Hr, damp = orc.prepare_hessian(G, N, 0.01)
    return G, N, (Hr, damp), orc.cholesky_inverse(Hr)


def ssr_inputs(n, m, b):
    """W with a few duplicated columns and one all-zero column; rem a proper subset of the
    columns in arbitrary order."""
    W = synth.weights(case_seed(n, m, 2), n, m)
    W[:, 1::29] = W[:, :1]
    W[:, 18] = 0.0
    rng = np.random.default_rng(n + m)
    cols = rng.permutation(m)
    rem = cols[(cols % 13) != 4].astype(np.int64)
    return W, rem


@functools.lru_cache(maxsize=None)
def ssr_case(n, m, b):
    W, rem = ssr_inputs(n, m, b)
    blk, newrem = orc.select_next_block_ssr(W, rem, b)
    return W, rem, orc.ssr_similarity(W, rem), blk, newrem


def layer_inputs(n, m, N, dtype, outliers=True):
    """-> (W, X) CPU torch tensors of the case's dtype."""
    return (to_dtype(synth.weights(case_seed(n, m, 3), n, m), dtype),
            to_dtype(synth.activations(case_seed(N, m, 4), N, m, outliers=outliers), dtype))


@functools.lru_cache(maxsize=None)
def layer_m_case(n, m, N, bs, ssr, dtype):
    W, X = layer_inputs(n, m, N, dtype)
    return W, X, orc.quantize_layer_m(W.float().numpy(), oracle_x(X), block_size=bs, use_ssr=ssr)


@functools.lru_cache(maxsize=None)
def layer_g_case(n, m, N, bs, ssr):
    W, X = layer_inputs(n, m, N, "fp32", outliers=False)
    W, X = W.numpy(), X.numpy()
    Hs = np.zeros((m, m), np.float32)
    for c in np.array_split(X, 2):
        orc.gram_accumulate(Hs, c)
    return W, X, orc.quantize_layer_g(W, Hs, N, block_size=bs, use_ssr=ssr)


@functools.lru_cache(maxsize=None)
def ef_case(n, m, bs):
    """-> (W, blk, rem, E, Hinv, W after the update); rem in arbitrary order."""
    rng = np.random.default_rng(n + m + bs)
    W = synth.weights(case_seed(n, m, 5), n, m)
    cols = rng.permutation(m)
    blk, rem = cols[:bs].astype(np.int64), cols[bs:].astype(np.int64)
    E = synth.weights(case_seed(n, bs, 6), n, bs) * np.float32(0.1)
    H, _ = orc.prepare_hessian(orc.gram(synth.activations(case_seed(m, 7), 2 * m, m)), 2 * m)
    Hinv, spd = orc.cholesky_inverse(H)
    assert spd
    return W, blk, rem, E, Hinv, orc.error_feedback(W, blk, rem, E, Hinv)
