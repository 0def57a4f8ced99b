"""tests/ragged_cases.py on the CPU: the case lists of test_gpu_ragged.py reach every fallback they
are there for (by the helper's restatement of the launch predicates), the oracle runs every case
on a positive definite Hessian, the expectations are not degenerate, and the helper's grouped-entry
verdicts are the library's own."""
import itertools

import numpy as np
import pytest

import ragged_cases as rc
from oracle import oracle as orc


def _sched(m, batch=1):
    return rc.chol_schedule(m, batch)


def test_inverse_cases_reach_the_odd_stride_kernels():
    assert {m % 4 for m in rc.INVERSE_M} == {1, 2, 3}
    for m in rc.INVERSE_M:
        steps = _sched(m)
        # no width with m % 4 != 0 runs the one-lane kernel (its float4 stage needs 16-byte rows)
        assert {k for s, k, _ in steps if s == "block"} == {"lpr"}, m
        assert any(s == "block" and nb == rc.NB for s, _, nb in steps), m  # ... whole blocks included
        # odd ld: every strip update and every chain GEMM takes the generic non-vector kernels,
        # and every diagonal block is factored by its own launch
        assert {k for s, k, _ in steps if s == "strip"} <= {"gemm2_novec"}, m
        assert {k for s, k, _ in steps if s == "big"} == {"gemm_novec"}, m
        assert sum(s == "diag" for s, _, _ in steps) == sum(s == "block" for s, _, _ in steps), m
        assert rc.prepare_hessian_form(m) == "fill"
    assert [nb for s, _, nb in _sched(65) if s == "block"] == [64, 1]
    # 257: the 256-row sub-panel's terms as one rank-256 chain GEMM with a 1-row target
    assert ("big", "gemm_novec", {"asks": False, "M": 1, "N": 1, "K": 256}) in _sched(257)
    # 1001: two 512-panels; 1537: four, and the lauum's 84 upper tiles ask for gemmx, which refuses
    assert sum(s == "big" and d["K"] == 512 for s, _, d in _sched(1001)) == 2
    lauum = _sched(1537)[-1]
    assert lauum == ("big", "gemm_novec", {"asks": True, "M": 1537, "N": 1537, "K": 1537})
    assert not any(d["asks"] for m in rc.INVERSE_M[:-1] for s, _, d in _sched(m) if s == "big")
    # the same widths rounded to a multiple of 4 take the fast forms: the predicates do flip
    fast = _sched(1540)
    assert {k for s, k, _ in fast if s == "block" and _ == rc.NB} == {"lane"}
    assert {k for s, k, _ in fast if s == "strip"} == {"rank_update2"}
    assert fast[-1][1] == "gemmx" and rc.prepare_hessian_form(1540) == "fill4"


def test_batched_inverse_cases_have_odd_item_strides():
    for m, batch, chunk in rc.BATCHED_INVERSE:
        assert (m * m) % 4 != 0 and batch >= 2
        steps = _sched(m, batch)
        assert {k for s, k, _ in steps if s == "block"} == {"lpr"}
        assert {k for s, k, _ in steps if s == "big"} == {"gemm_novec"}
        # chunk < batch: the second launch sequence starts at an item whose base is only 4-byte aligned
        if chunk < batch:
            assert (chunk * m * m) % 4 != 0
            assert rc.prepare_hessian_form(m, chunk * m * m) == "fill"
    assert any(chunk < batch for _, batch, chunk in rc.BATCHED_INVERSE)
    assert any(d["K"] == 512 for s, _, d in _sched(1001, 2) if s == "big")


def test_ssr_cases_reach_every_unfused_kernel():
    seen = {}
    for n, m, b in rc.SSR:
        seen[n] = rc.ssr_kernels(n)
        assert "wbar_fused" not in seen[n] and seen[n][-1] == "sim<0>", n
    assert seen[203] == seen[4099] == ["wbar_partial", "wbar_sumfinal", "sim<0>"]
    assert seen[12291] == ["wbar_partial", "wbar_sum", "wbar_final", "sim<0>"]
    assert seen[16388] == ["wbar_partial", "wbar_sum", "wbar_final", "sim<0>"] and 16388 % 4 == 0
    assert 4099 > 4096 and 12291 > rc.SUMN_LDS_MAX and 16388 > 16384
    # ... which the nearest aligned row counts do not take
    assert rc.ssr_kernels(204) == ["wbar_fused", "sim<16>"] and rc.ssr_kernels(12292)[-1] == "sim_split<4>"
    assert rc.ssr_kernels(4100) == ["wbar_fused", "sim_split<2>"] and rc.ssr_kernels(12288)[-1] == "sim_split<3>"
    assert rc.ssr_kernels(8192, fusable=False)[-1] == "sim_split<2>" and rc.ssr_kernels(4096, ldw=4099)[-1] == "sim<0>"


@pytest.mark.parametrize("n,m,b", rc.SSR)
def test_ssr_expectations_are_not_degenerate(n, m, b):
    W, rem, sim, blk, newrem = rc.ssr_case(n, m, b)
    assert 128 < len(rem) < m and not np.array_equal(rem, np.sort(rem))  # a proper subset, unsorted
    assert np.isfinite(sim).all()
    assert len(blk) == b and not np.array_equal(blk, rem[:b])  # the pick is no identity
    assert sorted(np.concatenate([blk, newrem])) == sorted(rem)
    # exact ties (duplicated columns) and the all-zero column are inside rem
    dup = [c for c in range(1, m, 29) if c in set(rem)]
    assert len(dup) >= 3 and 0 in rem and 18 in rem and not W[:, 18].any()
    pos = {c: i for i, c in enumerate(rem)}
    assert len({sim[pos[c]].tobytes() for c in dup + [0]}) == 1


def test_ef_entry_cases_take_both_paths():
    assert [rc.ef_entry_kernel(*c) for c in rc.EF] == ["ef2", "gemm_sub"]
    for n, m, bs in rc.EF:
        assert n % 4 and m % 4 and bs < m
    assert rc.ef_kernel(128, 204) == "ef2" and rc.ef_kernel(129, 204) == "gemm_sub" == rc.ef_kernel(64, 203)


def test_layer_cases_reach_every_fallback():
    per_case = {c: rc.layer_paths(*c) for c in rc.LAYER_M}
    union = set().union(*per_case.values())
    for name in ("hess:fill", "diag:chol_diag", "block:lpr", "strip:gemm2_novec", "big:gemm_novec",
                 "to_f32:scalar", "ssr:wbar_partial", "ssr:wbar_sumfinal", "ssr:sim<0>", "atq:rows",
                 "ef:gemm_sub", "ef_wbar:off", "i8T:scalar"):
        assert name in union, name
    # and none of the forms those conditions switch off
    for name in ("hess:fill4", "block:lane", "strip:rank_update2", "big:gemmx", "big:gemm_vec", "to_f32:tile16",
                 "ssr:wbar_fused", "ssr:wbar_from_ef", "atq:vec16", "ef:ef2", "ef_wbar:on", "i8T:x16"):
        assert name not in union, name
    for (n, m, N, bs, ssr, dt), names in per_case.items():
        assert rc.ceil_div(m, bs) >= 2 and not rc.ef_wbar_ok(n) and not rc.atq_block_vec(n, bs)
        assert ("ssr:sim<0>" in names) == ssr
    assert {c[5] for c in rc.LAYER_M} == {"fp32", "fp16", "bf16"} and rc.LAYER_M_F32_CODES in rc.LAYER_M
    assert rc.GRAPH_LAYER in rc.LAYER_M
    # the aligned neighbour of the first case takes every fast form
    near = rc.layer_paths(208, 384, 450, 128, True, "fp16")
    assert {"hess:fill4", "block:lane", "strip:rank_update2", "to_f32:tile16", "ssr:wbar_fused", "ssr:wbar_from_ef",
            "atq:vec16", "ef:ef2", "ef_wbar:on", "i8T:x16"} <= near


def test_layer_cases_with_ragged_rows_alone():
    for case in rc.LAYER_M_ROWS:
        names = rc.layer_paths(*case)
        assert {"hess:fill4", "block:lane", "strip:rank_update2", "to_f32:scalar", "ssr:wbar_partial", "ssr:sim<0>",
                "atq:rows", "ef:ef2", "ef_wbar:off", "i8T:scalar"} <= names, case
        assert not names & {"ef:gemm_sub", "ef_wbar:on", "ssr:wbar_fused", "ssr:wbar_from_ef", "to_f32:tile16"}, case
    assert {c[5] for c in rc.LAYER_M_ROWS} == {"fp32", "fp16"}


def test_residues_of_m_and_n():
    """The inverse, SSR and layer cases together reach every non-zero residue of m % 4 and n % 4."""
    ms = rc.INVERSE_M + [c[1] for c in rc.SSR + rc.LAYER_M + rc.PER_CHANNEL + rc.LAYER_G]
    ns = [c[0] for c in rc.SSR + rc.LAYER_M + rc.PER_CHANNEL + rc.LAYER_G]
    assert {m % 4 for m in ms} >= {1, 2, 3} and {n % 4 for n in ns} >= {1, 2, 3}
    assert {c[1] % 4 for c in rc.LAYER_M + rc.PER_CHANNEL} >= {1, 2, 3}
    assert {c[0] % 4 for c in rc.LAYER_M + rc.PER_CHANNEL} >= {1, 2, 3}


def test_per_channel_cases_are_refused_by_the_streamed_kernel():
    for n, m, N, bs, dt in rc.PER_CHANNEL:
        assert bs >= m > 512 and not rc.atq_pc_supported(dt, m)
        assert rc.block_loop_paths(n, m, bs, True, dt) == {"pc:atq_wide_rm"}
    assert rc.atq_pc_supported("fp32", 516) and rc.atq_pc_supported("bf16", 520) and not rc.atq_pc_supported("fp16", 516)
    # 16-bit weights of odd width: rows start on 2-byte boundaries
    assert any(dt != "fp32" and m % 2 for _, m, _, _, dt in rc.PER_CHANNEL)
    assert {dt for *_, dt in rc.PER_CHANNEL} == {"fp32", "fp16", "bf16"}


def test_variant_g_cases():
    paths = {c[3]: rc.block_loop_paths(c[0], c[1], c[3], c[4], "fp32", variant_g=True, codes_i8=False)
             for c in rc.LAYER_G}
    assert "hess_wide" not in paths[64] and "ssr:sim<0>" in paths[64] and "ef:gemm_sub" in paths[64]
    assert "hess_wide" in paths[150] and "ef:gemm_sub" in paths[150]   # a 150-wide hS product, odd ld
    assert "hess_wide" in paths[203] and not any(p.startswith(("ef:", "ssr:")) for p in paths[203])  # one block
    assert all(rc.ef_kernel(min(bs, 128), 203) == "gemm_sub" for bs in paths)


def test_grams_first_units_mix_the_paths():
    for bs, (batched, group) in itertools.product(rc.GF_BLOCK_SIZES, rc.GF_MODES):
        classes = {}
        for m, dt, ns, N in rc.GF_UNITS:
            for n in ns:
                classes[(n, m)] = rc.gf_class(n, m, bs, batched)
            if m == 333:  # per-item Grams (16-bit, m % 256) and "one" loops
                assert not rc.gram_batched_supported(dt, m) or dt == "fp32"
                assert all(classes[(n, m)] == "one" for n in ns)
            assert not (m == 515 and rc.gf_upper(m, bs, dt, batched))
        assert classes[(384, 512)] == ("group" if bs == 128 else "one")
        assert classes[(61, 515)] == ("pc" if bs == 1024 and batched else "one")
    assert not rc.gram_batched_supported("fp16", 333) and not rc.gram_batched_supported("bf16", 515)
    assert rc.gram_batched_supported("fp16", 512) and rc.gram_batched_supported("fp32", 333)
    # the upper rule does fire at the width the per-channel grams-first test uses
    assert rc.gf_upper(1024, 1024, "bf16", True) and not rc.gf_upper(1024, 1024, "bf16", False)
    assert not rc.gf_upper(1024, 128, "bf16", True) and not rc.gf_upper(1024, 1024, "fp32", True)


def test_group_supported_matches_the_library(pt2q):
    lib, L = pt2q._lib.lib(), pt2q._lib
    shapes = {(c[0], c[1], c[3]) for c in rc.LAYER_M + rc.LAYER_M_ROWS + rc.PER_CHANNEL + rc.LAYER_G}
    shapes |= {(n, m, bs) for m, _, ns, _ in rc.GF_UNITS for n in ns for bs in rc.GF_BLOCK_SIZES}
    shapes |= {(208, 384, 128), (4096, 4096, 128), (4096, 4098, 128), (4098, 4096, 128), (4096, 4096, 256),
               (4096, 128, 128), (16388, 512, 128), (16384, 40000, 128)}
    for n, m, b in sorted(shapes):
        for flags, g in ((L.FLAG_SSR | L.AGA_ACT, False), (L.AGA_ACT, False), (L.FLAG_SSR | L.AGA_HESS, True)):
            assert rc.group_supported(n, m, b, variant_g=g) == bool(lib.pt2q_quantize_blocks_group_supported(n, m, b, flags)), \
                (n, m, b, flags)
    assert any(rc.group_supported(*s) for s in shapes) and not all(rc.group_supported(*s) for s in shapes)
    assert pt2q.engine.perchannel_group_supported(515) == rc.perchannel_group_supported(515)
    assert pt2q.engine.needs_inverse(515, 1024) == rc.needs_inverse(515, 1024)


# ------------------------------------------------------------------ the oracle on every case

@pytest.mark.parametrize("m", rc.INVERSE_M + sorted({c[0] for c in rc.BATCHED_INVERSE}))
def test_oracle_inverse_is_spd(m):
    orc.set_threads(16)
    G, N, (Hr, damp), (Hinv, spd) = rc.inverse_case(m)
    assert spd and N == m + 50 and damp > 0 and np.isfinite(Hinv).all()
    assert np.array_equal(Hinv, Hinv.T)


def _check_layer(ref, n, m, bs):
    assert ref["spd"]
    assert set(np.unique(ref["T"])) == {-1, 0, 1}  # all three codes
    assert np.array_equal(np.sort(ref["perm"]), np.arange(m))
    assert np.isfinite(ref["alpha"]).all() and np.isfinite(ref["mu"]).all()
    # every block but a ragged last one (257 = 4 * 64 + 1: a one-column block is constant per row,
    # which ends the fit at iteration 0) runs the iterative fit
    assert (ref["iters"][: max(1, len(ref["iters"]) - 1)] > 0).all()
    assert ref["alpha"].shape == (n, rc.ceil_div(m, bs) if bs < m else 1)


@pytest.mark.parametrize("case", rc.LAYER_M + rc.LAYER_M_ROWS + rc.PER_CHANNEL, ids=lambda c: "-".join(map(str, c)))
def test_oracle_layer_m_cases(case):
    orc.set_threads(16)
    if len(case) == 5:
        n, m, N, bs, dt = case
        ssr = True
    else:
        n, m, N, bs, ssr, dt = case
    W, X, ref = rc.layer_m_case(n, m, N, bs, ssr, dt)
    _check_layer(ref, n, m, bs)
    if bs < m:
        assert ref["alpha"].shape[1] >= 2
        assert np.array_equal(ref["perm"], np.arange(m)) != ssr  # SSR reorders, sequential does not
    else:
        assert np.array_equal(ref["perm"], np.arange(m))


@pytest.mark.parametrize("case", rc.LAYER_G, ids=lambda c: "-".join(map(str, c)))
def test_oracle_layer_g_cases(case):
    n, m, N, bs, ssr = case
    W, X, ref = rc.layer_g_case(*case)
    _check_layer(ref, n, m, bs)
    assert (ref["alpha"].shape[1] >= 2) == (bs < m)


@pytest.mark.parametrize("case", rc.EF)
def test_oracle_ef_cases(case):
    W, blk, rem, E, Hinv, ref = rc.ef_case(*case)
    assert np.array_equal(ref[:, blk], W[:, blk]) and not np.array_equal(ref[:, rem], W[:, rem])
    assert not np.array_equal(rem, np.sort(rem)) and np.isfinite(ref).all()


def test_oracle_grams_first_units_are_spd():
    for k, (m, dt, ns, N) in enumerate(rc.GF_UNITS):
        W, X = rc.layer_inputs(ns[0], m, N, dt)
        H, _ = orc.prepare_hessian(orc.gram_any(rc.oracle_x(X)), N, 0.01)
        assert orc.cholesky_inverse(H)[1], (m, dt)
