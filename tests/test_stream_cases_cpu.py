"""tests/stream_cases.py without a GPU: the table covers every stream-taking entry of
include/pt2q.h, every decoy differs from its real input and is a valid value of its kind, and --
where the oracle is cheap -- real and decoy problems have different results in every output, so a
stale read cannot hide."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import stream_cases as sc

TESTS = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def inputs(cid, seed):
    return sc.BY_ID[cid].make(seed)


def missing_entries(cases):
    return sorted(set(sc.stream_entries()) - {c.entry for c in cases})


def test_header_coverage():
    entries = sc.stream_entries()
    assert len(entries) >= 31 and "pt2q_gram" in entries and "pt2q_ternary_decode_fused" in entries
    assert "pt2q_stage_timing" not in entries and "pt2q_gram_workspace_bytes" not in entries
    assert missing_entries(sc.CASES) == []
    assert {c.entry for c in sc.CASES} <= set(entries)  # no case for a function that is gone


def test_header_coverage_notices_a_removed_case():
    for entry in sc.stream_entries():
        assert missing_entries([c for c in sc.CASES if c.entry != entry]) == [entry]
    # ... and an entry added to the header
    import tempfile
    with tempfile.NamedTemporaryFile("w", suffix=".h") as f:
        f.write(open(sc.HEADER).read() + "\nint pt2q_new_thing(const float* a,\n   int n, void* stream);\n")
        f.flush()
        assert "pt2q_new_thing" in sc.stream_entries(f.name)


REQUIRED = """gram-f32-acc0 gram-f32-acc1 gram-f32-acc2 gram-f16-streamk gram-batched-f16 gram-batched-upper-bf16
prepare-hessian-fill4 prepare-hessian-fill cholesky-inverse-80 cholesky-inverse-700 cholesky-inverse-2200
cholesky-inverse-6208 inverse-batched-131x3-chunk3 inverse-batched-384x4-chunk3 blocks-act blocks-hess blocks-none
blocks-wide blocks-per-channel-s1-given blocks-group-3x256x512 perchannel-group quantize-layer atq-stage-init-64x128
atq-stage-grid-64x128 atq-stage-round-64x128 atq-stage-itf-64x128 atq-stage-aga-64x128 atq-stage-full-64x128
atq-stage-full-64x777 s1-from-gram s1-from-gram-batched s1-from-upper-batched ssr-select cosine-similarity
ssr-static-order quadform-rows layer-report error-feedback-bs50 error-feedback-bs128 dequantize pack-ternary
unpack-ternary sum-partials fill-synthetic ternary-pack-mode0 ternary-pack-mode1 ternary-linear ternary-decode-1tok
ternary-decode-8tok decode-group-plain3 decode-group-swiglu rmsnorm decode-fused-norm-residual""".split()


def test_every_launch_form_has_a_case():
    assert set(REQUIRED) <= set(sc.BY_ID)


@pytest.mark.parametrize("c", sc.CASES, ids=repr)
def test_pinning_test_exists(c):
    path, name = c.pinned.split("::")
    assert re.search(r"^def %s\(" % re.escape(name), open(os.path.join(TESTS, path)).read(), re.M), c.pinned


def differs(a, b):
    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and a.dtype == b.dtype and not torch.equal(a, b)
    return a != b


def check_index(kind, v, real):
    a = v.numpy().astype(np.int64)
    if kind[0] == "codes2":
        assert (((a[..., None] >> np.arange(0, 8, 2)) & 3) <= 2).all()
        return
    _, lo, hi = kind
    assert a.min() >= lo and a.max() < hi
    r = real.numpy().astype(np.int64)
    if r.ndim == 1 and np.array_equal(np.sort(r), np.arange(lo, hi)):
        assert np.array_equal(np.sort(a), np.arange(lo, hi))  # a permutation stays one
    if r.ndim == 1 and len(np.unique(r)) == len(r):
        assert len(np.unique(a)) == len(a)
    if r.ndim == 1 and (np.diff(r) > 0).all():
        assert (np.diff(a) > 0).all()  # an ascending list (pt2q_ssr_select's rem) stays ascending


@pytest.mark.parametrize("c", sc.CASES, ids=repr)
def test_decoys(c):
    real, decoy = inputs(c.id, sc.REAL_SEED), inputs(c.id, sc.DECOY_SEED)
    assert real.keys() == decoy.keys() and real
    for k in real:
        assert differs(real[k], decoy[k]), k
        if isinstance(real[k], torch.Tensor) and real[k].is_floating_point():
            assert torch.isfinite(real[k].float()).all() and torch.isfinite(decoy[k].float()).all(), k  # no poison
    for k, kind in c.index.items():
        check_index(kind, real[k], real[k])
        check_index(kind, decoy[k], real[k])
    # every integer input is declared index-like (and so checked above)
    for k, v in real.items():
        if isinstance(v, torch.Tensor) and not v.is_floating_point():
            assert k in c.index, k
    names = set(real) | set(c.out)
    assert set(c.outputs) <= names and not set(c.out) & set(real) and not set(c.ws) & names
    assert set(c.status) <= set(c.ws)


ORACLE = [c for c in sc.CASES if c.oracle is not None]


@pytest.mark.parametrize("c", ORACLE, ids=repr)
def test_oracle_results_differ_between_real_and_decoy(c):
    a, b = c.oracle(inputs(c.id, sc.REAL_SEED)), c.oracle(inputs(c.id, sc.DECOY_SEED))
    assert set(a) == set(c.outputs) == set(b)
    constant = {"cholesky-inverse-80": {"info"}}.get(c.id, set())  # both SPD: info is 0 for either
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        if k not in constant:
            assert not np.array_equal(x, y), k


def test_oracle_cases_span_the_library():
    assert len(ORACLE) >= 20 and len({c.entry for c in ORACLE}) >= 14
