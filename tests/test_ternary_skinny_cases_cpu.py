"""tests/ternary_skinny_cases.py on the CPU: the restated plan of csrc/ternary_skinny.hip equals the
library's two workspace queries over a sweep of its edges (the shared library loads without a GPU), the
small tables of the skinny GPU tests have the splits their comments give and only short K slices, the
long tables reach every plan class, and the exact data of every new shape stays order-free."""
import ctypes

import numpy as np
import pytest

import ternary_linear_ref as ref
import ternary_skinny_cases as tc

TOKENS = [1, 2, 16, 17, 32, 33, 48, 49, 64]
NS = [1, 63, 64, 65, 2047, 2048, 2049, 8127, 8128, 8129, 16319, 16320, 16321, 32703, 32704, 32705]
MS = sorted({k for k in range(128, 14337, 128)} |
            {k + d for k in (128, 256, 384, 512, 896, 1024, 4096, 8192, 11008, 13824, 14336) for d in (-1, 1)})


def _ints(v):
    return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)


def test_plan_equals_the_lone_workspace_query(pt2q):
    query = pt2q._lib.lib().pt2q_ternary_skinny_workspace_bytes
    for tokens in TOKENS:
        for n in NS:
            for m in MS:
                p = tc.skinny_plan(tokens, n, m)
                assert query(tokens, n, m) == p["workspace"], (tokens, n, m)
                assert sum(p["nb"]) == p["nkb"] and len(p["nb"]) == p["splits"] and min(p["nb"]) >= 1
    for tokens, n, m in ((0, 64, 128), (65, 64, 128), (-1, 64, 128), (2, 0, 128), (2, 64, 0)):
        assert tc.skinny_plan(tokens, n, m) is None and query(tokens, n, m) == 0


def test_plan_equals_the_group_workspace_query(pt2q):
    query = pt2q._lib.lib().pt2q_ternary_skinny_group_workspace_bytes
    groups = [(64,), (65, 1), (2049, 64, 130), (16321, 65), (32705, 65, 1, 8129), (8128, 8128), (16321, 16321), (65, 65)]
    for tokens in TOKENS:
        for ns in groups:
            for m in MS[::3] + [14336]:
                for epilogue in (0, 1):
                    g = tc.skinny_group_plan(tokens, m, ns, epilogue)
                    assert query(tokens, m, len(ns), _ints(ns), epilogue) == (g["workspace"] if g else 0), (tokens, m, ns)
                    if epilogue and len(ns) == 2 and ns[0] == ns[1]:
                        assert g["ticket_target"] == 2 * g["members"][0]["splits"] and g["ncnt"] == g["members"][0]["tiles"]
                        assert all(p["part_bytes"] > 0 for p in g["members"])
    refused = [(0, 512, (64, 64), 1), (65, 512, (64, 64), 1), (65, 512, (64,), 0), (0, 512, (64,), 0),
               (17, 512, (64, 33), 1), (17, 512, (64,) * 3, 1), (17, 512, (64,) * 5, 0), (17, 512, (64, 0), 0),
               (17, 512, (64,), 2)]
    for tokens, m, ns, epilogue in refused:
        assert tc.skinny_group_plan(tokens, m, ns, epilogue) is None
        assert query(tokens, m, len(ns), _ints(ns), epilogue) == 0, (tokens, m, ns, epilogue)
    assert tc.skinny_group_plan(17, 512, (64, 65), 0) is not None  # unequal n is SWIGLU's refusal only


def test_plan_examples():
    """The shapes the kernel was written and timed for: splits and blocks per slice."""
    for (n, m), splits, nbs in (((4096, 4096), 8, {4}), ((11008, 4096), 3, {10, 11}), ((4096, 11008), 8, {10, 11}),
                                ((32000, 4096), 2, {16})):
        p = tc.skinny_plan(8, n, m)
        assert p["splits"] == splits and set(p["nb"]) == nbs, (n, m, p)


def test_small_tables_have_the_splits_their_comments_give():
    assert [tc.skinny_plan(t, n, m)["splits"] for n, m, _, t, _ in tc.SHAPES] == tc.SHAPES_SPLITS
    assert tc.skinny_plan(17, 65, 640)["nb"] == [2, 3]
    assert [[p["splits"] for p in tc.skinny_group_plan(t, m, ns, 0)["members"]] for m, _, t, ns in tc.PLAIN] == tc.PLAIN_SPLITS
    assert [tc.skinny_group_plan(t, m, (n, n), 1)["members"][0]["splits"] for m, _, t, n in tc.SWIGLU] == tc.SWIGLU_SPLITS
    assert {tc.skinny_plan(t, n, m)["NT"] for n, m, _, t, _ in tc.SHAPES} == {1, 2, 3, 4}


def _small():
    return tc.runs_of(lone=tc.SHAPES, plain=tc.PLAIN, swiglu=tc.SWIGLU + tc.NORM_SWIGLU, norm=tc.NORM_SHAPES)


def _long():
    return tc.runs_of(lone=tc.LONG, wide=tc.WIDE, plain_1dt=tc.PLAIN_LONG, swiglu=tc.SWIGLU_LONG,
                      norm=[tc.NORM_LONG, tc.NORM_RES_LONG])


def test_small_tables_only_reach_short_slices():
    """What the long tables are there for: in the small ones the split is the cap (but for the 512-tile
    member, which wants 1), a slice has at most 4 blocks, and 4 only once, on that member's direct-store
    path at NT = 1; no class of CLASSES is reached."""
    plans = [p for r in _small() for p in r[3]]
    assert len(plans) > 80
    assert all(p["splits"] == p["cap"] <= p["want"] for p in plans if p["n"] != 32705)
    assert all(max(p["nb"]) <= 3 for p in plans if p["splits"] >= 2)
    four = {(p["n"], p["m"], p["NT"], p["splits"]) for p in plans if max(p["nb"]) >= 4}
    assert four == {(32705, 512, 1, 1)}
    assert tc.classes_of(_small()) == set()


def test_long_tables_reach_every_class():
    got = tc.classes_of(_long())
    assert got == set(tc.CLASSES), sorted(set(tc.CLASSES) - got)
    assert len(tc.CLASSES) == len(set(tc.CLASSES)) == 19


def test_long_tables_have_the_plans_their_comments_give():
    def plan(s):
        return tc.skinny_plan(s[3], s[0], s[1])
    assert [(plan(s)["NT"], plan(s)["splits"], sorted(set(plan(s)["nb"]))) for s in tc.LONG] == [
        (1, 16, [4]), (2, 16, [5]), (3, 16, [6, 7]), (4, 16, [7])]
    assert [(plan(s)["tiles"], plan(s)["want"], plan(s)["cap"], plan(s)["splits"], plan(s)["nb"], plan(s)["NT"])
            for s in tc.WIDE] == [(256, 2, 4, 2, [4, 4], 3), (171, 3, 6, 3, [4, 4, 4], 2), (512, 1, 3, 1, [7], 4)]
    assert plan(tc.WIDE[0])["part_bytes"] == 6 * tc.MIB
    assert {s[5] for s in tc.WIDE} == {"fp16", "bf16"}
    m, _, tokens, ns, _ = tc.PLAIN_LONG[0]
    g = tc.skinny_group_plan(tokens, m, ns, 0)
    assert [(p["splits"], p["nb"]) for p in g["members"]] == [(2, [4, 4]), (4, [2, 2, 2, 2])] and g["grid"] == (258, 4)
    m, _, tokens, n = tc.SWIGLU_LONG[0]
    g = tc.skinny_group_plan(tokens, m, (n, n), 1)
    assert g["ticket_target"] == 32 and set(g["members"][0]["nb"]) == {5}
    for m, _, tokens, ns in (tc.NORM_LONG, tc.NORM_RES_LONG):
        assert m >= 8192 and all(max(p["nb"]) >= 4 for p in tc.skinny_group_plan(tokens, m, ns, 0)["members"])


@pytest.mark.parametrize("n,m,bs,tokens", [s[:4] for s in tc.LONG])
def test_exactness_bound_holds_on_long_slices(n, m, bs, tokens):
    """exact_units asserts |any partial sum| < 2**20 units, for both compat modes (the wide shapes run
    that assertion in their GPU test: their integer reference takes seconds)."""
    c = ref.exact_case(n, m, bs, tokens, ref.case_seed(n, m, bs, tokens))
    for compat in (False, True):
        assert np.abs(ref.exact_units(c, compat, bias=True)).max() < ref.EXACT_BOUND


def test_group_bound_holds_on_long_slices():
    """The order-free bound of the grouped tests (88 m + 512 units, test_gpu_ternary_skinny_group.py)."""
    for m in [s[0] for s in tc.PLAIN_LONG + tc.SWIGLU_LONG]:
        assert 88 * m + 512 < ref.EXACT_BOUND
