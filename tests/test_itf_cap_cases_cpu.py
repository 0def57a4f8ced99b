"""tests/itf_cap_cases.py on the CPU: the cases of test_gpu_itf_cap.py bite.  Every case runs ITF for
k >= 5 applications when uncapped; every cap below k changes the oracle's bits against the uncapped
result and against the next cap (a kernel that ignores the cap, or is off by one, cannot pass); at
the cap some waves have stopped on their own and others are cut; the cases reach every ATQ kernel
(by the launch predicates of tests/ragged_cases.py); and a negative cap is refused by all five C
entries before any device work."""
import numpy as np
import pytest

import itf_cap_cases as ic
import ragged_cases as rc

STAGE_IDS = ["%dx%d" % c for c in ic.STAGE]


def _parts(r):
    """(alpha, mu, T) bytes of a result: (alpha, mu, T, iters) or the block loop's dict."""
    a, mu, T = (r["alpha"], r["mu"], r["T"]) if isinstance(r, dict) else r[:3]
    return a.tobytes(), mu.tobytes(), T.tobytes()


def _differs(a, b):
    """alpha or T bits differ."""
    return _parts(a)[0] != _parts(b)[0] or _parts(a)[2] != _parts(b)[2]


def _check_bite(ref, iters_of):
    """a, b and c of the cases' contract for one case: ref(cap, aga) -> result; -> k per flavour."""
    ks = {}
    for aga in (False, True):
        full = ref(ic.UNCAPPED, aga)
        k = ks[aga] = iters_of(full)
        assert 5 <= k < ic.UNCAPPED - 1, k                                   # a
        for c in ic.caps(k):
            r = ref(c, aga)
            assert iters_of(r) == min(c, k), (c, aga)
            if c >= k:                                                       # c: k and k + 1 are the uncapped run
                assert _parts(r) == _parts(full), (c, aga)
            elif not aga:                                                    # b: on the grid ITF leaves
                assert _differs(r, full) and _differs(r, ref(c + 1, aga)), c
            else:
                # after an AGA the grid follows the codes alone, and the k-th application changes
                # no code: the cut at k - 1 shows in the iteration count only
                assert _differs(r, full) == _differs(r, ref(c + 1, aga)) == (c < k - 1), c
    return ks


@pytest.mark.parametrize("case", ic.STAGE, ids=STAGE_IDS)
def test_stage_cases_bite(case):
    ks = _check_bite(lambda c, aga: ic.stage_ref(*case, c, aga), lambda r: r[3])
    assert ks[False] == ks[True] == ic.stage_k(*case)


@pytest.mark.parametrize("case", ic.BLOCKS, ids=lambda c: "-".join(map(str, c)))
def test_block_loop_cases_bite(case):
    n, m, bs = case
    ks = _check_bite(lambda c, aga: ic.blocks_ref(n, m, bs, c, aga), lambda r: int(r["iters"].max()))
    assert ks == {aga: ic.blocks_k(n, m, bs, aga=aga) for aga in (False, True)}
    full = ic.blocks_ref(n, m, bs, ic.UNCAPPED, True)
    assert len(full["iters"]) == rc.ceil_div(m, bs) >= 2 and (full["iters"] >= 3).all()
    # a capped block's result reaches the next block's input: at a cap that cuts block 0, the
    # columns SSR picks next or their codes differ from the uncapped run's
    cut = ic.blocks_ref(n, m, bs, 2, True)
    assert (cut["iters"] == 2).all()
    assert not np.array_equal(cut["W_final"], full["W_final"])
    assert not (np.array_equal(cut["perm"][bs:], full["perm"][bs:]) and
                np.array_equal(cut["T"][:, full["perm"][bs:]], full["T"][:, full["perm"][bs:]]))


def test_grouped_block_loop_members_bite():
    count, n, m, bs = ic.GROUP_BLOCKS
    assert rc.group_supported(n, m, bs) and count == 3
    for z in range(count):
        _check_bite(lambda c, aga: ic.blocks_ref(n, m, bs, c, aga, tag=11 + 2 * z), lambda r: int(r["iters"].max()))
    assert len({ic.blocks_inputs(n, m, 11 + 2 * z)[0].tobytes() for z in range(count)}) == count


@pytest.mark.parametrize("case", ic.PER_CHANNEL, ids=lambda c: "-".join(map(str, c)))
def test_per_channel_cases_bite(case):
    n, m, dt = case
    ks = _check_bite(lambda c, aga: ic.pc_ref(n, m, dt, c, aga), lambda r: r[3])
    assert ks[False] == ks[True] == ic.pc_k(*case)


@pytest.mark.parametrize("case", ic.PC_GROUPS, ids=lambda c: "%d-%s" % c[1:])
def test_per_channel_group_members(case):
    ns, m, dt = case
    assert len(set(ns)) == len(ns) == 3 and rc.perchannel_group_supported(m)
    for n, tag, zero in ic.pc_group_members(ns, m, dt):
        if zero:  # quantizer.py:164 stops at iteration 0 and the init grid of an all-zero block is 0, 0
            for c in (0, 2, ic.UNCAPPED):
                a, mu, T, it = ic.pc_ref(n, m, dt, c, True, tag, True)
                assert it == 0 and not a.any() and not mu.any() and not T.any()
        else:
            assert ic.pc_k(n, m, dt, tag) >= 5
            assert ic.pc_ref(n, m, dt, 2, True, tag)[3] == 2


def test_layer_case_bites():
    n, m, N, bs = ic.LAYER
    W, X, cut = ic.layer_case()
    _, _, full = ic.layer_case(ic.UNCAPPED)
    assert cut["spd"] and (cut["iters"] == ic.LAYER_CAP).all() and (full["iters"] >= 5).all()
    assert _differs(cut, full) and rc.ceil_div(m, bs) == 3


def _wave_groups(kr):
    """Per aligned group of four consecutive rows (one wave's rows): the rows' natural counts."""
    return [kr[i:i + 4] for i in range(0, len(kr), 4)]


def test_waves_stop_on_their_own_beside_cut_ones():
    """d: the narrow 128-column cases at cap 2 -- at least one wave whose every row has converged
    (<= 2 applications: the wave-level stop fires at or before the cap) and at least one that is cut."""
    blocks = [("stage", ic.stage_inputs(67, 128)[0])]
    for n, m, bs in [c for c in ic.BLOCKS if c[2] == 128] + [ic.GROUP_BLOCKS[1:]]:
        tag = 11 if (n, m, bs) == ic.GROUP_BLOCKS[1:] else 3
        W = ic.blocks_inputs(n, m, tag)[0]
        blocks.append(((n, m, bs), W[:, ic.blocks_ref(n, m, bs, ic.UNCAPPED, True, tag)["perm"][:bs]]))
    n, m, N, bs = ic.LAYER
    blocks.append(("layer", ic.layer_case()[0][:, ic.layer_case()[2]["perm"][:bs]]))
    assert len(blocks) == 5
    for name, Wb in blocks:
        assert Wb.shape[1] == 128
        groups = _wave_groups(ic.row_counts(np.ascontiguousarray(Wb)))
        done = [g for g in groups if g.max() <= 2]
        assert done and any(g.min() > 2 for g in groups), name
        assert any(g.max() == 1 for g in done), name            # the three-level rows: stopped before the cap
        assert any(g.min() <= 2 < g.max() for g in groups), name  # and waves that mix both kinds of row


def test_cases_reach_every_atq_kernel():
    """e"""
    union = set()
    for n, m, bs in ic.BLOCKS:
        union |= rc.block_loop_paths(n, m, bs, True, "fp32")
    per_pc = {c: ic.pc_paths(*c) for c in ic.PER_CHANNEL}
    union |= set().union(*per_pc.values())
    for name in ("atq:vec16", "atq:rows", "atq:wide", "pc:atq_pc", "pc:atq_wide_rm", "pc:atq_pcr"):
        assert name in union, name
    assert "atq:vec16" in rc.block_loop_paths(*ic.BLOCKS[0], True, "fp32")
    assert "atq:rows" in rc.block_loop_paths(*ic.BLOCKS[1], True, "fp32") and ic.BLOCKS[1][1] % ic.BLOCKS[1][2] == 44
    assert {"atq:wide", "atq:rows"} <= rc.block_loop_paths(*ic.BLOCKS[2], True, "fp32")  # 640, 640, 320
    assert "atq:vec16" in rc.block_loop_paths(*ic.GROUP_BLOCKS[1:], True, "fp32")
    assert "atq:vec16" in rc.block_loop_paths(*ic.LAYER[:2], ic.LAYER[3], True, "fp32")
    assert [sorted(per_pc[c]) for c in ic.PER_CHANNEL] == [
        sorted(rc.block_loop_paths(64, 256, 256, True, "fp32")), ["pc:atq_pc"], ["pc:atq_pc"], ["pc:atq_wide_rm"],
        ["pc:atq_wide_rm"], ["pc:atq_pc", "pc:atq_pcr"]]
    assert "atq:rows" in per_pc[ic.PER_CHANNEL[0]]              # one 256-column block: the narrow kernel, NS = 16
    assert ic.PCR_M == 5120 and ic.PC_COLS == 512               # the width of the register-resident kernel
    assert [sorted(ic.pc_paths(n, m, dt)) for ns, m, dt in ic.PC_GROUPS for n in ns[:1]] == [
        ["pc:atq_pc"], ["pc:atq_wide_rm"], ["pc:atq_pc", "pc:atq_pcr"]]
    # the stage entry: NS = 8 full and partial, b = 16, and two widths past the 512 the row kernels hold
    assert [(b <= 512, b % 16) for _, b in ic.STAGE] == [(True, 0), (True, 4), (True, 0), (False, 0), (False, 12)]
    # the plumbing units: a grouped and a lone loop at 128, the per-channel group at 2048
    cls = {bs: {rc.gf_class(n, m, bs, True) for m, dt, ns, N in units for n in ns} for bs, units in ic.PLUMB.items()}
    assert cls == {128: {"group", "one"}, 2048: {"pc"}}


def test_negative_cap_is_refused_without_device(pt2q):
    """f: max_iter = -1 is PT2Q_E_ARG from all five entries, before any device work."""
    E_ARG = 1
    calls, keep = ic.negative_cap_calls(pt2q._lib.lib())
    assert len(calls) == 5
    for name, call in calls.items():
        assert call(-1) == E_ARG, name
        assert call(-(2 ** 31)) == E_ARG, name
