"""The launch plan of the 2..64-token ternary kernel (csrc/ternary_skinny.hip: ts_plan, ts_group_plan)
restated on the CPU, and the shape tables of the three skinny GPU test files -- a plain helper, not a
conftest.  tests/test_ternary_skinny_cases_cpu.py pins the restatement to the library's two workspace
queries and checks that the tables reach every plan class listed in CLASSES.

Why the plan matters to the tests.  ts_body stages x through a 3-slot LDS ring loaded two stages ahead.
A K slice of nb blocks first overwrites a slot that has been read at nb >= 4 (dma(j + 2) into slot
(j - 1) % 3) and goes round the ring a second time at nb >= 7; the steady-state iteration (fetch, DMA,
vmcnt(NT) with an older DMA in flight, the barrier that frees slot j - 1) does not exist for nb <= 3.
The plan gives small shapes short slices: with n <= 200 and m <= 2100 every slice has 1..3 blocks.
SHAPES / PLAIN / SWIGLU are those small tables (ragged edges, scale-block edges, every NT); LONG, WIDE
and the *_LONG tables are the shapes whose slices wrap the ring, whose split count comes from the
workgroup target and not from the cap, and whose partial tiles outgrow one XCD's 4 MiB L2."""
F = 64            # TS_F: features per workgroup
PB = 128          # TS_PB: positions per packed block
WGS = 512         # TS_WGS: workgroups the plan aims at
MAX_TOKENS = 64   # TS_MAX_TOKENS
GROUP_MAX = 4     # PT2Q_DECODE_GROUP_MAX
PLAIN_EPILOGUE, SWIGLU_EPILOGUE = 0, 1
MIB = 1 << 20


def _up256(v):
    return -(-v // 256) * 256


def skinny_plan(tokens, n, m):
    """ts_plan and pt2q_ternary_skinny_workspace_bytes.  nb: the 128-position blocks of every K slice,
    (z + 1) nkb // splits - z nkb // splits as ts_body cuts them.  None for a call the query answers with 0."""
    if not (0 < tokens <= MAX_TOKENS and n > 0 and m > 0):
        return None
    P = -(-m // PB) * PB
    tiles, nkb = -(-n // F), P // PB
    cap = max(1, min(16, nkb // 2))
    want = -(-WGS // tiles)
    splits = min(want, cap)
    p = {"tokens": tokens, "n": n, "m": m, "P": P, "tiles": tiles, "nkb": nkb, "cap": cap, "want": want,
         "splits": splits, "NT": -(-tokens // 16),
         "nb": [(z + 1) * nkb // splits - z * nkb // splits for z in range(splits)],
         "xs_bytes": _up256(tokens * P * 2), "cnt_bytes": _up256(tiles * 4),
         "part_bytes": splits * tokens * tiles * F * 4 if splits > 1 else 0}
    p["workspace"] = p["xs_bytes"] + p["cnt_bytes"] + p["part_bytes"] + 256
    return p


def skinny_group_plan(tokens, m, ns, epilogue):
    """ts_group_plan and pt2q_ternary_skinny_group_workspace_bytes: every member's own plan (SWIGLU:
    partial tiles whatever the split), the tickets the last workgroup of a SWIGLU tile draws, the
    counters and the workspace.  None for a call the query answers with 0."""
    if not (0 < tokens <= MAX_TOKENS and m > 0 and 1 <= len(ns) <= GROUP_MAX):
        return None
    swiglu = epilogue == SWIGLU_EPILOGUE
    if not swiglu and epilogue != PLAIN_EPILOGUE:
        return None
    if swiglu and (len(ns) != 2 or ns[0] != ns[1]):
        return None
    if min(ns) <= 0:
        return None
    mem = [skinny_plan(tokens, n, m) for n in ns]
    for p in mem:
        if swiglu:
            p["part_bytes"] = p["splits"] * tokens * p["tiles"] * F * 4
        if p["part_bytes"] >= 1 << 31:  # the kernels' 32-bit byte offsets
            return None
    ncnt = mem[0]["tiles"] if swiglu else sum(p["tiles"] for p in mem)
    return {"members": mem, "swiglu": swiglu, "ticket_target": mem[0]["splits"] + mem[1]["splits"] if swiglu else None,
            "ncnt": ncnt, "grid": (sum(p["tiles"] for p in mem), max(p["splits"] for p in mem)),
            "workspace": len(ns) * mem[0]["xs_bytes"] + _up256(ncnt * 4) + sum(p["part_bytes"] for p in mem) + 256}


# ---- tests/test_gpu_ternary_skinny.py.  (n, m, bs, tokens, compat of the fp16 run; bf16 takes the other).
# The splits in brackets are asserted by the CPU test (SHAPES_SPLITS below).
SHAPES = [
    (1, 100, 16, 2, False),       # [1] one split, direct store; 16-position tables
    (40, 100, 128, 5, True),      # [1] per-channel
    (63, 200, 48, 15, True),      # [1] the table switches inside a block; ragged features and tokens
    (64, 1100, 80, 16, False),    # [4] exactly one feature tile and one token tile
    (65, 640, 192, 17, True),     # [2] a second tile of one row in both directions; uneven 2 + 3 blocks
    (130, 2100, 128, 33, False),  # [8] three token tiles; most splits
    (200, 1600, 128, 64, True),   # [6] the cap, NT = 4
    (127, 130, 130, 48, False),   # [1] per-channel, P = 256
    (40, 2100, 48, 31, False),    # [8] ceil(P / bs) = 46 > B = 44: the padding scale clamp (NaN guards)
]
SHAPES_SPLITS = [1, 1, 1, 4, 2, 8, 6, 1, 8]
# Slices that wrap the ring, fp16 and bf16: NT, splits (all 16: the clamp, nkb / 2 is 32 or more), blocks per slice
LONG = [
    (40, 8192, 48, 2, False),       # NT 1, nb 4; the table switches inside a block
    (130, 10240, 192, 17, True),    # NT 2, nb 5; three feature tiles
    (65, 13824, 13824, 33, False),  # NT 3, nb 6 and 7 (108 blocks over 16 slices); per-channel
    (65, 14336, 128, 64, True),     # NT 4, nb 7: twice round the ring
]
# Many tiles, so the split is the workgroup target's (want < cap); one dtype and one compat mode each,
# because the integer reference of 10^4 features takes seconds on the host.  (..., compat16, dtype)
WIDE = [
    (16321, 1024, 128, 48, True, "bf16"),   # 256 tiles, splits 2 of cap 4, nb 4, NT 3; 6 MiB of partials
    (10881, 1536, 128, 20, False, "fp16"),  # 171 tiles, splits 3 of cap 6, nb 4, NT 2
    (32705, 896, 128, 64, False, "fp16"),   # 512 tiles, want 1: direct store after 7 blocks, NT 4
]

# ---- tests/test_gpu_ternary_skinny_group.py.  (m, bs, tokens, ns): the members' splits in brackets
# (PLAIN_SPLITS below, asserted by the CPU test)
PLAIN = [
    (100, 16, 2, (1, 40)),              # [1, 1] direct stores
    (640, 192, 17, (65, 1, 130, 64)),   # [2, ...] uneven 2 + 3 blocks; two token tiles; one- and three-tile members
    (2100, 48, 33, (40, 130)),          # [8, 8] the table switches inside a block; the padding-scale clamp
    (1600, 128, 64, (200, 63)),         # [6, 6] NT = 4
    (130, 130, 48, (127,)),             # [1] per-channel; a group of one
    (512, 128, 3, (32705, 65)),         # [1, 2] 512 tiles store directly beside a member that takes tickets
]
PLAIN_SPLITS = [[1, 1], [2, 2, 2, 2], [8, 8], [6, 6], [1], [1, 2]]
SWIGLU = [(100, 16, 2, 40), (640, 192, 17, 65), (2100, 128, 33, 130), (1600, 128, 64, 200)]
SWIGLU_SPLITS = [1, 2, 8, 6]
# (m, bs, tokens, ns, dtype).  Splits 2 (nb 4, 4) beside splits 4 (nb 2): grid.y = 4, so the first member's
# 256 tiles each see two workgroups of slices they do not have, and both members take tickets
PLAIN_LONG = [(1024, 128, 48, (16321, 65), "fp16")]
SWIGLU_LONG = [(10240, 192, 17, 65)]  # 16 + 16 tickets per tile, nb 5

# ---- tests/test_gpu_ternary_skinny_norm.py: the norm prologue's 512 threads on rows of m >= 8192
NORM_SHAPES = [PLAIN[0], PLAIN[1], PLAIN[2], PLAIN[4]]
NORM_SWIGLU = [(100, 16, 2, 40), (640, 192, 17, 65), (1600, 128, 64, 200)]
NORM_LONG = (10240, 192, 17, (130, 65))       # norm on a PLAIN group of two
NORM_RES_LONG = (14336, 128, 64, (65,))       # norm and residual, lone, NT 4, nb 7

CLASSES = (
    # a ticket-path slice (splits >= 2) that overwrites a ring slot: max nb >= 4, for every NT and type
    [f"wrap-NT{nt}-{dt}" for nt in (1, 2, 3, 4) for dt in ("fp16", "bf16")] + [
        "lap2-NT4",           # ticket path, max nb >= 7: the ring goes round twice, four token tiles
        "lap2-NT<4",          # ... and with another slot size
        "uneven-long",        # slices of unequal length, the shortest of 4 blocks or more
        "clamp16",            # splits == 16 < nkb / 2
        "want2",              # splits == want == 2 < cap, nb >= 4
        "want3+",             # splits == want >= 3, want < cap, nb >= 4
        "want-over-4MiB",     # one of the two above with more than 4 MiB of partial tiles
        "direct-long-NT4",    # want == 1: the direct store after nb >= 7 blocks, NT 4
        "group-mixed",        # a PLAIN group: two ticket-path members, other split counts and slice lengths, one nb >= 4
        "swiglu-wrap",        # a SWIGLU pair with nb >= 4 and 2 * splits tickets per tile
        "norm-m8192",         # the norm prologue on rows of m >= 8192
    ])


def runs_of(lone=(), wide=(), plain=(), plain_1dt=(), swiglu=(), norm=()):
    """The kernel runs of the given tables as (kind, dtype, norm, [plans], ticket target)."""
    out = []
    both = ("fp16", "bf16")
    for n, m, bs, tokens, _ in lone:
        out += [("lone", dt, False, [skinny_plan(tokens, n, m)], None) for dt in both]
    for n, m, bs, tokens, _, dt in wide:
        out.append(("lone", dt, False, [skinny_plan(tokens, n, m)], None))
    for m, bs, tokens, ns in plain:
        out += [("plain", dt, False, skinny_group_plan(tokens, m, ns, 0)["members"], None) for dt in both]
    for m, bs, tokens, ns, dt in plain_1dt:
        out.append(("plain", dt, False, skinny_group_plan(tokens, m, ns, 0)["members"], None))
    for m, bs, tokens, n in swiglu:
        g = skinny_group_plan(tokens, m, (n, n), 1)
        out += [("swiglu", dt, False, g["members"], g["ticket_target"]) for dt in both]
    for m, bs, tokens, ns in norm:
        out += [("plain", dt, True, skinny_group_plan(tokens, m, ns, 0)["members"], None) for dt in both]
    return out


def classes_of(runs):
    """The subset of CLASSES that `runs` (runs_of) reaches."""
    got = set()
    for kind, dt, norm, plans, target in runs:
        for p in plans:
            nb, s = p["nb"], p["splits"]
            if s >= 2 and max(nb) >= 4:
                got.add(f"wrap-NT{p['NT']}-{dt}")
            if s >= 2 and max(nb) >= 7:
                got.add("lap2-NT4" if p["NT"] == 4 else "lap2-NT<4")
            if s >= 2 and min(nb) >= 4 and min(nb) != max(nb):
                got.add("uneven-long")
            if s == 16 and p["nkb"] // 2 > 16:
                got.add("clamp16")
            if s >= 2 and s == p["want"] < p["cap"] and min(nb) >= 4:
                got.add("want2" if s == 2 else "want3+")
                if p["part_bytes"] > 4 * MIB:
                    got.add("want-over-4MiB")
            if s == 1 and p["want"] == 1 and nb[0] >= 7 and p["NT"] == 4 and kind != "swiglu":
                got.add("direct-long-NT4")
            if norm and p["m"] >= 8192:
                got.add("norm-m8192")
        tick = [p for p in plans if p["splits"] >= 2]
        if kind == "plain" and any(a["splits"] != b["splits"] and max(a["nb"]) != max(b["nb"]) and
                                   max(max(a["nb"]), max(b["nb"])) >= 4 for a in tick for b in tick):
            got.add("group-mixed")
        if kind == "swiglu" and min(min(p["nb"]) for p in plans) >= 4 and target == 2 * plans[0]["splits"] >= 4:
            got.add("swiglu-wrap")
    assert got <= set(CLASSES)
    return got
