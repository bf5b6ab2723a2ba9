"""The tile-plan case table (tests/plan_cases.py) held to its rules: the planner port still restates the source, every plan a
planner can choose within the enumerated domain has a case, and that case is the smallest format of its plan.  No GPU."""
import os

import plan_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planners_still_stand_in_the_source():
    texts = {}
    for path, text in pc.ANCHORS:
        if path not in texts:
            with open(os.path.join(ROOT, path)) as f:
                texts[path] = f.read()
        assert text in texts[path], "%s no longer reads %r: restate the planner in tests/plan_cases.py" % (path, text)


def test_plan_stride_port_equals_the_loops_as_written():
    """The port counts banks with numpy and keeps only the stride modulo the lanes; the source's loops, literally, on a sample."""
    def literal(R, length, lanes):
        best, best_cost = length, -1
        for c in range(lanes):
            stride, cost = length + c, 0
            for s0 in range(0, R * lanes, lanes):
                banks = [0] * 32
                for lane in range(lanes):
                    s = s0 + lane
                    banks[((s % R) * stride + s // R) & (lanes - 1)] += 1
                worst = max(banks[:lanes])
                cost += worst - 2 if worst > 2 else 0
            if best_cost < 0 or cost < best_cost:
                best_cost, best = cost, stride
        return best

    for R, length, lanes in ((1, 1025, 16), (3, 1027, 16), (4, 1033, 16), (5, 519, 16), (10, 260, 16), (20, 258, 16), (63, 129, 16), (127, 33, 16),
                             (7, 300, 32), (16, 77, 32)):
        assert pc.plan_stride(R, length, lanes) == literal(R, length, lanes), (R, length, lanes)


def held(cases, more, plans, tile_of):
    """Every plan has a case, the first case of a plan is its smallest format, and the further cases add no plan of their own."""
    by_plan = {}
    for f in cases:
        by_plan.setdefault(tile_of(*f).plan, []).append(f)
    assert set(by_plan) == set(plans), (set(plans) - set(by_plan), set(by_plan) - set(plans))
    for plan, fs in by_plan.items():
        assert fs == [plans[plan]], (plan, fs, plans[plan])
    assert len(set(cases)) == len(cases) == len(plans)
    for f in more:
        assert tile_of(*f).plan in plans and f not in cases, f


def test_symsync_table_reaches_every_plan():
    plans = pc.symsync_plans()
    assert len(pc.symsync_domain()) == pc.SS_MAX_SPS * pc.SS_MAX_ROW and pc.SS_ROWS == tuple(range(1, pc.SS_MAX_ROW + 1))
    held(pc.SYMSYNC_CASES, pc.SYMSYNC_MORE, plans, pc.symsync_tile)
    # fifteen plans: every tile of the 40 KiB and 64 KiB tiers at the padded stride and at the unpadded one, and the widest symbols'
    P = pc.SsPlan
    assert set(plans) == {P("40K", TO, 256, U, padded) for TO, U in ((1024, 4), (512, 2), (256, 1)) for padded in (True, False)} | \
        {P("64K", TO, pc.tile_workgroup(TO), 1, padded) for TO in (256, 128, 64, 32) for padded in (True, False)} | {P("96K", 32, 64, 1, True)}
    # the further cases: 33 taps per phase on the six plans no test ran, at S that do not divide the workgroup
    want = [P("40K", 512, 256, 2, True), P("40K", 256, 256, 1, True), P("64K", 256, 256, 1, True), P("64K", 128, 128, 1, True),
            P("64K", 64, 64, 1, True), P("64K", 32, 64, 1, True)]
    assert [pc.symsync_tile(*f).plan for f in pc.SYMSYNC_MORE] == want
    for L, S, N in pc.SYMSYNC_MORE:
        t = pc.symsync_tile(L, S, N)
        assert t.NB == 9 and t.plan.WG % S != 0
    assert sum(S > 64 and pc.symsync_tile(L, S, N).plan.WG // S == 0 for L, S, N in pc.SYMSYNC_CASES + pc.SYMSYNC_MORE) >= 3     # de = 0
    # the planner's own claim: a tile always fits, and within the LDS a workgroup may ask for
    for f in pc.symsync_domain():
        assert pc.symsync_tile(*f).lds <= pc.SS_LDS_WIDE


def test_symsync_streams_hold_the_timing_offsets():
    for L, S, N in pc.SYMSYNC_CASES + pc.SYMSYNC_MORE:
        mus = pc.symsync_mus(L, S)
        assert all(0 <= mu < S * L for mu in mus) and {0, S * L - 1} <= set(mus)
        assert S < 2 or L + 3 in mus                                         # q = 1
        assert S < 4 or any(1 < mu // L < S - 1 for mu in mus)


def test_resample_table_reaches_every_plan_of_the_sample():
    plans = pc.resample_plans()
    held(pc.RESAMPLE_CASES, pc.RESAMPLE_MORE, plans, pc.resample_tile)
    P = pc.RsPlan
    # Complex<f32>: every tile beside the table in both tiers, down to the planner's smallest of 16 outputs, and every tile with the
    # table in global memory but that one
    c32 = {p for p in plans if p.dtype == "c32"}
    assert {(p.tier, p.TO) for p in c32 if p.tab_lds} == {("40K", 1024), ("40K", 512), ("40K", 256), ("64K", 1024), ("64K", 512), ("64K", 256),
                                                           ("64K", 128), ("64K", 64), ("64K", 32), ("64K", 16)}
    assert pc.resample_tile(1, 1, 5440, "c32").plan == P("c32", "64K", 16, 64, True)      # the window where LDS runs out
    assert {(p.tier, p.TO) for p in c32 if not p.tab_lds} == {("64K", TO) for TO in (1024, 512, 256, 128, 64, 32)}
    # f32: the table always fits, beside 64 samples or more
    assert all(p.tab_lds for p in plans if p.dtype == "f32")
    assert {(p.tier, p.TO) for p in plans if p.dtype == "f32"} == {("40K", 1024), ("40K", 512), ("40K", 256), ("64K", 1024), ("64K", 512),
                                                                   ("64K", 256), ("64K", 128), ("64K", 64)}
    assert all(p.WG == pc.tile_workgroup(p.TO) for p in plans)
    # the issue's examples of the tile nothing ran, one trip per lane
    assert pc.resample_tile(1, 10, 16, "c32").plan == P("c32", "40K", 256, 256, True)
    assert pc.resample_tile(1, 20, 16, "c32").plan == P("c32", "64K", 256, 256, True)
    for L, M, N, dt in pc.RESAMPLE_CASES + pc.RESAMPLE_MORE:
        assert pc.resample_in_range(L, M, N)


def test_channelizer_table_reaches_every_plan():
    plans = pc.channelizer_plans()
    held(pc.CHANNELIZER_CASES, pc.CHANNELIZER_MORE, plans, pc.channelizer_tile)
    assert {p.M for p in plans} == {1 << k for k in range(1, 11)}
    assert len(pc.channelizer_domain()) == sum(4 * (1 << lg) * 16 for lg in range(1, 11))
    P = pc.ChzPlan
    for M in sorted({p.M for p in plans}):
        mine = {p.halvings for p in plans if p.M == M and p.staged}
        # a full and a halved tile for every M, quartered ones at 256 and 512
        assert mine == ({0, 1, 2} if M in (256, 512) else {0, 1}), (M, mine)
    # samples in global memory and taps in global memory: the two largest M alone -- 512 with its halved and quartered tiles, 1024
    # with its two frames and its one
    assert {p for p in plans if not p.staged} == {P(512, 4, 0, False, False), P(1024, 2, 0, False, False)}
    assert {p for p in plans if p.staged and not p.tab_lds} == {P(512, 4, 0, True, False), P(512, 2, 1, True, False), P(512, 1, 2, True, False),
                                                                P(1024, 2, 0, True, False), P(1024, 1, 1, True, False)}
    assert len(plans) == 29
    for f in pc.CHANNELIZER_MORE:
        t = pc.channelizer_tile(*f)
        assert t.plan.halvings == 1 and t.plan.staged
    assert any(N % M for M, D, N in pc.CHANNELIZER_MORE) and any(D == 4 * M for M, D, N in pc.CHANNELIZER_MORE)
    # tests/test_gpu_channelizer.py::test_planner_boundaries_at_512_channels does reach halved and quartered tiles, at D = 512
    got = {Q: pc.channelizer_tile(512, 512, Q * 512).plan for Q in (8, 9, 14, 15, 16)}
    assert (got[8].halvings, got[9].halvings, got[14].halvings) == (1, 1, 2) and not got[15].staged and not got[16].staged


def test_streams_are_small():
    """The longest call of a case, 3 tiles + 5 outputs: a few MiB of input and output at the most."""
    for L, S, N in pc.SYMSYNC_CASES + pc.SYMSYNC_MORE:
        k = pc.call_outputs(pc.symsync_tile(L, S, N).plan.TO)[-1]
        assert 8 * k * (S + 1) <= 4 << 20
    for L, M, N, dt in pc.RESAMPLE_CASES + pc.RESAMPLE_MORE:
        k = pc.call_outputs(pc.resample_tile(L, M, N, dt).plan.TO)[-1]
        n = pc.resample_len(k, L, M)
        assert pc.ELEM[dt] * n * (1 + L) <= 4 << 20                       # the (L, 1) twin of the bit-for-bit test writes n L outputs
    for M, D, N in pc.CHANNELIZER_CASES + pc.CHANNELIZER_MORE:
        k = pc.call_outputs(pc.channelizer_tile(M, D, N).plan.F)[-1]
        assert 8 * k * (D + M) <= 4 << 20
