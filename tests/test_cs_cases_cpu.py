"""CPU guards of the camshift path tests (tests/test_gpu_camshift_paths.py): the inputs of tests/cs_cases.py, run through the oracle alone,
really reach the kernel states they are named after, and the reference itself is unambiguous on every one of them — so the GPU tests may
demand the oracle's integers on every call, with no tie class and no +-1 px."""
import numpy as np

import cs_cases as cc


def _calls(seq):
    return [(b, a, cc.ends_inside(seq.w, seq.h, b, a), to) for (b, a, to) in seq.oracle_calls()]


def test_no_new_sequence_loses_its_object():
    """no case here is named for a degenerate object: every call of every new sequence returns width > 0 and height > 0, and a
    non-empty next search window"""
    n = 0
    for seq in cc.all_track_sequences():
        for k, (_b, sw, to) in enumerate(seq.oracle_calls()):
            assert to["width"] > 0 and to["height"] > 0 and sw[2] > 0 and sw[3] > 0, (seq.name, k, to, sw)
            n += 1
    assert n >= 500


def test_every_new_sequence_is_insensitive_to_the_summation_order():
    """the oracle built with the three order variants of tools/cpu_cs_order_check.py returns the reference's track object and search
    window on every call of every new sequence: zero order-sensitive calls"""
    seqs = cc.all_track_sequences()
    ref = [s.oracle_calls() for s in seqs]
    for flag in cc.ORDER_VARIANTS:
        with cc.oracle_variant(flag):
            alt = [s.oracle_calls() for s in seqs]
        bad = [(s.name, k, flag) for s, ra, rb in zip(seqs, ref, alt) for k, (a, b) in enumerate(zip(ra, rb)) if not cc.same_call(a, b)]
        assert not bad, bad
    assert ref == [s.oracle_calls() for s in seqs]  # the real oracle is bound again


def test_jumping_sequences_leave_the_cached_region_and_also_stay():
    for seq in cc.jumping():
        calls = _calls(seq)
        inside = [c[2] for c in calls]
        assert None not in inside, (seq.name, inside)  # a region is cached in every call
        assert inside.count(False) >= 1 and inside.count(True) >= 1, (seq.name, inside)
        if "leaves" in seq.tags:
            assert 2 * inside.count(False) >= len(inside), (seq.name, inside)
        # the jumps stay below the window size, and the reference follows the blob instead of staying put
        for (b, a, _i, _to), g0, g1 in zip(calls, seq.gens, seq.gens[1:]):
            assert abs(g1[0] - g0[0]) < max(b[2], b[3]) and abs(g1[1] - g0[1]) < max(b[2], b[3])
            if "leaves" in seq.tags:
                assert abs(a[0] + b[2] // 2 - g1[0]) <= 12 and abs(a[1] + b[3] // 2 - g1[1]) <= 12, (seq.name, a, g1[:2])
    for seq in cc.static():
        assert [c[2] for c in _calls(seq)] == [True] * seq.ncalls


def test_edge_sequences_clamp_the_margin_on_the_intended_sides():
    seen = set()
    for seq in cc.edges():
        sides = set()
        for (b, _a, _to) in seq.oracle_calls():
            R = cc.region_rect(seq.w, seq.h, b)
            assert R is not None
            x0, y0, x1, y1 = cc.clamped_window(seq.w, seq.h, b)
            if any(R["clamped"].values()):
                assert (R["rw"], R["rh"]) != (x1 - x0 + 2 * R["mg"], y1 - y0 + 2 * R["mg"])
            sides |= {k for k, v in R["clamped"].items() if v}
        assert set(seq.tags) <= sides, (seq.name, sides)
        seen |= sides
    assert seen == {"left", "top", "right", "bottom"}
    names = {s.name: s for s in cc.edges()}
    # negative search-window origins and right / bottom overhang in the very first call (the init rect reaches outside the frame)
    assert names["corner-top-left"].rect[0] < 0 and names["corner-top-left"].rect[1] < 0
    r = names["corner-bottom-right"].rect
    assert r[0] + r[2] > 320 and r[1] + r[3] > 240
    first = _calls(names["interior-to-right-border"])[0]
    assert first[2] is False  # the jump towards the border leaves the region cached in the interior


def test_column_phase_cases_cover_all_sixteen_pairs():
    """(left edge mod 4, width mod 4) of the region of the FIRST call of each case: all sixteen, on a frame the fused kernel fills its
    cache from during the histogram pass (W % 4 == 0, W / 4 <= 512)"""
    pairs = set()
    for seq in cc.column_phases():
        assert seq.w % 4 == 0 and seq.w // 4 <= 512
        b = seq.oracle_calls()[0][0]
        assert tuple(b) == seq.rect
        R = cc.region_rect(seq.w, seq.h, b)
        assert R["mg"] == 16 and not any(R["clamped"].values())
        assert (R["x0"] % 4, R["rw"] % 4) == seq.tags
        pairs.add(seq.tags)
    assert pairs == {(i, j) for i in range(4) for j in range(4)}


def test_frame_width_cases_take_the_intended_cache_fill():
    """rows2d of k_cs_track_fused: W % 4 == 0 and W / 4 <= threads"""
    def rows2d(w, nt):
        return w % 4 == 0 and w // 4 <= nt
    got = {s.w: (rows2d(s.w, 1024), rows2d(s.w, 512)) for s in cc.frame_widths() + cc.column_phases()[:1]}
    assert got == {320: (True, True), 321: (False, False), 641: (False, False), 2052: (True, False), 4100: (False, False)}
    for seq in cc.frame_widths():
        for (b, a, inside, _to) in _calls(seq):
            assert inside is True, (seq.name, b, a)  # small moves: every pass of these calls reads the cache


def test_capacity_cases_fall_between_and_above_the_two_capacities():
    for seq in cc.capacities():
        for (b, a, _to) in seq.oracle_calls():
            A = cc.clamped_area(seq.w, seq.h, b)
            small, large = cc.region_rect(seq.w, seq.h, b, cc.REGION_CAP_SMALL), cc.region_rect(seq.w, seq.h, b, cc.REGION_CAP)
            if "between" in seq.tags:
                assert cc.REGION_CAP_SMALL < A <= cc.REGION_CAP and small is None and large is not None, (seq.name, b, A)
            else:
                assert A > cc.REGION_CAP and small is None and large is None, (seq.name, b, A)
            assert tuple(a[:2]) != tuple(b[:2])  # a moving target


def test_region_sweep_values_sit_on_the_capacity_and_margin_boundaries():
    for seq in cc.jumping() + cc.static():
        W, H, sw = seq.w, seq.h, list(seq.rect)
        vals = cc.region_sweep_values(W, H, sw)
        A = cc.clamped_area(W, H, sw)
        assert vals[:4] == [0, A - 1, A, A + 1] and vals[-2:] == [22528, 40960] and len(set(vals)) == len(vals)
        assert cc.region_rect(W, H, sw, 0) is None and cc.region_rect(W, H, sw, A - 1) is None
        assert cc.region_rect(W, H, sw, A)["mg"] == 0 and cc.region_rect(W, H, sw, A + 1)["mg"] == 0
        for m, v in zip((1, 3, 8, 15, 16), vals[4:9]):
            assert cc.region_rect(W, H, sw, v)["mg"] == m and cc.region_rect(W, H, sw, v - 1)["mg"] == m - 1, (seq.name, m, v)


def test_init_batches_reach_both_kernels_and_every_edge():
    """ht_camshift_init_batch dispatches the row-split kernel for n < 64 with G >= 2, G <= (tallest rect + 15) / 16"""
    kinds = {}
    for name, kernel, rects in cc.init_batches():
        n, tall = len(rects), max(r[3] for r in rects)
        assert ("rows" if n < 64 and (tall + 15) // 16 >= 2 else "wg") == kernel, name
        assert all(r[2] > 0 and r[3] > 0 for r in rects)  # zero- and negative-sized rects are the browser's business
        kinds.setdefault(kernel, set()).add(n)
    assert {64, 3, 1} <= kinds["wg"] and {1, 5, 40} <= kinds["rows"]
    batches = {name: rects for name, _k, rects in cc.init_batches()}
    # the one-workgroup kernel sees every width and height of the grid, too
    assert {(r[2], r[3]) for r in batches["n64-varied"]} >= {(w, h) for w in cc.INIT_WIDTHS for h in cc.INIT_HEIGHTS}
    tall = [r[3] for r in batches["n5-one-tall"]]
    assert max(tall) == 257 and sorted(tall)[-2] <= 16  # most row workgroups of the short streams get no rows
    W, H = cc.INIT_W, cc.INIT_H
    border = cc.init_border_rects()
    assert any(x < 0 < x + w for x, y, w, h in border) and any(x < W < x + w for x, y, w, h in border)
    assert any(y < 0 < y + h for x, y, w, h in border) and any(y < H < y + h for x, y, w, h in border)
    outside = [r for r in border if r[0] >= W or r[1] >= H or r[0] + r[2] <= 0 or r[1] + r[3] <= 0]
    assert len(outside) >= 2
    for r in outside:
        m = cc.model_histogram(cc.init_frame(0), r)
        assert m[0] == r[2] * r[3] and m.sum() == m[0]  # transparent black: everything in bin 0
    for x, y, w, h in cc.init_grid_rects():
        assert 0 <= x and x + w <= W and 0 <= y and y + h <= H


def test_hist_frames_are_what_their_families_promise():
    for w, h in cc.HIST_SIZES:
        for slot in range(3):
            px = {f: cc.hist_frame(f, w, h, slot).reshape(-1, 4) for f in cc.HIST_FAMILIES}
            bins = {f: (256 * (p[:, 0].astype(int) >> 4) + 16 * (p[:, 1].astype(int) >> 4) + (p[:, 2].astype(int) >> 4)) for f, p in px.items()}
            nq = w * h // 4
            quads = {f: b[: 4 * nq].reshape(nq, 4) for f, b in bins.items()}
            flat = {f: (q == q[:, :1]).all(axis=1) for f, q in quads.items()}
            assert flat["flat"].all() and flat["noise"].mean() < 0.01
            assert 0 < flat["blocks"].sum() < nq  # runs of 5 hold a whole group now and then, and groups straddle run boundaries
            assert all(int(cc.frame_histogram(p.reshape(h, w, 4)).sum()) == w * h for p in px.values())
            if slot:
                assert not np.array_equal(px["flat"], cc.hist_frame("flat", w, h, slot - 1).reshape(-1, 4))
    assert sorted(w * h for w, h in cc.HIST_SIZES) == [4095, 4096, 4097, 16384, 16385, 32768, 32769]
