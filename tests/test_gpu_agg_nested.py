"""hj3d_agg_nested on the GPU: COUNT / SUM / MIN / MAX over the rows stored nested tuples {a, ref_1 .. ref_k}
would unnest to, without unnesting them, and the plan hook star_plan_aggregate.

Expected values: tests/agg_nested_ref.py (numpy / Python integers; pinned by tests/test_agg_nested_ref.py)
over Table.export() and the host build relations, hj3d_unnestn on the same tuples (c_top, the row sums,
the emitted rows per a), and the reference binary's experiment-4 fixture. Integer work: every
comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import agg_nested_ref as AN
from test_gpu_expand_limits import cus, scattered
from test_gpu_group_agg import host64, relation, table_of
from test_gpu_select_nested import plan_relations
from test_gpu_unnest import NOREF, dev, host
from test_gpu_unnestn import parity  # noqa: F401  (the Zipf fixture: R, S, T, two tables of different bucket counts)

pytestmark = pytest.mark.gpu

# agg_nested.hip's constants (a change there must fail the size cases below, not empty them)
BLOCK, BATCH = 256, 2   # kBlock, kAggnBatch
TILE = BLOCK * BATCH    # tuples a workgroup takes per step
AGG_MAX = 8
CANARY = 0x5A5A5A5A5A5A5A5A
GUARD = 64


def grid_round(n_cus):  # tuples k_aggn covers before a workgroup takes its next tile
    return 8 * n_cus * TILE


def run(ctx, nested, tables, specs, cap=None):
    """(result, the rows written) with a canary tail behind the cap rows."""
    import torch
    n = nested.shape[0]
    cap = n if cap is None else cap
    buf = torch.full((cap + GUARD, len(specs)), CANARY, dtype=torch.int64, device="cuda")
    r = ctx.agg_nested(nested, tables, specs, out=buf[:cap])
    assert bool((buf[cap:] == CANARY).all())
    return r, host64(buf[:min(cap, n)])


def columns(tables, rels):
    """Per (table index, word, signed): (the library's column, the model's), each computed once."""
    import hj3d
    cols = {}

    def get(i, word, signed=True):
        if (i, word, signed) not in cols:
            d, h = rels[i]
            _, payload, sub = tables[i].export()
            dcol, _ = tables[i].group_agg(hj3d.Rel(d, key_word=1), word, signed)
            cols[(i, word, signed)] = (dcol, AN.group_agg(payload, sub, h, word, signed)["col"])
        return cols[(i, word, signed)]
    return get


def check(ctx, tuples, tables, specs_dev, specs_model, cap=None):
    """agg_nested of host tuples against the model: per-tuple rows, totals, counters, canary."""
    mains = [t.export()[1] for t in tables]
    want = AN.agg_nested(tuples, mains, specs_model)
    assert not want["unsupported"]
    r, rows = run(ctx, dev(tuples), tables, specs_dev, cap)
    n = len(tuples)
    assert (r["n_in"], r["n_live"], r["c_top"], r["total"]) == (n, want["n_live"], want["c_top"], want["total"])
    assert r["overflow"] is (cap is not None and cap < n)
    assert np.array_equal(rows, want["rows"][:len(rows)])
    return want, r


def both(get, ops):
    """(device specs, model specs) for [("count",) | (op, slot, table index, word[, signed])]."""
    sd, sm = [], []
    for sp in ops:
        if sp[0] == "count":
            sd.append(("count",))
            sm.append(("count",))
            continue
        op, slot, i, word = sp[:4]
        signed = sp[4] if len(sp) > 4 else True
        dcol, mcol = get(i, word, signed)
        sd.append((op, slot, dcol, signed))
        sm.append((op, slot, mcol, signed))
    return sd, sm


# ---- 1. chained tuples (Zipf 1.0, two tables): k = 2 from probe -> probe_refn, k = 1 from a MAINREF probe ----
@pytest.fixture(scope="module")
def chained(ctx, parity):  # noqa: F811
    import torch
    import hj3d
    p = parity
    trip = torch.zeros((4097, 3), dtype=torch.int32, device="cuda")
    rt = ctx.probe_refn(p["tt"], hj3d.Rel(p["R"], key_word=1), p["pairs"], out=trip)
    h = host(trip[:rt.n_out]).copy()
    h[::50, 1] = NOREF
    h[7::50, 2] = NOREF
    tables = [p["ts"], p["tt"]]
    rels = [(p["S"], host(p["S"])), (p["T"], host(p["T"]))]
    return {"h": h, "tables": tables, "get": columns(tables, rels), "pairs": host(p["pairs"])}


def test_chained_k2(ctx, chained):
    import torch
    c = chained
    ops = [("count",), ("sum", 1, 0, 0, False), ("sum", 2, 1, 0, False), ("min", 1, 0, 1), ("max", 2, 1, 1), ("min", 2, 1, 0, False)]
    sd, sm = both(c["get"], ops)
    want, r = check(ctx, c["h"], c["tables"], sd, sm)
    assert 0 < want["n_live"] < len(c["h"])  # dead tuples interleaved with live ones
    # the same tuples through the unnest: c_top, the row sums (word 0 is the row id), the rows per a
    x = dev(c["h"])
    un = ctx.unnestn(c["tables"], x)
    out = torch.zeros((un["c_top"], 3), dtype=torch.int32, device="cuda")
    un = ctx.unnestn(c["tables"], x, out=out)
    assert r["total"][0] == r["c_top"] == un["c_top"] and r["n_live"] == un["n_live"]
    assert r["total"][1:3] == un["sum_row"]
    a = c["h"][:, 0]
    assert len(np.unique(a)) == len(a)
    per_a = np.bincount(host(out)[:, 0], minlength=int(a.max()) + 1)
    assert np.array_equal(want["rows"][:, 0], per_a[a].astype(np.uint64))
    # totals only
    assert ctx.agg_nested(x, c["tables"], sd) == r
    assert ctx.agg_nested(x, c["tables"], sd, fetch=False) is None and ctx.agg_nested_result() == r


def test_mainref_dense_output_k1(ctx, chained):
    c = chained
    assert (c["pairs"][:, 1] == NOREF).any() and (c["pairs"][:, 1] != NOREF).any()
    sd, sm = both(c["get"], [("sum", 1, 0, 0, False), ("count",), ("max", 1, 0, 1, False)])
    want, r = check(ctx, c["pairs"], c["tables"][:1], sd, sm)
    un = ctx.unnestn(c["tables"][:1], dev(c["pairs"]))
    assert (r["total"][1], r["total"][0]) == (un["c_top"], un["sum_row"][0])


# ---- 2. k = 6 on one tiny table (a self join), every aggregate, nspec = 1 and HJ3D_AGG_MAX ----
@pytest.fixture(scope="module")
def tiny(ctx):
    rng = np.random.default_rng(23)
    h = relation(rng, scattered(rng, np.arange(40, dtype=np.uint32), 1 + np.arange(40) % 6))
    d = dev(h)
    t = table_of(ctx, d, 17)
    return {"t": t, "h": h, "d": d, "m": t.size()[1], "get": columns([t], [(d, h)])}


def random_refs(rng, n, k, m):
    """n tuples {distinct a, k refs}: mostly below m, some at m, m + 1 and 0xFFFFFFFF (dead)."""
    t = rng.integers(0, m + 2, (n, k + 1)).astype(np.uint32)
    t[:, 0] = rng.permutation(n) + 1000
    t[3::29, 1 + (k - 1) // 2] = NOREF
    return t


@pytest.mark.parametrize("signed", [True, False])
def test_wide_self_join(ctx, tiny, signed):
    x = tiny
    t6 = random_refs(np.random.default_rng(29), 700, 6, x["m"])
    ops = [("count",), ("sum", 1, 0, 2, signed), ("min", 2, 0, 2, signed), ("max", 3, 0, 2, signed), ("sum", 4, 0, 0, signed),
           ("min", 5, 0, 0, signed), ("max", 6, 0, 2, signed), ("sum", 6, 0, 2, signed)]
    assert len(ops) == AGG_MAX
    sd, sm = both(x["get"], ops)
    want, _ = check(ctx, t6, [x["t"]] * 6, sd, sm)
    assert 0 < want["n_live"] < len(t6)
    for one in range(AGG_MAX):  # nspec = 1, each aggregate alone
        w1, _ = check(ctx, t6[:100], [x["t"]] * 6, sd[one:one + 1], sm[one:one + 1])
        assert np.array_equal(w1["rows"][:, 0], want["rows"][:100, one])


# ---- 3. dead tuples, the empty input, tile sizes, capacity ----
def test_all_dead_and_empty(ctx, tiny):
    x = tiny
    sd, sm = both(x["get"], [("count",), ("sum", 1, 0, 2), ("min", 1, 0, 2), ("max", 2, 0, 2), ("min", 2, 0, 2, False),
                             ("max", 1, 0, 2, False)])
    dead = np.stack([np.arange(300), np.full(300, x["m"]), np.full(300, NOREF)], axis=1).astype(np.uint32)
    dead[::2, 1], dead[::2, 2] = 3, x["m"] + 5
    want, r = check(ctx, dead, [x["t"]] * 2, sd, sm)
    assert (r["n_live"], r["c_top"], r["total"]) == (0, 0, [0, 0, AN.I64_MAX, AN.I64_MIN, AN.M64, 0])
    assert want["rows"].tolist() == [[0, 0, AN.I64_MAX, AN.I64_MIN, AN.M64, 0]] * 300
    _, r0 = check(ctx, dead[:0], [x["t"]] * 2, sd, sm)
    assert (r0["n_in"], r0["total"]) == (0, r["total"])


@pytest.mark.parametrize("n", ["tile-1", "tile", "tile+1", "round+5"])
def test_tile_sizes(ctx, tiny, n):
    x = tiny
    n = {"tile-1": TILE - 1, "tile": TILE, "tile+1": TILE + 1, "round+5": grid_round(cus()) + 5}[n]
    t = random_refs(np.random.default_rng(n % 97), n, 2, x["m"])
    sd, sm = both(x["get"], [("count",), ("sum", 2, 0, 2)])
    want, _ = check(ctx, t, [x["t"]] * 2, sd, sm)
    assert 0 < want["n_live"] < n


@pytest.mark.parametrize("cap", [0, 1, TILE, TILE + 3, 2 * TILE + 76])
def test_capacity(ctx, tiny, cap):
    x = tiny
    n = 2 * TILE + 77
    t = random_refs(np.random.default_rng(31), n, 3, x["m"])
    sd, sm = both(x["get"], [("sum", 3, 0, 2), ("count",), ("min", 1, 0, 2)])
    check(ctx, t, [x["t"]] * 3, sd, sm, cap=cap)  # overflow, the first cap rows, the complete totals, the canary


# ---- 4. wrap-around and the magnitude rule ----
@pytest.fixture(scope="module")
def big(ctx):
    """One table with keys of 2^16, 2^15, 2048 and 3 rows; the word 0xFFFFFFFF in every tuple."""
    rng = np.random.default_rng(37)
    col = scattered(rng, np.array([7, 8, 9, 10], dtype=np.uint32), [1 << 16, 1 << 15, 3, 2048])
    h = np.ascontiguousarray(np.stack([np.arange(len(col), dtype=np.uint32), col, np.full(len(col), 0xFFFFFFFF, np.uint32)], axis=1))
    d = dev(h)
    t = table_of(ctx, d, 16)
    _, payload, _ = t.export()
    ref = {int(ln): m for m, ln in enumerate(payload[:, 3])}
    return {"t": t, "get": columns([t], [(d, h)]), "hot": ref[1 << 16], "mid": ref[1 << 15], "one": ref[3], "k2": ref[2048]}


def test_sum_wraps(ctx, big):
    b = big
    k2, one = b["k2"], b["one"]
    t = np.array([[1, k2, k2, k2, k2], [2, one, k2, one, k2], [3, one, one, one, one]], dtype=np.uint32)
    sd, sm = both(b["get"], [("sum", 1, 0, 2, False), ("count",), ("sum", 2, 0, 2, True), ("sum", 4, 0, 0, False)])
    want, r = check(ctx, t, [b["t"]] * 4, sd, sm)
    assert 2048 * 0xFFFFFFFF * 2048 ** 3 >= 1 << 64  # the first tuple's unsigned SUM wraps
    assert int(want["rows"][0, 0]) == (2048 * 0xFFFFFFFF * 2048 ** 3) & AN.M64
    assert int(want["rows"][0, 2]) == (-(2048 ** 4)) & AN.M64  # the word read as int32 is -1
    assert r["c_top"] == 2048 ** 4 + 9 * 2048 ** 2 + 81


def test_magnitude_rule(ctx, big):
    import hj3d
    b = big
    hot, mid, one = b["hot"], b["mid"], b["one"]
    sd, _ = both(b["get"], [("count",), ("sum", 1, 0, 2, False)])
    cases = {
        "one product of 2^63": [[1, one, one, one, one], [2, hot, hot, hot, mid], [3, one, one, one, one]],
        "one product of 2^64": [[1, one, one, one, one], [2, hot, hot, hot, hot]],
        "a total of 2^63": [[i, mid, mid, mid, mid] for i in range(8)],
        "a total of 2^64": [[i, mid, mid, mid, mid] for i in range(16)],
    }
    for what, rows in cases.items():
        t = np.array(rows, dtype=np.uint32)
        assert AN.agg_nested(t, [b["t"].export()[1]] * 4, [("count",)])["unsupported"], what
        with pytest.raises(hj3d.Hj3dError) as e:
            run(ctx, dev(t), [b["t"]] * 4, sd)
        assert e.value.status == hj3d.HJ3D_EUNSUPPORTED, what
        res = hj3d._AggNRes()
        assert hj3d.lib().hj3d_agg_nested_result(ctx.h, C.byref(res)) == hj3d.HJ3D_EUNSUPPORTED
        assert (res.n_in, res.n_live, res.c_top, list(res.total)) == (len(t), len(t), 0, [0] * AGG_MAX), what
    # just below: 7 products of 2^60, and the same context afterwards
    t = np.array([[i, mid, mid, mid, mid] for i in range(7)], dtype=np.uint32)
    r, _ = run(ctx, dev(t), [b["t"]] * 4, sd)
    assert (r["c_top"], r["total"][0], r["n_live"]) == (7 << 60, 7 << 60, 7)


# ---- 5. arguments ----
def test_result_slots_are_separate(ctx, chained):
    import hj3d
    c = chained
    x = dev(c["h"])
    sd, _ = both(c["get"], [("count",), ("sum", 1, 0, 0, False)])  # (group_agg reports through the probe slot)
    ctx.select_nested(x, [])
    pr = ctx.probe_result()
    un = ctx.unnestn(c["tables"], x)
    r = ctx.agg_nested(x, c["tables"], sd)
    assert ctx.probe_result() == pr and ctx.unnestn_result() == un and pr.n_probe == len(c["h"])
    assert ctx.agg_nested_result() == r


def test_refusals(ctx, chained):
    import torch
    import hj3d
    L = hj3d.lib()
    c = chained
    ts, tt = c["tables"]
    scol, _ = c["get"](0, 0, False)
    tcol, _ = c["get"](1, 0, False)
    nested = dev(c["h"][:64])
    out = torch.zeros((64, 3), dtype=torch.int64, device="cuda")
    E = hj3d.PROBE_EMIT
    tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, 64)
    tc.build(hj3d.Rel(dev(np.zeros((8, 2), np.uint32)), key_word=1))

    def arr(*hs):
        return (C.c_void_p * len(hs))(*hs)

    def specs(*sp):
        a = (hj3d._AggSpec * max(len(sp), 1))()
        for i, (op, slot, col, n) in enumerate(sp):
            a[i] = hj3d._AggSpec(op, slot, 0, 0, col, n)
        return a

    S, T = (hj3d.AGG_SUM, 1, scol.data_ptr(), scol.shape[0]), (hj3d.AGG_MIN, 2, tcol.data_ptr(), tcol.shape[0])
    CNT = (hj3d.AGG_COUNT, 0, None, 0)
    good = specs(S, CNT, T)

    def st(ctxh=ctx.h, ptr=nested.data_ptr(), n=64, k=2, tables=arr(ts.h, tt.h), sp=good, nspec=3, flags=E,
           optr=out.data_ptr(), cap=64):
        return L.hj3d_agg_nested(ctxh, ptr, n, k, tables, sp, nspec, flags, optr, cap)

    bad = hj3d.HJ3D_EINVAL
    fresh = hj3d.Context(0)
    assert L.hj3d_agg_nested_result(fresh.h, C.byref(hj3d._AggNRes())) == bad  # before any hj3d_agg_nested
    fresh.close()
    assert st() == hj3d.HJ3D_OK
    for f in (hj3d.PROBE_UNIQUE, hj3d.PROBE_UNNEST, hj3d.PROBE_CHECKSUM, hj3d.PROBE_ACCUMULATE, hj3d.PROBE_MAINREF, 0x40):
        assert st(flags=E | f) == bad
    assert st(ctxh=None) == bad and st(tables=None) == bad
    assert st(tables=arr(ts.h, None)) == bad and st(tables=arr(None, tt.h)) == bad
    assert st(tables=arr(ts.h, tc.h)) == bad
    assert st(k=0) == bad and st(k=7, tables=arr(*([ts.h] * 7))) == bad
    assert st(nspec=0) == bad and st(sp=specs(*([CNT] * 9)), nspec=9) == bad and st(sp=None) == bad
    assert st(sp=specs(*([CNT] * 8)), nspec=8, optr=None, cap=0) == hj3d.HJ3D_OK
    assert st(sp=specs((4, 1, scol.data_ptr(), scol.shape[0])), nspec=1) == bad                  # unknown op
    assert st(sp=specs((hj3d.AGG_SUM, 0, scol.data_ptr(), scol.shape[0])), nspec=1) == bad      # slot outside 1..k
    assert st(sp=specs((hj3d.AGG_SUM, 3, scol.data_ptr(), scol.shape[0])), nspec=1) == bad
    assert st(sp=specs((hj3d.AGG_COUNT, 1, None, 0)), nspec=1) == bad                            # COUNT: slot 0
    assert st(sp=specs((hj3d.AGG_MAX_, 1, None, scol.shape[0])), nspec=1) == bad                 # no column
    assert st(sp=specs((hj3d.AGG_SUM, 1, scol.data_ptr() + 4, scol.shape[0] - 1)), nspec=1) == bad  # misaligned column
    assert st(sp=specs((hj3d.AGG_SUM, 1, scol.data_ptr(), scol.shape[0] - 1)), nspec=1) == bad   # gcol_n too small
    assert st(sp=specs((hj3d.AGG_SUM, 2, scol.data_ptr(), tcol.shape[0] - 1)), nspec=1) == bad
    assert st(ptr=None) == bad and st(ptr=nested.data_ptr() + 2) == bad
    assert st(optr=out.data_ptr() + 4) == bad and st(flags=0, optr=out.data_ptr() + 4, cap=0) == bad
    assert st(optr=None) == bad and st(optr=None, cap=0) == hj3d.HJ3D_OK
    assert st(n=1 << 32) == bad
    assert st(ptr=None, n=0) == hj3d.HJ3D_OK
    r = ctx.agg_nested_result()
    assert (r["n_in"], r["n_live"], r["c_top"], r["overflow"]) == (0, 0, 0, False)
    with pytest.raises(ValueError):
        ctx.agg_nested(nested, [ts, tt], [])
    with pytest.raises(ValueError):
        ctx.agg_nested(nested, [ts, tt], [("avg", 1, scol)])
    with pytest.raises(ValueError):
        ctx.agg_nested(nested, [ts, tt], [("count",)], out=torch.zeros((64, 2), dtype=torch.int64, device="cuda"))
    tc.close()


# ---- 6. the plan hook ----
def test_plan_with_aggregates(ctx):
    import hj3d
    g, R, S, T = plan_relations()
    ref = g["plans"]["Ndu"]
    builds = [(dev(S), 1), (dev(T), 1)]
    plain = hj3d.star_plan_chained(ctx, dev(R), builds, g["nb"], keys=(0, 0))
    agg = [("count",), ("sum", 0, 0, False), ("sum", 1, 0, False), ("max", 1, 0, False), ("min", 0, 1)]
    got = hj3d.star_plan_aggregate(ctx, dev(R), builds, g["nb"], keys=(0, 0), aggregate=agg)
    assert got["c_top"] == plain["c_top"] == ref["c_top"] and not got["overflow"]
    assert got["total"][:3] == [plain["c_top"], plain["sum_row"][0], plain["sum_row"][1]]  # word 0 is the row id
    assert got["total"][1:3] == [ref["out"]["sum_b"], ref["out"]["sum_c"]]
    assert (got["n_in"], got["n_live"], got["c_probe"], got["c_probe_cmp"]) == \
        (plain["n_in"], plain["n_live"], plain["c_probe"], plain["c_probe_cmp"])
    # MAX(T.k) = the largest T row with a partner in R and S, MIN(S.a) the smallest joining key: from the keys alone
    in_both = np.intersect1d(np.intersect1d(R[:, 0], S[:, 1]), T[:, 1])
    assert got["total"][3] == int(np.nonzero(np.isin(T[:, 1], in_both))[0].max()) and got["total"][4] == int(in_both.min())
