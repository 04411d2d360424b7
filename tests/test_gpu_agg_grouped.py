"""hj3d_agg_grouped on the GPU: hj3d_agg_nested's aggregates reduced per build key (join + GROUP BY a build
key), its three kernel forms, and the plan hook star_plan_grouped.

Expected values: tests/agg_grouped_ref.py (numpy / Python integers; pinned by tests/test_agg_grouped_ref.py)
over Table.export() and the host relations, hj3d_agg_nested and hj3d_unnestn on the same tuples, and the
reference binary's experiment-4 fixture. Integer work: every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import agg_grouped_ref as AG
import agg_nested_ref as AN
from test_gpu_agg_nested import chained, columns, random_refs  # noqa: F401  (chained: the Zipf tuples, dead refs interleaved)
from test_gpu_expand_limits import cus, scattered
from test_gpu_group_agg import EDGE, host64, relation, table_of
from test_gpu_select_nested import plan_relations
from test_gpu_unnest import NOREF, dev, host
from test_gpu_unnestn import parity  # noqa: F401  (the fixture `chained` is made from)

pytestmark = pytest.mark.gpu

# agg_grouped.hip's constants (a change there must fail the size cases below, not empty them)
BLOCK, BATCH = 256, 2   # kBlock, kGbyBatch
TILE = BLOCK * BATCH    # tuples a workgroup takes per step
LDS_WORDS = 4096        # kGbyLdsWords: u64 fields of the column form 2 holds in LDS
CACHE_WORDS = 4096      # kGbyCacheWords: accumulators of form 3's cache
AGG_MAX = 8
CANARY = 0x5A5A5A5A5A5A5A5A
GUARD = 64
FORMS = (1, 2, 3, 0)    # direct, LDS column, LDS cache, automatic


def grid_round(n_cus):  # tuples the widest grid (form 1's; forms 2 / 3 run fewer workgroups) covers per step
    return 8 * n_cus * TILE


def cache_slots(nspec):  # form 3: the largest power of two with slots * nspec <= kGbyCacheWords
    s = CACHE_WORDS
    while s * nspec > CACHE_WORDS:
        s //= 2
    return s


def run(ctx, nested, tables, by, specs, base=None, cap=None, accumulate=False, into=None, form=0, shift=0):
    """(result, the column as uint64 words) with a canary tail behind the cap rows. into: what the column holds
    before the call; shift: rows the column starts behind a 16-byte boundary."""
    import torch
    m = tables[by - 1].size()[1]
    cap = m if cap is None else cap
    buf = torch.full((shift + cap + GUARD, len(specs)), CANARY, dtype=torch.int64, device="cuda")
    if into is not None:
        buf[shift:shift + m] = torch.from_numpy(np.ascontiguousarray(into).view(np.int64)).cuda()
    ctx.gby_form(form)
    try:
        col, r = ctx.agg_grouped(nested, tables, by, specs, base=base, out=buf[shift:shift + cap], accumulate=accumulate)
    finally:
        ctx.gby_form(0)
    assert bool((buf[shift + cap:] == CANARY).all()) and bool((buf[:shift] == CANARY).all())
    assert col.shape == (m, len(specs))
    return r, host64(col)


def both(get, ops):
    """(device specs, model specs) for [("count",) | (op, slot, table index, word[, signed]) | (op, "base", word[, signed])]."""
    sd, sm = [], []
    for sp in ops:
        if sp[0] == "count" or sp[1] == "base":
            sd.append(sp)
            sm.append(sp)
            continue
        op, slot, i, word = sp[:4]
        signed = sp[4] if len(sp) > 4 else True
        dcol, mcol = get(i, word, signed)
        sd.append((op, slot, dcol, signed))
        sm.append((op, slot, mcol, signed))
    return sd, sm


def check(ctx, tuples, tables, by, sd, sm, base=None, forms=(0,), into=None, accumulate=False, shift=0):
    """agg_grouped of host tuples against the model, for every form: the column, the totals, the counters.
    base: (Rel, host array). Returns (the model's dict, the last result)."""
    mains = [t.export()[1] for t in tables]
    want = AG.agg_grouped(tuples, mains, by, sm, base=None if base is None else base[1], into=into)
    assert not want["unsupported"]
    x = dev(tuples)
    r = None
    for form in forms:
        r, col = run(ctx, x, tables, by, sd, base=None if base is None else base[0], into=into, accumulate=accumulate,
                     form=form, shift=shift)
        assert (r["n_in"], r["n_live"], r["c_top"], r["total"]) == \
            (len(tuples), want["n_live"], want["c_top"], want["total"]), form
        assert np.array_equal(col, want["col"]), form
    return want, r


def reduce_column(col, sm):
    """The reduce of every column over all groups, in the spec's order."""
    out = []
    for s, sp in enumerate(sm):
        if sp[0] in ("count", "sum"):
            out.append(AN._sum64(col[:, s]))
        else:
            vals = [AN._ordered(int(v), AG.signed_of(sp)) for v in col[:, s]]
            out.append(((min(vals) if sp[0] == "min" else max(vals)) & AN.M64) if vals else AG.identity(sp))
    return out


def row_groups(table):
    """build row -> main ref, from the exported table."""
    _, payload, sub = table.export()
    g = np.full(int(sub.max()) + 1, -1, dtype=np.int64)
    for m, (_, _, off, ln) in enumerate(payload):
        g[sub[off:off + ln]] = m
    return g


# ---- 1. chained tuples (Zipf 1.0, two tables): k = 2 from probe -> probe_refn, k = 1 from a MAINREF probe ----
@pytest.fixture(scope="module")
def rbase(parity):  # noqa: F811
    """A base relation for the chained tuples' a (rows of R): EDGE words; shorter than R, so some a lie outside."""
    import hj3d
    rng = np.random.default_rng(83)
    h = np.ascontiguousarray(np.stack([EDGE[rng.integers(0, len(EDGE), 4000)], np.arange(4000, dtype=np.uint32)], axis=1))
    d = dev(h)
    return hj3d.Rel(d, key_word=1), h


@pytest.mark.parametrize("by", [1, 2])
def test_chained_k2(ctx, chained, rbase, by):  # noqa: F811
    import torch
    c = chained
    ops = [("count",), ("sum", 1, 0, 0, False), ("min", 2, 1, 1), ("max", 1, 0, 1, False), ("sum", "base", 0, True),
           ("min", "base", 0, False), ("max", "base", 0, True), ("sum", 2, 1, 0, True)]
    assert len(ops) == AGG_MAX
    sd, sm = both(c["get"], ops)
    want, r = check(ctx, c["h"], c["tables"], by, sd, sm, base=rbase, forms=FORMS)
    assert 0 < want["n_live"] < len(c["h"]) and (c["h"][:, 0] >= 4000).any()
    assert r["total"] == reduce_column(want["col"], sm)
    for one in range(AGG_MAX):  # nspec = 1, each aggregate alone
        w1, _ = check(ctx, c["h"], c["tables"], by, sd[one:one + 1], sm[one:one + 1], base=rbase)
        if ops[one][0] != "count" and ops[one][1] == "base":  # (alone, COUNT or a spec on a column leaves a opaque: more live tuples)
            assert np.array_equal(w1["col"][:, 0], want["col"][:, one])
    # without a base word: the totals are agg_nested's, the COUNT column the emitted rows per group of their by-row
    x = dev(c["h"])
    sd4, sm4 = sd[:4], sm[:4]
    w4, r4 = check(ctx, c["h"], c["tables"], by, sd4, sm4, forms=FORMS)
    an = ctx.agg_nested(x, c["tables"], sd4)
    assert (r4["n_in"], r4["n_live"], r4["c_top"], r4["total"]) == (an["n_in"], an["n_live"], an["c_top"], an["total"])
    assert r4["total"] == reduce_column(w4["col"], sm4)
    out = torch.zeros((an["c_top"], 3), dtype=torch.int32, device="cuda")
    un = ctx.unnestn(c["tables"], x, out=out)
    assert un["c_top"] == an["c_top"] and not un["overflow"]
    g = row_groups(c["tables"][by - 1])
    per_group = np.bincount(g[host(out)[:, by]], minlength=len(w4["col"]))
    assert np.array_equal(w4["col"][:, 0], per_group.astype(np.uint64))


def test_mainref_dense_output_k1(ctx, chained, rbase):  # noqa: F811
    c = chained
    assert (c["pairs"][:, 1] == NOREF).any() and (c["pairs"][:, 1] != NOREF).any()
    sd, sm = both(c["get"], [("sum", 1, 0, 0, False), ("count",), ("max", 1, 0, 1, False), ("min", "base", 0, True)])
    want, r = check(ctx, c["pairs"], c["tables"][:1], 1, sd, sm, base=rbase, forms=FORMS)
    assert r["total"] == reduce_column(want["col"], sm)
    w3, r3 = check(ctx, c["pairs"], c["tables"][:1], 1, sd[:3], sm[:3], forms=FORMS, shift=1)  # (a column 8 mod 16)
    un = ctx.unnestn(c["tables"][:1], dev(c["pairs"]))
    assert (r3["total"][1], r3["total"][0]) == (un["c_top"], un["sum_row"][0])
    # one live tuple per matched probe row: COUNT = the group's size times the probe rows that name it
    sizes = c["tables"][0].export()[1][:, 3].astype(np.uint64)
    refs = c["pairs"][:, 1]
    hits = np.bincount(refs[refs != NOREF], minlength=len(sizes)).astype(np.uint64)
    assert np.array_equal(w3["col"][:, 1], sizes * hits)


# ---- 2. every form on the same inputs ----
@pytest.fixture(scope="module")
def tiny(ctx):
    """40 groups of 1..6 rows at scattered row ids; a base relation of EDGE words for a = 1000 .."""
    import hj3d
    rng = np.random.default_rng(23)
    h = relation(rng, scattered(rng, np.arange(40, dtype=np.uint32), 1 + np.arange(40) % 6))
    d = dev(h)
    t = table_of(ctx, d, 17)
    return {"t": t, "h": h, "d": d, "m": t.size()[1], "get": columns([t], [(d, h)])}


def dense_table(ctx, groups, seed):
    """A table of exactly `groups` main records: keys 0 .. groups - 1 at scattered rows, every eleventh twice."""
    rng = np.random.default_rng(seed)
    h = relation(rng, scattered(rng, np.arange(groups, dtype=np.uint32), 1 + (np.arange(groups) % 11 == 0)))
    d = dev(h)
    t = table_of(ctx, d, max(groups // 2, 1))
    assert t.size()[1] == groups
    return {"t": t, "h": h, "d": d, "m": groups, "get": columns([t], [(d, h)])}


@pytest.fixture(scope="module")
def dense(ctx):
    made = {}

    def get(groups):
        if groups not in made:
            made[groups] = dense_table(ctx, groups, groups)
        return made[groups]
    return get


OPS2 = [("count",), ("max", 2, 0, 2)]
OPS4 = [("count",), ("sum", 1, 0, 2), ("min", 1, 0, 2), ("max", 1, 0, 2, False)]
OPS8 = OPS4 + [("sum", 1, 0, 0, False), ("min", 1, 0, 2, False), ("max", 1, 0, 2), ("count",)]


@pytest.mark.parametrize("n", ["tile-1", "tile", "round+tile+3"])
def test_tile_sizes(ctx, tiny, n):
    x = tiny
    n = {"tile-1": TILE - 1, "tile": TILE, "round+tile+3": grid_round(cus()) + TILE + 3}[n]
    t = random_refs(np.random.default_rng(n % 97), n, 2, x["m"])
    sd, sm = both(x["get"], OPS2)
    want, _ = check(ctx, t, [x["t"]] * 2, 2, sd, sm, forms=FORMS)
    assert 0 < want["n_live"] < n and x["m"] * len(OPS2) <= LDS_WORDS


def test_one_group(ctx, dense):
    """A by-table of one group: every live tuple on one address."""
    x = dense(1)
    t = np.stack([np.arange(3000), np.zeros(3000)], axis=1).astype(np.uint32)
    t[5::37, 1] = NOREF
    t[9::41, 1] = 1
    sd, sm = both(x["get"], OPS8)
    want, r = check(ctx, t, [x["t"]], 1, sd, sm, forms=FORMS)
    assert want["col"].shape == (1, 8) and 0 < want["n_live"] < 3000
    assert r["total"] == [int(v) for v in want["col"][0]]


@pytest.mark.parametrize("groups,ops", [(LDS_WORDS // 4, OPS4), (LDS_WORDS // 4 + 1, OPS4), (LDS_WORDS, OPS4[:1]),
                                        (LDS_WORDS + 1, OPS4[:1]), (LDS_WORDS // 8, OPS8), (LDS_WORDS // 8 + 1, OPS8)])
def test_at_and_past_the_lds_budget(ctx, dense, groups, ops):
    """n_mains * nspec exactly at form 2's budget and one group past it, where a forced form 2 falls back to
    form 1 (and an automatic rule that takes form 2 would change form): the same column every time."""
    x = dense(groups)
    assert (groups * len(ops) <= LDS_WORDS) == (groups % 2 == 0)
    rng = np.random.default_rng(groups)
    n = 3 * TILE + 5
    t = np.stack([np.arange(n), rng.integers(0, groups, n)], axis=1).astype(np.uint32)
    t[:4, 1] = [0, groups - 1, groups - 1, groups]  # the first and the last group; one ref just past them
    t[7::53, 1] = NOREF
    sd, sm = both(x["get"], ops)
    want, _ = check(ctx, t, [x["t"]], 1, sd, sm, forms=FORMS)
    assert int(want["col"][groups - 1, 0]) >= 2


@pytest.mark.parametrize("ops", [OPS8, OPS4, OPS4[:1]])
def test_refs_colliding_on_one_cache_slot(ctx, dense, ops):
    """Form 3: every ref = c mod slots. Two hot refs alternate, cold ones between them: one ref owns the slot,
    every other goes to the global atomics."""
    x = dense(2 * CACHE_WORDS + 16)
    slots = cache_slots(len(ops))
    c = 5
    same = np.arange(c, x["m"], slots, dtype=np.uint32)
    assert len(same) >= 3 and (same % slots == c).all()
    hot1, hot2, cold = same[-1], same[0], same[1:-1]
    n = 2 * TILE + 11
    refs = np.where(np.arange(n) % 2 == 0, hot1, hot2).astype(np.uint32)
    refs[4::5] = cold[np.arange(len(refs[4::5])) % len(cold)]
    t = np.stack([np.arange(n, dtype=np.uint32), refs], axis=1)
    sd, sm = both(x["get"], ops)
    want, _ = check(ctx, t, [x["t"]], 1, sd, sm, forms=FORMS)
    assert int(want["col"][hot1, 0]) > n // 3 and int(want["col"][hot2, 0]) > n // 3


def test_scattered_refs_empty_input_and_cleared_table(ctx, tiny, dense):
    import hj3d
    x, big = tiny, dense(LDS_WORDS // 4 + 1)
    rng = np.random.default_rng(61)
    n = 2 * TILE + 77
    # k = 2 over two tables, refs scattered over all of the larger one, grouped by either
    t = np.stack([np.arange(n), rng.integers(0, x["m"] + 2, n), rng.permutation(n) % (big["m"] + 1)], axis=1).astype(np.uint32)
    get = columns([x["t"], big["t"]], [(x["d"], x["h"]), (big["d"], big["h"])])
    sd, sm = both(get, [("count",), ("sum", 1, 0, 2), ("max", 2, 1, 2, False), ("min", 2, 1, 0)])
    for by in (1, 2):
        want, _ = check(ctx, t, [x["t"], big["t"]], by, sd, sm, forms=FORMS)
        assert 0 < want["n_live"] < n
    # n = 0: the column is initialised
    w0, r0 = check(ctx, t[:0], [x["t"], big["t"]], 2, sd, sm, forms=FORMS)
    assert r0["n_in"] == 0 and w0["col"].tolist() == [[0, 0, 0, AN.I64_MAX]] * big["m"]
    # a cleared by-table: nothing is written, no tuple is live
    gone = hj3d.Table(ctx, hj3d.HJ3D_NESTED, 16)
    gone.build(hj3d.Rel(x["d"], key_word=1))
    gone.clear()
    for form in FORMS:
        r, col = run(ctx, dev(t), [x["t"], gone], 2, sd[:2], cap=5, form=form)
        assert col.shape == (0, 2) and (r["n_in"], r["n_live"], r["c_top"], r["total"]) == (n, 0, 0, [0, 0])
    gone.close()


# ---- 3. capacity ----
def test_capacity(ctx, tiny):
    import torch
    import hj3d
    x = tiny
    t = random_refs(np.random.default_rng(31), TILE + 9, 1, x["m"])
    sd, sm = both(x["get"], OPS4)
    buf = torch.full((x["m"] + GUARD, 4), CANARY, dtype=torch.int64, device="cuda")
    for form in FORMS:
        ctx.gby_form(form)
        try:
            with pytest.raises(hj3d.Hj3dError) as e:
                ctx.agg_grouped(dev(t), [x["t"]], 1, sd, out=buf[:x["m"] - 1])
        finally:
            ctx.gby_form(0)
        assert e.value.status == hj3d.HJ3D_EOVERFLOW
        ctx.sync()
        assert bool((buf == CANARY).all())
    check(ctx, t, [x["t"]], 1, sd, sm, forms=FORMS)  # out_cap = n_mains exactly: the guard rows behind it are intact


# ---- 4. ACCUMULATE ----
def test_accumulate(ctx, tiny):
    x = tiny
    m = x["m"]
    n = 2 * TILE + 10
    rng = np.random.default_rng(67)
    t = random_refs(rng, n, 2, m)
    half = n // 2
    t[:half, 1] %= m // 2  # groups m / 2 .. m - 1 are hit by the second half only
    ops = [("count",), ("sum", 2, 0, 2), ("min", 1, 0, 2), ("max", 1, 0, 2), ("min", 2, 0, 2, False), ("max", 2, 0, 2, False)]
    sd, sm = both(x["get"], ops)
    tabs = [x["t"]] * 2
    whole, _ = check(ctx, t, tabs, 1, sd, sm)
    for form in FORMS:
        first, _ = check(ctx, t[:half], tabs, 1, sd, sm, forms=(form,))
        assert (first["col"][m // 2:] == np.array([AG.identity(sp) for sp in sm], dtype=np.uint64)).all()
        both_, r = check(ctx, t[half:], tabs, 1, sd, sm, forms=(form,), into=first["col"], accumulate=True)
        assert np.array_equal(both_["col"], whole["col"]) and not np.array_equal(first["col"], whole["col"])
        assert (both_["col"][m // 2:, 0] > 0).any() and r["n_in"] == n - half  # the result restarts
    # another tuple set folded in: the model of the concatenation
    other = random_refs(np.random.default_rng(71), TILE + 3, 2, m)
    cat, _ = check(ctx, np.concatenate([t, other]), tabs, 1, sd, sm)
    check(ctx, other, tabs, 1, sd, sm, forms=FORMS, into=whole["col"], accumulate=True)
    assert np.array_equal(AG.agg_grouped(other, [x["t"].export()[1]] * 2, 1, sm, into=whole["col"])["col"], cat["col"])


# ---- 5. magnitude: a product or a total of 2^64, in a process of its own under a time limit ----
def test_magnitude_is_refused_promptly():
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "agg_grouped_magnitude_case.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "magnitude OK" in r.stdout


# ---- 6. arguments ----
def test_result_slots_are_separate(ctx, chained):  # noqa: F811
    c = chained
    x = dev(c["h"])
    sd, _ = both(c["get"], [("count",), ("sum", 1, 0, 0, False)])
    ctx.select_nested(x, [])
    pr = ctx.probe_result()
    un = ctx.unnestn(c["tables"], x)
    an = ctx.agg_nested(x[:100], c["tables"], sd)
    _, r = ctx.agg_grouped(x, c["tables"], 2, sd)
    assert ctx.probe_result() == pr and ctx.unnestn_result() == un and ctx.agg_nested_result() == an
    assert ctx.agg_grouped_result() == r and r["n_in"] == len(c["h"]) != an["n_in"]


def test_refusals(ctx, chained, rbase):  # noqa: F811
    import torch
    import hj3d
    L = hj3d.lib()
    c = chained
    ts, tt = c["tables"]
    scol, _ = c["get"](0, 0, False)
    tcol, _ = c["get"](1, 0, False)
    nested = dev(c["h"][:64])
    ms, mt = ts.size()[1], tt.size()[1]
    out = torch.zeros((max(ms, mt), 3), dtype=torch.int64, device="cuda")
    A = hj3d.PROBE_ACCUMULATE
    tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, 64)
    tc.build(hj3d.Rel(dev(np.zeros((8, 2), np.uint32)), key_word=1))
    base = rbase[0]
    explicit = hj3d.Rel(base.tensor, key_word=1, row_word=1)
    broken = hj3d.Rel(base.tensor, key_word=1)
    broken.c.stride = 6

    def arr(*hs):
        return (C.c_void_p * len(hs))(*hs)

    def specs(*sp):
        a = (hj3d._GbySpec * max(len(sp), 1))()
        for i, (op, slot, col, n, *woff) in enumerate(sp):
            a[i] = hj3d._GbySpec(op, slot, 0, woff[0] if woff else 0, col, n)
        return a

    S, T = (hj3d.AGG_SUM, 1, scol.data_ptr(), scol.shape[0]), (hj3d.AGG_MIN, 2, tcol.data_ptr(), tcol.shape[0])
    CNT, BW = (hj3d.AGG_COUNT, 0, None, 0), (hj3d.AGG_MAX_, 0, None, 0, 4)
    good = specs(S, CNT, T)

    def st(ctxh=ctx.h, ptr=nested.data_ptr(), n=64, k=2, tables=arr(ts.h, tt.h), by=1, b=None, sp=good, nspec=3, flags=0,
           optr=out.data_ptr(), cap=out.shape[0]):
        return L.hj3d_agg_grouped(ctxh, ptr, n, k, tables, by, None if b is None else C.byref(b.c), sp, nspec, flags, optr, cap)

    bad = hj3d.HJ3D_EINVAL
    fresh = hj3d.Context(0)
    assert L.hj3d_agg_grouped_result(fresh.h, C.byref(hj3d._AggNRes())) == bad  # before any hj3d_agg_grouped
    fresh.close()
    assert st() == hj3d.HJ3D_OK and st(flags=A) == hj3d.HJ3D_OK and st(by=2) == hj3d.HJ3D_OK
    for f in (hj3d.PROBE_UNIQUE, hj3d.PROBE_UNNEST, hj3d.PROBE_EMIT, hj3d.PROBE_CHECKSUM, hj3d.PROBE_MAINREF, 0x40):
        assert st(flags=f) == bad and st(flags=A | f) == bad                                  # any other flag
    assert st(ctxh=None) == bad and st(tables=None) == bad and st(sp=None) == bad             # null ctx / tables / specs
    assert st(tables=arr(ts.h, None)) == bad and st(tables=arr(None, tt.h)) == bad            # a null table entry
    assert st(tables=arr(ts.h, tc.h)) == bad                                                  # a chaining table
    assert st(k=0) == bad and st(k=7, tables=arr(*([ts.h] * 7))) == bad                       # k outside 1 .. HJ3D_NEST_MAX
    assert st(by=0) == bad and st(by=3) == bad                                                # by_slot outside 1 .. k
    assert st(nspec=0) == bad and st(sp=specs(*([CNT] * 9)), nspec=9) == bad                  # nspec outside 1 .. HJ3D_AGG_MAX
    out8 = torch.zeros((ms, 8), dtype=torch.int64, device="cuda")
    assert st(sp=specs(*([CNT] * 8)), nspec=8, optr=out8.data_ptr(), cap=ms) == hj3d.HJ3D_OK
    assert st(sp=specs((4, 1, scol.data_ptr(), scol.shape[0])), nspec=1) == bad               # an unknown op
    assert st(sp=specs((hj3d.AGG_SUM, 3, scol.data_ptr(), scol.shape[0])), nspec=1) == bad    # slot > k
    assert st(sp=specs((hj3d.AGG_COUNT, 1, None, 0)), nspec=1) == bad                         # COUNT with slot != 0
    assert st(sp=specs((hj3d.AGG_COUNT, 1, scol.data_ptr(), scol.shape[0])), nspec=1) == bad
    assert st(sp=specs((hj3d.AGG_MAX_, 1, None, scol.shape[0])), nspec=1) == bad              # slot >= 1 with a null gcol
    assert st(sp=specs((hj3d.AGG_SUM, 1, scol.data_ptr(), scol.shape[0] - 1)), nspec=1) == bad  # gcol_n too small
    assert st(sp=specs((hj3d.AGG_SUM, 2, scol.data_ptr(), tcol.shape[0] - 1)), nspec=1) == bad
    assert st(sp=specs(BW), nspec=1, b=base) == hj3d.HJ3D_OK
    assert st(sp=specs(BW), nspec=1) == bad                                                   # a base word: base null,
    assert st(sp=specs(BW), nspec=1, b=broken) == bad                                         # invalid,
    assert st(sp=specs(BW), nspec=1, b=explicit) == bad                                       # with explicit rows
    assert st(sp=specs((hj3d.AGG_MAX_, 0, None, 0, 2)), nspec=1, b=base) == bad               # word_off not a multiple of 4
    assert st(sp=specs((hj3d.AGG_MAX_, 0, None, 0, 8)), nspec=1, b=base) == bad               # word_off outside the tuple
    assert st(sp=specs(CNT), nspec=1, b=broken) == hj3d.HJ3D_OK                               # (no base word: base is not looked at)
    assert st(sp=specs((hj3d.AGG_SUM, 1, scol.data_ptr() + 4, scol.shape[0] - 1)), nspec=1) == bad  # misaligned pointers
    assert st(ptr=nested.data_ptr() + 2) == bad and st(optr=out.data_ptr() + 4) == bad
    assert st(ptr=None) == bad                                                                # n && !nested_dev
    assert st(optr=None) == bad and st(optr=None, cap=0) == bad                               # no column, a non-empty by-table
    assert st(n=1 << 32) == bad
    assert st(cap=ms - 1) == hj3d.HJ3D_EOVERFLOW and st(by=2, cap=mt - 1) == hj3d.HJ3D_EOVERFLOW
    assert st(ptr=None, n=0) == hj3d.HJ3D_OK
    r = ctx.agg_grouped_result()
    assert (r["n_in"], r["n_live"], r["c_top"]) == (0, 0, 0)
    with pytest.raises(hj3d.Hj3dError):
        ctx.set_option(hj3d.OPT_GBY_FORM, 4)
    with pytest.raises(ValueError):
        ctx.agg_grouped(nested, [ts, tt], 1, [])
    with pytest.raises(ValueError):
        ctx.agg_grouped(nested, [ts, tt], 3, [("count",)])
    with pytest.raises(ValueError):
        ctx.agg_grouped(nested, [ts, tt], 1, [("avg", 1, scol)])
    with pytest.raises(ValueError):
        ctx.agg_grouped(nested, [ts, tt], 1, [("sum", "base", 0)])  # no base given
    with pytest.raises(ValueError):
        ctx.agg_grouped(nested, [ts, tt], 1, [("count",)], out=torch.zeros((ms, 2), dtype=torch.int64, device="cuda"))
    tc.close()


# ---- 7. a context on a side stream: the tuples and a column written late on it ----
def test_side_stream_late_inputs():
    import torch
    import hj3d
    import stream_cases as SC
    import stream_order as SO
    s = torch.cuda.Stream()
    side = hj3d.Context(0, stream=s)
    try:
        rng = np.random.default_rng(89)
        h = relation(rng, scattered(rng, np.arange(300, dtype=np.uint32), 1 + np.arange(300) % 5))
        with torch.cuda.stream(s):
            d = SO.to_device(h)
            t = table_of(side, d, 101)
            m = t.size()[1]
            col, _ = t.group_agg(hj3d.Rel(d, key_word=1), 2, True)
            col_np = host64(col)
            side.sync()
        tuples = random_refs(rng, 3 * TILE + 17, 1, m)
        sm = [("count",), ("sum", 1, col_np), ("min", 1, col_np), ("max", 1, col_np)]
        want = AG.agg_grouped(tuples, [t.export()[1]], 1, sm)
        assert 0 < want["n_live"] < len(tuples)
        late_n = SO.Late.of(tuples, SC.decoy_nested(tuples))
        late_c = SO.Late.of(col_np, SC.decoy_column(col_np))
        with torch.cuda.stream(s):
            out = torch.zeros((m + 8, 4), dtype=torch.int64, device="cuda")
        sd = [("count",), ("sum", 1, late_c.tensor), ("min", 1, late_c.tensor), ("max", 1, late_c.tensor)]
        harness = SO.Harness(s)

        def call():
            side.agg_grouped(late_n.tensor, [t], 1, sd, out=out[:m], fetch=False)
        o = harness.run("agg_grouped", [late_n, late_c], call, outputs=[out], fully_async=True, reset=call)
        r = side.agg_grouped_result()
        assert (r["n_in"], r["n_live"], r["c_top"], r["total"]) == (len(tuples), want["n_live"], want["c_top"], want["total"])
        got = harness.host(o.clones[0]).view(np.uint64)
        assert (got[m:] == SO.CANARY).all()
        assert np.array_equal(got[:m], want["col"])
        t.close()
    finally:
        side.close()


# ---- 8. the plan hook ----
def by_key(col, key_field, specs):
    """{key: the row} of the groups a tuple hit (their MIN(key word) names them); the other rows hold identities."""
    ident = [AG.identity(sp) for sp in specs]
    out = {}
    for row in col.tolist():
        if row == ident:
            continue
        assert row[key_field] not in out
        out[row[key_field]] = row
    return out


@pytest.mark.parametrize("by", [0, 1])
def test_plan_grouped(ctx, by):
    import hj3d
    g, R, S, T = plan_relations()
    ref = g["plans"]["Ndu"]
    builds = [(dev(S), 1), (dev(T), 1)]
    agg = [("count",), ("min", by, 1, False), ("sum", 0, 0, False), ("max", 1, 0, False), ("sum", "base", 0, False), ("min", "base", 0)]
    got = hj3d.star_plan_grouped(ctx, dev(R), builds, g["nb"], keys=(0, 0), by=by, aggregate=agg)
    col = host64(got["column"])
    distinct = len(np.unique((S, T)[by][:, 1]))
    assert col.shape == (distinct, len(agg))
    assert AN._sum64(col[:, 0]) == got["c_top"] == got["total"][0] == ref["c_top"]
    assert got["total"][2] == ref["out"]["sum_b"] == AN._sum64(col[:, 2])
    plain = hj3d.star_plan_aggregate(ctx, dev(R), builds, g["nb"], keys=(0, 0), aggregate=agg[:4])
    assert (got["n_in"], got["n_live"], got["c_probe"], got["total"][:4]) == \
        (plain["n_in"], plain["n_live"], plain["c_probe"], plain["total"])
    # with a filter: the model on the filtered chain, over tables laid out by numpy, compared per key
    k = R[:, 0].astype(np.int64)
    tabs = [AN.table_arrays(S[:, 1]), AN.table_arrays(T[:, 1])]
    keep = (k >= 100) & (k < 700)
    refs = [np.array([tab[2].get(int(v), NOREF) if ok else NOREF for v, ok in zip(k, keep)], dtype=np.uint32) for tab in tabs]
    tuples = np.stack([np.arange(len(R), dtype=np.uint32)] + refs, axis=1)
    gcols = {(lvl, w): AN.group_agg(tabs[lvl][0], tabs[lvl][1], (S, T)[lvl], w, False)["col"] for lvl, w in ((by, 1), (0, 0), (1, 0))}
    sm = [("count",), ("min", by + 1, gcols[(by, 1)], False), ("sum", 1, gcols[(0, 0)], False), ("max", 2, gcols[(1, 0)], False),
          ("sum", "base", 0, False), ("min", "base", 0)]
    want = AG.agg_grouped(tuples, [tabs[0][0], tabs[1][0]], by + 1, sm, base=R)
    got = hj3d.star_plan_grouped(ctx, dev(R), builds, g["nb"], keys=(0, 0), by=by, aggregate=agg,
                                 filters={0: [("base", 0, "range", 100, 700)]})
    assert 0 < want["n_live"] < plain["n_live"]
    assert (got["n_live"], got["c_top"], got["total"]) == (want["n_live"], want["c_top"], want["total"])
    assert by_key(host64(got["column"]), 1, sm) == by_key(want["col"], 1, sm) != {}
