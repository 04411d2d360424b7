"""hj3d_select_nested on the GPU: the selection between the nested probe and the unnest
(AlgSelection / AlgDynSelection, algebra.hh:278-358, stacked on AlgNestJoinProbe, algebra.hh:435-459)
over stored nested tuples {a, ref_1 .. ref_k}, and the plan hook star_plan_chained(filters=...).

Expected values: tests/select_nested_ref.py (numpy; pinned by tests/test_select_nested_ref.py) over
Table.export(), the host's own filters, hj3d_probe_sel (the pushed-down form of a base predicate),
tests/expand_n_ref.py over the build key columns, and the reference binary's experiment-4 fixture.
Integer work: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import expand_n_ref as XN
import expand_ref as X
import oracle as O
import select_nested_ref as SN
from test_gpu_expand_limits import canary_buffer, key_refs, nested_table, scattered, tail_intact
from test_gpu_unnest import CANARY, EXP4, NOREF, dev, host, mainref_probe, nrs_table
from test_gpu_unnestn import parity  # noqa: F401  (the Zipf fixture: R, S, T, two tables of different bucket counts)

pytestmark = pytest.mark.gpu

# select_nested.hip's constants (a change there must fail the size cases below, not empty them)
BLOCK, ITEMS = 256, 16  # kBlock, kNselItems
TILE = BLOCK * ITEMS    # kNselTile: tuples per workgroup; one workgroup per tile (no grid stride)
EDGE = np.array([0, 1, 5, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)


def fields(r) -> tuple:
    return (r.n_probe, r.n_matched, r.n_out, r.n_cmps, r.sum_a, r.sum_b, r.sum_c, r.sum_h, r.xor_h)


def run(ctx, nested, preds, cap, **kw):
    """(result, the rows written) with a canary tail behind the cap rows."""
    buf = canary_buffer(cap, nested.shape[1])
    r = ctx.select_nested(nested, preds, out=buf[:cap], **kw)
    assert tail_intact(buf, cap)
    return r, host(buf[:min(cap, r.n_out)])


def check(ctx, tuples, preds, model_kw=None, **kw):
    """select_nested of host tuples against the model: counters, rows in order, canary."""
    want = SN.select_nested(tuples, preds, **(model_kw or {}))
    r, rows = run(ctx, dev(tuples), preds, len(tuples), **kw)
    assert fields(r) == SN.counters(want) and not r.overflow
    assert np.array_equal(rows, want["rows"])
    return want


# ---- 1. compaction of a MAINREF probe's dense output ----
def test_compaction(ctx):
    import torch
    t, probe, nR = nrs_table(ctx, "exp1_R1024_S4096_zipf")
    pr, nested = mainref_probe(ctx, t, probe, nR)
    h = host(nested)
    keep = h[h[:, 1] != NOREF]
    assert 0 < pr.n_matched == len(keep) < nR
    for tables in (None, [t]):
        r, rows = run(ctx, nested, [], nR, base=probe, tables=tables)
        assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps, r.overflow) == (nR, pr.n_matched, pr.n_matched, 0, False)
        assert np.array_equal(rows, keep)  # in input order
        assert fields(r) == SN.counters(SN.select_nested(h, []))
    full, part = ctx.unnest(t, nested), ctx.unnest(t, dev(rows))
    assert fields(full)[1:] == fields(part)[1:] and part.n_probe == len(keep) and full.n_out > full.n_matched
    out_a = torch.zeros((full.n_out, 2), dtype=torch.int32, device="cuda")
    out_b = torch.zeros((full.n_out, 2), dtype=torch.int32, device="cuda")
    ctx.unnest(t, nested, out=out_a)
    ctx.unnest(t, dev(rows), out=out_b)
    assert np.array_equal(XN.sort_rows(host(out_a)), XN.sort_rows(host(out_b)))


# ---- 2. a base predicate here equals the same predicate pushed below the probe ----
@pytest.fixture(scope="module")
def pushdown(ctx):
    import hj3d
    Rk, Sa, _ = O.gen_exp1(1024, 4096, True, 1.0, 0)
    rng = np.random.default_rng(71)
    R = np.stack([Rk, rng.integers(0, 40, len(Rk)).astype(np.uint32), EDGE[rng.integers(0, len(EDGE), len(Rk))]], axis=1)
    R = np.ascontiguousarray(R.astype(np.uint32))
    dR, dS = dev(R), dev(O.tuples3(np.arange(4096, dtype=np.uint32), Sa))
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, O.num_distinct(Sa))
    t.build(hj3d.Rel(dS, key_word=1))
    probe = hj3d.Rel(dR, key_word=0)
    pr, nested = mainref_probe(ctx, t, probe, len(R))
    assert 0 < pr.n_matched < len(R)
    return {"R": R, "dR": dR, "dS": dS, "t": t, "probe": probe, "nested": nested}


PUSH = [[(2, op, lo, lo + 3, signed)] for op in SN.OPS for signed in (True, False) for lo in (0x7FFFFFFF, 5)] + [
    [(1, ">=", 10), (2, "<", 0)],
    [(1, "range", 5, 30), (2, "!=", 5, None, False), (0, "<", 900)],
    [(1, ">", 3), (1, "<=", 35), (2, ">", 0x7FFFFFFF, None, False), (0, "range", 16, 1000)],
    [(1, "range", 7, 7)],                         # empty interval
    [(2, "range", 0, 1 << 32, False)],            # full interval
]


@pytest.mark.parametrize("preds", PUSH, ids=lambda p: "&".join(f"w{q[0]}{q[1]}{q[2]}{'' if len(q) < 5 or q[4] else 'u'}" for q in p))
def test_pushdown_equivalence(ctx, pushdown, preds):
    import torch
    p = pushdown
    n = len(p["R"])
    mine = [("base",) + tuple(q) for q in preds]
    want = SN.select_nested(host(p["nested"]), mine, base=p["R"])
    r, rows = run(ctx, p["nested"], mine, n, base=p["probe"], tables=[p["t"]])
    assert fields(r) == SN.counters(want) and np.array_equal(rows, want["rows"])
    dense = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    ps = ctx.probe_sel(p["t"], p["probe"], preds, out=dense, mainref=True)
    d = host(dense)[:ps.n_probe]
    d = d[d[:, 1] != NOREF]
    assert ps.n_matched == len(d) == r.n_out
    assert np.array_equal(XN.sort_rows(d), XN.sort_rows(rows))


# ---- 3. predicates on the groups: COUNT, FIRST, conjunctions (Zipf 1.0, two tables, k = 2) ----
@pytest.fixture(scope="module")
def triples(ctx, parity):  # noqa: F811
    import torch
    import hj3d
    p = parity
    trip = torch.zeros((4097, 3), dtype=torch.int32, device="cuda")
    rt = ctx.probe_refn(p["tt"], hj3d.Rel(p["R"], key_word=1), p["pairs"], out=trip)
    h = host(trip[:rt.n_out]).copy()
    h[::50, 1] = NOREF
    h[7::50, 2] = NOREF
    return {"h": h, "x": dev(h), "ms": p["ts"].export()[1], "mt": p["tt"].export()[1], "R": host(p["R"]),
            "S": host(p["S"]), "T": host(p["T"])}


GROUP = [
    [("count", 1, ">=", 2)], [("count", 2, ">=", 2)], [("count", 1, "range", 2, 6)], [("count", 2, "==", 1)],
    [("first", 1, 1, "<", 100)], [("first", 2, 1, ">=", 40)], [("first", 2, 0, "range", 1000, 3000)],
    [("count", 1, ">=", 2), ("count", 2, ">=", 2)],
    [("count", 1, "<=", 3), ("first", 1, 1, "!=", 0), ("base", 1, "<", 300)],
    [("base", 0, ">", 500), ("count", 2, "<", 4), ("first", 1, 0, ">", 100), ("first", 2, 1, "<", 500)],
    [("count", 1, ">=", 2), ("count", 1, "<", 50), ("first", 1, 1, ">", 2), ("first", 1, 0, "<", 4000)],  # one slot, four readers
]


@pytest.mark.parametrize("preds", GROUP, ids=lambda p: "&".join(f"{q[0]}{q[1]}" for q in p))
def test_group_predicates(ctx, parity, triples, preds):  # noqa: F811
    import hj3d
    p, x = parity, triples
    want = SN.select_nested(x["h"], preds, base=x["R"], mains=[x["ms"], x["mt"]], builds=[x["S"], x["T"]])
    assert 0 < want["n_out"] < want["n_matched"] < len(x["h"])  # some pass, some fail, some are dead
    r, rows = run(ctx, x["x"], preds, len(x["h"]), base=hj3d.Rel(p["R"], key_word=0), tables=[p["ts"], p["tt"]],
                  builds=[hj3d.Rel(p["S"], key_word=1), hj3d.Rel(p["T"], key_word=1)])
    assert fields(r) == SN.counters(want) and not r.overflow
    assert np.array_equal(rows, want["rows"])


# ---- 4. the selection commutes with the unnest ----
def test_commutes_with_unnest(ctx, parity, triples):  # noqa: F811
    import torch
    import hj3d
    p, x = parity, triples
    tables = [p["ts"], p["tt"]]
    preds = [("base", 1, "<", 300), ("count", 1, ">=", 2)]
    r, kept = run(ctx, x["x"], preds, len(x["h"]), base=hj3d.Rel(p["R"], key_word=0), tables=tables)
    assert 0 < r.n_out < r.n_matched
    full = ctx.unnestn(tables, x["x"])
    out_full = torch.zeros((full["c_top"], 3), dtype=torch.int32, device="cuda")
    ctx.unnestn(tables, x["x"], out=out_full)
    sel = ctx.unnestn(tables, dev(kept))
    out_sel = torch.zeros((sel["c_top"], 3), dtype=torch.int32, device="cuda")
    sel = ctx.unnestn(tables, dev(kept), out=out_sel)
    # the host filter over the unfiltered expansion: R.y of row a, and the size of the S group the row
    # s_row belongs to, from the S key column alone
    rows = host(out_full)
    Sa = x["S"][:, 1]
    size = X.group_index(Sa).locate(Sa[rows[:, 1]].astype(np.int64))[1]
    want = rows[(x["R"][rows[:, 0], 1].astype(np.int64) < 300) & (size >= 2)]
    assert 0 < len(want) < len(rows) and not sel["overflow"]
    assert sel["c_top"] == len(want)
    assert np.array_equal(XN.sort_rows(host(out_sel)), XN.sort_rows(want))


# ---- 5. every width, the tile boundaries, rows that are 4-byte aligned only ----
SIZES = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)


def opaque_tuples(k, n, seed):
    """n tuples of k opaque refs with a NOREF at each position in turn (and some tuples with several)."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 1 << 32, (n, k + 1), dtype=np.uint64).astype(np.uint32)
    t[:, 1:][t[:, 1:] == NOREF] = 0
    for j in range(1, k + 1):
        t[j::2 * k + 1, j] = NOREF
    if k:
        t[5::97, 1:] = NOREF
    return t


@pytest.mark.parametrize("k", range(7))
def test_every_width_and_size(ctx, k):
    for n in SIZES:
        t = opaque_tuples(k, n, 100 * k + n % 89)
        want = check(ctx, t, [])
        if n >= 63 and k:
            assert 0 < want["n_out"] < n, n
        if k == 0:
            assert want["n_out"] == n
    nock = ctx.select_nested(dev(t), [], checksum=False)
    assert (nock.sum_h, nock.xor_h) == (0, 0) and fields(nock)[:7] == SN.counters(want)[:7]


@pytest.mark.parametrize("k", range(7))
def test_rows_not_16_byte_aligned(ctx, k):
    import torch
    W, n = k + 1, TILE + 1
    t = opaque_tuples(k, n, 900 + k)
    src = torch.full((n * W + 8,), CANARY, dtype=torch.int32, device="cuda")
    dst = torch.full((n * W + 8,), CANARY, dtype=torch.int32, device="cuda")
    nested, out = src[1:1 + n * W].view(n, W), dst[1:1 + n * W].view(n, W)
    assert nested.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    nested.copy_(dev(t))
    want = SN.select_nested(t, [])
    r = ctx.select_nested(nested, [], out=out)
    assert fields(r) == SN.counters(want) and not r.overflow
    d = host(dst)
    assert np.array_equal(d[1:1 + r.n_out * W].reshape(-1, W), want["rows"])
    assert d[0] == CANARY and (d[1 + r.n_out * W:] == CANARY).all()


# ---- 6. capacity ----
def test_capacity(ctx):
    n = 2 * TILE + 77
    t = opaque_tuples(2, n, 61)
    want = SN.select_nested(t, [])
    x = dev(t)
    assert TILE < want["n_out"] < n
    for cap in (want["n_out"] - 1, TILE + 3, 1, 0):
        r, rows = run(ctx, x, [], cap)  # (checks the canary rows behind cap)
        assert r.overflow and fields(r) == SN.counters(want), cap  # complete counters
        assert np.array_equal(rows, want["rows"][:cap]), cap         # the first cap passing tuples, in order
    r, rows = run(ctx, x, [], want["n_out"])
    assert not r.overflow and np.array_equal(rows, want["rows"])
    r = ctx.select_nested(x, [])  # no buffer: counters only
    assert not r.overflow and fields(r) == SN.counters(want)
    r = ctx.select_nested(x, [], checksum=False)
    assert (r.sum_h, r.xor_h) == (0, 0) and fields(r)[:7] == SN.counters(want)[:7]
    r = ctx.select_nested(x, [], fetch=False)
    assert r is None and fields(ctx.probe_result()) == SN.counters(want)


# ---- 7. dead tuples and stale refs ----
def test_a_outside_a_base_with_row_base(ctx):
    import hj3d
    rng = np.random.default_rng(83)
    B = np.stack([np.arange(500), rng.integers(0, 100, 500)], axis=1).astype(np.uint32)
    a = rng.integers(990, 1000 + 500 + 10, 3000).astype(np.uint32)
    a[::40] = rng.integers(0, 1 << 32, len(a[::40]), dtype=np.uint64).astype(np.uint32)
    a[1::40] = 999 + np.arange(len(a[1::40])) % 2    # the first row and the one below it
    a[2::40] = 1499 + np.arange(len(a[2::40])) % 2   # the last row and the one above it
    t = np.stack([a, rng.integers(0, 9, len(a)).astype(np.uint32)], axis=1)
    base = hj3d.Rel(dev(B), key_word=0, row_base=1000)
    for preds in ([], [("base", 1, "<", 50)]):
        want = check(ctx, t, preds, dict(base=B, base_row_base=1000), base=base)
        assert 0 < want["n_out"] < want["n_probe"] and want["n_matched"] == int(((a >= 1000) & (a < 1500)).sum())


def test_stale_refs_and_first_rows(ctx):
    import hj3d
    rng = np.random.default_rng(59)
    old_col = scattered(rng, np.arange(200, dtype=np.uint32), np.full(200, 2))
    t, _rel = nested_table(ctx, old_col, 97)
    old_refs = key_refs(ctx, t, np.arange(200, dtype=np.uint32))
    refs = np.array([old_refs[k] for k in range(200)], dtype=np.uint32)
    tup = np.stack([np.arange(200, dtype=np.uint32), refs], axis=1)
    assert sorted(refs.tolist()) == list(range(200))
    # rebuilt smaller: refs at or above the new main-record count are dropped when the table is given
    new_col = scattered(rng, np.arange(50, dtype=np.uint32) + 1000, 1 + np.arange(50) % 5)
    new_rel = dev(O.tuples2(np.arange(len(new_col), dtype=np.uint32), new_col))
    t.build(hj3d.Rel(new_rel, key_word=1))
    assert t.build_path(finish=False).endswith("?")
    r, rows = run(ctx, dev(tup), [("count", 1, ">=", 1)], 200, tables=[t])  # the call finishes the build
    assert "?" not in t.build_path(finish=False)
    _, payload, _ = t.export()
    assert len(payload) == 50
    want = SN.select_nested(tup, [("count", 1, ">=", 1)], mains=[payload])
    assert fields(r) == SN.counters(want) and np.array_equal(rows, want["rows"])
    assert r.n_matched == r.n_out == 50 == int((refs < 50).sum())
    # group predicates over the refs that stayed valid (they name the new content's groups)
    build = hj3d.Rel(new_rel, key_word=1)
    for preds in ([("count", 1, ">=", 3)], [("first", 1, 1, "<", 1025)], [("count", 1, "<", 4), ("first", 1, 0, ">=", 20)]):
        want = check(ctx, tup, preds, dict(mains=[payload], builds=[host(new_rel)]), tables=[t], builds=[build])
        assert 0 < want["n_out"] < want["n_matched"] == 50
    # without the table the refs are opaque: every tuple is kept
    check(ctx, tup, [])
    assert SN.select_nested(tup, [])["n_out"] == 200
    # a FIRST row outside its build relation: the relation given is a prefix of the one built from
    half = len(new_col) // 2
    short = hj3d.Rel(new_rel, key_word=1, n=half)
    want = check(ctx, tup, [("first", 1, 1, ">=", 0)], dict(mains=[payload], builds=[host(new_rel)[:half]]), tables=[t],
                 builds=[short])
    assert 0 < want["n_matched"] == int((payload[:, 1] < half).sum()) < 50
    # cleared: no ref is valid when the table is given
    t.clear()
    r, rows = run(ctx, dev(tup), [], 200, tables=[t])
    assert (r.n_probe, r.n_matched, r.n_out, r.sum_a, r.sum_h, r.xor_h, len(rows)) == (200, 0, 0, 0, 0, 0, 0)
    r = ctx.select_nested(dev(tup), [], tables=[None])
    assert r.n_out == 200
    t.close()


# ---- 8. refusals ----
def test_refusals(ctx, parity, triples):  # noqa: F811
    import torch
    import hj3d
    L = hj3d.lib()
    p, x = parity, triples
    tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, 64)
    tc.build(hj3d.Rel(p["S"], key_word=1))
    nested = x["x"][:64].contiguous()
    out = torch.zeros((64, 3), dtype=torch.int32, device="cuda")
    E = hj3d.PROBE_EMIT
    base = hj3d.Rel(p["R"], key_word=0)
    explicit = hj3d.Rel(p["R"], key_word=0, row_word=2)
    good_preds = [("base", 1, "<", 300), ("count", 1, ">=", 2), ("first", 2, 1, "<", 500)]

    def arr(*hs):
        return (C.c_void_p * len(hs))(*hs)

    def rels(*rs):
        return (hj3d._Rel * len(rs))(*[hj3d._Rel() if r is None else r.c for r in rs])

    both = rels(hj3d.Rel(p["S"], key_word=1), hj3d.Rel(p["T"], key_word=1))

    def st(c=ctx.h, ptr=nested.data_ptr(), n=64, k=2, b=base, tables=arr(p["ts"].h, p["tt"].h), builds=both,
           preds=good_preds, npred=None, flags=E, optr=out.data_ptr(), cap=64, raw=None):
        pa = raw if raw is not None else hj3d._nsel_preds(preds)
        return L.hj3d_select_nested(c, ptr, n, k, None if b is None else C.byref(b.c), tables, builds, pa,
                                    len(preds) if npred is None else npred, flags, optr, cap)

    bad = hj3d.HJ3D_EINVAL
    assert st() == hj3d.HJ3D_OK
    for f in (hj3d.PROBE_UNIQUE, hj3d.PROBE_UNNEST, hj3d.PROBE_ACCUMULATE, hj3d.PROBE_MAINREF, 0x40):
        assert st(flags=E | f) == bad
    assert st(c=None) == bad
    assert st(k=hj3d.HJ3D_NEST_MAX + 1, preds=[]) == bad
    five = hj3d._nsel_preds([("base", 1, "<", 300)] * 5)
    assert st(raw=five, npred=5) == bad and st(raw=None, preds=[("base", 1, "<", 300)], npred=None) == hj3d.HJ3D_OK
    assert st(raw=C.POINTER(hj3d._NSelPred)(), npred=1) == bad  # npred && !preds
    assert st(preds=[("count", 0, ">=", 1)]) == bad and st(preds=[("count", 3, ">=", 1)]) == bad
    assert st(preds=[("first", 0, 1, ">=", 1)]) == bad and st(preds=[("first", 3, 1, ">=", 1)]) == bad
    raw = hj3d._nsel_preds([("base", 1, "<", 300)])
    raw[0].slot = 1
    assert st(raw=raw, npred=1) == bad          # BASE: slot 0
    raw = hj3d._nsel_preds([("base", 1, "<", 300)])
    raw[0].source = 3
    assert st(raw=raw, npred=1) == bad          # unknown source
    for kind in (("base", 1), ("count", 1), ("first", 1, 1)):
        raw = hj3d._nsel_preds([kind + ("<", 300)])
        raw[0].pred.op = 7
        assert st(raw=raw, npred=1) == bad      # unknown op
    assert st(preds=[("base", 3, "<", 1)]) == bad and st(preds=[("first", 1, 2, "<", 1)]) == bad  # word outside the tuple
    raw = hj3d._nsel_preds([("base", 1, "<", 300)])
    raw[0].pred.word_off = 2
    assert st(raw=raw, npred=1) == bad
    assert st(tables=arr(p["ts"].h, tc.h)) == bad and st(tables=arr(tc.h, None), preds=[]) == bad  # a chaining table
    assert st(b=explicit) == bad and st(b=explicit, preds=[]) == bad
    assert st(builds=rels(hj3d.Rel(p["S"], key_word=1), hj3d.Rel(p["T"], key_word=1, row_word=0))) == bad
    # a predicate whose source object is missing
    assert st(b=None) == bad and st(tables=None) == bad and st(tables=arr(None, p["tt"].h)) == bad
    assert st(builds=None) == bad and st(builds=rels(hj3d.Rel(p["S"], key_word=1), None)) == bad
    assert st(b=None, tables=None, builds=None, preds=[]) == hj3d.HJ3D_OK
    assert st(ptr=None) == bad
    assert st(ptr=nested.data_ptr() + 2) == bad and st(optr=out.data_ptr() + 2) == bad
    assert st(flags=0, optr=out.data_ptr() + 1, cap=0) == bad
    assert st(optr=None) == bad and st(optr=None, cap=0) == hj3d.HJ3D_OK
    assert st(n=1 << 32) == bad
    # a valid call on the same context, and the empty input
    want = SN.select_nested(x["h"][:64], good_preds, base=x["R"], mains=[x["ms"], x["mt"]], builds=[x["S"], x["T"]])
    assert st(flags=E | hj3d.PROBE_CHECKSUM) == hj3d.HJ3D_OK
    assert fields(ctx.probe_result()) == SN.counters(want)
    assert st(ptr=None, n=0, optr=None, cap=0) == hj3d.HJ3D_OK
    assert fields(ctx.probe_result()) == (0,) * 9
    with pytest.raises(ValueError):
        ctx.select_nested(dev(np.zeros((4, 8), np.uint32)), [])
    with pytest.raises(ValueError):
        ctx.select_nested(nested, [], tables=[p["ts"]])
    with pytest.raises(ValueError):
        ctx.select_nested(nested, [("base", 1, "<", 300)] * 5, base=base)
    tc.close()


# ---- 9. the plan hook ----
PLAN = "exp4_R10_a3_A2_b2_B3"


def plan_relations():
    g = EXP4[PLAN]
    log2R, a, A, b, B = g["generator_args"][1:6]
    Sa, Ta = O.gen_exp4(log2R, a, A, b, B)
    n, cardR = len(Sa), 1 << log2R
    R = O.tuples2(np.arange(cardR, dtype=np.uint32), np.zeros(cardR, np.uint32))
    return g, R, O.tuples2(np.arange(n, dtype=np.uint32), Sa), O.tuples2(np.arange(n, dtype=np.uint32), Ta)


@pytest.mark.parametrize("thr", [2, 3])  # (every tuple that reaches level 1 has a T group of 2 rows: all pass, none pass)
def test_plan_with_filters(ctx, thr):
    import hj3d
    g, R, S, T = plan_relations()
    gs, gt = X.group_index(S[:, 1]), X.group_index(T[:, 1])
    k = R[:, 0].astype(np.int64)
    in_s, size_t = gs.locate(k)[1] > 0, gt.locate(k)[1]
    lvl0 = in_s & (k >= 100) & (k < 700)           # the R-word range, behind the S probe
    lvl1 = lvl0 & (size_t >= thr)                  # COUNT >= thr on the T group, behind the T probe
    assert 0 < (lvl0 & (size_t > 0)).sum() < lvl0.sum() < in_s.sum()
    assert lvl1.sum() == ((lvl0 & (size_t > 0)).sum() if thr == 2 else 0)
    keys = [[int(v) if ok else None for v, ok in zip(k, lvl1)]] * 2
    a = np.arange(len(R), dtype=np.uint32)
    c, cs = XN.counters(keys, [gs, gt]), XN.row_checksums(XN.expand_rows(a, keys, [gs, gt]))
    want = XN.sort_rows(XN.expand_rows(a, keys, [gs, gt]))
    buf = canary_buffer(c["c_top"], 3)
    got = hj3d.star_plan_chained(ctx, dev(R), [(dev(S), 1), (dev(T), 1)], g["nb"], keys=(0, 0), out=buf[:c["c_top"]],
                                 filters={0: [("base", 0, "range", 100, 700)], 1: [("count", 2, ">=", thr)]})
    assert got["c_select"] == [int(lvl0.sum()), int(lvl1.sum())]
    assert got["c_probe"] == [int(in_s.sum()), int((lvl0 & (size_t > 0)).sum())]
    assert (got["n_in"], got["n_live"], got["c_unnest"], got["c_top"]) == (c["n_live"], c["n_live"], c["c_unnest"], c["c_top"])
    assert (got["sum_a"], got["sum_row"], got["sum_h"], got["xor_h"]) == (cs["sum_a"], cs["sum_row"], cs["sum_h"], cs["xor_h"])
    assert not got["overflow"] and tail_intact(buf, c["c_top"])
    assert np.array_equal(XN.sort_rows(host(buf[:c["c_top"]])), want)


def test_plan_with_an_always_true_filter_equals_the_reference(ctx):
    import hj3d
    g, R, S, T = plan_relations()
    ref = g["plans"]["Ndu"]
    buf = canary_buffer(ref["c_top"], 3)
    true = {0: [("base", 0, ">=", 0), ("count", 1, ">=", 1)], 1: [("count", 2, ">=", 1), ("first", 1, 0, ">=", 0)]}
    got = hj3d.star_plan_chained(ctx, dev(R), [(dev(S), 1), (dev(T), 1)], g["nb"], keys=(0, 0), out=buf[:ref["c_top"]],
                                 filters=true)
    plain = hj3d.star_plan_chained(ctx, dev(R), [(dev(S), 1), (dev(T), 1)], g["nb"], keys=(0, 0))
    assert "c_select" not in plain and {k: v for k, v in got.items() if k != "c_select"} == plain
    assert got["c_select"] == [ref["c_probe_RS"], ref["c_probe_RT"]]
    seven = (got["c_probe"][0], got["c_probe_cmp"][0], got["c_probe"][1], got["c_probe_cmp"][1], got["c_unnest"][0],
             got["c_unnest"][1], got["c_top"])
    assert seven == (ref["c_probe_RS"], ref["c_probe_RS_cmp"], ref["c_probe_RT"], ref["c_probe_RT_cmp"], ref["c_unnest_1"],
                     ref["c_unnest_2"], ref["c_top"])
    out = ref["out"]
    assert (got["sum_a"], got["sum_row"], got["sum_h"], got["xor_h"]) == \
        (out["sum_a"], [out["sum_b"], out["sum_c"]], out["sum_h"], out["xor_h"])
    assert tail_intact(buf, ref["c_top"])
    assert hj3d.triple_checksums(host(buf[:ref["c_top"]])) == {k: out[k] for k in ("n", "sum_a", "sum_b", "sum_c", "sum_h", "xor_h")}
