"""Wide nested tuples on the GPU: hj3d_probe_refn (the chained nested probe over tuples of 1..6 words),
hj3d_unnestn (k stacked unnests over {a, ref_1 .. ref_k}, k <= HJ3D_NEST_MAX) and the k-way star plan
built from them (probe -> probe_refn x (k - 1) -> unnestn).

Expected values: the existing operators on the same input (k = 1, 2), the reference binary's
experiment-4 fixtures (plan Ndu), tests/expand_n_ref.py (numpy over the build key columns and the
tuples' keys; pinned by tests/test_expand_n_ref.py) and hj3d_probe over the survivors' keys for the
per-level comparison counts. The one library result used as an input is the key -> main ref
translation (test_gpu_expand_limits.key_refs). Integer work: every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import expand_n_ref as XN
import expand_ref as X
import oracle as O
from test_gpu_expand_limits import canary_buffer, key_refs, nested_table, refs_of, scattered, tail_intact
from test_gpu_unnest import CANARY, EXP4, NOREF, PATHS, dev, host, on_path

pytestmark = pytest.mark.gpu

# the constants of k_unn_expand's walk, nested_tuple.hpp (a change there must fail the branch assertions below, not empty the cases)
CHUNK = 2048        # kChunk: outputs per workgroup and step
CHUNK_SLOTS = 2048  # kChunkSlots: slot offsets of a chunk staged in LDS


def wide_input(a, keys, refmaps, n_mains):
    """{a, ref_1 .. ref_k} on the device for per-tuple keys (None: that ref is invalid)."""
    cols = [np.asarray(a, dtype=np.uint32)] + [refs_of(k, m, nm) for k, m, nm in zip(keys, refmaps, n_mains)]
    return dev(np.stack(cols, axis=1))


def expect(a, keys, cols):
    """(counters, checksums, sorted rows) of the numpy reference."""
    rows = XN.expand_rows(a, keys, cols)
    return XN.counters(keys, cols), XN.row_checksums(rows), XN.sort_rows(rows)


def assert_counters(got, c, cs, checksum=True):
    assert (got["n_in"], got["n_live"], got["c_unnest"], got["c_top"]) == (c["n_in"], c["n_live"], c["c_unnest"], c["c_top"])
    assert (got["sum_a"], got["sum_row"]) == (cs["sum_a"], cs["sum_row"])
    assert (got["sum_h"], got["xor_h"]) == ((cs["sum_h"], cs["xor_h"]) if checksum else (0, 0))


def run_emit(ctx, tables, nested, cap, checksum=True):
    buf = canary_buffer(cap, len(tables) + 1)
    got = ctx.unnestn(tables, nested, out=buf[:cap], checksum=checksum)
    assert tail_intact(buf, cap)
    return got, host(buf[:cap])


# ---- 1. parity with the existing operators (Zipf 1.0, |build| = 4096, n = 4097) ----
@pytest.fixture(scope="module")
def parity(ctx):
    import torch
    import hj3d
    Rk, Sa, _ = O.gen_exp1(4097, 4096, True, 1.0, 0)
    rng = np.random.default_rng(31)
    Ta = rng.permutation(Sa)
    y = Sa[rng.integers(0, len(Sa), len(Rk))].astype(np.uint32)  # R's second attribute: keys of T (Zipf as well)
    y[::17] = 5000  # some without a partner
    R, S, T = dev(O.tuples3(Rk, y)), dev(O.tuples2(np.arange(4096, dtype=np.uint32), Sa)), \
        dev(O.tuples2(np.arange(4096, dtype=np.uint32), Ta))
    ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, O.num_distinct(Sa)), hj3d.Table(ctx, hj3d.HJ3D_NESTED, 701)
    ts.build(hj3d.Rel(S, key_word=1))
    tt.build(hj3d.Rel(T, key_word=1))
    pairs = torch.zeros((4097, 2), dtype=torch.int32, device="cuda")
    rs = ctx.probe(ts, hj3d.Rel(R, key_word=0), out=pairs, mainref=True)
    assert 0 < rs.n_matched < 4097
    return {"R": R, "S": S, "T": T, "ts": ts, "tt": tt, "pairs": pairs}


def test_parity_k1(ctx, parity):
    import torch
    p = parity
    old = ctx.unnest(p["ts"], p["pairs"])
    out_old = torch.zeros((old.n_out, 2), dtype=torch.int32, device="cuda")
    old = ctx.unnest(p["ts"], p["pairs"], out=out_old)
    new, rows = run_emit(ctx, [p["ts"]], p["pairs"], old.n_out)
    assert not new["overflow"] and old.n_out > old.n_matched > 0
    assert (new["n_in"], new["n_live"], new["c_unnest"], new["c_top"]) == (4097, old.n_matched, [old.n_out], old.n_out)
    assert (new["sum_a"], new["sum_row"], new["sum_h"], new["xor_h"]) == (old.sum_a, [old.sum_b], old.sum_h, old.xor_h)
    assert np.array_equal(XN.sort_rows(rows), XN.sort_rows(host(out_old)))


@pytest.mark.parametrize("words", [1, 2])
def test_parity_probe_refn(ctx, parity, words):
    import torch
    import hj3d
    p = parity
    base = hj3d.Rel(p["R"], key_word=1)
    nested = p["pairs"][:, :words].contiguous()
    a = torch.full((4097 + 8, words + 1), CANARY, dtype=torch.int32, device="cuda")
    b = torch.full((4097 + 8, words + 1), CANARY, dtype=torch.int32, device="cuda")
    for checksum in (True, False):
        old = ctx.probe_ref(p["tt"], base, nested, out=a[:4097], checksum=checksum)
        new = ctx.probe_refn(p["tt"], base, nested, out=b[:4097], checksum=checksum)
        assert old == new and 0 < old.n_out < 4097 and not new.overflow
        assert np.array_equal(XN.sort_rows(host(a[:old.n_out])), XN.sort_rows(host(b[:new.n_out])))
        assert (host(b[new.n_out:]) == CANARY).all()
    assert ctx.probe_refn(p["tt"], base, nested) == ctx.probe_ref(p["tt"], base, nested)


def test_parity_k2(ctx, parity):
    import torch
    import hj3d
    p = parity
    trip = torch.zeros((4097, 3), dtype=torch.int32, device="cuda")
    rt = ctx.probe_refn(p["tt"], hj3d.Rel(p["R"], key_word=1), p["pairs"], out=trip)
    trip = trip[:rt.n_out]
    # the dense first-probe output's dead tuples were dropped by the probe; put some dead triples back
    h = host(trip).copy()
    h[::50, 1] = NOREF
    h[7::50, 2] = NOREF
    trip = dev(h)
    old = ctx.unnest2(p["ts"], p["tt"], trip)
    out_old = torch.zeros((old["c_top"], 3), dtype=torch.int32, device="cuda")
    old = ctx.unnest2(p["ts"], p["tt"], trip, out=out_old)
    new, rows = run_emit(ctx, [p["ts"], p["tt"]], trip, old["c_top"])
    assert not new["overflow"] and not old["overflow"] and old["c_top"] > len(h)
    assert (new["c_unnest"], new["c_top"]) == ([old["c_unnest_1"], old["c_unnest_2"]], old["c_top"])
    assert (new["sum_a"], new["sum_row"], new["sum_h"], new["xor_h"]) == \
        (old["sum_a"], [old["sum_b"], old["sum_c"]], old["sum_h"], old["xor_h"])
    assert new["n_in"] == len(h) and 0 < new["n_live"] < len(h)
    assert np.array_equal(XN.sort_rows(rows), XN.sort_rows(host(out_old)))
    nock = ctx.unnestn([p["ts"], p["tt"]], trip, checksum=False)
    assert (nock["sum_h"], nock["xor_h"], nock["sum_row"], nock["c_top"]) == (0, 0, new["sum_row"], new["c_top"])


# ---- 2. the reference's experiment 4 through the wide entry points ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["exp4_R10_a3_A2_b2_B3", "exp4_R16_a3_A4_b2_B2"])
def test_star_plan_equals_reference_exp4(ctx, name, path):
    import hj3d
    g = EXP4[name]
    ref = g["plans"]["Ndu"]
    log2R, a, A, b, B = g["generator_args"][1:6]
    Sa, Ta = O.gen_exp4(log2R, a, A, b, B)
    n, cardR = len(Sa), 1 << log2R
    R = dev(O.tuples2(np.arange(cardR, dtype=np.uint32), np.zeros(cardR, np.uint32)))
    S = dev(O.tuples2(np.arange(n, dtype=np.uint32), Sa))
    T = dev(O.tuples2(np.arange(n, dtype=np.uint32), Ta))
    buf = canary_buffer(ref["c_top"], 3)
    with on_path(ctx, path):
        got = hj3d.star_plan_chained(ctx, R, [(S, 1), (T, 1)], g["nb"], keys=(0, 0), out=buf[:ref["c_top"]])
    assert got["c_probe"] == [ref["c_probe_RS"], ref["c_probe_RT"]]
    assert got["c_probe_cmp"] == [ref["c_probe_RS_cmp"], ref["c_probe_RT_cmp"]]
    assert got["c_unnest"] == [ref["c_unnest_1"], ref["c_unnest_2"]] and got["c_top"] == ref["c_top"]
    assert not got["overflow"] and got["n_in"] == got["n_live"] == ref["c_probe_RT"]
    out = ref["out"]
    assert (got["sum_a"], got["sum_row"], got["sum_h"], got["xor_h"]) == \
        (out["sum_a"], [out["sum_b"], out["sum_c"]], out["sum_h"], out["xor_h"])
    assert tail_intact(buf, ref["c_top"])
    assert hj3d.triple_checksums(host(buf[:ref["c_top"]])) == {k: out[k] for k in ("n", "sum_a", "sum_b", "sum_c", "sum_h", "xor_h")}


# ---- 3. k = 3, 4, 6 against the numpy helper ----
STAR_NB = (509, 64, 1237, 300)  # the four builds' bucket counts
STAR = {3: ((0, 1, 2), (0, 1, 2)), 4: ((0, 1, 2, 1), (0, 1, 2, 3)), 6: ((0, 1, 2, 1, 3, 0), (0, 1, 2, 3, 1, 2))}


@pytest.fixture(scope="module")
def star():
    """R with four key words over one key domain and four builds of different sizes; some R keys and
    some domain values have no build row."""
    rng = np.random.default_rng(47)
    dom = 400
    sizes = (1600, 800, 2400, 600)
    cols = []
    for i, m in enumerate(sizes):
        c = rng.integers(0, dom, m).astype(np.uint32)
        c[c % 13 == i] = (c[c % 13 == i] + 1) % dom  # every build lacks some keys
        cols.append(c)
    R = rng.integers(0, dom + 20, (60_000, 4)).astype(np.uint32)
    return R, cols


@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k", [3, 4, 6])
def test_star_against_numpy(ctx, star, k, path):
    import hj3d
    Rall, cols = star
    which, words = STAR[k]
    groups = [X.group_index(c) for c in cols]
    # the prefix of R whose result has about 1e6 rows
    prod = np.ones(len(Rall), dtype=np.int64)
    for b, w in zip(which, words):
        prod *= groups[b].locate(Rall[:, w].astype(np.int64))[1]
    n = int(np.searchsorted(np.cumsum(prod), 1_000_000)) + 1
    assert 64 < n <= len(Rall)
    Rh = Rall[:n]
    a = np.arange(n, dtype=np.uint32)
    keys = [Rh[:, w].astype(np.int64) for w in words]
    c, cs, want = expect(a, keys, [groups[b] for b in which])
    assert 1_000_000 <= c["c_top"] < 2_000_000 and 0 < c["n_live"] < n
    R = dev(Rh)
    rels = [dev(O.tuples2(np.arange(len(col), dtype=np.uint32), col)) for col in cols]
    buf = canary_buffer(c["c_top"], k + 1)
    with on_path(ctx, path):
        got = hj3d.star_plan_chained(ctx, R, [(rels[b], 1) for b in which], [STAR_NB[b] for b in which], words,
                                     out=buf[:c["c_top"]])
        # per level: hj3d_probe over the survivors' keys (explicit rows), on a table of the same build
        alive = np.ones(n, dtype=bool)
        for lvl, (b, w) in enumerate(zip(which, words)):
            surv = np.nonzero(alive)[0].astype(np.uint32)
            t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, STAR_NB[b])
            t.build(hj3d.Rel(rels[b], key_word=1))
            pr = ctx.probe(t, hj3d.Rel(dev(np.stack([Rh[surv, w], surv], axis=1)), key_word=0, row_word=1))
            assert (got["c_probe"][lvl], got["c_probe_cmp"][lvl]) == (pr.n_matched, pr.n_cmps), lvl
            alive &= groups[b].locate(keys[lvl])[1] > 0
            assert pr.n_matched == int(alive.sum())
            t.close()
    assert not got["overflow"]
    c["n_in"] = c["n_live"]  # the chain hands only survivors to the unnest
    assert_counters(got, c, cs)
    assert tail_intact(buf, c["c_top"])
    assert np.array_equal(XN.sort_rows(host(buf[:c["c_top"]])), want)


# ---- 4. kernel edges ----
@pytest.fixture(scope="module")
def edge(ctx):
    """Two small tables: A with groups of 1..30 rows (keys 0..59; key 100: 2048 rows, key 101: 2 rows),
    B with groups of 1..20 rows (keys 0..39)."""
    rng = np.random.default_rng(53)
    ka, kb = np.arange(60, dtype=np.uint32), np.arange(40, dtype=np.uint32)
    Aa = scattered(rng, np.concatenate([ka, [100, 101]]), np.concatenate([1 + ka % 30, [2048, 2]]))
    Ba = scattered(rng, kb, 1 + (kb * 7) % 20)
    ga, gb = X.group_index(Aa), X.group_index(Ba)
    (ta, ra), (tb, rb) = nested_table(ctx, Aa, 37), nested_table(ctx, Ba, 64)
    return {"ga": ga, "gb": gb, "ta": ta, "tb": tb, "rels": (ra, rb), "ra": key_refs(ctx, ta, ga.keys),
            "rb": key_refs(ctx, tb, gb.keys), "n_mains": (len(ga), len(gb))}


def edge_run(ctx, e, a, ka1, kb, ka2, cap=None, checksum=True):
    """k = 3 over (A, B, A): (result, written rows, counters, checksums, sorted expected rows)."""
    nested = wide_input(a, [ka1, kb, ka2], [e["ra"], e["rb"], e["ra"]], [e["n_mains"][0], e["n_mains"][1], e["n_mains"][0]])
    c, cs, want = expect(a, [ka1, kb, ka2], [e["ga"], e["gb"], e["ga"]])
    got, rows = run_emit(ctx, [e["ta"], e["tb"], e["ta"]], nested, c["c_top"] if cap is None else cap, checksum)
    return got, rows, c, cs, want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2049])
def test_sizes(ctx, edge, n):
    rng = np.random.default_rng(200 + n)
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ka1 = [int(v) if v < 60 else None for v in rng.integers(0, 66, n)]
    kb = [int(v) if v < 40 else None for v in rng.integers(0, 44, n)]
    ka2 = [int(v) for v in rng.integers(0, 8, n)]
    got, rows, c, cs, want = edge_run(ctx, edge, a, ka1, kb, ka2)
    assert not got["overflow"]
    assert_counters(got, c, cs)
    assert np.array_equal(XN.sort_rows(rows), want)
    if n >= 63:
        assert 0 < c["n_live"] < n


def test_empty_run_inside_a_chunk_and_repeats(ctx, edge):
    """More than kChunkSlots consecutive empty slots inside one chunk (its offsets are searched in
    HBM, not staged), between live tuples that repeat one input tuple."""
    live = 100
    dead = CHUNK_SLOTS + 1000
    a = np.concatenate([np.full(live, 7), np.arange(dead), np.full(live, 7)]).astype(np.uint32)
    ka1 = [0] * live + [None] * dead + [0] * live      # |G| = 1
    kb = [0] * live + [3] * dead + [0] * live          # (B key 0: 1 row)
    ka2 = [0] * (2 * live + dead)
    got, rows, c, cs, want = edge_run(ctx, edge, a, ka1, kb, ka2)
    assert c["c_top"] == 2 * live < CHUNK and c["n_live"] == 2 * live  # one chunk, spanning every slot
    assert_counters(got, c, cs)
    assert np.array_equal(XN.sort_rows(rows), want) and len(np.unique(rows, axis=0)) == 1


def test_slot_straddles_chunks(ctx, edge):
    """One slot of 30 x 20 x 30 = 18000 outputs (nine chunks) between small ones, and dead tuples with
    an invalid ref in each position."""
    a = np.arange(1000, 1009, dtype=np.uint32)
    ka1 = [3, 29, 5, None, 7, 7, 29, 2, 1]
    kb = [4, 37, 6, 8, None, 8, 37, 2, 1]      # B key 37: 1 + 259 % 20 = 20 rows
    ka2 = [5, 59, 7, 9, 9, None, 59, 2, 1]     # A key 29 / 59: 30 rows
    assert len(edge["ga"].rows(29)) == 30 and len(edge["gb"].rows(37)) == 20 and len(edge["ga"].rows(59)) == 30
    got, rows, c, cs, want = edge_run(ctx, edge, a, ka1, kb, ka2)
    assert c["n_live"] == 6 and c["c_top"] > 2 * 18000 > 16 * CHUNK
    assert_counters(got, c, cs)
    assert np.array_equal(XN.sort_rows(rows), want)


def test_stale_refs_after_a_smaller_rebuild(ctx, edge):
    """Refs taken from a table that is then rebuilt with fewer keys: a ref at or above the new
    main-record count is skipped, one below it names the new content's group."""
    import hj3d
    rng = np.random.default_rng(59)
    old_col = scattered(rng, np.arange(200, dtype=np.uint32), np.full(200, 2))
    t, _rel = nested_table(ctx, old_col, 97)
    old_refs = key_refs(ctx, t, np.arange(200, dtype=np.uint32))
    new_col = scattered(rng, np.arange(50, dtype=np.uint32) + 1000, 1 + np.arange(50) % 5)
    new_rel = dev(O.tuples2(np.arange(len(new_col), dtype=np.uint32), new_col))
    t.build(hj3d.Rel(new_rel, key_word=1))
    t.finish()
    new_refs = key_refs(ctx, t, np.arange(50, dtype=np.uint32) + 1000)
    key_of_ref = {r: k for k, r in new_refs.items()}
    assert sorted(key_of_ref) == list(range(50))
    refs = np.array([old_refs[k] for k in range(200)], dtype=np.uint32)
    assert (refs >= 50).sum() == 150
    a = np.arange(200, dtype=np.uint32)
    keys_t = [key_of_ref.get(int(r)) for r in refs]  # None: stale
    kb = [int(v) % 40 for v in a]
    nested = dev(np.stack([a, refs, refs_of(kb, edge["rb"], edge["n_mains"][1])], axis=1))
    c, cs, want = expect(a, [keys_t, kb], [X.group_index(new_col), edge["gb"]])
    got, rows = run_emit(ctx, [t, edge["tb"]], nested, c["c_top"])
    assert c["n_live"] == 50
    assert_counters(got, c, cs)
    assert np.array_equal(XN.sort_rows(rows), want)


def test_slot_product_beyond_32_bits(ctx, edge):
    """One slot of 2048 x 2048 x 2048 x 2 = 2^34 outputs (k = 4 on table A): the index inside the slot
    passes 2^32, where the digits are split with 64-bit divisions. Without EMIT; counters and row sums
    against the analytic form (no enumeration): a wrong digit in any position moves that position's sum."""
    ga = edge["ga"]
    assert len(ga.rows(100)) == 2048 and len(ga.rows(101)) == 2
    a = np.array([0xFFFF_FF01, 0xFFFF_FF02, 0xFFFF_FF03], dtype=np.uint32)
    keys = [[7, 100, 31], [8, 100, 32], [9, 100, 33], [10, 101, 34]]
    parts = [XN.analytic_groups(a[i], [ga.rows(k[i]) for k in keys]) for i in range(3)]
    assert parts[1]["c_top"] == 1 << 34 and parts[0]["c_top"] > 0 and parts[2]["c_top"] > 0
    want = XN.add_results(*parts)
    nested = wide_input(a, keys, [edge["ra"]] * 4, [edge["n_mains"][0]] * 4)
    got = ctx.unnestn([edge["ta"]] * 4, nested, checksum=False)
    assert got["overflow"] is False and (got["sum_h"], got["xor_h"]) == (0, 0) and got["n_in"] == 3
    assert {k: got[k] for k in want} == want


# ---- 5. capacity ----
@pytest.mark.parametrize("where", ["zero", "one_short", "exact"])
def test_capacity(ctx, edge, where):
    rng = np.random.default_rng(61)
    n = 700
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ka1 = [int(v) if v < 60 else None for v in rng.integers(0, 64, n)]
    kb = [int(v) for v in rng.integers(0, 40, n)]
    ka2 = [int(v) for v in rng.integers(0, 6, n)]
    c_top = XN.counters([ka1, kb, ka2], [edge["ga"], edge["gb"], edge["ga"]])["c_top"]
    cap = {"zero": 0, "one_short": c_top - 1, "exact": c_top}[where]
    got, rows, c, cs, want = edge_run(ctx, edge, a, ka1, kb, ka2, cap=cap)  # (checks the canary rows behind cap)
    assert c_top > 50_000 and got["overflow"] is (where != "exact")
    assert_counters(got, c, cs)  # complete: every row is counted
    assert XN.is_sub_multiset(rows, want)
    if where == "exact":
        assert np.array_equal(XN.sort_rows(rows), want)


# ---- 6. magnitude: a product or a total of 2^64, in a process of its own under a time limit ----
def test_magnitude_is_refused_promptly():
    """tests/unnestn_magnitude_case.py: code without the check would wrap both totals to 0 and end
    at once with wrong counters; code that walked the products would not end. The time limit is for
    the second kind."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "unnestn_magnitude_case.py")
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "magnitude OK" in r.stdout


# ---- 7. refusals ----
def test_refusals(ctx, edge):
    import torch
    import hj3d
    L = hj3d.lib()
    e = edge
    tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, 64)
    tc.build(hj3d.Rel(e["rels"][1], key_word=1))
    a = np.arange(16, dtype=np.uint32)
    nested = wide_input(a, [[int(v) for v in a], [int(v) for v in a]], [e["ra"], e["rb"]], e["n_mains"])
    out = torch.zeros((4096, 3), dtype=torch.int32, device="cuda")
    E = hj3d.PROBE_EMIT

    def arr(*hs):
        return (C.c_void_p * len(hs))(*hs)

    def st(c=ctx.h, tables=arr(e["ta"].h, e["tb"].h), k=2, ptr=nested.data_ptr(), n=16, flags=E, optr=out.data_ptr(),
           cap=4096):
        return L.hj3d_unnestn(c, tables, k, ptr, n, flags, optr, cap)

    bad = hj3d.HJ3D_EINVAL
    assert st(c=None) == bad and st(tables=None) == bad
    assert st(tables=arr(e["ta"].h, None)) == bad and st(tables=arr(None, e["tb"].h)) == bad
    assert st(tables=arr(e["ta"].h, tc.h)) == bad
    seven = arr(*([e["ta"].h] * 7))
    assert st(k=0) == bad and st(tables=seven, k=7) == bad
    for f in (hj3d.PROBE_UNIQUE, hj3d.PROBE_UNNEST, hj3d.PROBE_ACCUMULATE, hj3d.PROBE_MAINREF, 0x40):
        assert st(flags=E | f) == bad
    assert st(ptr=None) == bad
    assert st(ptr=nested.data_ptr() + 2) == bad and st(optr=out.data_ptr() + 2) == bad
    assert st(flags=0, optr=out.data_ptr() + 1, cap=0) == bad
    assert st(optr=None) == bad
    assert st(n=1 << 32) == bad
    # a valid call on the same context, and the empty input
    c, cs, _ = expect(a, [a.astype(np.int64), a.astype(np.int64)], [e["ga"], e["gb"]])
    assert st(flags=E | hj3d.PROBE_CHECKSUM) == hj3d.HJ3D_OK
    ctx._unnestn_k = 2
    assert_counters(ctx.unnestn_result(), c, cs)
    assert st(ptr=None, n=0, optr=None, cap=0) == hj3d.HJ3D_OK
    r = ctx.unnestn_result()
    assert (r["n_in"], r["n_live"], r["c_top"], r["c_unnest"], r["overflow"]) == (0, 0, 0, [0, 0], False)
    # the chained probes: the wide one takes 1..6 words, the narrow one still 1 or 2
    base = hj3d.Rel(e["rels"][0], key_word=1)
    three = dev(np.zeros((16, 3), np.uint32))
    six = dev(np.zeros((16, 6), np.uint32))
    wide_out = torch.zeros((16, 7), dtype=torch.int32, device="cuda")

    def pr(fn, words, ptr):
        return fn(ctx.h, e["ta"].h, C.byref(base.c), ptr, 16, words, E, wide_out.data_ptr(), 16)

    assert pr(L.hj3d_probe_ref, 3, three.data_ptr()) == bad
    assert pr(L.hj3d_probe_refn, 3, three.data_ptr()) == hj3d.HJ3D_OK
    assert pr(L.hj3d_probe_refn, 6, six.data_ptr()) == hj3d.HJ3D_OK
    assert pr(L.hj3d_probe_refn, 0, six.data_ptr()) == bad and pr(L.hj3d_probe_refn, 7, six.data_ptr()) == bad
    with pytest.raises(ValueError):
        ctx.probe_refn(e["ta"], base, dev(np.zeros((4, 7), np.uint32)))
    with pytest.raises(ValueError):
        ctx.unnestn([e["ta"]] * 7, dev(np.zeros((4, 8), np.uint32)))
    tc.close()
