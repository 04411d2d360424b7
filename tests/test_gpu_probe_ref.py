"""hj3d_probe_ref on the GPU: the chained nested probe (AlgNestJoinProbe over another nested probe's
output, main_experiment4.cc:847-850). Stored nested tuples {a} / {a, ref} probe a further nested table
with a key fetched from the probe-side base relation; the survivors come out with one more ref.

Expected values: the reference binary's experiment-4 fixtures (plan Ndu: the second probe sees only
the first one's survivors), the oracle's nested probe over explicit-row pairs {key, a} of the live
tuples, and numpy models over what Table.export() returns. Integer work: every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from test_gpu_unnest import (CANARY, EXP1, EXP4, EXP4_NAMES, NOREF, PATHS, dev, exp1_rel, group_index, host,
                             is_sub_multiset, on_path, res_out, rowsort)

pytestmark = pytest.mark.gpu

SUMS = ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")
ZERO_OUT = {"n": 0, "sum_a": 0, "sum_b": 0, "sum_c": 0, "sum_h": 0, "xor_h": 0}


def murmur32(x: np.ndarray) -> np.ndarray:
    m = np.uint64(0xFFFFFFFF)
    x = x.astype(np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85ebca6b)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xc2b2ae35)) & m
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def live_mask(nested: np.ndarray, n_base: int, row_base: int = 0) -> np.ndarray:
    idx = nested[:, 0].astype(np.int64) - row_base
    live = (idx >= 0) & (idx < n_base)
    if nested.shape[1] == 2:
        live &= nested[:, 1] != NOREF
    return live


def np_probe_ref(nested: np.ndarray, base_keys: np.ndarray, payload: np.ndarray, row_base: int = 0) -> np.ndarray:
    """The operator on the host: every live tuple whose key has a main record in `payload` (a table's
    exported main records {hash, first row, sub_off, sub_len}), with that record's index appended."""
    live = live_mask(nested, len(base_keys), row_base)
    t = nested[live]
    h = murmur32(base_keys[t[:, 0].astype(np.int64) - row_base])
    if len(payload) == 0:
        return np.zeros((0, nested.shape[1] + 1), np.uint32)
    order = np.argsort(payload[:, 0], kind="stable")
    hs = payload[order, 0]
    pos = np.minimum(np.searchsorted(hs, h), len(hs) - 1)
    hit = hs[pos] == h
    return np.concatenate([t[hit], order[pos[hit]].astype(np.uint32)[:, None]], axis=1).astype(np.uint32)


def oracle_probe(build: np.ndarray, bkey: int, nb: int, nested: np.ndarray, base_keys: np.ndarray, row_base: int = 0):
    """(live tuples, matches, comparisons, checksums) of the nested probe (no unnest) over the
    explicit-row pairs {key, a} of the live tuples: what hj3d_probe_ref must report."""
    live = live_mask(nested, len(base_keys), row_base)
    a = nested[live, 0]
    if len(a) == 0:
        return 0, 0, 0, dict(ZERO_OUT)
    pairs = np.stack([base_keys[a.astype(np.int64) - row_base], a], axis=1).astype(np.uint32)
    e = O.nested_plan(build, bkey, pairs, 0, nb, False, prow=1)
    return len(a), e.c_probe, e.c_cmp, e.out


def assert_result(r, want, checksum=True):
    n_live, matched, cmps, out = want
    assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps) == (n_live, matched, matched, cmps)
    assert r.sum_a == out["sum_a"] and r.sum_c == 0
    if checksum:
        assert res_out(r) == out
    else:
        assert (r.sum_b, r.sum_h, r.xor_h) == (0, 0, 0)


def run(ctx, t, base, nested, cap=None, checksum=True, pad=8):
    """probe_ref into a canary-filled buffer of `cap` tuples (default: one per input tuple) plus `pad`
    guard tuples: (result, written region on the host, guard region on the host)."""
    import torch
    n, w = nested.shape
    cap = n if cap is None else cap
    buf = torch.full((cap + pad, w + 1), CANARY, dtype=torch.int32, device="cuda")
    r = ctx.probe_ref(t, base, nested, out=buf[:cap], checksum=checksum)
    h = host(buf)
    return r, h[:cap], h[cap:]


@pytest.fixture(scope="module")
def zipf():
    """Fixture exp1_R1024_S4096_zipf: the nested table goes on S.a, R is the base relation."""
    name = "exp1_R1024_S4096_zipf"
    R, S, nb = exp1_rel(name)
    return R, S, nb


def zipf_table(ctx, zipf, finish=True):
    import hj3d
    R, S, nb = zipf
    dS = dev(S)
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    t.build(hj3d.Rel(dS, key_word=1))
    if finish:
        t.finish()
    return t, dS


# ---- 1. the reference's experiment 4, operator by operator ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", EXP4_NAMES)
def test_chained_strand_equals_reference_exp4(ctx, name, path):
    import torch
    import hj3d
    g = EXP4[name]
    ref = g["plans"]["Ndu"]
    log2R, a, A, b, B = g["generator_args"][1:6]
    Sa, Ta = O.gen_exp4(log2R, a, A, b, B)
    n, cardR = len(Sa), 1 << log2R
    R = dev(O.tuples2(np.arange(cardR, dtype=np.uint32), np.zeros(cardR, np.uint32)))
    S = dev(O.tuples2(np.arange(n, dtype=np.uint32), Sa))
    T = dev(O.tuples2(np.arange(n, dtype=np.uint32), Ta))
    ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, g["nb"]), hj3d.Table(ctx, hj3d.HJ3D_NESTED, g["nb"])
    ctx.build_many([ts, tt], [hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)])
    base = hj3d.Rel(R, key_word=0)
    c_top = ref["c_top"]
    with on_path(ctx, path):
        pairs = torch.zeros((cardR, 2), dtype=torch.int32, device="cuda")
        rs = ctx.probe(ts, base, out=pairs, mainref=True)
        # the first probe's dense output as it stands, 0xFFFFFFFF refs included
        trip = torch.full((ref["c_probe_RS"] + 8, 3), CANARY, dtype=torch.int32, device="cuda")
        rt = ctx.probe_ref(tt, base, pairs, out=trip[: ref["c_probe_RS"]])
        out = torch.full((c_top + 8, 3), CANARY, dtype=torch.int32, device="cuda")
        got = ctx.unnest2(ts, tt, trip[: rt.n_out], out=out[:c_top])
        plan = hj3d.exp4_plan_chained(ctx, R, S, T, g["nb"])
    assert (rs.n_matched, rs.n_cmps) == (ref["c_probe_RS"], ref["c_probe_RS_cmp"])
    assert not rt.overflow
    assert (rt.n_probe, rt.n_matched, rt.n_out, rt.n_cmps) == \
        (ref["c_probe_RS"], ref["c_probe_RT"], ref["c_probe_RT"], ref["c_probe_RT_cmp"])
    assert (host(trip)[rt.n_out:] == CANARY).all()
    assert not got["overflow"]
    for k in ("c_unnest_1", "c_unnest_2", "c_top"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert {k: got[k] for k in SUMS} == {k: ref["out"][k] for k in SUMS}
    h = host(out)
    assert hj3d.triple_checksums(h[:c_top]) == {k: ref["out"][k] for k in ("n",) + SUMS}
    assert (h[c_top:] == CANARY).all()
    # the plan: all seven counters of the fixture and the checksums in one dict
    want = {"c_probe_rs": ref["c_probe_RS"], "c_probe_rs_cmp": ref["c_probe_RS_cmp"], "c_probe_rt": ref["c_probe_RT"],
            "c_probe_rt_cmp": ref["c_probe_RT_cmp"], "c_unnest_1": ref["c_unnest_1"], "c_unnest_2": ref["c_unnest_2"],
            "c_top": ref["c_top"], "overflow": False, **{k: ref["out"][k] for k in SUMS}}
    assert plan == want


# ---- 2. what probe2 cannot do: two probe attributes, two geometries, no host glue ----
@pytest.fixture(scope="module")
def two_attr():
    """test_unnest2_two_attributes' data and its numpy triple join."""
    rng = np.random.default_rng(23)
    nR, nS, nT, dom = 5000, 20000, 20000, 2500
    x = rng.integers(0, dom + 100, nR).astype(np.uint32)  # some R tuples find no partner
    y = rng.integers(0, dom + 100, nR).astype(np.uint32)
    Sa = rng.integers(0, dom, nS).astype(np.uint32)
    Ta = rng.integers(0, dom, nT).astype(np.uint32)
    Sa[Sa == 11] = 12
    Ta[Ta == 23] = 24
    Sa[rng.choice(nS, 300, replace=False)] = 11  # one pair of groups of 300 x 400 rows
    Ta[rng.choice(nT, 400, replace=False)] = 23
    x[0], y[0] = 11, 23
    oS, fS, cS = group_index(Sa, dom + 100)
    oT, fT, cT = group_index(Ta, dom + 100)
    prod = cS[x] * cT[y]
    assert prod[0] == 300 * 400
    total = int(prod.sum())
    rr = np.repeat(np.arange(nR, dtype=np.int64), prod)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(prod) - prod, prod)
    ws = cS[x][rr]
    want = np.stack([rr, oS[fS[x][rr] + within % ws], oT[fT[y][rr] + within // ws]], axis=1).astype(np.uint32)
    R = O.tuples3(x, y)
    S = O.tuples3(np.arange(nS, dtype=np.uint32), Sa)
    T = O.tuples3(np.arange(nT, dtype=np.uint32), Ta)
    survivors = np.nonzero(cS[x] > 0)[0].astype(np.uint32)
    assert 0 < len(survivors) < nR
    return R, S, T, rowsort(want), survivors


@pytest.mark.parametrize("checksum", [True, False])
@pytest.mark.parametrize("path", ["direct", "partitioned"])
def test_two_attributes_two_geometries(ctx, two_attr, path, checksum):
    import torch
    import hj3d
    R, S, T, want, survivors = two_attr
    nR = len(R)
    dR, dS, dT = dev(R), dev(S), dev(T)
    ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, 2500), hj3d.Table(ctx, hj3d.HJ3D_NESTED, 1237)
    ts.build(hj3d.Rel(dS, key_word=1))
    tt.build(hj3d.Rel(dT, key_word=1))
    with on_path(ctx, path):
        pairs = torch.zeros((nR, 2), dtype=torch.int32, device="cuda")
        rs = ctx.probe(ts, hj3d.Rel(dR, key_word=0), out=pairs, mainref=True)
        trip = torch.zeros((rs.n_matched, 3), dtype=torch.int32, device="cuda")
        rt = ctx.probe_ref(tt, hj3d.Rel(dR, key_word=1), pairs, out=trip, checksum=checksum)
        out = torch.zeros((len(want), 3), dtype=torch.int32, device="cuda")
        got = ctx.unnest2(ts, tt, trip[: rt.n_out], out=out)
    assert rs.n_matched == len(survivors) and not rt.overflow
    # the oracle's nested probe of T over the survivors of the first join (explicit rows, no unnest)
    stored = np.stack([survivors, np.zeros_like(survivors)], axis=1)
    assert_result(rt, oracle_probe(T, 1, 1237, stored, R[:, 1]), checksum)
    assert not got["overflow"] and got["c_top"] == len(want)
    assert (rowsort(host(out)) == want).all()
    plan = hj3d.exp4_plan_chained(ctx, dR, dS, dT, (2500, 1237), keys=(0, 1), checksum=False)
    assert (plan["c_probe_rs"], plan["c_probe_rs_cmp"]) == (rs.n_matched, rs.n_cmps)
    assert (plan["c_probe_rt"], plan["c_probe_rt_cmp"]) == (rt.n_matched, rt.n_cmps)
    assert (plan["c_top"], plan["sum_a"], plan["sum_b"], plan["sum_c"]) == (got["c_top"], got["sum_a"], got["sum_b"], got["sum_c"])


# ---- 3. a tuple is its position in the input, not its row ----
@pytest.mark.parametrize("path", ["direct", "partitioned"])
def test_identity_by_position(ctx, two_attr, path):
    import torch
    import hj3d
    R, S, T, _, _ = two_attr
    nR = len(R)
    dR, dS, dT = dev(R), dev(S), dev(T)
    ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, 2500), hj3d.Table(ctx, hj3d.HJ3D_NESTED, 1237)
    ts.build(hj3d.Rel(dS, key_word=1))
    tt.build(hj3d.Rel(dT, key_word=1))
    # two first-probe outputs of the same rows, by R.x and by R.y: every a twice, with different refs
    p1 = torch.zeros((nR, 2), dtype=torch.int32, device="cuda")
    p2 = torch.zeros((nR, 2), dtype=torch.int32, device="cuda")
    ctx.probe(ts, hj3d.Rel(dR, key_word=0), out=p1, mainref=True)
    ctx.probe(ts, hj3d.Rel(dR, key_word=1), out=p2, mainref=True)
    both = np.concatenate([host(p1), host(p2)])
    both = both[np.random.default_rng(3).permutation(len(both))]
    live = both[both[:, 1] != NOREF]
    refs_of = {}
    for a, r in live:
        refs_of.setdefault(int(a), set()).add(int(r))
    assert sum(len(v) == 2 for v in refs_of.values()) > 100  # the same a with two different refs
    with on_path(ctx, path):
        r, written, guard = run(ctx, tt, hj3d.Rel(dR, key_word=1), dev(both))
    _, payload, _ = tt.export()
    want = np_probe_ref(both, R[:, 1], payload)
    assert r.n_probe == len(live) and r.n_out == len(want) and not r.overflow
    assert (rowsort(written[: r.n_out]) == rowsort(want)).all()
    assert (written[r.n_out:] == CANARY).all() and (guard == CANARY).all()
    assert_result(r, oracle_probe(T, 1, 1237, both, R[:, 1]))


# ---- 4. in_words == 1: a row list, then hj3d_unnest ----
@pytest.mark.parametrize("case", ["permutation", "repeats", "row_base"])
def test_row_list_then_unnest(ctx, zipf, case):
    import torch
    import hj3d
    R, S, nb = zipf
    nR = len(R)
    t, dS = zipf_table(ctx, zipf)
    rng = np.random.default_rng(11)
    row_base = 1000 if case == "row_base" else 0
    idx = rng.permutation(nR) if case != "repeats" else rng.integers(0, nR // 3, 700)
    rows = (idx + row_base).astype(np.uint32)
    dR = dev(R)
    # the same rows as an explicit-row relation {key, row}: probe + fused unnest
    explicit = dev(np.stack([R[idx, 0], rows], axis=1).astype(np.uint32))
    fused = ctx.probe(t, hj3d.Rel(explicit, key_word=0, row_word=1), unnest=True)
    r, written, guard = run(ctx, t, hj3d.Rel(dR, key_word=0, row_base=row_base), dev(rows[:, None]))
    assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps) == (len(rows), fused.n_matched, fused.n_matched, fused.n_cmps)
    assert (guard == CANARY).all() and (written[r.n_out:] == CANARY).all()
    assert_result(r, oracle_probe(S, 1, nb, rows[:, None], R[:, 0], row_base))
    _, payload, _ = t.export()
    assert (rowsort(written[: r.n_out]) == rowsort(np_probe_ref(rows[:, None], R[:, 0], payload, row_base))).all()
    out = torch.zeros((max(fused.n_out, 1), 2), dtype=torch.int32, device="cuda")
    u = ctx.unnest(t, dev(written[: r.n_out]), out=out)
    assert not u.overflow and u.n_matched == fused.n_matched
    assert res_out(u) == res_out(fused)


# ---- 5. sizes: the wave tail, the empty wave, the cursor's workgroup boundary ----
@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4097])
def test_sizes(ctx, zipf, n, path):
    import hj3d
    R, S, nb = zipf
    nR = len(R)
    t, dS = zipf_table(ctx, zipf)
    _, payload, _ = t.export()
    base = hj3d.Rel(dev(R), key_word=0)
    rng = np.random.default_rng(100 + n)
    nested = np.stack([rng.integers(0, nR, n), rng.integers(0, 1 << 31, n)], axis=1).astype(np.uint32)
    variants = [nested]
    if n:
        dead = nested.copy()
        dead[:, 1] = NOREF  # all dead
        one = dead.copy()
        one[n // 2] = (int(np.nonzero(np.isin(R[:, 0], S[:, 1]))[0][0]), 7)  # a single live tuple, with a match
        variants += [dead, one]
    with on_path(ctx, path):
        for v in variants:
            r, written, guard = run(ctx, t, base, dev(v))
            want = np_probe_ref(v, R[:, 0], payload)
            assert_result(r, oracle_probe(S, 1, nb, v, R[:, 0]))
            assert r.n_out == len(want) and not r.overflow
            assert (rowsort(written[: r.n_out]) == rowsort(want)).all()
            assert (written[r.n_out:] == CANARY).all() and (guard == CANARY).all()
    if n:
        assert len(np_probe_ref(variants[2], R[:, 0], payload)) == 1 and len(np_probe_ref(variants[1], R[:, 0], payload)) == 0


# ---- 6. dead tuples change nothing ----
@pytest.mark.parametrize("path", ["direct", "partitioned"])
def test_dead_tuples_are_skipped(ctx, zipf, path):
    import hj3d
    R, S, nb = zipf
    nR = len(R)
    t, dS = zipf_table(ctx, zipf)
    row_base = 5
    base = hj3d.Rel(dev(R), key_word=0, row_base=row_base)
    rng = np.random.default_rng(5)
    clean = np.stack([rng.integers(0, nR, 900) + row_base, rng.integers(0, 1000, 900)], axis=1).astype(np.uint32)
    outside = np.array([row_base - 1, row_base + nR, 0xFFFFFFFF, 0, row_base + nR + 12345], dtype=np.uint32)
    dead = np.stack([np.repeat(outside, 40), np.arange(200, dtype=np.uint32)], axis=1)
    noref = np.stack([rng.integers(0, nR, 100) + row_base, np.full(100, NOREF)], axis=1).astype(np.uint32)
    mixed = np.concatenate([clean, dead, noref])
    mixed = mixed[rng.permutation(len(mixed))]
    with on_path(ctx, path):
        r_clean, w_clean, _ = run(ctx, t, base, dev(clean))
        r_mixed, w_mixed, guard = run(ctx, t, base, dev(mixed))
    assert r_clean == r_mixed and r_clean.n_probe == len(clean) and 0 < r_clean.n_out < len(clean)
    assert (rowsort(w_clean[: r_clean.n_out]) == rowsort(w_mixed[: r_mixed.n_out])).all()
    assert (w_mixed[r_mixed.n_out:] == CANARY).all() and (guard == CANARY).all()
    assert_result(r_mixed, oracle_probe(S, 1, nb, mixed, R[:, 0], row_base))


# ---- 7. capacity ----
@pytest.mark.parametrize("words", [1, 2])
def test_capacity(ctx, zipf, words):
    import hj3d
    R, S, nb = zipf
    nR = len(R)
    t, dS = zipf_table(ctx, zipf)
    base = hj3d.Rel(dev(R), key_word=0)
    rng = np.random.default_rng(9)
    nested = np.stack([rng.integers(0, nR, 3000), rng.integers(0, 1000, 3000)], axis=1).astype(np.uint32)[:, :words]
    d = dev(nested)
    full, w_full, _ = run(ctx, t, base, d)
    n_out = full.n_out
    assert not full.overflow and 1 < n_out < len(nested)
    low, w_low, guard = run(ctx, t, base, d, cap=n_out - 1, pad=64)
    assert low.overflow
    assert (low.n_probe, low.n_matched, low.n_out, low.n_cmps) == (full.n_probe, full.n_matched, n_out, full.n_cmps)
    assert res_out(low) == res_out(full)
    assert (guard == CANARY).all()
    assert is_sub_multiset(w_low, w_full[:n_out])
    exact, w_exact, guard = run(ctx, t, base, d, cap=n_out)
    assert not exact.overflow and (guard == CANARY).all()
    assert (rowsort(w_exact) == rowsort(w_full[:n_out])).all()
    # without `out`: counters only
    r0 = ctx.probe_ref(t, base, d)
    assert not r0.overflow and r0 == full
    nock = ctx.probe_ref(t, base, d, checksum=False)
    assert (nock.sum_b, nock.sum_h, nock.xor_h) == (0, 0, 0)
    assert (nock.n_probe, nock.n_matched, nock.n_out, nock.n_cmps, nock.sum_a) == \
        (full.n_probe, full.n_matched, full.n_out, full.n_cmps, full.sum_a)


# ---- 8. table states ----
def test_table_states(ctx, zipf):
    import hj3d
    R, S, nb = zipf
    nR = len(R)
    rng = np.random.default_rng(13)
    nested = np.stack([rng.integers(0, nR, 2000), rng.integers(0, 1000, 2000)], axis=1).astype(np.uint32)
    d = dev(nested)
    base = hj3d.Rel(dev(R), key_word=0)
    # a nested build still pending is finished by the call
    t, dS = zipf_table(ctx, zipf, finish=False)
    assert t.build_path(finish=False).endswith("?")
    r, written, guard = run(ctx, t, base, d)
    assert not t.build_path(finish=False).endswith("?")
    assert_result(r, oracle_probe(S, 1, nb, nested, R[:, 0]))
    _, payload, _ = t.export()
    assert (rowsort(written[: r.n_out]) == rowsort(np_probe_ref(nested, R[:, 0], payload))).all()
    # a cleared table matches nothing
    t.clear()
    r, written, guard = run(ctx, t, base, d)
    assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps, r.overflow) == (len(nested), 0, 0, 0, False)
    assert res_out(r) == ZERO_OUT
    assert (written == CANARY).all() and (guard == CANARY).all()
    # rebuilt from another relation: the new content's result
    S2 = O.tuples3(np.arange(300, dtype=np.uint32), (np.arange(300, dtype=np.uint32) * 7) % 1024)
    dS2 = dev(S2)
    t.build(hj3d.Rel(dS2, key_word=1))
    r, written, guard = run(ctx, t, base, d)
    assert_result(r, oracle_probe(S2, 1, nb, nested, R[:, 0]))
    _, payload, _ = t.export()
    want = np_probe_ref(nested, R[:, 0], payload)
    assert 0 < len(want) == r.n_out
    assert (rowsort(written[: r.n_out]) == rowsort(want)).all() and (guard == CANARY).all()


# ---- 9. refusals ----
def test_refusals(ctx, zipf):
    import torch
    import hj3d
    L = hj3d.lib()
    R, S, nb = zipf
    dR = dev(R)
    tn, dS = zipf_table(ctx, zipf)
    tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, nb)
    tc.build(hj3d.Rel(dS, key_word=1))
    base = hj3d.Rel(dR, key_word=0)
    nested = dev(np.stack([np.arange(16), np.arange(16)], axis=1).astype(np.uint32))
    out = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
    E = hj3d.PROBE_EMIT

    def st(c=ctx.h, t=tn.h, b=base, ptr=nested.data_ptr(), n=16, words=2, flags=E, optr=out.data_ptr(), cap=16):
        return L.hj3d_probe_ref(c, t, C.byref(b.c) if b is not None else None, ptr, n, words, flags, optr, cap)

    bad = hj3d.HJ3D_EINVAL
    assert st(c=None) == bad and st(t=None) == bad and st(b=None) == bad
    assert st(t=tc.h) == bad
    assert st(words=0) == bad and st(words=3) == bad
    for f in (hj3d.PROBE_UNIQUE, hj3d.PROBE_UNNEST, hj3d.PROBE_ACCUMULATE, hj3d.PROBE_MAINREF, 0x40):
        assert st(flags=E | f) == bad
    assert st(optr=None) == bad
    assert st(ptr=nested.data_ptr() + 2) == bad and st(optr=out.data_ptr() + 2) == bad
    assert st(flags=0, optr=out.data_ptr() + 1, cap=0) == bad
    assert st(ptr=None) == bad
    assert st(n=1 << 32) == bad
    explicit = hj3d.Rel(dR, key_word=0, row_word=1)
    assert st(b=explicit) == bad
    broken = hj3d.Rel(dR, key_word=0)
    broken.c.stride = 0
    assert st(b=broken) == bad
    broken.c.stride, broken.c.key_off = 12, 12
    assert st(b=broken) == bad
    broken.c.key_off, broken.c.row_base = 0, (1 << 32) - 5
    assert st(b=broken) == bad
    # a valid call on the same context
    assert st(flags=E | hj3d.PROBE_CHECKSUM) == hj3d.HJ3D_OK
    r = ctx.probe_result()
    assert_result(r, oracle_probe(S, 1, nb, host(nested), R[:, 0]))
    assert st() == hj3d.HJ3D_OK  # (without HJ3D_PROBE_CHECKSUM: the row sum only)
    assert_result(ctx.probe_result(), oracle_probe(S, 1, nb, host(nested), R[:, 0]), checksum=False)
    assert st(ptr=None, n=0, optr=None, cap=0) == hj3d.HJ3D_OK
    r = ctx.probe_result()
    assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps, r.overflow) == (0, 0, 0, 0, False)
