"""Composable deferred unnesting on the GPU: HJ3D_PROBE_MAINREF (the nested result tuple carries the
index of its main record), hj3d_unnest (AlgUnnestHt as an operator of its own over stored nested
tuples) and hj3d_unnest2 (experiment 4's two stacked unnests over {a, ref_s, ref_t} triples).

Expected values: the reference binary's fixtures (plans NrsNU / Nrs of experiment 1, Ndu of
experiment 4), the oracle, and numpy expansions of what Table.export() returns. Integer work: every
comparison is exact.
"""
import ctypes as C
import functools
from contextlib import contextmanager

import numpy as np
import pytest

import oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

NOREF = 0xFFFFFFFF
EXP1 = dict(load_golden("exp1_*.json", headline=False))
EXP4 = dict(load_golden("exp4_*.json", headline=False))
EXP1_NAMES = ("exp1_R8_S16_zipf", "exp1_R5_S3_uni_b4", "exp1_R1_S7_uni", "exp1_R1024_S4096_zipf",
              "exp1_R10007_S100003_zipf08_t1_b3")
EXP4_NAMES = ("exp4_R3_a2_A2_b2_B1", "exp4_R10_a3_A2_b2_B3", "exp4_R16_a3_A4_b2_B2")
PATHS = ("direct", "partitioned", "two_level")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


@contextmanager
def on_path(ctx, path):
    """direct: no partitioned kernels; partitioned: the LDS-slice probe from 64 tuples on;
    two_level: the same with a slice bound of 2 buckets (as test_nested_probe_two_level_slices sets
    its bound)."""
    try:
        if path == "direct":
            ctx.force_direct(True)
        elif path != "default":
            ctx.radix_min(64)
            if path == "two_level":
                ctx.pk_slice_max(2)
        yield
    finally:
        ctx.force_direct(False)
        ctx.radix_min(1 << 20)
        ctx.pk_slice_max(0)


@functools.lru_cache(maxsize=None)
def exp1_rel(name):
    g = EXP1[name]
    _, nR, nS, skew, theta, t, b = g["generator_args"][:7]
    Rk, Sa, _ = O.gen_exp1(nR, nS, bool(skew), theta, t)
    R = O.tuples3(Rk, np.zeros_like(Rk))
    S = O.tuples3(np.arange(nS, dtype=np.uint32), Sa)
    return R, S, max(g["numDvSa"] // b, 1)


def host_checksums(pairs: np.ndarray) -> dict:
    a = pairs[:, 0].astype(np.uint64)
    b = pairs[:, 1].astype(np.uint64)
    z = (a << np.uint64(32)) | b
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        z = z ^ (z >> np.uint64(31))
        return {"n": len(pairs), "sum_a": int(a.sum(dtype=np.uint64)), "sum_b": int(b.sum(dtype=np.uint64)),
                "sum_c": 0, "sum_h": int(z.sum(dtype=np.uint64)), "xor_h": int(np.bitwise_xor.reduce(z)) if len(z) else 0}


def res_out(r) -> dict:
    return {"n": r.n_out, "sum_a": r.sum_a, "sum_b": r.sum_b, "sum_c": r.sum_c, "sum_h": r.sum_h, "xor_h": r.xor_h}


def np_expand(pairs: np.ndarray, payload: np.ndarray, sub: np.ndarray):
    """AlgUnnestHt on the host: ({a, build row} pairs of every valid {a, ref}, #valid)."""
    ok = pairs[:, 1].astype(np.int64) < len(payload)
    p = pairs[ok]
    m = payload[p[:, 1].astype(np.int64)]
    lens = m[:, 3].astype(np.int64)
    first = np.cumsum(lens) - lens
    within = np.arange(int(lens.sum()), dtype=np.int64) - np.repeat(first, lens)
    rows = sub[np.repeat(m[:, 2].astype(np.int64), lens) + within]
    return np.stack([np.repeat(p[:, 0], lens), rows], axis=1).astype(np.uint32), int(ok.sum())


def keys64(pairs: np.ndarray) -> np.ndarray:
    return np.sort((pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64))


def rowsort(t: np.ndarray) -> np.ndarray:
    return t[np.lexsort(t.T[::-1])]


def is_sub_multiset(part: np.ndarray, full: np.ndarray) -> bool:
    """Every row of `part` occurs in `full` at least as often."""
    def rows(t):
        return np.ascontiguousarray(t).view([("", t.dtype)] * t.shape[1]).ravel()
    ku, cu = np.unique(rows(part), return_counts=True)
    kf, cf = np.unique(rows(full), return_counts=True)
    pos = np.minimum(np.searchsorted(kf, ku), len(kf) - 1)
    return bool((kf[pos] == ku).all() and (cu <= cf[pos]).all())


def nrs_table(ctx, name):
    """Plan Nrs / NrsNU: the nested table on S.a, and R as the probe relation."""
    import hj3d
    R, S, nb = exp1_rel(name)
    dR, dS = dev(R), dev(S)
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    t.build(hj3d.Rel(dS, key_word=1))
    t.finish()
    return t, hj3d.Rel(dR, key_word=0), len(R)


def assert_refs_match(p: np.ndarray, q: np.ndarray, payload: np.ndarray):
    """p: the plain dense output {a, first build row}, q: the MAINREF one {a, main ref}, of the same n
    implicit-row probe tuples: both cover every probe row once, and joined on a the ref is missing
    exactly where the row is, else it names the main record with that first row."""
    n = len(p)
    assert (np.sort(p[:, 0]) == np.arange(n, dtype=np.uint32)).all()
    assert (np.sort(q[:, 0]) == np.arange(n, dtype=np.uint32)).all()
    b_plain = np.empty(n, np.uint32)
    b_plain[p[:, 0]] = p[:, 1]
    refs = np.empty(n, np.uint32)
    refs[q[:, 0]] = q[:, 1]
    valid = refs != NOREF
    assert ((b_plain != NOREF) == valid).all()
    assert (refs[valid] < len(payload)).all()
    assert (payload[refs[valid], 1] == b_plain[valid]).all()


def mainref_probe(ctx, t, probe, n):
    import torch
    out = torch.zeros((max(n, 1), 2), dtype=torch.int32, device="cuda")
    r = ctx.probe(t, probe, out=out, mainref=True)
    return r, out[:n]


# ---- 1. refs point at the right group ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", EXP1_NAMES)
def test_mainref_points_at_the_group(ctx, name, path):
    import torch
    ref = EXP1[name]["plans"]["NrsNU"]
    with on_path(ctx, path):
        t, probe, nR = nrs_table(ctx, name)
        plain_out = torch.zeros((max(nR, 1), 2), dtype=torch.int32, device="cuda")
        plain = ctx.probe(t, probe, out=plain_out)
        got, ref_out = mainref_probe(ctx, t, probe, nR)
        _, payload, _ = t.export()
    assert got == plain
    assert (got.n_probe, got.n_matched, got.n_cmps, got.n_out) == (nR, ref["c_probe"], ref["c_cmp"], ref["c_top"])
    assert res_out(got) == ref["out"]
    assert_refs_match(host(plain_out)[:nR], host(ref_out), payload)


# ---- 2. the separate unnest equals the fused one ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", EXP1_NAMES)
def test_unnest_equals_fused_unnest(ctx, name, path):
    import torch
    plans = EXP1[name]["plans"]
    ref = plans["Nrs"]
    with on_path(ctx, path):
        t, probe, nR = nrs_table(ctx, name)
        _, nested = mainref_probe(ctx, t, probe, nR)
        out = torch.zeros((max(ref["out"]["n"], 1), 2), dtype=torch.int32, device="cuda")
        r = ctx.unnest(t, nested, out=out)
        r_nock = ctx.unnest(t, nested, out=out, checksum=False)
        r_count = ctx.unnest(t, nested)
    assert not r.overflow
    assert res_out(r) == ref["out"] and r.n_out == ref["c_unnest"]
    assert host_checksums(host(out)[: r.n_out]) == ref["out"]
    assert (r.n_probe, r.n_matched, r.n_cmps) == (nR, plans["NrsNU"]["c_probe"], 0)
    assert (r_nock.sum_h, r_nock.xor_h) == (0, 0)
    assert (r_nock.n_probe, r_nock.n_matched, r_nock.n_out, r_nock.n_cmps, r_nock.sum_a, r_nock.sum_b, r_nock.sum_c) == \
           (r.n_probe, r.n_matched, r.n_out, r.n_cmps, r.sum_a, r.sum_b, r.sum_c)
    assert r_count == r


# ---- 3. one heavy group ----
@pytest.fixture(scope="module")
def hot():
    """test_skewed_hot_key_heavy_unnest's relations: 70 % of S on key 17 (~210,000 rows)."""
    rng = np.random.default_rng(7)
    nR, nS = 1000, 300_000
    Rk = rng.permutation(nR).astype(np.uint32)
    Sa = rng.integers(0, nR, nS).astype(np.uint32)
    Sa[rng.random(nS) < 0.7] = 17
    R = O.tuples3(Rk, np.zeros(nR, np.uint32))
    S = O.tuples3(np.arange(nS, dtype=np.uint32), Sa)
    nb = O.num_distinct(Sa)
    return R, S, nb, O.nested_plan(S, 1, R, 0, nb, True)


def test_unnest_heavy_group(ctx, hot):
    import torch
    import hj3d
    R, S, nb, exp = hot
    dR, dS = dev(R), dev(S)
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    t.build(hj3d.Rel(dS, key_word=1))
    _, nested = mainref_probe(ctx, t, hj3d.Rel(dR, key_word=0), len(R))
    out = torch.zeros((exp.out["n"], 2), dtype=torch.int32, device="cuda")
    r = ctx.unnest(t, nested, out=out)
    assert not r.overflow and r.n_out == exp.c_unnest and r.n_matched == exp.c_probe
    assert res_out(r) == exp.out
    assert host_checksums(host(out)) == exp.out
    # ten copies of the hot key's nested tuple: ten expansions of ~210,000 rows each
    _, payload, sub = t.export()
    r17 = int(np.nonzero(R[:, 0] == 17)[0][0])
    one = nested[nested[:, 0] == r17]
    assert one.shape[0] == 1 and payload[host(one)[0, 1], 3] > 8192 * 20
    ten = one.repeat(10, 1).contiguous()
    want, _ = np_expand(host(ten), payload, sub)
    out = torch.zeros((len(want), 2), dtype=torch.int32, device="cuda")
    r = ctx.unnest(t, ten, out=out)
    assert (r.n_probe, r.n_matched, r.n_out, r.overflow) == (10, 10, len(want), False)
    assert res_out(r) == host_checksums(want)
    assert host_checksums(host(out)) == host_checksums(want)


# ---- 4. something between the probe and the unnest ----
def test_unnest_after_filter_reverse_concat(ctx):
    import torch
    t, probe, nR = nrs_table(ctx, "exp1_R1024_S4096_zipf")
    _, nested = mainref_probe(ctx, t, probe, nR)
    _, payload, sub = t.export()
    kept = nested[nested[:, 0] % 3 == 0].flip(0)
    misses = torch.stack([torch.arange(50, dtype=torch.int32, device="cuda"),
                          torch.full((50,), -1, dtype=torch.int32, device="cuda")], dim=1)
    stale = torch.tensor([[7, len(payload) + 5]], dtype=torch.int32, device="cuda")
    mixed = torch.cat([kept, misses, stale]).contiguous()
    want, nvalid = np_expand(host(mixed), payload, sub)
    assert 0 < nvalid <= kept.shape[0] and len(want) > nvalid
    out = torch.zeros((len(want), 2), dtype=torch.int32, device="cuda")
    r = ctx.unnest(t, mixed, out=out)
    assert (r.n_probe, r.n_matched, r.n_out, r.overflow) == (mixed.shape[0], nvalid, len(want), False)
    assert (keys64(host(out)) == keys64(want)).all()
    assert res_out(r) == host_checksums(want)


# ---- 5. capacity ----
CANARY = 0x5A5A5A5A


def test_unnest_capacity(ctx):
    import torch
    name = "exp1_R1024_S4096_zipf"
    ref = EXP1[name]["plans"]["Nrs"]
    t, probe, nR = nrs_table(ctx, name)
    _, nested = mainref_probe(ctx, t, probe, nR)
    n = ref["out"]["n"]
    full = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    r_full = ctx.unnest(t, nested, out=full)
    buf = torch.full((n + 64, 2), CANARY, dtype=torch.int32, device="cuda")
    r = ctx.unnest(t, nested, out=buf[: n - 1])
    assert r.overflow and not r_full.overflow
    assert res_out(r) == ref["out"] and (r.n_probe, r.n_matched) == (r_full.n_probe, r_full.n_matched)
    h = host(buf)
    assert (h[n - 1:] == CANARY).all()
    assert is_sub_multiset(h[: n - 1], host(full))
    # capacity 0 with a null buffer: nothing is written, the counters are complete
    r0 = ctx.unnest(t, nested, out=buf[:0])
    assert r0.overflow and res_out(r0) == ref["out"] and (r0.n_probe, r0.n_matched) == (r.n_probe, r.n_matched)
    assert (host(buf) == h).all()


# ---- 6. edges ----
def test_unnest_edges(ctx):
    import torch
    import hj3d
    t, probe, nR = nrs_table(ctx, "exp1_R1024_S4096_zipf")
    _, nested = mainref_probe(ctx, t, probe, nR)
    out = torch.full((4096, 2), CANARY, dtype=torch.int32, device="cuda")
    r = ctx.unnest(t, nested[:0], out=out)
    assert (r.n_probe, r.n_matched, r.n_out, r.sum_a, r.sum_b, r.sum_h, r.xor_h, r.overflow) == (0,) * 7 + (False,)
    t.clear()
    r = ctx.unnest(t, nested, out=out)
    assert (r.n_probe, r.n_matched, r.n_out, r.overflow) == (nR, 0, 0, False)
    # rebuilt from one tuple: the old refs are stale, at most ref 0 is still in range
    one = dev(O.tuples3(np.array([0], np.uint32), np.array([3], np.uint32)))
    t.build(hj3d.Rel(one, key_word=1))
    r = ctx.unnest(t, nested, out=out)
    assert r.n_probe == nR and r.n_matched <= 1 and r.n_out == r.n_matched
    assert (host(out)[1:] == CANARY).all()


# ---- 7. refusals ----
def test_refusals(ctx):
    import torch
    import hj3d
    L = hj3d.lib()
    R, S, nb = exp1_rel("exp1_R1024_S4096_zipf")
    dR, dS = dev(R), dev(S)
    probe = hj3d.Rel(dR, key_word=0)
    tn = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    tn.build(hj3d.Rel(dS, key_word=1))
    tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, nb)
    tc.build(hj3d.Rel(dS, key_word=1))
    out = torch.zeros((len(S), 2), dtype=torch.int32, device="cuda")
    out3 = torch.zeros((16, 3), dtype=torch.int32, device="cuda")
    M, E, U = hj3d.PROBE_MAINREF, hj3d.PROBE_EMIT, hj3d.PROBE_UNNEST

    def probe_st(t, flags, ptr=out.data_ptr(), cap=out.shape[0]):
        return L.hj3d_probe(ctx.h, t.h, C.byref(probe.c), flags, ptr, cap)

    assert probe_st(tc, M | E) == hj3d.HJ3D_EINVAL
    assert probe_st(tn, M | E | U) == hj3d.HJ3D_EINVAL
    assert probe_st(tn, M, None, 0) == hj3d.HJ3D_EINVAL
    preds = hj3d._sel_preds([(0, "<", 100)])
    assert L.hj3d_probe_sel(ctx.h, tn.h, C.byref(probe.c), preds, 1, M, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_probe_sel(ctx.h, tc.h, C.byref(probe.c), preds, 1, M | E, out.data_ptr(), out.shape[0]) == \
        hj3d.HJ3D_EINVAL
    assert probe_st(tn, M | E) == hj3d.HJ3D_OK
    nested = out[: len(R)]

    def unnest_st(t, flags, ptr=out.data_ptr(), cap=16):
        return L.hj3d_unnest(ctx.h, t.h, nested.data_ptr(), 8, flags, ptr, cap)

    assert unnest_st(tc, E) == hj3d.HJ3D_EINVAL
    assert unnest_st(tn, E | hj3d.PROBE_UNIQUE) == hj3d.HJ3D_EINVAL
    assert unnest_st(tn, E | hj3d.PROBE_ACCUMULATE) == hj3d.HJ3D_EINVAL
    assert unnest_st(tn, E | U) == hj3d.HJ3D_EINVAL
    assert unnest_st(tn, E, None, 16) == hj3d.HJ3D_EINVAL
    assert L.hj3d_unnest(ctx.h, tn.h, nested.data_ptr(), 1 << 32, 0, None, 0) == hj3d.HJ3D_EINVAL
    for ts, tt in ((tc, tn), (tn, tc)):
        assert L.hj3d_unnest2(ctx.h, ts.h, tt.h, out3.data_ptr(), 4, E, out3.data_ptr(), 4) == hj3d.HJ3D_EINVAL
    assert L.hj3d_unnest2(ctx.h, tn.h, tn.h, out3.data_ptr(), 4, E | hj3d.PROBE_UNIQUE, out3.data_ptr(), 4) == \
        hj3d.HJ3D_EINVAL
    assert L.hj3d_unnest2(ctx.h, tn.h, tn.h, out3.data_ptr(), 4, E, None, 4) == hj3d.HJ3D_EINVAL
    ctx.sync()


# ---- 8. unnest2 against the reference's experiment 4 ----
def scatter_refs(out, n):
    """Refs ordered by probe row from a dense MAINREF output (a = the probe row)."""
    import torch
    refs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    refs[out[:, 0].long()] = out[:, 1]
    return refs


@pytest.mark.parametrize("path", ["default", "partitioned"])
@pytest.mark.parametrize("name", EXP4_NAMES)
def test_unnest2_equals_reference_exp4(ctx, name, path):
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
    probe = hj3d.Rel(R, key_word=0)
    with on_path(ctx, path):
        _, out_s = mainref_probe(ctx, ts, probe, cardR)
        _, out_t = mainref_probe(ctx, tt, probe, cardR)
    trip = torch.stack([torch.arange(cardR, dtype=torch.int32, device="cuda"), scatter_refs(out_s, cardR),
                        scatter_refs(out_t, cardR)], dim=1).contiguous()
    c_top = ref["c_top"]
    out = torch.full((c_top + 8, 3), CANARY, dtype=torch.int32, device="cuda")
    got = ctx.unnest2(ts, tt, trip, out=out[:c_top])
    assert not got["overflow"]
    for k in ("c_top", "c_unnest_1", "c_unnest_2"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert all(got[k] == 0 for k in ("c_probe_rs", "c_probe_rs_cmp", "c_probe_rt", "c_probe_rt_cmp"))
    sums = ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")
    assert {k: got[k] for k in sums} == {k: ref["out"][k] for k in sums}
    h = host(out)
    cs = hj3d.triple_checksums(h[:c_top])
    assert cs == {k: ref["out"][k] for k in ("n",) + sums}
    assert (h[c_top:] == CANARY).all()
    nock = ctx.unnest2(ts, tt, trip, checksum=False)
    assert (nock["sum_h"], nock["xor_h"]) == (0, 0)
    assert all(nock[k] == got[k] for k in ("c_top", "c_unnest_1", "c_unnest_2", "sum_a", "sum_b", "sum_c"))
    # capacity c_top - 1: complete counters, nothing past the capacity, a sub-multiset written
    buf = torch.full((c_top + 8, 3), CANARY, dtype=torch.int32, device="cuda")
    low = ctx.unnest2(ts, tt, trip, out=buf[: c_top - 1])
    assert low["overflow"] and all(low[k] == got[k] for k in got if k != "overflow")
    hb = host(buf)
    assert (hb[c_top - 1:] == CANARY).all()
    assert is_sub_multiset(hb[: c_top - 1], h[:c_top])


# ---- 9. what probe2 cannot do: two probe attributes, two geometries ----
def group_index(keys, dom):
    order = np.argsort(keys, kind="stable")
    cnt = np.bincount(keys, minlength=dom).astype(np.int64)
    return order, np.cumsum(cnt) - cnt, cnt


@pytest.mark.parametrize("path", ["default", "partitioned"])
def test_unnest2_two_attributes(ctx, path):
    import torch
    import hj3d
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
    R = dev(O.tuples3(x, y))
    S = dev(O.tuples3(np.arange(nS, dtype=np.uint32), Sa))
    T = dev(O.tuples3(np.arange(nT, dtype=np.uint32), Ta))
    # the numpy triple join
    oS, fS, cS = group_index(Sa, dom + 100)
    oT, fT, cT = group_index(Ta, dom + 100)
    prod = cS[x] * cT[y]
    assert prod[0] == 300 * 400
    total = int(prod.sum())
    rr = np.repeat(np.arange(nR, dtype=np.int64), prod)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(prod) - prod, prod)
    ws = cS[x][rr]
    want = np.stack([rr, oS[fS[x][rr] + within % ws], oT[fT[y][rr] + within // ws]], axis=1).astype(np.uint32)
    ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, 2500), hj3d.Table(ctx, hj3d.HJ3D_NESTED, 1237)
    ts.build(hj3d.Rel(S, key_word=1))
    tt.build(hj3d.Rel(T, key_word=1))
    with on_path(ctx, path):
        _, out_s = mainref_probe(ctx, ts, hj3d.Rel(R, key_word=0), nR)
        _, out_t = mainref_probe(ctx, tt, hj3d.Rel(R, key_word=1), nR)
    trip = torch.stack([torch.arange(nR, dtype=torch.int32, device="cuda"), scatter_refs(out_s, nR),
                        scatter_refs(out_t, nR)], dim=1).contiguous()
    out = torch.zeros((total, 3), dtype=torch.int32, device="cuda")
    got = ctx.unnest2(ts, tt, trip, out=out)
    assert not got["overflow"] and got["c_top"] == got["c_unnest_2"] == total
    assert got["c_unnest_1"] == int(cT[y][prod > 0].sum())
    assert (rowsort(host(out)) == rowsort(want)).all()
    cs = hj3d.triple_checksums(want)
    assert {k: got[k] for k in ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")} == {k: cs[k] for k in cs if k != "n"}


# ---- the packed two-level partition and the fused selection carry the refs too ----
def test_mainref_on_packed_two_level_slices(ctx):
    """test_nested_probe_two_level_slices' table (200K buckets in slices of 64: 3125 slices, beyond the
    one-level partitioner) with HJ3D_PROBE_MAINREF: same result as without, refs at the right groups,
    and hj3d_unnest of them equals the fused unnest of the same probe. Probed with S itself as well:
    its Zipf keys overflow some partition regions, so those tuples' refs come from the overflow kernel."""
    import torch
    import hj3d
    rng = np.random.default_rng(41)
    nb, nR, nS = 200_000, 300_000, 800_000
    Rk = rng.permutation(nR).astype(np.uint32)
    Sa = np.minimum(rng.zipf(1.5, nS) - 1, nR - 1).astype(np.uint32)
    Sa[: nS // 2] = rng.integers(0, nR, nS // 2, dtype=np.uint32)
    dR = dev(O.tuples3(Rk, np.zeros_like(Rk)))
    dS = dev(O.tuples3(np.arange(nS, dtype=np.uint32), Sa))
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    t.build(hj3d.Rel(dS, key_word=1))
    probe = hj3d.Rel(dR, key_word=0)
    ctx.radix_min(0)
    ctx.pk_slice_max(64)
    try:
        plain_out = torch.zeros((nR, 2), dtype=torch.int32, device="cuda")
        plain = ctx.probe(t, probe, out=plain_out)
        got, ref_out = mainref_probe(ctx, t, probe, nR)
        fused = ctx.probe(t, probe, unnest=True)
        self_probe = hj3d.Rel(dS, key_word=1)
        plain_s_out = torch.zeros((nS, 2), dtype=torch.int32, device="cuda")
        plain_s = ctx.probe(t, self_probe, out=plain_s_out)
        got_s, ref_s_out = mainref_probe(ctx, t, self_probe, nS)
    finally:
        ctx.radix_min(1 << 20)
        ctx.pk_slice_max(0)
    assert got == plain and got_s == plain_s and got_s.n_matched == nS
    _, payload, _ = t.export()
    assert_refs_match(host(plain_out), host(ref_out), payload)
    assert_refs_match(host(plain_s_out), host(ref_s_out), payload)
    r = ctx.unnest(t, ref_out)
    assert res_out(r) == res_out(fused) and (r.n_matched, r.n_out) == (fused.n_matched, nS)


def test_mainref_on_slices_wider_than_lds(ctx):
    """The partitioned probe's HBM form (slices that do not fit a workgroup's LDS, read through L2 by
    16 workgroups each): a 24M-bucket table whose slice bound of 2 buckets (HJ3D_OPT_PK_SLICE) keeps it
    off the packed two-level partition, so the one-level partitioner's 2048 slices are ~11,700 buckets
    wide. Device-generated relations; the refs are checked by what they unnest to: hj3d_unnest of the
    MAINREF output equals the fused unnest of the same probe, counters and checksums."""
    import torch
    import hj3d
    n, nR = 24_000_000, 2_000_000
    g = torch.Generator(device="cuda").manual_seed(5)
    S = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    S[:, 0] = torch.arange(n, dtype=torch.int32, device="cuda")
    S[:, 1] = torch.randint(0, n, (n,), dtype=torch.int32, device="cuda", generator=g)
    R = torch.zeros((nR, 3), dtype=torch.int32, device="cuda")
    R[:, 0] = torch.randint(0, n, (nR,), dtype=torch.int32, device="cuda", generator=g)
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, n)
    t.build(hj3d.Rel(S, key_word=1))
    probe = hj3d.Rel(R, key_word=0)
    plain_out = torch.zeros((nR, 2), dtype=torch.int32, device="cuda")
    ctx.pk_slice_max(2)
    try:
        plain = ctx.probe(t, probe, out=plain_out)
        got, ref_out = mainref_probe(ctx, t, probe, nR)
        fused = ctx.probe(t, probe, unnest=True)
    finally:
        ctx.pk_slice_max(0)
    assert got == plain and got.n_probe == nR and 0 < got.n_matched < nR
    p, q = plain_out[torch.argsort(plain_out[:, 0])], ref_out[torch.argsort(ref_out[:, 0])]
    rows = torch.arange(nR, dtype=torch.int32, device="cuda")
    assert bool((p[:, 0] == rows).all()) and bool((q[:, 0] == rows).all())
    assert bool(((p[:, 1] == -1) == (q[:, 1] == -1)).all())
    r = ctx.unnest(t, ref_out)
    assert (r.n_probe, r.n_matched, r.n_out) == (nR, fused.n_matched, fused.n_out)
    assert res_out(r) == res_out(fused)


def test_mainref_with_fused_selection(ctx):
    import torch
    name = "exp1_R10007_S100003_zipf08_t1_b3"
    preds = [(0, "<", 5000)]
    with on_path(ctx, "partitioned"):
        t, probe, nR = nrs_table(ctx, name)
        plain_out = torch.full((nR, 2), CANARY, dtype=torch.int32, device="cuda")
        plain = ctx.probe_sel(t, probe, preds, out=plain_out)
        ref_out = torch.full((nR, 2), CANARY, dtype=torch.int32, device="cuda")
        got = ctx.probe_sel(t, probe, preds, out=ref_out, mainref=True)
        _, payload, _ = t.export()
    R, _, _ = exp1_rel(name)
    npass = int((R[:, 0] < 5000).sum())
    assert got == plain and got.n_probe == npass
    p, q = host(plain_out)[:npass], host(ref_out)[:npass]
    p, q = p[np.argsort(p[:, 0])], q[np.argsort(q[:, 0])]
    assert (p[:, 0] == q[:, 0]).all() and (p[:, 0] == np.nonzero(R[:, 0] < 5000)[0]).all()
    valid = q[:, 1] != NOREF
    assert ((p[:, 1] != NOREF) == valid).all()
    assert (payload[q[valid, 1], 1] == p[valid, 1]).all()
