"""Experiment-4 triple output (hj3d_probe2 with HJ3D_PROBE_EMIT) on the GPU.

The written triples are compared with the reference binary's fixtures (checksums of the written
rows, and for the fixtures that carry their columns the exact triple set) and with a numpy
brute-force join. The committed fixtures have products |S(k)| x |T(k)| <= 5, so they stay on the
inline path; a synthetic skewed input drives the heavy kernels (products 64 inline, 72, 42,000 and
300 heavy, and a key that matches S but not T). Every buffer has 64 guard rows behind its capacity,
pre-filled with 0xFFFFFFFF (never a row id here), which must stay untouched."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

EXP4 = load_golden("exp4_*.json", headline=False)
PLANS = ("Ndu", "Chj")
PATHS = ("default", "partitioned")
GUARD = 64
SENT = 0xFFFFFFFF
CK = ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")
COUNTERS = ("c_probe_rs", "c_probe_rs_cmp", "c_probe_rt", "c_probe_rt_cmp", "c_top")


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def brute_join(Rk, Sa, Ta) -> np.ndarray:
    """All (r, s, t) row triples with R.k[r] == S.a[s] == T.a[t], sorted by row, (n, 3) uint32."""
    Sa, Ta = np.asarray(Sa, dtype=np.uint32), np.asarray(Ta, dtype=np.uint32)
    so, to = np.argsort(Sa, kind="stable"), np.argsort(Ta, kind="stable")
    ss, st = Sa[so], Ta[to]
    out = [np.zeros((0, 3), dtype=np.uint32)]
    for r, k in enumerate(np.asarray(Rk, dtype=np.uint32)):
        s = so[np.searchsorted(ss, k, "left"):np.searchsorted(ss, k, "right")]
        t = to[np.searchsorted(st, k, "left"):np.searchsorted(st, k, "right")]
        if len(s) and len(t):
            blk = np.empty((len(s) * len(t), 3), dtype=np.uint32)
            blk[:, 0] = r
            blk[:, 1] = np.repeat(s, len(t))
            blk[:, 2] = np.tile(t, len(s))
            out.append(blk)
    return rowsort(np.concatenate(out))


def rowsort(t: np.ndarray) -> np.ndarray:
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def relations(Rk, Sa, Ta):
    R = dev(O.tuples2(np.asarray(Rk, dtype=np.uint32), np.zeros(len(Rk), np.uint32)))
    S = dev(O.tuples2(np.arange(len(Sa), dtype=np.uint32), np.asarray(Sa, dtype=np.uint32)))
    T = dev(O.tuples2(np.arange(len(Ta), dtype=np.uint32), np.asarray(Ta, dtype=np.uint32)))
    return R, S, T


def fixture_relations(g):
    log2R, a, A, b, B = g["generator_args"][1:6]
    Sa, Ta = O.gen_exp4(log2R, a, A, b, B)
    return relations(np.arange(1 << log2R, dtype=np.uint32), Sa, Ta)


def buffer(cap):
    import torch
    return torch.full((cap + GUARD, 3), -1, dtype=torch.int32, device="cuda")


def host(buf) -> np.ndarray:
    return buf.cpu().numpy().view(np.uint32)


def emit(ctx, plan, R, S, T, nb, cap, path="default", sharded=0, **kw):
    """One run into a fresh guarded buffer of capacity cap: (result dict, host copy of the buffer)."""
    import hj3d
    buf = buffer(cap)
    if path == "partitioned":
        ctx.radix_min(1 << 6)
    try:
        if sharded:
            got = hj3d.exp4_plan_sharded(ctx, plan, R, S, T, nb, sharded, out=buf[:cap], **kw)
        else:
            got = hj3d.exp4_plan(ctx, plan, R, S, T, nb, out=buf[:cap], **kw)
    finally:
        ctx.radix_min(1 << 20)
    return got, host(buf)


def assert_guard(h, cap):
    assert (h[cap:] == SENT).all(), "rows at or beyond the capacity were written"


def compare_counters(plan, got, ref, out):
    """got (probe2 dict) against reference counters `ref` (lower-case keys) and checksums `out`."""
    for k in COUNTERS:
        assert got[k] == ref[k], (plan, k, got[k], ref[k])
    if plan == "Ndu":
        assert (got["c_unnest_1"], got["c_unnest_2"]) == (ref["c_unnest_1"], ref["c_unnest_2"]), plan
    assert {k: got[k] for k in CK} == {k: out[k] for k in CK}, plan


# ---- the reference binary's fixtures ----

@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,g", EXP4, ids=[n for n, _ in EXP4])
def test_emit_fixtures(ctx, name, g, path):
    import hj3d
    R, S, T = fixture_relations(g)
    exact = brute_join(np.arange(g["cardR"], dtype=np.uint32), g["Sa"], g["Ta"]) if "Sa" in g else None
    for plan in PLANS:
        ref = g["plans"][plan]
        cap = ref["c_top"]
        got, h = emit(ctx, plan, R, S, T, g["nb"], cap, path)
        assert got["overflow"] is False, plan
        compare_counters(plan, got, {k.lower(): v for k, v in ref.items() if k != "out"}, ref["out"])
        assert_guard(h, cap)
        assert hj3d.triple_checksums(h[:cap]) == ref["out"], plan
        if exact is not None:
            assert np.array_equal(rowsort(h[:cap]), exact), plan


def test_fixtures_with_columns_present():
    assert {n for n, g in EXP4 if "Sa" in g} >= {"exp4_R3_a2_A2_b2_B1", "exp4_R10_a3_A2_b2_B3"}


# ---- skew: the heavy kernels ----

SKEW_NB = 1536
SKEW_N = 46532  # 64 + 72 + 42,000 + 300 + 4,096


@pytest.fixture(scope="module")
def skew():
    """R.k = arange(4096); |S(k)| x |T(k)|: key 5: 8 x 8 (the last inline product), 3: 9 x 8 (the first
    heavy one), 11: 600 x 70, 13: 1 x 300, 17: 50 x 0 (matches S, fails T), 1024..3071: 1 x 2."""
    mult = {5: (8, 8), 3: (9, 8), 11: (600, 70), 13: (1, 300), 17: (50, 0)}
    mult.update({k: (1, 2) for k in range(1024, 3072)})
    rng = np.random.default_rng(0)
    Sa = rng.permutation(np.repeat(np.array(list(mult), dtype=np.uint32), [m[0] for m in mult.values()]))
    Ta = rng.permutation(np.repeat(np.array(list(mult), dtype=np.uint32), [m[1] for m in mult.values()]))
    Rk = np.arange(4096, dtype=np.uint32)
    exact = brute_join(Rk, Sa, Ta)
    assert len(exact) == SKEW_N
    Rh, Sh, Th = (O.tuples2(Rk, np.zeros(4096, np.uint32)), O.tuples2(np.arange(len(Sa), dtype=np.uint32), Sa),
                  O.tuples2(np.arange(len(Ta), dtype=np.uint32), Ta))
    orc = {plan: O.exp4_plan(Rh, Sh, Th, SKEW_NB, plan == "Ndu") for plan in PLANS}
    return {"dev": relations(Rk, Sa, Ta), "exact": exact, "oracle": orc, "miss": relations(Rk + 100000, Sa, Ta)}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("plan", PLANS)
def test_emit_skew_heavy_paths(ctx, skew, plan, path):
    orc = skew["oracle"][plan]
    assert orc["c_top"] == SKEW_N and orc["out"]["n"] == SKEW_N
    got, h = emit(ctx, plan, *skew["dev"], SKEW_NB, SKEW_N, path)
    assert got["overflow"] is False
    compare_counters(plan, got, orc, orc["out"])
    assert_guard(h, SKEW_N)
    assert np.array_equal(rowsort(h[:SKEW_N]), skew["exact"])  # no loss, no duplicate


# ---- overflow ----

def as_keys(t: np.ndarray) -> np.ndarray:
    """One comparable key per triple (r < 2^12, s and t < 2^13 on the skew input)."""
    t = t.astype(np.uint64)
    return (t[:, 0] << np.uint64(40)) | (t[:, 1] << np.uint64(20)) | t[:, 2]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("plan", PLANS)
def test_emit_overflow_keeps_counters_and_bounds(ctx, skew, plan, path):
    orc = skew["oracle"][plan]
    cap = SKEW_N - 5
    got, h = emit(ctx, plan, *skew["dev"], SKEW_NB, cap, path)
    assert got["overflow"] is True
    compare_counters(plan, got, orc, orc["out"])  # c_top and the checksums count every triple
    assert_guard(h, cap)
    keys = as_keys(h[:cap])
    assert len(np.unique(keys)) == cap, "written triples repeat"
    assert np.isin(keys, as_keys(skew["exact"])).all(), "a written triple is not in the result"


@pytest.mark.parametrize("plan", PLANS)
def test_emit_capacity_zero_with_buffer(ctx, skew, plan):
    """cap = 0 with a valid pointer (through the C ABI: the Python wrapper passes NULL for an empty
    tensor): nothing is written, the overflow is reported."""
    import hj3d
    R, S, T = skew["dev"]
    kind = hj3d.HJ3D_NESTED if plan == "Ndu" else hj3d.HJ3D_CHAIN
    ts, tt = hj3d.Table(ctx, kind, SKEW_NB), hj3d.Table(ctx, kind, SKEW_NB)
    ctx.build_many([ts, tt], [hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)])
    buf = buffer(0)
    rel = hj3d.Rel(R, key_word=0)
    st = hj3d.lib().hj3d_probe2(ctx.h, ts.h, tt.h, C.byref(rel.c), hj3d.PROBE_EMIT | hj3d.PROBE_CHECKSUM,
                                buf.data_ptr(), 0)
    assert st == hj3d.HJ3D_OK
    got = ctx.probe2_result()
    assert got["overflow"] is True
    orc = skew["oracle"][plan]
    compare_counters(plan, got, orc, orc["out"])
    assert_guard(host(buf), 0)
    ts.close()
    tt.close()


# ---- flags ----

@pytest.mark.parametrize("plan", PLANS)
def test_emit_without_checksum(ctx, skew, plan):
    orc = skew["oracle"][plan]
    got, h = emit(ctx, plan, *skew["dev"], SKEW_NB, SKEW_N, checksum=False)
    assert got["overflow"] is False
    assert (got["sum_h"], got["xor_h"]) == (0, 0)
    assert {k: got[k] for k in ("sum_a", "sum_b", "sum_c", "c_top")} == \
           {"sum_a": orc["out"]["sum_a"], "sum_b": orc["out"]["sum_b"], "sum_c": orc["out"]["sum_c"], "c_top": SKEW_N}
    assert_guard(h, SKEW_N)
    assert np.array_equal(rowsort(h[:SKEW_N]), skew["exact"])


@pytest.mark.parametrize("plan", PLANS)
def test_emit_invalid_arguments(ctx, skew, plan):
    import hj3d
    R, S, T = skew["dev"]
    kind = hj3d.HJ3D_NESTED if plan == "Ndu" else hj3d.HJ3D_CHAIN
    ts, tt = hj3d.Table(ctx, kind, SKEW_NB), hj3d.Table(ctx, kind, SKEW_NB)
    ctx.build_many([ts, tt], [hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)])
    rel = hj3d.Rel(R, key_word=0)
    buf = buffer(16)
    L = hj3d.lib()
    st = L.hj3d_probe2(ctx.h, ts.h, tt.h, C.byref(rel.c), hj3d.PROBE_EMIT | hj3d.PROBE_ACCUMULATE, buf.data_ptr(), 16)
    assert st == hj3d.HJ3D_EINVAL
    st = L.hj3d_probe2(ctx.h, ts.h, tt.h, C.byref(rel.c), hj3d.PROBE_EMIT, None, 16)
    assert st == hj3d.HJ3D_EINVAL
    ctx.sync()
    assert_guard(host(buf), 0)  # neither call wrote anything
    # ACCUMULATE without EMIT stays accepted (and ignored), as before
    st = L.hj3d_probe2(ctx.h, ts.h, tt.h, C.byref(rel.c), hj3d.PROBE_CHECKSUM | hj3d.PROBE_ACCUMULATE, None, 0)
    assert st == hj3d.HJ3D_OK
    got = ctx.probe2_result()
    assert got["overflow"] is False and got["c_top"] == SKEW_N
    ts.close()
    tt.close()


# ---- empty results ----

@pytest.mark.parametrize("plan", PLANS)
def test_emit_empty_probe_relation(ctx, skew, plan):
    R, S, T = skew["dev"]
    got, h = emit(ctx, plan, R[:0], S, T, SKEW_NB, 32)
    assert got["c_top"] == 0 and got["overflow"] is False
    assert_guard(h, 0)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("plan", PLANS)
def test_emit_all_keys_miss(ctx, skew, plan, path):
    got, h = emit(ctx, plan, *skew["miss"], SKEW_NB, 32, path)
    assert got["c_top"] == 0 and got["overflow"] is False
    assert_guard(h, 0)


# ---- owner split ----

def _split_case(ctx, plan, R, S, T, nb, n):
    one, h1 = emit(ctx, plan, R, S, T, nb, n)
    got, h = emit(ctx, plan, R, S, T, nb, n, sharded=3)
    assert one["overflow"] is False and got["overflow"] is False
    for k in COUNTERS + ("c_unnest_1", "c_unnest_2") + CK:
        assert got[k] == one[k], (plan, k)
    assert_guard(h, n)
    assert np.array_equal(rowsort(h[:n]), rowsort(h1[:n])), plan


@pytest.mark.parametrize("plan", PLANS)
def test_emit_owner_split_skew(ctx, skew, plan):
    _split_case(ctx, plan, *skew["dev"], SKEW_NB, SKEW_N)


@pytest.mark.parametrize("plan", PLANS)
def test_emit_owner_split_fixture(ctx, plan):
    g = dict(EXP4)["exp4_R10_a3_A2_b2_B3"]
    _split_case(ctx, plan, *fixture_relations(g), g["nb"], g["plans"][plan]["c_top"])
