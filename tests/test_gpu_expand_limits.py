"""The expansion kernels past their first grid round and at their internal size limits.

Every operator that turns nested matches into output tuples ends in a kernel that strides a fixed,
chip-sized grid over work whose size only the device knows: k_expand_light / k_heavy_offsets /
k_expand_heavy_flat (hj3d_unnest and the fused hj3d_probe with UNNEST | EMIT), k_un2_slots /
k_un2_expand (hj3d_unnest2), k_ndu_heavy / k_chj_heavy (hj3d_probe2). The other tests stay inside the
first round and below every constant; the inputs here are sized from the device's CU count and the
kernels' constants so that each case provably (host-side assert) takes the branch it is about.

Expected values come from tests/expand_ref.py (numpy over the relations' key columns and the input
tuples' keys) and the oracle; nothing is derived from a table export or from another run of the
library. The one library result used as an input is the key -> main ref translation (a MAINREF
probe of one tuple per distinct key), from which the tests assemble their own input tuples.
Integer work: every comparison is exact."""
import math

import numpy as np
import pytest

import expand_ref as X
import oracle as O
from test_gpu_exp4_emit import compare_counters
from test_gpu_unnest import CANARY, dev, host, mainref_probe, on_path, res_out, scatter_refs

pytestmark = pytest.mark.gpu

# the kernels' constants (a change there must fail the branch assertions below, not empty the cases)
HEAVY_OUT = 8192        # nested.hip:257  kHeavyOut: more outputs than this make a slot heavy
HEAVY_SPAN = 1024       # nested.hip:434  kHeavySpan: flattened heavy outputs per wave and round
OFFSETS_ROUND = 1024    # nested.hip:392,401  k_heavy_offsets: heavy slots scanned per round (one workgroup)
UN2_CHUNK = 2048        # nested_tuple.hpp:62  kChunk: outputs per workgroup and step
UN2_CHUNK_SLOTS = 2048  # nested_tuple.hpp:63  kChunkSlots: slot offsets of a chunk staged in LDS
INLINE2 = 64            # exp4.hip:27  kInline2: larger products are queued for the heavy kernels
BLOCK, WAVE = 256, 64   # hj3d_internal.hpp:31  kBlock, hj3d_device.hpp:13  kWave
NOREF = X.NOREF
GUARD = 64
PROBE2_ZERO = ("c_probe_rs", "c_probe_rs_cmp", "c_probe_rt", "c_probe_rt_cmp")
SUMS = ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")


def cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def heavy_groups(n_cus):  # nested.hip:723, exp4.hip:552,565: workgroups of the heavy kernels
    return 4 * n_cus


def heavy_flat_round(n_cus):  # outputs k_expand_heavy_flat covers before a wave takes its next span
    return heavy_groups(n_cus) * (BLOCK // WAVE) * HEAVY_SPAN


def un2_round(n_cus):  # unnest2.hip:108: outputs k_un2_expand covers before a workgroup takes its next chunk
    return 8 * n_cus * UN2_CHUNK


def canary_buffer(rows, words):
    import torch
    return torch.full((rows + GUARD, words), CANARY, dtype=torch.int32, device="cuda")


def tail_intact(buf, cap) -> bool:
    return bool((buf[cap:] == CANARY).all())


def nested_table(ctx, col, nb):
    """A nested table on the key column `col` (rows implicit); the relation is returned with it."""
    import hj3d
    rel = dev(O.tuples2(np.arange(len(col), dtype=np.uint32), col))
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    t.build(hj3d.Rel(rel, key_word=1))
    assert t.build_path().startswith("nested_"), t.build_path()
    return t, rel


def key_refs(ctx, t, keys) -> dict:
    """{key: main ref in t} of distinct keys (NOREF: the key has no group), by a MAINREF probe of one
    tuple per key."""
    import hj3d
    k = np.asarray(keys, dtype=np.uint32)
    assert len(np.unique(k)) == len(k)
    rel = dev(O.tuples2(k, np.zeros(len(k), np.uint32)))
    _, out = mainref_probe(ctx, t, hj3d.Rel(rel, key_word=0), len(k))
    refs = host(scatter_refs(out, len(k)))
    return {int(key): int(r) for key, r in zip(k, refs)}


def refs_of(keys, refmap, n_mains):
    """The ref word of every input tuple: its key's main ref, or for a dead tuple (key None) in turn
    0xFFFFFFFF and a ref >= n_mains (a table rebuilt smaller since the probe)."""
    out = np.empty(len(keys), dtype=np.uint32)
    for i, k in enumerate(keys):
        out[i] = refmap[int(k)] if k is not None else (NOREF if (i // 2) % 2 else n_mains + i % 7)
    return out


def scattered(rng, keys, sizes) -> np.ndarray:
    """A key column with sizes[j] rows of keys[j], at scattered row ids."""
    return rng.permutation(np.repeat(np.asarray(keys, dtype=np.uint32), sizes))


# ---- a / b / c: many heavy slots through k_heavy_offsets and k_expand_heavy_flat ----
KEY_A, KEY_B, KEY_MISSING = 700_001, 700_002, 700_003


def heavy_copies(n_cus) -> int:
    """Copies of the 8193-row group's tuple: more than one k_heavy_offsets round, and 2.25 grid rounds
    of k_expand_heavy_flat."""
    return max(OFFSETS_ROUND + 1, math.ceil(2.25 * heavy_flat_round(n_cus) / (HEAVY_OUT + 1)))


def interleave(rng, H, small_keys, dead):
    """The key of every tuple: three small tuples, then H times {the 8193-row key, a filler}; of eight
    fillers one is the 8192-row key, five are small keys, two are `dead` (None, or a key without group)."""
    keys = [int(k) for k in small_keys[:3]]
    for j in range(H):
        keys.append(KEY_A)
        f = j % 8
        keys.append(KEY_B if f == 0 else dead if f in (5, 6) else int(small_keys[rng.integers(len(small_keys))]))
    return keys


def assert_heavy_branches(cnt, n_cus, H):
    """The per-slot output counts put the case where it claims to be."""
    heavy = cnt > HEAVY_OUT
    assert int(heavy.sum()) == H > OFFSETS_ROUND  # k_heavy_offsets carries into a second round
    assert int(cnt[heavy].sum()) > 2 * heavy_flat_round(n_cus)  # every wave of the flat kernel takes a third span
    assert (cnt == HEAVY_OUT).any() and (cnt == HEAVY_OUT + 1).any()  # both sides of cc > kHeavyOut
    assert int(cnt[:3].sum()) >= 3 and not heavy[:3].any()  # outputs before the first heavy slot


@pytest.fixture(scope="module")
def big_s(ctx):
    """S: one group of 8193 rows, one of 8192, 300 small groups of 1 to 40 rows; its nested table and
    the main ref of every key."""
    rng = np.random.default_rng(101)
    small = np.arange(1000, 1300, dtype=np.uint32)
    sizes = rng.integers(1, 41, len(small))
    sizes[:3] = (2, 3, 5)
    Sa = scattered(rng, np.concatenate([[KEY_A, KEY_B], small]), np.concatenate([[HEAVY_OUT + 1, HEAVY_OUT], sizes]))
    groups = X.group_index(Sa)
    t, rel = nested_table(ctx, Sa, len(groups))
    refmap = key_refs(ctx, t, np.concatenate([groups.keys, [KEY_MISSING]]))
    live = [refmap[int(k)] for k in groups.keys]
    assert refmap[KEY_MISSING] == NOREF and sorted(live) == list(range(len(groups)))
    return {"Sa": Sa, "groups": groups, "small": small, "t": t, "rel": rel, "refs": refmap, "n_mains": len(groups)}


@pytest.fixture(scope="module")
def heavy_case(big_s):
    """Case a's stored nested tuples {a, main ref} and what they must expand to."""
    import torch
    n_cus = cus()
    H = heavy_copies(n_cus)
    rng = np.random.default_rng(102)
    keys = interleave(rng, H, big_s["small"], None)
    n = len(keys)
    a = (rng.permutation(n) + 5000).astype(np.uint32)  # distinct
    refs = refs_of(keys, big_s["refs"], big_s["n_mains"])
    cnt = X.pair_counts(keys, big_s["groups"])
    assert_heavy_branches(cnt, n_cus, H)
    kinds = np.array([0 if k == KEY_A else 1 if k == KEY_B else 2 for k in keys])
    for b in range(n // BLOCK):  # both big groups inside the same 256-slot block of k_expand_light
        blk = kinds[b * BLOCK:(b + 1) * BLOCK]
        assert (blk == 0).any() and (blk == 1).any()
    assert (refs == NOREF).any() and ((refs >= big_s["n_mains"]) & (refs != NOREF)).any()
    want = X.expand_pairs(a, keys, big_s["groups"])
    ooff = np.concatenate([[0], np.cumsum(cnt)])
    nested = torch.from_numpy(np.stack([a, refs], axis=1).view(np.int32)).cuda().contiguous()
    return {"t": big_s["t"], "nested": nested, "n": n, "total": len(want), "want_sorted": np.sort(X.pack_pairs(want)),
            "cs": X.pair_checksums(want), "counters": X.pair_counters(a, keys, big_s["groups"]), "ooff": ooff,
            "heavy_slots": np.nonzero(cnt > HEAVY_OUT)[0]}


def counters_of(r) -> dict:
    return {"n_probe": r.n_probe, "n_matched": r.n_matched, "n_out": r.n_out}


def test_unnest_many_heavy_slots(ctx, heavy_case):
    c = heavy_case
    t, nested, total = c["t"], c["nested"], c["total"]
    assert c["counters"]["n_out"] == total
    buf = canary_buffer(total, 2)
    r = ctx.unnest(t, nested, out=buf[:total])
    assert not r.overflow and r.n_cmps == 0
    assert counters_of(r) == c["counters"]
    assert res_out(r) == c["cs"]
    assert tail_intact(buf, total)
    assert np.array_equal(np.sort(X.pack_pairs(host(buf[:total]))), c["want_sorted"])  # no loss, no duplicate
    assert ctx.unnest(t, nested) == r  # counters and sums only
    nock = ctx.unnest(t, nested, out=buf[:total], checksum=False)
    assert (nock.sum_h, nock.xor_h, nock.overflow) == (0, 0, False)
    assert counters_of(nock) == c["counters"]
    assert (nock.sum_a, nock.sum_b, nock.sum_c) == (c["cs"]["sum_a"], c["cs"]["sum_b"], 0)
    assert tail_intact(buf, total)
    assert np.array_equal(np.sort(X.pack_pairs(host(buf[:total]))), c["want_sorted"])


@pytest.mark.parametrize("path", ["direct", "partitioned"])
def test_fused_probe_unnest_many_heavy_slots(ctx, big_s, path):
    """The same expansion behind the probe itself: H probe tuples on the 8193-row key (the probe
    relation is not key-unique), the implicit probe rows are the a values."""
    import hj3d
    n_cus = cus()
    H = heavy_copies(n_cus)
    keys = interleave(np.random.default_rng(103), H, big_s["small"], KEY_MISSING)
    Rk = np.array(keys, dtype=np.uint32)
    nR = len(Rk)
    cnt = X.pair_counts(Rk, big_s["groups"])
    assert_heavy_branches(cnt, n_cus, H)
    a = np.arange(nR, dtype=np.uint32)
    want = X.expand_pairs(a, Rk, big_s["groups"])
    total = len(want)
    R = O.tuples2(Rk, np.zeros(nR, np.uint32))
    S = O.tuples2(np.arange(len(big_s["Sa"]), dtype=np.uint32), big_s["Sa"])
    exp = O.nested_plan(S, 1, R, 0, big_s["n_mains"], True)
    assert exp.c_unnest == total and exp.out == X.pair_checksums(want)
    dR = dev(R)
    buf = canary_buffer(total, 2)
    with on_path(ctx, path):
        got = ctx.probe(big_s["t"], hj3d.Rel(dR, key_word=0), unnest=True, out=buf[:total])
    assert not got.overflow
    assert (got.n_probe, got.n_matched, got.n_out, got.n_cmps) == (nR, exp.c_probe, exp.c_unnest, exp.c_cmp)
    assert res_out(got) == exp.out
    assert tail_intact(buf, total)
    assert np.array_equal(np.sort(X.pack_pairs(host(buf[:total]))), np.sort(X.pack_pairs(want)))


@pytest.mark.parametrize("where", ["zero_with_buffer", "one", "before_first_heavy", "inside_heavy", "total_minus_1"])
def test_unnest_capacity_inside_heavy_work(ctx, heavy_case, where):
    import hj3d
    c = heavy_case
    t, nested, total, ooff, hs = c["t"], c["nested"], c["total"], c["ooff"], c["heavy_slots"]
    mid = int(hs[len(hs) // 2])
    cap = {"zero_with_buffer": 0, "one": 1, "before_first_heavy": int(ooff[hs[0]]) - 1,
           "inside_heavy": int(ooff[mid]) + HEAVY_OUT // 2 + 1, "total_minus_1": total - 1}[where]
    assert 0 <= cap < total
    if where == "before_first_heavy":
        assert 1 < cap == int(ooff[hs[0]]) - 1  # every heavy output is cut, the light ones before it are not
    if where == "inside_heavy":
        assert ooff[mid] < cap < ooff[mid + 1] and ooff[mid + 1] - ooff[mid] > HEAVY_OUT
    buf = canary_buffer(total, 2)
    if cap:
        r = ctx.unnest(t, nested, out=buf[:cap])
    else:  # through the C ABI: the wrapper passes NULL for an empty tensor
        st = hj3d.lib().hj3d_unnest(ctx.h, t.h, nested.data_ptr(), c["n"], hj3d.PROBE_EMIT | hj3d.PROBE_CHECKSUM,
                                    buf.data_ptr(), 0)
        assert st == hj3d.HJ3D_OK
        r = ctx.probe_result()
    assert r.overflow
    assert counters_of(r) == c["counters"] and res_out(r) == c["cs"]  # complete: every pair is counted
    assert tail_intact(buf, cap)
    assert X.is_sub_multiset(X.pack_pairs(host(buf[:cap])), c["want_sorted"])


# ---- d / e / f: hj3d_unnest2 ----
def unnest2_input(a, key_s, key_t, refs_s, refs_t, n_mains):
    """{a, ref_s, ref_t} on the device for per-tuple keys (None: that ref is invalid)."""
    import torch
    trip = np.stack([np.asarray(a, dtype=np.uint32), refs_of(key_s, refs_s, n_mains[0]),
                     refs_of(key_t, refs_t, n_mains[1])], axis=1)
    return torch.from_numpy(trip.view(np.int32)).cuda().contiguous()


def chunk_slots(prod) -> np.ndarray:
    """nq of every k_un2_expand chunk: the slots from the one holding the chunk's first output to the
    one holding its last (for_each_output, nested_tuple.hpp:92-94)."""
    ooff = np.concatenate([[0], np.cumsum(prod)])
    total = int(ooff[-1])
    first = np.arange(0, total, UN2_CHUNK)
    last = np.minimum(first + UN2_CHUNK, total) - 1
    return (np.searchsorted(ooff, last, "right") - 1) - (np.searchsorted(ooff, first, "right") - 1) + 1


def assert_unnest2_exact(ctx, ts, tt, trip, want, counters, checksum=True):
    """EMIT into an exact-size buffer: the triples as a multiset, every counter and checksum."""
    total = len(want)
    buf = canary_buffer(total, 3)
    got = ctx.unnest2(ts, tt, trip, out=buf[:total], checksum=checksum)
    assert got["overflow"] is False
    assert {k: got[k] for k in counters} == counters
    assert all(got[k] == 0 for k in PROBE2_ZERO)
    cs = X.triple_checksums(want)
    assert {k: got[k] for k in SUMS} == {k: cs[k] for k in SUMS}
    assert tail_intact(buf, total)
    assert np.array_equal(np.sort(X.pack_triples(host(buf[:total]))), np.sort(X.pack_triples(want)))
    return got


@pytest.fixture(scope="module")
def small_st(ctx):
    """S and T for the staging cases: group sizes 1, 2 and 3 on S.a, 1 and 2 on T.a; tables of
    different geometry."""
    rng = np.random.default_rng(201)
    ks = np.arange(200, dtype=np.uint32)
    Sa = scattered(rng, ks, np.where(ks < 100, 1, np.where(ks < 150, 3, 2)))
    Ta = scattered(rng, ks + 5000, np.where(ks < 150, 1, 2))
    gs, gt = X.group_index(Sa), X.group_index(Ta)
    (ts, rs), (tt, rt) = nested_table(ctx, Sa, 256), nested_table(ctx, Ta, 157)
    return {"gs": gs, "gt": gt, "ts": ts, "tt": tt, "rels": (rs, rt), "refs_s": key_refs(ctx, ts, gs.keys),
            "refs_t": key_refs(ctx, tt, gt.keys), "n_mains": (len(gs), len(gt))}


def staging_keys(which):
    """(key_s, key_t) per input triple. Products: S key < 100 with T key < 5150: 1; S key 100..149: 3."""
    one = [(k % 100, 5000 + (7 * k) % 150) for k in range(4000)]
    three = (120, 5003)
    if which == "staged_2048":
        return one[:2048]
    if which == "unstaged_2049":
        return one[:2047] + [(None, 5001)] + one[2047:2048]
    dead = [(None, 5000 + k % 200) if k % 3 == 0 else (k % 200, None) if k % 3 == 1 else (None, None) for k in range(5000)]
    rng = np.random.default_rng(202)
    tail = [(int(s), 5000 + int(t)) for s, t in zip(rng.integers(0, 200, 3001), rng.integers(0, 200, 3001))]
    return [three] + dead + [three] + tail


@pytest.mark.parametrize("which", ["staged_2048", "unstaged_2049", "dead_run"])
def test_unnest2_slot_staging_boundary(ctx, small_st, which):
    c = small_st
    keys = staging_keys(which)
    key_s, key_t = [k[0] for k in keys], [k[1] for k in keys]
    a = np.arange(len(keys), dtype=np.uint32) * 3 + 1
    cs, ct = X.triple_counts(key_s, key_t, c["gs"], c["gt"])
    prod = cs * ct
    nq = chunk_slots(prod)
    if which == "staged_2048":  # the largest chunk that still stages its slot offsets in LDS
        assert nq.tolist() == [UN2_CHUNK_SLOTS] and int(prod.sum()) == UN2_CHUNK and (prod == 1).all()
    elif which == "unstaged_2049":  # one slot more: the search goes to the scanned offsets in HBM
        assert nq.tolist() == [UN2_CHUNK_SLOTS + 1] and int(prod.sum()) == UN2_CHUNK
    else:
        assert prod[0] == 3 and not prod[1:5001].any() and prod[5001] == 3
        assert nq[0] > UN2_CHUNK_SLOTS and (nq[1:] <= UN2_CHUNK_SLOTS).all() and len(nq) >= 3
        assert int(prod.sum()) % UN2_CHUNK  # the last chunk ends before its 2048th output
        assert {1, 2, 3, 4, 6} <= set(prod.tolist())
    trip = unnest2_input(a, key_s, key_t, c["refs_s"], c["refs_t"], c["n_mains"])
    want = X.expand_triples(a, key_s, key_t, c["gs"], c["gt"])
    assert_unnest2_exact(ctx, c["ts"], c["tt"], trip, want, X.triple_counters(key_s, key_t, c["gs"], c["gt"]))


@pytest.fixture(scope="module")
def rounds_case(ctx):
    """Case e: groups of 20 to 60 rows on two attributes and two geometries plus one 3000 x 1000 pair
    of groups, as many input triples as give 2.25 grid rounds of k_un2_expand."""
    n_cus = cus()
    need = math.ceil(2.25 * un2_round(n_cus))
    rng = np.random.default_rng(301)
    ks, kt = np.arange(200, dtype=np.uint32), np.arange(180, dtype=np.uint32) + 9000
    HOT_S, HOT_T = 777, 9777
    Sa = scattered(rng, np.concatenate([ks, [HOT_S]]), np.concatenate([rng.integers(20, 61, len(ks)), [3000]]))
    Ta = scattered(rng, np.concatenate([kt, [HOT_T]]), np.concatenate([rng.integers(20, 61, len(kt)), [1000]]))
    gs, gt = X.group_index(Sa), X.group_index(Ta)
    (ts, rs), (tt, rt) = nested_table(ctx, Sa, 2500), nested_table(ctx, Ta, 1237)
    m = 16000
    x = rng.integers(0, 210, m).tolist()  # 200..209: no S group
    y = (rng.integers(0, 190, m) + 9000).tolist()  # 9180..9189: no T group
    x[1500], y[1500] = HOT_S, HOT_T
    refs_s = key_refs(ctx, ts, np.concatenate([gs.keys, np.arange(200, 210, dtype=np.uint32)]))
    refs_t = key_refs(ctx, tt, np.concatenate([gt.keys, np.arange(9180, 9190, dtype=np.uint32)]))
    cs, ct = X.triple_counts(np.array(x), np.array(y), gs, gt)
    run = np.cumsum(cs * ct)
    assert run[-1] >= need, "not enough candidate triples for this chip"
    n = max(int(np.searchsorted(run, need)) + 1, 1501)
    x, y = np.array(x[:n]), np.array(y[:n])
    a = np.arange(n, dtype=np.uint32)
    prod = (cs * ct)[:n]
    total = int(prod.sum())
    assert total >= need > 2 * un2_round(n_cus)  # every workgroup takes a second chunk, a quarter of them a third
    assert prod[1500] == 3000 * 1000 and (prod == 0).any()
    trip = unnest2_input(a, x.tolist(), y.tolist(), refs_s, refs_t, (len(gs), len(gt)))
    want = X.expand_triples(a, x, y, gs, gt)
    assert len(want) == total
    return {"ts": ts, "tt": tt, "rels": (rs, rt), "trip": trip, "total": total, "cs": X.triple_checksums(want),
            "want_sorted": np.sort(X.pack_triples(want)), "counters": X.triple_counters(x, y, gs, gt)}


def test_unnest2_third_grid_round(ctx, rounds_case):
    c = rounds_case
    total = c["total"]
    buf = canary_buffer(total, 3)
    got = ctx.unnest2(c["ts"], c["tt"], c["trip"], out=buf[:total])
    assert got["overflow"] is False
    assert {k: got[k] for k in c["counters"]} == c["counters"]
    assert all(got[k] == 0 for k in PROBE2_ZERO)
    assert {k: got[k] for k in SUMS} == {k: c["cs"][k] for k in SUMS}
    assert tail_intact(buf, total)
    assert np.array_equal(np.sort(X.pack_triples(host(buf[:total]))), c["want_sorted"])  # no loss, no duplicate


@pytest.mark.parametrize("where", ["chunk", "chunk_plus_1", "mid", "total_minus_1"])
def test_unnest2_capacity_across_rounds(ctx, rounds_case, where):
    c = rounds_case
    total = c["total"]
    cap = {"chunk": UN2_CHUNK, "chunk_plus_1": UN2_CHUNK + 1, "mid": total // 2 + 777, "total_minus_1": total - 1}[where]
    assert 0 < cap < total
    if where == "mid":
        assert cap % UN2_CHUNK and cap > un2_round(cus())  # inside a chunk of the second grid round
    buf = canary_buffer(total, 3)
    got = ctx.unnest2(c["ts"], c["tt"], c["trip"], out=buf[:cap])
    assert got["overflow"] is True
    assert {k: got[k] for k in c["counters"]} == c["counters"]  # complete: every triple is counted
    assert {k: got[k] for k in SUMS} == {k: c["cs"][k] for k in SUMS}
    assert tail_intact(buf, cap)
    assert X.is_sub_multiset(X.pack_triples(host(buf[:cap])), c["want_sorted"])


def test_unnest2_product_beyond_32_bits(ctx):
    """One pair of groups of 65,600 x 65,600 rows: the triple index k inside the slot passes 2^32, where
    k_un2_expand splits it with 64-bit arithmetic (unnest2.hip:61-67). sum_b and sum_c both move if
    k / |S|, k % |S| is wrong there. Counters against the analytic form (no enumeration)."""
    HOT = 65_600
    rng = np.random.default_rng(401)
    small = np.arange(50, dtype=np.uint32)
    Sa = scattered(rng, np.concatenate([small, [900]]), np.concatenate([rng.integers(1, 6, 50), [HOT]]))
    Ta = scattered(rng, np.concatenate([small + 100, [901]]), np.concatenate([rng.integers(1, 6, 50), [HOT]]))
    gs, gt = X.group_index(Sa), X.group_index(Ta)
    assert HOT * HOT == 4_303_360_000 and HOT * HOT - (1 << 32) > 8_000_000
    (ts, _rs), (tt, _rt) = nested_table(ctx, Sa, 64), nested_table(ctx, Ta, 51)
    # a small live triple, the hot one, a small live one: the hot slot's offset is not 0 and a slot follows it
    key_s, key_t = [7, 900, 31], [107, 901, 131]
    a = np.array([0xFFFF_FF01, 0xFFFF_FF02, 0xFFFF_FF03], dtype=np.uint32)
    parts = [X.analytic_pair_of_groups(a[i], gs.rows(key_s[i]), gt.rows(key_t[i])) for i in range(3)]
    assert parts[0]["c_top"] > 0 and parts[2]["c_top"] > 0 and parts[1]["c_top"] == HOT * HOT >= 1 << 32
    want = X.add_counters(*parts)
    trip = unnest2_input(a, key_s, key_t, key_refs(ctx, ts, gs.keys), key_refs(ctx, tt, gt.keys), (len(gs), len(gt)))
    got = ctx.unnest2(ts, tt, trip, checksum=False)
    assert got["overflow"] is False and (got["sum_h"], got["xor_h"]) == (0, 0)
    assert {k: got[k] for k in want} == want
    cap = 4096
    buf = canary_buffer(cap, 3)
    low = ctx.unnest2(ts, tt, trip, out=buf[:cap], checksum=False)
    assert low["overflow"] is True
    assert {k: low[k] for k in want} == want
    assert tail_intact(buf, cap)
    h = host(buf[:cap])
    assert len(np.unique(h, axis=0)) == cap  # distinct
    member = np.zeros(cap, dtype=bool)
    for i in range(3):
        m = h[:, 0] == a[i]
        member |= m & np.isin(h[:, 1], gs.rows(key_s[i])) & np.isin(h[:, 2], gt.rows(key_t[i]))
    assert member.all()  # every written triple belongs to its tuple's product


# ---- g: hj3d_probe2's heavy kernels beyond two items per workgroup ----
SKEW_NB = 1536


@pytest.fixture(scope="module")
def many_heavy():
    """test_gpu_exp4_emit's skew mix with 9 * CUs + 37 keys of the first heavy product, 9 x 8 = 72."""
    n_cus = cus()
    K = 9 * heavy_groups(n_cus) // 4 + 37
    mult = {5: (8, 8), 6: (8, 8), 7: (8, 8), 11: (600, 70), 13: (1, 300), 17: (50, 0)}
    mult.update({k: (1, 2) for k in range(1024, 1536)})
    mult.update({k: (9, 8) for k in range(10_000, 10_000 + K)})
    rng = np.random.default_rng(501)
    ks = np.array(list(mult), dtype=np.uint32)
    Sa = scattered(rng, ks, [m[0] for m in mult.values()])
    Ta = scattered(rng, ks, [m[1] for m in mult.values()])
    Rk = rng.permutation(np.concatenate([ks, np.arange(20, 120, dtype=np.uint32)]))  # 100 keys find nothing
    nR = len(Rk)
    cs, ct = X.triple_counts(Rk, Rk, Sa, Ta)
    prod = cs * ct
    n_heavy = int((prod > INLINE2).sum())
    assert n_heavy == K + 2 > 2 * heavy_groups(n_cus)  # some workgroups take a third item: sbase[0] is reused
    assert (prod == INLINE2).sum() == 3 and (prod == 72).sum() == K
    want = X.expand_triples(np.arange(nR, dtype=np.uint32), Rk, Rk, Sa, Ta)
    Rh, Sh, Th = (O.tuples2(Rk, np.zeros(nR, np.uint32)), O.tuples2(np.arange(len(Sa), dtype=np.uint32), Sa),
                  O.tuples2(np.arange(len(Ta), dtype=np.uint32), Ta))
    orc = {plan: O.exp4_plan(Rh, Sh, Th, SKEW_NB, plan == "Ndu") for plan in ("Ndu", "Chj")}
    return {"host": (Rh, Sh, Th), "want_sorted": np.sort(X.pack_triples(want)), "total": len(want), "oracle": orc,
            "light_total": int(prod[prod <= INLINE2].sum()), "cs": X.triple_checksums(want)}


@pytest.mark.parametrize("path", ["default", "partitioned"])
@pytest.mark.parametrize("plan", ["Ndu", "Chj"])
def test_probe2_more_than_two_rounds_of_heavy_items(ctx, many_heavy, plan, path):
    import hj3d
    c = many_heavy
    total, orc = c["total"], c["oracle"][plan]
    assert orc["c_top"] == total and orc["out"] == c["cs"]
    R, S, T = (dev(r) for r in c["host"])
    kind = hj3d.HJ3D_NESTED if plan == "Ndu" else hj3d.HJ3D_CHAIN
    ts, tt = hj3d.Table(ctx, kind, SKEW_NB), hj3d.Table(ctx, kind, SKEW_NB)
    rel = hj3d.Rel(R, key_word=0)
    cap = total // 2 + 5
    assert c["light_total"] < cap < total - c["light_total"] and cap % 72  # the cut falls into heavy items
    full, low = canary_buffer(total, 3), canary_buffer(cap, 3)
    with on_path(ctx, path):
        ctx.build_many([ts, tt], [hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)])
        for t in (ts, tt):
            bp = t.build_path()
            assert bp.startswith("nested_") if plan == "Ndu" else bp in ("radix", "direct"), bp
        got = ctx.probe2(ts, tt, rel, out=full[:total])
        count = ctx.probe2(ts, tt, rel)
        cut = ctx.probe2(ts, tt, rel, out=low[:cap])
    assert got["overflow"] is False and count["overflow"] is False and cut["overflow"] is True
    for r in (got, count, cut):  # c_top and the checksums count every triple, written or not
        compare_counters(plan, r, orc, orc["out"])
    assert tail_intact(full, total) and tail_intact(low, cap)
    assert np.array_equal(np.sort(X.pack_triples(host(full[:total]))), c["want_sorted"])  # no loss, no duplicate
    keys = X.pack_triples(host(low[:cap]))
    assert len(np.unique(keys)) == cap, "written triples repeat"
    assert X.is_sub_multiset(keys, c["want_sorted"]), "a written triple is not in the result"
    ts.close()
    tt.close()
