"""tests/expand_ref.py (the numpy reference of the expansion operators) against the reference binary's
experiment-4 fixtures, the oracle's unnested Nrs plan and a hand-enumerated example, on the CPU: the
helper is pinned before tests/test_gpu_expand_limits.py judges a kernel with it."""
import numpy as np
import pytest

import expand_ref as X
import oracle as O
from conftest import load_golden

EXP4 = dict(load_golden("exp4_*.json", headline=False))
WITH_COLUMNS = ("exp4_R3_a2_A2_b2_B1", "exp4_R10_a3_A2_b2_B3")


def test_group_index_rows_ascend():
    keys = np.array([7, 3, 7, 9, 3, 7], dtype=np.uint32)
    g = X.group_index(keys)
    assert len(g) == 3
    assert g.rows(7).tolist() == [0, 2, 5] and g.rows(3).tolist() == [1, 4] and g.rows(9).tolist() == [3]
    assert g.rows(8).tolist() == []
    first, cnt = g.locate(np.array([9, 8, 3, -1, 2 ** 32 - 1]))
    assert cnt.tolist() == [1, 0, 2, 0, 0]
    assert g.order[first[2]: first[2] + 2].tolist() == [1, 4]


def test_expand_by_hand():
    Sa = np.array([5, 6, 5, 8], dtype=np.uint32)
    Ta = np.array([6, 5, 5, 5], dtype=np.uint32)
    a = [10, 11, 12, 13]
    pairs = X.expand_pairs(a, [5, None, 7, 8], Sa)
    assert pairs.tolist() == [[10, 0], [10, 2], [13, 3]]
    assert X.pair_counters(a, [5, None, 7, 8], Sa) == {"n_probe": 4, "n_matched": 2, "n_out": 3}
    trip = X.expand_triples(a, [5, 6, None, 8], [5, None, 5, 6], Sa, Ta)
    # tuple 10: S rows {0, 2} x T rows {1, 2, 3}, the S row changing fastest; tuple 13: {3} x {0}
    assert trip.tolist() == [[10, 0, 1], [10, 2, 1], [10, 0, 2], [10, 2, 2], [10, 0, 3], [10, 2, 3], [13, 3, 0]]
    assert X.triple_counters([5, 6, None, 8], [5, None, 5, 6], Sa, Ta) == {"c_unnest_1": 4, "c_unnest_2": 7, "c_top": 7}
    # a key with S rows but no T row is skipped by both counters
    assert X.triple_counters([5], [9], Sa, Ta) == {"c_unnest_1": 0, "c_unnest_2": 0, "c_top": 0}
    assert X.expand_triples([1], [5], [9], Sa, Ta).shape == (0, 3)
    # integer key arrays: negative = dead
    assert np.array_equal(X.expand_pairs(a, np.array([5, -1, 7, 8]), Sa), pairs)


def test_checksums_equal_the_scalar_definitions():
    import hj3d
    rng = np.random.default_rng(3)
    t = rng.integers(0, 1 << 32, (257, 3), dtype=np.uint64).astype(np.uint32)
    cs = X.triple_checksums(t)
    hs = [hj3d.triple_hash(int(r[0]), int(r[1]), int(r[2])) for r in t]
    x = 0
    for h in hs:
        x ^= h
    assert cs == {"n": 257, "sum_a": int(t[:, 0].astype(np.uint64).sum()), "sum_b": int(t[:, 1].astype(np.uint64).sum()),
                  "sum_c": int(t[:, 2].astype(np.uint64).sum()), "sum_h": sum(hs) & X.M64, "xor_h": x}
    assert cs == hj3d.triple_checksums(t)
    ps = [hj3d.pair_hash(int(r[0]), int(r[1])) for r in t]
    x = 0
    for h in ps:
        x ^= h
    pc = X.pair_checksums(t[:, :2])
    assert (pc["sum_h"], pc["xor_h"], pc["sum_c"], pc["n"]) == (sum(ps) & X.M64, x, 0, 257)
    assert X.pair_checksums(t[:0, :2]) == {"n": 0, "sum_a": 0, "sum_b": 0, "sum_c": 0, "sum_h": 0, "xor_h": 0}


@pytest.mark.parametrize("name", WITH_COLUMNS)
def test_expand_triples_reproduces_exp4_fixture(name):
    g = EXP4[name]
    ref = g["plans"]["Ndu"]
    Rk = np.arange(g["cardR"], dtype=np.uint32)
    Sa, Ta = np.array(g["Sa"], dtype=np.uint32), np.array(g["Ta"], dtype=np.uint32)
    gen_Sa, gen_Ta = O.gen_exp4(*g["generator_args"][1:6])
    assert np.array_equal(Sa, gen_Sa) and np.array_equal(Ta, gen_Ta)
    trip = X.expand_triples(Rk, Rk, Rk, Sa, Ta)
    assert X.triple_checksums(trip) == ref["out"]
    assert X.triple_counters(Rk, Rk, Sa, Ta) == {k: ref[k] for k in ("c_unnest_1", "c_unnest_2", "c_top")}
    assert len(np.unique(X.pack_triples(trip))) == len(trip)


def test_expand_pairs_reproduces_oracle_unnest():
    rng = np.random.default_rng(11)
    nR, nS = 3000, 40_000
    Rk = rng.permutation(nR + 500)[:nR].astype(np.uint32)  # some probe keys have no build row
    Sa = np.minimum(rng.zipf(1.3, nS) - 1, nR - 1).astype(np.uint32)
    R, S = O.tuples3(Rk, np.zeros(nR, np.uint32)), O.tuples3(np.arange(nS, dtype=np.uint32), Sa)
    exp = O.nested_plan(S, 1, R, 0, O.num_distinct(Sa), True)
    a = np.arange(nR, dtype=np.uint32)
    pairs = X.expand_pairs(a, Rk, Sa)
    assert X.pair_checksums(pairs) == exp.out
    assert X.pair_counters(a, Rk, Sa) == {"n_probe": nR, "n_matched": exp.c_probe, "n_out": exp.c_unnest}
    assert exp.c_unnest == exp.out["n"] > nR


def test_analytic_pair_of_groups_equals_enumeration():
    rng = np.random.default_rng(5)
    nS, nT = 20_000, 30_000
    Sa = rng.integers(100, 2000, nS).astype(np.uint32)
    Ta = rng.integers(100, 2000, nT).astype(np.uint32)
    Sa[rng.choice(nS, 300, replace=False)] = 11
    Ta[rng.choice(nT, 400, replace=False)] = 23
    gs, gt = X.group_index(Sa), X.group_index(Ta)
    a = 0xFFFF_FFF0  # sum_a = a * 120,000 needs more than 32 bits
    trip = X.expand_triples([a], [11], [23], gs, gt)
    assert len(trip) == 300 * 400
    cs = X.triple_checksums(trip)
    an = X.analytic_pair_of_groups(a, gs.rows(11), gt.rows(23))
    assert an == {"c_top": cs["n"], "c_unnest_1": 400, "c_unnest_2": cs["n"], "sum_a": cs["sum_a"],
                  "sum_b": cs["sum_b"], "sum_c": cs["sum_c"]}
    assert an == {**X.triple_counters([11], [23], gs, gt), **{k: cs[k] for k in ("sum_a", "sum_b", "sum_c")}}
    # sums wrap mod 2^64 like the device's u64 accumulators
    big = X.analytic_pair_of_groups(0xFFFFFFFF, np.full(1 << 16, 0xFFFFFFFF, np.uint32), np.full(1 << 17, 0xFFFFFFFE, np.uint32))
    assert big["sum_a"] == (0xFFFFFFFF << 33) & X.M64 and big["c_top"] == 1 << 33
    assert big["sum_b"] == ((1 << 17) * (1 << 16) * 0xFFFFFFFF) & X.M64
    dead = X.analytic_pair_of_groups(7, gs.rows(11), gt.rows(99_999))
    assert dead["c_top"] == dead["c_unnest_1"] == dead["sum_b"] == 0
    assert X.add_counters(an, an)["sum_b"] == (2 * an["sum_b"]) & X.M64


def test_packing_and_sub_multiset():
    t = np.array([[1, 2, 3], [1, 2, 3], [4, 5, 6]], dtype=np.uint32)
    full = np.sort(X.pack_triples(t))
    assert X.is_sub_multiset(X.pack_triples(t[:2]), full)
    assert X.is_sub_multiset(X.pack_triples(t[:0]), full)
    assert not X.is_sub_multiset(X.pack_triples(t[[2, 2]]), full)  # more often than in the result
    assert not X.is_sub_multiset(X.pack_triples(np.array([[1, 2, 4]], dtype=np.uint32)), full)
    with pytest.raises(AssertionError):
        X.pack_triples(np.array([[1 << 24, 0, 0]], dtype=np.uint32))
    p = np.array([[0xFFFFFFFF, 0xFFFFFFFE]], dtype=np.uint32)
    assert int(X.pack_pairs(p)[0]) == 0xFFFFFFFF_FFFFFFFE
