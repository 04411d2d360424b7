"""tests/tablestruct.py (the numpy reference of hj3d_table_export's structure) pinned to the oracle
and to a dictionary-based grouping, on the CPU, before tests/test_gpu_table_lifecycle.py lets it judge
a kernel: its HtStatistics equal O.chain_plan(...).stats / O.nested_plan(...).stats on every build
relation the GPU tests use and on the degenerate ones (empty relation, one tuple, NB = 1)."""
import collections

import numpy as np
import pytest

import oracle as O
import tablestruct as TS

PROBE = O.tuples3(np.arange(4, dtype=np.uint32), np.zeros(4, np.uint32))  # (the statistics do not depend on it)


def oracle_stats(kind, keys, nb):
    B = O.tuples3(np.arange(len(keys), dtype=np.uint32), np.asarray(keys, dtype=np.uint32))
    plan = O.chain_plan if kind == TS.CHAIN else O.nested_plan
    return plan(B, 1, PROBE, 0, nb, False).stats


def helper_stats(kind, keys, nb, lo=0, hi=None):
    rows = np.arange(len(keys), dtype=np.uint32)
    return (TS.chain_stats if kind == TS.CHAIN else TS.nested_stats)(keys, rows, nb, lo, hi)


@pytest.mark.parametrize("name", TS.SHAPES)
def test_statistics_equal_the_oracle_on_the_gpu_tests_shapes(name):
    kind, keys, nb = TS.shape(name)
    assert helper_stats(kind, keys, nb) == {k: oracle_stats(kind, keys, nb)[k] for k in TS.STAT_KEYS}


DEGENERATE = {
    "empty": (np.zeros(0, np.uint32), 7),
    "empty_nb1": (np.zeros(0, np.uint32), 1),
    "one_tuple": (np.array([0xFFFFFFFF], np.uint32), 5),
    "one_tuple_nb1": (np.array([3], np.uint32), 1),
    "nb1": (np.random.default_rng(3).integers(0, 50, 400, dtype=np.uint32), 1),
    "one_key": (np.full(100, 9, np.uint32), 3),
}


@pytest.mark.parametrize("kind", [TS.CHAIN, TS.NESTED], ids=["chain", "nested"])
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_statistics_equal_the_oracle_on_degenerate_relations(name, kind):
    keys, nb = DEGENERATE[name]
    assert helper_stats(kind, keys, nb) == {k: oracle_stats(kind, keys, nb)[k] for k in TS.STAT_KEYS}


@pytest.mark.parametrize("name", ["chain", "nested"])
def test_shard_statistics_follow_from_the_oracle_on_the_owned_tuples(name):
    """The oracle has no bucket ranges. A shard [lo, hi) of NB buckets stores the tuples of its buckets
    only, so every statistic that does not count the buckets outside the range equals the oracle's on
    those tuples alone (over all NB buckets, the others empty); `empty` differs by their number."""
    kind, keys, nb = TS.shape(name)
    lo, hi = nb // 3, nb - nb // 4
    b = (TS.fmix32(keys).astype(np.uint64) % np.uint64(nb)).astype(np.int64)
    e = oracle_stats(kind, keys[(b >= lo) & (b < hi)], nb)
    got = helper_stats(kind, keys, nb, lo, hi)
    same = ("entries", "distinct", "cc0_max", "cc0_sum", "cc1_min", "cc1_max", "cc1_sum", "cc1_cnt")
    assert {k: got[k] for k in same} == {k: e[k] for k in same}
    assert got["nb"] == got["cc0_cnt"] == hi - lo
    assert got["empty"] == e["empty"] - (nb - (hi - lo))


def test_structure_equals_a_dictionary_grouping():
    """chain_struct / nested_struct against the grouping written out with dictionaries: explicit
    ascending rows with gaps, duplicate keys, a bucket range inside [0, NB)."""
    rng = np.random.default_rng(11)
    n, nb, lo, hi = 3000, 97, 10, 80
    keys = rng.integers(0, 700, n, dtype=np.uint32)
    rows = np.sort(rng.choice(1 << 31, n, replace=False)).astype(np.uint32)
    buckets = collections.defaultdict(list)               # local bucket -> [(hash, row)] in scan order
    per_key = collections.defaultdict(list)               # (local bucket, hash) -> rows in scan order
    for k, r in zip(keys.tolist(), rows.tolist()):
        h = int(TS.fmix32(k))
        if lo <= h % nb < hi:
            buckets[h % nb - lo].append((h, r))
            per_key[(h % nb - lo, h)].append(r)
    c = TS.chain_struct(keys, rows, nb, lo, hi)
    assert c["off"].tolist() == [sum(len(buckets[b]) for b in range(k)) for k in range(hi - lo + 1)]
    assert c["ent"].tolist() == [list(e) for b in range(hi - lo) for e in sorted(buckets[b], key=lambda e: e[1])]
    s = TS.nested_struct(keys, rows, nb, lo, hi)
    ks = sorted(per_key)
    assert s["off"].tolist() == [sum(1 for b, _ in ks if b < k) for k in range(hi - lo + 1)]
    assert list(zip(s["bucket"].tolist(), s["hash"].tolist())) == ks
    assert s["first_row"].tolist() == [min(per_key[k]) for k in ks]
    assert s["sub_len"].tolist() == [len(per_key[k]) for k in ks]
    assert [r.tolist() for r in s["rows"]] == [sorted(per_key[k]) for k in ks]
    assert s["n_rows"] == sum(len(v) for v in per_key.values())
