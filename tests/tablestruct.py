"""The table structure hj3d_table_export promises, in plain numpy (a helper module for the tests, not
a conftest).

"Group the build tuples by bucket and key", nothing else: h = fmix32(key), bucket = h % NB, a table of
the bucket range [lo, hi) stores the tuples with lo <= bucket < hi under local bucket = bucket - lo.
  chaining: off = CSR offsets of the stored tuples per local bucket, entries {h, row} ordered by
            (local bucket, row);
  nested:   off = CSR offsets of the distinct stored keys per local bucket, and per key its hash, its
            first row (the smallest: build rows ascend in scan order), its tuple count and its rows.
HtStatistics (ht_statistics.hh:18-54) follow from `off` and the stored tuples' hashes alone.
tests/test_tablestruct.py pins these statistics to the oracle's before the helper judges a kernel.

Host only (numpy)."""
import functools
import zlib

import numpy as np

from keyspace import fmix32  # noqa: F401  (re-exported: the tests hash with the same function)

STAT_KEYS = ("nb", "empty", "entries", "distinct", "cc0_min", "cc0_max", "cc0_sum", "cc0_cnt",
             "cc1_min", "cc1_max", "cc1_sum", "cc1_cnt")
U64_MAX = (1 << 64) - 1


def owned(keys, rows, nb, lo=0, hi=None):
    """(h, row, local bucket) of the tuples a table of buckets [lo, hi) stores, in scan order."""
    hi = nb if hi is None else hi
    keys = np.asarray(keys, dtype=np.uint32)
    rows = np.asarray(rows, dtype=np.uint32)
    h = fmix32(keys)
    b = (h.astype(np.uint64) % np.uint64(nb)).astype(np.int64)
    m = (b >= lo) & (b < hi)
    return h[m], rows[m], b[m] - lo


def _csr(local, nb_local):
    return np.concatenate([[0], np.cumsum(np.bincount(local, minlength=nb_local))]).astype(np.int64)


def chain_struct(keys, rows, nb, lo=0, hi=None):
    """{"off": int64[nb_local + 1], "ent": uint32 (n, 2) = {h, row} ordered by (local bucket, row)}."""
    hi = nb if hi is None else hi
    h, r, local = owned(keys, rows, nb, lo, hi)
    order = np.lexsort((r, local))
    return {"off": _csr(local, hi - lo), "ent": np.stack([h[order], r[order]], axis=1).astype(np.uint32)}


def nested_struct(keys, rows, nb, lo=0, hi=None):
    """{"off": int64[nb_local + 1] over the distinct keys, "bucket", "hash", "first_row", "sub_len": one
    value per key, ordered by (local bucket, hash), "rows": per key its rows, ascending, "n_rows": the
    stored tuples}."""
    hi = nb if hi is None else hi
    h, r, local = owned(keys, rows, nb, lo, hi)
    order = np.lexsort((r, h, local))  # equal hashes are equal keys (fmix32 is a bijection): one bucket
    h, r, local = h[order], r[order], local[order]
    head = np.ones(len(h), dtype=bool)
    head[1:] = h[1:] != h[:-1]
    start = np.nonzero(head)[0]
    end = np.append(start[1:], len(h))
    return {"off": _csr(local[start], hi - lo), "bucket": local[start], "hash": h[start].astype(np.uint32),
            "first_row": r[start].astype(np.uint32), "sub_len": (end - start).astype(np.int64),
            "rows": [r[a:b] for a, b in zip(start, end)], "n_rows": len(h)}


def stats_from(off, hashes):
    """HtStatistics of a table whose CSR offsets are `off` and whose stored tuples have `hashes` (one
    per tuple; a nested export gives them as its main hashes repeated sub_len times). Chain length =
    diff(off): entries per bucket (chaining) or distinct keys per bucket (nested)."""
    off = np.asarray(off, dtype=np.int64)
    hashes = np.asarray(hashes, dtype=np.uint32)
    ln = np.diff(off)
    nz = ln[ln > 0]
    return {"nb": len(ln), "empty": int((ln == 0).sum()), "entries": len(hashes), "distinct": len(np.unique(hashes)),
            "cc0_min": int(ln.min()) if len(ln) else U64_MAX, "cc0_max": int(ln.max()) if len(ln) else 0,
            "cc0_sum": int(ln.sum()), "cc0_cnt": len(ln),
            "cc1_min": int(nz.min()) if len(nz) else U64_MAX, "cc1_max": int(nz.max()) if len(nz) else 0,
            "cc1_sum": int(nz.sum()), "cc1_cnt": len(nz)}


# ---- the build relations of tests/test_gpu_table_lifecycle.py (test_tablestruct.py pins the helper
# to the oracle on the same ones) ----
N_R, N_S = 100_000, 400_000  # the sizes of the nested path tests (test_nested_agg_build_vs_oracle)
CHAIN, NESTED = 0, 1         # hj3d.HJ3D_CHAIN / HJ3D_NESTED


@functools.lru_cache(maxsize=None)
def shape(name):
    """(kind, build keys, NB) of a named build relation; rows are implicit (the index)."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "chain":      # ~4 entries per bucket, one key with ~1 % of the rows (a bucket above 32)
        k = rng.integers(0, N_R, N_S, dtype=np.uint32)
        k[rng.random(N_S) < 0.01] = 12345
        return CHAIN, k, 100_000
    if name == "chain_small":  # 2e4 tuples of other keys than "chain" / "chain_big"
        k = rng.integers(1 << 20, (1 << 20) + 5_000, 20_000, dtype=np.uint32)
        k[rng.random(20_000) < 0.01] = 777
        return CHAIN, k, 100_000
    if name == "chain_big":    # 3e5 tuples
        k = rng.integers(0, 200_000, 300_000, dtype=np.uint32)
        k[rng.random(300_000) < 0.01] = 4242
        return CHAIN, k, 100_000
    if name in ("slices", "slices_hot", "slices_fill13"):
        # fill 1.0 (1.3: fine regions beyond the slice build's register-held form) over 2^20 buckets,
        # random u32 keys and one hot key. "slices_hot": the key carries
        # ~5 % of the rows (test_slice_build_large_slices_vs_oracle's shape), which overflows the
        # slice partitioner's regions, so the direct build replaces the slice build. "slices": ~0.05 %
        # (~500 rows, ~4 per 8192-tuple tile: inside the 8-sigma slack of the partitioner's regions,
        # which ~0.25 % already overflowed), which the slice build keeps.
        n = int((1 << 20) * (1.3 if name == "slices_fill13" else 1.0))
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        k[rng.random(n) < (0.05 if name == "slices_hot" else 0.0005)] = 12345
        return CHAIN, k, 1 << 20
    if name == "fused":      # key/FK at fill 1 (test_fused_partition_chaining_build's smallest), 40 rows of one key
        n = 1_000_003
        k = rng.permutation(n).astype(np.uint32)
        k[rng.choice(n, 40, replace=False)] = 99
        return CHAIN, k, n
    if name == "nested":       # ~5 keys per bucket
        return NESTED, rng.integers(0, N_R, N_S, dtype=np.uint32), 20_000
    if name == "nested_other":  # as "nested", other keys
        return NESTED, rng.integers(50_000, 50_000 + N_R, N_S, dtype=np.uint32), 20_000
    if name == "nested_small":
        return NESTED, rng.integers(0, 9_000, 30_000, dtype=np.uint32), 20_000
    if name == "nested_giveup":  # GiveUpData's shape: ~50 keys per bucket, the aggregation build gives up
        return NESTED, rng.integers(0, N_R, N_S, dtype=np.uint32), 2_000
    if name in ("nested2k", "nested2k_other"):  # ~4 keys per bucket over nested_giveup's 2 000 buckets
        base = 0 if name == "nested2k" else 5_000
        return NESTED, rng.integers(base, base + 8_000, N_S, dtype=np.uint32), 2_000
    if name == "nested_reg":   # test_nested_slices_register_form, keys_per_bucket = 1
        return NESTED, rng.integers(0, 100_000, 600_000, dtype=np.uint32), 100_000
    raise KeyError(name)


SHAPES = ("chain", "chain_small", "chain_big", "slices", "slices_hot", "slices_fill13", "fused", "nested", "nested_other",
          "nested_small", "nested_giveup", "nested2k", "nested2k_other", "nested_reg")


def chain_stats(keys, rows, nb, lo=0, hi=None):
    s = chain_struct(keys, rows, nb, lo, hi)
    return stats_from(s["off"], s["ent"][:, 0])


def nested_stats(keys, rows, nb, lo=0, hi=None):
    s = nested_struct(keys, rows, nb, lo, hi)
    return stats_from(s["off"], np.repeat(s["hash"], s["sub_len"]))
