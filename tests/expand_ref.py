"""What the expansion operators must produce, in plain numpy (a helper module for the tests, not a
conftest).

hj3d_unnest turns a stored nested tuple {a, main ref} into one pair {a, s_row} per build row of the
ref's group; hj3d_unnest2 and hj3d_probe2 turn {a, ref_s, ref_t} (or a probe key matching both
tables) into one triple {a, s_row, t_row} per pair of rows of the two groups. A group is "the build
rows with this key", so the expected output follows from the build relations' key columns and the
KEY of each input tuple alone: no table export, no main record, no library result. A tuple whose key
is None (or negative in an integer array) is dead; a key without build rows gives no output either.

Everything is vectorised; the checksums are the library's (pair_hash / triple_hash of
hj3d_device.hpp: splitmix64's finaliser over the packed rows), sums mod 2^64.
tests/test_expand_ref.py pins this module to the reference binary's fixtures and to the oracle before
it judges a kernel.

Host only (numpy)."""
import numpy as np

M64 = (1 << 64) - 1
NOREF = 0xFFFFFFFF


class Groups:
    """The build rows of every key of a key column: rows(k) ascending; first / count for key arrays."""

    def __init__(self, keys):
        keys = np.asarray(keys, dtype=np.uint32)
        self.order = np.argsort(keys, kind="stable").astype(np.int64)  # rows grouped by key, ascending inside
        self.keys, self.first, self.cnt = np.unique(keys[self.order], return_index=True, return_counts=True)
        self.first = self.first.astype(np.int64)
        self.cnt = self.cnt.astype(np.int64)

    def __len__(self):
        return len(self.keys)

    def locate(self, k, live=None):
        """(first, count) into `order` of the groups of keys k (int64 array); count 0 where the key
        has no build row or `live` is False."""
        k = np.asarray(k, dtype=np.int64)
        if len(self.keys) == 0:
            return np.zeros(len(k), np.int64), np.zeros(len(k), np.int64)
        pos = np.minimum(np.searchsorted(self.keys, k), len(self.keys) - 1)
        hit = self.keys[pos].astype(np.int64) == k
        if live is not None:
            hit &= live
        return np.where(hit, self.first[pos], 0), np.where(hit, self.cnt[pos], 0)

    def rows(self, key) -> np.ndarray:
        f, c = self.locate(np.array([key], dtype=np.int64))
        return self.order[f[0]: f[0] + c[0]].astype(np.uint32)


def group_index(keys) -> Groups:
    """Each key's build rows (row = position in `keys`) in ascending order."""
    return Groups(keys)


def _keys(key_of_tuple):
    """(int64 keys, live mask) of a sequence of keys in which None (or a negative value) is dead."""
    if isinstance(key_of_tuple, np.ndarray) and key_of_tuple.dtype != object:
        k = key_of_tuple.astype(np.int64)
    else:
        k = np.array([-1 if v is None else int(v) for v in key_of_tuple], dtype=np.int64)
    return k, k >= 0


def _within(cnt):
    """For counts c_0, c_1, ...: (index i of every output, its position 0 .. c_i - 1 inside i)."""
    total = int(cnt.sum())
    idx = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    first = np.cumsum(cnt) - cnt
    return idx, np.arange(total, dtype=np.int64) - first[idx]


def pair_counts(key_of_tuple, Sa) -> np.ndarray:
    """Output pairs per input tuple."""
    g = Sa if isinstance(Sa, Groups) else Groups(Sa)
    k, live = _keys(key_of_tuple)
    return g.locate(k, live)[1]


def expand_pairs(a, key_of_tuple, Sa) -> np.ndarray:
    """hj3d_unnest: {a, s_row} for every row s_row of S with S.a == the tuple's key, (n, 2) uint32 in
    input order, rows ascending inside a tuple."""
    g = Sa if isinstance(Sa, Groups) else Groups(Sa)
    a = np.asarray(a, dtype=np.uint32)
    k, live = _keys(key_of_tuple)
    assert len(a) == len(k)
    first, cnt = g.locate(k, live)
    idx, w = _within(cnt)
    out = np.empty((len(idx), 2), dtype=np.uint32)
    out[:, 0] = a[idx]
    out[:, 1] = g.order[first[idx] + w]
    return out


def triple_counts(key_s, key_t, Sa, Ta):
    """(|S group|, |T group|) per input tuple; both 0 unless both are non-empty (the tuple is skipped)."""
    gs = Sa if isinstance(Sa, Groups) else Groups(Sa)
    gt = Ta if isinstance(Ta, Groups) else Groups(Ta)
    ks, ls = _keys(key_s)
    kt, lt = _keys(key_t)
    cs, ct = gs.locate(ks, ls)[1], gt.locate(kt, lt)[1]
    ok = (cs > 0) & (ct > 0)
    return np.where(ok, cs, 0), np.where(ok, ct, 0)


def expand_triples(a, key_s, key_t, Sa, Ta) -> np.ndarray:
    """hj3d_unnest2 / hj3d_probe2: {a, s_row, t_row} for every pair of rows with S.a == key_s and
    T.a == key_t, (n, 3) uint32 in input order (inside a tuple: t_row major, s_row minor)."""
    gs = Sa if isinstance(Sa, Groups) else Groups(Sa)
    gt = Ta if isinstance(Ta, Groups) else Groups(Ta)
    a = np.asarray(a, dtype=np.uint32)
    ks, ls = _keys(key_s)
    kt, lt = _keys(key_t)
    assert len(a) == len(ks) == len(kt)
    fs, cs = gs.locate(ks, ls)
    ft, ct = gt.locate(kt, lt)
    idx, w = _within(cs * ct)
    out = np.empty((len(idx), 3), dtype=np.uint32)
    out[:, 0] = a[idx]
    ws = cs[idx]
    out[:, 1] = gs.order[fs[idx] + w % ws]
    out[:, 2] = gt.order[ft[idx] + w // ws]
    return out


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def _fold(cols, h) -> dict:
    d = {"n": int(len(h))}
    for name, c in zip(("sum_a", "sum_b", "sum_c"), cols + [None] * (3 - len(cols))):
        d[name] = 0 if c is None else int(c.sum(dtype=np.uint64))
    d["sum_h"] = int(h.sum(dtype=np.uint64))
    d["xor_h"] = int(np.bitwise_xor.reduce(h)) if len(h) else 0
    return d


def pair_checksums(pairs) -> dict:
    """{n, sum_a, sum_b, sum_c = 0, sum_h, xor_h} of (n, 2) pairs as the probe and hj3d_unnest fold them."""
    p = np.asarray(pairs)
    assert p.ndim == 2 and p.shape[1] == 2
    a, b = p[:, 0].astype(np.uint64), p[:, 1].astype(np.uint64)
    with np.errstate(over="ignore"):
        return _fold([a, b], _mix((a << np.uint64(32)) | b))


def triple_checksums(triples) -> dict:
    """{n, sum_a, sum_b, sum_c, sum_h, xor_h} of (n, 3) triples as hj3d_probe2 / hj3d_unnest2 fold them."""
    t = np.asarray(triples)
    assert t.ndim == 2 and t.shape[1] == 3
    a, b, c = (t[:, j].astype(np.uint64) for j in range(3))
    with np.errstate(over="ignore"):
        return _fold([a, b, c], _mix(_mix((a << np.uint64(32)) | b) ^ c))


def pair_counters(a, key_of_tuple, Sa) -> dict:
    """hj3d_unnest's counters: every input tuple is scanned, one with a group is matched."""
    cnt = pair_counts(key_of_tuple, Sa)
    return {"n_probe": len(cnt), "n_matched": int((cnt > 0).sum()), "n_out": int(cnt.sum())}


def triple_counters(key_s, key_t, Sa, Ta) -> dict:
    """The unnest counters of experiment 4's Ndu: the first unnest emits |T group| tuples per input
    tuple that has both groups, the second the whole product."""
    cs, ct = triple_counts(key_s, key_t, Sa, Ta)
    total = int((cs * ct).sum())
    return {"c_unnest_1": int(ct.sum()), "c_unnest_2": total, "c_top": total}


def analytic_pair_of_groups(a, s_rows, t_rows) -> dict:
    """One input tuple {a, S group, T group} without enumerating the product, in Python integers
    mod 2^64: every triple carries a, every S row occurs |T| times and every T row |S| times."""
    ns, nt = len(s_rows), len(t_rows)
    sum_s = sum(int(v) for v in np.asarray(s_rows).tolist())
    sum_t = sum(int(v) for v in np.asarray(t_rows).tolist())
    live = ns > 0 and nt > 0
    return {"c_top": ns * nt, "c_unnest_1": nt if live else 0, "c_unnest_2": ns * nt,
            "sum_a": (int(a) * ns * nt) & M64, "sum_b": (nt * sum_s) & M64, "sum_c": (ns * sum_t) & M64}


def add_counters(*parts) -> dict:
    """Counters and row sums of several inputs together (mod 2^64)."""
    out = {}
    for p in parts:
        for k, v in p.items():
            out[k] = (out.get(k, 0) + v) & M64
    return out


def pack_pairs(pairs) -> np.ndarray:
    """One u64 per pair: a << 32 | row (exact)."""
    p = np.asarray(pairs)
    return (p[:, 0].astype(np.uint64) << np.uint64(32)) | p[:, 1].astype(np.uint64)


def pack_triples(triples, bits=(24, 20, 20)) -> np.ndarray:
    """One u64 per triple: a | s_row | t_row in bit fields of the given widths (asserted to fit), so a
    multiset of millions of triples sorts as integers."""
    t = np.asarray(triples)
    assert sum(bits) <= 64
    for j in range(3):
        assert len(t) == 0 or int(t[:, j].max()) < (1 << bits[j]), (j, bits)
    u = t.astype(np.uint64)
    return (u[:, 0] << np.uint64(bits[1] + bits[2])) | (u[:, 1] << np.uint64(bits[2])) | u[:, 2]


def is_sub_multiset(part_keys, full_sorted) -> bool:
    """Every packed key of `part_keys` occurs in the sorted key array `full_sorted` at least as often."""
    ku, cu = np.unique(np.asarray(part_keys, dtype=np.uint64), return_counts=True)
    lo = np.searchsorted(full_sorted, ku, "left")
    hi = np.searchsorted(full_sorted, ku, "right")
    return bool((cu <= hi - lo).all())
