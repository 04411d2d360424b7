"""What hj3d_unnestn must produce, in plain numpy (a helper module for the tests, not a conftest): the
k-table form of tests/expand_ref.py, whose `Groups` it reuses.

hj3d_unnestn turns a stored nested tuple {a, ref_1 .. ref_k} into one row {a, row_1 .. row_k} per
combination of rows of the k groups. A group is "the build rows with this key", so the expected output
follows from the k build key columns and the k KEYS of each input tuple alone: no table export, no
main record, no library result. A tuple with a dead key (None, or negative in an integer array) or a
key without build rows in any position gives no output.

Counters in the reference's order (the last table probed is unnested first, main_experiment4.cc:435-466):
c_unnest[j] = sum over the live tuples of |G_k| * .. * |G_{k-j}|, c_top = c_unnest[k - 1]. Checksums:
h = pair(a, row_1), then h = mix64(h ^ row_i) for i = 2..k (hj3d_device.hpp), sums mod 2^64.
tests/test_expand_n_ref.py pins this module to expand_ref and to the experiment-4 fixtures.

Host only (numpy)."""
import numpy as np

from expand_ref import M64, Groups, _keys, _mix, _within


def _groups(cols):
    return [c if isinstance(c, Groups) else Groups(c) for c in cols]


def locate_n(keys, cols):
    """([first_i], [count_i]) per table for the per-tuple key arrays keys[i]; every count of a tuple
    is 0 unless all of its k groups are non-empty (the tuple is skipped)."""
    gs = _groups(cols)
    assert len(keys) == len(gs) >= 1
    fc = []
    for k_i, g in zip(keys, gs):
        k, live = _keys(k_i)
        fc.append(g.locate(k, live))
    ok = np.ones(len(fc[0][1]), dtype=bool)
    for _, c in fc:
        ok &= c > 0
    return [f for f, _ in fc], [np.where(ok, c, 0) for _, c in fc]


def counters(keys, cols) -> dict:
    """{n_in, n_live, c_unnest (list of k), c_top} in Python integers (exact at any magnitude)."""
    _, cnt = locate_n(keys, cols)
    k = len(cnt)
    c = [x.astype(object) for x in cnt]  # Python integers: no wrap
    n = len(c[0])
    c_unnest = []
    part = (cnt[0] > 0).astype(np.int64).astype(object)  # live tuples start at 1
    for j in range(k):
        part = part * c[k - 1 - j]
        c_unnest.append(int(part.sum()) if n else 0)
    return {"n_in": n, "n_live": int((cnt[0] > 0).sum()), "c_unnest": c_unnest, "c_top": c_unnest[-1]}


def expand_rows(a, keys, cols) -> np.ndarray:
    """{a, row_1 .. row_k} for every combination of rows, (n_out, k + 1) uint32 in input order; inside
    a tuple group 1 is the fastest digit, rows ascending inside a group."""
    gs = _groups(cols)
    a = np.asarray(a, dtype=np.uint32)
    first, cnt = locate_n(keys, gs)
    prod = np.ones(len(a), dtype=np.int64)
    for c in cnt:
        prod = prod * c
    idx, w = _within(prod)
    out = np.empty((len(idx), len(gs) + 1), dtype=np.uint32)
    out[:, 0] = a[idx]
    for i, g in enumerate(gs):
        ci = cnt[i][idx]
        out[:, 1 + i] = g.order[first[i][idx] + w % ci]
        w = w // ci
    return out


def row_checksums(rows) -> dict:
    """{n, sum_a, sum_row (list of k), sum_h, xor_h} of (n, k + 1) rows as hj3d_unnestn folds them."""
    r = np.asarray(rows)
    assert r.ndim == 2 and r.shape[1] >= 2
    u = [r[:, j].astype(np.uint64) for j in range(r.shape[1])]
    with np.errstate(over="ignore"):
        h = _mix((u[0] << np.uint64(32)) | u[1])
        for c in u[2:]:
            h = _mix(h ^ c)
        return {"n": int(len(h)), "sum_a": int(u[0].sum(dtype=np.uint64)),
                "sum_row": [int(c.sum(dtype=np.uint64)) for c in u[1:]],
                "sum_h": int(h.sum(dtype=np.uint64)), "xor_h": int(np.bitwise_xor.reduce(h)) if len(h) else 0}


def analytic_groups(a, rows_of_group) -> dict:
    """One input tuple {a, G_1 .. G_k} (rows_of_group[i]: the rows of G_{i+1}) without enumerating
    the product, in Python integers mod 2^64: every output carries a, and a row of G_i occurs
    product / |G_i| times."""
    sizes = [len(g) for g in rows_of_group]
    k = len(sizes)
    live = all(s > 0 for s in sizes)
    prod = 1
    for s in sizes:
        prod *= s
    c_unnest, part = [], 1 if live else 0
    for j in range(k):
        part *= sizes[k - 1 - j]
        c_unnest.append(part)
    sums = [((prod // s) * sum(int(v) for v in np.asarray(g).tolist())) & M64 if live else 0
            for s, g in zip(sizes, rows_of_group)]
    return {"n_live": 1 if live else 0, "c_unnest": c_unnest, "c_top": prod if live else 0,
            "sum_a": (int(a) * prod) & M64 if live else 0, "sum_row": sums}


def add_results(*parts) -> dict:
    """Counters and row sums of several inputs together (lists element-wise; sums mod 2^64)."""
    out = {}
    for p in parts:
        for key, v in p.items():
            if isinstance(v, list):
                cur = out.get(key, [0] * len(v))
                out[key] = [(x + y) & M64 for x, y in zip(cur, v)]
            else:
                out[key] = (out.get(key, 0) + v) & M64
    return out


def sort_rows(rows) -> np.ndarray:
    """The rows in lexicographic order (a multiset compares as np.array_equal of two)."""
    r = np.asarray(rows, dtype=np.uint32)
    return r[np.lexsort(r.T[::-1])]


def _records(rows):
    r = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32))
    return r.view([("", np.uint32)] * r.shape[1]).ravel()


def is_sub_multiset(part_rows, full_rows) -> bool:
    """Every row of `part_rows` occurs in `full_rows` at least as often."""
    ku, cu = np.unique(_records(part_rows), return_counts=True)
    if len(ku) == 0:
        return True
    kf, cf = np.unique(_records(full_rows), return_counts=True)
    if len(kf) == 0:
        return False
    pos = np.minimum(np.searchsorted(kf, ku), len(kf) - 1)
    return bool((kf[pos] == ku).all() and (cu <= cf[pos]).all())
