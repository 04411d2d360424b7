"""What hj3d_group_agg and hj3d_agg_nested must produce, in numpy and Python integers (a helper module for
the tests, not a conftest), written from the operators' contract in include/hj3d.h and not from the kernels.

The model works on what Table.export() returns, (off, payload, sub): payload[m] = {hash, first_row,
sub_off, sub_len} is main record m, whose group is the rows sub[sub_off : sub_off + sub_len]; and on the
host copy of the build relation ((n, words) uint32). group_agg slices sub per main record, gathers the
word, reduces; agg_nested multiplies the group sizes of every tuple as Python integers and reduces mod 2^64.
tests/test_agg_nested_ref.py pins this module to tests/expand_n_ref.py and the experiment-4 fixtures.

Host only (numpy)."""
import numpy as np

M64 = (1 << 64) - 1
I64_MAX, I64_MIN = (1 << 63) - 1, 1 << 63  # as two's complement words


def identities(signed: bool):
    """(min, max) of a group without folded rows, as 64-bit words."""
    return (I64_MAX, I64_MIN) if signed else (M64, 0)


def group_agg(payload, sub, build, word, signed=True, row_base=0) -> dict:
    """{col: (n_mains, 3) uint64 {sum, min, max} words, n_probe, n_matched, n_out, sum_a}."""
    payload = np.asarray(payload, dtype=np.uint32).reshape(-1, 4)
    m = len(payload)
    col = np.zeros((m, 3), dtype=np.uint64)
    mn_id, mx_id = identities(signed)
    col[:, 1], col[:, 2] = mn_id, mx_id
    if m == 0:
        return {"col": col, "n_probe": 0, "n_matched": 0, "n_out": 0, "sum_a": 0}
    off, ln = payload[:, 2].astype(np.int64), payload[:, 3].astype(np.int64)
    assert (ln > 0).all()
    start = np.cumsum(ln) - ln
    pos = np.repeat(off - start, ln) + np.arange(int(ln.sum()), dtype=np.int64)  # every group's slice of sub, in turn
    idx = np.asarray(sub)[pos].astype(np.int64) - row_base
    ok = (idx >= 0) & (idx < len(build))
    w = np.zeros(len(idx), dtype=np.uint32)
    w[ok] = np.asarray(build)[idx[ok], word]
    v = w.view(np.int32).astype(np.int64) if signed else w.astype(np.int64)  # the extended value
    cnt = np.add.reduceat(ok.astype(np.int64), start)
    with np.errstate(over="ignore"):
        s = np.add.reduceat(np.where(ok, v, 0).astype(np.uint64), start)  # two's complement, exact mod 2^64
    big = np.int64(1) << np.int64(40)
    mn = np.minimum.reduceat(np.where(ok, v, big), start)
    mx = np.maximum.reduceat(np.where(ok, v, -big), start)
    some = cnt > 0
    col[:, 0] = s
    col[some, 1] = mn[some].astype(np.uint64)
    col[some, 2] = mx[some].astype(np.uint64)
    return {"col": col, "n_probe": m, "n_matched": int((cnt == ln).sum()), "n_out": int(cnt.sum()),
            "sum_a": _sum64(s)}


def _sum64(a) -> int:
    with np.errstate(over="ignore"):
        return int(np.asarray(a, dtype=np.uint64).sum(dtype=np.uint64))


def _ordered(word: int, signed: bool) -> int:
    """The value a 64-bit word stands for in the spec's order."""
    return word - (1 << 64) if signed and word >> 63 else word


def agg_nested(tuples, mains, specs) -> dict:
    """tuples: (n, k + 1) uint32 {a, ref_1 .. ref_k}; mains: the k tables' main-record arrays; specs:
    ("count",) or (op, slot, col[, signed]) with col the model's (or the library's) hj3d_gagg column as
    (n_mains, 3) uint64 words. Returns {rows: (n, nspec) uint64, n_in, n_live, c_top (exact), total,
    unsupported}: `unsupported` when a tuple's product or c_top reaches 2^63 (the library then reports
    HJ3D_EUNSUPPORTED and only n_in / n_live)."""
    t = np.asarray(tuples, dtype=np.uint32)
    n, k = t.shape[0], t.shape[1] - 1
    assert k == len(mains) >= 1
    mains = [np.asarray(p, dtype=np.uint32).reshape(-1, 4) for p in mains]
    live = np.ones(n, dtype=bool)
    for j in range(k):
        live &= t[:, 1 + j].astype(np.int64) < len(mains[j])
    ref = [np.where(live, t[:, 1 + j], 0).astype(np.int64) for j in range(k)]
    lens = []
    for j in range(k):
        ln = np.zeros(n, dtype=object)
        if len(mains[j]):
            ln[live] = mains[j][ref[j][live], 3].astype(object)
        lens.append(ln)  # Python integers: no wrap
    alive = live.astype(np.int64).astype(object)
    P = alive.copy()
    for ln in lens:
        P = P * ln
    rows = np.zeros((n, len(specs)), dtype=np.uint64)
    total = []
    for s, sp in enumerate(specs):
        op = sp[0]
        if op == "count":
            vals = P
        else:
            slot, col = sp[1], np.asarray(sp[2], dtype=np.uint64).reshape(-1, 3)
            signed = sp[3] if len(sp) > 3 else True
            g = np.zeros(n, dtype=object)
            field = {"sum": 0, "min": 1, "max": 2}[op]
            if len(col):
                g[live] = col[ref[slot - 1][live], field].astype(object)
            if op == "sum":
                others = alive.copy()
                for j in range(k):
                    if j != slot - 1:
                        others = others * lens[j]
                vals = g * others
            else:
                vals = g
                vals[~live] = identities(signed)[0 if op == "min" else 1]
        vals = (vals & M64).astype(np.uint64) if n else np.zeros(0, np.uint64)
        rows[:, s] = vals
        if op in ("count", "sum"):
            total.append(_sum64(vals))
        else:
            signed = sp[3] if len(sp) > 3 else True
            lv = [_ordered(int(v), signed) for v in vals[live]]
            ident = identities(signed)[0 if op == "min" else 1]
            total.append(((min(lv) if op == "min" else max(lv)) & M64) if lv else ident)
    c_top = int(sum(P.tolist())) if n else 0
    unsupported = c_top >= 1 << 63 or bool((P >= 1 << 63).any())
    return {"rows": rows, "n_in": n, "n_live": int(live.sum()), "c_top": c_top, "total": total, "unsupported": unsupported}


def table_arrays(col):
    """A nested table's (payload, sub, {key: main ref}) for the key column `col` (rows implicit), laid out
    by numpy for the CPU tests: main records in ascending key order, a group's rows ascending, the hash
    word left 0. Any layout with disjoint groups is a valid table to aggregate over."""
    col = np.asarray(col, dtype=np.uint32)
    order = np.argsort(col, kind="stable")
    keys, first, cnt = np.unique(col[order], return_index=True, return_counts=True)
    payload = np.zeros((len(keys), 4), dtype=np.uint32)
    payload[:, 1] = order[first]
    payload[:, 2] = first
    payload[:, 3] = cnt
    return payload, order.astype(np.uint32), {int(k): i for i, k in enumerate(keys)}
