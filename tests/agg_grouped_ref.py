"""What hj3d_agg_grouped must produce, in numpy and Python integers (a helper module for the tests, not a
conftest), written from the operator's contract in include/hj3d.h and not from the kernels.

The per-tuple values are those of agg_nested_ref.agg_nested (COUNT and the specs on a group's column), or, for
a base-word spec, SUM = ext(w) * P mod 2^64 and MIN / MAX = ext(w) with w the word of base row a and P the
tuple's COUNT. A tuple whose a is not a row of base is dead when some spec reads a base word. The values of
the live tuples are then reduced per main ref of the by-table: np.add.at on uint64 (COUNT, SUM), the minimum /
maximum in the spec's order (MIN, MAX), the identities of hj3d_group_agg for a group no live tuple hits.
tests/test_agg_grouped_ref.py pins this module against a brute-force GROUP BY over the unnested rows.

Host only (numpy)."""
import numpy as np

import agg_nested_ref as AN

M64 = AN.M64
NOREF = 0xFFFFFFFF


def is_base(sp) -> bool:
    return len(sp) > 1 and isinstance(sp[1], str)


def signed_of(sp) -> bool:
    return sp[3] if len(sp) > 3 else True


def identity(sp) -> int:
    """The word a group without a live tuple holds for spec sp."""
    if sp[0] in ("count", "sum"):
        return 0
    return AN.identities(signed_of(sp))[0 if sp[0] == "min" else 1]


def extend(w, signed: bool):
    """u32 words sign- or zero-extended, as 64-bit two's complement words (uint64)."""
    w = np.asarray(w, dtype=np.uint32)
    return w.view(np.int32).astype(np.int64).view(np.uint64) if signed else w.astype(np.uint64)


def values(tuples, mains, specs, base=None, row_base=0) -> dict:
    """The per-tuple values: {rows: (n, nspec) uint64, live: (n,) bool, n_in, n_live, c_top, total, unsupported}.
    specs: ("count",) | (op, slot, col[, signed]) | (op, "base", word[, signed]); base: the host copy of the
    base relation ((n_base, words) uint32), needed by the last kind."""
    t = np.array(tuples, dtype=np.uint32, copy=True)
    n, k = t.shape[0], t.shape[1] - 1
    reads_base = any(is_base(sp) for sp in specs)
    arow = t[:, 0].astype(np.int64) - row_base
    if reads_base:
        assert base is not None
        outside = (arow < 0) | (arow >= len(base))
        t[outside, 1] = NOREF  # dead: a is not a row of base
    inner = [("count",) if is_base(sp) else sp for sp in specs]
    r = AN.agg_nested(t, mains, inner)
    live = np.ones(n, dtype=bool)
    for j in range(k):
        live &= t[:, 1 + j].astype(np.int64) < len(np.asarray(mains[j]).reshape(-1, 4))
    rows, total = r["rows"].copy(), list(r["total"])
    for s, sp in enumerate(specs):
        if not is_base(sp):
            continue
        op, word, signed = sp[0], sp[2], signed_of(sp)
        P = r["rows"][:, s]  # the COUNT put in its place
        ext = np.zeros(n, dtype=np.uint64)
        ext[live] = extend(np.asarray(base)[arow[live], word], signed)
        if op == "sum":
            with np.errstate(over="ignore"):
                vals = ext * P  # uint64: mod 2^64
            total[s] = AN._sum64(vals)
        else:
            vals = np.where(live, ext, np.uint64(identity(sp)))
            lv = [AN._ordered(int(v), signed) for v in vals[live]]
            total[s] = ((min(lv) if op == "min" else max(lv)) & M64) if lv else identity(sp)
        rows[:, s] = vals
    return {"rows": rows, "live": live, "n_in": n, "n_live": int(live.sum()), "c_top": r["c_top"], "total": total,
            "unsupported": r["unsupported"]}


def empty_column(n_groups: int, specs) -> np.ndarray:
    col = np.zeros((n_groups, len(specs)), dtype=np.uint64)
    for s, sp in enumerate(specs):
        col[:, s] = identity(sp)
    return col


def fold(col, refs, rows, specs) -> np.ndarray:
    """rows[i] folded into col[refs[i]] (in place; returns col)."""
    refs = np.asarray(refs, dtype=np.int64)
    for s, sp in enumerate(specs):
        v = np.ascontiguousarray(rows[:, s])
        if sp[0] in ("count", "sum"):
            with np.errstate(over="ignore"):
                np.add.at(col[:, s], refs, v)
        else:
            at = np.minimum.at if sp[0] == "min" else np.maximum.at
            c = np.ascontiguousarray(col[:, s])
            if signed_of(sp):
                ci = c.view(np.int64)
                at(ci, refs, v.view(np.int64))
                col[:, s] = ci.view(np.uint64)
            else:
                at(c, refs, v)
                col[:, s] = c
    return col


def agg_grouped(tuples, mains, by, specs, base=None, row_base=0, into=None) -> dict:
    """values() reduced per main ref of mains[by - 1]: {col: (n_mains, nspec) uint64, n_in, n_live, c_top,
    total, unsupported}. into: the column an ACCUMULATE call folds into (not modified)."""
    v = values(tuples, mains, specs, base, row_base)
    m = len(np.asarray(mains[by - 1]).reshape(-1, 4))
    col = empty_column(m, specs) if into is None else np.array(into, dtype=np.uint64, copy=True).reshape(m, len(specs))
    live = v["live"]
    refs = np.asarray(tuples, dtype=np.uint32)[live, by]
    fold(col, refs, v["rows"][live], specs)
    out = {key: v[key] for key in ("n_in", "n_live", "c_top", "total", "unsupported")}
    out["col"] = col
    return out
