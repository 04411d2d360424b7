"""What hj3d_select_nested must produce, in plain numpy (a helper module for the tests, not a conftest).

The operator forwards, in input order, the stored nested tuples {a, ref_1 .. ref_k} that are live and
pass a conjunction of predicates. Inputs of the model: the tuples, the base relation's words, each
table's exported main records {hash, first_row, sub_off, sub_len} (Table.export()'s payload) and the
build relations' words. A predicate is one of
    ("base", word, op, lo[, hi][, signed])          word of base row a
    ("count", slot, op, lo[, hi])                   sub_len of main record ref_slot (u32 compare)
    ("first", slot, word, op, lo[, hi][, signed])   word of the build tuple whose row is first_row
with op in OPS, compared as int32 unless signed is False (sel_one of hj3d_internal.hpp).

A tuple is dead when base is given and a is not one of its rows, when any ref is 0xFFFFFFFF, when a ref
whose table is given is not below that table's main-record count, or when a "first" predicate's first
row lies outside its build relation. tests/test_select_nested_ref.py pins this module against a plain
Python loop.

Host only (numpy)."""
import numpy as np

M64 = (1 << 64) - 1
NOREF = 0xFFFFFFFF
OPS = ("<", "<=", ">", ">=", "==", "!=", "range")


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def parse_pred(pr):
    """(source, slot, word, op, lo, hi, signed) of a predicate tuple."""
    kind = pr[0]
    if kind == "base":
        slot, rest = 0, pr[1:]
    elif kind == "count":
        slot, rest = pr[1], (0, pr[2], pr[3], pr[4] if len(pr) > 4 else None, False)
    elif kind == "first":
        slot, rest = pr[1], pr[2:]
    else:
        raise ValueError(kind)
    word, op, lo = rest[0], rest[1], rest[2]
    hi = rest[3] if len(rest) > 3 and rest[3] is not None else 0
    signed = rest[4] if len(rest) > 4 else True
    assert op in OPS
    return kind, int(slot), int(word), op, int(lo), int(hi), bool(signed)


def compare(words, op, lo, hi, signed) -> np.ndarray:
    """sel_one over an array of u32 words."""
    w = np.asarray(words, dtype=np.uint32)
    v = w.view(np.int32).astype(np.int64) if signed else w.astype(np.int64)
    if op == "<":
        return v < lo
    if op == "<=":
        return v <= lo
    if op == ">":
        return v > lo
    if op == ">=":
        return v >= lo
    if op == "==":
        return v == lo
    if op == "!=":
        return v != lo
    return (v >= lo) & (v < hi)


def row_hashes(rows) -> np.ndarray:
    """h = mix64(a) for k = 0; else pair(a, ref_1), then mix64(h ^ ref_i) for i = 2..k."""
    u = [rows[:, j].astype(np.uint64) for j in range(rows.shape[1])]
    with np.errstate(over="ignore"):
        if len(u) == 1:
            return _mix(u[0])
        h = _mix((u[0] << np.uint64(32)) | u[1])
        for c in u[2:]:
            h = _mix(h ^ c)
        return h


def select_nested(tuples, preds, base=None, base_row_base=0, mains=None, builds=None, build_row_base=None,
                  checksum=True) -> dict:
    """tuples: (n, k + 1) u32; base: (rows, words) u32 or None; mains / builds: lists of k entries, each
    None or the table's (m, 4) main records / the build relation's (rows, words) u32 array;
    build_row_base: list of k row bases (None: all 0). Returns {live, mask (bool arrays), rows (the
    passing tuples in order), n_probe, n_matched, n_out, n_cmps, sum_a, sum_b, sum_c, sum_h, xor_h}."""
    t = np.ascontiguousarray(np.asarray(tuples, dtype=np.uint32))
    assert t.ndim == 2 and 1 <= t.shape[1] <= 7
    n, k = len(t), t.shape[1] - 1
    mains = [None] * k if mains is None else list(mains)
    builds = [None] * k if builds is None else list(builds)
    rb = [0] * k if build_row_base is None else list(build_row_base)
    assert len(mains) == k and len(builds) == k and len(preds) <= 4
    a = t[:, 0].astype(np.int64)
    live = np.ones(n, dtype=bool)
    arow = a - int(base_row_base)
    if base is not None:
        base = np.asarray(base, dtype=np.uint32)
        live &= (arow >= 0) & (arow < len(base))
    for j in range(k):
        ref = t[:, 1 + j].astype(np.int64)
        live &= ref != NOREF
        if mains[j] is not None:
            live &= ref < len(mains[j])
    parsed = [parse_pred(p) for p in preds]
    # "first" rows outside their build relation kill the tuple before any predicate is evaluated
    frow = {}
    for i, (kind, slot, _w, _op, _lo, _hi, _s) in enumerate(parsed):
        if kind != "first":
            continue
        assert 1 <= slot <= k and mains[slot - 1] is not None and builds[slot - 1] is not None
        m = np.asarray(mains[slot - 1], dtype=np.uint32).reshape(-1, 4)
        ref = np.where(live, t[:, slot], 0).astype(np.int64)
        fr = (m[ref, 1].astype(np.int64) if len(m) else np.zeros(n, np.int64)) - int(rb[slot - 1])
        live &= (fr >= 0) & (fr < len(builds[slot - 1]))
        frow[i] = fr
    mask = live.copy()
    for i, (kind, slot, word, op, lo, hi, signed) in enumerate(parsed):
        if kind == "base":
            assert base is not None and slot == 0
            w = base[np.where(live, arow, 0), word] if len(base) else np.zeros(n, np.uint32)
        elif kind == "count":
            assert 1 <= slot <= k and mains[slot - 1] is not None
            m = np.asarray(mains[slot - 1], dtype=np.uint32).reshape(-1, 4)
            w = m[np.where(live, t[:, slot], 0).astype(np.int64), 3] if len(m) else np.zeros(n, np.uint32)
        else:
            b = np.asarray(builds[slot - 1], dtype=np.uint32)
            w = b[np.where(live, frow[i], 0), word] if len(b) else np.zeros(n, np.uint32)
        mask &= compare(w, op, lo, hi, signed)
    rows = t[mask]
    h = row_hashes(rows) if checksum and len(rows) else np.zeros(0, np.uint64)
    return {"live": live, "mask": mask, "rows": rows, "n_probe": n, "n_matched": int(live.sum()),
            "n_out": int(mask.sum()), "n_cmps": 0, "sum_a": int(rows[:, 0].sum(dtype=np.uint64)), "sum_b": 0,
            "sum_c": 0, "sum_h": int(h.sum(dtype=np.uint64)), "xor_h": int(np.bitwise_xor.reduce(h)) if len(h) else 0}


COUNTERS = ("n_probe", "n_matched", "n_out", "n_cmps", "sum_a", "sum_b", "sum_c", "sum_h", "xor_h")


def counters(model: dict) -> tuple:
    return tuple(model[f] for f in COUNTERS)
