"""tests/select_nested_ref.py (the numpy model of hj3d_select_nested) pinned against a plain Python
loop on a tiny case: every op, signed against unsigned at 0x7FFFFFFF / 0x80000000, `range` with an empty
and a full interval, every way a tuple is dead, the checksums (CPU suite)."""
import numpy as np
import pytest

import select_nested_ref as SN

NOREF = SN.NOREF
M64 = SN.M64
EDGE = [0, 1, 5, 6, 7, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF]


def mix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def one(w, op, lo, hi, signed):
    v = w - (1 << 32) if signed and w >= (1 << 31) else w
    return {"<": v < lo, "<=": v <= lo, ">": v > lo, ">=": v >= lo, "==": v == lo, "!=": v != lo,
            "range": lo <= v < hi}[op]


def loop_model(tuples, preds, base, base_row_base, mains, builds, build_row_base):
    """The contract of include/hj3d.h, tuple by tuple."""
    live, mask = [], []
    for t in tuples.tolist():
        a, refs = t[0], t[1:]
        ok = True
        if base is not None and not 0 <= a - base_row_base < len(base):
            ok = False
        for j, r in enumerate(refs):
            if r == NOREF or (mains[j] is not None and r >= len(mains[j])):
                ok = False
        words = []
        if ok:
            for pr in preds:
                kind, slot, word, op, lo, hi, signed = SN.parse_pred(pr)
                if kind == "first":
                    fr = int(mains[slot - 1][refs[slot - 1]][1]) - build_row_base[slot - 1]
                    if not 0 <= fr < len(builds[slot - 1]):
                        ok = False
        if ok:
            for pr in preds:
                kind, slot, word, op, lo, hi, signed = SN.parse_pred(pr)
                if kind == "base":
                    w = int(base[a - base_row_base][word])
                elif kind == "count":
                    w = int(mains[slot - 1][refs[slot - 1]][3])
                else:
                    w = int(builds[slot - 1][int(mains[slot - 1][refs[slot - 1]][1]) - build_row_base[slot - 1]][word])
                words.append(one(w, op, lo, hi, signed))
        live.append(ok)
        mask.append(ok and all(words))
    rows = [t for t, m in zip(tuples.tolist(), mask) if m]
    sum_h = xor_h = 0
    for t in rows:
        h = mix64(t[0]) if len(t) == 1 else mix64((t[0] << 32) | t[1])
        for r in t[2:]:
            h = mix64(h ^ r)
        sum_h = (sum_h + h) & M64
        xor_h ^= h
    return {"live": live, "mask": mask, "rows": rows, "n_probe": len(tuples), "n_matched": sum(live), "n_out": len(rows),
            "n_cmps": 0, "sum_a": sum(t[0] for t in rows) & M64, "sum_b": 0, "sum_c": 0, "sum_h": sum_h, "xor_h": xor_h}


def agree(tuples, preds, base=None, base_row_base=0, mains=None, builds=None, build_row_base=None):
    k = tuples.shape[1] - 1
    mains = [None] * k if mains is None else mains
    builds = [None] * k if builds is None else builds
    rb = [0] * k if build_row_base is None else build_row_base
    got = SN.select_nested(tuples, preds, base, base_row_base, mains, builds, rb)
    want = loop_model(tuples, preds, base, base_row_base, mains, builds, rb)
    assert got["live"].tolist() == want["live"] and got["mask"].tolist() == want["mask"]
    assert got["rows"].tolist() == want["rows"]
    assert SN.counters(got) == SN.counters(want)
    return got


@pytest.fixture(scope="module")
def tiny():
    """base: one row per EDGE value in word 1 (rows 100 ..); two tables whose groups have 1..3 and 1..5
    rows; builds whose word 1 repeats EDGE."""
    base = np.stack([np.arange(len(EDGE)), EDGE, np.arange(len(EDGE)) * 3], axis=1).astype(np.uint32)
    m1 = np.array([[0, 4, 0, 1], [0, 0, 1, 2], [0, 9, 3, 3], [0, 40, 6, 1]], dtype=np.uint32)  # first_row 40: outside
    m2 = np.array([[0, 10 + i, 2 * i, 1 + i] for i in range(5)], dtype=np.uint32)
    b1 = np.stack([np.arange(12), np.resize(EDGE, 12)], axis=1).astype(np.uint32)
    b2 = np.stack([np.arange(10), np.resize(EDGE[::-1], 10)], axis=1).astype(np.uint32)  # rows 10 .. 19
    rng = np.random.default_rng(5)
    n = 300
    t = np.stack([rng.integers(98, 100 + len(EDGE) + 2, n), rng.integers(0, 6, n), rng.integers(0, 7, n)], axis=1)
    t = t.astype(np.uint32)
    t[::11, 1] = NOREF
    t[5::13, 2] = NOREF
    return {"base": base, "mains": [m1, m2], "builds": [b1, b2], "rb": [0, 10], "t": t}


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("op", SN.OPS)
def test_every_op_at_the_sign_boundary(tiny, op, signed):
    t = tiny["t"]
    for lo in (0x7FFFFFFF, 0x80000000, -0x80000000, -1, 0, 6):
        got = agree(t, [("base", 1, op, lo, lo + 2, signed)], tiny["base"], 100, tiny["mains"], tiny["builds"], tiny["rb"])
        assert 0 < got["n_matched"] < len(t)
    # a word of 0x80000000 is below 0 signed and above 0x7FFFFFFF unsigned
    w = np.array([[0], [1]], dtype=np.uint32)
    b = np.array([[0x7FFFFFFF], [0x80000000]], dtype=np.uint32)
    assert SN.select_nested(w, [("base", 0, "<", 0, None, True)], b)["mask"].tolist() == [False, True]
    assert SN.select_nested(w, [("base", 0, "<", 0, None, False)], b)["mask"].tolist() == [False, False]
    assert SN.select_nested(w, [("base", 0, ">", 0x7FFFFFFF, None, False)], b)["mask"].tolist() == [False, True]
    assert SN.select_nested(w, [("base", 0, ">", 0x7FFFFFFF, None, True)], b)["mask"].tolist() == [False, False]


def test_range_empty_and_full(tiny):
    t, kw = tiny["t"], dict(base=tiny["base"], base_row_base=100, mains=tiny["mains"], builds=tiny["builds"],
                            build_row_base=tiny["rb"])
    empty = agree(t, [("base", 1, "range", 7, 7)], **kw)
    assert empty["n_out"] == 0 and empty["n_matched"] > 0 and (empty["sum_a"], empty["sum_h"], empty["xor_h"]) == (0, 0, 0)
    full_s = agree(t, [("base", 1, "range", -(1 << 31), 1 << 31, True)], **kw)
    full_u = agree(t, [("base", 1, "range", 0, 1 << 32, False)], **kw)
    none = agree(t, [], **kw)
    assert full_s["n_out"] == full_u["n_out"] == none["n_out"] == none["n_matched"] > 0
    assert full_s["rows"].tolist() == none["rows"].tolist()


def test_group_predicates_and_dead_tuples(tiny):
    t, kw = tiny["t"], dict(base=tiny["base"], base_row_base=100, mains=tiny["mains"], builds=tiny["builds"],
                            build_row_base=tiny["rb"])
    for preds in ([("count", 1, ">=", 2)], [("count", 2, "range", 2, 4)], [("count", 1, "!=", 3), ("count", 2, "<", 5)],
                  [("first", 2, 1, "<", 0)], [("first", 2, 1, ">", 0x7FFFFFFF, None, False)], [("first", 1, 1, ">=", 6)],
                  [("base", 2, ">", 9), ("count", 2, ">=", 2), ("first", 1, 0, "!=", 4), ("first", 2, 1, ">", 5)]):
        got = agree(t, preds, **kw)
        assert 0 < got["n_out"] < got["n_matched"] < len(t), preds
    # main record 3 of table 1 has its first row outside the build relation: dead under a FIRST
    # predicate on slot 1 only
    with_first = agree(t, [("first", 1, 1, ">=", 0, None, False)], **kw)
    without = agree(t, [("count", 1, ">=", 0)], **kw)
    assert with_first["n_matched"] == without["n_matched"] - int(((t[:, 1] == 3) & without["live"]).sum()) < without["n_matched"]
    # refs without their table are opaque: only NOREF kills
    opaque = agree(t, [], base=None)
    assert opaque["n_matched"] == int(((t[:, 1] != NOREF) & (t[:, 2] != NOREF)).sum())
    given = agree(t, [], base=None, mains=tiny["mains"])
    assert given["n_matched"] < opaque["n_matched"]


@pytest.mark.parametrize("k", range(7))
def test_every_width_checksum(k):
    rng = np.random.default_rng(k)
    t = rng.integers(0, 1 << 32, (40, k + 1), dtype=np.uint64).astype(np.uint32)
    for j in range(1, k + 1):
        t[j::9, j] = NOREF
    got = agree(t, [])
    assert got["n_out"] == got["n_matched"] == int((t[:, 1:] != NOREF).all(axis=1).sum()) > 0
    nock = SN.select_nested(t, [], checksum=False)
    assert (nock["sum_h"], nock["xor_h"], nock["sum_a"]) == (0, 0, got["sum_a"])
