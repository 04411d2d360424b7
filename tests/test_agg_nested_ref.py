"""tests/agg_nested_ref.py (the numpy / Python-int model of hj3d_group_agg and hj3d_agg_nested) pinned on
the CPU before tests/test_gpu_group_agg.py and tests/test_gpu_agg_nested.py judge a kernel with it: on
tiny inputs its per-tuple values must equal a brute-force reduction over the rows tests/expand_n_ref.py
enumerates, its c_top expand_n_ref's, and on the experiment-4 fixtures c_top and (S.k and T.k being
iota) the SUM(k) totals the reference binary's counters and row sums."""
import json
import os

import numpy as np
import pytest

import agg_nested_ref as AN
import expand_n_ref as XN
import expand_ref as X
from conftest import GOLDEN

EDGE = np.array([0, 1, 5, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)


def ext(w, signed):
    """A u32 word extended to a Python integer."""
    w = int(w)
    return w - (1 << 32) if signed and w >> 31 else w


@pytest.fixture(scope="module")
def tiny():
    """Two build relations {row id, key, an EDGE word}, their table arrays, and tuples over (A, B, A) with
    distinct a, dead refs included."""
    rng = np.random.default_rng(5)
    cols = [rng.integers(0, 12, 70).astype(np.uint32), rng.integers(0, 9, 40).astype(np.uint32)]
    builds = [np.stack([np.arange(len(c), dtype=np.uint32), c, EDGE[rng.integers(0, len(EDGE), len(c))]], axis=1)
              for c in cols]
    tabs = [AN.table_arrays(c) for c in cols]
    which = (0, 1, 0)
    n = 60
    keys = [[None if v >= 14 else int(v) for v in rng.integers(0, 16, n)] for _ in which]  # 12, 13: no group
    refs = np.empty((n, 4), dtype=np.uint32)
    refs[:, 0] = rng.permutation(n) + 100
    for j, b in enumerate(which):
        refmap, m = tabs[b][2], len(tabs[b][0])
        refs[:, 1 + j] = [refmap.get(k, X.NOREF if i % 2 else m + i % 3) if k is not None else X.NOREF
                          for i, k in enumerate(keys[j])]
    return {"cols": cols, "builds": builds, "tabs": tabs, "which": which, "keys": keys, "tuples": refs}


@pytest.mark.parametrize("signed", [True, False])
def test_group_agg_by_hand(tiny, signed):
    for b in range(2):
        payload, sub, refmap = tiny["tabs"][b]
        build, col = tiny["builds"][b], tiny["cols"][b]
        got = AN.group_agg(payload, sub, build, 2, signed)
        for key, m in refmap.items():
            vals = [ext(build[r, 2], signed) for r in np.nonzero(col == key)[0]]
            assert [int(x) for x in got["col"][m]] == [sum(vals) & AN.M64, min(vals) & AN.M64, max(vals) & AN.M64]
        assert (got["n_probe"], got["n_matched"], got["n_out"]) == (len(refmap), len(refmap), len(col))
        assert got["sum_a"] == sum(ext(w, signed) for w in build[:, 2]) & AN.M64
        # a shorter relation: its missing rows are skipped, a group without folded row keeps the identities
        half = AN.group_agg(payload, sub, build[:len(build) // 2], 2, signed)
        for key, m in refmap.items():
            vals = [ext(build[r, 2], signed) for r in np.nonzero(col == key)[0] if r < len(build) // 2]
            want = [sum(vals) & AN.M64, min(vals) & AN.M64, max(vals) & AN.M64] if vals else [0, *AN.identities(signed)]
            assert [int(x) for x in half["col"][m]] == want
        whole = sum(1 for key in refmap if np.nonzero(col == key)[0].max() < len(build) // 2)
        assert half["n_out"] == len(build) // 2 and half["n_matched"] == whole < half["n_probe"]


@pytest.mark.parametrize("signed", [True, False])
def test_per_tuple_values_equal_a_reduction_over_the_enumerated_rows(tiny, signed):
    t = tiny
    which = t["which"]
    mains = [t["tabs"][b][0] for b in which]
    gcol = [AN.group_agg(t["tabs"][b][0], t["tabs"][b][1], t["builds"][b], 2, signed)["col"] for b in range(2)]
    specs = [("count",)] + [(op, slot, gcol[which[slot - 1]], signed) for slot in (1, 2, 3) for op in ("sum", "min", "max")]
    got = AN.agg_nested(t["tuples"], mains, specs)
    # the rows hj3d_unnestn would emit, from the keys alone
    a = t["tuples"][:, 0]
    rows = XN.expand_rows(a, t["keys"], [t["cols"][b] for b in which])
    c = XN.counters(t["keys"], [t["cols"][b] for b in which])
    assert (got["n_in"], got["n_live"], got["c_top"]) == (c["n_in"], c["n_live"], c["c_top"]) and not got["unsupported"]
    assert 0 < c["n_live"] < len(a) and c["c_top"] == len(rows) > len(a)
    mn_id, mx_id = AN.identities(signed)
    totals = [0] * len(specs)
    seen_min, seen_max = {}, {}
    for i, ai in enumerate(a):
        mine = rows[rows[:, 0] == ai]
        want = [len(mine)]
        for slot in (1, 2, 3):
            vals = [ext(t["builds"][which[slot - 1]][r, 2], signed) for r in mine[:, slot]]
            want += [sum(vals) & AN.M64, (min(vals) & AN.M64) if vals else mn_id, (max(vals) & AN.M64) if vals else mx_id]
            if vals:
                seen_min[slot] = min(seen_min.get(slot, min(vals)), min(vals))
                seen_max[slot] = max(seen_max.get(slot, max(vals)), max(vals))
        assert [int(x) for x in got["rows"][i]] == want, i
        totals = [(x + y) & AN.M64 for x, y in zip(totals, want)]
    for s, sp in enumerate(specs):
        if sp[0] in ("count", "sum"):
            assert got["total"][s] == totals[s]
        else:
            assert got["total"][s] == (seen_min if sp[0] == "min" else seen_max)[sp[1]] & AN.M64
    assert got["total"][0] == c["c_top"]


def test_dead_and_empty_inputs(tiny):
    t = tiny
    mains = [t["tabs"][0][0]]
    gcol = AN.group_agg(t["tabs"][0][0], t["tabs"][0][1], t["builds"][0], 2, True)["col"]
    specs = [("count",), ("sum", 1, gcol), ("min", 1, gcol), ("max", 1, gcol, True)]
    dead = np.array([[1, X.NOREF], [2, len(mains[0])]], dtype=np.uint32)
    got = AN.agg_nested(dead, mains, specs)
    assert (got["n_live"], got["c_top"], got["total"]) == (0, 0, [0, 0, AN.I64_MAX, AN.I64_MIN])
    assert got["rows"].tolist() == [[0, 0, AN.I64_MAX, AN.I64_MIN]] * 2
    none = AN.agg_nested(np.zeros((0, 2), np.uint32), mains, specs)
    assert (none["n_in"], none["total"]) == (0, [0, 0, AN.I64_MAX, AN.I64_MIN])
    assert AN.agg_nested(dead, mains, [("min", 1, gcol, False), ("max", 1, gcol, False)])["total"] == [AN.M64, 0]


def test_wrap_and_magnitude():
    # one group of 2^16 rows four times: P = 2^64; three times: 2^48, SUM wraps 2^64
    payload = np.array([[0, 0, 0, 1 << 16]], dtype=np.uint32)
    col = np.array([[0xFFFFFFFF << 16, 0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint64)
    t3 = np.array([[7, 0, 0, 0]], dtype=np.uint32)
    got = AN.agg_nested(t3, [payload] * 3, [("count",), ("sum", 2, col, False)])
    assert got["total"] == [1 << 48, ((0xFFFFFFFF << 16) << 32) & AN.M64] and not got["unsupported"]
    t4 = np.array([[7, 0, 0, 0, 0]], dtype=np.uint32)
    assert AN.agg_nested(t4, [payload] * 4, [("count",)])["unsupported"]
    half = np.array([[0, 0, 0, 1 << 21]], dtype=np.uint32)
    t63 = np.array([[7, 0, 0, 0]], dtype=np.uint32)
    assert AN.agg_nested(t63, [half] * 3, [("count",)])["c_top"] == 1 << 63
    assert AN.agg_nested(t63, [half] * 3, [("count",)])["unsupported"]


@pytest.mark.parametrize("name", ["exp4_R10_a3_A2_b2_B3", "exp4_R16_a3_A4_b2_B2"])
def test_exp4_fixture_c_top_and_row_sums(name):
    import hj3d
    with open(os.path.join(GOLDEN, name + ".json")) as fh:
        g = json.load(fh)
    ref = g["plans"]["Ndu"]
    Sa, Ta = hj3d.gen_exp4_ref(*g["generator_args"][1:6])
    tabs = [AN.table_arrays(Sa), AN.table_arrays(Ta)]
    builds = [np.stack([np.arange(len(c), dtype=np.uint32), c], axis=1) for c in (Sa, Ta)]  # S.k, T.k = iota
    Rk = np.arange(g["cardR"], dtype=np.uint32)
    tuples = np.stack([Rk] + [np.array([tab[2].get(int(k), X.NOREF) for k in Rk], dtype=np.uint32) for tab in tabs], axis=1)
    gcol = [AN.group_agg(tab[0], tab[1], b, 0, False)["col"] for tab, b in zip(tabs, builds)]
    got = AN.agg_nested(tuples, [tabs[0][0], tabs[1][0]], [("count",), ("sum", 1, gcol[0], False), ("sum", 2, gcol[1], False)])
    assert got["c_top"] == ref["c_top"] == got["total"][0] and got["n_live"] == ref["c_probe_RT"]
    assert got["total"][1:] == [ref["out"]["sum_b"], ref["out"]["sum_c"]]
