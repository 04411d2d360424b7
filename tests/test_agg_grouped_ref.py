"""tests/agg_grouped_ref.py (the numpy / Python-int model of hj3d_agg_grouped) pinned on the CPU before
tests/test_gpu_agg_grouped.py judges a kernel with it: on tiny tables from agg_nested_ref.table_arrays the
column must equal a brute-force GROUP BY over the rows tests/expand_n_ref.py enumerates: every output row
mapped to the group of its by-row, the gathered words aggregated with plain Python integers."""
import numpy as np
import pytest

import agg_grouped_ref as AG
import agg_nested_ref as AN
import expand_n_ref as XN
import expand_ref as X

EDGE = np.array([0, 1, 5, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
ROW_BASE = 100


def ext(w, signed):
    w = int(w)
    return w - (1 << 32) if signed and w >> 31 else w


@pytest.fixture(scope="module")
def tiny():
    """Two build relations {row id, key, an EDGE word}, their table arrays, tuples over (A, B, A) with distinct
    a = 100 .., dead refs included, and a base relation {an EDGE word, 0} of rows 100 .. 100 + 54: five a lie
    outside it."""
    rng = np.random.default_rng(5)
    cols = [rng.integers(0, 12, 70).astype(np.uint32), rng.integers(0, 9, 40).astype(np.uint32)]
    builds = [np.stack([np.arange(len(c), dtype=np.uint32), c, EDGE[rng.integers(0, len(EDGE), len(c))]], axis=1)
              for c in cols]
    tabs = [AN.table_arrays(c) for c in cols]
    which = (0, 1, 0)
    n = 60
    keys = [[None if v >= 14 else int(v) for v in rng.integers(0, 16, n)] for _ in which]  # 12, 13: no group
    refs = np.empty((n, 4), dtype=np.uint32)
    refs[:, 0] = rng.permutation(n) + ROW_BASE
    for j, b in enumerate(which):
        refmap, m = tabs[b][2], len(tabs[b][0])
        refs[:, 1 + j] = [refmap.get(k, X.NOREF if i % 2 else m + i % 3) if k is not None else X.NOREF
                          for i, k in enumerate(keys[j])]
    base = np.stack([EDGE[rng.integers(0, len(EDGE), n - 5)], np.zeros(n - 5, np.uint32)], axis=1)
    return {"cols": cols, "builds": builds, "tabs": tabs, "which": which, "keys": keys, "tuples": refs, "base": base}


def brute(t, k, by, specs_plain, signed, use_base):
    """The column by plain Python: {group: [values per spec]} over the enumerated rows {a, row_1 .. row_k}.
    specs_plain: ("count",) | (op, slot) | (op, "base")."""
    which = t["which"][:k]
    a = t["tuples"][:, 0]
    keys = [list(kk) for kk in t["keys"][:k]]
    if use_base:  # a tuple whose a is not a row of base is dead: no key
        for i, ai in enumerate(a):
            if not 0 <= int(ai) - ROW_BASE < len(t["base"]):
                keys[0][i] = None
    rows = XN.expand_rows(a, keys, [t["cols"][b] for b in which])
    refmap, byrel = t["tabs"][which[by - 1]][2], t["cols"][which[by - 1]]
    groups = {}
    for row in rows:
        m = refmap[int(byrel[row[by]])]  # the group of the row's by-row
        groups.setdefault(m, []).append(row)
    out = {}
    for m, rs in groups.items():
        vals = []
        for sp in specs_plain:
            if sp[0] == "count":
                vals.append(len(rs))
                continue
            if sp[1] == "base":
                ws = [ext(t["base"][int(r[0]) - ROW_BASE, 0], signed) for r in rs]
            else:
                ws = [ext(t["builds"][which[sp[1] - 1]][r[sp[1]], 2], signed) for r in rs]
            vals.append({"sum": sum, "min": min, "max": max}[sp[0]](ws) & AG.M64)
        out[m] = vals
    return out, len(rows)


@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_column_equals_a_brute_force_group_by(tiny, k, signed):
    t = tiny
    which = t["which"][:k]
    mains = [t["tabs"][b][0] for b in which]
    gcol = [AN.group_agg(t["tabs"][b][0], t["tabs"][b][1], t["builds"][b], 2, signed)["col"] for b in range(2)]
    tuples = t["tuples"][:, :k + 1]
    for use_base in (False, True):
        plain = [("count",)] + [(op, slot) for slot in range(1, k + 1) for op in ("sum", "min", "max")][:6]
        if use_base:
            plain = plain[:4] + [("sum", "base"), ("min", "base"), ("max", "base")]
        specs = [sp if sp[0] == "count" else
                 ((sp[0], "base", 0, signed) if sp[1] == "base" else (sp[0], sp[1], gcol[which[sp[1] - 1]], signed))
                 for sp in plain]
        for by in range(1, k + 1):
            got = AG.agg_grouped(tuples, mains, by, specs, base=t["base"] if use_base else None, row_base=ROW_BASE)
            want, n_rows = brute(t, k, by, plain, signed, use_base)
            assert not got["unsupported"] and got["c_top"] == n_rows > 0
            m_by = len(mains[by - 1])
            assert got["col"].shape == (m_by, len(specs))
            assert 0 < len(want) <= m_by and (by != 1 or len(want) < m_by)  # by table A: a group no tuple hits
            for m in range(m_by):
                ident = [AG.identity(sp) for sp in specs]
                assert [int(x) for x in got["col"][m]] == want.get(m, ident), (by, m)
            # the totals are the reduce of the column over all groups
            for s, sp in enumerate(specs):
                hit = [int(got["col"][m, s]) for m in want]
                if sp[0] in ("count", "sum"):
                    assert got["total"][s] == sum(hit) & AG.M64
                else:
                    sg = AG.signed_of(sp)
                    red = (min if sp[0] == "min" else max)(AN._ordered(v, sg) for v in hit)
                    assert got["total"][s] == red & AG.M64
            assert got["total"][0] == got["c_top"]
    # five a lie outside base: with a base-word spec those tuples are dead, without one a is opaque
    opaque = AG.agg_grouped(tuples, mains, 1, [("count",)])
    based = AG.agg_grouped(tuples, mains, 1, [("count",), ("max", "base", 0)], base=t["base"], row_base=ROW_BASE)
    outside = np.array([not 0 <= int(ai) - ROW_BASE < len(t["base"]) for ai in tuples[:, 0]])
    assert outside.sum() == 5
    assert based["n_live"] == opaque["n_live"] - int((outside & AG.values(tuples, mains, [("count",)])["live"]).sum())


def test_dead_and_empty_inputs(tiny):
    t = tiny
    mains = [t["tabs"][0][0]]
    m = len(mains[0])
    gcol = AN.group_agg(t["tabs"][0][0], t["tabs"][0][1], t["builds"][0], 2, True)["col"]
    specs = [("count",), ("sum", 1, gcol), ("min", 1, gcol), ("max", 1, gcol, True), ("min", "base", 0, False),
             ("max", "base", 0, False)]
    ident = [0, 0, AN.I64_MAX, AN.I64_MIN, AN.M64, 0]
    dead = np.array([[ROW_BASE + 1, X.NOREF], [ROW_BASE + 2, m], [ROW_BASE - 1, 0], [ROW_BASE + 55, 1]], dtype=np.uint32)
    got = AG.agg_grouped(dead, mains, 1, specs, base=t["base"], row_base=ROW_BASE)
    assert (got["n_in"], got["n_live"], got["c_top"], got["total"]) == (4, 0, 0, ident)
    assert got["col"].tolist() == [ident] * m
    none = AG.agg_grouped(np.zeros((0, 2), np.uint32), mains, 1, specs, base=t["base"], row_base=ROW_BASE)
    assert (none["n_in"], none["total"]) == (0, ident) and none["col"].tolist() == [ident] * m
    # without a base-word spec a is opaque: the last two tuples are live
    got = AG.agg_grouped(dead, mains, 1, specs[:4])
    assert got["n_live"] == 2 and int(got["col"][0, 0]) == int(mains[0][0, 3]) and int(got["col"][1, 0]) == int(mains[0][1, 3])


def test_accumulate_folds_into_the_given_column(tiny):
    t = tiny
    mains = [t["tabs"][b][0] for b in t["which"][:2]]
    gcol = AN.group_agg(t["tabs"][1][0], t["tabs"][1][1], t["builds"][1], 2, True)["col"]
    specs = [("count",), ("min", 2, gcol), ("max", "base", 0), ("sum", "base", 0, False)]
    tuples = t["tuples"][:, :3]
    kw = {"base": t["base"], "row_base": ROW_BASE}
    whole = AG.agg_grouped(tuples, mains, 1, specs, **kw)
    first = AG.agg_grouped(tuples[:30], mains, 1, specs, **kw)
    both = AG.agg_grouped(tuples[30:], mains, 1, specs, into=first["col"], **kw)
    assert np.array_equal(both["col"], whole["col"]) and not np.array_equal(first["col"], whole["col"])
    assert both["n_in"] == 30 and both["c_top"] + first["c_top"] == whole["c_top"]
