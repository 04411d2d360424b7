"""tests/expand_n_ref.py (the numpy reference of hj3d_unnestn) pinned on the CPU before
tests/test_gpu_unnestn.py judges a kernel with it: for k = 1 and k = 2 it must be tests/expand_ref.py
(itself pinned by tests/test_expand_ref.py), for k = 2 also the reference binary's experiment-4
counters on the bit-exact generator's inputs, and for k = 3 a hand-enumerated example."""
import json
import os

import numpy as np
import pytest

import expand_n_ref as XN
import expand_ref as X
from conftest import GOLDEN


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(17)
    Sa = np.minimum(rng.zipf(1.4, 3000) - 1, 199).astype(np.uint32)
    Ta = rng.integers(0, 180, 2500).astype(np.uint32)
    n = 900
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ks = rng.integers(-3, 230, n)  # negative: dead; >= 200: no S row
    kt = rng.integers(-3, 200, n)
    return Sa, Ta, a, ks, kt


def test_k1_equals_expand_pairs(data):
    Sa, _, a, ks, _ = data
    rows = XN.expand_rows(a, [ks], [Sa])
    pairs = X.expand_pairs(a, ks, Sa)
    assert np.array_equal(rows, pairs) and len(rows) > len(a)
    pc, rc = X.pair_checksums(pairs), XN.row_checksums(rows)
    assert (rc["n"], rc["sum_a"], rc["sum_row"], rc["sum_h"], rc["xor_h"]) == \
        (pc["n"], pc["sum_a"], [pc["sum_b"]], pc["sum_h"], pc["xor_h"])
    c, want = XN.counters([ks], [Sa]), X.pair_counters(a, ks, Sa)
    assert (c["n_in"], c["n_live"], c["c_unnest"], c["c_top"]) == \
        (want["n_probe"], want["n_matched"], [want["n_out"]], want["n_out"])


def test_k2_equals_expand_triples(data):
    Sa, Ta, a, ks, kt = data
    rows = XN.expand_rows(a, [ks, kt], [Sa, Ta])
    trip = X.expand_triples(a, ks, kt, Sa, Ta)
    assert np.array_equal(rows, trip) and len(rows) > len(a)
    tc, rc = X.triple_checksums(trip), XN.row_checksums(rows)
    assert (rc["n"], rc["sum_a"], rc["sum_row"], rc["sum_h"], rc["xor_h"]) == \
        (tc["n"], tc["sum_a"], [tc["sum_b"], tc["sum_c"]], tc["sum_h"], tc["xor_h"])
    c, want = XN.counters([ks, kt], [Sa, Ta]), X.triple_counters(ks, kt, Sa, Ta)
    assert c["c_unnest"] == [want["c_unnest_1"], want["c_unnest_2"]] and c["c_top"] == want["c_top"]
    cs, ct = X.triple_counts(ks, kt, Sa, Ta)
    assert c["n_live"] == int(((cs > 0) & (ct > 0)).sum()) and c["n_in"] == len(a)


@pytest.mark.parametrize("name", ["exp4_R10_a3_A2_b2_B3", "exp4_R16_a3_A4_b2_B2"])
def test_k2_reproduces_exp4_fixture(name):
    import hj3d
    with open(os.path.join(GOLDEN, name + ".json")) as fh:
        g = json.load(fh)
    ref = g["plans"]["Ndu"]
    Sa, Ta = hj3d.gen_exp4_ref(*g["generator_args"][1:6])
    Rk = np.arange(g["cardR"], dtype=np.uint32)
    c = XN.counters([Rk, Rk], [Sa, Ta])
    assert c["c_unnest"] == [ref["c_unnest_1"], ref["c_unnest_2"]] and c["c_top"] == ref["c_top"]
    assert c["n_live"] == ref["c_probe_RT"]  # the second probe's survivors are the tuples with both groups
    rc = XN.row_checksums(XN.expand_rows(Rk, [Rk, Rk], [Sa, Ta]))
    out = ref["out"]
    assert (rc["n"], rc["sum_a"], rc["sum_row"], rc["sum_h"], rc["xor_h"]) == \
        (out["n"], out["sum_a"], [out["sum_b"], out["sum_c"]], out["sum_h"], out["xor_h"])


def test_k3_by_hand():
    import hj3d
    A = np.array([5, 6, 5, 8], dtype=np.uint32)     # 5: rows {0, 2}, 6: {1}, 8: {3}
    B = np.array([6, 5, 5, 5], dtype=np.uint32)     # 5: rows {1, 2, 3}, 6: {0}
    a = [10, 11, 12]
    keys = [[5, 6, 8], [5, None, 6], [6, 5, 5]]     # tables A, B, A again (a self join)
    rows = XN.expand_rows(a, keys, [A, B, A])
    # tuple 10: {0, 2} x {1, 2, 3} x {1}, group 1 fastest; tuple 11: dead; tuple 12: {3} x {0} x {0, 2}
    assert rows.tolist() == [[10, 0, 1, 1], [10, 2, 1, 1], [10, 0, 2, 1], [10, 2, 2, 1], [10, 0, 3, 1], [10, 2, 3, 1],
                             [12, 3, 0, 0], [12, 3, 0, 2]]
    # the last table first: |G_3| = 1 + 2, |G_3||G_2| = 3 + 2, the product = 6 + 2
    assert XN.counters(keys, [A, B, A]) == {"n_in": 3, "n_live": 2, "c_unnest": [3, 5, 8], "c_top": 8}
    rc = XN.row_checksums(rows)
    hs = [hj3d.mix64(hj3d.triple_hash(*r[:3]) ^ r[3]) for r in rows.tolist()]
    x = 0
    for h in hs:
        x ^= h
    assert rc == {"n": 8, "sum_a": 84, "sum_row": [12, 12, 8], "sum_h": sum(hs) & X.M64, "xor_h": x}
    # a key without rows in one position silences the whole tuple
    assert XN.expand_rows([1], [[5], [5], [7]], [A, B, A]).shape == (0, 4)
    assert XN.counters([[5], [5], [7]], [A, B, A])["c_unnest"] == [0, 0, 0]


def test_analytic_groups_equal_enumeration(data):
    Sa, Ta, _, _, _ = data
    gs, gt = X.group_index(Sa), X.group_index(Ta)
    keys = [[3], [7], [2]]
    cols = [gs, gt, gs]
    rows = XN.expand_rows([0xFFFFFFF0], keys, cols)
    rc, c = XN.row_checksums(rows), XN.counters(keys, cols)
    got = XN.analytic_groups(0xFFFFFFF0, [g.rows(k[0]) for g, k in zip(cols, keys)])
    assert got == {"n_live": 1, "c_unnest": c["c_unnest"], "c_top": c["c_top"], "sum_a": rc["sum_a"],
                   "sum_row": rc["sum_row"]}
    assert c["c_top"] == len(rows) > 10_000
    dead = XN.analytic_groups(3, [gs.rows(0), gt.rows(9999)])
    assert dead == {"n_live": 0, "c_unnest": [0, 0], "c_top": 0, "sum_a": 0, "sum_row": [0, 0]}
    both = XN.add_results(got, got)
    assert both["c_top"] == 2 * c["c_top"] and both["sum_row"][2] == (2 * rc["sum_row"][2]) & X.M64
    # magnitudes beyond 64 bits stay exact
    big = XN.analytic_groups(1, [np.zeros(1 << 16, np.uint32)] * 4)
    assert big["c_top"] == 1 << 64


def test_sorted_rows_and_sub_multiset():
    r = np.array([[1, 2, 3, 4], [1, 2, 3, 4], [0, 9, 9, 9]], dtype=np.uint32)
    full = XN.sort_rows(r)
    assert len(full) == 3 and XN.is_sub_multiset(r[:2], full) and XN.is_sub_multiset(r[:0], full)
    assert not XN.is_sub_multiset(np.repeat(r[:1], 3, axis=0), full)
    assert not XN.is_sub_multiset(np.array([[1, 2, 3, 5]], dtype=np.uint32), full)
