"""CPU side of the stream-ordering tests: for every case of tests/test_gpu_streams.py the reference
result of the decoy differs from that of the real data, so a library that read the decoy (work on the
wrong stream, or work that ran after the clobber) cannot pass; and the parts of the harness
(tests/stream_order.py) that need no device.

Probes and operators must differ in n_out, n_cmps and sum_h wherever the operator computes the
field (an unnest compares nothing: its n_cmps is 0 for any input; hj3d_agg_nested and hj3d_group_agg
report totals and a column instead of hashes). Builds must differ in distinct and cc0_max: `entries`
of a full table is its build relation's tuple count, which a decoy of the same shape cannot change,
so the bucket offsets are compared as well."""
import numpy as np
import pytest

import stream_cases as SC
import stream_order as SO
import tablestruct as TS
import test_gpu_probe_api as PA
import test_gpu_streams as GS
import test_gpu_table_lifecycle as LC


def test_delay_target_and_the_failure_of_its_own():
    assert SO.target_ms(0.0) == SO.target_ms(1.25) == 5.0 and SO.target_ms(2.0) == 8.0
    e = SO.too_short("case", 5.2, 7.1)
    assert isinstance(e, AssertionError) and str(e).startswith("delay too short: case")


def test_every_case_is_classified_and_every_dispatch_path_is_a_case():
    assert set(SC.PROBES) | set(SC.PROBE2) | set(GS.UNNEST_KEYS) == set(PA.EXPECTED_LAUNCHES) | {"packed_zipf_overflow"}
    assert set(GS.UNNEST_KEYS.values()) <= set(SC.OPERATORS) and len(set(GS.UNNEST_KEYS.values())) == 6
    assert set(GS.NOT_ASYNC) <= set(GS.CASE_NAMES) and len(set(GS.CASE_NAMES)) == len(GS.CASE_NAMES)
    assert set(GS.BUILDS) == set(LC.SELECTIONS) | set(LC.MORE_SELECTIONS) | {"giveup_then_sort_sync"}
    for name in ("sel_unfused_chain", "slices", "nested_sort"):
        assert not GS.FULLY_ASYNC[name]
    for name in ("radix", "giveup_then_sort", "packed_two_levels", "unnestn", "unnest_count", "comm_exchange", "two_contexts"):
        assert GS.FULLY_ASYNC[name]


def test_the_world_is_that_of_the_probe_api_tests():
    """Same seeds, same draws as test_gpu_probe_api.make_world / big_chain / big_nested (the GPU module
    compares the device relations with these arrays)."""
    w = SC.world()
    assert (len(w.R), len(w.S), len(w.T)) == (3001, 5003, 4001)
    assert int((w.S[:, 1] == 77).sum()) >= 300 and int((w.T[:, 1] == 77).sum()) >= 200
    assert np.array_equal(np.sort(w.R[:, 0]), np.arange(3001))


@pytest.mark.parametrize("name", sorted(SC.PROBES))
def test_probe_decoy_differs(name):
    case = SC.PROBES[name]
    _, real, _ = SC.probe_arrays(case)
    a, _ = SC.probe_expected(case, real)
    b, _ = SC.probe_expected(case, SC.decoy_rel(real, case["pkey"]))
    assert a["n_out"] > 0 and a["n_out"] != b["n_out"] and a["n_cmps"] != b["n_cmps"]
    if "sum_h" in a:
        assert a["sum_h"] != b["sum_h"]


@pytest.mark.parametrize("name", sorted(SC.PROBE2))
def test_probe2_decoy_differs(name):
    case, R = SC.PROBE2[name], SC.world().R
    a, b = SC.probe2_expected(case, R), SC.probe2_expected(case, SC.decoy_rel(R, 0))
    assert a["c_top"] > 0
    for k in ("c_top", "c_probe_rs_cmp", "c_probe_rt_cmp", "sum_h"):
        assert a[k] != b[k], k


@pytest.mark.parametrize("name", list(GS.BUILDS) + ["build_many"])
def test_build_decoy_differs(name):
    for shape in (["nested", "nested_other"] if name == "build_many" else [GS.BUILDS[name][0]]):
        real = SC.build_tuples(shape)
        kind, keys, nb = TS.shape(shape)
        a, b = SC.build_stats(shape, real), SC.build_stats(shape, SC.decoy_build(real, 1))
        assert a["entries"] == len(real) > 0
        assert a["distinct"] != b["distinct"] and a["cc0_max"] != b["cc0_max"], (a, b)
        rows = np.arange(len(real), dtype=np.uint32)
        struct = TS.chain_struct if kind == TS.CHAIN else TS.nested_struct
        assert not np.array_equal(struct(real[:, 1], rows, nb)["off"], struct(SC.decoy_build(real, 1)[:, 1], rows, nb)["off"])


@pytest.mark.parametrize("op", SC.OPERATORS)
def test_operator_decoy_differs(op):
    """On numpy-laid tables (agg_nested_ref.table_arrays): the counters do not depend on the layout."""
    import agg_nested_ref as AN
    w = SC.world()
    pairs, trip, (mains_s, sub_s), (mains_t, sub_t) = SC.model_tuples()
    col_s = AN.group_agg(mains_s, sub_s, w.S, SC.AGG_WORD, True)["col"]
    col_t = AN.group_agg(mains_t, sub_t, w.T, SC.AGG_WORD, True)["col"]
    base_op, checksum, _, _ = SC.UNNEST_FORMS.get(op, (op, True, True, None))
    nested = {"unnest": pairs, "probe_ref": pairs, "unnestn": SC.wide_tuples(trip), "group_agg": None}.get(base_op, trip)
    kw = dict(mains_s=mains_s, mains_t=mains_t, sub_s=sub_s, col_s=col_s, col_t=col_t)
    a, rows_a = SC.operator_expected(op, w.R, w.S, nested, **kw)
    late = dict(kw, col_s=SC.decoy_column(col_s), col_t=SC.decoy_column(col_t))
    b, rows_b = SC.operator_expected(op, SC.decoy_rel(w.R, 0), SC.decoy_rel(w.S, 0),
                                     None if nested is None else SC.decoy_nested(nested), **late)
    assert rows_a is None or len(rows_a) > 0
    if op in SC.UNNEST_FORMS:
        size = "n_out" if base_op == "unnest" else "c_top"
        assert a[size] > 0 and a[size] != b[size] and a["sum_a"] != b["sum_a"]
        assert (a["sum_h"] != b["sum_h"]) if checksum else (a["sum_h"] == 0)
    elif op == "group_agg":
        assert a["sum_a"] != b["sum_a"] and not np.array_equal(rows_a, rows_b)
    elif op == "agg_nested":
        assert a["c_top"] != b["c_top"] and a["total"] != b["total"] and a["n_live"] != b["n_live"]
    elif op in ("unnest2", "unnestn"):
        assert a["c_top"] != b["c_top"] and a["sum_h"] != b["sum_h"]
    else:
        assert a["n_out"] > 0 and a["n_out"] != b["n_out"]
        if op in ("probe_ref", "probe_refn"):
            assert a["n_cmps"] != b["n_cmps"]
        else:
            assert a["sum_h"] != b["sum_h"]


def test_exchange_decoys_differ():
    real = SC.xrel()
    decoy = SC.decoy_rel(real, 1)
    for preds in (None, SC.X_PREDS):
        (ca, pa), (cb, pb) = SC.partition_expected(real, preds), SC.partition_expected(decoy, preds)
        assert ca != cb and min(ca) > 0 and (pa.shape != pb.shape or not np.array_equal(pa, pb))
    (bm_a, out_a, dv_a), (bm_b, out_b, dv_b) = SC.bitmap_expected(real), SC.bitmap_expected(decoy)
    assert (out_a, dv_b) == (0, 0) and dv_a > 0 and out_b == len(real) and not np.array_equal(bm_a, bm_b)


def test_ticketed_exchange_decoy_differs():
    real, _ = SC.comm_case()
    a, b = SC.comm_expected(real), SC.comm_expected(SC.decoy_rel(real, 0))
    assert a["n_out"] > 0
    for k in ("n_out", "n_cmps", "sum_h"):
        assert a[k] != b[k], k


@pytest.mark.parametrize("rnd", range(SC.TWO_ROUNDS))
def test_two_contexts_decoys_differ(rnd):
    """Every round, the warm-up included: a probe over a decoy relation, or of a table built from a decoy,
    reports other n_out, n_cmps and sum_h; the tables built from the decoys have other statistics."""
    r = SC.two_ctx_round(rnd)
    (RA, SA, SB, RB), (dRA, dSA, dSB, dRB) = r.real, r.decoy
    eA, eB = SC.two_ctx_expected(RA, SA, SB, RB)
    late_probes = SC.two_ctx_expected(RA, dSA, SB, dRB)
    late_builds = SC.two_ctx_expected(dRA, SA, dSB, RB)
    for e, others in ((eA, (late_probes[0], late_builds[0])), (eB, (late_probes[1], late_builds[1]))):
        assert e.out["n"] > 0
        for o in others:
            assert (e.out["n"], e.c_cmp, e.out["sum_h"]) != (o.out["n"], o.c_cmp, o.out["sum_h"])
            assert e.out["n"] != o.out["n"] and e.c_cmp != o.c_cmp and e.out["sum_h"] != o.out["sum_h"]
    for a, b in zip(SC.two_ctx_stats(RA, SB), SC.two_ctx_stats(dRA, dSB)):
        assert a["distinct"] != b["distinct"] and a["cc0_max"] != b["cc0_max"], (a, b)
    if rnd:  # other data every round
        assert not np.array_equal(RA, SC.two_ctx_round(rnd - 1).real[0])


def test_partition_model_follows_part_range():
    """The host arithmetic of hj3d_part_range, which the partition model restates: the ranges tile
    [0, NB) and differ by at most one bucket."""
    b = SC.part_bounds(SC.X_NB, SC.X_PARTS)
    assert b[0] == 0 and b[-1] == SC.X_NB and max(np.diff(b)) - min(np.diff(b)) <= 1
