"""hj3d_select_nested in the C ABI: declared, exported, its predicate struct's layout, refusing null
and invalid arguments without a device, and reachable from the Python layer (CPU suite)."""
import ctypes as C
import inspect

import pytest

import hj3d


def test_declared_and_exported():
    L = hj3d.lib()
    assert "hj3d_select_nested" in hj3d.declared_symbols()
    assert hasattr(L, "hj3d_select_nested")
    assert L.hj3d_select_nested.argtypes is not None and len(L.hj3d_select_nested.argtypes) == 12
    with open(hj3d.HEADER_PATH) as fh:
        text = fh.read()
    assert "HJ3D_NSEL_BASE = 0" in text and "HJ3D_NSEL_COUNT = 1" in text and "HJ3D_NSEL_FIRST = 2" in text
    assert (hj3d.NSEL_BASE, hj3d.NSEL_COUNT, hj3d.NSEL_FIRST) == (0, 1, 2)


def test_predicate_struct_layout():
    # u32 source, u32 slot, then hj3d_sel_pred {u32 word_off, op, is_signed, reserved, i64 lo, hi}
    assert C.sizeof(hj3d._SelPred) == 32
    assert C.sizeof(hj3d._NSelPred) == 40
    assert (hj3d._NSelPred.source.offset, hj3d._NSelPred.slot.offset, hj3d._NSelPred.pred.offset) == (0, 4, 8)


def test_null_and_invalid_arguments_rejected():
    L = hj3d.lib()
    E = hj3d.PROBE_EMIT
    bad = hj3d.HJ3D_EINVAL
    assert L.hj3d_select_nested(None, None, 0, 0, None, None, None, None, 0, 0, None, 0) == bad
    assert L.hj3d_select_nested(None, None, 0, 1, None, None, None, None, 0, E, None, 0) == bad
    tables = (C.c_void_p * 2)(None, None)
    rels = (hj3d._Rel * 2)()
    preds = hj3d._nsel_preds([("count", 1, ">=", 2), ("base", 0, "<", 5)])
    assert L.hj3d_select_nested(None, None, 0, 2, None, tables, rels, preds, 2, E | hj3d.PROBE_CHECKSUM, None, 0) == bad
    # out-of-range k / npred / flags with a null context: still a plain refusal
    assert L.hj3d_select_nested(None, None, 0, hj3d.HJ3D_NEST_MAX + 1, None, None, None, None, 0, 0, None, 0) == bad
    assert L.hj3d_select_nested(None, None, 0, 0, None, None, None, preds, hj3d.SEL_MAX + 1, 0, None, 0) == bad
    assert L.hj3d_select_nested(None, None, 0, 0, None, None, None, None, 0, hj3d.PROBE_UNNEST, None, 0) == bad


def test_predicate_marshalling():
    arr = hj3d._nsel_preds([("base", 2, "range", -3, 9), ("base", 1, "<", 7, None, False), ("count", 3, ">=", 2),
                            ("count", 1, "range", 2, 5), ("first", 2, 1, "!=", -1), ("first", 6, 0, ">", 4, None, False)])
    got = [(p.source, p.slot, p.pred.word_off, p.pred.op, p.pred.is_signed, p.pred.lo, p.pred.hi) for p in arr]
    assert got == [(0, 0, 8, hj3d.SEL_RANGE, 1, -3, 9), (0, 0, 4, hj3d.SEL_LT, 0, 7, 0), (1, 3, 0, hj3d.SEL_GE, 0, 2, 0),
                   (1, 1, 0, hj3d.SEL_RANGE, 0, 2, 5), (2, 2, 4, hj3d.SEL_NE, 1, -1, 0), (2, 6, 0, hj3d.SEL_GT, 0, 4, 0)]
    with pytest.raises(ValueError):
        hj3d._nsel_preds([("group", 1, "<", 2)])


def test_python_surface():
    p = inspect.signature(hj3d.Context.select_nested).parameters
    assert list(p) == ["self", "nested", "preds", "base", "tables", "builds", "out", "checksum", "fetch"]
    assert (p["base"].default, p["tables"].default, p["builds"].default, p["out"].default) == (None, None, None, None)
    assert (p["checksum"].default, p["fetch"].default) == (True, True)
    q = inspect.signature(hj3d.star_plan_chained).parameters
    assert list(q) == ["ctx", "R", "builds", "nb", "keys", "out", "checksum", "filters"]
    assert q["filters"].default is None and q["filters"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert (q["out"].default, q["checksum"].default) == (None, True)
