"""The wide nested-tuple operators in the C ABI (hj3d_probe_refn, hj3d_unnestn, hj3d_unnestn_result):
declared, exported, refusing null handles without a device, and reachable from the Python layer (CPU
suite)."""
import ctypes as C
import inspect

import hj3d

NEW = ("hj3d_probe_refn", "hj3d_unnestn", "hj3d_unnestn_result")


def test_declared_and_exported():
    L = hj3d.lib()
    for name in NEW:
        assert name in hj3d.declared_symbols()
        assert hasattr(L, name)
    assert hj3d.HJ3D_NEST_MAX == 6
    with open(hj3d.HEADER_PATH) as fh:
        assert "#define HJ3D_NEST_MAX 6" in fh.read()


def test_result_struct_layout():
    # n_in, n_live, c_unnest[6], c_top, sum_a, sum_row[6], sum_h, xor_h: 18 u64 words
    assert C.sizeof(hj3d._UnnestNRes) == 8 * (6 + 2 * hj3d.HJ3D_NEST_MAX)
    assert hj3d._UnnestNRes.c_top.offset == 8 * (2 + hj3d.HJ3D_NEST_MAX)
    assert hj3d._UnnestNRes.xor_h.offset == 8 * (5 + 2 * hj3d.HJ3D_NEST_MAX)


def test_null_arguments_rejected():
    L = hj3d.lib()
    assert L.hj3d_probe_refn(None, None, None, None, 0, 0, 0, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_probe_refn(None, None, None, None, 0, 6, hj3d.PROBE_EMIT, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_unnestn(None, None, 0, None, 0, 0, None, 0) == hj3d.HJ3D_EINVAL
    tables = (C.c_void_p * 2)(None, None)
    assert L.hj3d_unnestn(None, tables, 2, None, 0, hj3d.PROBE_EMIT, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_unnestn_result(None, None) == hj3d.HJ3D_EINVAL
    assert L.hj3d_unnestn_result(None, C.byref(hj3d._UnnestNRes())) == hj3d.HJ3D_EINVAL


def test_python_surface():
    p = inspect.signature(hj3d.Context.probe_refn).parameters
    assert list(p)[:4] == ["self", "table", "base", "nested"]
    assert (p["out"].default, p["checksum"].default, p["fetch"].default) == (None, True, True)
    u = inspect.signature(hj3d.Context.unnestn).parameters
    assert list(u)[:3] == ["self", "tables", "nested"]
    assert (u["out"].default, u["checksum"].default, u["fetch"].default) == (None, True, True)
    assert list(inspect.signature(hj3d.Context.unnestn_result).parameters) == ["self"]
    q = inspect.signature(hj3d.star_plan_chained).parameters
    assert list(q)[:5] == ["ctx", "R", "builds", "nb", "keys"]
    assert (q["out"].default, q["checksum"].default) == (None, True)
