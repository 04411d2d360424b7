"""The chained nested probe in the C ABI (hj3d_probe_ref): declared, exported, refusing null handles
without a device, and reachable from the Python layer (CPU suite)."""
import inspect

import hj3d


def test_probe_ref_declared_and_exported():
    L = hj3d.lib()
    assert "hj3d_probe_ref" in hj3d.declared_symbols()
    assert hasattr(L, "hj3d_probe_ref")


def test_probe_ref_null_arguments_rejected():
    L = hj3d.lib()
    assert L.hj3d_probe_ref(None, None, None, None, 0, 0, 0, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_probe_ref(None, None, None, None, 0, 2, hj3d.PROBE_EMIT, None, 0) == hj3d.HJ3D_EINVAL


def test_probe_ref_python_surface():
    p = inspect.signature(hj3d.Context.probe_ref).parameters
    assert list(p)[:4] == ["self", "table", "base", "nested"]
    assert (p["out"].default, p["checksum"].default, p["fetch"].default) == (None, True, True)
    q = inspect.signature(hj3d.exp4_plan_chained).parameters
    assert list(q)[:5] == ["ctx", "R", "S", "T", "nb"]
    assert (q["keys"].default, q["out"].default, q["checksum"].default) == ((0, 0), None, True)
