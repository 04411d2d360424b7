"""The deferred-unnest entry points in the C ABI (hj3d_unnest, hj3d_unnest2, HJ3D_PROBE_MAINREF):
declared, exported, and refusing null handles without a device (CPU suite)."""
import hj3d


def test_unnest_entry_points_declared_and_exported():
    L = hj3d.lib()
    declared = hj3d.declared_symbols()
    for name in ("hj3d_unnest", "hj3d_unnest2"):
        assert name in declared, name
        assert hasattr(L, name), name


def test_unnest_null_arguments_rejected():
    L = hj3d.lib()
    assert L.hj3d_unnest(None, None, None, 0, 0, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_unnest2(None, None, None, None, 0, 0, None, 0) == hj3d.HJ3D_EINVAL


def test_mainref_flag_value():
    assert hj3d.PROBE_MAINREF == 0x20
    others = (hj3d.PROBE_UNIQUE, hj3d.PROBE_UNNEST, hj3d.PROBE_EMIT, hj3d.PROBE_CHECKSUM, hj3d.PROBE_ACCUMULATE)
    assert len({hj3d.PROBE_MAINREF, *others}) == 6
    assert all(hj3d.PROBE_MAINREF & f == 0 for f in others)
    # the header carries the same value
    import re
    text = open(hj3d.HEADER_PATH).read()
    assert int(re.search(r"#define\s+HJ3D_PROBE_MAINREF\s+(0x[0-9a-fA-F]+)u", text).group(1), 16) == hj3d.PROBE_MAINREF
