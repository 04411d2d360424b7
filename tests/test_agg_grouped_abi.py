"""hj3d_agg_grouped in the C ABI (hj3d_agg_grouped, hj3d_agg_grouped_result): declared, exported, refusing
null handles without a device, its spec struct laid out as the header's, and reachable from the Python layer
(CPU suite)."""
import ctypes as C
import inspect
import re

import hj3d

NEW = ("hj3d_agg_grouped", "hj3d_agg_grouped_result")


def test_declared_and_exported():
    L = hj3d.lib()
    for name in NEW:
        assert name in hj3d.declared_symbols()
        assert hasattr(L, name)
    with open(hj3d.HEADER_PATH) as fh:
        text = fh.read()
    assert re.search(r"HJ3D_OPT_GBY_FORM\s*=\s*18\b", text) and hj3d.OPT_GBY_FORM == 18


def test_spec_struct_layout():
    """hj3d_gby_spec: four u32, a pointer, a u64, in the header's order (ctypes arithmetic; the header's
    field list is read from the file)."""
    with open(hj3d.HEADER_PATH) as fh:
        text = fh.read()
    body = re.search(r"typedef struct \{([^}]*)\} hj3d_gby_spec;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const void\*|uint32_t|uint64_t)\s+(.*)", decl)
        ctype, names = m.group(1), [x.strip() for x in m.group(2).split(",")]
        fields += [(nm, ctype) for nm in names]
    assert fields == [("op", "uint32_t"), ("slot", "uint32_t"), ("is_signed", "uint32_t"), ("word_off", "uint32_t"),
                      ("gcol", "const void*"), ("gcol_n", "uint64_t")]
    size = {"uint32_t": 4, "uint64_t": 8, "const void*": C.sizeof(C.c_void_p)}
    off = 0
    for (nm, ctype), (pname, ptype) in zip(fields, hj3d._GbySpec._fields_):
        off = (off + size[ctype] - 1) // size[ctype] * size[ctype]  # natural alignment
        assert nm == pname and C.sizeof(ptype) == size[ctype]
        assert getattr(hj3d._GbySpec, nm).offset == off, nm
        off += size[ctype]
    assert C.sizeof(hj3d._GbySpec) == (off + 7) // 8 * 8 == 32
    # the result is hj3d_agg_nested's struct
    assert C.sizeof(hj3d._AggNRes) == 8 * (3 + hj3d.AGG_MAX)


def test_null_arguments_rejected():
    L = hj3d.lib()
    tables = (C.c_void_p * 2)(None, None)
    specs = (hj3d._GbySpec * 1)(hj3d._GbySpec(hj3d.AGG_COUNT, 0, 0, 0, None, 0))
    assert L.hj3d_agg_grouped(None, None, 0, 0, None, 0, None, None, 0, 0, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_agg_grouped(None, None, 0, 2, tables, 1, None, specs, 1, 0, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_agg_grouped(None, None, 0, 2, tables, 1, None, specs, 1, hj3d.PROBE_ACCUMULATE, None, 0) == hj3d.HJ3D_EINVAL
    assert L.hj3d_agg_grouped_result(None, None) == hj3d.HJ3D_EINVAL
    assert L.hj3d_agg_grouped_result(None, C.byref(hj3d._AggNRes())) == hj3d.HJ3D_EINVAL


def test_python_surface():
    p = inspect.signature(hj3d.Context.agg_grouped).parameters
    assert list(p)[:5] == ["self", "nested", "tables", "by", "specs"]
    assert (p["base"].default, p["out"].default, p["accumulate"].default, p["fetch"].default) == (None, None, False, True)
    assert list(inspect.signature(hj3d.Context.agg_grouped_result).parameters) == ["self"]
    assert list(inspect.signature(hj3d.Context.gby_form).parameters) == ["self", "f"]
    q = inspect.signature(hj3d.star_plan_grouped).parameters
    assert list(q)[:7] == ["ctx", "R", "builds", "nb", "keys", "by", "aggregate"]
    assert (q["filters"].default, q["out"].default) == (None, None)
