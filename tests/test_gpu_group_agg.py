"""hj3d_group_agg on the GPU: {sum, min, max} of a build word over every group of a nested table, as a
column indexed by main ref (the per-group half of aggregation without unnesting; include/hj3d.h).

Expected values: tests/agg_nested_ref.py (numpy; pinned by tests/test_agg_nested_ref.py) over
Table.export() and the host copy of the build relation. Integer work: every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import agg_nested_ref as AN
from test_gpu_expand_limits import cus, scattered
from test_gpu_unnest import dev, exp1_rel
from test_gpu_unnestn import parity  # noqa: F401  (the Zipf fixture: S, T and their two tables)

pytestmark = pytest.mark.gpu

# group_agg.hip's constants (a change there must fail the branch assertions below, not empty the cases)
SHORT = 16           # kGaggShort: largest group a lane folds alone
HOT = 8192           # kGaggHot: largest group a wave folds alone; larger ones go to the hot list
BATCH = 4            # kGaggBatch: rows per lane and step
BLOCK, WAVE = 256, 64
CHUNK = BLOCK * BATCH  # kGaggChunk: rows of a hot group a workgroup takes per step
EDGE = np.array([0, 1, 5, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
CANARY = 0x5A5A5A5A5A5A5A5A
GUARD = 64


def groups_round(n_cus):  # main records k_gagg_groups covers before a workgroup takes its next 256
    return 8 * n_cus * BLOCK


def hot_round(n_cus):  # rows of the hot groups k_gagg_hot covers before a workgroup takes its next chunk
    return 8 * n_cus * CHUNK


def host64(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def canary(rows):
    import torch
    return torch.full((rows + GUARD, 3), CANARY, dtype=torch.int64, device="cuda")


def intact(buf, rows) -> bool:
    return bool((buf[rows:] == CANARY).all())


def relation(rng, col):
    """{row id, key, a word drawn from EDGE} for the key column `col`."""
    col = np.asarray(col, dtype=np.uint32)
    return np.ascontiguousarray(np.stack([np.arange(len(col), dtype=np.uint32), col, EDGE[rng.integers(0, len(EDGE), len(col))]],
                                         axis=1))


def table_of(ctx, d_rel, nb):
    import hj3d
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    t.build(hj3d.Rel(d_rel, key_word=1))
    return t


def check(ctx, t, d_rel, h_rel, word, signed, n=None):
    """group_agg against the model: the column, the counters, nothing written behind n_mains records."""
    import hj3d
    _, payload, sub = t.export()
    m = len(payload)
    want = AN.group_agg(payload, sub, h_rel if n is None else h_rel[:n], word, signed)
    buf = canary(m)
    col, r = t.group_agg(hj3d.Rel(d_rel, key_word=1, n=n), word, signed, out=buf)  # (the capacity exceeds n_mains)
    assert col.shape == (m, 3) and intact(buf, m)
    assert np.array_equal(host64(col), want["col"])
    assert (r.n_probe, r.n_matched, r.n_out, r.sum_a) == (want["n_probe"], want["n_matched"], want["n_out"], want["sum_a"])
    assert (r.n_cmps, r.sum_b, r.sum_c, r.sum_h, r.xor_h, r.overflow) == (0, 0, 0, 0, 0, False)
    return want, payload


# ---- 1. the golden fixtures' tables ----
@pytest.mark.parametrize("signed", [True, False])
def test_exp1_fixture(ctx, signed):
    _, S, nb = exp1_rel("exp1_R1024_S4096_zipf")
    dS = dev(S)
    t = table_of(ctx, dS, nb)
    for word in (0, 1, 2):
        want, payload = check(ctx, t, dS, S, word, signed)
        assert want["n_out"] == t.size()[0] == len(S) and want["n_matched"] == len(payload)
    col, r = t.group_agg(__import__("hj3d").Rel(dS, key_word=1), 0, signed)  # no buffer given: one is made
    assert col.shape == (len(payload), 3) and r.n_out == len(S)
    t.close()


@pytest.mark.parametrize("signed", [True, False])
def test_parity_fixture_tables(ctx, parity, signed):  # noqa: F811
    p = parity
    for t, rel in ((p["ts"], p["S"]), (p["tt"], p["T"])):
        h = rel.cpu().numpy().view(np.uint32)
        for word in (0, 1):
            want, _ = check(ctx, t, rel, h, word, signed)
            assert want["n_out"] == t.size()[0] == 4096


# ---- 2. value edges, and every class bound ----
SIZES = [1, 2, BATCH - 1, BATCH, BATCH + 1, SHORT - 1, SHORT, SHORT + 1, WAVE - 1, WAVE, WAVE + 1,
         WAVE * BATCH - 1, WAVE * BATCH, WAVE * BATCH + 1, HOT - 1, HOT, HOT + 1, HOT + CHUNK, HOT + CHUNK + 1]


@pytest.fixture(scope="module")
def bounds(ctx):
    """Groups of exactly bound - 1, bound, bound + 1 rows for every class bound and batch size, two of
    each, between 300 one-row keys; the words drawn from EDGE."""
    rng = np.random.default_rng(11)
    sizes = np.array(SIZES * 2 + [1] * 300)
    keys = rng.permutation(len(sizes)).astype(np.uint32) + 50
    h = relation(rng, scattered(rng, keys, sizes))
    d = dev(h)
    return {"h": h, "d": d, "t": table_of(ctx, d, 211), "sizes": sizes}


@pytest.mark.parametrize("signed", [True, False])
def test_class_bounds_and_value_edges(ctx, bounds, signed):
    b = bounds
    want, payload = check(ctx, b["t"], b["d"], b["h"], 2, signed)
    lens = np.sort(payload[:, 3])
    assert np.array_equal(lens, np.sort(b["sizes"]))  # the table holds the groups the case is about
    for bound in (SHORT, HOT):
        assert {bound - 1, bound, bound + 1} <= set(lens.tolist())
    assert (lens > HOT).sum() >= 2 and (lens == 1).sum() >= 300  # hot keys next to one-row keys
    # every EDGE value is a minimum and a maximum somewhere (one-row groups), in the chosen order
    one = want["col"][payload[:, 3] == 1]
    assert np.array_equal(one[:, 1], one[:, 2]) and len(np.unique(one[:, 1])) == len(EDGE)
    assert (one[:, 1] >> np.uint64(32) != 0).any() == signed  # sign extension


def test_row_id_word_sums(ctx, bounds):
    """Word 0 is the row id: a group's sum is the sum of its rows of sub."""
    b = bounds
    _, payload, sub = b["t"].export()
    col, _ = b["t"].group_agg(__import__("hj3d").Rel(b["d"], key_word=1), 0, signed=False)
    c = host64(col)
    for m in np.argsort(payload[:, 3])[[0, len(payload) // 2, -3, -1]]:
        rows = sub[payload[m, 2]: payload[m, 2] + payload[m, 3]].astype(np.uint64)
        assert (int(c[m, 0]), int(c[m, 1]), int(c[m, 2])) == (int(rows.sum()), int(rows.min()), int(rows.max()))


# ---- 3. the hot path beyond one workgroup and one grid round; the short class beyond one grid round ----
@pytest.mark.parametrize("signed", [True, False])
def test_hot_keys_past_one_grid_round(ctx, signed):
    n_cus = cus()
    rng = np.random.default_rng(13)
    sizes = np.array([hot_round(n_cus) + CHUNK + 77, HOT + 3 * CHUNK + 5, HOT + 1] + [1] * 1000)
    assert sizes[0] > hot_round(n_cus) and sizes[1] > 2 * CHUNK  # more than one round; more than one workgroup
    keys = rng.permutation(len(sizes)).astype(np.uint32) + 7
    h = relation(rng, scattered(rng, keys, sizes))
    d = dev(h)
    t = table_of(ctx, d, 509)
    want, payload = check(ctx, t, d, h, 2, signed)
    assert (payload[:, 3] > HOT).sum() == 3 and len(payload) == len(sizes)
    # a shorter relation under the hot path: skipped rows, groups not folded whole
    cut = len(h) - len(h) // 3
    short, _ = check(ctx, t, d, h, 2, signed, n=cut)
    assert short["n_out"] == cut and short["n_matched"] < want["n_matched"] == len(payload)
    t.close()


def test_more_main_records_than_one_grid_round(ctx):
    n_cus = cus()
    rng = np.random.default_rng(17)
    nk = groups_round(n_cus) + 3 * BLOCK + 9
    sizes = np.ones(nk, dtype=np.int64)
    sizes[::1001] = 2
    sizes[5::40_003] = SHORT + 1
    h = relation(rng, scattered(rng, np.arange(nk, dtype=np.uint32), sizes))
    d = dev(h)
    t = table_of(ctx, d, nk)
    _, payload = check(ctx, t, d, h, 2, True)
    assert len(payload) == nk > groups_round(n_cus)
    t.close()


# ---- 4. lifecycle and guards ----
def test_lifecycle(ctx):
    import hj3d
    rng = np.random.default_rng(19)
    h = relation(rng, scattered(rng, np.arange(200, dtype=np.uint32), 1 + np.arange(200) % 7))
    d = dev(h)
    t = table_of(ctx, d, 97)
    want, payload = check(ctx, t, d, h, 2, True)
    m = len(payload)
    assert m == 200
    # fewer output records than main records: refused, nothing written
    buf = canary(m)
    with pytest.raises(hj3d.Hj3dError) as e:
        t.group_agg(hj3d.Rel(d, key_word=1), 2, out=buf[:m - 1])
    assert e.value.status == hj3d.HJ3D_EOVERFLOW and bool((buf == CANARY).all())
    # a relation shorter than the one the table was built from
    half = len(h) // 2
    short, _ = check(ctx, t, d, h, 2, False, n=half)
    assert short["n_out"] == half and 0 < short["n_matched"] < short["n_probe"] == m
    none = (short["col"][:, 0] == 0) & (short["col"][:, 1] == AN.M64) & (short["col"][:, 2] == 0)
    assert none.any()  # groups with no folded row: the identities
    empty, _ = check(ctx, t, d, h, 2, True, n=0)
    assert (empty["n_out"], empty["n_matched"]) == (0, 0) and (empty["col"][:, 1] == AN.I64_MAX).all()
    # rebuilt smaller (the call finishes the pending build)
    h2 = relation(rng, scattered(rng, np.arange(50, dtype=np.uint32) + 1000, 1 + np.arange(50) % 5))
    d2 = dev(h2)
    t.build(hj3d.Rel(d2, key_word=1))
    _, payload2 = check(ctx, t, d2, h2, 2, True)
    assert len(payload2) == 50
    # cleared: nothing written, zeros
    t.clear()
    buf = canary(8)
    col, r = t.group_agg(hj3d.Rel(d2, key_word=1), 2, out=buf)
    assert col.shape == (0, 3) and bool((buf == CANARY).all())
    assert (r.n_probe, r.n_matched, r.n_out, r.sum_a, r.overflow) == (0, 0, 0, 0, False)
    assert hj3d.lib().hj3d_group_agg(ctx.h, t.h, C.byref(hj3d.Rel(d2, key_word=1).c), 8, 1, None, 0) == hj3d.HJ3D_OK
    t.close()


def test_refusals(ctx, bounds):
    import torch
    import hj3d
    L = hj3d.lib()
    b = bounds
    rel = hj3d.Rel(b["d"], key_word=1)
    explicit = hj3d.Rel(b["d"], key_word=1, row_word=0)
    m = b["t"].size()[1]
    out = torch.zeros((m, 3), dtype=torch.int64, device="cuda")
    tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, 64)
    tc.build(rel)

    def st(c=ctx.h, t=b["t"].h, r=rel, word_off=8, signed=1, optr=out.data_ptr(), cap=m):
        return L.hj3d_group_agg(c, t, None if r is None else C.byref(r.c), word_off, signed, optr, cap)

    bad = hj3d.HJ3D_EINVAL
    assert st() == hj3d.HJ3D_OK
    assert st(c=None) == bad and st(t=None) == bad and st(r=None) == bad
    assert st(t=tc.h) == bad
    assert st(r=explicit) == bad
    broken = hj3d.Rel(b["d"], key_word=1)
    broken.c.stride = 10
    assert st(r=broken) == bad
    assert st(word_off=2) == bad and st(word_off=12) == bad and st(word_off=0xFFFFFFFC) == bad
    assert st(optr=out.data_ptr() + 4) == bad
    assert st(optr=None) == bad
    assert st(cap=m - 1) == hj3d.HJ3D_EOVERFLOW and st(cap=0) == hj3d.HJ3D_EOVERFLOW
    assert st(signed=0) == hj3d.HJ3D_OK
    with pytest.raises(ValueError):
        b["t"].group_agg(rel, 2, out=torch.zeros((m, 2), dtype=torch.int64, device="cuda"))
    tc.close()
