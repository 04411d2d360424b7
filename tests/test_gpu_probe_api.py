"""Pins the host plumbing around the probe kernels (api.cpp and the launchers it dispatches to): how
many kernels each strand enqueues on every path the dispatch can take, the status of refused calls,
and the overflow bookkeeping of hj3d_probe / hj3d_unnest (result slot words and ctx state) and of
hj3d_probe2 / hj3d_unnest2 (c_top against the capacity).

The launch counts are hj3d_launch_count() deltas of one call after a warm-up call of the same shape
(no allocation in the counted call). They do not depend on the data, only on the shapes and options
below. In every case the result counters must also equal those of the same call under
HJ3D_OPT_FORCE_DIRECT. Integer work: every comparison is exact.
"""
import ctypes as C
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Kernel launches per call, recorded on an MI355X from the library built at commit 78ffd57 (the
# parent of the host-plumbing refactor, which may not change any of them).
EXPECTED_LAUNCHES = {
    "chain_direct_count": 1,
    "chain_direct_nonunique_emit": 6,
    "chain_direct_unique_dense": 1,
    "chain_part_count": 7,
    "chain_part_nonunique_emit": 14,
    "chain_part_unique_dense": 7,
    "nested_direct_agg": 1,
    "nested_direct_aggun": 2,
    "nested_direct_countun": 9,
    "nested_direct_dense": 1,
    "nested_direct_denseref": 1,
    "nested_part_agg": 9,
    "nested_part_aggun": 10,
    "nested_part_countun": 17,
    "nested_part_dense": 9,
    "nested_part_denseref": 9,
    "nested_pk_slices_countun": 18,
    "nested_pk_slices_dense": 10,
    "packed_one_level": 2,
    "packed_refused": 7,
    "packed_two_levels": 3,
    "probe2_chain": 3,
    "probe2_chain_emit": 3,
    "probe2_nested_direct": 3,
    "probe2_nested_direct_emit": 3,
    "probe2_nested_part": 6,
    "probe2_nested_part_emit": 6,
    "sel_accumulate_chain": 10,
    "sel_accumulate_nested": 11,
    "sel_fused_chain": 7,
    "sel_fused_nested": 8,
    "sel_fused_packed": 2,
    "sel_unfused_chain": 10,
    "sel_unfused_nested": 12,
    "unnest": 8,
    "unnest2": 6,
    "unnest2_emit": 6,
    "unnest_ck": 8,
    "unnest_ck_emit": 9,
    "unnest_emit": 9,
}


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def rows3(c0, c1):
    t = np.zeros((len(c0), 3), dtype=np.uint32)
    t[:, 0] = c0
    t[:, 1] = c1
    return t


@contextmanager
def options(ctx, radix_min=1 << 20, packed=True, slice_max=0, unfused=False, direct=False):
    try:
        ctx.radix_min(radix_min)
        ctx.packed_probe(packed)
        ctx.pk_slice_max(slice_max)
        ctx.sel_unfused(unfused)
        ctx.force_direct(direct)
        yield
    finally:
        ctx.radix_min(1 << 20)
        ctx.packed_probe(True)
        ctx.pk_slice_max(0)
        ctx.sel_unfused(False)
        ctx.force_direct(False)


def table(ctx, kind, nb, rel):
    import hj3d
    t = hj3d.Table(ctx, kind, nb)
    t.build(rel)
    t.finish()
    return t


def scatter_refs(out, n):
    import torch
    refs = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    refs[out[:, 0].long()] = out[:, 1]
    return refs


def make_world(ctx):
    """R: 3001 tuples {k, 0, 0} with unique keys (implicit rows). S: 5003 and T: 4001 tuples
    {row, a, 0} (explicit rows) whose a references R.k, some without a partner, one key with 300 rows
    in S and 200 in T. Chaining and nested tables of 2053 / 1500 buckets on each."""
    import torch
    import hj3d
    rng = np.random.default_rng(2024)
    nR, nS, nT, dom = 3001, 5003, 4001, 3300
    Rk = rng.permutation(nR).astype(np.uint32)
    Sa = rng.integers(0, dom, nS).astype(np.uint32)
    Ta = rng.integers(0, dom, nT).astype(np.uint32)
    Sa[rng.choice(nS, 300, replace=False)] = 77
    Ta[rng.choice(nT, 200, replace=False)] = 77
    w = SimpleNamespace(ctx=ctx, nR=nR, nS=nS, nT=nT)
    w.dR, w.dS, w.dT = dev(rows3(Rk, np.zeros(nR))), dev(rows3(np.arange(nS), Sa)), dev(rows3(np.arange(nT), Ta))
    w.R = hj3d.Rel(w.dR, key_word=0)
    w.S = hj3d.Rel(w.dS, key_word=1, row_word=0)
    w.T = hj3d.Rel(w.dT, key_word=1, row_word=0)
    w.cR = table(ctx, hj3d.HJ3D_CHAIN, 2053, w.R)
    w.cS = table(ctx, hj3d.HJ3D_CHAIN, 2053, w.S)
    w.cT = table(ctx, hj3d.HJ3D_CHAIN, 2053, w.T)
    w.nS_ = table(ctx, hj3d.HJ3D_NESTED, 1500, w.S)
    w.nT_ = table(ctx, hj3d.HJ3D_NESTED, 1500, w.T)
    # output sizes of the non-dense forms (every R key below 3001 occurs once)
    w.n_rs = int((Sa < nR).sum())  # pairs of R probing a table on S.a
    cS = np.bincount(Sa, minlength=dom)[:nR].astype(np.int64)
    cT = np.bincount(Ta, minlength=dom)[:nR].astype(np.int64)
    w.c_top = int((cS * cT).sum())
    w.out2 = torch.zeros((max(nS, w.n_rs) + 8, 2), dtype=torch.int32, device="cuda")
    w.out3 = torch.zeros((w.c_top + 8, 3), dtype=torch.int32, device="cuda")
    # stored nested tuples {a, main ref} and triples {a, ref_s, ref_t} for the unnest operators
    w.nested = torch.zeros((nR, 2), dtype=torch.int32, device="cuda")
    ctx.probe(w.nS_, w.R, out=w.nested, mainref=True)
    reft = torch.zeros((nR, 2), dtype=torch.int32, device="cuda")
    ctx.probe(w.nT_, w.R, out=reft, mainref=True)
    w.trip = torch.stack([torch.arange(nR, dtype=torch.int32, device="cuda"), scatter_refs(w.nested, nR),
                          scatter_refs(reft, nR)], dim=1).contiguous()
    w.preds = [(0, "<", 2000)]
    return w


def big_chain(w):
    """2^17 buckets, unique keys, 2^18 probe tuples: with a slice bound of 16 buckets the packed probe
    takes its two partition levels (8192 slices)."""
    import hj3d
    if not hasattr(w, "cBig"):
        rng = np.random.default_rng(5)
        n = 1 << 17
        w.dBigR = dev(rows3(rng.permutation(n), np.zeros(n)))
        w.dBigS = dev(rows3(np.arange(2 * n), rng.integers(0, n + 1000, 2 * n)))
        w.cBig = table(w.ctx, hj3d.HJ3D_CHAIN, n, hj3d.Rel(w.dBigR, key_word=0))
        w.BigS = hj3d.Rel(w.dBigS, key_word=1, row_word=0)
    return w.cBig, w.BigS


def big_nested(w):
    """200,000 buckets in slices of 64: 3125 slices, beyond the one-level probe partitioner's 2048
    (the pk_probe_slices form of the partitioned nested probe)."""
    import hj3d
    if not hasattr(w, "nBig"):
        rng = np.random.default_rng(6)
        nb, nR, nS = 200_000, 100_000, 200_000
        w.dBigNR = dev(rows3(rng.permutation(nR), np.zeros(nR)))
        w.dBigNS = dev(rows3(np.arange(nS), rng.integers(0, nR, nS)))
        w.nBig = table(w.ctx, hj3d.HJ3D_NESTED, nb, hj3d.Rel(w.dBigNS, key_word=1))
        w.BigNR = hj3d.Rel(w.dBigNR, key_word=0)
    return w.nBig, w.BigNR


PART = dict(radix_min=64)
NESTED_MODES = {"agg": {}, "dense": dict(emit=True), "denseref": dict(emit=True, mainref=True),
                "aggun": dict(unnest=True), "countun": dict(unnest=True, emit=True)}


def probe_case(tab, rel, unique=False, unnest=False, emit=False, mainref=False, out_rows=0, **opts):
    def make(w):
        t, r = (tab(w) if callable(tab) else (getattr(w, tab), getattr(w, rel)))
        rows = max(r.n, out_rows)
        out = w.out2 if emit and rows <= w.out2.shape[0] else None
        if emit and out is None:
            import torch
            out = torch.zeros((rows, 2), dtype=torch.int32, device="cuda")
        call = lambda: w.ctx.probe(t, r, unique=unique, unnest=unnest, out=out, mainref=mainref, fetch=False)  # noqa: E731
        return None, call, w.ctx.probe_result
    return opts, make


def sel_case(tab, rel, unique=False, accumulate=False, **opts):
    def make(w):
        import hj3d
        L, ctx = hj3d.lib(), w.ctx
        t, r = getattr(w, tab), getattr(w, rel)
        flags = (hj3d.PROBE_UNIQUE if unique else 0) | hj3d.PROBE_CHECKSUM
        preds = hj3d._sel_preds(w.preds)
        # ACCUMULATE: a strand of two calls over the halves of R, the second one counted
        half = r.n // 2
        a = hj3d.Rel(r.tensor[:half], key_word=0)
        b = hj3d.Rel(r.tensor[half:], key_word=0, row_base=half)

        def sel(rel_, fl):
            st = L.hj3d_probe_sel(ctx.h, t.h, C.byref(rel_.c), preds, 1, fl, None, 0)
            assert st == hj3d.HJ3D_OK, st
        if accumulate:
            return (lambda: sel(a, flags)), (lambda: sel(b, flags | hj3d.PROBE_ACCUMULATE)), ctx.probe_result
        return None, (lambda: sel(r, flags)), ctx.probe_result
    return opts, make


def probe2_case(ts, tt, emit, **opts):
    def make(w):
        out = w.out3[: w.c_top] if emit else None
        call = lambda: w.ctx.probe2(getattr(w, ts), getattr(w, tt), w.R, out=out, fetch=False)  # noqa: E731
        return None, call, w.ctx.probe2_result
    return opts, make


def unnest_case(checksum, emit):
    def make(w):
        out = w.out2[: w.n_rs] if emit else None
        call = lambda: w.ctx.unnest(w.nS_, w.nested, out=out, checksum=checksum, fetch=False)  # noqa: E731
        return None, call, w.ctx.probe_result
    return {}, make


def unnest2_case(emit):
    def make(w):
        out = w.out3[: w.c_top] if emit else None
        call = lambda: w.ctx.unnest2(w.nS_, w.nT_, w.trip, out=out, fetch=False)  # noqa: E731
        return None, call, w.ctx.probe2_result
    return {}, make


CASES = {}
# chaining: S probes the table on R.k (unique: one dense slot per tuple); R probes the table on S.a
for path, opts in (("direct", {}), ("part", dict(PART, packed=False))):
    CASES[f"chain_{path}_count"] = probe_case("cS", "R", **opts)
    CASES[f"chain_{path}_unique_dense"] = probe_case("cR", "S", unique=True, emit=True, **opts)
    CASES[f"chain_{path}_nonunique_emit"] = probe_case("cS", "R", emit=True, **opts)
# the packed unique probe: slices of 512 buckets (one level), of 16 at 2^17 buckets (two levels), and the
# table whose bucket number and quotient do not fit the packed word in one slice (refused: partitioned)
CASES["packed_one_level"] = probe_case("cR", "S", unique=True, emit=True, slice_max=512, **PART)
CASES["packed_refused"] = probe_case("cR", "S", unique=True, emit=True, **PART)
CASES["packed_two_levels"] = probe_case(big_chain, None, unique=True, emit=True, radix_min=64, slice_max=16)
for mode, kw in NESTED_MODES.items():
    CASES[f"nested_direct_{mode}"] = probe_case("nS_", "R", **kw)
    CASES[f"nested_part_{mode}"] = probe_case("nS_", "R", **kw, **PART)
CASES["nested_pk_slices_dense"] = probe_case(big_nested, None, emit=True, radix_min=64, slice_max=64)
CASES["nested_pk_slices_countun"] = probe_case(big_nested, None, unnest=True, emit=True, out_rows=200_000,
                                               radix_min=64, slice_max=64)
CASES["sel_fused_packed"] = sel_case("cR", "R", unique=True, slice_max=512, **PART)
CASES["sel_fused_chain"] = sel_case("cS", "R", **PART)
CASES["sel_fused_nested"] = sel_case("nS_", "R", **PART)
CASES["sel_unfused_chain"] = sel_case("cS", "R", radix_min=64, unfused=True)
CASES["sel_unfused_nested"] = sel_case("nS_", "R", radix_min=64, unfused=True)
CASES["sel_accumulate_chain"] = sel_case("cS", "R", accumulate=True, **PART)
CASES["sel_accumulate_nested"] = sel_case("nS_", "R", accumulate=True, **PART)
for emit in (False, True):
    e = "_emit" if emit else ""
    CASES[f"probe2_nested_part{e}"] = probe2_case("nS_", "nT_", emit, **PART)
    CASES[f"probe2_nested_direct{e}"] = probe2_case("nS_", "nT_", emit)
    CASES[f"probe2_chain{e}"] = probe2_case("cS", "cT", emit, **PART)
    CASES[f"unnest2{e}"] = unnest2_case(emit)
    for ck in (False, True):
        CASES[f"unnest{'_ck' if ck else ''}{e}"] = unnest_case(ck, emit)


def run_case(w, name):
    """(launches of the counted call, its result, the result of the same call under force_direct)."""
    import hj3d
    L, ctx = hj3d.lib(), w.ctx
    opts, make = CASES[name]
    prep, call, result = make(w)

    def strand():
        if prep:
            prep()
        c0 = L.hj3d_launch_count()
        call()
        return L.hj3d_launch_count() - c0
    with options(ctx, **opts):
        strand()  # warm-up: scratch of this shape allocated
        ctx.sync()
        n = strand()
        got = result()
    with options(ctx, direct=True):
        strand()
        want = result()
    return n, got, want


@pytest.fixture(scope="module")
def world(ctx):
    return make_world(ctx)


@pytest.mark.parametrize("name", sorted(CASES))
def test_launch_sequence_length(world, name):
    n, got, want = run_case(world, name)
    print(f"launches {name}: {n}")
    assert got == want
    assert not (got["overflow"] if isinstance(got, dict) else got.overflow)
    assert n == EXPECTED_LAUNCHES[name]


# ---- status matrix ----
def test_status_matrix_probe_and_probe_sel(world):
    import hj3d
    w, L, ctx = world, hj3d.lib(), world.ctx
    EINVAL = hj3d.HJ3D_EINVAL
    E, U, M, A = hj3d.PROBE_EMIT, hj3d.PROBE_UNNEST, hj3d.PROBE_MAINREF, hj3d.PROBE_ACCUMULATE
    out, cap = w.out2.data_ptr(), w.out2.shape[0]
    good = w.R.c
    one = hj3d._sel_preds(w.preds)

    def probe(c=ctx.h, t=w.nS_.h, rel=good, flags=0, ptr=None, n=0):
        return L.hj3d_probe(c, t, C.byref(rel), flags, ptr, n)

    def probe_sel(c=ctx.h, t=w.nS_.h, rel=good, flags=0, ptr=None, n=0, preds=one, npred=1):
        return L.hj3d_probe_sel(c, t, C.byref(rel), preds, npred, flags, ptr, n)

    def rel(stride=12, key_off=0, row_off=hj3d.HJ3D_ROW_IMPLICIT):
        return hj3d._Rel(w.dR.data_ptr(), w.nR, stride, key_off, row_off, 0, 0)

    for entry in (probe, probe_sel):
        assert entry() == hj3d.HJ3D_OK, entry.__name__
        assert entry(c=None) == EINVAL
        assert entry(t=None) == EINVAL
        assert entry(rel=rel(stride=0)) == EINVAL
        assert entry(rel=rel(key_off=2)) == EINVAL
        assert entry(rel=rel(key_off=12)) == EINVAL  # key_off + 4 > stride
        assert entry(flags=E, ptr=None, n=16) == EINVAL
        assert entry(t=w.cS.h, flags=U) == EINVAL
        assert entry(t=w.cS.h, flags=M | E, ptr=out, n=cap) == EINVAL
        assert entry(flags=M | E | U, ptr=out, n=cap) == EINVAL
        assert entry(flags=M) == EINVAL
        assert entry(flags=E, ptr=out, n=cap) == hj3d.HJ3D_OK
    five = hj3d._sel_preds([(0, "<", 2000)] * 5)
    assert probe_sel(preds=five, npred=hj3d.SEL_MAX + 1) == EINVAL
    assert probe_sel(preds=five, npred=hj3d.SEL_MAX) == hj3d.HJ3D_OK
    bad = hj3d._sel_preds(w.preds)
    bad[0].word_off = 2
    assert probe_sel(preds=bad) == EINVAL
    bad[0].word_off = 12  # word_off + 4 > stride
    assert probe_sel(preds=bad) == EINVAL
    bad[0].word_off, bad[0].op = 0, hj3d.SEL_RANGE + 1
    assert probe_sel(preds=bad) == EINVAL
    # hj3d_probe2
    p2 = lambda ts, tt, flags, ptr=None, n=0: L.hj3d_probe2(ctx.h, ts.h, tt.h, C.byref(good), flags, ptr, n)  # noqa: E731
    assert p2(w.nS_, w.cT, 0) == EINVAL
    assert p2(w.cS, w.nT_, 0) == EINVAL
    assert p2(w.nS_, w.nT_, E | A, w.out3.data_ptr(), w.out3.shape[0]) == EINVAL
    assert p2(w.nS_, w.nT_, 0) == hj3d.HJ3D_OK
    ctx.sync()


# ---- overflow bookkeeping ----
PATHS = {"direct": {}, "partitioned": dict(radix_min=64), "packed": dict(radix_min=64, slice_max=512)}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_dense_emit_overflow(world, path):
    """One slot per probe tuple: n - 1 slots overflow, n do not (chaining unique, nested without unnest)."""
    w, ctx = world, world.ctx
    with options(ctx, **PATHS[path]):
        for t, r, kw in ((w.cR, w.S, dict(unique=True)), (w.nS_, w.R, {}), (w.nS_, w.R, dict(mainref=True))):
            full = ctx.probe(t, r, out=w.out2[: r.n], **kw)
            low = ctx.probe(t, r, out=w.out2[: r.n - 1], **kw)
            assert not full.overflow and low.overflow
            assert (low.n_probe, low.n_matched, low.n_out, low.n_cmps) == (full.n_probe, full.n_matched, full.n_out, full.n_cmps)
            # a fresh probe that fits, after the overflowing one
            assert not ctx.probe(t, r, out=w.out2[: r.n], **kw).overflow


@pytest.mark.parametrize("path", sorted(PATHS))
def test_non_dense_emit_overflow(world, path):
    """As many pairs as found: n_out - 1 slots overflow, n_out do not (non-unique chaining, nested
    unnest, hj3d_unnest)."""
    w, ctx = world, world.ctx
    n = w.n_rs
    forms = ((lambda out: ctx.probe(w.cS, w.R, out=out)), (lambda out: ctx.probe(w.nS_, w.R, unnest=True, out=out)),
             (lambda out: ctx.unnest(w.nS_, w.nested, out=out)))
    with options(ctx, **PATHS[path]):
        for f in forms:
            full = f(w.out2[:n])
            low = f(w.out2[: n - 1])
            assert full.n_out == n and not full.overflow
            assert low.overflow and (low.n_probe, low.n_matched, low.n_out) == (full.n_probe, full.n_matched, n)
            assert not f(w.out2[:n]).overflow


@pytest.mark.parametrize("path", sorted(PATHS))
def test_accumulated_strand_keeps_the_first_overflow(world, path):
    """A strand of two calls (the second with ACCUMULATE) of which only the first overflows still
    reports the overflow; dense (nested, one slot per tuple) and non-dense (non-unique chaining,
    nested unnest). A fresh probe afterwards that fits reports none."""
    import hj3d
    w, ctx = world, world.ctx
    half = w.nR // 2
    a = hj3d.Rel(w.dR[:half], key_word=0)
    b = hj3d.Rel(w.dR[half:], key_word=0, row_base=half)
    with options(ctx, **PATHS[path]):
        for t, kw, dense in ((w.nS_, {}, True), (w.cS, {}, False), (w.nS_, dict(unnest=True), False)):
            n_a = half if dense else ctx.probe(t, a, **kw).n_out
            whole = ctx.probe(t, w.R, **kw)
            ctx.probe(t, a, out=w.out2[: n_a - 1], fetch=False, **kw)
            r = ctx.probe(t, b, out=w.out2, accumulate=True, **kw)
            assert r.overflow, (path, dense, kw)
            assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps) == (whole.n_probe, whole.n_matched, whole.n_out, whole.n_cmps)
            # the same strand with room in both calls, then a fresh probe
            ctx.probe(t, a, out=w.out2[:n_a], fetch=False, **kw)
            assert not ctx.probe(t, b, out=w.out2, accumulate=True, **kw).overflow
            ctx.probe(t, a, out=w.out2[: n_a - 1], fetch=False, **kw)
            assert not ctx.probe(t, w.R, out=w.out2, **kw).overflow


@pytest.mark.parametrize("path", ["direct", "partitioned"])
def test_probe2_and_unnest2_overflow(world, path):
    w, ctx = world, world.ctx
    c = w.c_top
    with options(ctx, **PATHS[path]):
        for f in ((lambda out: ctx.probe2(w.nS_, w.nT_, w.R, out=out)), (lambda out: ctx.probe2(w.cS, w.cT, w.R, out=out)),
                  (lambda out: ctx.unnest2(w.nS_, w.nT_, w.trip, out=out))):
            full = f(w.out3[:c])
            low = f(w.out3[: c - 1])
            assert full["c_top"] == c and not full["overflow"]
            assert low["overflow"] and all(low[k] == full[k] for k in full if k != "overflow")
            assert not f(w.out3[:c])["overflow"]
            assert not f(None)["overflow"]
