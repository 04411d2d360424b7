"""The contents hj3d_table_export hands out, and one table object living through several contents.

Structure: for every build path (chaining radix / slices / direct, nested nested_agg / nested_agg_reg /
nested_agg_slices / nested_agg_slices_reg / nested_sort, the aggregation build that gives up and is
replaced by the sort build, the slice build that gives up and is replaced by the direct build) the
exported arrays equal tests/tablestruct.py's "group the build tuples by
bucket and key": CSR offsets, chaining entries (buckets of <= 32 entries in row order), nested main
records {hash, first_row, sub_len} per bucket and each key's rows as a set, the sub ranges disjoint
inside [0, n_sub). The same with explicit row ids and on a bucket-range shard fed the whole relation.

Reuse: one table rebuilt from other relations, sizes and paths, emptied (hj3d_table_clear) and
pre-sized (hj3d_table_reserve) gives, after every step, the export, statistics, size, build path and
probe results of a fresh table given only that step.

All of it integer work: every comparison is exact. Every case asserts the build path it names."""
import contextlib
import functools

import numpy as np
import pytest

import oracle as O
import tablestruct as TS

pytestmark = pytest.mark.gpu

SORTED_MAX = 32  # hj3d.h: chaining buckets of <= 32 entries come sorted by row
OPTION_DEFAULTS = dict(radix_min=1 << 20, force_direct=False, nested_sort=False, nested_pk=False, pk_build=False,
                       rp_unfused=False, diag_lookback=0)
RM0 = dict(radix_min=0)

# name -> (shape of tablestruct.shape, context options, the build path they select)
SELECTIONS = {
    "radix": ("chain", RM0, "radix"),
    "direct": ("chain", dict(force_direct=True), "direct"),
    "slices": ("slices", dict(radix_min=0, pk_build=True), "slices"),
    "nested_agg": ("nested", RM0, "nested_agg"),
    "nested_agg_reg": ("nested_reg", RM0, "nested_agg_reg"),
    "nested_agg_slices": ("nested", dict(radix_min=0, nested_pk=True), "nested_agg_slices"),
    "nested_agg_slices_reg": ("nested_reg", dict(radix_min=0, nested_pk=True), "nested_agg_slices_reg"),
    "nested_sort": ("nested", dict(radix_min=0, nested_sort=True), "nested_sort"),
    "giveup_then_sort": ("nested_giveup", RM0, "nested_sort"),
}
# Two more routes of the slice build: at fill 1.3 its fine regions exceed the register-held form (the
# in-kernel HBM path of k_pk_build); and its own give-up, where a key with ~5 % of the rows overflows
# the partitioner's regions and the direct build runs instead.
MORE_SELECTIONS = {
    "slices_fill13": ("slices_fill13", dict(radix_min=0, pk_build=True), "slices"),
    "slices_overflow_then_direct": ("slices_hot", dict(radix_min=0, pk_build=True), "direct"),
}


@contextlib.contextmanager
def options(ctx, **kw):
    """Context options set for the block and put back to their defaults after it."""
    try:
        for k, v in kw.items():
            getattr(ctx, k)(v)
        yield
    finally:
        for k in kw:
            getattr(ctx, k)(OPTION_DEFAULTS[k])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


class Data:
    """A build relation {0, key, row}: key word 1; row word 2 holds explicit row ids when `explicit`
    (ascending with gaps), else the rows are the indices. n: only the first n tuples of the shape."""

    def __init__(self, name, explicit=False, n=None):
        self.name = name
        self.kind, keys, self.nb = TS.shape(name)
        self.keys = keys if n is None else keys[:n]
        m = len(self.keys)
        self.explicit = explicit
        if explicit:
            rng = np.random.default_rng(m)
            self.rows = np.sort(rng.choice(2_000_000_000, m, replace=False)).astype(np.uint32)
        else:
            self.rows = np.arange(m, dtype=np.uint32)
        self.tuples = np.zeros((m, 3), np.uint32)
        self.tuples[:, 1] = self.keys
        self.tuples[:, 2] = self.rows

    @functools.cached_property
    def device(self):
        return dev(self.tuples)

    def rel(self):
        import hj3d
        return hj3d.Rel(self.device, 1, row_word=2 if self.explicit else None)

    @functools.cached_property
    def probe_tuples(self):
        """Probe side {key, 0, 0}: half of its keys drawn from the build keys, half from the whole
        range the build keys span (partners, duplicates and misses), 120 000 tuples."""
        rng = np.random.default_rng(len(self.keys) + 1)
        m = 60_000
        a = self.keys[rng.integers(0, len(self.keys), m)] if len(self.keys) else np.zeros(0, np.uint32)
        hi = int(self.keys.max()) + 2 if len(self.keys) else 1000
        b = rng.integers(0, hi, 2 * m - len(a), dtype=np.uint64).astype(np.uint32)
        return O.tuples3(np.concatenate([a, b]), np.zeros(2 * m, np.uint32))

    @functools.cached_property
    def probe_device(self):
        return dev(self.probe_tuples)

    def owned_tuples(self, lo, hi):
        """The tuples a shard [lo, hi) stores, as a relation with explicit rows (for the oracle, which
        has no bucket ranges: the other buckets stay empty and compare nothing)."""
        b = (TS.fmix32(self.keys).astype(np.uint64) % np.uint64(self.nb)).astype(np.int64)
        return self.tuples[(b >= lo) & (b < hi)]

    @functools.lru_cache(maxsize=None)
    def oracle(self, flag, lo=0, hi=None):
        """chaining: flag = unique; nested: flag = unnest."""
        B = self.tuples if hi is None else self.owned_tuples(lo, hi)
        plan = O.chain_plan if self.kind == TS.CHAIN else O.nested_plan
        return plan(B, 1, self.probe_tuples, 0, self.nb, flag, brow=2)


@functools.lru_cache(maxsize=None)
def _data(name, explicit, n):
    return Data(name, explicit, n)


def data(name, explicit=False, n=None):
    return _data(name, bool(explicit), n)


EMPTY = {TS.CHAIN: "chain", TS.NESTED: "nested"}


def empty_data(kind):
    return data(EMPTY[kind], n=0)


# ---- the checks ----

def check_chain_export(t, d, lo=0, hi=None, ordered=True):
    """Export of a chaining table against the reference; returns the statistics recomputed from it."""
    ref = TS.chain_struct(d.keys, d.rows, d.nb, lo, hi)
    off, ent, sub = t.export()
    assert len(sub) == 0 and ent.shape == (len(ref["ent"]), 2), (ent.shape, len(ref["ent"]), len(sub))
    assert np.array_equal(off, ref["off"])
    ln = np.diff(ref["off"])
    local = np.repeat(np.arange(len(ln)), ln)
    order = np.lexsort((ent[:, 1], local))
    assert np.array_equal(ent[order], ref["ent"])
    # buckets of <= 32 entries: the exported order itself ascends by row
    small = ln[local] <= SORTED_MAX
    assert np.array_equal(ent[small], ref["ent"][small])
    if ordered:  # (not vacuous: long buckets beside many short ones in which an order exists)
        assert (ln > SORTED_MAX).sum() >= 1 and ((ln >= 2) & (ln <= SORTED_MAX)).sum() >= 1000, d.name
    return TS.stats_from(off, ent[:, 0])


def check_nested_export(t, d, lo=0, hi=None):
    """Export of a nested table against the reference; returns the statistics recomputed from it."""
    ref = TS.nested_struct(d.keys, d.rows, d.nb, lo, hi)
    full = lo == 0 and hi is None
    off, mains, sub = t.export()
    assert mains.shape == (len(ref["hash"]), 4), (mains.shape, len(ref["hash"]))
    assert np.array_equal(off, ref["off"])
    local = np.repeat(np.arange(len(off) - 1), np.diff(ref["off"]))
    m = mains[np.lexsort((mains[:, 0], local))]  # per bucket by hash, as the reference
    assert np.array_equal(m[:, 0], ref["hash"])
    assert np.array_equal(m[:, 1], ref["first_row"])
    assert np.array_equal(m[:, 3], ref["sub_len"])
    # the ranges [sub_off, sub_off + sub_len): inside [0, n_sub), pairwise disjoint
    so, sl = m[:, 2].astype(np.int64), m[:, 3].astype(np.int64)
    n_sub = len(sub)
    assert n_sub == len(d.keys)  # the extent of sub: the build relation's tuples
    assert (sl >= 1).all() and (so + sl <= n_sub).all()
    cover = np.zeros(n_sub + 1, np.int64)
    np.add.at(cover, so, 1)
    np.add.at(cover, so + sl, -1)
    cover = np.cumsum(cover)[:n_sub]
    assert (cover <= 1).all()
    # positions outside every range (a shard fed tuples of other buckets) belong to no main record:
    # there are exactly n_sub - stored rows of them, none for a table that stores every tuple
    assert int((cover == 0).sum()) == n_sub - ref["n_rows"]
    if full:
        assert (cover == 1).all()  # the ranges tile [0, n)
    # the rows of each range, as a set
    key_of = np.repeat(np.arange(len(sl)), sl)
    pos = np.repeat(so - (np.cumsum(sl) - sl), sl) + np.arange(int(sl.sum()))
    got = sub[pos]
    got = got[np.lexsort((got, key_of))]
    want = np.concatenate(ref["rows"]) if ref["rows"] else np.zeros(0, np.uint32)
    assert np.array_equal(got, want)
    return TS.stats_from(off, np.repeat(m[:, 0], sl))


def check_export(t, d, lo=0, hi=None, ordered=True):
    if d.kind == TS.CHAIN:
        st = check_chain_export(t, d, lo, hi, ordered)
    else:
        st = check_nested_export(t, d, lo, hi)
    got = t.stats()
    assert {k: got[k] for k in TS.STAT_KEYS} == st
    assert t.size() == (st["entries"], st["distinct"])
    return st


def probe_fields(r):
    return {f: getattr(r, f) for f in ("n_probe", "n_matched", "n_out", "n_cmps", "sum_a", "sum_b", "sum_h", "xor_h")}


def expected_probe(d, flag, lo=0, hi=None):
    """The oracle's counters in hj3d_probe_res's terms (chaining: n_out = c_probe; nested:
    n_matched = c_probe, n_out = c_unnest with unnest, else the matched probe tuples)."""
    e = d.oracle(flag, lo, hi)
    out = {"n_probe": len(d.probe_tuples), "n_cmps": e.c_cmp, "n_out": e.out["n"],
           "sum_a": e.out["sum_a"], "sum_b": e.out["sum_b"], "sum_h": e.out["sum_h"], "xor_h": e.out["xor_h"]}
    if d.kind == TS.NESTED:
        out["n_matched"] = e.c_probe
        assert out["n_out"] == (e.c_unnest if flag else e.c_probe)
    else:
        assert out["n_out"] == e.c_probe
    return out


def probes(ctx, t, d):
    """Both probe forms of the table's kind over d's probe side."""
    import hj3d
    rel = hj3d.Rel(d.probe_device, 0)
    if d.kind == TS.CHAIN:
        return {flag: probe_fields(ctx.probe(t, rel, unique=flag)) for flag in (True, False)}
    return {flag: probe_fields(ctx.probe(t, rel, unnest=flag)) for flag in (True, False)}


def check_probes(ctx, t, d, lo=0, hi=None):
    got = probes(ctx, t, d)
    for flag, g in got.items():
        e = expected_probe(d, flag, lo, hi)
        assert {k: g[k] for k in e} == e, (d.name, flag)
    return got


def canonical(t, kind):
    """An export in a form two tables of equal content share: offsets; chaining entries by (bucket,
    row) and the short buckets as exported; nested main records by (bucket, hash) without their sub
    offsets, and every key's rows ascending."""
    off, pay, sub = t.export()
    ln = np.diff(off.astype(np.int64))
    local = np.repeat(np.arange(len(ln)), ln)
    if kind == TS.CHAIN:
        return [off, pay[np.lexsort((pay[:, 1], local))], pay[ln[local] <= SORTED_MAX]]
    m = pay[np.lexsort((pay[:, 0], local))]
    so, sl = m[:, 2].astype(np.int64), m[:, 3].astype(np.int64)
    key_of = np.repeat(np.arange(len(sl)), sl)
    rows = sub[np.repeat(so - (np.cumsum(sl) - sl), sl) + np.arange(int(sl.sum()))]
    return [off, m[:, [0, 1, 3]], rows[np.lexsort((rows, key_of))]]


def snapshot(ctx, t, d):
    return {"export": canonical(t, d.kind), "stats": t.stats(), "size": t.size(), "path": t.build_path(),
            "probes": probes(ctx, t, d)}


def assert_same(a, b, what):
    assert (a["path"], a["size"], a["stats"], a["probes"]) == (b["path"], b["size"], b["stats"], b["probes"]), what
    for x, y in zip(a["export"], b["export"]):
        assert np.array_equal(x, y), what


def new_table(ctx, d, lo=0, hi=None):
    import hj3d
    return hj3d.Table(ctx, d.kind, d.nb, lo, hi)


def step(ctx, t, d, opts, path, what, ordered=False, started=None):
    """Rebuild t from d under opts; t must then equal the reference, the oracle and a fresh table.
    started: the path the unresolved build reports when another build than `path` was begun."""
    with options(ctx, **opts):
        t.build(d.rel())
        if started:
            assert t.build_path(finish=False) == started, (what, t.build_path(finish=False))
        assert t.build_path() == path, (what, t.build_path())
        check_export(t, d, ordered=ordered)
        check_probes(ctx, t, d)
        got = snapshot(ctx, t, d)
        f = new_table(ctx, d)
        f.build(d.rel())
        want = snapshot(ctx, f, d)
        f.close()
    assert_same(got, want, what)


# ---- structure of one build, per path ----

@pytest.mark.parametrize("sel", list(SELECTIONS) + list(MORE_SELECTIONS))
def test_export_structure_per_build_path(ctx, sel):
    """Full table, implicit rows: the export equals the reference; the statistics recomputed from it
    equal hj3d_table_stats and hj3d_table_size; the probes equal the oracle's."""
    name, opts, path = {**SELECTIONS, **MORE_SELECTIONS}[sel]
    d = data(name)
    with options(ctx, **opts):
        t = new_table(ctx, d)
        t.build(d.rel())
        if sel == "giveup_then_sort":  # the aggregation build was started; its give-up shows at the first use
            assert t.build_path(finish=False) == "nested_agg?"
        assert t.build_path() == path, t.build_path()
        check_export(t, d)
        check_probes(ctx, t, d)
        t.close()


@pytest.mark.parametrize("sel", ["radix", "direct", "nested_agg", "nested_sort", "giveup_then_sort"])
def test_export_structure_explicit_rows(ctx, sel):
    """Explicit ascending row ids with gaps (row word): entries, first rows and sub rows carry them."""
    name, opts, path = SELECTIONS[sel]
    d = data(name, explicit=True)
    with options(ctx, **opts):
        t = new_table(ctx, d)
        t.build(d.rel())
        assert t.build_path() == path, t.build_path()
        check_export(t, d)
        check_probes(ctx, t, d)
        t.close()


def shard_range(d):
    """[lo, hi) with 0 < lo and hi < NB, 5/12 of the buckets, around the fullest bucket (so a chaining
    shard keeps its bucket above 32 entries)."""
    b = (TS.fmix32(d.keys).astype(np.uint64) % np.uint64(d.nb)).astype(np.int64)
    hot, width = int(np.bincount(b, minlength=d.nb).argmax()), d.nb * 5 // 12
    lo = min(max(hot - width // 2, 1), d.nb - 1 - width)
    return lo, lo + width


@pytest.mark.parametrize("explicit", [False, True], ids=["implicit_rows", "explicit_rows"])
@pytest.mark.parametrize("sel", ["radix", "direct", "nested_agg", "nested_agg_slices", "nested_sort",
                                 "giveup_then_sort"])
def test_export_structure_bucket_range_shard(ctx, sel, explicit):
    """A shard of buckets [lo, hi), 0 < lo, hi < NB, fed the whole relation: it stores the tuples of its
    buckets only. n_sub stays the build relation's size; the ranges cover the stored rows and nothing
    refers to the other positions (hj3d.h, hj3d_table_export)."""
    name, opts, path = SELECTIONS[sel]
    d = data(name, explicit=explicit)
    lo, hi = shard_range(d)
    assert 0 < lo < hi < d.nb
    with options(ctx, **opts):
        t = new_table(ctx, d, lo, hi)
        t.build(d.rel())
        assert t.build_path() == path, t.build_path()
        st = check_export(t, d, lo, hi)
        assert 0 < st["entries"] < len(d.keys)
        check_probes(ctx, t, d, lo, hi)
        t.close()


# ---- reuse: one table object through a sequence of contents ----

NPK = dict(radix_min=0, nested_pk=True)
SORT = dict(radix_min=0, nested_sort=True)
SEQUENCES = {
    # chaining
    "radix_then_direct": [("chain_big", RM0, "radix"), ("chain_small", dict(force_direct=True), "direct")],
    "direct_then_radix": [("chain_small", dict(force_direct=True), "direct"), ("chain_big", RM0, "radix")],
    # (one table has one bucket count: the radix step builds the slice relation itself; 2^20 buckets are
    # inside the radix build's range)
    "slices_radix_slices": [SELECTIONS["slices"], ("slices", RM0, "radix"), SELECTIONS["slices"]],
    # nested. A fourth element names the build that was started and then gave up: on 20 000 buckets the
    # slice form made to give up by HJ3D_OPT_DIAG_LOOKBACK (its look-back times out after 1 ms, as
    # test_nested_slices_lookback_timeout_falls_back), on 2 000 buckets the shape whose keys are too dense
    # for the aggregation build's LDS table (2 000 buckets are too few for the slice form).
    "every_nested_path": [SELECTIONS["nested_sort"], ("nested_other", RM0, "nested_agg"),
                          ("nested", dict(NPK, diag_lookback=100_000), "nested_sort", "nested_agg_slices?"),
                          ("nested_other", NPK, "nested_agg_slices"), SELECTIONS["nested_sort"]],
    "giveup_between_builds": [("nested2k", SORT, "nested_sort"), ("nested2k_other", RM0, "nested_agg"),
                              ("nested_giveup", RM0, "nested_sort", "nested_agg?"), ("nested2k", RM0, "nested_agg"),
                              ("nested2k_other", SORT, "nested_sort")],
    # (30 000 tuples over the 20 partitions: the register form takes the small one)
    "large_small_large": [SELECTIONS["nested_agg"], ("nested_small", RM0, "nested_agg_reg"),
                          ("nested_other", RM0, "nested_agg")],
}


@pytest.mark.parametrize("seq", list(SEQUENCES))
def test_table_rebuilt_from_other_relations_by_other_paths(ctx, seq):
    steps = SEQUENCES[seq]
    first = data(steps[0][0])
    assert all((data(s[0]).nb, data(s[0]).kind) == (first.nb, first.kind) for s in steps)
    t = new_table(ctx, first)
    for k, (name, opts, path, *started) in enumerate(steps):
        step(ctx, t, data(name), opts, path, (seq, k, name), started=started[0] if started else None)
    t.close()


def test_chaining_fused_then_two_launch_partition(ctx):
    """The fused one-launch partition, then the two-launch form (HJ3D_OPT_RP_UNFUSED) on the same
    table: both "radix"; the launch counts tell them apart (2 and 3 launches per build, as
    test_fused_partition_chaining_build)."""
    import hj3d
    lib = hj3d.lib()
    d = data("fused")
    t = new_table(ctx, d)
    for unfused, launches in ((False, 2), (True, 3), (False, 2)):
        with options(ctx, rp_unfused=unfused):
            l0 = lib.hj3d_launch_count()
            t.build(d.rel())
            assert lib.hj3d_launch_count() - l0 == launches, unfused
        step(ctx, t, d, dict(rp_unfused=unfused), "radix", ("fused", unfused), ordered=True)
    t.close()


@pytest.mark.parametrize("radix_min", [0, 1 << 20], ids=["radix_min_0", "radix_min_default"])
@pytest.mark.parametrize("kind", [TS.CHAIN, TS.NESTED], ids=["chain", "nested"])
def test_full_empty_full(ctx, kind, radix_min):
    """A relation, the empty relation, the relation again. With HJ3D_OPT_RADIX_MIN = 0 an empty build
    passes the size gates of the partitioned builds, which must all decline it."""
    d, e = data(EMPTY[kind]), empty_data(kind)
    opts = dict(radix_min=radix_min)
    full = "radix" if kind == TS.CHAIN else "nested_agg"
    none = "direct" if kind == TS.CHAIN else "nested_sort"
    t = new_table(ctx, d)
    for k, (x, path) in enumerate(((d, full), (e, none), (d, full))):
        step(ctx, t, x, opts, path, ("full_empty_full", k))
    t.close()


@pytest.mark.parametrize("first", ["nested", "nested_giveup"])
def test_nested_rebuild_over_an_unresolved_build(ctx, first):
    """hj3d_build twice with no use of the table in between: the first build's counts (and, for
    `nested_giveup`, its give-up flag) are still in flight when the second replaces it."""
    a, b = data(first), data("nested_other" if first == "nested" else "nested2k")
    t = new_table(ctx, a)
    with options(ctx, **RM0):
        t.build(a.rel())
        assert t.build_path(finish=False) == "nested_agg?"
    step(ctx, t, b, RM0, "nested_agg", ("unresolved", first))
    t.close()


def test_build_many_over_tables_that_hold_other_content(ctx):
    """hj3d_build_many (one launch sequence for two nested tables of one geometry) into tables that
    hold other builds: one resolved sort build, one unresolved aggregation build of a smaller relation."""
    a, b, old0, old1 = data("nested"), data("nested_other"), data("nested_other"), data("nested_small")
    ts = [new_table(ctx, a), new_table(ctx, b)]
    with options(ctx, radix_min=0, nested_sort=True):
        ts[0].build(old0.rel())
        assert ts[0].build_path() == "nested_sort"
    with options(ctx, **RM0):
        ts[1].build(old1.rel())
        assert ts[1].build_path(finish=False) == "nested_agg_reg?"
        ctx.build_many(ts, [a.rel(), b.rel()])
        fresh = [new_table(ctx, a), new_table(ctx, b)]
        ctx.build_many(fresh, [a.rel(), b.rel()])
        for t, f, d in zip(ts, fresh, (a, b)):
            assert t.build_path() == "nested_agg", t.build_path()
            check_export(t, d)
            check_probes(ctx, t, d)
            assert_same(snapshot(ctx, t, d), snapshot(ctx, f, d), d.name)
            t.close()
            f.close()


# ---- clear ----

@functools.lru_cache(maxsize=None)
def empty_stats(kind, nb):
    """The oracle's HtStatistics of a table of nb buckets built from the empty relation."""
    plan = O.chain_plan if kind == TS.CHAIN else O.nested_plan
    return plan(np.zeros((0, 3), np.uint32), 1, np.zeros((1, 3), np.uint32), 0, nb, False).stats


ZERO = {"n_matched": 0, "n_out": 0, "n_cmps": 0, "sum_a": 0, "sum_b": 0, "sum_h": 0, "xor_h": 0}


def check_empty_table(ctx, t, d):
    """A cleared (or never built) table: every getter succeeds and shows an empty table; probes,
    small and direct and offered to the partitioned and packed kernels, match nothing."""
    import hj3d
    import torch
    assert t.build_path(finish=False) == "none"
    t.finish()
    assert t.build_path() == "none"
    off, pay, sub = t.export()
    assert len(pay) == 0 and len(sub) == 0 and len(off) == d.nb + 1 and not off.any()
    want = empty_stats(d.kind, d.nb)
    assert want["nb"] == d.nb and want["entries"] == 0
    got = t.stats()
    assert {k: got[k] for k in TS.STAT_KEYS} == {k: want[k] for k in TS.STAT_KEYS}
    assert t.size() == (0, 0)
    small = d.probe_device[:1000].contiguous()
    for opts, pdev in ((dict(force_direct=True), small), ({}, small), (RM0, d.probe_device)):
        with options(ctx, **opts):
            rel = hj3d.Rel(pdev, 0)
            for flag in (True, False):
                kw = dict(unique=flag) if d.kind == TS.CHAIN else dict(unnest=flag)
                r = probe_fields(ctx.probe(t, rel, **kw))
                assert r == dict(ZERO, n_probe=len(pdev)), (opts, flag, r)
            if d.kind == TS.CHAIN:  # dense output of the unique probe: every slot unmatched
                out = torch.zeros((len(pdev), 2), dtype=torch.int32, device="cuda")
                r = ctx.probe(t, rel, unique=True, out=out)
                assert probe_fields(r) == dict(ZERO, n_probe=len(pdev)) and not r.overflow, opts
                host = out.cpu().numpy().view(np.uint32)
                assert (host[:, 1] == 0xFFFFFFFF).all(), opts
                assert np.array_equal(np.sort(host[:, 0]), np.arange(len(pdev), dtype=np.uint32)), opts


@pytest.mark.parametrize("sel", list(SELECTIONS))
def test_clear_after_every_build_path(ctx, sel):
    name, opts, path = SELECTIONS[sel]
    d = data(name)
    with options(ctx, **opts):
        t = new_table(ctx, d)
        t.build(d.rel())
        assert t.build_path() == path, t.build_path()
        t.clear()
    check_empty_table(ctx, t, d)
    step(ctx, t, d, opts, path, ("rebuild after clear", sel))  # equals a fresh table
    t.clear()
    t.clear()  # (twice in a row)
    check_empty_table(ctx, t, d)
    t.close()


def test_clear_drops_an_unresolved_build(ctx):
    """hj3d_table_clear straight after hj3d_build of a nested table whose aggregation build gives up:
    the pending sort build must not run at the next use and refill the cleared table."""
    d = data("nested_giveup")
    with options(ctx, **RM0):
        t = new_table(ctx, d)
        t.build(d.rel())
        assert t.build_path(finish=False) == "nested_agg?"
        t.clear()
    check_empty_table(ctx, t, d)
    t.close()


@pytest.mark.parametrize("kind", [TS.CHAIN, TS.NESTED], ids=["chain", "nested"])
def test_never_built_table_reads_as_empty(kind):
    """On a context of its own, so no earlier build has sized any scratch the probes might lean on."""
    import hj3d
    d = data(EMPTY[kind])
    c = hj3d.Context()
    try:
        t = new_table(c, d)
        check_empty_table(c, t, d)
        t.close()
    finally:
        c.close()


@pytest.mark.parametrize("cleared", ["s", "t"])
@pytest.mark.parametrize("kind", [TS.CHAIN, TS.NESTED], ids=["chj", "ndu"])
@pytest.mark.parametrize("radix_min", [0, 1 << 20], ids=["radix_min_0", "radix_min_default"])
def test_probe2_over_a_cleared_and_a_built_table(ctx, kind, cleared, radix_min):
    """Experiment 4's strand with one side emptied: no triple (c_top = 0), and the counters of the
    built side as the oracle gives them for an empty relation on the other."""
    import hj3d
    d, other = data(EMPTY[kind]), data("chain_big" if kind == TS.CHAIN else "nested_other")
    S = d.tuples if cleared == "t" else d.tuples[:0]
    T = d.tuples[:0] if cleared == "t" else d.tuples
    e = O.exp4_plan(d.probe_tuples, S, T, d.nb, kind == TS.NESTED, keys=(0, 1, 1))
    with options(ctx, radix_min=radix_min):
        ts, tt = new_table(ctx, d), new_table(ctx, d)
        (ts if cleared == "t" else tt).build(d.rel())
        victim = tt if cleared == "t" else ts
        victim.build(other.rel())
        victim.clear()
        got = ctx.probe2(ts, tt, hj3d.Rel(d.probe_device, 0))
        ts.close()
        tt.close()
    assert got["c_top"] == 0 and not got["overflow"]
    fields = ("c_probe_rs", "c_probe_rs_cmp", "c_probe_rt", "c_probe_rt_cmp", "c_unnest_1", "c_unnest_2", "c_top")
    assert {k: got[k] for k in fields} == {k: e[k] for k in fields}
    assert {k: got[k] for k in ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")} == {k: 0 for k in
                                                                                 ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")}


# ---- reserve ----

@pytest.mark.parametrize("kind", [TS.CHAIN, TS.NESTED], ids=["chain", "nested"])
def test_reserve_then_smaller_equal_and_larger_builds(ctx, kind):
    """hj3d_table_reserve(n), then builds of n / 2, n and 2 n tuples: each equals a fresh table."""
    n = 200_000
    name = EMPTY[kind]
    t = new_table(ctx, data(name))
    t.reserve(n)
    # (nested: up to ~13 900 pairs per partition, 20 partitions here, the register form aggregates)
    paths = ("radix",) * 3 if kind == TS.CHAIN else ("nested_agg_reg", "nested_agg_reg", "nested_agg")
    for m, path in zip((n // 2, n, 2 * n), paths):
        step(ctx, t, data(name, n=m), RM0, path, ("reserve", m))
    t.close()
