"""GPU parity of every fused-selection form of the probe-side partitioners (hj3d_probe_sel with one
predicate): k_pk_part<*, SEL, 1> (window form), k_pk_part<*, SEL, 2> (stage form), either in front of
k_pk_split (chain_pk.hip), and k_rp_part1r<..., SEL> (radix.hip) under the non-unique chaining probe
and the nested probe, each with implicit and with explicit rows.

Expectations come from the oracle (O.select, then O.chain_plan / O.nested_plan on the passing tuples)
and from plain numpy on the build keys; nothing is expected from the library. Every case runs fused
and select-first (sel_unfused), and both must meet the same expectation: counters, the output
checksums, the materialised pairs one by one, and a canary behind everything the probe may write.

Proof of path: the packed geometry is asserted with pk_plan before the probe, and the fused call must
take at least SELECT_LAUNCHES fewer kernel launches than the select-first call (hj3d_launch_count
after a warm-up call of the same shape): a silent fall-back to select-first would not.

Shapes: both partitioners take 8192-tuple tiles on min(tiles, CUs) workgroups. N_SMALL = 2 tiles + 17;
big_n() = 2 * CUs tiles + 17, where every workgroup takes two full tiles (one a ragged third): only
there does a predicate word that comes from the wrong tile of the same workgroup show (the word is
loaded one tile ahead, next to the key), and only with a pass pattern that differs between a
workgroup's tiles ("rounds"; "odd" tells neighbouring tiles apart).
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

TILE = 8192
N_SMALL = 2 * TILE + 17
TAIL = 193            # canary rows behind `out`
NONE = 0xFFFFFFFF     # partner of a probe tuple without one; a canary row is (NONE, NONE)
SELECT_LAUNCHES = 3   # select_pairs (select.hip): k_sel_count, the tile scan (k_scan_lb), k_sel_write
NB = 1 << 16          # the chaining table
NB_NESTED = 1 << 12
I32MIN, I32MAX, U32MAX, I64MIN, I64MAX = -2**31, 2**31 - 1, 2**32 - 1, -2**63, 2**63 - 1
BOUNDARY_WORDS = np.array([0, 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
BOUNDARY_CONSTS = [I64MIN, I64MIN + 1, -2**32, I32MIN - 1, I32MIN, I32MIN + 1, -1, 0, 1, I32MAX - 1, I32MAX, I32MAX + 1,
                   U32MAX - 1, U32MAX, U32MAX + 1, I64MAX - 1, I64MAX]
RANGE_CONSTS = [I64MIN, I32MIN - 1, I32MIN, -1, 0, I32MAX, U32MAX, U32MAX + 1, I64MAX]
PRED = [(2, "<", 37)]  # on the mark word of {row, key, mark} probe tuples


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def fmix32(x):
    h = np.asarray(x, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85ebca6b)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xc2b2ae35)
    h ^= h >> np.uint32(16)
    return h


def host_checksums(pairs):
    a = pairs[:, 0].astype(np.uint64)
    b = pairs[:, 1].astype(np.uint64)
    z = (a << np.uint64(32)) | b
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        z = z ^ (z >> np.uint64(31))
        return {"n": len(pairs), "sum_a": int(a.sum(dtype=np.uint64)), "sum_b": int(b.sum(dtype=np.uint64)),
                "sum_h": int(z.sum(dtype=np.uint64)), "xor_h": int(np.bitwise_xor.reduce(z)) if len(z) else 0}


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def big_n():
    return 2 * cus() * TILE + 17


class Tab:
    """A built table, its build tuples (key word 0, implicit rows unless `rows` is given) and the numpy
    lookup of the build rows of a key, ascending."""

    def __init__(self, ctx, kind, nb, keys, lo=0, hi=None, rows=None):
        import hj3d
        self.nb, self.keys, self.nested = nb, keys, kind == hj3d.HJ3D_NESTED
        self.t = hj3d.Table(ctx, kind, nb, lo, hi)
        if rows is None:
            self.B, self.brow = O.tuples3(keys, np.zeros(len(keys), np.uint32)), None
            rows = np.arange(len(keys), dtype=np.uint32)
        else:
            self.B, self.brow = np.stack([keys, rows], axis=1).astype(np.uint32), 1
        self.brel = hj3d.Rel(dev(self.B), 0, row_word=self.brow)  # kept: a nested build reads it at first use
        self.t.build(self.brel)
        order = np.lexsort((rows, keys))
        self.sk, self.srow = keys[order], rows[order]

    def groups(self, keys):
        """(first index into srow, group size) of each key."""
        l = np.searchsorted(self.sk, keys, "left")
        return l, np.searchsorted(self.sk, keys, "right") - l

    def pairs(self, prow, pkeys):
        """Every (probe row, build row) with equal keys."""
        l, c = self.groups(pkeys)
        rep = np.repeat(np.arange(len(pkeys)), c)
        k = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        return np.stack([prow[rep], self.srow[l[rep] + k]], axis=1).astype(np.uint32)

    def first(self, pkeys):
        """The first build row of each key's group, NONE without one."""
        l, c = self.groups(pkeys)
        return np.where(c > 0, self.srow[np.minimum(l, len(self.srow) - 1)], np.uint32(NONE)).astype(np.uint32)


class World:
    def __init__(self, ctx):
        import hj3d
        self.ctx, self.hj3d, self.cache = ctx, hj3d, {}
        rng = np.random.default_rng(NB)
        self.chain = Tab(ctx, hj3d.HJ3D_CHAIN, NB, rng.choice(1 << 26, size=NB, replace=False).astype(np.uint32))
        # nested: ~3 build rows per key, a quarter of the probe keys without a partner
        kset = rng.choice(1 << 26, size=NB_NESTED, replace=False).astype(np.uint32)
        self.nested = Tab(ctx, hj3d.HJ3D_NESTED, NB_NESTED, kset[rng.integers(0, NB_NESTED, 3 * NB_NESTED)])
        self.tabs = [self.chain, self.nested]

    def table(self, form):
        return self.nested if FORMS[form]["mode"] in ("unnest", "nested") else self.chain

    def probe_keys(self, tab, n, seed):
        rng = np.random.default_rng(seed)
        k = tab.keys[rng.integers(0, len(tab.keys), n)]
        if tab.nested:
            miss = rng.random(n) < 0.25
            k[miss] = rng.integers(1 << 26, 1 << 32, int(miss.sum()), dtype=np.uint64).astype(np.uint32)
        return k

    def rel(self, tab, n, explicit, pattern, seed=1):
        """{row, key, mark} probe tuples (cached with their device copy): row = the index, or explicit ids,
        ascending with gaps, about half of them with bit 31 set; mark by the pass pattern under PRED."""
        key = (id(tab), n, explicit, pattern, seed)
        if key not in self.cache:
            rng = np.random.default_rng([seed, n, int(explicit)])
            Pt = O.tuples3(np.arange(n, dtype=np.uint32), self.probe_keys(tab, n, seed))
            if explicit:
                step = (2**32 - 2) // n
                rows = np.cumsum(rng.integers(1, step + 1, n, dtype=np.uint64))
                rows += (np.uint64(2**32 - 2) - rows[-1]) // np.uint64(2)
                assert int(rows[-1]) < NONE and int(rows[0]) < 2**31 <= int(rows[-1])
                Pt[:, 0] = rows.astype(np.uint32)
            i = np.arange(n)
            lo_mark, hi_mark = rng.integers(0, 37, n).astype(np.uint32), rng.integers(37, 100, n).astype(np.uint32)
            if pattern == "random":    # (a) ~37 % pass
                Pt[:, 2] = rng.integers(0, 100, n).astype(np.uint32)
            elif pattern == "odd":     # (b) exactly the odd-numbered 8192-tuple blocks pass
                Pt[:, 2] = np.where((i // TILE) & 1, lo_mark, hi_mark)
            elif pattern == "rounds":  # a workgroup's tiles t, t + G, t + 2 G alternate: fail, pass, fail
                g = min(-(-n // TILE), cus())
                Pt[:, 2] = np.where((i // TILE // g) & 1, lo_mark, hi_mark)
            elif pattern == "all":     # (c)
                Pt[:, 2] = lo_mark
            elif pattern == "none":    # (d)
                Pt[:, 2] = hi_mark
            elif pattern == "ragged":  # (e) only the final ragged tile passes
                assert n % TILE
                Pt[:, 2] = np.where(i >= n - n % TILE, lo_mark, hi_mark)
            else:                      # (f) a hot key on every second tuple, half of each half pass
                assert pattern == "hot"
                Pt[::2, 1] = tab.keys[12345 % len(tab.keys)]
                Pt[:, 2] = rng.integers(0, 74, n).astype(np.uint32)
            self.cache[key] = (Pt, dev(Pt))
        return self.cache[key]


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.cache.clear()
    for tab in w.tabs:
        tab.t.close()


@pytest.fixture
def opts(ctx):
    """Partitioned probes at every size; options restored afterwards."""
    ctx.radix_min(0)
    yield ctx
    ctx.sel_unfused(False)
    ctx.pk_slice_max(0)
    ctx.pk_stage(0)
    ctx.radix_min(1 << 20)


# form -> probe mode, the slice bound that reaches it at NB buckets, and the pk_plan geometry that says so
FORMS = {
    "pk_window": dict(mode="unique", w=64, geom=lambda pl: (pl["P"], pl["P1"], pl["C"]) == (1024, 1024, 1)),
    "pk_stage": dict(mode="unique", w=40, geom=lambda pl: 1024 < pl["P1"] <= 2048 and pl["C"] == 1),
    "pk_split": dict(mode="unique", w=16, geom=lambda pl: pl["C"] > 1 and pl["P1"] <= 1024),
    "rp_chain": dict(mode="chain"),
    "rp_unnest": dict(mode="unnest"),
    "rp_nested": dict(mode="nested"),
}
ROWS = ["implicit", "explicit"]


def setup_form(ctx, form, tab):
    f = FORMS[form]
    if "w" in f:
        ctx.pk_slice_max(f["w"])
        pl = ctx.pk_plan(tab.nb, len(tab.keys))
        assert f["geom"](pl), (form, pl)
        print(f"{form}: pk_plan {pl}")
    return f["mode"]


def expectation(tab, Pt, preds, mode, key, row_word):
    """The oracle's plan on the passing tuples as (key, row) pairs, and those pairs."""
    idx = O.select(Pt, key, preds)[:, 1]
    rows = Pt[:, row_word] if row_word is not None else np.arange(len(Pt), dtype=np.uint32)
    sel = np.stack([Pt[idx, key], rows[idx]], axis=1).astype(np.uint32)
    if mode in ("unique", "chain"):
        e = O.chain_plan(tab.B, 0, sel, 0, tab.nb, mode == "unique", brow=tab.brow, prow=1)
    else:
        e = O.nested_plan(tab.B, 0, sel, 0, tab.nb, mode == "unnest", brow=tab.brow, prow=1)
    return e, sel


def probe(ctx, tab, rel, preds, mode, out):
    kw = dict(unique=mode == "unique", unnest=mode == "unnest", out=out)
    return ctx.probe_sel(tab.t, rel, preds, **kw) if preds is not None else ctx.probe(tab.t, rel, **kw)


def packed(pairs):
    return np.sort((pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64))


def verify(r, buf, e, sel, tab, mode, what, owned=None):
    """One probe's result and output buffer against the oracle's plan e and the passing (key, row)
    pairs sel. owned (bucket-range shards): the passing tuples the table holds the bucket of; the
    comparison count is then the caller's to check."""
    assert not r.overflow, what
    assert r.n_probe == len(sel), what
    if owned is None:
        assert r.n_cmps == e.c_cmp, what
        own = sel
    else:
        own = sel[owned]
    exp_pairs = tab.pairs(own[:, 1], own[:, 0])
    got = {"n": r.n_out, "sum_a": r.sum_a, "sum_b": r.sum_b, "sum_c": r.sum_c, "sum_h": r.sum_h, "xor_h": r.xor_h}
    host = buf.cpu().numpy().view(np.uint32)
    if mode in ("unique", "nested"):  # dense: one slot per passing tuple, {row, first build row or NONE}
        first = tab.first(own[:, 0])
        matched = own[first != NONE]
        exp_out = np.stack([matched[:, 1], first[first != NONE]], axis=1)
        if owned is None:
            assert got == e.out and r.n_out == e.c_top, what
            if mode == "nested":
                assert r.n_matched == e.c_probe, what
            written = host[:r.n_probe]
            assert (host[r.n_probe:] == NONE).all(), what  # the unused slots and the canary tail
            order, by_row = np.argsort(written[:, 0], kind="stable"), np.argsort(own[:, 1], kind="stable")
            assert np.array_equal(written[order, 0], own[by_row, 1]), what  # every passing row exactly once
            assert np.array_equal(written[order, 1], first[by_row]), what
        else:  # unowned tuples are dropped: the slots that carry a partner
            written = host[: len(host) - TAIL]
            assert (host[len(host) - TAIL:] == NONE).all(), what
        with_partner = written[written[:, 1] != NONE]
        assert np.array_equal(packed(with_partner), packed(exp_out)), what
        assert {k: got[k] for k in ("n", "sum_a", "sum_b", "sum_h", "xor_h")} == host_checksums(with_partner), what
        return with_partner
    # chain (non-unique) / unnest: the multiset of pairs in the first n_out slots
    if owned is None:
        assert got == e.out and r.n_out == e.c_top, what
        if mode == "unnest":
            assert r.n_matched == e.c_probe, what
    assert r.n_out == len(exp_pairs), what
    assert (host[r.n_out:] == NONE).all(), what
    assert np.array_equal(packed(host[:r.n_out]), packed(exp_pairs)), what
    assert {k: got[k] for k in ("n", "sum_a", "sum_b", "sum_h", "xor_h")} == host_checksums(host[:r.n_out]), what
    return host[:r.n_out]


def launches_of(fn):
    import hj3d
    L = hj3d.lib()
    c0 = L.hj3d_launch_count()
    r = fn()
    return r, L.hj3d_launch_count() - c0


def run(ctx, tab, Pt, rel, preds, mode, key=1, row_word=None, prove=True, what=""):
    """Pt through probe_sel, fused and select-first, each against the oracle; with prove, the fused call
    takes at least SELECT_LAUNCHES fewer launches. Returns the fused result."""
    import torch
    e, sel = expectation(tab, Pt, preds, mode, key, row_word)
    cap = len(Pt) if mode in ("unique", "nested") else max(e.c_top, 1)
    delta, res = {}, {}
    for unfused in (False, True):
        ctx.sel_unfused(unfused)
        buf = torch.full((cap + TAIL, 2), -1, dtype=torch.int32, device="cuda")
        if prove:
            probe(ctx, tab, rel, preds, mode, buf[:cap])  # warm-up: scratch sized, nothing allocated below
            buf.fill_(-1)
        res[unfused], delta[unfused] = launches_of(lambda: probe(ctx, tab, rel, preds, mode, buf[:cap]))
        verify(res[unfused], buf, e, sel, tab, mode, (what, "unfused" if unfused else "fused"))
    ctx.sel_unfused(False)
    print(f"{what}: n {len(Pt)} passing {len(sel)} launches fused {delta[False]} unfused {delta[True]}")
    if prove:
        assert delta[True] - delta[False] >= SELECT_LAUNCHES, (what, delta)
    return res[False]


def row_word_of(rows):
    return 0 if rows == "explicit" else None


def rel_of(world, Pt, dPt, rows):
    return world.hj3d.Rel(dPt, 1, row_word=row_word_of(rows))


# ---- the form matrix ----
@pytest.mark.parametrize("pattern", ["odd", "rounds"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("form", list(FORMS))
def test_two_full_tiles_per_workgroup(opts, world, form, rows, pattern):
    """n = 2 * CUs * 8192 + 17: workgroup g takes tiles g and g + CUs (workgroup 0 a ragged third).
    odd, pattern (b): the predicate word passes exactly in the odd-numbered 8192-tuple blocks; a word
    taken from the neighbouring tile shows. With an even workgroup count the tiles of one workgroup
    have the same parity, so a word taken from the workgroup's own next or previous tile does not show:
    rounds: the word passes exactly in tiles [CUs, 2 CUs), every workgroup's second tile. (Tried on a
    build whose window form never hands the next tile's predicate words over, so every tile is tested
    with the words of the workgroup's first: `rounds` fails there, `odd` and the small shapes pass.)"""
    tab = world.table(form)
    mode = setup_form(opts, form, tab)
    Pt, dPt = world.rel(tab, big_n(), rows == "explicit", pattern)
    run(opts, tab, Pt, rel_of(world, Pt, dPt, rows), PRED, mode, row_word=row_word_of(rows),
        what=f"{form}/{rows}/{pattern}/big")


@pytest.mark.parametrize("pattern", ["random", "odd", "ragged"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("form", list(FORMS))
def test_pass_patterns(opts, world, form, rows, pattern):
    """Patterns (a), (b), (e) at two tiles + 17."""
    tab = world.table(form)
    mode = setup_form(opts, form, tab)
    Pt, dPt = world.rel(tab, N_SMALL, rows == "explicit", pattern)
    run(opts, tab, Pt, rel_of(world, Pt, dPt, rows), PRED, mode, row_word=row_word_of(rows),
        what=f"{form}/{rows}/{pattern}")


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("form", list(FORMS))
def test_everything_passes_equals_probe(opts, world, form, rows):
    """Pattern (c): every field of the result equals that of ctx.probe on the same relation."""
    tab = world.table(form)
    mode = setup_form(opts, form, tab)
    Pt, dPt = world.rel(tab, N_SMALL, rows == "explicit", "all")
    rel = rel_of(world, Pt, dPt, rows)
    r = run(opts, tab, Pt, rel, PRED, mode, row_word=row_word_of(rows), what=f"{form}/{rows}/all")
    assert r.n_probe == len(Pt)
    assert r == probe(opts, tab, rel, None, mode, None)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("form", list(FORMS))
def test_nothing_passes_after_a_passing_probe(opts, world, form, rows):
    """Pattern (d), directly after a passing probe on the same context: the n_probe atomic is skipped
    when a wave counted nothing, and nothing of the probe before may show: every counter and checksum
    zero, not one slot written."""
    import torch
    tab = world.table(form)
    mode = setup_form(opts, form, tab)
    Pa, dPa = world.rel(tab, N_SMALL, rows == "explicit", "random")
    Pn, dPn = world.rel(tab, N_SMALL, rows == "explicit", "none")
    assert len(O.select(Pn, 1, PRED)) == 0
    for unfused in (False, True):
        opts.sel_unfused(unfused)
        buf = torch.full((N_SMALL + TAIL, 2), -1, dtype=torch.int32, device="cuda")
        before = probe(opts, tab, rel_of(world, Pa, dPa, rows), PRED, mode, buf[:N_SMALL])
        assert before.n_probe > 0 and before.n_out > 0
        buf.fill_(-1)
        r = probe(opts, tab, rel_of(world, Pn, dPn, rows), PRED, mode, buf[:N_SMALL])
        assert not r.overflow
        assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps) == (0, 0, 0, 0), unfused
        assert (r.sum_a, r.sum_b, r.sum_c, r.sum_h, r.xor_h) == (0, 0, 0, 0, 0), unfused
        assert bool((buf == -1).all()), unfused


@pytest.mark.parametrize("unnest", [True, False])
def test_empty_probe_side_of_a_nested_table(opts, world, unnest):
    """What select-first hands to hj3d_probe when nothing passed: a relation of zero tuples. With
    HJ3D_OPT_RADIX_MIN = 0 it once reached the partitioned nested probe, whose geometry divides by the
    workgroup count min(tiles, CUs) = 0 on the host."""
    _, dPt = world.rel(world.nested, N_SMALL, False, "random")
    r = opts.probe(world.nested.t, world.hj3d.Rel(dPt, 1, n=0), unnest=unnest)
    assert (r.n_probe, r.n_matched, r.n_out, r.n_cmps, r.sum_a, r.sum_b, r.sum_h, r.xor_h) == (0,) * 8


@pytest.mark.parametrize("form,stage", [("pk_window", 0), ("pk_stage", 1), ("rp_chain", 0)])
def test_hot_key_overflow_list(opts, world, form, stage):
    """Pattern (f): one key on every second tuple, half of them passing. A full tile then holds ~2048
    passing pairs of the hot slice against regions of 64 pairs (packed: 8 expected per slice and
    workgroup + 8 sigma + 32) or ~1500 (k_rp_part1r at 7 slices: 1170 expected + 8 sigma + 32, with
    the slice's ~290 other passing pairs on top), so the regions overflow and the overflow list is probed.
    pk_stage: the stage form with the carry flush after every tile (HJ3D_OPT_PK_STAGE = 1)."""
    tab = world.table(form)
    mode = setup_form(opts, form, tab)
    opts.pk_stage(stage)
    Pt, dPt = world.rel(tab, N_SMALL, False, "hot")
    run(opts, tab, Pt, rel_of(world, Pt, dPt, "implicit"), PRED, mode, what=f"{form}/hot/stage{stage}")


# ---- predicate semantics on the device ----
def sweep_cases(ops_consts):
    for signed in (True, False):
        for op, lo, hi in ops_consts:
            yield op, lo, hi, signed


def semantics(ctx, world, form, cases):
    """Every predicate of `cases` on a word that cycles through the boundary words, mixed with random
    ones, fused and select-first; expected with exact integer compares (no arithmetic on the constants):
    n_probe == n_out == the passing tuples (every probe key is a build key), sum_a == the sum of their rows."""
    tab = world.chain
    mode = setup_form(ctx, form, tab)
    Pt, _ = world.rel(tab, N_SMALL, False, "random", seed=2)
    Pt = Pt.copy()
    rng = np.random.default_rng(9)
    Pt[:, 2] = np.where(np.arange(N_SMALL) % 3 != 2, BOUNDARY_WORDS[np.arange(N_SMALL) % 8],
                        rng.integers(0, 2**32, N_SMALL, dtype=np.uint64).astype(np.uint32))
    rel = world.hj3d.Rel(dev(Pt), 1)
    v_s, v_u = Pt[:, 2].view(np.int32).astype(np.int64), Pt[:, 2].astype(np.int64)
    rows = np.arange(N_SMALL, dtype=np.int64)
    cmpf = {"<": lambda v, lo, hi: v < lo, "<=": lambda v, lo, hi: v <= lo, ">": lambda v, lo, hi: v > lo,
            ">=": lambda v, lo, hi: v >= lo, "==": lambda v, lo, hi: v == lo, "!=": lambda v, lo, hi: v != lo,
            "range": lambda v, lo, hi: (v >= lo) & (v < hi)}
    for op, lo, hi, signed in cases:
        ok = cmpf[op](v_s if signed else v_u, np.int64(lo), np.int64(hi))
        want = (int(ok.sum()), int(rows[ok].sum()))
        for unfused in (False, True):
            ctx.sel_unfused(unfused)
            r = ctx.probe_sel(tab.t, rel, [(2, op, lo, hi, signed)], unique=mode == "unique")
            assert (r.n_probe, r.n_out, r.sum_a) == (want[0], want[0], want[1]), (op, lo, hi, signed, unfused)
    ctx.sel_unfused(False)


@pytest.mark.parametrize("op", ["<", "<=", ">", ">=", "==", "!="])
def test_predicate_semantics_compare_ops(opts, world, op):
    """Packed window form: op x signedness x the 17 boundary constants."""
    semantics(opts, world, "pk_window", sweep_cases([(op, c, 0) for c in BOUNDARY_CONSTS]))


def test_predicate_semantics_range(opts, world):
    """Packed window form: RANGE over every (lo, hi) pair of nine constants with both int64 extremes."""
    semantics(opts, world, "pk_window", sweep_cases([("range", lo, hi) for lo in RANGE_CONSTS for hi in RANGE_CONSTS]))


def test_predicate_semantics_int64_extremes_rp(opts, world):
    """k_rp_part1r (non-unique chaining probe): the three predicates whose range form once overflowed
    int64 (< INT64_MIN, > INT64_MAX, RANGE with hi = INT64_MIN)."""
    semantics(opts, world, "rp_chain", sweep_cases([("<", I64MIN, 0), (">", I64MAX, 0)] +
                                                    [("range", lo, I64MIN) for lo in RANGE_CONSTS]))


# ---- layouts ----
@pytest.mark.parametrize("variant", ["five_words", "one_word", "unaligned_base"])
@pytest.mark.parametrize("form", ["pk_window", "rp_chain"])
def test_layouts(opts, world, form, variant):
    """The predicate word as the last word of a 5-word tuple, as the key word itself of a 1-word tuple
    (stride 4), and behind a base pointer 12 bytes off 16-byte alignment."""
    import torch
    tab = world.chain
    mode = setup_form(opts, form, tab)
    keys = world.probe_keys(tab, N_SMALL, 3)
    rng = np.random.default_rng(4)
    mark = rng.integers(0, 100, N_SMALL).astype(np.uint32)
    if variant == "five_words":
        Pt = rng.integers(0, 2**32, (N_SMALL, 5), dtype=np.uint64).astype(np.uint32)
        Pt[:, 1], Pt[:, 4] = keys, mark
        d, key, preds = dev(Pt), 1, [(4, "<", 37)]
    elif variant == "one_word":
        Pt = keys.reshape(N_SMALL, 1).copy()
        d, key, preds = dev(Pt), 0, [(0, "<", 1 << 25, None, False)]  # keys are below 2^26
    else:
        Pt = O.tuples3(np.arange(N_SMALL, dtype=np.uint32), keys)
        Pt[:, 2] = mark
        T = torch.zeros((N_SMALL + 1, 3), dtype=torch.int32, device="cuda")
        T[1:] = dev(Pt)
        d, key, preds = T[1:], 1, PRED
    rel = world.hj3d.Rel(d, key)
    if variant == "unaligned_base":
        assert rel.c.base % 16 == 12
    run(opts, tab, Pt, rel, preds, mode, key=key, what=f"{form}/{variant}")


# ---- bucket-range shards ----
@pytest.mark.parametrize("form", ["pk_window", "rp_chain"])
def test_bucket_range_shards(opts, world, form):
    """Three tables over hj3d.part_range(NB, 3, p) (bucket_lo != 0 for two of them), each probed with
    all tuples, explicit rows and a fused selection: n_probe counts every passing tuple, owned or not
    (what both partitioners count and the select-first path reports), n_out the owned ones; the three
    shards' pairs together are the single table's, and their comparison counts add up to chain_plan's."""
    import torch
    hj3d = world.hj3d
    full = world.chain
    mode = FORMS[form]["mode"]
    Pt, dPt = world.rel(full, N_SMALL, True, "random")
    rel = hj3d.Rel(dPt, 1, row_word=0)
    e, sel = expectation(full, Pt, PRED, mode, 1, 0)
    bucket = fmix32(sel[:, 0]) % np.uint32(NB)
    bbucket = fmix32(full.keys) % np.uint32(NB)
    all_pairs = {False: [], True: []}
    cmps = {False: 0, True: 0}
    for p in range(3):
        lo, hi = hj3d.part_range(NB, 3, p)
        assert p == 0 or lo != 0
        mine = (bbucket >= lo) & (bbucket < hi)
        tab = Tab(opts, hj3d.HJ3D_CHAIN, NB, full.keys[mine], lo, hi, rows=np.nonzero(mine)[0].astype(np.uint32))
        try:
            if form == "pk_window":
                opts.pk_slice_max(64)
                pl = opts.pk_plan(hi - lo, int(mine.sum()))
                assert pl["P1"] <= 1024 and pl["C"] == 1, pl
            owned = (bucket >= lo) & (bucket < hi)
            cap = N_SMALL
            delta = {}
            for unfused in (False, True):
                opts.sel_unfused(unfused)
                buf = torch.full((cap + TAIL, 2), -1, dtype=torch.int32, device="cuda")
                probe(opts, tab, rel, PRED, mode, buf[:cap])
                buf.fill_(-1)
                r, delta[unfused] = launches_of(lambda: probe(opts, tab, rel, PRED, mode, buf[:cap]))
                got = verify(r, buf, e, sel, tab, mode, (form, p, unfused), owned=owned)
                assert r.n_out == int(owned.sum())  # every probe key is a build key
                all_pairs[unfused].append(got)
                cmps[unfused] += r.n_cmps
            print(f"{form}/shard{p}: launches fused {delta[False]} unfused {delta[True]}")
            assert delta[True] - delta[False] >= SELECT_LAUNCHES, (form, p, delta)
        finally:
            opts.sel_unfused(False)
            tab.t.close()
    exp = full.pairs(sel[:, 1], sel[:, 0])
    for unfused in (False, True):
        assert np.array_equal(packed(np.concatenate(all_pairs[unfused])), packed(exp)), unfused
        assert cmps[unfused] == e.c_cmp, unfused


# ---- combinations that select first by design: results only ----
def test_two_predicates_select_first(opts, world):
    """Fall-back by design: two predicates are never fused (SelRange::from takes one); hj3d_select runs
    first on both settings. Packed window geometry and the k_rp_part1r chaining probe."""
    for form in ("pk_window", "rp_chain"):
        tab = world.table(form)
        mode = setup_form(opts, form, tab)
        Pt, dPt = world.rel(tab, N_SMALL, False, "random")
        run(opts, tab, Pt, rel_of(world, Pt, dPt, "implicit"), [(2, ">=", 10), (2, "<", 60)], mode, prove=False,
            what=f"{form}/two_preds")


@pytest.mark.parametrize("w,levels", [(128, 1), (64, 2)])
@pytest.mark.parametrize("unnest", [True, False])
def test_nested_beyond_1024_slices_select_first(opts, world, unnest, w, levels):
    """Fall-backs by design on a nested table of 2^18 buckets: with slices of 128 buckets the one-level
    partitioner has 2048 slices (k_rp_part1, which has no fused form: more than 1024 slices), with 64 the
    probe takes the packed partitioner's two levels, which the fused call does not enter; both select
    first."""
    hj3d = world.hj3d
    if "wide" not in world.cache:
        rng = np.random.default_rng(18)
        kset = rng.choice(1 << 26, size=1 << 17, replace=False).astype(np.uint32)
        world.cache["wide"] = Tab(opts, hj3d.HJ3D_NESTED, 1 << 18, kset[rng.integers(0, 1 << 17, 1 << 18)])
        world.tabs.append(world.cache["wide"])
    tab = world.cache["wide"]
    opts.pk_slice_max(w)
    Pt, dPt = world.rel(tab, N_SMALL, False, "random")
    run(opts, tab, Pt, rel_of(world, Pt, dPt, "implicit"), PRED, "unnest" if unnest else "nested", prove=False,
        what=f"nested_wide/w{w}/unnest{int(unnest)}")
