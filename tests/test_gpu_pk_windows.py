"""GPU parity of the packed partitioner's window form (chain_pk.hip, k_pk_part with one slice per
thread: per-slice segment windows in LDS, whole segments flushed round by round).

Every case probes a chaining table with unique build keys through the packed unique probe
(radix_min(0)) and compares the counters and output checksums with the oracle's (O.chain_plan);
the materialised pairs are checked pair by pair: every probe row once, paired with the build row
that holds its key. Probe keys are always build keys, so every probe tuple has a partner.
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

TILE = 8192  # tuples per partitioner tile
SEG = 16     # pairs per region segment


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
                "sum_c": 0, "sum_h": int(z.sum(dtype=np.uint64)), "xor_h": int(np.bitwise_xor.reduce(z)) if len(z) else 0}


class World:
    """Chaining tables of nb buckets over nb unique keys (built once per size), and one pool of
    random probe keys per table."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.tables = {}

    def table(self, nb):
        import hj3d
        if nb not in self.tables:
            rng = np.random.default_rng(nb)
            keys = rng.choice(1 << 26, size=nb, replace=False).astype(np.uint32)
            B = O.tuples3(keys, np.zeros(nb, np.uint32))
            t = hj3d.Table(self.ctx, hj3d.HJ3D_CHAIN, nb)
            t.build(hj3d.Rel(dev(B), 0))
            pool = keys[rng.integers(0, nb, 258 * TILE)]
            self.tables[nb] = (t, B, pool)
        return self.tables[nb]


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    for t, _, _ in w.tables.values():
        t.close()


@pytest.fixture
def pk(ctx):
    """Packed probe on every probe size; options restored afterwards."""
    ctx.radix_min(0)
    yield ctx
    ctx.pk_slice_max(0)
    ctx.pk_stage(0)
    ctx.radix_min(1 << 20)


def probe_rel(keys, mark=None):
    """{row index, key, mark} probe tuples."""
    Pt = O.tuples3(np.arange(len(keys), dtype=np.uint32), np.asarray(keys, dtype=np.uint32))
    if mark is not None:
        Pt[:, 2] = mark
    return Pt


def check(ctx, world, nb, Pt, preds=None, row_word=None):
    """One probe of Pt (key word 1) against the nb-bucket table, against the oracle."""
    import torch
    import hj3d
    t, B, _ = world.table(nb)
    exp_rel = Pt
    if preds is not None:  # the oracle takes the passing tuples with their row ids (word 0)
        exp_rel = Pt[O.select(Pt, 1, preds)[:, 1]]
    rw = row_word if row_word is not None else 0 if preds is not None else None
    e = O.chain_plan(B, 0, exp_rel, 1, nb, True, prow=rw)
    out = torch.full((len(Pt), 2), -1, dtype=torch.int32, device="cuda")
    rel = hj3d.Rel(dev(Pt), 1, row_word=row_word)
    r = ctx.probe_sel(t, rel, preds, unique=True, out=out) if preds is not None else ctx.probe(t, rel, unique=True, out=out)
    assert not r.overflow
    assert r.n_probe == len(exp_rel)
    assert (r.n_out, r.n_cmps) == (e.c_probe, e.c_cmp)
    assert {"n": r.n_out, "sum_a": r.sum_a, "sum_b": r.sum_b, "sum_c": 0, "sum_h": r.sum_h, "xor_h": r.xor_h} == e.out
    assert r.n_out == len(exp_rel)  # every probe key is a build key
    host = out.cpu().numpy().view(np.uint32)[:r.n_out]
    assert host_checksums(host) == e.out
    # every probe row once, each paired with the build row that holds its key
    rows = exp_rel[:, rw] if rw is not None else np.arange(len(Pt), dtype=np.uint32)
    by_row = np.argsort(rows, kind="stable")
    order = np.argsort(host[:, 0], kind="stable")
    assert np.array_equal(host[order, 0], rows[by_row])
    assert np.array_equal(exp_rel[by_row, 1], B[host[order, 1], 0])


def plan_p(ctx, nb, w, p):
    """Set the slice bound and check that the table lands on p slices in one level."""
    ctx.pk_slice_max(w)
    pl = ctx.pk_plan(nb, nb)
    assert (pl["P"], pl["P1"], pl["C"]) == (p, p, 1), pl


NB = 1 << 16
SIZES = [1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 256 * TILE - 1, 256 * TILE, 256 * TILE + 1]


@pytest.mark.parametrize("n", SIZES)
def test_probe_sizes(pk, world, n):
    """The final flush alone, one ragged tile, exactly one tile per workgroup (256 CUs) and one more."""
    plan_p(pk, NB, 64, 1024)
    check(pk, world, NB, probe_rel(world.table(NB)[2][:n]))


# (buckets, slice bound, slices): from half the CUs on, P is rounded to whole waves of workgroups (256 CUs)
@pytest.mark.parametrize("nb,w,p", [(8192, 0, 1), (8192, 2731, 3), (40000, 48, 1000), (NB, 64, 1024)])
def test_slice_counts(pk, world, nb, w, p):
    """Threads without a slice (P < 1024) and a narrower last slice (P = 3 and 1000)."""
    plan_p(pk, nb, w, p)
    for n in (17, 3 * TILE + 5):
        check(pk, world, nb, probe_rel(world.table(nb)[2][:n]))


@pytest.fixture(scope="module")
def by_slice(world):
    """Build keys of NB's table split into those of one slice (W = 64 buckets) and the others."""
    _, B, pool = world.table(NB)
    sl = (fmix32(B[:, 0]) % np.uint32(NB)) // np.uint32(64)
    s = int(np.bincount(sl, minlength=1024).argmax())
    mine = B[sl == s, 0]
    pool_sl = (fmix32(pool) % np.uint32(NB)) // np.uint32(64)
    return mine, pool[pool_sl != s]


@pytest.mark.parametrize("stacked", [False, True])
@pytest.mark.parametrize("k", [15, 16, 17, 31, 32, 33, 48])
def test_round_boundaries(pk, world, by_slice, k, stacked):
    """One slice receives exactly k pairs in one tile and none later: the round boundaries, the slot
    pos % 16 and the vote. stacked: the workgroup's tile before left that slice's window at fill 15
    (workgroup 0 takes tiles 0 and G; G = the CUs, so the relation has one tile more than CUs)."""
    import torch
    plan_p(pk, NB, 64, 1024)
    assert world.ctx.pk_plan(NB, NB)["W"] == 64
    mine, others = by_slice
    assert len(mine) >= 4
    rng = np.random.default_rng(k)
    if not stacked:
        keys = others[:TILE].copy()
        keys[rng.choice(TILE, k, replace=False)] = mine[rng.integers(0, len(mine), k)]
    else:
        g = torch.cuda.get_device_properties(0).multi_processor_count
        assert (g + 1) * TILE <= len(others)
        keys = others[:(g + 1) * TILE].copy()
        keys[rng.choice(TILE, SEG - 1, replace=False)] = mine[rng.integers(0, len(mine), SEG - 1)]
        keys[g * TILE + rng.choice(TILE, k, replace=False)] = mine[rng.integers(0, len(mine), k)]
    check(pk, world, NB, probe_rel(keys))


def hot_keys(world, half):
    _, B, pool = world.table(NB)
    keys = np.full(100_000, B[12345, 0], dtype=np.uint32)
    if half:
        keys[1::2] = pool[:50_000]
    return keys


@pytest.mark.parametrize("half", [False, True])
def test_hot_key(pk, world, half):
    """Every probe key equal (and: half the tuples on one key, half uniform): many rounds until the
    hot slice's region is full, the slice closing, its later pairs going straight to the overflow
    list; every row still appears once in the output."""
    plan_p(pk, NB, 64, 1024)
    check(pk, world, NB, probe_rel(hot_keys(world, half)))


def test_explicit_rows(pk, world):
    """The explicit-row form: row ids from a tuple word."""
    plan_p(pk, NB, 64, 1024)
    n = TILE + 1
    Pt = probe_rel(world.table(NB)[2][:n])
    Pt[:, 0] = np.random.default_rng(3).permutation(n).astype(np.uint32) + np.uint32(1000)
    check(pk, world, NB, Pt, row_word=0)


def test_explicit_rows_bucket_range_shards(pk, world):
    """Explicit rows on tables over bucket ranges [lo, hi) with lo != 0 (exp1_plan_sharded)."""
    import torch
    import hj3d
    pk.pk_slice_max(64)
    _, B, pool = world.table(NB)
    Pt = probe_rel(pool[:256 * TILE + 1])
    e = O.chain_plan(B, 0, Pt, 1, NB, True)
    out = torch.full((len(Pt), 2), -1, dtype=torch.int32, device="cuda")
    got = hj3d.exp1_plan_sharded(pk, "Csr", dev(B), dev(Pt), NB, 3, out=out)
    assert (got["c_probe"], got["c_cmp"], got["c_top"]) == (e.c_probe, e.c_cmp, e.c_top)
    assert got["out"] == e.out
    host = out.cpu().numpy().view(np.uint32)
    assert host_checksums(host) == e.out
    order = np.argsort(host[:, 0], kind="stable")
    assert np.array_equal(host[order, 0], np.arange(len(Pt), dtype=np.uint32))
    assert np.array_equal(Pt[:, 1], B[host[order, 1], 0])


def test_fused_selection(pk, world):
    """The SEL form: a one-word selection fused into the partitioner (probe_sel)."""
    plan_p(pk, NB, 64, 1024)
    n = 256 * TILE + 1
    mark = np.random.default_rng(5).integers(0, 100, n).astype(np.uint32)
    check(pk, world, NB, probe_rel(world.table(NB)[2][:n], mark), preds=[(2, "<", 37)])


def test_three_probes_in_a_row(pk, world):
    """Uniform, hot key, uniform on one context: the control words and the overflow list are back
    to zero after each probe, nothing is carried from one launch to the next."""
    plan_p(pk, NB, 64, 1024)
    uni = probe_rel(world.table(NB)[2][:3 * TILE + 7])
    check(pk, world, NB, uni)
    check(pk, world, NB, probe_rel(hot_keys(world, True)))
    check(pk, world, NB, uni)
