"""GPU parity of the packed probe's LDS walk (chain_pk.hip, k_pk_probe / pk_probe_items): the entry
reads of walk positions 0, 1, 2 batched over the items of a chunk (all K, or two halves of them),
the per-item walk of the later positions, the order-free form of long buckets, and the output
stores of present and absent items at every capacity.

Every case probes a chaining table with unique build keys through the packed unique probe
(radix_min(0)) and compares n_out, n_cmps and the output checksums with the oracle's
(O.chain_plan); the materialised pairs are checked pair by pair. `out` is always a view of the
first rows of a larger tensor prefilled with a canary: rows behind the view must keep it.

Shapes (hj3d_probe_geometry / pk_layout): a probe of n tuples has G = min(ceil(n / 8192), CUs)
regions per slice, P slices, expected region length n / (G P); below 256 the flat walk runs
(K = 8 unless forced), from 256 on the per-region walk (K chosen from the length).
"""
import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

TILE = 8192          # tuples per partitioner tile
CANARY = 0x5A5A5A5A  # no row id or partner of these tests
TAIL = 193           # canary rows behind `out`
NONE = 0xFFFFFFFF    # partner of a probe tuple without one


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
    """Chaining tables of nb buckets over nr unique keys below 2^26 (built once each), the probe
    relations drawn from them and the oracle's results, each computed once."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.tables = {}
        self.rels = {}
        self.refs = {}

    def table(self, nb, nr):
        import hj3d
        if (nb, nr) not in self.tables:
            rng = np.random.default_rng(nb * 131 + nr)
            keys = rng.choice(1 << 26, size=nr, replace=False).astype(np.uint32)
            B = O.tuples3(keys, np.zeros(nr, np.uint32))
            t = hj3d.Table(self.ctx, hj3d.HJ3D_CHAIN, nb)
            t.build(hj3d.Rel(dev(B), 0))
            self.tables[(nb, nr)] = (t, B)
        return self.tables[(nb, nr)]

    def rel(self, nb, nr, n, stray=0.0):
        """{row index, key, 0} probe tuples: build keys, a share `stray` of them replaced by keys
        no build tuple has (>= 2^26)."""
        k = (nb, nr, n, stray)
        if k not in self.rels:
            _, B = self.table(nb, nr)
            rng = np.random.default_rng(n * 7 + nb)
            keys = B[rng.integers(0, nr, n), 0].copy()
            if stray:
                lost = rng.random(n) < stray
                keys[lost] = rng.integers(1 << 26, 1 << 27, int(lost.sum())).astype(np.uint32)
            self.rels[k] = O.tuples3(np.arange(n, dtype=np.uint32), keys)
        return self.rels[k]

    def ref(self, nb, nr, n, stray=0.0):
        k = (nb, nr, n, stray)
        if k not in self.refs:
            self.refs[k] = O.chain_plan(self.table(nb, nr)[1], 0, self.rel(nb, nr, n, stray), 1, nb, True)
        return self.refs[k]


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    for t, _ in w.tables.values():
        t.close()


@pytest.fixture
def pk(ctx):
    """Packed probe on every probe size; options restored afterwards."""
    ctx.radix_min(0)
    yield ctx
    ctx.probe_items(0)
    ctx.pk_slice_max(0)
    ctx.radix_min(1 << 20)


def check_pairs(host, Pt, B, complete, rows=None):
    """host: the written rows {row, partner}. Every row id at most once (complete: each exactly
    once); a partner holds the row's key, a row without partner has a key no build tuple has."""
    rows = np.arange(len(Pt), dtype=np.uint32) if rows is None else rows
    assert not np.any(host[:, 0] == CANARY), "a row below the capacity was not written"
    order = np.argsort(host[:, 0], kind="stable")
    got = host[order]
    by_row = np.argsort(rows, kind="stable")
    if complete:
        assert np.array_equal(got[:, 0], rows[by_row])
        keys = Pt[by_row, 1]
    else:
        assert len(np.unique(got[:, 0])) == len(got)
        pos = np.searchsorted(rows[by_row], got[:, 0])
        assert np.all(pos < len(rows)) and np.array_equal(rows[by_row][pos], got[:, 0])
        keys = Pt[by_row[pos], 1]
    m = got[:, 1] != NONE
    assert np.all(got[m, 1] < len(B))
    assert np.array_equal(B[got[m, 1], 0], keys[m])
    assert not np.any(np.isin(keys[~m], B[:, 0]))
    return got[m]


def check(ctx, world, nb, nr, n, stray=0.0, cap=None):
    """One probe of n tuples against the (nb, nr) table into a view of cap rows (default n)."""
    import torch
    import hj3d
    t, B = world.table(nb, nr)
    Pt = world.rel(nb, nr, n, stray)
    e = world.ref(nb, nr, n, stray)
    cap = n if cap is None else cap
    big = torch.full((cap + TAIL, 2), CANARY, dtype=torch.int32, device="cuda")
    r = ctx.probe(t, hj3d.Rel(dev(Pt), 1), unique=True, out=big[:cap])
    # counters and checksums cover every probe tuple, whatever the capacity (as before this walk)
    assert r.overflow == (cap < n)
    assert r.n_probe == n
    assert (r.n_out, r.n_cmps) == (e.c_probe, e.c_cmp)
    assert {"n": r.n_out, "sum_a": r.sum_a, "sum_b": r.sum_b, "sum_c": 0, "sum_h": r.sum_h, "xor_h": r.xor_h} == e.out
    host = big.cpu().numpy().view(np.uint32)
    assert np.all(host[cap:] == CANARY), "a store landed behind the capacity"
    matched = check_pairs(host[:min(cap, n)], Pt, B, complete=cap >= n)
    if cap >= n:
        assert host_checksums(matched) == e.out
        if not stray:
            assert r.n_out == n


def plan(ctx, nb, w, p):
    ctx.pk_slice_max(w)
    pl = ctx.pk_plan(nb, nb)
    assert (pl["P"], pl["C"]) == (p, 1), pl


ONE = (8192, 0, 1)        # (buckets = build keys, slice bound, slices)
THREE = (25000, 10000, 3)
# flat walk (expected region length n / (G P) < 256: one tile, so G = 1) and per-region walk; region
# lengths that are no multiple of 64, one pair, one pair more than a K = 8 / K = 7 chunk
SIZES_ONE = [1, 63, 200, 255, 256, 449, 513, 3 * TILE + 5]
SIZES_THREE = [17, 700, 767, 768, 4 * TILE + 77, 64 * TILE + 1]


@pytest.mark.parametrize("n", SIZES_ONE)
def test_one_slice(pk, world, n):
    """1 slice: n < 256 flat, beyond per region (n = 3 tiles + 5: 4 workgroups of one region)."""
    nb, w, p = ONE
    plan(pk, nb, w, p)
    check(pk, world, nb, nb, n)


@pytest.mark.parametrize("n", SIZES_THREE)
def test_three_slices(pk, world, n):
    """3 slices: n < 768 flat (regions of ~n / 3 pairs), beyond per region; 64 tiles: 64 regions
    per slice over 64 workgroups each."""
    nb, w, p = THREE
    plan(pk, nb, w, p)
    check(pk, world, nb, nb, n)


@pytest.mark.parametrize("n", [20 * TILE + 3, 40 * TILE + 3])
def test_flat_many_regions(pk, world, n):
    """1024 slices of 64 buckets: regions of ~8 pairs, 20 and 40 per slice, so a wave's flat stream
    crosses region boundaries inside every chunk."""
    nb = 1 << 16
    plan(pk, nb, 64, 1024)
    check(pk, world, nb, nb, n)


@pytest.mark.parametrize("k", [5, 6, 7, 8])
@pytest.mark.parametrize("n", [255, 64 * 7 + 1, 4 * TILE + 77])
def test_every_k(pk, world, k, n):
    """K forced: flat (n = 255), one region of 64 * 7 + 1 pairs (K = 7: one pair more than a chunk),
    and ~2 760-pair regions of 3 slices."""
    nb, w, p = ONE if n < TILE else THREE
    plan(pk, nb, w, p)
    pk.probe_items(k)
    check(pk, world, nb, nb, n, stray=0.25 if n == 255 else 0.0)


@pytest.mark.parametrize("k", [5, 6, 7, 8])
def test_region_of_one_chunk_and_a_pair(pk, world, k):
    """One region of exactly 64 K + 1 pairs (1 slice, one tile, per-region walk from 256 pairs on)."""
    nb, w, p = ONE
    plan(pk, nb, w, p)
    pk.probe_items(k)
    check(pk, world, nb, nb, 64 * k + 1)


@pytest.mark.parametrize("k", [0, 7, 8])
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("n", [250, 2 * TILE + 9])
def test_deep_buckets(pk, world, depth, n, k):
    """nb = |R| / 8 and |R| / 16: most probes walk past position 3 (the per-item tail and its
    n_cmps), flat and per region; K chosen by the library, 7, and 8 (two half chunks)."""
    nb = 1024
    pk.probe_items(k)
    check(pk, world, nb, nb * depth, n, stray=0.1)


@pytest.mark.parametrize("k", [0, 7, 8])
@pytest.mark.parametrize("n", [250, TILE + 11])
def test_long_buckets(pk, world, n, k):
    """64 buckets of ~40 entries: most hold more than 32 (the order-free form), the others walk
    the sorted form in the same chunk."""
    nb, nr = 64, 2560
    _, B = world.table(nb, nr)
    fill = np.bincount(fmix32(B[:, 0]) % np.uint32(nb), minlength=nb)
    assert (fill > 32).sum() >= 32 and (fill <= 32).sum() >= 2
    pk.probe_items(k)
    check(pk, world, nb, nr, n, stray=0.1)


@pytest.mark.parametrize("nb,w,p,n", [ONE + (200,), ONE + (3 * TILE + 5,), THREE + (700,), THREE + (4 * TILE + 77,)])
def test_without_partner(pk, world, nb, w, p, n):
    """A third of the probe keys have no partner: the slot is written with partner 0xFFFFFFFF."""
    plan(pk, nb, w, p)
    check(pk, world, nb, nb, n, stray=0.33)


@pytest.mark.parametrize("nb,w,p,n", [ONE + (200,), ONE + (3 * TILE + 5,), THREE + (700,), THREE + (4 * TILE + 77,)])
@pytest.mark.parametrize("cap", ["half", 1])
def test_capacity_below_probe_count(pk, world, nb, w, p, n, cap):
    """`out` holds n / 2 rows, and one row: counters and checksums as with room for all, overflow
    reported, the rows below the capacity valid pairs, the canary behind it intact."""
    plan(pk, nb, w, p)
    check(pk, world, nb, nb, n, cap=n // 2 if cap == "half" else 1)


@pytest.mark.parametrize("nb,w,p,sizes", [ONE + ((201, 3 * TILE + 5, 77, 449),), THREE + ((701, 4 * TILE + 77, 333, 65 * TILE + 1),)])
def test_accumulated_probes(pk, world, nb, w, p, sizes):
    """A strand of four probes into one `out`, the last three accumulating: each writes behind the
    one before, so the output bases are nonzero, odd and not 64-aligned. The totals are the
    oracle's for the concatenated probe side (explicit row ids)."""
    import torch
    import hj3d
    plan(pk, nb, w, p)
    t, B = world.table(nb, nb)
    n = sum(sizes)
    Pt = world.rel(nb, nb, n, 0.2).copy()
    Pt[:, 0] = np.random.default_rng(n).permutation(n).astype(np.uint32) + np.uint32(1000)
    e = O.chain_plan(B, 0, Pt, 1, nb, True, prow=0)
    big = torch.full((n + TAIL, 2), CANARY, dtype=torch.int32, device="cuda")
    o = 0
    for i, m in enumerate(sizes):
        rel = hj3d.Rel(dev(Pt[o:o + m]), 1, row_word=0)
        r = pk.probe(t, rel, unique=True, out=big[o:o + m], accumulate=i > 0, fetch=i == len(sizes) - 1)
        o += m
    assert not r.overflow
    assert r.n_probe == n
    assert (r.n_out, r.n_cmps) == (e.c_probe, e.c_cmp)
    assert {"n": r.n_out, "sum_a": r.sum_a, "sum_b": r.sum_b, "sum_c": 0, "sum_h": r.sum_h, "xor_h": r.xor_h} == e.out
    host = big.cpu().numpy().view(np.uint32)
    assert np.all(host[n:] == CANARY)
    assert host_checksums(check_pairs(host[:n], Pt, B, complete=True, rows=Pt[:, 0])) == e.out
