"""GPU parity on keys with CHOSEN hashes and on keys that use all 32 bits (tests/keyspace.py).

The other parity tests draw their keys from a small dense domain, so the hashes the kernels see are
whatever murmur makes of them. Here fmix32 is inverted on the host and the kernels that work on
hashes (FastMod, FastDiv32, the packed {bucket-in-slice | h / NB} words of chain_pk.hip, the LDS
aggregation table of nested_agg.hip and its `empty` marker) are fed hash 0, hash 0xFFFFFFFF, the
last incomplete quotient row, the first and last bucket of every slice / partition / owner range and
identity hashes h == bucket, next to full-range random keys (the nested sort build's 4-pass width).

Every expectation comes from the oracle (O.chain_plan, O.nested_plan, O.exp4_plan) or from plain
Python integers; nothing is expected from the library. Every case asserts all counters, the 12
statistics and the output checksums bit-exact, and the table's build path, so that a silent
fallback cannot pass as coverage."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import keyspace as KS
import oracle as O

pytestmark = pytest.mark.gpu

STAT_KEYS = ("nb", "empty", "entries", "distinct", "cc0_min", "cc0_max", "cc0_sum", "cc0_cnt",
             "cc1_min", "cc1_max", "cc1_sum", "cc1_cnt")
N_R, N_S = 100_000, 400_000  # the shapes of test_nested_agg_build_vs_oracle
NESTED_WIDTHS = (384, 1024, 1536, 6144)
CHAIN_WIDTHS = (64, 1024, 8192, 16384)
# entries per chosen bucket (keyspace.adversarial_keys `group`), per nested nb: 48 unless a group of
# 48 pushed an aggregation build onto the sort fallback (never below 33). None was reduced.
NESTED_GROUP = {}

OPTION_DEFAULTS = dict(radix_min=1 << 20, force_direct=False, nested_sort=False, nested_pk=False, pk_slice_max=0,
                       pk_build=False, packed_probe=True, diag_gbar=0)


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


def host_checksums(pairs: np.ndarray) -> dict:
    """Order-independent checksums of emitted (a, b) pairs, computed on the host."""
    a = pairs[:, 0].astype(np.uint64)
    b = pairs[:, 1].astype(np.uint64)
    z = (a << np.uint64(32)) | b
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        z = z ^ (z >> np.uint64(31))
        return {"n": len(pairs), "sum_a": int(a.sum(dtype=np.uint64)), "sum_b": int(b.sum(dtype=np.uint64)),
                "sum_c": 0, "sum_h": int(z.sum(dtype=np.uint64)), "xor_h": int(np.bitwise_xor.reduce(z)) if len(z) else 0}


class Exp1Data:
    """R {k = K, 0, 0} and S {i, a, 0} over adversarial keys K for a table of nb buckets: 320 000 of
    S.a are K[random], a further quarter of that number (80 000) are full-range random keys (drawn
    from a pool a fifth of |R| wide, mostly without a partner), 400 000 tuples in all. The oracle's
    plans are computed once and shared."""

    def __init__(self, nb, widths, group=48, lo=0, hi=None, identity=None):
        rng = np.random.default_rng(1000 + nb)
        self.nb = nb
        self.K = KS.adversarial_keys(nb, N_R, widths, rng, group=group, lo=lo, hi=hi, identity=identity)
        n_match = N_S * 4 // 5
        pool = rng.integers(0, 1 << 32, N_R // 5, dtype=np.uint64).astype(np.uint32)
        Sa = np.concatenate([self.K[rng.integers(0, N_R, n_match)], pool[rng.integers(0, len(pool), N_S - n_match)]])
        Sa = rng.permutation(Sa).astype(np.uint32)
        self.R = O.tuples3(self.K, np.zeros(N_R, np.uint32))
        self.S = O.tuples3(np.arange(N_S, dtype=np.uint32), Sa)
        self._plans = {}

    def oracle(self, plan):
        if plan not in self._plans:
            R, S, nb = self.R, self.S, self.nb
            self._plans[plan] = {
                "Csr": lambda: O.chain_plan(R, 0, S, 1, nb, True), "CsrUU": lambda: O.chain_plan(R, 0, S, 1, nb, False),
                "Crs": lambda: O.chain_plan(S, 1, R, 0, nb, False), "Nsr": lambda: O.nested_plan(R, 0, S, 1, nb, True),
                "Nrs": lambda: O.nested_plan(S, 1, R, 0, nb, True), "NrsNU": lambda: O.nested_plan(S, 1, R, 0, nb, False),
            }[plan]()
        return self._plans[plan]


_EXP1 = {}


def exp1_data(nb, widths, group=48, lo=0, hi=None, identity=None):
    key = (nb, tuple(widths), group, lo, hi, identity)
    if key not in _EXP1:
        _EXP1[key] = Exp1Data(nb, widths, group, lo, hi, identity)
    return _EXP1[key]


def check_plan(got, e, tag):
    assert (got["c_probe"], got["c_cmp"], got["c_unnest"], got["c_top"]) == \
        (e.c_probe, e.c_cmp, e.c_unnest, e.c_top), tag
    assert got["out"] == e.out, tag
    if "stats" in got:
        assert {k: got["stats"][k] for k in STAT_KEYS} == {k: e.stats[k] for k in STAT_KEYS}, tag


# ---- case 1: nested ----

NESTED_MODES = {
    "agg": {}, "slices": {"nested_pk": True}, "sort": {"nested_sort": True}, "direct": {"force_direct": True},
    "slice64_probe": {"pk_slice_max": 64},  # the partitioned probe on 64-bucket slices
}


def nested_path_ok(mode, nb, path):
    if mode in ("sort", "direct"):  # direct: HJ3D_OPT_FORCE_DIRECT sends nested builds to the sort build
        return path == "nested_sort"  # full-range keys: the LSD sort's 4-pass (32-bit) width
    if mode == "slices":
        # below 20 000 buckets (14 or more distinct keys per bucket here) the slice form gives up by
        # design, as in test_nested_agg_build_vs_oracle: its 1024-bucket slices keep the 512-thread
        # form's table of ~8 keys per bucket
        return path.startswith("nested_agg_slices") if nb >= 20000 else path == "nested_sort"
    return path.startswith("nested_agg")


@pytest.mark.parametrize("nb", [7000, 20000, 100000])
def test_nested_chosen_hashes(ctx, nb):
    """Nsr, Nrs and NrsNU at ~14-17, 5-6 and 1 distinct keys per bucket by the aggregation build, the
    aggregation build on the packed slices, the sort build and the direct (unpartitioned) kernels.
    The counters, statistics and checksums of every plan and mode are compared first; the build
    paths are asserted after them.

    At nb = 7000 the path assertion found a silent fallback: the aggregation build started
    ("nested_agg?") and gave up, so every table ended as "nested_sort", at any group size (48, 40,
    33, 1) and with the dense keys of test_nested_agg_build_vs_oracle too. A 7000-bucket table gets
    1024-bucket partitions, and the 512-thread form's LDS table of 2113 slots holds ~8 distinct keys
    per bucket in its last halved round of 256 buckets; 100 000 build keys in 7000 buckets are 14.
    One-level tables of at most one partition per CU now take the 1024-thread form's table (~24
    keys per bucket), and the group stays at 48."""
    import hj3d
    d = exp1_data(nb, NESTED_WIDTHS, NESTED_GROUP.get(nb, 48))
    assert int(d.K.max()) == 0xFFFFFFFF and int(d.S[:, 1].max()) >= 1 << 31  # 32-bit keys on both build sides
    dR, dS = dev(d.R), dev(d.S)
    wrong_paths = []
    for plan in ("Nsr", "Nrs", "NrsNU"):
        e = d.oracle(plan)
        for mode, opts in NESTED_MODES.items():
            with options(ctx, radix_min=0, **opts):
                t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
                got = hj3d.exp1_plan(ctx, plan, dR, dS, nb, table=t)
                path = t.build_path()
                t.close()
            check_plan(got, e, (plan, mode, path))
            if not nested_path_ok(mode, nb, path):
                wrong_paths.append((plan, mode, path))
    assert not wrong_paths, wrong_paths


@pytest.mark.parametrize("plan", ["Nrs", "NrsNU", "Nsr"])
def test_nested_two_level_probe_chosen_hashes(ctx, plan):
    """The nested probe on the packed partitioner's two levels (more than 2048 slices: a 200 K-bucket
    table under a slice bound of 64 buckets, as test_nested_probe_two_level_slices), chosen hashes at
    the slice edges; the materialised pairs too."""
    import torch
    import hj3d
    nb = 200_000
    d = exp1_data(nb, (64, 61, 1024, 6144))
    e = d.oracle(plan)
    dR, dS = dev(d.R), dev(d.S)
    with options(ctx, radix_min=0, pk_slice_max=64):
        t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
        got = hj3d.exp1_plan(ctx, plan, dR, dS, nb, table=t)
        path = t.build_path()
        check_plan(got, e, (plan, path))
        assert path.startswith("nested_agg"), path
        out = torch.zeros((max(e.out["n"], N_S, N_R), 2), dtype=torch.int32, device="cuda")
        got = hj3d.exp1_plan(ctx, plan, dR, dS, nb, out=out, stats=False, table=t)
        t.close()
    assert not got["overflow"]
    pairs = out.cpu().numpy().view(np.uint32)
    if plan == "NrsNU":  # one slot per probe tuple (R), unmatched slots carry 0xFFFFFFFF
        pairs = pairs[:N_R]
        pairs = pairs[pairs[:, 1] != 0xFFFFFFFF]
    else:
        pairs = pairs[: e.out["n"]]
    assert host_checksums(pairs) == e.out, plan


# ---- case 2: chaining ----

CHAIN_MODES = {
    "radix": ({}, "radix"), "direct": ({"force_direct": True}, "direct"), "slices": ({"pk_build": True}, "slices"),
    "unpacked_probe": ({"packed_probe": False}, "radix"), "two_level_packed": ({"pk_slice_max": 64}, "radix"),
}


@pytest.mark.parametrize("nb", [100_000, 131072, 99991], ids=["fill1", "pow2", "prime"])
def test_chaining_chosen_hashes(ctx, nb):
    """Csr, CsrUU and Crs at nb = |R|, a power of two (FastDiv32's magic-0 branch) and a prime, by
    the radix build, the direct build and the two-level slice build, with the packed unique probe on
    (one and two partition levels) and off. Csr's dense output pairs are checked as well."""
    g = ctx.pk_plan(nb, N_R)
    widths = tuple(sorted({int(g["W"]), int(g["W1"]), *CHAIN_WIDTHS} - {0}))
    # The slice build falls back to the direct build when a partition region overflows. 50 000
    # identity hashes fill the lowest buckets only (1.5 times the mean in the first slices, beyond
    # the regions' 8-sigma slack), so that mode runs on keys with 256 of them; every other chosen
    # hash is the same.
    for d, modes in ((exp1_data(nb, widths), [m for m in CHAIN_MODES if m != "slices"]),
                     (exp1_data(nb, widths, identity=256), ["slices", "radix"])):
        _chaining_case(ctx, d, nb, modes)


def _chaining_case(ctx, d, nb, modes):
    import torch
    import hj3d
    dR, dS = dev(d.R), dev(d.S)
    for plan in ("Csr", "CsrUU", "Crs"):
        e = d.oracle(plan)
        for mode in modes:
            opts, want = CHAIN_MODES[mode]
            with options(ctx, radix_min=0, **opts):
                t = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, nb)
                got = hj3d.exp1_plan(ctx, plan, dR, dS, nb, table=t)
                path = t.build_path()
                check_plan(got, e, (plan, mode, path))
                assert path == want, (plan, mode, path)
                if plan == "Csr":  # one slot per probe tuple, unmatched slots carry 0xFFFFFFFF
                    out = torch.zeros((N_S, 2), dtype=torch.int32, device="cuda")
                    got = hj3d.exp1_plan(ctx, plan, dR, dS, nb, out=out, stats=False, table=t)
                    assert not got["overflow"], mode
                    pairs = out.cpu().numpy().view(np.uint32)
                    assert (np.sort(pairs[:, 0]) == np.arange(N_S, dtype=np.uint32)).all(), mode
                    assert host_checksums(pairs[pairs[:, 1] != 0xFFFFFFFF]) == e.out, mode
                t.close()


# ---- case 3: owner ranges ----

@pytest.mark.parametrize("parts", [3, 8])
def test_owner_ranges_chosen_hashes(ctx, parts, monkeypatch):
    """hj3d.exp1_plan_sharded (exchange partitioner, then one table per owned bucket range, explicit
    global rows) with chosen hashes in the first and last bucket of every owner: the merged counters,
    statistics and checksums equal the single-table oracle's."""
    import hj3d
    nb = 20000
    rng_ = [hj3d.part_range(nb, parts, p) for p in range(parts)]
    d = exp1_data(nb, NESTED_WIDTHS + (64, 8192), 48, tuple(lo for lo, _ in rng_), tuple(hi for _, hi in rng_))
    h = (KS.fmix32(d.K).astype(np.uint64) % np.uint64(nb)).tolist()
    for lo, hi in rng_:
        assert h.count(lo) >= 48 and h.count(hi - 1) >= 48, (lo, hi)
    paths = []

    class Recorded(hj3d.Table):  # the owners' tables are made inside exp1_plan_sharded
        def close(self):
            if getattr(self, "h", None):
                paths.append(self.build_path())
            super().close()
    monkeypatch.setattr(hj3d.plans, "Table", Recorded)
    dR, dS = dev(d.R), dev(d.S)
    with options(ctx, radix_min=0):
        for plan, single, ok in (("Csr", False, lambda p: p == "radix"), ("Csr", True, lambda p: p == "radix"),
                                 ("Nrs", False, lambda p: p.startswith("nested_agg"))):
            del paths[:]
            got = hj3d.exp1_plan_sharded(ctx, plan, dR, dS, nb, parts, single_pass=single)
            check_plan(got, d.oracle(plan), (plan, single, paths))
            assert len(paths) == parts and all(ok(p) for p in paths), (plan, paths)


# ---- case 4: experiment 4 ----

class Exp4Data:
    def __init__(self):
        rng = np.random.default_rng(4)
        self.nb, nR = 8192, 1 << 16
        K = KS.adversarial_keys(self.nb, nR, (64, 384, 1024, 1536), rng)
        quarter = K[: nR // 4]
        self.R = O.tuples2(K, np.zeros(nR, np.uint32))
        n = 3 * nR
        self.S = O.tuples2(np.arange(n, dtype=np.uint32), quarter[rng.integers(0, len(quarter), n)])
        self.T = O.tuples2(np.arange(n, dtype=np.uint32), quarter[rng.integers(0, len(quarter), n)])
        self.oracle = {"Ndu": O.exp4_plan(self.R, self.S, self.T, self.nb, True),
                       "Chj": O.exp4_plan(self.R, self.S, self.T, self.nb, False)}


@functools.lru_cache(maxsize=1)
def exp4_data():
    return Exp4Data()


EXP4_COUNTERS = ("c_probe_rs", "c_probe_rs_cmp", "c_probe_rt", "c_probe_rt_cmp", "c_top")


def check_exp4(plan, got, e, tag):
    keys = EXP4_COUNTERS + (("c_unnest_1", "c_unnest_2") if plan == "Ndu" else ())
    assert {k: got[k] for k in keys} == {k: e[k] for k in keys}, tag
    assert {k: got[k] for k in ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")} == \
        {k: e["out"][k] for k in ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")}, tag
    assert e["out"]["n"] == e["c_top"] == got["c_top"], tag


@pytest.mark.parametrize("probe", ["default", "partitioned"])
@pytest.mark.parametrize("plan,fused,sort,want", [("Ndu", True, False, "nested_agg"), ("Ndu", False, False, "nested_agg"),
                                                  ("Ndu", False, True, "nested_sort"), ("Chj", True, False, "radix")],
                         ids=["Ndu_build_many", "Ndu_two_builds", "Ndu_sort_build", "Chj"])
def test_exp4_chosen_hashes(ctx, monkeypatch, plan, fused, sort, want, probe):
    """Experiment 4 (log2R = 16, 8192 buckets) on adversarial R keys, S.a and T.a from their first
    quarter (three tuples per R tuple): Ndu with both tables from one hj3d_build_many and from two
    hj3d_build calls, by the aggregation and by the sort build (32-bit keys: four passes), and Chj;
    the default and the partitioned probe strand."""
    import hj3d
    d = exp4_data()
    tables = []

    class Recorded(hj3d.Table):  # exp4_plan makes its own tables
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            tables.append(self)
    monkeypatch.setattr(hj3d.plans, "Table", Recorded)
    opts = {"radix_min": 1 << 6} if probe == "partitioned" else {}
    with options(ctx, nested_sort=sort, **opts):
        got = hj3d.exp4_plan(ctx, plan, dev(d.R), dev(d.S), dev(d.T), d.nb, fused=fused)
        paths = [t.build_path() for t in tables]
    for t in tables:
        t.close()
    check_exp4(plan, got, d.oracle[plan], (plan, fused, sort, probe, paths))
    assert len(paths) == 2 and all(p.startswith(want) if want == "nested_agg" else p == want for p in paths), paths


@pytest.mark.parametrize("plan", ["Ndu", "Chj"])
def test_exp4_chosen_hashes_triples(ctx, plan):
    """The materialised (r, s, t) triples of the same run reproduce the oracle's checksums."""
    import torch
    import hj3d
    d = exp4_data()
    e = d.oracle[plan]
    out = torch.full((e["c_top"], 3), -1, dtype=torch.int32, device="cuda")
    got = hj3d.exp4_plan(ctx, plan, dev(d.R), dev(d.S), dev(d.T), d.nb, out=out)
    assert got["overflow"] is False
    check_exp4(plan, got, e, plan)
    assert hj3d.triple_checksums(out.cpu().numpy().view(np.uint32)) == e["out"]


# ---- case 5: row ids and layouts ----

LAYOUTS = ("top_rows", "bit31_rows", "one_word", "five_words", "unaligned_base")
LAYOUT_NB, LAYOUT_NBUILD, LAYOUT_NPROBE = 7000, 20_000, 60_000


def layout(keys, variant, rng):
    """One relation over the key column `keys` in the given layout: (device Rel and what keeps its
    memory alive, oracle array, oracle key word, oracle row word or None)."""
    import torch
    import hj3d
    n = len(keys)
    if variant == "top_rows":  # implicit rows row_base + i up to 2^32 - 2 (0xFFFFFFFF is not a row)
        base = (1 << 32) - 1 - n
        A = O.tuples3(keys, np.zeros(n, np.uint32))
        rows = (np.arange(n, dtype=np.uint64) + np.uint64(base)).astype(np.uint32)
        assert int(rows[-1]) == 0xFFFFFFFE
        return hj3d.Rel(dev(A), 0, row_base=base), np.stack([keys, rows], axis=1), 0, 1
    if variant == "bit31_rows":  # explicit ascending row ids with bit 31 set
        rows = (np.sort(rng.choice((1 << 31) - 1, n, replace=False)).astype(np.uint64) + np.uint64(1 << 31)).astype(np.uint32)
        A = np.stack([keys, rows], axis=1)
        return hj3d.Rel(dev(A), 0, row_word=1), A, 0, 1
    if variant == "one_word":  # stride 4
        A = keys.reshape(n, 1).copy()
        return hj3d.Rel(dev(A), 0), A, 0, None
    if variant == "five_words":  # stride 20, the key in word 3, other words arbitrary
        A = rng.integers(0, 1 << 32, (n, 5), dtype=np.uint64).astype(np.uint32)
        A[:, 3] = keys
        return hj3d.Rel(dev(A), 3), A, 3, None
    assert variant == "unaligned_base"  # a tensor sliced from row 1: 4-byte, not 16-byte aligned
    A = O.tuples3(keys, np.zeros(n, np.uint32))
    T = torch.zeros((n + 1, 3), dtype=torch.int32, device="cuda")
    T[1:] = dev(A)
    rel = hj3d.Rel(T[1:], 0)
    assert rel.c.base % 16 == 12
    return rel, A, 0, None


@functools.lru_cache(maxsize=1)
def layout_keys():
    rng = np.random.default_rng(5)
    K = KS.adversarial_keys(LAYOUT_NB, LAYOUT_NBUILD, NESTED_WIDTHS + (64,), rng)
    n_match = LAYOUT_NPROBE * 3 // 4
    P = np.concatenate([K[rng.integers(0, len(K), n_match)],
                        rng.integers(0, 1 << 32, LAYOUT_NPROBE - n_match, dtype=np.uint64).astype(np.uint32)])
    return K, rng.permutation(P).astype(np.uint32)


@pytest.mark.parametrize("variant", LAYOUTS)
@pytest.mark.parametrize("kind", ["chaining", "nested"])
def test_row_ids_and_layouts(ctx, kind, variant):
    """Row ids at the top of the u32 range and with bit 31 set, tuples of 1 and of 5 words and a base
    pointer that is not 16-byte aligned, on both sides of a chaining and of a nested join at 7000
    buckets; the oracle gets the same rows through brow / prow."""
    import hj3d
    K, P = layout_keys()
    rng = np.random.default_rng(LAYOUTS.index(variant))
    brel, BA, bkey, brow = layout(K, variant, rng)
    prel, PA, pkey, prow = layout(P, variant, rng)
    nested = kind == "nested"
    if nested:
        cases = [(dict(unnest=True), O.nested_plan(BA, bkey, PA, pkey, LAYOUT_NB, True, brow=brow, prow=prow)),
                 (dict(unnest=False), O.nested_plan(BA, bkey, PA, pkey, LAYOUT_NB, False, brow=brow, prow=prow))]
    else:
        cases = [(dict(unique=u), O.chain_plan(BA, bkey, PA, pkey, LAYOUT_NB, u, brow=brow, prow=prow))
                 for u in (True, False)]
    for mode, opts, want in (("partitioned", {}, "nested_agg" if nested else "radix"),
                             ("direct", {"force_direct": True}, "nested_sort" if nested else "direct")):
        with options(ctx, radix_min=0, **opts):
            t = hj3d.Table(ctx, hj3d.HJ3D_NESTED if nested else hj3d.HJ3D_CHAIN, LAYOUT_NB)
            t.build(brel)
            for flags, e in cases:
                r = ctx.probe(t, prel, **flags)
                tag = (kind, variant, mode, flags)
                if nested:
                    un = flags["unnest"]
                    assert (r.n_matched, r.n_cmps, r.n_out if un else 0, r.n_out if un else r.n_matched) == \
                        (e.c_probe, e.c_cmp, e.c_unnest, e.c_top), tag
                else:
                    assert (r.n_out, r.n_cmps) == (e.c_probe, e.c_cmp), tag
                assert {"n": r.n_out, "sum_a": r.sum_a, "sum_b": r.sum_b, "sum_c": r.sum_c, "sum_h": r.sum_h,
                        "xor_h": r.xor_h} == e.out, tag
            st = t.stats()
            assert {k: st[k] for k in STAT_KEYS} == {k: cases[0][1].stats[k] for k in STAT_KEYS}, (kind, variant, mode)
            path = t.build_path()
            t.close()
        assert path.startswith(want) if want == "nested_agg" else path == want, (kind, variant, mode, path)


# ---- case 6: the exchange partitioners at the extremes of NB ----

XP_NPARTS = (1, 2, 3, 7, 256)


def partition_hashes(NB, rng, n=20_000):
    """~n hashes at m * NB + {-1, 0, 1}, in the first and last bucket of every owner range of every
    part count, the top 1000 u32 values, and random ones for the rest."""
    h = set(range((1 << 32) - 1000, 1 << 32))
    qmax = ((1 << 32) - 1) // NB
    for m in sorted({0, 1, 2, qmax // 2, qmax - 1, qmax, qmax + 1} | set(range(min(qmax, 64)))):
        h.update(m * NB + dlt for dlt in (-1, 0, 1))
    for parts in XP_NPARTS:
        for p in range(parts + 1):
            b = -(-p * NB // parts)
            for q in (0, 1, qmax):
                h.update(q * NB + b + dlt for dlt in (-1, 0))
    h = np.array(sorted(v for v in h if 0 <= v < (1 << 32)), dtype=np.uint64)
    extra = rng.integers(0, 1 << 32, max(n - len(h), 0), dtype=np.uint64)
    return rng.permutation(np.concatenate([h, extra])).astype(np.uint32)


@pytest.mark.parametrize("NB", [1, 3, 1 << 31, (1 << 31) + 1, 4294967291, (1 << 32) - 1])
def test_exchange_partitioners_at_extreme_bucket_counts(ctx, NB):
    """hj3d_partition (stable) and hj3d_partition_strided (stride = n) for the smallest and the
    largest bucket counts and 1 to 256 parts (part counts at and above NB included: the strided
    form's owner magic is clamped there): per-destination counts, the multiset of (key, row) pairs per
    destination and, for the stable form, input order inside a destination. Expected owner of hash h:
    (h % NB) * nparts // NB in Python integers."""
    import torch
    import hj3d
    rng = np.random.default_rng(NB % 1000)
    H = partition_hashes(NB, rng)
    keys = KS.unfmix32(H)
    n = len(keys)
    rel = hj3d.Rel(dev(keys.reshape(n, 1)), 0)
    pairs = np.stack([keys, np.arange(n, dtype=np.uint32)], axis=1)
    hs = [int(v) for v in H]
    for parts in XP_NPARTS:
        own = np.array([(h % NB) * parts // NB for h in hs], dtype=np.int64)
        assert own.min() >= 0 and own.max() < parts
        want_counts = np.bincount(own, minlength=parts)
        order = np.argsort(own, kind="stable")
        starts = np.concatenate([[0], np.cumsum(want_counts)])
        # stable form: destinations back to back, input order kept
        out = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(parts, dtype=torch.int64, device="cuda")
        ctx.partition(rel, NB, parts, out, cnt)
        ctx.sync()
        assert cnt.cpu().numpy().tolist() == want_counts.tolist(), (NB, parts, "stable")
        assert np.array_equal(out.cpu().numpy().view(np.uint32), pairs[order]), (NB, parts, "stable")
        # single-pass form: destination p at rows [p * n, p * n + counts[p]), any order
        out = torch.full((parts * n, 2), -1, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(parts, dtype=torch.int64, device="cuda")
        ctx.partition(rel, NB, parts, out, cnt, stride=n)
        ctx.sync()
        assert cnt.cpu().numpy().tolist() == want_counts.tolist(), (NB, parts, "strided")
        got = out.cpu().numpy().view(np.uint32).reshape(parts, n, 2)
        for p in np.nonzero(want_counts)[0]:
            g = got[p, : want_counts[p]]
            w = pairs[order[starts[p]:starts[p + 1]]]
            assert np.array_equal(g[np.argsort(g[:, 1])], w), (NB, parts, int(p), "strided")  # rows are unique
        # nothing past a destination's count was written
        tail = np.arange(n)[None, :] >= want_counts[:, None]
        assert (got[tail] == 0xFFFFFFFF).all(), (NB, parts, "strided tail")


# ---- case 7: the fused partition's barrier tag stays off nested tables ----

class GiveUpData:
    """The shape whose aggregation build gives up (~50 distinct keys per bucket): dense keys."""

    def __init__(self):
        rng = np.random.default_rng(7)
        self.nb = 2000
        self.R = O.tuples3(rng.permutation(N_R).astype(np.uint32), np.zeros(N_R, np.uint32))
        self.S = O.tuples3(np.arange(N_S, dtype=np.uint32), rng.integers(0, N_R, N_S).astype(np.uint32))
        self.e = O.nested_plan(self.S, 1, self.R, 0, self.nb, True)


@functools.lru_cache(maxsize=1)
def give_up_data():
    return GiveUpData()


def table_getters(ctx, t):
    import hj3d
    lib = hj3d.lib()
    npay, nsub = C.c_uint64(), C.c_uint64()
    return {"stats": t.stats, "finish": t.finish,
            "size": lambda: ctx._check(lib.hj3d_table_size(ctx.h, t.h, None, None), "size"),
            "export": lambda: ctx._check(lib.hj3d_table_export(ctx.h, t.h, None, None, None, C.byref(npay),
                                                               C.byref(nsub)), "export")}


@pytest.mark.parametrize("first_use", ["stats", "finish", "size", "export"])
def test_nested_tables_carry_no_barrier_tag_on_a_fresh_context(first_use):
    """The first build on a fresh context is a small implicit-row nested build that gives up. The
    fused partition's first launch on a context carries tag 1, and 1 is also the give-up flag a
    nested table keeps in the same counts word: a tag recorded on the table made its first getter
    report a barrier timeout (HJ3D_EDEVICE) instead of running the sort build. Nested builds take the
    two-launch partition, so every getter as the table's first use finishes the build."""
    import hj3d
    d = give_up_data()
    c = hj3d.Context()
    try:
        c.radix_min(0)
        dR, dS = dev(d.R), dev(d.S)
        t = hj3d.Table(c, hj3d.HJ3D_NESTED, d.nb)
        t.build(hj3d.Rel(dS, 1))
        assert t.build_path(finish=False) == "nested_agg?"
        table_getters(c, t)[first_use]()
        assert t.build_path(finish=False) == "nested_sort"
        st = t.stats()
        assert {k: st[k] for k in STAT_KEYS} == {k: d.e.stats[k] for k in STAT_KEYS}
        assert t.build_path() == "nested_sort"
        r = c.probe(t, hj3d.Rel(dR, 0), unnest=True)
        assert (r.n_matched, r.n_cmps, r.n_out) == (d.e.c_probe, d.e.c_cmp, d.e.c_unnest)
        assert {"n": r.n_out, "sum_a": r.sum_a, "sum_b": r.sum_b, "sum_c": r.sum_c, "sum_h": r.sum_h,
                "xor_h": r.xor_h} == d.e.out
        for call in table_getters(c, t).values():  # (after the sort build the word holds the largest key)
            call()
        t.close()
    finally:
        c.close()


def test_barrier_diagnostic_does_not_reach_nested_builds(ctx):
    """HJ3D_OPT_DIAG_GBAR makes every fused partition's barrier time out. A nested build does not take
    the fused partition (k_nagg_order would erase the timeout word and the aggregation would consume
    partial partition sizes), so under the option a small implicit-row nested build and its probe are
    exact and every getter succeeds; a chaining build under the same option is still reported."""
    import hj3d
    d = exp1_data(20000, NESTED_WIDTHS, NESTED_GROUP.get(20000, 48))
    e = d.oracle("Nrs")
    dR, dS = dev(d.R), dev(d.S)
    with options(ctx, radix_min=0, diag_gbar=100_000):  # 1 ms
        t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, d.nb)
        got = hj3d.exp1_plan(ctx, "Nrs", dR, dS, d.nb, table=t)
        check_plan(got, e, "nested under diag_gbar")
        for call in table_getters(ctx, t).values():
            call()
        assert t.build_path().startswith("nested_agg"), t.build_path()
        t.close()
        # the chaining build: as test_fused_partition_barrier_timeout_is_reported
        tc = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, N_S)
        tc.build(hj3d.Rel(dS, 1))
        assert tc.build_path(finish=False) == "radix"
        for what, call in table_getters(ctx, tc).items():
            with pytest.raises(hj3d.Hj3dError) as ei:
                call()
            assert ei.value.status == hj3d.HJ3D_EDEVICE and "barrier" in str(ei.value), what
        with pytest.raises(hj3d.Hj3dError) as ei:
            ctx.probe(tc, hj3d.Rel(dR, 0), unique=False)
        assert ei.value.status == hj3d.HJ3D_EDEVICE
    # without the diagnostic the same table rebuilds exact and reads clean
    ec = O.chain_plan(d.S, 1, d.R, 0, N_S, False)
    with options(ctx, radix_min=0):
        got = hj3d.exp1_plan(ctx, "Crs", dR, dS, N_S, table=tc)
    check_plan(got, ec, "chaining rebuild")
    tc.close()
