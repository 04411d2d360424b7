"""The data and the CPU references of the stream-ordering cases (a helper module for
tests/test_gpu_streams.py and tests/test_stream_order_ref.py, not a conftest). Host only: numpy and
the oracle.

Every case has one or more *late* inputs. A late input exists twice: the real data, from which the
expected result is computed here, and a decoy of the same shape that the library must never see. The
decoy of a relation carries the real keys plus SHIFT (outside every key domain used here, so a join
over it matches nothing and its buckets are others); the decoy of a build relation folds the keys onto
64 keys from SHIFT on, so the table built from it has other statistics; the decoy of stored nested
tuples has every ref dead; the decoy of an aggregate column is the column plus a constant.

The probe world is that of tests/test_gpu_probe_api.py (3001 / 5003 / 4001 tuples, `big_chain`,
`big_nested`): world() redraws it from the same seeds, and the GPU module asserts that its device
relations equal these arrays before it trusts an expectation computed from them."""
import functools
from types import SimpleNamespace

import numpy as np

import agg_nested_ref as AN
import expand_n_ref as XN
import expand_ref as X
import oracle as O
import select_nested_ref as SN
import tablestruct as TS

SHIFT = 1 << 24
NOREF = 0xFFFFFFFF
PREDS = [(0, "<", 2000)]  # test_gpu_probe_api.make_world's selection
CHAIN, NESTED = TS.CHAIN, TS.NESTED


def rows3(c0, c1):
    t = np.zeros((len(c0), 3), dtype=np.uint32)
    t[:, 0] = c0
    t[:, 1] = c1
    return t


# ---- decoys ----
def decoy_rel(tuples, key_word):
    """A probe-side (or exchanged) relation: every key plus SHIFT."""
    d = np.array(tuples, dtype=np.uint32, copy=True)
    d[:, key_word] += np.uint32(SHIFT)
    return d


def decoy_build(tuples, key_word):
    """A build relation: 64 keys from SHIFT on (key mod 64): few distinct keys in long groups."""
    d = np.array(tuples, dtype=np.uint32, copy=True)
    d[:, key_word] = np.uint32(SHIFT) + d[:, key_word] % np.uint32(64)
    return d


def decoy_nested(tuples):
    """Stored nested tuples {a, ref ..}: a moved on by one, every ref dead."""
    d = np.array(tuples, dtype=np.uint32, copy=True)
    d[:, 0] = np.roll(d[:, 0], 1)
    d[:, 1:] = NOREF
    return d


def decoy_column(col):
    """A group_agg column (n_mains, 3) of 64-bit words: every word plus 12345."""
    with np.errstate(over="ignore"):
        return np.asarray(col, dtype=np.uint64) + np.uint64(12345)


# ---- the probe world ----
@functools.lru_cache(maxsize=None)
def world():
    rng = np.random.default_rng(2024)
    nR, nS, nT, dom = 3001, 5003, 4001, 3300
    Rk = rng.permutation(nR).astype(np.uint32)
    Sa = rng.integers(0, dom, nS).astype(np.uint32)
    Ta = rng.integers(0, dom, nT).astype(np.uint32)
    Sa[rng.choice(nS, 300, replace=False)] = 77
    Ta[rng.choice(nT, 200, replace=False)] = 77
    return SimpleNamespace(R=rows3(Rk, np.zeros(nR)), S=rows3(np.arange(nS), Sa), T=rows3(np.arange(nT), Ta))


@functools.lru_cache(maxsize=None)
def big_chain():
    rng = np.random.default_rng(5)
    n = 1 << 17
    return SimpleNamespace(R=rows3(rng.permutation(n), np.zeros(n)), S=rows3(np.arange(2 * n), rng.integers(0, n + 1000, 2 * n)))


@functools.lru_cache(maxsize=None)
def big_nested():
    rng = np.random.default_rng(6)
    nR, nS = 100_000, 200_000
    return SimpleNamespace(R=rows3(rng.permutation(nR), np.zeros(nR)), S=rows3(np.arange(nS), rng.integers(0, nR, nS)))


ZIPF = "exp1_R131072_S1048576_zipf1"  # tests/test_gpu_pk_levels.py's region-overflow shape


@functools.lru_cache(maxsize=None)
def zipf():
    """(R, S, NB of the Csr table) of the Zipf(1) fixture."""
    from conftest import load_golden
    g = dict(load_golden("exp1_*.json", headline=False))[ZIPF]
    _, nR, nS, skew, theta, t, b = g["generator_args"][:7]
    Rk, Sa, _ = O.gen_exp1(nR, nS, bool(skew), theta, t)
    return SimpleNamespace(R=O.tuples3(Rk, np.zeros_like(Rk)), S=O.tuples3(np.arange(nS, dtype=np.uint32), Sa),
                           nb=max(nR // b, 1))


# A probe case: the table (kind, build relation with key / row words, buckets), the late probe relation
# (key / row words) and the call's form. `world`: which of the functions above holds the arrays.
def _p(world, kind, build, bkey, brow, nb, probe, pkey, prow, **form):
    return dict(world=world, kind=kind, build=build, bkey=bkey, brow=brow, nb=nb, probe=probe, pkey=pkey, prow=prow,
                form=form)


_cS = ("world", CHAIN, "S", 1, 0, 2053, "R", 0, None)    # R probes the chaining table on S.a
_cR = ("world", CHAIN, "R", 0, None, 2053, "S", 1, 0)    # S probes the chaining table on R.k
_nS = ("world", NESTED, "S", 1, 0, 1500, "R", 0, None)   # R probes the nested table on S.a
_bigc = ("big_chain", CHAIN, "R", 0, None, 1 << 17, "S", 1, 0)
_bign = ("big_nested", NESTED, "S", 1, None, 200_000, "R", 0, None)
_zipf = ("zipf", CHAIN, "R", 0, None, None, "S", 1, 0)
PART = dict(radix_min=64)
NESTED_MODES = {"agg": {}, "dense": dict(emit=True), "denseref": dict(emit=True, mainref=True),
                "aggun": dict(unnest=True), "countun": dict(unnest=True, emit=True)}

PROBES = {}
for _path, _o in (("direct", {}), ("part", dict(PART, packed=False))):
    PROBES[f"chain_{_path}_count"] = _p(*_cS, opts=_o)
    PROBES[f"chain_{_path}_unique_dense"] = _p(*_cR, unique=True, emit=True, opts=_o)
    PROBES[f"chain_{_path}_nonunique_emit"] = _p(*_cS, emit=True, opts=_o)
PROBES["packed_one_level"] = _p(*_cR, unique=True, emit=True, opts=dict(PART, slice_max=512))
PROBES["packed_refused"] = _p(*_cR, unique=True, emit=True, opts=PART)
PROBES["packed_two_levels"] = _p(*_bigc, unique=True, emit=True, opts=dict(radix_min=64, slice_max=16))
for _mode, _kw in NESTED_MODES.items():
    PROBES[f"nested_direct_{_mode}"] = _p(*_nS, opts={}, **_kw)
    PROBES[f"nested_part_{_mode}"] = _p(*_nS, opts=PART, **_kw)
PROBES["nested_pk_slices_dense"] = _p(*_bign, emit=True, opts=dict(radix_min=64, slice_max=64))
PROBES["nested_pk_slices_countun"] = _p(*_bign, unnest=True, emit=True, opts=dict(radix_min=64, slice_max=64))
PROBES["sel_fused_packed"] = _p(*_cR[:6], "R", 0, None, unique=True, sel=True, opts=dict(PART, slice_max=512))
PROBES["sel_fused_chain"] = _p(*_cS, sel=True, opts=PART)
PROBES["sel_fused_nested"] = _p(*_nS, sel=True, opts=PART)
PROBES["sel_unfused_chain"] = _p(*_cS, sel=True, opts=dict(radix_min=64, unfused=True))
PROBES["sel_unfused_nested"] = _p(*_nS, sel=True, opts=dict(radix_min=64, unfused=True))
PROBES["sel_accumulate_chain"] = _p(*_cS, sel=True, accumulate=True, opts=PART)
PROBES["sel_accumulate_nested"] = _p(*_nS, sel=True, accumulate=True, opts=PART)
# the overflow list of the packed probe walked (not keyed in EXPECTED_LAUNCHES: its launches follow the data)
PROBES["packed_zipf_overflow"] = _p(*_zipf, unique=True, emit=True, opts=dict(radix_min=0, slice_max=16))

# hj3d_probe2: (world tables' kind, buckets, EMIT, options)
PROBE2 = {}
for _emit in (False, True):
    _e = "_emit" if _emit else ""
    PROBE2[f"probe2_nested_part{_e}"] = dict(kind=NESTED, nb=1500, emit=_emit, opts=PART)
    PROBE2[f"probe2_nested_direct{_e}"] = dict(kind=NESTED, nb=1500, emit=_emit, opts={})
    PROBE2[f"probe2_chain{_e}"] = dict(kind=CHAIN, nb=2053, emit=_emit, opts=PART)

WORLDS = {"world": world, "big_chain": big_chain, "big_nested": big_nested, "zipf": zipf}


def probe_arrays(case):
    """(build relation, late probe relation, buckets) of a probe case."""
    w = WORLDS[case["world"]]()
    return getattr(w, case["build"]), getattr(w, case["probe"]), (case["nb"] if case["nb"] else w.nb)


def probe_expected(case, probe):
    """hj3d_probe_res's fields the oracle fixes, for `probe` in place of the case's probe relation."""
    build, _, nb = probe_arrays(case)
    f = case["form"]
    pkey, prow = case["pkey"], case["prow"]
    if f.get("sel"):  # scan -> selection -> probe: the passing tuples with their rows (hj3d_probe_sel)
        probe, pkey, prow = O.select(probe, pkey, PREDS), 0, 1
    plan = O.chain_plan if case["kind"] == CHAIN else O.nested_plan
    flag = bool(f.get("unique")) if case["kind"] == CHAIN else bool(f.get("unnest"))
    if len(probe) == 0:
        probe = np.zeros((0, 3), np.uint32)
    e = plan(build, case["bkey"], probe, pkey, nb, flag, brow=case["brow"], prow=prow)
    out = {"n_probe": len(probe), "n_cmps": e.c_cmp, "n_out": e.out["n"]}
    if not f.get("mainref"):  # (the checksums of a MAINREF probe fold main refs: the table's layout)
        out.update({k: e.out[k] for k in ("sum_a", "sum_b", "sum_h", "xor_h")})
    if case["kind"] == NESTED:
        out["n_matched"] = e.c_probe
    return out, e.out


EXP4_FIELDS = ("c_probe_rs", "c_probe_rs_cmp", "c_probe_rt", "c_probe_rt_cmp", "c_unnest_1", "c_unnest_2", "c_top")


def probe2_expected(case, R):
    w = world()
    e = O.exp4_plan(R, w.S, w.T, case["nb"], case["kind"] == NESTED, keys=(0, 1, 1), rows=(None, 0, 0))
    out = {k: e[k] for k in EXP4_FIELDS}
    out.update({k: e["out"][k] for k in ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")})
    return out


# ---- builds: tests/test_gpu_table_lifecycle.py's selections, at tablestruct's shapes ----
def build_tuples(shape):
    """The build relation {0, key, row} of test_gpu_table_lifecycle.Data (key word 1, implicit rows)."""
    _, keys, _ = TS.shape(shape)
    t = np.zeros((len(keys), 3), np.uint32)
    t[:, 1] = keys
    t[:, 2] = np.arange(len(keys))
    return t


def build_stats(shape, tuples):
    kind, _, nb = TS.shape(shape)
    rows = np.arange(len(tuples), dtype=np.uint32)
    return (TS.chain_stats if kind == CHAIN else TS.nested_stats)(tuples[:, 1], rows, nb)


# ---- operators over stored nested tuples, on the probe world's nested tables ----
# the other forms of hj3d_unnest / hj3d_unnest2 that test_gpu_probe_api.EXPECTED_LAUNCHES keys ("unnest" and
# "unnest2" below are its unnest_ck_emit and unnest2_emit): name -> (operator, checksum, EMIT, its key there)
UNNEST_FORMS = {"unnest_count": ("unnest", False, False, "unnest"), "unnest_ck": ("unnest", True, False, "unnest_ck"),
                "unnest_emit": ("unnest", False, True, "unnest_emit"), "unnest2_count": ("unnest2", True, False, "unnest2")}
OPERATORS = ("unnest", "unnest2", "unnestn", "probe_ref", "probe_refn", "select_nested", "agg_nested", "group_agg",
             *UNNEST_FORMS)
NSEL_PREDS = [("base", 0, "<", 2000), ("count", 1, ">=", 2)]
AGG_WORD = 0  # the word of S hj3d_group_agg folds (its row ids), signed


def key_of(R, a, ref):
    """The key a live stored tuple carries for a table built on a relation that references R.k: that of
    base row a; None where the ref is dead."""
    k = R[a, 0].astype(np.int64)
    return np.where(ref != NOREF, k, -1)


def model_refs(col, keys):
    """Main refs into agg_nested_ref.table_arrays(col)'s layout for per-tuple keys (negative: dead)."""
    _, _, ref_of = AN.table_arrays(col)
    return np.array([ref_of.get(int(k), NOREF) if k >= 0 else NOREF for k in keys], dtype=np.uint32)


def model_tuples():
    """The world's stored nested tuples on numpy-laid tables (what the CPU test uses; the GPU module
    takes the library's own refs and main records): pairs {a, ref_s}, triples {a, ref_s, ref_t}."""
    w = world()
    a = np.arange(len(w.R), dtype=np.uint32)
    k = w.R[:, 0].astype(np.int64)
    rs, rt = model_refs(w.S[:, 1], k), model_refs(w.T[:, 1], k)
    return np.stack([a, rs], 1), np.stack([a, rs, rt], 1), AN.table_arrays(w.S[:, 1])[:2], AN.table_arrays(w.T[:, 1])[:2]


def wide_tuples(trip):
    """unnestn's k = 3 input {a, ref_s, ref_t, ref_s} over (S, T, S); the tuple of the hot key (300 x 200
    x 300 rows) is made dead so that the output stays small enough to compare row by row."""
    w = world()
    t = np.concatenate([trip, trip[:, 1:2]], axis=1).astype(np.uint32)
    t[w.R[t[:, 0], 0] == 77, 3] = NOREF
    return t


def operator_expected(op, R, S, nested, mains_s=None, mains_t=None, sub_s=None, col_s=None, col_t=None):
    """What operator `op` must report for the late inputs R (base relation), S (group_agg's build
    relation), `nested` (stored tuples) and the aggregate columns; mains_* / sub_s: the tables' main
    records and row array (any layout). Returns (counters, rows or None)."""
    if op in UNNEST_FORMS:  # the same operator without the hashes (sum_h = xor_h = 0) and / or without output rows
        base_op, checksum, emit, _ = UNNEST_FORMS[op]
        c, rows = operator_expected(base_op, R, S, nested)
        if not checksum:
            c["sum_h"] = c["xor_h"] = 0
        return c, (rows if emit else None)
    w = world()
    Sa, Ta = w.S[:, 1], w.T[:, 1]
    a = nested[:, 0] if nested is not None else None
    inside = (a < len(R)) if a is not None else None
    if op == "unnest":
        ks = key_of(w.R, a, nested[:, 1])  # (unnest reads the table, not the base relation)
        rows = X.expand_pairs(a, ks, Sa)
        c = dict(X.pair_counters(a, ks, Sa), **{k: v for k, v in X.pair_checksums(rows).items() if k not in ("n", "sum_c")})
        return c, rows
    if op == "unnest2":
        ks, kt = key_of(w.R, a, nested[:, 1]), key_of(w.R, a, nested[:, 2])
        rows = X.expand_triples(a, ks, kt, Sa, Ta)
        c = dict(X.triple_counters(ks, kt, Sa, Ta), **{k: v for k, v in X.triple_checksums(rows).items() if k != "n"})
        return c, rows
    if op == "unnestn":
        ks = [key_of(w.R, a, nested[:, 1]), key_of(w.R, a, nested[:, 2]), key_of(w.R, a, nested[:, 3])]
        rows = XN.expand_rows(a, ks, [Sa, Ta, Sa])
        c = dict(XN.counters(ks, [Sa, Ta, Sa]), **{k: v for k, v in XN.row_checksums(rows).items() if k != "n"})
        return c, rows
    if op in ("probe_ref", "probe_refn"):
        # the live tuples probe the other table with the key word of base row a
        live = inside & (nested[:, 1:] != NOREF).all(axis=1)
        build, nb = (w.T, 1500) if op == "probe_ref" else (w.S, 1500)
        P = R[a[live]] if live.any() else np.zeros((0, 3), np.uint32)
        e = O.nested_plan(build, 1, P, 0, nb, False, brow=0)
        hit = np.isin(P[:, 0], build[:, 1])
        c = {"n_probe": int(live.sum()), "n_matched": e.c_probe, "n_out": e.c_probe, "n_cmps": e.c_cmp,
             "sum_a": int(a[live][hit].sum(dtype=np.uint64))}
        return c, nested[live][hit]  # (the caller appends the matched main ref)
    if op == "select_nested":
        m = SN.select_nested(nested, NSEL_PREDS, base=R, mains=[mains_s, mains_t])
        return {k: m[k] for k in SN.COUNTERS}, m["rows"]
    if op == "agg_nested":
        specs = [("count",), ("sum", 1, col_s), ("min", 2, col_t), ("max", 1, col_s)]
        m = AN.agg_nested(nested, [mains_s, mains_t], specs)
        return {k: m[k] for k in ("n_in", "n_live", "c_top", "total")}, m["rows"]
    if op == "group_agg":
        m = AN.group_agg(mains_s, sub_s, S, AGG_WORD, True)
        return {k: m[k] for k in ("n_probe", "n_matched", "n_out", "sum_a")}, m["col"]
    raise KeyError(op)


# ---- exchange helpers: 2^16 tuples {row, key, 0} ----
X_N, X_NB, X_PARTS, X_DOMAIN = 1 << 16, 100_003, 8, 1 << 20
X_PREDS = [(1, "<", 1 << 19)]


@functools.lru_cache(maxsize=None)
def xrel():
    rng = np.random.default_rng(77)
    return rows3(np.arange(X_N), rng.integers(0, X_DOMAIN, X_N))


def part_bounds(nb, parts):
    """hj3d_part_range's first buckets: part p owns [ceil(p * nb / parts), ceil((p + 1) * nb / parts))."""
    return [(nb * p + parts - 1) // parts for p in range(parts + 1)]


def partition_expected(rel, preds=None):
    """(counts per destination, the stable (key, row) pairs grouped by destination) of hj3d_partition."""
    pairs = O.select(rel, 1, preds or [])
    b = TS.fmix32(pairs[:, 0]).astype(np.uint64) % np.uint64(X_NB)
    dest = np.searchsorted(np.array(part_bounds(X_NB, X_PARTS)[1:], dtype=np.uint64), b, side="right")
    order = np.argsort(dest, kind="stable")
    return np.bincount(dest, minlength=X_PARTS).tolist(), pairs[order]


def bitmap_expected(rel):
    """(bitmap words, keys outside the domain, distinct keys inside) of hj3d_key_bitmap / _or_popcount."""
    k = rel[:, 1].astype(np.int64)
    ins = k[k < X_DOMAIN]
    bm = np.zeros((X_DOMAIN + 31) // 32, np.uint32)
    np.bitwise_or.at(bm, ins >> 5, (np.uint32(1) << (ins & 31).astype(np.uint32)))
    return bm, int((k >= X_DOMAIN).sum()), len(np.unique(ins))


# ---- the ticketed exchange: the (key, row) pairs of xrel() sent to this rank itself, then probed ----
X_TABLE_N, X_TABLE_NB = 8192, 4099


def comm_case():
    """(the late send buffer: (key, row) pairs, the build relation of the chaining table they probe)."""
    return O.select(xrel(), 1, []), xrel()[:X_TABLE_N]


def comm_expected(pairs):
    """hj3d_probe_res's fields for the received `pairs` probing the table on comm_case()'s build relation."""
    _, B = comm_case()
    e = O.chain_plan(B, 1, pairs, 0, X_TABLE_NB, False, brow=0, prow=1)
    return {"n_probe": len(pairs), "n_out": e.out["n"], "n_cmps": e.c_cmp, "sum_a": e.out["sum_a"], "sum_b": e.out["sum_b"],
            "sum_h": e.out["sum_h"], "xor_h": e.out["xor_h"]}


# ---- two contexts at once: A = chaining radix build + packed EMIT probe, B = nested_agg build + unnest EMIT probe ----
TWO_NA, TWO_NB_B, TWO_ROUNDS = 1 << 16, 20_000, 4  # (round 0 is the warm-up)


@functools.lru_cache(maxsize=None)
def two_ctx_round(rnd):
    """The four relations of a round, each with its decoy: RA (A's build, unique keys), SA (A's probe), SB (B's
    build: tablestruct's "nested" shape), RB (B's probe)."""
    rng = np.random.default_rng(900 + rnd)
    nA = TWO_NA
    RA = rows3(rng.permutation(nA), np.zeros(nA))
    SA = rows3(np.arange(2 * nA), rng.integers(0, nA + 500, 2 * nA))
    SB = rows3(np.arange(400_000), rng.integers(0, 100_000, 400_000))
    RB = rows3(rng.permutation(100_500), np.zeros(100_500))
    return SimpleNamespace(real=[RA, SA, SB, RB],
                           decoy=[decoy_build(RA, 0), decoy_rel(SA, 1), decoy_build(SB, 1), decoy_rel(RB, 0)])


def two_ctx_expected(RA, SA, SB, RB):
    """(A's probe, B's probe) as the oracle's plan results, for these relations in place of a round's."""
    return (O.chain_plan(RA, 0, SA, 1, TWO_NA, True, prow=0), O.nested_plan(SB, 1, RB, 0, TWO_NB_B, True, brow=0))


def two_ctx_stats(RA, SB):
    """HtStatistics of A's chaining and B's nested table."""
    return (TS.chain_stats(RA[:, 0], np.arange(len(RA), dtype=np.uint32), TWO_NA),
            TS.nested_stats(SB[:, 1], SB[:, 0], TWO_NB_B))
