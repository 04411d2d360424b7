"""Aggregation without unnesting (hj3d_group_agg + hj3d_agg_nested) against the only way without them, on
one GPU, in one process, the forms alternating (each round times every form in turn, `--reps` calls each).

1. At config E's relations (log2R = 22, alpha=3 A=4 beta=2 B=2: bench.py --workload E): COUNT(*), SUM(S.k)
   and SUM(T.k) per R tuple behind the chain probe(MAINREF) -> probe_refn.
     unnest   the only way without the operators: unnestn(EMIT) of every output row, a torch gather of the
              build words of the rows and one index_add_ per aggregate
     agg      agg_nested over the same tuples, one dense row of three values per tuple; the two group_agg
              columns it reads are timed separately (they depend on the tables only) and counted once in
              `agg_with_columns`
   The forms' outputs are checked against each other first.
2. group_agg alone on a config-C table (|S| = --rows, default 1e8; keys over --rows / 10 values): unique keys
   (|G| = 1), uniform keys (|G| about 10), Zipf 0.8 and 1.0, with hj3d_stream_copy's peak taken in the same
   run. Algorithmic bytes (4 B sub + 4 B word per row, 16 B + 24 B per key) are quoted against it, over the
   whole call (zeroing launch, two kernels).

Per form: ms per call of every round, their median and spread ((max - min) / median). The result goes to
profiles/agg_nested.json and is printed as one JSON line. The run ends itself after --timeout seconds
(default 420). --skip-chain leaves part 1 out (the class-bound sweep runs part 2 per library, HJ3D_LIB).
usage: python scripts/time_agg_nested.py [--reps N] [--rounds K] [--log2R K] [--rows N] [--skip-chain]
                                         [--timeout S] [--out FILE]"""
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-hashjoin_amd", "python"))


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


signal.alarm(arg("--timeout", 420))  # its own time limit: SIGALRM ends the process
import torch  # noqa: E402
import hj3d  # noqa: E402

reps, rounds = arg("--reps", 10), arg("--rounds", 3)
out_path = arg("--out", os.path.join(ROOT, "profiles", "agg_nested.json"), str)
ctx = hj3d.Context(0)


def timed(fn):
    torch.cuda.synchronize()
    x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    x.record()
    for _ in range(reps):
        fn()
    y.record()
    torch.cuda.synchronize()
    return x.elapsed_time(y) / reps


def alternate(forms):
    for fn in forms.values():
        fn()  # warm-up of every form (scratch sizes, code objects)
    ms = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            ms[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    return {"ms": ms, "ms_median": med, "spread": spread}


res = {"reps": reps, "rounds": rounds, "library": os.environ.get("HJ3D_LIB", "default")}

# the box's copy peak, in this run
src = torch.empty(64 << 20, dtype=torch.int32, device="cuda")
dst = torch.empty(64 << 20, dtype=torch.int32, device="cuda")
peak = ctx.stream_copy_peak(dst, src)
res["stream_copy"] = peak
del src, dst

if "--skip-chain" not in sys.argv:
    log2R, al, A, be, B = arg("--log2R", 22), 3, 4, 2, 2
    nR = 1 << log2R
    R, S, T = hj3d.exp4_relations_ref(log2R, al, A, be, B, device="cuda")
    nb = (nR >> al) + (nR >> be)
    relR, relS, relT = hj3d.Rel(R, key_word=0), hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)
    ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb), hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    ctx.build_many([ts, tt], [relS, relT])
    pairs = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
    r1 = ctx.probe(ts, relR, out=pairs, mainref=True, checksum=False)
    trip = torch.empty((max(r1.n_matched, 1), 3), dtype=torch.int32, device="cuda")
    n_trip = ctx.probe_refn(tt, relR, pairs, out=trip, checksum=False).n_out
    trip = trip[:n_trip]
    c_top = ctx.unnestn([ts, tt], trip, checksum=False)["c_top"]
    rows = torch.empty((max(c_top, 1), 3), dtype=torch.int32, device="cuda")
    col_s = torch.empty((ts.size()[1], 3), dtype=torch.int64, device="cuda")
    col_t = torch.empty((tt.size()[1], 3), dtype=torch.int64, device="cuda")
    vals = torch.empty((max(n_trip, 1), 3), dtype=torch.int64, device="cuda")
    per_r = torch.zeros((3, nR), dtype=torch.int64, device="cuda")
    ones = torch.ones(max(c_top, 1), dtype=torch.int64, device="cuda")

    def columns():
        ts.group_agg(relS, 0, signed=False, out=col_s, fetch=False)
        tt.group_agg(relT, 0, signed=False, out=col_t, fetch=False)

    def agg():
        ctx.agg_nested(trip, [ts, tt], [("count",), ("sum", 1, col_s, False), ("sum", 2, col_t, False)], out=vals, fetch=False)

    def unnest():
        ctx.unnestn([ts, tt], trip, out=rows, checksum=False, fetch=False)
        a = rows[:c_top, 0].long()
        per_r.zero_()
        per_r[0].index_add_(0, a, ones[:c_top])
        per_r[1].index_add_(0, a, S[rows[:c_top, 1].long(), 0].long())
        per_r[2].index_add_(0, a, T[rows[:c_top, 2].long(), 0].long())

    def agg_with_columns():
        columns()
        agg()

    # the forms agree: the dense rows of the tuples, scattered to their R rows, are the index_add_ sums
    columns()
    agg()
    unnest()
    ctx.sync()
    mine = torch.zeros((3, nR), dtype=torch.int64, device="cuda")
    mine[:, trip[:, 0].long()] = vals[:n_trip].t()
    assert torch.equal(mine, per_r), "agg_nested and unnestn + index_add_ disagree"
    r = ctx.agg_nested_result()
    assert r["c_top"] == c_top == int(per_r[0].sum()) and r["total"][1] == int(per_r[1].sum()), r
    m = alternate({"unnest": unnest, "agg": agg, "columns": columns, "agg_with_columns": agg_with_columns})
    med = m["ms_median"]
    m.update(config=f"E: log2R={log2R} alpha={al} A={A} beta={be} B={B}, |S|=|T|={S.shape[0]}, nb={nb}",
             tuples=n_trip, c_top=c_top, keys=[col_s.shape[0], col_t.shape[0]],
             agg_over_unnest=med["agg"] / med["unnest"],
             agg_with_columns_over_unnest=med["agg_with_columns"] / med["unnest"],
             agg_bytes=n_trip * (12 + 2 * 16 + 2 * 8 + 24))
    m["agg_GBs"] = m["agg_bytes"] / med["agg"] / 1e6
    res["chain"] = m
    del R, S, T, ts, tt, pairs, trip, rows, ones, per_r, mine, vals

# group_agg alone under skew
n = arg("--rows", 100_000_000)
dom = max(n // 10, 1)
S = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
S[:, 2] = torch.arange(n, dtype=torch.int32, device="cuda") * 40503  # the aggregated word
rel = hj3d.Rel(S, key_word=1)
res["group_agg"] = {"rows": n, "domain": dom, "keys": {}}
for name, theta in (("unique", None), ("uniform", 0.0), ("zipf0.8", 0.8), ("zipf1.0", 1.0)):
    if theta is None:
        ctx.gen_keys(S, 1, 0, n, 7)
    elif theta > 0:
        ctx.gen_zipf(S, 1, 0, dom, theta, 13)
    else:
        ctx.gen_fk(S, 1, 0, dom, 13)
    nb = n if theta is None else ctx.num_distinct(rel, dom)
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    t.build(rel)
    keys = t.size()[1]
    st = t.stats()
    col = torch.empty((keys, 3), dtype=torch.int64, device="cuda")
    _, r = t.group_agg(rel, 2, out=col)
    assert (r.n_probe, r.n_matched, r.n_out) == (keys, keys, n), r
    assert r.sum_a == int(S[:, 2].long().sum()) & hj3d.MASK64  # every row folded once
    m = alternate({"group_agg": lambda: t.group_agg(rel, 2, out=col, fetch=False)})
    algo = 8 * n + 40 * keys
    gbs = algo / m["ms_median"]["group_agg"] / 1e6
    m.update(keys=keys, path=t.build_path(), algorithmic_bytes=algo, GBs=gbs,
             fraction_of_copy_peak=gbs / peak["copy_peak_GBs"], longest_group=st.get("cc1_max"))
    res["group_agg"]["keys"][name] = m
    t.close()
    del col
g = res["group_agg"]["keys"]
res["group_agg"]["zipf1.0_over_uniform"] = g["zipf1.0"]["ms_median"]["group_agg"] / g["uniform"]["ms_median"]["group_agg"]
res["group_agg"]["zipf0.8_over_uniform"] = g["zipf0.8"]["ms_median"]["group_agg"] / g["uniform"]["ms_median"]["group_agg"]
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(res))
