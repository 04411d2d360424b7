"""hj3d_unnestn and the chain that feeds it, on one GPU, in one process, forms alternating (each round
times every form in turn, `--reps` calls each), checksum=False, at config E's R (log2R = 22, alpha=3
A=4 beta=2 B=2: the relations of bench.py --workload E):

  1  unnestn(k = 2, EMIT) against hj3d_unnest2(EMIT) on the same 8,388,608-row result's triples (the
     survivors of probe -> probe_ref): the two move the same bytes.
  2  a four-table star on R.k: tables on S.a, T.a and on S'.a, T'.a (S, T with their rows permuted), so
     a live R tuple (|S group| = 8, |T group| = 2) has (8 * 2)^2 = 256 output rows.
       chained  probe(MAINREF) -> probe_refn x 3 -> unnestn(k = 4, EMIT); the survivor counts come from
                the validation call, nothing is read back
       eager    probe(UNNEST | EMIT) on S, then level by level: the expanded pairs' keys gathered from R
                (torch), probe(UNNEST | EMIT) of the next table over {key, pair index}. It ends with the
                last level's {index, row} pairs: the existing operators do not assemble the 5-word rows.

The counters of the forms are checked against each other first. Per form: ms per call of every round,
their median and spread ((max - min) / median). The result goes to profiles/unnestn.json and is printed
as one JSON line. The run ends itself after --timeout seconds (default 420).
usage: python scripts/time_unnestn.py [--reps N] [--rounds K] [--log2R K] [--no-star] [--timeout S] [--out FILE]"""
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
out_path = arg("--out", os.path.join(ROOT, "profiles", "unnestn.json"), str)
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
    return ms, med, spread


log2R, al, A, be, B = arg("--log2R", 22), 3, 4, 2, 2
nR = 1 << log2R
R, S, T = hj3d.exp4_relations_ref(log2R, al, A, be, B, device="cuda")
nb = (nR >> al) + (nR >> be)
relR, relS, relT = hj3d.Rel(R, key_word=0), hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)
ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb), hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
ctx.build_many([ts, tt], [relS, relT])

# ---- 1. k = 2 against hj3d_unnest2 ----
pairs = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
r1 = ctx.probe(ts, relR, out=pairs, mainref=True, checksum=False)
trip = torch.empty((r1.n_matched, 3), dtype=torch.int32, device="cuda")
r2 = ctx.probe_ref(tt, relR, pairs, out=trip, checksum=False)
trip = trip[:r2.n_out]
a = ctx.unnest2(ts, tt, trip, checksum=False)
c_top = a["c_top"]
out = torch.empty((c_top, 3), dtype=torch.int32, device="cuda")
a = ctx.unnest2(ts, tt, trip, out=out, checksum=False)
b = ctx.unnestn([ts, tt], trip, out=out, checksum=False)
assert not a["overflow"] and not b["overflow"]
assert (b["c_unnest"], b["c_top"], b["sum_a"], b["sum_row"]) == \
    ([a["c_unnest_1"], a["c_unnest_2"]], a["c_top"], a["sum_a"], [a["sum_b"], a["sum_c"]]), (a, b)
ms2, med2, spread2 = alternate({
    "unnest2": lambda: ctx.unnest2(ts, tt, trip, out=out, checksum=False, fetch=False),
    "unnestn_k2": lambda: ctx.unnestn([ts, tt], trip, out=out, checksum=False, fetch=False),
})
res = {
    "config": f"E: log2R={log2R} alpha={al} A={A} beta={be} B={B}, |S|=|T|={S.shape[0]}, nb={nb}",
    "reps": reps, "rounds": rounds, "checksum": False,
    "k2": {"triples_in": int(trip.shape[0]), "c_top": c_top, "ms": ms2, "ms_median": med2, "spread": spread2,
           "unnestn_over_unnest2": med2["unnestn_k2"] / med2["unnest2"],
           "rows_per_s": {k: c_top / v * 1e3 for k, v in med2.items()}},
}
del out

# ---- 2. the four-table star ----
if "--no-star" not in sys.argv:
    g = torch.Generator(device="cuda").manual_seed(5)
    S2 = S.clone()
    T2 = T.clone()
    S2[:, 1] = S[torch.randperm(S.shape[0], device="cuda", generator=g), 1]
    T2[:, 1] = T[torch.randperm(T.shape[0], device="cuda", generator=g), 1]
    ts2, tt2 = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb), hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    ctx.build_many([ts2, tt2], [hj3d.Rel(S2, key_word=1), hj3d.Rel(T2, key_word=1)])
    tables = [ts, tt, ts2, tt2]
    plan = hj3d.star_plan_chained(ctx, R, [(S, 1), (T, 1), (S2, 1), (T2, 1)], nb, (0, 0, 0, 0), checksum=False)
    n_lvl = [nR] + plan["c_probe"]  # tuples entering each level, then the unnest
    star_top = plan["c_top"]
    # the first probe's output is dense (one slot per R tuple), the chained probes' are compact
    bufs = [torch.empty((nR if i == 0 else max(n_lvl[i + 1], 1), i + 2), dtype=torch.int32, device="cuda")
            for i in range(4)]
    wide = torch.empty((star_top, 5), dtype=torch.int32, device="cuda")

    def chained(fetch=False):
        ctx.probe(tables[0], relR, out=bufs[0], mainref=True, fetch=False, checksum=False)
        cur = bufs[0][:nR]
        for i in range(1, 4):
            ctx.probe_refn(tables[i], relR, cur, out=bufs[i], checksum=False, fetch=False)
            cur = bufs[i][:n_lvl[i + 1]]
        return ctx.unnestn(tables, cur, out=wide, checksum=False, fetch=fetch)

    # eager: the expanded pairs of every level ({index of the previous level's pair, build row})
    Rk = R[:, 0].contiguous()
    e_n = [ctx.probe(tables[0], relR, unnest=True, checksum=False).n_out]
    e_buf = [torch.empty((e_n[0], 2), dtype=torch.int32, device="cuda")]
    keyrel = []

    def eager(fetch=False, size=False):
        ctx.probe(tables[0], relR, unnest=True, out=e_buf[0], fetch=False, checksum=False)
        rrow = e_buf[0][:, 0].long()  # the R row of every pair of the current level
        r = None
        for i in range(1, 4):
            kr = torch.stack([Rk[rrow], torch.arange(rrow.shape[0], dtype=torch.int32, device="cuda")], dim=1).contiguous()
            rel = hj3d.Rel(kr, key_word=0, row_word=1)
            if size:
                e_n.append(ctx.probe(tables[i], rel, unnest=True, checksum=False).n_out)
                e_buf.append(torch.empty((e_n[i], 2), dtype=torch.int32, device="cuda"))
            r = ctx.probe(tables[i], rel, unnest=True, out=e_buf[i], fetch=fetch and i == 3, checksum=False)
            keyrel.append(kr)  # (kept alive until the stream has used it)
            del keyrel[:-4]
            rrow = rrow[e_buf[i][:, 0].long()]
        return r

    ee = eager(True, size=True)
    cc = chained(True)
    assert not cc["overflow"] and cc["c_top"] == star_top == ee.n_out == e_n[3], (cc, ee, e_n)
    msS, medS, spreadS = alternate({"chained": chained, "eager": eager})
    res["star4"] = {"tables": "S.a, T.a, S'.a, T'.a on R.k", "tuples_per_level": n_lvl, "c_top": star_top,
                    "c_unnest": cc["c_unnest"], "eager_pairs_per_level": e_n, "ms": msS, "ms_median": medS,
                    "spread": spreadS, "chained_over_eager": medS["chained"] / medS["eager"],
                    "rows_per_s": {k: star_top / v * 1e3 for k, v in medS.items()}}
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(res))
