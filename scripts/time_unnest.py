"""Deferred unnesting as separate operators against the fused strands, on one GPU, in one process and
alternating (round k times the fused form, then the split form, `--reps` calls each):

  config C (|R| = 1e7, |S| = 1e8, S.a ~ Zipf(0.8), plan Nrs: the relations of bench.py --workload C)
    fused  hj3d_probe(UNNEST | EMIT)
    split  hj3d_probe(MAINREF | EMIT) into |R| nested tuples, then hj3d_unnest(EMIT)
  config E (log2R = 22, alpha=3 A=4 beta=2 B=2: the relations of bench.py --workload E)
    fused  hj3d_probe2(EMIT)
    split  two hj3d_probe(MAINREF | EMIT), a torch combine of their outputs by probe row into
           {r, ref_s, ref_t} triples, then hj3d_unnest2(EMIT)

checksum=False everywhere; the split forms' counters are checked against the fused forms' first. Per
form: ms per call of every round, their median, and the split / fused ratio. The result goes to
profiles/unnest_split.json and is printed as one JSON line. The run ends itself after --timeout
seconds (default 420).
usage: python scripts/time_unnest.py [--reps N] [--rounds K] [--nR N --nS N] [--log2R K] [--only C|E]
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
only = arg("--only", "", str)
out_path = arg("--out", os.path.join(ROOT, "profiles", "unnest_split.json"), str)
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


def alternate(fused, split):
    fused()
    split()  # warm-up of both forms (scratch sizes, code objects)
    f, s = [], []
    for _ in range(rounds):
        f.append(timed(fused))
        s.append(timed(split))
    mf, ms = statistics.median(f), statistics.median(s)
    return {"fused_ms": f, "split_ms": s, "fused_ms_median": mf, "split_ms_median": ms, "split_over_fused": ms / mf}


res = {"reps": reps, "rounds": rounds, "checksum": False}

if only in ("", "C"):
    nR, nS, theta = arg("--nR", 10_000_000), arg("--nS", 100_000_000), 0.8
    R, S = hj3d.exp1_relations_ref(nR, nS, True, theta, 0, device="cuda")
    relR, relS = hj3d.Rel(R, key_word=0), hj3d.Rel(S, key_word=1)
    dv = ctx.num_distinct(relS, nR)
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, dv)
    t.reserve(nS)
    t.build(relS)
    t.finish()
    out = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
    nested = torch.empty((nR, 2), dtype=torch.int32, device="cuda")

    def fused_c(fetch=False):
        return ctx.probe(t, relR, unnest=True, out=out, fetch=fetch, checksum=False)

    def split_c(fetch=False):
        ctx.probe(t, relR, out=nested, mainref=True, fetch=False, checksum=False)
        return ctx.unnest(t, nested, out=out, fetch=fetch, checksum=False)

    a, b = fused_c(True), split_c(True)
    assert not a.overflow and not b.overflow and (a.n_out, a.n_matched) == (b.n_out, b.n_matched), (a, b)
    c = alternate(fused_c, split_c)
    c.update({"config": f"C: |R|={nR} |S|={nS} S.a~Zipf({theta}), nb={dv}, plan Nrs", "n_out": a.n_out,
              "nested_bytes_per_probe_tuple": 8,
              "fused_out_tuples_per_s": a.n_out / (c["fused_ms_median"] * 1e-3),
              "split_out_tuples_per_s": a.n_out / (c["split_ms_median"] * 1e-3)})
    res["C"] = c
    del out, nested, R, S
    t.close()
    torch.cuda.empty_cache()

if only in ("", "E"):
    log2R, al, A, be, B = arg("--log2R", 22), 3, 4, 2, 2
    nR = 1 << log2R
    R, S, T = hj3d.exp4_relations_ref(log2R, al, A, be, B, device="cuda")
    nb = (nR >> al) + (nR >> be)
    relR, relS, relT = hj3d.Rel(R, key_word=0), hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)
    ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb), hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
    ts.reserve(S.shape[0])
    tt.reserve(T.shape[0])
    ctx.build_many([ts, tt], [relS, relT])
    n = ctx.probe2(ts, tt, relR, checksum=False)["c_top"]
    out = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    ns_, nt_ = (torch.empty((nR, 2), dtype=torch.int32, device="cuda") for _ in range(2))
    trip = torch.empty((nR, 3), dtype=torch.int32, device="cuda")
    rows = torch.arange(nR, dtype=torch.int32, device="cuda")

    def fused_e(fetch=False):
        return ctx.probe2(ts, tt, relR, fetch=fetch, checksum=False, out=out)

    def split_e(fetch=False):
        ctx.probe(ts, relR, out=ns_, mainref=True, fetch=False, checksum=False)
        ctx.probe(tt, relR, out=nt_, mainref=True, fetch=False, checksum=False)
        # the combine: both outputs ordered by probe row (a scatter each), side by side
        trip[:, 0] = rows
        trip[ns_[:, 0].long(), 1] = ns_[:, 1]
        trip[nt_[:, 0].long(), 2] = nt_[:, 1]
        return ctx.unnest2(ts, tt, trip, out=out, fetch=fetch, checksum=False)

    a, b = fused_e(True), split_e(True)
    keys = ("c_top", "c_unnest_1", "c_unnest_2", "sum_a", "sum_b", "sum_c")
    assert not a["overflow"] and not b["overflow"] and all(a[k] == b[k] for k in keys), (a, b)
    e = alternate(fused_e, split_e)
    # the split form's parts, each alone
    e["split_parts_ms"] = {
        "two_mainref_probes": timed(lambda: (ctx.probe(ts, relR, out=ns_, mainref=True, fetch=False, checksum=False),
                                             ctx.probe(tt, relR, out=nt_, mainref=True, fetch=False, checksum=False))),
        "unnest2": timed(lambda: ctx.unnest2(ts, tt, trip, out=out, fetch=False, checksum=False)),
    }
    e.update({"config": f"E: log2R={log2R} alpha={al} A={A} beta={be} B={B}, |S|=|T|={S.shape[0]}, nb={nb}, plan Ndu",
              "c_top": n, "fused_triples_per_s": n / (e["fused_ms_median"] * 1e-3),
              "split_triples_per_s": n / (e["split_ms_median"] * 1e-3)})
    res["E"] = e
    ts.close()
    tt.close()

ctx.close()
doc = {}
if os.path.exists(out_path):
    with open(out_path) as fh:
        doc = json.load(fh)
doc.update(res)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(doc, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(res))
