"""hj3d_agg_grouped at config-C size on one GPU: the dense MAINREF output of a nested probe (|R| = 1e7 build,
|S| = 1e8 probing; one tuple {s_row, ref} per S row) grouped by the build key, for S.a uniform, Zipf 0.8 and
Zipf 1.1 over R's keys and for a small domain of 4096 groups; nspec = 1 (COUNT) and nspec = 4 (COUNT, SUM of a
base word, MIN and MAX of a build word). Timed: every forced kernel form, the automatic choice, and the
baseline a plan had before the operator: agg_nested(out=rows), the ref column pulled apart in torch, one
index_add_ / scatter_reduce_ per aggregate into a pre-initialised column (SUM of a base word: gathered and
weighted in torch, since no operator reads it). Each run is timed by its own pair of events on the context's
stream; medians are reported. The automatic column is compared with the baseline's. Prints one JSON line per
(distribution, nspec).
Algorithmic bytes per tuple: 8 read, 16 per live ref (its main record), 4 / 8 per gathered word, and 8 nspec of
64-bit atomics where a tuple misses the workgroup's LDS state.
usage: python scripts/time_agg_grouped.py [--reps N] [--n-probe N] [--n-build N] [--dists a,b] [--forms 1,2,3,0]
       [--no-baseline] [--tag NAME]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-hashjoin_amd", "python"))
import torch  # noqa: E402
import hj3d  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


reps = int(arg("--reps", 20))
nR, nS = int(arg("--n-build", 10_000_000)), int(arg("--n-probe", 100_000_000))
dists = arg("--dists", "uniform,zipf0.8,zipf1.1,small4096").split(",")
forms = [int(f) for f in arg("--forms", "1,2,3,0").split(",")]
baseline = "--no-baseline" not in sys.argv
tag = arg("--tag", "default")
SMALL = 4096
FORM_NAME = {0: "auto", 1: "direct", 2: "lds_column", 3: "lds_cache"}

ctx = hj3d.Context(0)
R = torch.zeros((nR, 3), dtype=torch.int32, device="cuda")
S = torch.zeros((nS, 3), dtype=torch.int32, device="cuda")
ctx.gen_keys(R, 0, 0, nR, 11)
ctx.gen_fk(R, 2, 0, 1 << 20, 3)   # R.b: the build word MIN / MAX fold
ctx.gen_keys(S, 0, 0, 0, 0)
ctx.gen_fk(S, 2, 0, 100, 5)       # S.b: the base word SUM folds
dense = torch.empty((nS, 2), dtype=torch.int32, device="cuda")
srel = hj3d.Rel(S, 1)


def timed(fn):
    """Median and spread (ms) of `reps` runs, each between its own events, after two warm-up runs."""
    fn()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def table_for(dist):
    """(the nested table, its build relation, main records) and S.a drawn for `dist`."""
    if dist == "small4096":  # a build relation of its own: SMALL keys, a permutation of [0, SMALL)
        keys = SMALL
        rel = torch.zeros((SMALL, 3), dtype=torch.int32, device="cuda")
        ctx.gen_keys(rel, 0, 0, SMALL, 11)
        ctx.gen_fk(rel, 2, 0, 1 << 20, 3)
        ctx.gen_fk(S, 1, 0, SMALL, 7)
    else:
        rel, keys = R, nR
        if dist == "uniform":
            ctx.gen_fk(S, 1, 0, nR, 7)
        else:
            ctx.gen_zipf(S, 1, 0, nR, float(dist[4:]), 7)
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, keys)
    t.build(hj3d.Rel(rel, 0))
    return t, rel, t.size()[1]


for dist in dists:
    tab, brel, m = table_for(dist)
    pr = ctx.probe(tab, srel, out=dense, mainref=True, checksum=False)
    gcol, _ = tab.group_agg(hj3d.Rel(brel, 0), 2, True)
    for nspec in (1, 4):
        specs = [("count",)] if nspec == 1 else [("count",), ("sum", "base", 2, True), ("min", 1, gcol), ("max", 1, gcol)]
        col = torch.empty((m, nspec), dtype=torch.int64, device="cuda")
        line = {"tag": tag, "dist": dist, "nspec": nspec, "n": nS, "n_live": pr.n_matched, "groups": m, "reps": reps,
                "lib": os.path.basename(os.path.dirname(hj3d.LIB_PATH)), "forms": {}}
        for f in forms:
            ctx.gby_form(f)
            med, lo, hi = timed(lambda: ctx.agg_grouped(dense, [tab], 1, specs, base=srel, out=col, fetch=False))
            line["forms"][FORM_NAME[f]] = {"ms": med, "min_ms": lo, "max_ms": hi, "tuples_per_s": nS / (med * 1e-3),
                                           "atomic_bytes_per_s_if_direct": 8 * nspec * pr.n_matched / (med * 1e-3)}
        ctx.gby_form(0)
        _, r = ctx.agg_grouped(dense, [tab], 1, specs, base=srel, out=col)
        line["c_top"] = r["c_top"]
        if baseline:
            nested_specs = [sp for sp in specs if sp[0] == "count" or sp[1] != "base"]
            rows = torch.empty((nS, len(nested_specs)), dtype=torch.int64, device="cuda")
            bcol = torch.empty((m + 1, nspec), dtype=torch.int64, device="cuda")  # row m: the dead tuples' sink
            I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)

            def base_run():
                ctx.agg_nested(dense, [tab], nested_specs, out=rows, fetch=False)
                ref = dense[:, 1].long()
                idx = torch.where(ref < 0, m, ref)  # 0xFFFFFFFF: no partner
                bcol[:, 0] = 0
                bcol[:, 0].index_add_(0, idx, rows[:, 0])
                if nspec == 4:
                    bcol[:, 1] = 0
                    bcol[:, 1].index_add_(0, idx, S[dense[:, 0].long(), 2].long() * rows[:, 0])  # (tuple i is S row a_i)
                    bcol[:, 2] = I64_MAX
                    bcol[:, 2].scatter_reduce_(0, idx, rows[:, 1], "amin", include_self=True)
                    bcol[:, 3] = I64_MIN
                    bcol[:, 3].scatter_reduce_(0, idx, rows[:, 2], "amax", include_self=True)
            med, lo, hi = timed(base_run)
            line["baseline"] = {"ms": med, "min_ms": lo, "max_ms": hi, "tuples_per_s": nS / (med * 1e-3)}
            line["equal_to_baseline"] = bool(torch.equal(col, bcol[:m]))
            del rows, bcol
        print(json.dumps(line), flush=True)
    tab.close()
