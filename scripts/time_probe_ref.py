"""The chained nested probe (hj3d_probe_ref) against the two other forms of experiment 4's Ndu probe
strand, on one GPU, in one process and alternating (each round times form a, then b, then c, `--reps`
calls each), at config E (log2R = 22, alpha=3 A=4 beta=2 B=2: the relations of bench.py --workload E):

  a  fused    hj3d_probe2(EMIT)
  b  split    two hj3d_probe(MAINREF | EMIT) of all of R, a torch combine of their outputs by probe row
              into {r, ref_s, ref_t} triples, then hj3d_unnest2(EMIT)
  c  chained  hj3d_probe(MAINREF | EMIT), hj3d_probe_ref(EMIT) over its dense output, then
              hj3d_unnest2(EMIT) of the survivors; the survivor count is read from probe_ref's result
              (one synchronisation per call, as a plan needs it). c_known: the same with the count
              taken from the validation call, nothing read back.

checksum=False everywhere; the forms' counters are checked against each other first. Per form: ms per
call of every round and their median; hj3d_probe_ref alone as well. The result goes to
profiles/probe_ref.json and is printed as one JSON line. The run ends itself after --timeout seconds
(default 420).
usage: python scripts/time_probe_ref.py [--reps N] [--rounds K] [--log2R K] [--timeout S] [--out FILE]"""
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
out_path = arg("--out", os.path.join(ROOT, "profiles", "probe_ref.json"), str)
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


log2R, al, A, be, B = arg("--log2R", 22), 3, 4, 2, 2
nR = 1 << log2R
R, S, T = hj3d.exp4_relations_ref(log2R, al, A, be, B, device="cuda")
nb = (nR >> al) + (nR >> be)
relR, relS, relT = hj3d.Rel(R, key_word=0), hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)
ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb), hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
ts.reserve(S.shape[0])
tt.reserve(T.shape[0])
ctx.build_many([ts, tt], [relS, relT])
c_top = ctx.probe2(ts, tt, relR, checksum=False)["c_top"]
out = torch.empty((c_top, 3), dtype=torch.int32, device="cuda")
ns_, nt_ = (torch.empty((nR, 2), dtype=torch.int32, device="cuda") for _ in range(2))
trip = torch.empty((nR, 3), dtype=torch.int32, device="cuda")
rows = torch.arange(nR, dtype=torch.int32, device="cuda")


def fused(fetch=False):
    return ctx.probe2(ts, tt, relR, fetch=fetch, checksum=False, out=out)


def split(fetch=False):
    ctx.probe(ts, relR, out=ns_, mainref=True, fetch=False, checksum=False)
    ctx.probe(tt, relR, out=nt_, mainref=True, fetch=False, checksum=False)
    # the combine: both outputs ordered by probe row (a scatter each), side by side
    trip[:, 0] = rows
    trip[ns_[:, 0].long(), 1] = ns_[:, 1]
    trip[nt_[:, 0].long(), 2] = nt_[:, 1]
    return ctx.unnest2(ts, tt, trip, out=out, fetch=fetch, checksum=False)


def first_probe():
    return ctx.probe(ts, relR, out=ns_, mainref=True, fetch=False, checksum=False)


def chained(fetch=False, survivors=None):
    first_probe()
    if survivors is None:
        survivors = ctx.probe_ref(tt, relR, ns_, out=trip, checksum=False).n_out
    else:
        ctx.probe_ref(tt, relR, ns_, out=trip, checksum=False, fetch=False)
    return ctx.unnest2(ts, tt, trip[:survivors], out=out, fetch=fetch, checksum=False)


a, b, c = fused(True), split(True), chained(True)
first_probe()
rs = ctx.probe_result()
rt = ctx.probe_ref(tt, relR, ns_, out=trip, checksum=False)
keys = ("c_top", "c_unnest_1", "c_unnest_2", "sum_a", "sum_b", "sum_c")
assert not a["overflow"] and not b["overflow"] and not c["overflow"], (a, b, c)
assert all(a[k] == b[k] == c[k] for k in keys), (a, b, c)
# the reference's probe counters: the first probe's and, over its survivors only, the second's
assert (rs.n_matched, rs.n_cmps) == (a["c_probe_rs"], a["c_probe_rs_cmp"]), (rs, a)
assert (rt.n_probe, rt.n_matched, rt.n_cmps) == (a["c_probe_rs"], a["c_probe_rt"], a["c_probe_rt_cmp"]), (rt, a)
known = rt.n_out

forms = {"fused": fused, "split": split, "chained": chained, "chained_known": lambda: chained(survivors=known)}
for fn in forms.values():
    fn()  # warm-up of every form (scratch sizes, code objects)
ms = {k: [] for k in forms}
for _ in range(rounds):
    for k, fn in forms.items():
        ms[k].append(timed(fn))
first_probe()
parts = {
    "first_mainref_probe": timed(first_probe),
    "probe_ref": timed(lambda: ctx.probe_ref(tt, relR, ns_, out=trip, checksum=False, fetch=False)),
    "unnest2_of_survivors": timed(lambda: ctx.unnest2(ts, tt, trip[:known], out=out, fetch=False, checksum=False)),
}
med = {k: statistics.median(v) for k, v in ms.items()}
res = {
    "config": f"E: log2R={log2R} alpha={al} A={A} beta={be} B={B}, |S|=|T|={S.shape[0]}, nb={nb}, plan Ndu",
    "reps": reps, "rounds": rounds, "checksum": False, "c_top": c_top,
    "probe_ref_input_tuples": nR, "probe_ref_live_tuples": rt.n_probe, "probe_ref_survivors": known,
    "ms": ms, "ms_median": med, "chained_parts_ms": parts,
    "chained_over_split": med["chained"] / med["split"], "chained_over_fused": med["chained"] / med["fused"],
}
ts.close()
tt.close()
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(res))
