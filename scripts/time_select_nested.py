"""hj3d_select_nested against the same selection done in torch, between probe(MAINREF) and probe_ref, on
one GPU, in one process, the forms alternating (each round times every form in turn, `--reps` calls each),
checksum=False, at config E's relations (log2R = 22, alpha=3 A=4 beta=2 B=2: bench.py --workload E). R's
second word is filled with a hash of the row id (16 bits), so `R.w < threshold` selects about 1, 1/2 or
1/16 of the tuples.

  torch    the parent's way: gather R[a, 1] (torch), mask = (ref != 0xFFFFFFFF) & (w < threshold), boolean
           indexing of the dense probe output (which reads the count back)
  device   hj3d_select_nested(base predicate) in the same place; the survivor count comes from the
           validation call, nothing is read back

Per selectivity: the selection alone, the selection followed by probe_ref, and the whole chain
probe(MAINREF) -> [selection] -> probe_ref -> unnest2(EMIT); the chain without a selection once. The
forms' outputs are checked against each other first (torch keeps input order, as the operator does).
hj3d_stream_copy's peak is measured in the same run; the operator's algorithmic bytes per second
(8 B read per tuple, 4 B base word per live tuple, 8 B read again and 8 B written per survivor) are
quoted against it, over the whole call (memset, two kernels, scan, overflow check).
Per form: ms per call of every round, their median and spread ((max - min) / median). The result goes to
profiles/select_nested.json and is printed as one JSON line. The run ends itself after --timeout
seconds (default 420).
usage: python scripts/time_select_nested.py [--reps N] [--rounds K] [--log2R K] [--timeout S] [--out FILE]"""
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
out_path = arg("--out", os.path.join(ROOT, "profiles", "select_nested.json"), str)
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


log2R, al, A, be, B = arg("--log2R", 22), 3, 4, 2, 2
nR = 1 << log2R
R, S, T = hj3d.exp4_relations_ref(log2R, al, A, be, B, device="cuda")
R[:, 1] = ((R[:, 0].long() * 2654435761) >> 7 & 0xFFFF).int()  # 16 hashed bits of the row id
nb = (nR >> al) + (nR >> be)
relR, relS, relT = hj3d.Rel(R, key_word=0), hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)
ts, tt = hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb), hj3d.Table(ctx, hj3d.HJ3D_NESTED, nb)
ctx.build_many([ts, tt], [relS, relT])

# the box's copy peak, in this run
src = torch.empty(64 << 20, dtype=torch.int32, device="cuda")
dst = torch.empty(64 << 20, dtype=torch.int32, device="cuda")
peak = ctx.stream_copy_peak(dst, src)
del src, dst

pairs = torch.empty((nR, 2), dtype=torch.int32, device="cuda")
r1 = ctx.probe(ts, relR, out=pairs, mainref=True, checksum=False)
kept = torch.empty((r1.n_matched, 2), dtype=torch.int32, device="cuda")
trip = torch.empty((r1.n_matched, 3), dtype=torch.int32, device="cuda")
res = {
    "config": f"E: log2R={log2R} alpha={al} A={A} beta={be} B={B}, |S|=|T|={S.shape[0]}, nb={nb}",
    "reps": reps, "rounds": rounds, "checksum": False, "tuples_in": nR, "live": r1.n_matched,
    "stream_copy": peak, "selectivity": {},
}


def torch_select(thr):
    w = R[pairs[:, 0].long(), 1]
    return pairs[(pairs[:, 1] != -1) & (w < thr)]


for name, thr in (("1", 1 << 16), ("1/2", 1 << 15), ("1/16", 1 << 12)):
    preds = [("base", 1, "<", thr)]
    v = ctx.select_nested(pairs, preds, base=relR, out=kept, checksum=False)
    ref = torch_select(thr)
    assert not v.overflow and v.n_matched == r1.n_matched and v.n_out == ref.shape[0], (v, ref.shape)
    assert torch.equal(kept[:v.n_out], ref)  # the same tuples in the same order
    n_kept = v.n_out
    rt = ctx.probe_ref(tt, relR, kept[:n_kept], out=trip, checksum=False)
    n_trip = rt.n_out
    u = ctx.unnest2(ts, tt, trip[:n_trip], checksum=False)
    out = torch.empty((max(u["c_top"], 1), 3), dtype=torch.int32, device="cuda")

    def dev_select():
        ctx.select_nested(pairs, preds, base=relR, out=kept, checksum=False, fetch=False)

    def dev_then_probe():
        dev_select()
        ctx.probe_ref(tt, relR, kept[:n_kept], out=trip, checksum=False, fetch=False)

    def torch_then_probe():
        ctx.probe_ref(tt, relR, torch_select(thr), out=trip, checksum=False, fetch=False)

    def dev_chain():
        ctx.probe(ts, relR, out=pairs, mainref=True, fetch=False, checksum=False)
        dev_then_probe()
        ctx.unnest2(ts, tt, trip[:n_trip], out=out, checksum=False, fetch=False)

    def torch_chain():
        ctx.probe(ts, relR, out=pairs, mainref=True, fetch=False, checksum=False)
        torch_then_probe()
        ctx.unnest2(ts, tt, trip[:n_trip], out=out, checksum=False, fetch=False)

    m = alternate({"torch_select": lambda: torch_select(thr), "device_select": dev_select,
                   "torch_select_probe_ref": torch_then_probe, "device_select_probe_ref": dev_then_probe,
                   "torch_chain": torch_chain, "device_chain": dev_chain})
    algo = 8 * nR + 4 * r1.n_matched + 16 * n_kept
    gbs = algo / m["ms_median"]["device_select"] / 1e6
    m.update(threshold=thr, passing=n_kept, triples=n_trip, c_top=u["c_top"], algorithmic_bytes=algo,
             device_select_GBs=gbs, fraction_of_copy_peak=gbs / peak["copy_peak_GBs"],
             device_over_torch={k: m["ms_median"]["device_" + k] / m["ms_median"]["torch_" + k]
                                for k in ("select", "select_probe_ref", "chain")})
    res["selectivity"][name] = m
    del out

# the chain without a selection (the dense probe output goes to probe_ref as it stands)
rt = ctx.probe_ref(tt, relR, pairs, out=trip, checksum=False)
n_trip = rt.n_out
u = ctx.unnest2(ts, tt, trip[:n_trip], checksum=False)
out = torch.empty((u["c_top"], 3), dtype=torch.int32, device="cuda")


def plain_chain():
    ctx.probe(ts, relR, out=pairs, mainref=True, fetch=False, checksum=False)
    ctx.probe_ref(tt, relR, pairs, out=trip, checksum=False, fetch=False)
    ctx.unnest2(ts, tt, trip[:n_trip], out=out, checksum=False, fetch=False)


res["chain_without_selection"] = dict(alternate({"chain": plain_chain}), triples=n_trip, c_top=u["c_top"])
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(res))
