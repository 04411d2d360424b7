"""Triple write-out of the experiment-4 probe strand at config E on one GPU (log2R = 22, alpha=3 A=4
beta=2 B=2: the relations of bench.py --workload E): hj3d_probe2 with plans Ndu and Chj, each counting
only, with HJ3D_PROBE_EMIT into a buffer of c_top triples and with EMIT at capacity 0 (the slot
reservations without the stores), checksum=False. Probe ms per call, probe
tuples/s, output triples/s and the achieved write rate (12 B x c_top / probe time) go to
profiles/exp4_emit_E.json under "emit" (other keys of that file, e.g. recorded bench.py runs, are
kept) and are printed as one JSON line. The run ends itself after --timeout seconds (default 300).
usage: python scripts/time_exp4_emit.py [--reps N] [--log2R K] [--timeout S] [--out FILE]"""
import json
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3d-hashjoin_amd", "python"))


def arg(name, default, conv=int):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


signal.alarm(arg("--timeout", 300))  # its own time limit: SIGALRM ends the process
import torch  # noqa: E402
import hj3d  # noqa: E402

reps = arg("--reps", 20)
log2R, a, A, b, B = arg("--log2R", 22), 3, 4, 2, 2
out_path = arg("--out", os.path.join(ROOT, "profiles", "exp4_emit_E.json"), str)
nR = 1 << log2R
ctx = hj3d.Context(0)
R, S, T = hj3d.exp4_relations_ref(log2R, a, A, b, B, device="cuda")
nb = (nR >> a) + (nR >> b)
relR, relS, relT = hj3d.Rel(R, key_word=0), hj3d.Rel(S, key_word=1), hj3d.Rel(T, key_word=1)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    x.record()
    for _ in range(reps):
        fn()
    y.record()
    torch.cuda.synchronize()
    return x.elapsed_time(y) / reps


res = {"config": f"E: log2R={log2R} alpha={a} A={A} beta={b} B={B}, |S|=|T|={S.shape[0]}, nb={nb}", "reps": reps,
       "checksum": False, "plans": {}}
for plan, kind in (("Ndu", hj3d.HJ3D_NESTED), ("Chj", hj3d.HJ3D_CHAIN)):
    ts, tt = hj3d.Table(ctx, kind, nb), hj3d.Table(ctx, kind, nb)
    ts.reserve(S.shape[0])
    tt.reserve(T.shape[0])
    ctx.build_many([ts, tt], [relS, relT])
    count = ctx.probe2(ts, tt, relR, checksum=False)
    n = count["c_top"]
    out = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    emit = ctx.probe2(ts, tt, relR, checksum=False, out=out)
    keys = [k for k in count if k != "overflow"]
    assert not emit["overflow"] and all(emit[k] == count[k] for k in keys), (plan, count, emit)
    ms0 = timed(lambda: ctx.probe2(ts, tt, relR, fetch=False, checksum=False))
    ms1 = timed(lambda: ctx.probe2(ts, tt, relR, fetch=False, checksum=False, out=out))
    # capacity 0: every slot is reserved (the cursor's atomics run) and no triple is stored
    ms2 = timed(lambda: ctx.probe2(ts, tt, relR, fetch=False, checksum=False, out=out[:0]))
    res["plans"][plan] = {
        "c_top": n, "probe_ms": ms0, "probe_emit_ms": ms1, "emit_over_count": ms1 / ms0,
        "probe_emit_cap0_ms": ms2,
        "probe_tuples_per_s": nR / (ms0 * 1e-3), "probe_tuples_per_s_emit": nR / (ms1 * 1e-3),
        "triples_per_s_emit": n / (ms1 * 1e-3), "write_bytes_per_s_emit": 12 * n / (ms1 * 1e-3),
    }
    del out
    ts.close()
    tt.close()
ctx.close()
doc = {}
if os.path.exists(out_path):
    with open(out_path) as fh:
        doc = json.load(fh)
doc["emit"] = res
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(doc, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(json.dumps(res))
