"""Every operator on a side stream with late inputs (tests/stream_order.py): what include/hj3d.h
promises about streams, checked where a violation shows. The contexts here run on non-blocking side
streams; torch's current stream stays the default one except inside the harness. Every comparison is
exact, against the CPU references of tests/stream_cases.py computed from the real data (the oracle,
tablestruct, expand_ref, expand_n_ref, select_nested_ref, agg_nested_ref); results are read through
the library's synchronous getters with no synchronisation before them. Every case asserts the build
path, or the launch count that test_gpu_probe_api.EXPECTED_LAUNCHES pins to its dispatch path.

FULLY_ASYNC classifies the cases by reading api.cpp and the launchers (a host wait is a
hipStreamSynchronize / hipEventSynchronize / polled event on the path of the call):
  * every probe form on a finished table, the operators over stored nested tuples, group_agg, the
    exchange partitioners, the bitmap helpers and the ticketed exchange enqueue only;
  * hj3d_probe_ref / _refn enqueue only on the partitioned probe path (HJ3D_OPT_RADIX_MIN = 64 here),
    where the liveness test is fused into the probe partitioner;
  * chaining radix and direct builds enqueue only; hj3d_build of a nested table by the aggregation
    builds enqueues only, and the wait is in hj3d_table_finish (sampled before it);
  * NOT fully asynchronous: the slice build (pk_overflow_check reads its overflow count), also when it
    gives up for the direct build; the sort build (it reads the key width); HJ3D_OPT_SYNC_BUILD;
    unfused probe_sel (it reads the selection's count), and a probe_sel with HJ3D_PROBE_ACCUMULATE:
    api.cpp's hj3d_probe_sel keeps ACCUMULATE out of its fused branch, so both calls of such a strand select
    first and read the selection's count on the host.
For the cases that are not fully asynchronous the late input proves only that the wait is on the
context's stream (a wait elsewhere returns at once and the rest reads the decoy); what they enqueue
after their last wait is checked by the clone and the clobber only as far as the host runs ahead of
the device, i.e. probabilistically. A nested table's first use after a build that gave up is
hj3d_table_finish here: the build call before it is fully asynchronous, the finish is not.

Two contexts at once: scan.hip's look-back takes its tiles by ticket (a tile's predecessors belong to
workgroups already running), the nested aggregation build's timed look-back exists only in its slice
form, which the case does not take, and the fused build partition's grid barrier is switched off
(HJ3D_OPT_RP_UNFUSED); no kernel of the two strands needs more co-residency than dispatch order gives.

Measured on an MI355X, one run, ms: case delay / host enqueue in the warm-up / in the counted call. The
delay is by torch events on the side stream (the calibrated repeat count's own measurement); the host
time is the wall time of the enqueue sequence (late copies, call, clones, clobber; for a nested build up
to hj3d_table_finish). * marks a call that returned after the delay had ended: the stand-in that
synchronises, and the cases classified as not fully asynchronous, whose counted host time is the delay
they waited for. Every fully asynchronous case returned in under 0.1 ms against a delay of 6.0 ms.
  standin_same_stream 6.0/0.085/0.037, standin_second_stream 6.0/0.050/0.041
  standin_host_sync 6.0/0.046/5.452*, radix 6.0/0.026/0.020, direct 6.0/0.035/0.026
  slices 6.0/0.103/5.532*, nested_agg 6.0/0.033/0.028, nested_agg_reg 6.0/0.029/0.030
  nested_agg_slices 6.0/0.027/0.028, nested_agg_slices_reg 6.0/0.038/0.039
  nested_sort 6.0/0.115/5.571*, giveup_then_sort 6.0/0.027/0.028, slices_fill13 6.0/0.155/5.577*
  slices_overflow_then_direct 6.0/0.280/5.632*, giveup_then_sort_sync 24.1/3.396/24.957*
  build_many 6.0/0.040/0.038, chain_direct_count 6.0/0.016/0.022
  chain_direct_nonunique_emit 6.0/0.049/0.036, chain_direct_unique_dense 6.0/0.021/0.021
  chain_part_count 6.0/0.045/0.044, chain_part_nonunique_emit 6.0/0.076/0.071
  chain_part_unique_dense 6.0/0.049/0.049, nested_direct_agg 6.0/0.016/0.016
  nested_direct_aggun 6.0/0.021/0.021, nested_direct_countun 6.0/0.047/0.048
  nested_direct_dense 6.0/0.020/0.021, nested_direct_denseref 6.0/0.021/0.021
  nested_part_agg 6.0/0.037/0.037, nested_part_aggun 6.0/0.046/0.043
  nested_part_countun 6.0/0.066/0.066, nested_part_dense 6.0/0.044/0.043
  nested_part_denseref 6.0/0.043/0.043, nested_pk_slices_countun 6.0/0.073/0.073
  nested_pk_slices_dense 6.0/0.052/0.050, packed_one_level 6.0/0.023/0.023
  packed_refused 6.0/0.050/0.050, packed_two_levels 6.0/0.027/0.026
  packed_zipf_overflow 6.0/0.028/0.027, sel_accumulate_chain 6.0/0.190/5.610*
  sel_accumulate_nested 6.0/0.135/5.544*, sel_fused_chain 6.0/0.045/0.046
  sel_fused_nested 6.0/0.041/0.042, sel_fused_packed 6.0/0.019/0.020
  sel_unfused_chain 6.0/0.089/5.460*, sel_unfused_nested 6.0/0.082/5.458*
  probe2_chain 6.0/0.023/0.020, probe2_chain_emit 6.0/0.027/0.026
  probe2_nested_direct 6.0/0.018/0.019, probe2_nested_direct_emit 6.0/0.025/0.025
  probe2_nested_part 6.0/0.028/0.027, probe2_nested_part_emit 6.0/0.037/0.034, unnest 6.0/0.051/0.050
  unnest2 6.0/0.045/0.036, unnestn 6.0/0.066/0.037, probe_ref 6.0/0.093/0.071
  probe_refn 6.0/0.082/0.071, select_nested 6.0/0.067/0.049, agg_nested 6.0/0.062/0.045
  group_agg 6.0/0.026/0.026, unnest_count 6.0/0.041/0.039, unnest_ck 6.0/0.041/0.039
  unnest_emit 6.0/0.050/0.049, unnest2_count 6.0/0.029/0.028, partition 6.0/0.034/0.031
  partition_sel 6.0/0.033/0.032, partition_strided 6.0/0.026/0.026, bitmap 6.0/0.037/0.036
  comm_exchange 6.0/0.058/0.047, set_stream 6.3/0.017/0.046
Two contexts (rounds 1-3): delays 6.0 / 6.2 ms on the two streams, 0.5 ms on the host for the late copies,
both builds and A's probe in the warm-up round; both delays still ran before B's probe in every round.
"""
import ctypes as C
import time
from contextlib import contextmanager
from types import SimpleNamespace

import numpy as np
import pytest

import agg_nested_ref as AN
import expand_n_ref as XN
import expand_ref as X
import oracle as O
import stream_cases as SC
import stream_order as SO
import tablestruct as TS
import test_gpu_probe_api as PA
import test_gpu_table_lifecycle as LC

pytestmark = pytest.mark.gpu

NOREF = 0xFFFFFFFF

NOT_ASYNC = {
    "slices": "pk_overflow_check", "slices_fill13": "pk_overflow_check",
    "slices_overflow_then_direct": "pk_overflow_check", "nested_sort": "the sort build's key-width read",
    "giveup_then_sort_sync": "HJ3D_OPT_SYNC_BUILD finishes inside hj3d_build",
    "sel_unfused_chain": "the selection's count read", "sel_unfused_nested": "the selection's count read",
    "sel_accumulate_chain": "an ACCUMULATE strand is never fused: the selection's count read",
    "sel_accumulate_nested": "an ACCUMULATE strand is never fused: the selection's count read",
}
BUILDS = {**LC.SELECTIONS, **LC.MORE_SELECTIONS}
BUILDS["giveup_then_sort_sync"] = LC.SELECTIONS["giveup_then_sort"]
# EXPECTED_LAUNCHES' hj3d_unnest / hj3d_unnest2 keys -> the operator case below that runs that form
UNNEST_KEYS = {"unnest_ck_emit": "unnest", "unnest2_emit": "unnest2", **{v[3]: k for k, v in SC.UNNEST_FORMS.items()}}
CASE_NAMES = (list(BUILDS) + ["build_many"] + list(SC.PROBES) + list(SC.PROBE2) + list(SC.OPERATORS) +
              ["partition", "partition_sel", "partition_strided", "bitmap", "comm_exchange", "set_stream", "two_contexts"])
FULLY_ASYNC = {name: name not in NOT_ASYNC for name in CASE_NAMES}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def side():
    import torch
    import hj3d
    s = torch.cuda.Stream()
    ctx = hj3d.Context(0, stream=s)
    assert ctx.stream_handle() == s.cuda_stream != 0
    yield SimpleNamespace(s=s, ctx=ctx, h=SO.Harness(s))
    ctx.close()


@pytest.fixture(scope="module")
def pw(side):
    """test_gpu_probe_api's world on the side-stream context (made with that stream current, so that the
    fills of its buffers are ordered before the library's writes)."""
    import torch
    with torch.cuda.stream(side.s):
        w = PA.make_world(side.ctx)
        PA.big_chain(w)
        PA.big_nested(w)
        side.ctx.sync()
        ref, bc, bn = SC.world(), SC.big_chain(), SC.big_nested()
        for t, a in ((w.dR, ref.R), (w.dS, ref.S), (w.dT, ref.T), (w.dBigR, bc.R), (w.dBigS, bc.S), (w.dBigNR, bn.R),
                     (w.dBigNS, bn.S)):
            assert np.array_equal(u32(t.cpu().numpy()), a)
        w.late = {}
    return w


def late_of(w, name, tensor, real, decoy):
    """The Late `name` of a tensor the world holds, for the host arrays `real` (what it holds) and `decoy`.
    name: the tensor and the word its decoy changes ("world.S.key1"), one Late per name."""
    if name not in w.late:
        w.late[name] = SO.Late.wrap(tensor, real, decoy)
    assert w.late[name].tensor is tensor
    return w.late[name]


@contextmanager
def lent(side, inputs):
    """The world's tensors get their real data back whatever the case did to them."""
    import torch
    try:
        yield
    finally:
        with torch.cuda.stream(side.s):
            for i in inputs:
                i.tensor.copy_(i.real)
            torch.cuda.synchronize()


def zeros(side, shape, dtype=None):
    import torch
    with torch.cuda.stream(side.s):
        return torch.zeros(shape, dtype=dtype or torch.int32, device="cuda")


def counted(box, fn):
    """fn() with its kernel launches counted into box["n"]."""
    import hj3d
    L = hj3d.lib()

    def run():
        c0 = L.hj3d_launch_count()
        fn()
        box["n"] = L.hj3d_launch_count() - c0
    return run


# ---- the harness itself (torch only) ----
def standin(side, how):
    """A stand-in operator that sums its late input into a one-element tensor."""
    import torch
    real = np.arange(1 << 16, dtype=np.uint32).reshape(-1, 2)
    late = SO.Late.of(real, real + np.uint32(SC.SHIFT))
    out = zeros(side, 1, torch.int64)
    other = torch.cuda.Stream()

    def call():
        if how == "second_stream":
            with torch.cuda.stream(other):
                out.copy_(late.tensor.sum())
        else:
            out.copy_(late.tensor.sum())
        if how == "host_sync":
            torch.cuda.current_stream().synchronize()
    o = side.h.run(f"standin_{how}", [late], call, outputs=[out])
    side.s.synchronize()
    other.synchronize()
    return int(side.h.host(o.clones[0])[0]), int(real.sum())


def test_harness_reports_a_correct_operator(side):
    got, want = standin(side, "same_stream")
    assert got == want


def test_harness_reports_the_wrong_stream_as_a_mismatch(side):
    got, want = standin(side, "second_stream")
    assert got != want


def test_harness_reports_a_host_wait_as_not_asynchronous(side):
    import torch
    with pytest.raises(SO.DelayTooShort, match="delay too short"):
        standin(side, "host_sync")
    torch.cuda.synchronize()


# ---- builds ----
def check_late_build(side, name, tables, lates, call, datas, path, started=None):
    nested = datas[0].kind == TS.NESTED

    def finish():
        for t in tables:
            if started:  # (the deferred finish: the build that was begun is still unresolved)
                assert t.build_path(finish=False) == started, t.build_path(finish=False)
            t.finish()

    def clear():
        for t in tables:
            t.clear()
    side.h.run(name, lates, call, fully_async=FULLY_ASYNC[name], before_clobber=finish if nested else None, reset=clear)
    for t, d in zip(tables, datas):
        assert t.build_path() == path, (name, t.build_path())
        LC.check_export(t, d)
        LC.check_probes(side.ctx, t, d)


@pytest.mark.parametrize("sel", list(BUILDS))
def test_build_with_a_late_relation(side, sel):
    import hj3d
    ctx = side.ctx
    name, opts, path = BUILDS[sel]
    d = LC.data(name)
    assert np.array_equal(SC.build_tuples(name), d.tuples)
    late = SO.Late.of(d.tuples, SC.decoy_build(d.tuples, 1))
    rel = hj3d.Rel(late.tensor, 1)
    try:
        ctx.sync_build(sel == "giveup_then_sort_sync")
        with LC.options(ctx, **opts):
            t = LC.new_table(ctx, d)
            check_late_build(side, sel, [t], [late], lambda: t.build(rel), [d], path,
                             started="nested_agg?" if sel == "giveup_then_sort" else None)
            t.close()
    finally:
        ctx.sync_build(False)


def test_build_many_with_two_late_relations(side):
    import hj3d
    ctx = side.ctx
    ds = [LC.data("nested"), LC.data("nested_other")]
    lates = [SO.Late.of(d.tuples, SC.decoy_build(d.tuples, 1)) for d in ds]
    rels = [hj3d.Rel(x.tensor, 1) for x in lates]
    with LC.options(ctx, **LC.RM0):
        ts = [LC.new_table(ctx, d) for d in ds]
        check_late_build(side, "build_many", ts, lates, lambda: ctx.build_many(ts, rels), ds, "nested_agg",
                         started="nested_agg?")
        for t in ts:
            t.close()


# ---- probes ----
@pytest.fixture(scope="module")
def zipf_table(side):
    import torch
    import hj3d
    z = SC.zipf()
    with torch.cuda.stream(side.s):
        dR, dS = SO.to_device(z.R), SO.to_device(z.S)
        t = PA.table(side.ctx, hj3d.HJ3D_CHAIN, z.nb, hj3d.Rel(dR, key_word=0))
        side.ctx.sync()
    yield SimpleNamespace(t=t, dR=dR, dS=dS, S=hj3d.Rel(dS, key_word=1, row_word=0), late={}, ctx=side.ctx)
    t.close()


def probe_objects(pw, zt, case):
    """(table, probe Rel, the world that holds the probe tensor) of a probe case."""
    if case["world"] == "zipf":
        return zt.t, zt.S, zt
    if case["world"] == "big_chain":
        return pw.cBig, pw.BigS, pw
    if case["world"] == "big_nested":
        return pw.nBig, pw.BigNR, pw
    tab = {(SC.CHAIN, "S"): pw.cS, (SC.CHAIN, "R"): pw.cR, (SC.NESTED, "S"): pw.nS_}[(case["kind"], case["build"])]
    return tab, (pw.R if case["probe"] == "R" else pw.S), pw


@pytest.mark.parametrize("name", sorted(SC.PROBES))
def test_probe_with_a_late_relation(side, pw, zipf_table, name):
    import hj3d
    ctx, L = side.ctx, hj3d.lib()
    case = SC.PROBES[name]
    f = case["form"]
    t, rel, holder = probe_objects(pw, zipf_table, case)
    _, real, _ = SC.probe_arrays(case)
    late = late_of(holder, f'{case["world"]}.{case["probe"]}.key{case["pkey"]}', rel.tensor, real,
                   SC.decoy_rel(real, case["pkey"]))
    want, agg = SC.probe_expected(case, real)
    out = zeros(side, (max(len(real), want["n_out"]) + 8, 2)) if f.get("emit") else None
    kw = dict(unique=bool(f.get("unique")), unnest=bool(f.get("unnest")), mainref=bool(f.get("mainref")))
    box = {}
    if f.get("sel") and f.get("accumulate"):  # a strand of two calls over the halves of R, the second one counted
        flags = (hj3d.PROBE_UNIQUE if kw["unique"] else 0) | hj3d.PROBE_CHECKSUM
        preds = hj3d._sel_preds(SC.PREDS)
        half = rel.n // 2
        a = hj3d.Rel(rel.tensor[:half], key_word=0)
        b = hj3d.Rel(rel.tensor[half:], key_word=0, row_base=half)

        def sel(r, fl):
            assert L.hj3d_probe_sel(ctx.h, t.h, C.byref(r.c), preds, 1, fl, None, 0) == hj3d.HJ3D_OK
        second = counted(box, lambda: sel(b, flags | hj3d.PROBE_ACCUMULATE))

        def call():
            sel(a, flags)
            second()
    elif f.get("sel"):
        call = counted(box, lambda: ctx.probe_sel(t, rel, SC.PREDS, unique=kw["unique"], fetch=False))
    else:
        call = counted(box, lambda: ctx.probe(t, rel, out=out, fetch=False, **kw))
    with PA.options(ctx, **f["opts"]), lent(side, [late]):
        o = side.h.run(name, [late], call, outputs=[out] if out is not None else [], fully_async=FULLY_ASYNC[name],
                       reset=call)
        got = ctx.probe_result()
    if name in PA.EXPECTED_LAUNCHES:
        assert box["n"] == PA.EXPECTED_LAUNCHES[name], box
    else:  # the packed probe ran (the partitioned probe it would fall back to takes more launches)
        assert box["n"] < PA.EXPECTED_LAUNCHES["packed_refused"], box
    assert not got.overflow
    assert {k: getattr(got, k) for k in want} == want
    if out is not None:
        rows = u32(side.h.host(o.clones[0]))
        n = len(real)
        if f.get("unnest") or (case["kind"] == SC.CHAIN and not f.get("unique")):  # as many pairs as found
            assert {**X.pair_checksums(rows[: want["n_out"]]), "sum_c": 0} == {**agg, "sum_c": 0}
            assert (rows[want["n_out"]:] == SO.CANARY).all()
        else:  # one slot per probe tuple
            assert np.array_equal(np.sort(rows[:n, 0]), np.arange(n, dtype=np.uint32))
            assert (rows[n:] == SO.CANARY).all()
            if case["kind"] == SC.CHAIN:
                assert {**X.pair_checksums(rows[:n][rows[:n, 1] != NOREF]), "sum_c": 0} == {**agg, "sum_c": 0}
            elif f.get("mainref"):
                assert int((rows[:n, 1] != NOREF).sum()) == want["n_matched"]


@pytest.mark.parametrize("name", sorted(SC.PROBE2))
def test_probe2_with_a_late_relation(side, pw, name):
    ctx = side.ctx
    case = SC.PROBE2[name]
    ts, tt = (pw.nS_, pw.nT_) if case["kind"] == SC.NESTED else (pw.cS, pw.cT)
    late = late_of(pw, "world.R.key0", pw.dR, SC.world().R, SC.decoy_rel(SC.world().R, 0))
    want = SC.probe2_expected(case, SC.world().R)
    out = zeros(side, (want["c_top"] + 8, 3)) if case["emit"] else None
    box = {}
    call = counted(box, lambda: ctx.probe2(ts, tt, pw.R, out=out[: want["c_top"]] if case["emit"] else None, fetch=False))
    with PA.options(ctx, **case["opts"]), lent(side, [late]):
        o = side.h.run(name, [late], call, outputs=[out] if case["emit"] else [], fully_async=FULLY_ASYNC[name], reset=call)
        got = ctx.probe2_result()
    assert box["n"] == PA.EXPECTED_LAUNCHES[name], box
    assert not got["overflow"] and {k: got[k] for k in want} == want
    if case["emit"]:
        rows = u32(side.h.host(o.clones[0]))
        cs = X.triple_checksums(rows[: want["c_top"]])
        assert {k: cs[k] for k in ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")} == {k: want[k] for k in
                                                                                     ("sum_a", "sum_b", "sum_c", "sum_h", "xor_h")}
        assert (rows[want["c_top"]:] == SO.CANARY).all()


# ---- operators over stored nested tuples ----
@pytest.fixture(scope="module")
def ops(side, pw):
    """The world's stored tuples and the tables' arrays on the host, and the group_agg columns."""
    import torch
    import hj3d
    with torch.cuda.stream(side.s):
        o = SimpleNamespace()
        o.pairs, o.trip = u32(pw.nested.cpu().numpy()).copy(), u32(pw.trip.cpu().numpy()).copy()
        _, o.mains_s, o.sub_s = pw.nS_.export()
        _, o.mains_t, _ = pw.nT_.export()
        o.relS, o.relT = hj3d.Rel(pw.dS, key_word=1), hj3d.Rel(pw.dT, key_word=1)
        o.col_s = pw.nS_.group_agg(o.relS, SC.AGG_WORD)[0].clone()
        o.col_t = pw.nT_.group_agg(o.relT, SC.AGG_WORD)[0].clone()
        side.ctx.sync()
        o.col_s_np = o.col_s.cpu().numpy().view(np.uint64).copy()
        o.col_t_np = o.col_t.cpu().numpy().view(np.uint64).copy()
        # a dense probe output is in no specified order: the refs by base row
        o.ref_s, o.ref_t = o.trip[:, 1].copy(), o.trip[:, 2].copy()
        assert np.array_equal(o.trip[:, 0], np.arange(len(o.trip), dtype=np.uint32))
    return o


@pytest.mark.parametrize("op", SC.OPERATORS)
def test_operator_with_late_nested_tuples_and_base(side, pw, ops, op):
    import torch
    import hj3d
    ctx, w = side.ctx, SC.world()
    base = hj3d.Rel(pw.dR, key_word=0)
    late_R = late_of(pw, "world.R.key0", pw.dR, w.R, SC.decoy_rel(w.R, 0))
    n = len(w.R)
    box, opts, ordered = {}, {}, False
    arrays = dict(mains_s=ops.mains_s, mains_t=ops.mains_t, sub_s=ops.sub_s, col_s=ops.col_s_np, col_t=ops.col_t_np)
    launches = {v: k for k, v in UNNEST_KEYS.items()}.get(op)  # the EXPECTED_LAUNCHES key of an unnest form
    base_op, checksum, emit, _ = SC.UNNEST_FORMS.get(op, (op, True, True, None))
    if base_op == "unnest":
        tuples, late_n = ops.pairs, late_of(pw, "nested", pw.nested, ops.pairs, SC.decoy_nested(ops.pairs))
        want, rows = SC.operator_expected(op, w.R, w.S, tuples)
        out, inputs, getter = (zeros(side, (len(rows) + 8, 2)) if emit else None), [late_n], ctx.probe_result
        call = lambda: ctx.unnest(pw.nS_, pw.nested, out=out[: len(rows)] if emit else None, checksum=checksum,  # noqa: E731
                                  fetch=False)
    elif base_op == "unnest2":
        tuples, late_n = ops.trip, late_of(pw, "trip", pw.trip, ops.trip, SC.decoy_nested(ops.trip))
        want, rows = SC.operator_expected(op, w.R, w.S, tuples)
        out, inputs, getter = (zeros(side, (len(rows) + 8, 3)) if emit else None), [late_n], ctx.probe2_result
        call = lambda: ctx.unnest2(pw.nS_, pw.nT_, pw.trip, out=out[: len(rows)] if emit else None, fetch=False)  # noqa: E731
    elif op == "unnestn":
        tuples = SC.wide_tuples(ops.trip)
        late_n = SO.Late.of(tuples, SC.decoy_nested(tuples))
        want, rows = SC.operator_expected(op, w.R, w.S, tuples)
        out, inputs, getter = zeros(side, (len(rows) + 8, 4)), [late_n], ctx.unnestn_result
        call = lambda: ctx.unnestn([pw.nS_, pw.nT_, pw.nS_], late_n.tensor, out=out[: len(rows)], fetch=False)  # noqa: E731
    elif op in ("probe_ref", "probe_refn"):
        src, tab, ref = (pw.nested, pw.nT_, ops.ref_t) if op == "probe_ref" else (pw.trip, pw.nS_, ops.ref_s)
        tuples = ops.pairs if op == "probe_ref" else ops.trip
        late_n = late_of(pw, "nested" if op == "probe_ref" else "trip", src, tuples, SC.decoy_nested(tuples))
        want, kept = SC.operator_expected(op, w.R, w.S, tuples)
        rows = np.concatenate([kept, ref[kept[:, 0]][:, None]], axis=1)  # the matched main ref appended
        out, inputs, getter = zeros(side, (n + 8, tuples.shape[1] + 1)), [late_n, late_R], ctx.probe_result
        opts = SC.PART  # the partitioned probe path: the liveness test fused, no count read
        fn = ctx.probe_ref if op == "probe_ref" else ctx.probe_refn
        call = lambda: fn(tab, base, src, out=out[:n], fetch=False)  # noqa: E731
    elif op == "select_nested":
        tuples, late_n = ops.trip, late_of(pw, "trip", pw.trip, ops.trip, SC.decoy_nested(ops.trip))
        want, rows = SC.operator_expected(op, w.R, w.S, tuples, **arrays)
        out, inputs, getter, ordered = zeros(side, (n + 8, 3)), [late_n, late_R], ctx.probe_result, True
        call = lambda: ctx.select_nested(pw.trip, SC.NSEL_PREDS, base=base, tables=[pw.nS_, pw.nT_], out=out[:n],  # noqa: E731
                                         fetch=False)
    elif op == "agg_nested":
        tuples, late_n = ops.trip, late_of(pw, "trip", pw.trip, ops.trip, SC.decoy_nested(ops.trip))
        late_cs = late_of(pw, "col_s", ops.col_s, ops.col_s_np, SC.decoy_column(ops.col_s_np))
        late_ct = late_of(pw, "col_t", ops.col_t, ops.col_t_np, SC.decoy_column(ops.col_t_np))
        want, rows = SC.operator_expected(op, w.R, w.S, tuples, **arrays)
        out, inputs, getter, ordered = zeros(side, (n + 8, 4), torch.int64), [late_n, late_cs, late_ct], ctx.agg_nested_result, True
        specs = [("count",), ("sum", 1, ops.col_s), ("min", 2, ops.col_t), ("max", 1, ops.col_s)]
        call = lambda: ctx.agg_nested(pw.trip, [pw.nS_, pw.nT_], specs, out=out[:n], fetch=False)  # noqa: E731
    else:  # group_agg: the build relation late
        late_n = late_of(pw, "world.S.key0", pw.dS, w.S, SC.decoy_rel(w.S, 0))  # (the folded word is word 0)
        want, rows = SC.operator_expected(op, w.R, w.S, None, **arrays)
        out, inputs, getter, ordered = zeros(side, (len(rows) + 8, 3), torch.int64), [late_n], ctx.probe_result, True
        call = lambda: pw.nS_.group_agg(ops.relS, SC.AGG_WORD, out=out[: len(rows)], fetch=False)  # noqa: E731
    call = counted(box, call)
    with PA.options(ctx, **opts), lent(side, inputs):
        o = side.h.run(op, inputs, call, outputs=[out] if out is not None else [], fully_async=FULLY_ASYNC[op], reset=call)
        raw = getter()
    if launches:
        assert box["n"] == PA.EXPECTED_LAUNCHES[launches], box
    got = raw if isinstance(raw, dict) else {k: getattr(raw, k) for k in want}
    assert {k: got[k] for k in want} == want and (want.get("n_out") or want.get("c_top") or len(rows)) > 0
    assert not (raw["overflow"] if isinstance(raw, dict) else raw.overflow)
    if out is None:  # a form without EMIT: counters only
        return
    host = side.h.host(o.clones[0])
    host = host.view(np.uint64) if host.dtype == np.int64 else u32(host)
    assert (host[len(rows):] == SO.CANARY).all()
    if ordered:
        assert np.array_equal(host[: len(rows)], rows)
    else:
        assert np.array_equal(XN.sort_rows(host[: len(rows)]), XN.sort_rows(rows))


# ---- exchange helpers ----
@pytest.mark.parametrize("form", ["partition", "partition_sel", "partition_strided", "bitmap"])
def test_exchange_helper_with_a_late_relation(side, form):
    import torch
    import hj3d
    ctx = side.ctx
    real = SC.xrel()
    late = SO.Late.of(real, SC.decoy_rel(real, 1))
    rel = hj3d.Rel(late.tensor, key_word=1, row_word=0)
    n, parts = SC.X_N, SC.X_PARTS
    if form == "bitmap":
        bm, cnt = zeros(side, (1, (SC.X_DOMAIN + 31) // 32)), zeros(side, 2, torch.int64)

        def call():
            bm.zero_()
            cnt.zero_()
            ctx.key_bitmap(rel, SC.X_DOMAIN, bm, cnt[1:])
            ctx.bitmap_or_popcount(bm, cnt[:1])
        o = side.h.run(form, [late], call, outputs=[bm, cnt], fully_async=FULLY_ASYNC[form], reset=call)
        ctx.sync()
        want_bm, outside, distinct = SC.bitmap_expected(real)
        assert side.h.host(o.clones[1]).tolist() == [distinct, outside] and distinct > 0
        assert np.array_equal(u32(side.h.host(o.clones[0]))[0], want_bm)
        return
    preds = SC.X_PREDS if form == "partition_sel" else None
    stride = n if form == "partition_strided" else None
    pairs = zeros(side, (parts * n if stride else n, 2))
    counts = zeros(side, parts, torch.int64)
    call = lambda: ctx.partition(rel, SC.X_NB, parts, pairs, counts, preds=preds, stride=stride)  # noqa: E731
    o = side.h.run(form, [late], call, outputs=[pairs, counts], fully_async=FULLY_ASYNC[form], reset=call)
    ctx.sync()
    want_counts, want_pairs = SC.partition_expected(real, preds)
    got_pairs, got_counts = u32(side.h.host(o.clones[0])), side.h.host(o.clones[1]).tolist()
    assert got_counts == want_counts and min(want_counts) > 0
    off = np.concatenate([[0], np.cumsum(want_counts)])
    if stride is None:  # stable: the destinations back to back, scan order inside each
        assert np.array_equal(got_pairs[: off[-1]], want_pairs)
        assert (got_pairs[off[-1]:] == SO.CANARY).all()
    else:
        for p in range(parts):
            got = got_pairs[p * stride: p * stride + want_counts[p]]
            assert np.array_equal(XN.sort_rows(got), XN.sort_rows(want_pairs[off[p]: off[p + 1]])), p
            assert (got_pairs[p * stride + want_counts[p]: (p + 1) * stride] == SO.CANARY).all(), p


def test_ticketed_exchange_with_a_late_send_buffer(side):
    """hj3d_comm_exchange at world size 1 with a ticket: the exchange stream waits for the late send
    buffer through the `ready` event, and hj3d_comm_wait orders the probe of the received pairs (and the
    clobber of the send buffer) after the exchange."""
    import hj3d
    ctx = side.ctx
    import torch
    real, B = SC.comm_case()
    late = SO.Late.of(real, SC.decoy_rel(real, 0))
    recv = zeros(side, (len(real), 2))
    with torch.cuda.stream(side.s):
        dB = SO.to_device(B)  # (an upload the host waits for, made with the side stream current)
        t = PA.table(ctx, hj3d.HJ3D_CHAIN, SC.X_TABLE_NB, hj3d.Rel(dB, key_word=1, row_word=0))
    comm = hj3d.Comm(ctx, hj3d.Comm.unique_id(ctx), 0, 1)
    n = len(real)
    try:
        def call():
            _, ticket = comm.exchange(late.tensor, [n], [n], recv)
            comm.wait(ticket)
            ctx.probe(t, hj3d.Rel(recv, key_word=0, row_word=1), fetch=False)
        o = side.h.run("comm_exchange", [late], call, outputs=[recv], fully_async=FULLY_ASYNC["comm_exchange"], reset=call)
        got = ctx.probe_result()
    finally:
        comm.close()
        t.close()
    want = SC.comm_expected(real)
    assert np.array_equal(u32(side.h.host(o.clones[0])), real)
    assert {k: getattr(got, k) for k in want} == want and want["n_out"] > 0


# ---- hj3d_ctx_set_stream ----
def test_set_stream_moves_later_calls_and_orders_nothing():
    """A build on s1, s2.wait_stream(s1) by the caller, set_stream(s2), then a late-input probe on s2."""
    import torch
    import hj3d
    w = SC.world()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = hj3d.Context(0, stream=s1)
    try:
        with torch.cuda.stream(s1):
            dS = SO.to_device(w.S)
            t = hj3d.Table(ctx, hj3d.HJ3D_CHAIN, 2053)
            t.build(hj3d.Rel(dS, key_word=1, row_word=0))
        s2.wait_stream(s1)
        ctx.set_stream(s2)
        assert ctx.stream is s2 and ctx.stream_handle() == s2.cuda_stream != s1.cuda_stream
        h = SO.Harness(s2)
        late = SO.Late.of(w.R, SC.decoy_rel(w.R, 0))
        rel = hj3d.Rel(late.tensor, key_word=0)
        call = lambda: ctx.probe(t, rel, fetch=False)  # noqa: E731
        h.run("set_stream", [late], call, fully_async=FULLY_ASYNC["set_stream"], reset=call)
        got = ctx.probe_result()
        want, _ = SC.probe_expected(SC.PROBES["chain_direct_count"], w.R)
        assert {k: getattr(got, k) for k in want} == want
        t.close()
    finally:
        ctx.close()


# ---- two contexts at once ----
def test_two_contexts_interleaved_from_one_host_thread():
    """Context A on s1: a chaining radix build and a packed EMIT probe. Context B on s2: a nested_agg
    build and an unnest EMIT probe. The calls alternate, nothing is fetched, all four relations are late;
    three rounds on other data. Both builds and A's probe are fully asynchronous: both delays must still
    run when they have been enqueued. B's probe then finishes B's table first (a host wait on B's build
    event, behind the delay on s2), so its own tail, the clones and the clobbers are covered only as far as
    the host runs ahead."""
    import torch
    import hj3d
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    A, B = hj3d.Context(0, stream=s1), hj3d.Context(0, stream=s2)
    nA, nbB = SC.TWO_NA, SC.TWO_NB_B
    try:
        for c in (A, B):
            c.rp_unfused(True)
            c.radix_min(0)
        A.pk_slice_max(512)
        dA, dB = SO.Delay(s1), SO.Delay(s2)
        warm_ms = 0.0
        tA, tB = hj3d.Table(A, hj3d.HJ3D_CHAIN, nA), hj3d.Table(B, hj3d.HJ3D_NESTED, nbB)
        lates = None
        for rnd in range(SC.TWO_ROUNDS):  # round 0 is the warm-up (scratch grown, then everything synchronised)
            real, decoy = SC.two_ctx_round(rnd).real, SC.two_ctx_round(rnd).decoy
            RA, SA, SB, RB = real
            if lates is None:
                lates = [SO.Late.of(r, d) for r, d in zip(real, decoy)]
                outA = torch.zeros((2 * nA, 2), dtype=torch.int32, device="cuda")
                outB = torch.zeros((400_000, 2), dtype=torch.int32, device="cuda")
            else:
                for x, r, d in zip(lates, real, decoy):
                    x.real.copy_(SO.to_device(r))
                    x.decoy.copy_(SO.to_device(d))
                    x.tensor.copy_(x.decoy)
            outA.fill_(SO.CANARY)
            outB.fill_(SO.CANARY)
            tA.clear()
            tB.clear()
            torch.cuda.synchronize()
            rels = [hj3d.Rel(lates[0].tensor, 0), hj3d.Rel(lates[1].tensor, 1, 0), hj3d.Rel(lates[2].tensor, 1, 0),
                    hj3d.Rel(lates[3].tensor, 0)]
            ends = []
            for s, d in ((s1, dA), (s2, dB)):
                d.reps_for(SO.target_ms(warm_ms))  # (calibrated first: a calibration between the delays outlasts one)
            for s, d in ((s1, dA), (s2, dB)):
                with torch.cuda.stream(s):
                    if rnd:
                        ends.append(d.enqueue(SO.target_ms(warm_ms)))
            t0 = time.perf_counter()
            for s, mine in ((s1, lates[:2]), (s2, lates[2:])):
                with torch.cuda.stream(s):
                    for x in mine:
                        x.tensor.copy_(x.real, non_blocking=True)
            tA.build(rels[0])
            tB.build(rels[2])
            A.probe(tA, rels[1], unique=True, out=outA, fetch=False)
            host_ms = (time.perf_counter() - t0) * 1e3
            still = [not end.query() for end, _ in ends]
            warm_ms = host_ms if rnd == 0 else warm_ms  # (the delays' target: 4 x the warm-up round's host time)
            B.probe(tB, rels[3], unnest=True, out=outB, fetch=False)
            print(f"stream-order two_contexts round {rnd}: delays {[round(ms, 1) for _, ms in ends]} ms, host enqueue "
                  f"{host_ms:.3f} ms, delays still running: {still}")
            if FULLY_ASYNC["two_contexts"] and not all(still):
                raise SO.too_short(f"two_contexts round {rnd}", min(ms for _, ms in ends), host_ms)
            with torch.cuda.stream(s1):
                cA = outA.clone()
                for x in lates[:2]:
                    x.tensor.copy_(x.decoy, non_blocking=True)
            with torch.cuda.stream(s2):
                cB = outB.clone()
                for x in lates[2:]:
                    x.tensor.copy_(x.decoy, non_blocking=True)
            gA, gB = A.probe_result(), B.probe_result()
            assert (tA.build_path(), tB.build_path()) == ("radix", "nested_agg")
            eA, eB = SC.two_ctx_expected(RA, SA, SB, RB)
            for g, e, what in ((gA, eA, "A"), (gB, eB, "B")):
                assert (g.n_out, g.n_cmps, g.sum_a, g.sum_b, g.sum_h, g.xor_h) == \
                    (e.out["n"], e.c_cmp, e.out["sum_a"], e.out["sum_b"], e.out["sum_h"], e.out["xor_h"]), (rnd, what)
                assert not g.overflow and e.out["n"] > 0
            assert gB.n_matched == eB.c_probe
            with torch.cuda.stream(s1):
                rows = u32(cA.cpu().numpy())
            assert {**X.pair_checksums(rows[rows[:, 1] != NOREF]), "sum_c": 0} == {**eA.out, "sum_c": 0}, rnd
            with torch.cuda.stream(s2):
                rows = u32(cB.cpu().numpy())
            assert {**X.pair_checksums(rows[: eB.out["n"]]), "sum_c": 0} == {**eB.out, "sum_c": 0}, rnd
            torch.cuda.synchronize()
        tA.close()
        tB.close()
    finally:
        A.close()
        B.close()


# ---- the wrapper's own allocations ----
def test_wrapper_calls_off_the_context_stream(side):
    """The context runs on the side stream, the caller's current stream is the default one and is busy
    (the delay runs on it); the inputs are ready. The wrappers' own counters and outputs must be made on
    the context's stream: zeroed on the current one, the fill lands after the library's write (select,
    num_distinct, expected_fk_join and exp1_plan_sharded were wrong that way before Context.on_stream;
    group_agg only allocates)."""
    import torch
    import hj3d
    ctx, w = side.ctx, SC.world()
    cur = torch.cuda.current_stream()
    assert cur.cuda_stream != side.s.cuda_stream
    delay = SO.Delay(cur)
    rng = np.random.default_rng(12)
    nk = 4096
    Rk = SC.rows3(rng.permutation(nk), np.zeros(nk))
    Sf = SC.rows3(np.arange(3 * nk), rng.integers(0, nk, 3 * nk))
    dRk, dSf, dS = SO.to_device(Rk), SO.to_device(Sf), SO.to_device(w.S)
    t = PA.table(ctx, hj3d.HJ3D_NESTED, 1500, hj3d.Rel(dS, key_word=1, row_word=0))
    _, mains, sub = t.export()
    torch.cuda.synchronize()

    def late(fn):
        """fn() while the current stream is busy, after a warm-up call of the same shape (scratch that grows
        synchronises the device, which would order the fill and prove nothing)."""
        fn()
        torch.cuda.synchronize()
        delay.enqueue(SO.MIN_DELAY_MS)
        try:
            return fn()
        finally:
            torch.cuda.synchronize()

    e = O.chain_plan(Rk, 0, Sf, 1, nk, True)
    try:
        pairs, _, n = late(lambda: ctx.select(hj3d.Rel(dSf, key_word=1), [(1, "<", 1000)]))
        want = O.select(Sf, 1, [(1, "<", 1000)])
        assert n == len(want) > 0
        assert np.array_equal(u32(side.h.host(pairs[:n])), want)

        assert late(lambda: ctx.num_distinct(hj3d.Rel(dSf, key_word=1), nk)) == O.num_distinct(Sf[:, 1])

        got = late(lambda: ctx.expected_fk_join(hj3d.Rel(dRk, 0), hj3d.Rel(dSf, 1), nk))
        assert got == {k: e.out[k] for k in got} and got["n"] == 3 * nk

        col, r = late(lambda: t.group_agg(hj3d.Rel(dS, key_word=1), SC.AGG_WORD))
        m = AN.group_agg(mains, sub, w.S, SC.AGG_WORD, True)
        assert (r.n_probe, r.n_matched, r.n_out, r.sum_a) == (m["n_probe"], m["n_matched"], m["n_out"], m["sum_a"])
        assert np.array_equal(side.h.host(col).view(np.uint64), m["col"])

        got = late(lambda: hj3d.exp1_plan_sharded(ctx, "Csr", dRk, dSf, nk, 3))
        assert (got["c_probe"], got["c_cmp"], got["c_top"]) == (e.c_probe, e.c_cmp, e.c_top)
        assert got["out"] == e.out
        assert {k: got["stats"][k] for k in TS.STAT_KEYS} == {k: e.stats[k] for k in TS.STAT_KEYS}
    finally:
        t.close()
        torch.cuda.synchronize()
