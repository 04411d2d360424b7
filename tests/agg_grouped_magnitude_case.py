"""hj3d_agg_grouped's magnitude rule on the GPU, as a program of its own (tests/test_gpu_agg_grouped.py runs
it under a time limit): one table holds a key of 2^16 rows and a key of 2^15 rows. One tuple with k = 4 on
the first has the product 2^64; 16 tuples with k = 4 on the second have products of 2^60 and the total 2^64.
Both wrap to 0 in 64-bit arithmetic. hj3d_agg_grouped_result must return HJ3D_EUNSUPPORTED for either, in
every kernel form, promptly, with only n_in and n_live set and nothing written behind the column. Prints
"magnitude OK"."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-hashjoin_amd", "python"), os.path.dirname(os.path.abspath(__file__))]

CANARY = 0x5A5A5A5A5A5A5A5A


def main():
    import torch
    import hj3d
    ctx = hj3d.Context(0)
    HOT, MID, ONE = 7, 8, 9
    col = np.random.default_rng(71).permutation(
        np.repeat(np.array([HOT, MID, ONE], dtype=np.uint32), [1 << 16, 1 << 15, 3]))
    rel = torch.from_numpy(np.stack([np.arange(len(col), dtype=np.uint32), col], axis=1).view(np.int32)).cuda()
    t = hj3d.Table(ctx, hj3d.HJ3D_NESTED, 16)
    t.build(hj3d.Rel(rel, key_word=1))
    keys = torch.tensor([[HOT, 0], [MID, 0], [ONE, 0]], dtype=torch.int32, device="cuda")
    dense = torch.zeros((3, 2), dtype=torch.int32, device="cuda")
    ctx.probe(t, hj3d.Rel(keys, key_word=0), out=dense, mainref=True)
    ref = {int(a): int(r) for a, r in dense.cpu().numpy().view(np.uint32)}
    hot, mid, one = ref[0], ref[1], ref[2]
    assert len({hot, mid, one}) == 3 and max(hot, mid, one) < 3
    gcol, _ = t.group_agg(hj3d.Rel(rel, key_word=1), 0, False)
    specs = [("count",), ("sum", 2, gcol, False), ("max", 3, gcol, False)]

    def tuples(rows):
        return torch.from_numpy(np.array(rows, dtype=np.uint32).view(np.int32)).cuda()

    cases = {
        "one product of 2^64": tuples([[1, one, one, one, one], [2, hot, hot, hot, hot], [3, one, one, one, one]]),
        "a total of 2^64": tuples([[i, mid, mid, mid, mid] for i in range(16)]),
    }
    for what, nested in cases.items():
        for form in (0, 1, 2, 3):
            buf = torch.full((3 + 64, 3), CANARY, dtype=torch.int64, device="cuda")
            ctx.gby_form(form)
            t0 = time.perf_counter()
            try:
                ctx.agg_grouped(nested, [t] * 4, 1, specs, out=buf[:3])
                raise AssertionError(f"{what}: not refused")
            except hj3d.Hj3dError as e:
                assert e.status == hj3d.HJ3D_EUNSUPPORTED, (what, e.status)
            dt = time.perf_counter() - t0
            assert dt < 5.0, (what, dt)
            res = hj3d._AggNRes()
            assert hj3d.lib().hj3d_agg_grouped_result(ctx.h, C.byref(res)) == hj3d.HJ3D_EUNSUPPORTED
            assert (res.n_in, res.n_live, res.c_top, list(res.total)) == (nested.shape[0], nested.shape[0], 0, [0] * 8), what
            assert bool((buf[3:] == CANARY).all()), what
    # the same context afterwards: an ordinary input (3^4 rows of the 3-row key), every form
    for form in (0, 1, 2, 3):
        ctx.gby_form(form)
        column, ok = ctx.agg_grouped(tuples([[5, one, one, one, one]]), [t] * 4, 1, specs[:1])
        assert (ok["n_live"], ok["c_top"], ok["total"]) == (1, 81, [81])
        assert column.cpu().numpy()[:, 0].tolist() == [81 if m == one else 0 for m in range(3)]
    ctx.close()
    print("magnitude OK")


if __name__ == "__main__":
    main()
