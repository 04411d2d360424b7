"""hj3d_unnestn's magnitude rule on the GPU, as a program of its own (tests/test_gpu_unnestn.py runs it
under a time limit): one table holds a key of 2^16 rows and a key of 2^15 rows. One tuple with k = 4 on
the first has the product 2^64; 16 tuples with k = 4 on the second have products of 2^60 and the total
2^64. Both wrap to 0 in 64-bit arithmetic. hj3d_unnestn_result must return HJ3D_EUNSUPPORTED for
either, promptly, with no output row written. Prints "magnitude OK"."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-hashjoin_amd", "python"), os.path.dirname(os.path.abspath(__file__))]

CANARY = 0x5A5A5A5A


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

    def tuples(rows):
        return torch.from_numpy(np.array(rows, dtype=np.uint32).view(np.int32)).cuda()

    cases = {
        "one product of 2^64": tuples([[1, one, one, one, one], [2, hot, hot, hot, hot], [3, one, one, one, one]]),
        "a total of 2^64": tuples([[i, mid, mid, mid, mid] for i in range(16)]),
    }
    for what, nested in cases.items():
        for emit in (True, False):
            buf = torch.full((4096 + 64, 5), CANARY, dtype=torch.int32, device="cuda")
            t0 = time.perf_counter()
            try:
                ctx.unnestn([t] * 4, nested, out=buf[:4096] if emit else None)
                raise AssertionError(f"{what}: not refused")
            except hj3d.Hj3dError as e:
                assert e.status == hj3d.HJ3D_EUNSUPPORTED, (what, e.status)
            dt = time.perf_counter() - t0
            assert dt < 5.0, (what, dt)
            assert bool((buf == CANARY).all()), what
    # the same context afterwards: an ordinary input is expanded (3^4 rows of the 3-row key)
    ok = ctx.unnestn([t] * 4, tuples([[5, one, one, one, one]]))
    assert (ok["n_live"], ok["c_unnest"], ok["c_top"], ok["overflow"]) == (1, [3, 9, 27, 81], 81, False)
    ctx.close()
    print("magnitude OK")


if __name__ == "__main__":
    main()
