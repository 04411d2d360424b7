"""Host side of the experiment-4 triple output (no GPU): hj3d.triple_checksums over a brute-force
join of the fixtures' own dumped columns reproduces the reference binary's output checksums, and the
Python interface takes an output buffer."""
import inspect

import numpy as np
import pytest

from conftest import load_golden

DUMPED = [(n, g) for n, g in load_golden("exp4_*.json") if "Sa" in g and "Ta" in g]


def brute_join(Rk, Sa, Ta) -> np.ndarray:
    """All (r, s, t) row triples with R.k[r] == S.a[s] == T.a[t], as an (n, 3) uint32 array."""
    Sa, Ta = np.asarray(Sa, dtype=np.uint32), np.asarray(Ta, dtype=np.uint32)
    so, to = np.argsort(Sa, kind="stable"), np.argsort(Ta, kind="stable")
    ss, st = Sa[so], Ta[to]
    out = [np.zeros((0, 3), dtype=np.uint32)]
    for r, k in enumerate(np.asarray(Rk, dtype=np.uint32)):
        s = so[np.searchsorted(ss, k, "left"):np.searchsorted(ss, k, "right")]
        t = to[np.searchsorted(st, k, "left"):np.searchsorted(st, k, "right")]
        if len(s) and len(t):
            blk = np.empty((len(s) * len(t), 3), dtype=np.uint32)
            blk[:, 0] = r
            blk[:, 1] = np.repeat(s, len(t))
            blk[:, 2] = np.tile(t, len(s))
            out.append(blk)
    return np.concatenate(out)


def test_dumped_fixtures_present():
    assert {n for n, _ in DUMPED} >= {"exp4_R3_a2_A2_b2_B1", "exp4_R10_a3_A2_b2_B3"}


@pytest.mark.parametrize("name,g", DUMPED, ids=[n for n, _ in DUMPED])
def test_triple_checksums_of_brute_force_join_equal_fixture(name, g):
    import hj3d
    trip = brute_join(np.arange(g["cardR"], dtype=np.uint32), g["Sa"], g["Ta"])
    got = hj3d.triple_checksums(trip)
    assert got == g["plans"]["Ndu"]["out"]
    assert got == g["plans"]["Chj"]["out"]
    assert got["n"] == g["plans"]["Ndu"]["c_top"]
    # as signed device words (an int32 tensor's view) the rows are the same rows
    assert hj3d.triple_checksums(trip.view(np.int32)) == got


def test_triple_hash_scalar_equals_vectorised():
    import hj3d
    rng = np.random.default_rng(1)
    trip = rng.integers(0, 1 << 32, size=(7, 3), dtype=np.uint64).astype(np.uint32)
    trip[0] = (0xFFFFFFFF, 0, 0xFFFFFFFE)
    hs = [hj3d.triple_hash(int(a), int(b), int(c)) for a, b, c in trip]
    got = hj3d.triple_checksums(trip)
    assert got["sum_h"] == sum(hs) & hj3d.MASK64
    x = 0
    for h in hs:
        x ^= h
    assert got["xor_h"] == x
    assert hj3d.triple_hash(1, 2, 3) == hj3d.mix64(hj3d.pair_hash(1, 2) ^ 3)
    assert hj3d.triple_checksums(np.zeros((0, 3), dtype=np.uint32)) == \
        {"n": 0, "sum_a": 0, "sum_b": 0, "sum_c": 0, "sum_h": 0, "xor_h": 0}
    with pytest.raises(ValueError):
        hj3d.triple_checksums(np.zeros((4, 2), dtype=np.uint32))


def test_interface_takes_an_output_buffer():
    import hj3d
    assert inspect.signature(hj3d.Context.probe2).parameters["out"].default is None
    assert inspect.signature(hj3d.exp4_plan).parameters["out"].default is None
    assert inspect.signature(hj3d.exp4_plan_sharded).parameters["out"].default is None
