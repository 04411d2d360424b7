"""tests/gen_model.py (the numpy model of the device generators and of the key/FK verifier) against the
host ABI's hashes, the oracle and its own definitions, on the CPU: the model is pinned before
tests/test_gpu_generators.py judges a kernel with it."""
import numpy as np
import pytest

import gen_model as G
import oracle as O

EDGE = [0, 1, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1]
PERM_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 255, 256, 257, 1023, 1025, 65535, 65537, 2 ** 20, 2 ** 20 + 1]


def test_hashes_match_host_abi():
    import hj3d
    rng = np.random.default_rng(1)
    vals = EDGE + [int(v) for v in rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)]
    assert G.mix64(vals).tolist() == [hj3d.mix64(v) for v in vals]
    a = [v & 0xFFFFFFFF for v in vals] + [0, 2 ** 32 - 1, 2 ** 31]
    b = [v >> 32 for v in vals] + [2 ** 32 - 1, 0, 2 ** 31]
    assert G.pair_hash(a, b).tolist() == [hj3d.pair_hash(x, y) for x, y in zip(a, b)]
    # words above 2^32 are cut like the host ABI's
    assert int(G.pair_hash([2 ** 40 + 5], [2 ** 33 + 7])[0]) == hj3d.pair_hash(2 ** 40 + 5, 2 ** 33 + 7)


def test_feistel_geometry():
    """Even bit counts, at least 2 bits; the domain is below 4 n + 4."""
    assert [G.feistel_geometry(n)[0] for n in (0, 1, 2, 3, 4, 5, 16, 17, 256, 257, 2 ** 20, 2 ** 20 + 1, 2 ** 32)] == \
        [1, 1, 1, 1, 1, 2, 2, 3, 4, 5, 10, 11, 16]
    for n in PERM_SIZES:
        half, mask = G.feistel_geometry(n)
        assert mask == (1 << half) - 1 and n <= 1 << (2 * half) <= max(4, 4 * (n - 1))


@pytest.mark.parametrize("n", PERM_SIZES)
def test_feistel_is_a_bijection_and_inv_undoes_it(n):
    x = np.arange(n, dtype=np.uint64)
    for seed in (G.SEED_R, 0, 2 ** 64 - 1):
        st = {}
        y = G.feistel_perm(x, n, seed, stats=st)
        assert y.dtype == np.uint64 and np.array_equal(np.sort(y), x), seed
        assert np.array_equal(G.feistel_inv(y, n, seed), x), seed
        assert np.array_equal(G.feistel_perm(G.feistel_inv(x, n, seed), n, seed), x), seed
        if n > 16:
            assert not np.array_equal(y, x)
        if seed == G.SEED_R:
            assert st.get("walk_rounds", 0) <= 53  # (cycle walking over at most a 4x domain)


def test_feistel_by_hand():
    """n = 3 works on 2 bits (half = 1): every round is L, R = R, L ^ (mix64(R ^ key) & 1), spelled out with
    the host ABI's scalar mix64."""
    import hj3d
    n, seed = 3, G.SEED_R

    def enc(x):
        L, R = x >> 1, x & 1
        for k in range(4):
            L, R = R, L ^ (hj3d.mix64(R ^ ((seed + 0x9e3779b97f4a7c15 * (k + 1)) & G.M64)) & 1)
        return (L << 1) | R

    want = []
    for x in range(n):
        y = enc(x)
        while y >= n:
            y = enc(y)
        want.append(y)
    assert G.feistel_perm(np.arange(n), n, seed).tolist() == want


def test_gen_keys_and_gen_fk_definitions():
    import hj3d
    assert G.gen_keys(10, 2 ** 32 - 5, 0, 0).tolist() == [(2 ** 32 - 5 + i) & 0xFFFFFFFF for i in range(10)]
    assert G.gen_keys(0, 0, 7, 1).shape == (0,) and G.gen_keys(4, 0, 1, 9).tolist() == [0] * 4
    whole = G.gen_keys(257, 0, 257, 5)
    assert np.array_equal(np.concatenate([G.gen_keys(100, 0, 257, 5), G.gen_keys(157, 100, 257, 5)]), whole)
    for fk_max in (1, 3, 1000, 2 ** 31, 2 ** 32 - 1):
        got = G.gen_fk(50, 2 ** 40, fk_max, G.SEED_S)
        assert got.tolist() == [((hj3d.mix64((2 ** 40 + i) ^ G.SEED_S) >> 32) * fk_max) >> 32 for i in range(50)]
        assert (got.astype(np.int64) < fk_max).all()


def _key_fk_case():
    """As tests/test_gpu_streams.py builds it: R.k a permutation of [0, nk), S.a uniform over it."""
    rng = np.random.default_rng(12)
    nk = 1024
    R = O.tuples3(rng.permutation(nk), np.zeros(nk))
    S = O.tuples3(np.arange(3 * nk), rng.integers(0, nk, 3 * nk))
    return nk, R, S


def test_expected_fk_equals_oracle_both_orientations():
    nk, R, S = _key_fk_case()
    e = O.chain_plan(R, 0, S, 1, nk, True).out
    got = G.expected_fk(R[:, 0], np.arange(nk), S[:, 1], np.arange(len(S)), nk, False)
    assert got == {f: e[f] for f in G.FIELDS} and got["n"] == len(S)
    # swap: the same pair set with a and b exchanged. Sums change places; the hashes are those of the
    # exchanged pairs, taken from the oracle's probe in the other direction (build on S.a, probe with R.k)
    e2 = O.chain_plan(S, 1, R, 0, nk, False).out
    assert (e2["n"], e2["sum_a"], e2["sum_b"]) == (e["n"], e["sum_b"], e["sum_a"])
    got = G.expected_fk(R[:, 0], np.arange(nk), S[:, 1], np.arange(len(S)), nk, True)
    assert got == {f: e2[f] for f in G.FIELDS}


def test_expected_fk_by_hand():
    import hj3d
    bk, br = [2, 0, 5, 9], [10, 11, 12, 13]  # key 9 is outside the domain of 6 keys; keys 1, 3, 4 have no row
    pk, pr = [0, 1, 2, 5, 5, 9, 6], [20, 21, 22, 23, 24, 25, 26]
    pairs = [(20, 11), (22, 10), (23, 12), (24, 12)]
    for swap in (False, True):
        ps = [(b, a) for a, b in pairs] if swap else pairs
        hs = [hj3d.pair_hash(a, b) for a, b in ps]
        x = 0
        for h in hs:
            x ^= h
        assert G.expected_fk(bk, br, pk, pr, 6, swap) == {
            "n": 4, "sum_a": sum(a for a, _ in ps), "sum_b": sum(b for _, b in ps), "sum_h": sum(hs) & G.M64, "xor_h": x}
    zero = {f: 0 for f in G.FIELDS}
    assert G.expected_fk(bk, br, pk, pr, 0, False) == zero
    assert G.expected_fk([], [], pk, pr, 6, False) == zero and G.expected_fk(bk, br, [], [], 6, True) == zero
    # sums wrap mod 2^64; parts add up
    big = G.fold(np.full(5, 2 ** 32 - 1, np.uint64), np.arange(5))
    assert big["sum_a"] == 5 * (2 ** 32 - 1)
    a, b = np.arange(10), np.arange(10) * 7
    assert G.add(G.fold(a[:3], b[:3]), G.fold(a[3:], b[3:])) == G.fold(a, b)


# ---- Zipf ----

def test_zipf_pmf():
    p = G.zipf_pmf(1000, 0.8)
    assert abs(p.sum() - 1.0) < 1e-12 and (np.diff(p) < 0).all()
    assert np.allclose(p[:3] / p[0], [1.0, 2.0 ** -0.8, 3.0 ** -0.8], rtol=1e-14)
    assert G.zipf_pmf(1, 2.0).tolist() == [1.0]
    e = G.zipf_bins(1_000_000)
    assert e[0] == 0 and e[-1] == 1_000_000 and len(e) == 16 + 24 + 1 and (np.diff(e) > 0).all()
    assert e[:17].tolist() == list(range(17))


def test_zipf_constants_by_hand():
    """theta = 2: H(x) = 1 - 1/x, h(x) = x^-2, H^-1(u) = 1 / (1 - u), in closed form."""
    z = G._Zipf(1000, 2.0)
    assert z.hx1 == pytest.approx(1 - 1 / 1.5 - 1, rel=1e-14) and z.hn == pytest.approx(1 - 1 / 1000.5, rel=1e-14)
    assert z.s == pytest.approx(2 - 1 / (1 - (1 - 1 / 2.5 - 0.25)), rel=1e-13)
    # theta = 1 takes the series branches: H = log, H^-1 = exp
    z = G._Zipf(1000, 1.0)
    assert z.hn == pytest.approx(np.log(1000.5), rel=1e-15) and z.s == pytest.approx(2 - np.exp(np.log(2.5) - 0.5), rel=1e-14)
    x = np.array([1.5, 7.25, 900.0])
    assert np.allclose(z.Hinv(z.H(x)), x, rtol=1e-13)
    for theta in (0.05, 0.8, 1 + 1e-9, 1 - 1e-12):
        z = G._Zipf(1000, theta)
        assert np.allclose(z.Hinv(z.H(x)), x, rtol=1e-9), theta
    z = G._Zipf(1000, 10.0)  # (H is flat within an ulp from x ~ 50 on: only small x come back)
    assert np.allclose(z.Hinv(z.H(x[:2])), x[:2], rtol=1e-6)


@pytest.mark.parametrize("fk_max,theta", G.ZIPF_SMALL_CASES)
def test_zipf_undecided_share_is_capped(fk_max, theta):
    """The per-row device comparison skips undecided rows, so their share must stay negligible: at most
    1e-4 of each case's rows (measured: none in any case)."""
    val, und = G.zipf_small_case(fk_max, theta)
    share = und.mean()
    print(f"fk_max={fk_max} theta={theta!r}: undecided {int(und.sum())} of {len(und)} rows ({share:.2e})")
    assert share <= 1e-4
    assert (val.astype(np.int64) < fk_max).all()
    # a rank's rows are the matching slice of the whole relation
    lo, n = 77_001, 5000
    v2, u2 = G.gen_zipf(n, lo, fk_max, theta, G.SEED_S)
    assert np.array_equal(v2, val[lo: lo + n]) and np.array_equal(u2, und[lo: lo + n])
    # ... and the sample follows the pmf
    cnt, mean, bound = G.zipf_bin_deviation(val, fk_max, theta)
    assert (np.abs(cnt - mean) < bound).all(), (cnt, mean)


@pytest.mark.parametrize("theta", G.ZIPF_DIST_THETAS)
def test_zipf_model_histogram_follows_pmf(theta):
    """The model's own sample at the distribution test's shape, head and tail (5-sigma bounds)."""
    val, und = G.gen_zipf(G.ZIPF_DIST_N, 0, G.ZIPF_DIST_FK_MAX, theta, G.SEED_S)
    cnt, mean, bound = G.zipf_bin_deviation(val, G.ZIPF_DIST_FK_MAX, theta)
    assert len(cnt) == 40 and (np.abs(cnt - mean) < bound).all(), (cnt, mean)


def test_zipf_model_widest_domain():
    val, _ = G.gen_zipf(G.ZIPF_SMALL_N, 0, 2 ** 32 - 1, 0.5, G.SEED_S)
    assert int(val.max()) == 4294907786 and int(val.min()) >= 0
