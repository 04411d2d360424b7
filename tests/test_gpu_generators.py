"""The device generators (hj3d_gen_keys / hj3d_gen_fk / hj3d_gen_zipf) and the key/FK verifier
(hj3d_expected_fk_join / hj3d_expected_fk_join_gen) against tests/gen_model.py, the plain numpy model that
tests/test_gen_model.py pins on the CPU.

Full-size runs are accepted when a probe's aggregates equal the verifier's on generated relations, so here
the verifier itself is verified: the generators bit-exactly (Zipf: on every row whose floating-point decisions
are not within 1e-9 of flipping, and as a distribution), the verifier against a brute-force join in both
orientations, with keys outside the domain, explicit and based row ids, more than one grid round,
accumulation over shards and a build side that holds only part of the key domain.

Every buffer starts as a sentinel word, so a stray write shows."""
import ctypes as C

import numpy as np
import pytest

import gen_model as G

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5
SEEDS = (0, G.SEED_R, 2 ** 64 - 1)
N_ROUNDS = 2 ** 20 + 257  # the generators launch at most 4096 workgroups of 256: the smallest n with a second round
ZERO = {f: 0 for f in G.FIELDS}


def sentinel(rows, words):
    import torch
    return torch.from_numpy(np.full((rows, words), SENT, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def cuts(n):
    """Three uneven shards [lo, hi) of n rows (empty ones where n is tiny)."""
    a, b = n // 5, n - n // 3
    return [(0, a), (a, b), (b, n)]


def column(gen, n, words=3, word=1, shards=None):
    """Column `word` of n sentinel tuples after gen(tensor, word, row_base), whole or shard by shard; every
    other word must still be the sentinel."""
    t = sentinel(n, words)
    for lo, hi in shards or [(0, n)]:
        gen(t[lo:hi], word, lo)
    h = host(t)
    other = np.delete(h, word, axis=1)
    assert (other == SENT).all()
    return h[:, word]


GENERATORS = {
    "keys": (lambda ctx: lambda t, w, base: ctx.gen_keys(t, w, base, 1000, G.SEED_R),
             lambda n, base: G.gen_keys(n, base, 1000, G.SEED_R)),
    "identity": (lambda ctx: lambda t, w, base: ctx.gen_keys(t, w, base, 0, 0),
                 lambda n, base: G.gen_keys(n, base, 0, 0)),
    "fk": (lambda ctx: lambda t, w, base: ctx.gen_fk(t, w, base, 1000, G.SEED_S),
           lambda n, base: G.gen_fk(n, base, 1000, G.SEED_S)),
    "zipf": (lambda ctx: lambda t, w, base: ctx.gen_zipf(t, w, base, 1000, 0.8, G.SEED_S),
             lambda n, base: G.zipf_small_case(1000, 0.8)[0][base: base + n]),
}
LAYOUTS = [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 3), (5, 0), (5, 2), (5, 4)]


@pytest.mark.parametrize("name", list(GENERATORS))
def test_layout_and_noop(ctx, name):
    """Tuples of 2 .. 5 words with the key first, in the middle and last, in a slice that starts one tuple
    into its buffer (8, 12, 16, 20 bytes: 16-B aligned only for 4 words): the key column is the model's, every
    other word and the rows around the slice keep the sentinel. n = 0 writes nothing."""
    gen, model = GENERATORS[name][0](ctx), GENERATORS[name][1]
    n, base = 777, 123
    und = G.zipf_small_case(1000, 0.8)[1][base: base + n]
    for words, word in LAYOUTS:
        buf = sentinel(n + 2, words)
        gen(buf[1: n + 1], word, base)
        h = host(buf)
        assert (h[0] == SENT).all() and (h[n + 1] == SENT).all(), (words, word)
        assert (np.delete(h[1: n + 1], word, axis=1) == SENT).all(), (words, word)
        got, want = h[1: n + 1, word], model(n, base)
        assert not (got == SENT).any()
        ok = und | (got == want) if name == "zipf" else got == want
        assert ok.all(), (words, word)
        gen(buf[1:1], word, base)
        gen(buf[n + 2:], word, base)
        assert np.array_equal(host(buf), h), (words, word)


# ---- gen_keys ----

@pytest.mark.parametrize("n_keys", [1, 2, 3, 5, 17, 257, 65537, 2 ** 20 + 1, N_ROUNDS])
def test_gen_keys_is_the_models_permutation(ctx, n_keys):
    """Bit-exact against the model; a permutation of [0, n_keys); the rows a rank generates (row_base) are the
    matching slice of the whole relation."""
    for seed in SEEDS if n_keys != N_ROUNDS else (G.SEED_R,):
        def gen(t, w, base):
            ctx.gen_keys(t, w, base, n_keys, seed)
        whole = column(gen, n_keys)
        assert np.array_equal(whole, G.gen_keys(n_keys, 0, n_keys, seed)), seed
        assert np.array_equal(np.sort(whole), np.arange(n_keys, dtype=np.uint32)), seed
        assert np.array_equal(column(gen, n_keys, shards=cuts(n_keys)), whole), seed


def test_gen_keys_identity_wraps_to_32_bits(ctx):
    def gen(t, w, base):
        ctx.gen_keys(t, w, base, 0, 99)
    assert column(gen, 10).tolist() == list(range(10))
    t = sentinel(10, 2)
    ctx.gen_keys(t, 1, 2 ** 32 - 5, 0, 99)
    h = host(t)
    assert h[:, 1].tolist() == [(2 ** 32 - 5 + i) & 0xFFFFFFFF for i in range(10)] == G.gen_keys(10, 2 ** 32 - 5, 0, 99).tolist()
    assert (h[:, 0] == SENT).all()
    big = column(gen, N_ROUNDS, shards=cuts(N_ROUNDS))
    assert np.array_equal(big, np.arange(N_ROUNDS, dtype=np.uint32))


# ---- gen_fk ----

@pytest.mark.parametrize("fk_max", [1, 2, 3, 1000, 2 ** 31, 2 ** 32 - 1])
def test_gen_fk_is_the_models_column(ctx, fk_max):
    def gen(t, w, base):
        ctx.gen_fk(t, w, base, fk_max, G.SEED_S)
    n = N_ROUNDS
    whole = column(gen, n)
    assert np.array_equal(whole, G.gen_fk(n, 0, fk_max, G.SEED_S))
    assert int(whole.max()) < fk_max
    if fk_max == 2 ** 32 - 1:
        assert int(whole.max()) >= 2 ** 31  # (a signed clamp or multiply would lose these)
    if fk_max >= 1000:
        assert len(np.unique(whole)) > 990
    assert np.array_equal(column(gen, n, shards=cuts(n)), whole)
    # another seed and a row_base past 2^32 give the model's other columns
    t = sentinel(1000, 2)
    ctx.gen_fk(t, 0, 2 ** 40 + 3, fk_max, 2 ** 64 - 1)
    assert np.array_equal(host(t)[:, 0], G.gen_fk(1000, 2 ** 40 + 3, fk_max, 2 ** 64 - 1))


# ---- gen_zipf ----

@pytest.mark.parametrize("fk_max,theta", G.ZIPF_SMALL_CASES)
def test_gen_zipf_rows_equal_the_model(ctx, fk_max, theta):
    """Per row, on every row that is not undecided (tests/test_gen_model.py caps their share at 1e-4 per
    case; there are none); an undecided row only has to lie in the domain."""
    def gen(t, w, base):
        ctx.gen_zipf(t, w, base, fk_max, theta, G.SEED_S)
    want, und = G.zipf_small_case(fk_max, theta)
    n = len(want)
    whole = column(gen, n)
    bad = int(((whole != want) & ~und).sum())
    print(f"gen_zipf fk_max={fk_max} theta={theta!r}: {bad} mismatches on {int((~und).sum())} decided rows, "
          f"{int(und.sum())} undecided")
    assert bad == 0
    assert int(whole.max()) < fk_max
    assert np.array_equal(column(gen, n, shards=cuts(n)), whole)


@pytest.mark.parametrize("theta", G.ZIPF_DIST_THETAS)
def test_gen_zipf_distribution_head_and_tail(ctx, theta):
    """fk_max = 1e6, 2e6 rows: the counts of the 16 most frequent values and of 24 log-spaced bins over the rest
    of the domain lie within 5 sd + 1 of N p, p from the exact pmf (the bound of test_device_zipf_matches_pmf)."""
    def gen(t, w, base):
        ctx.gen_zipf(t, w, base, G.ZIPF_DIST_FK_MAX, theta, G.SEED_S)
    val = column(gen, G.ZIPF_DIST_N)
    assert int(val.max()) < G.ZIPF_DIST_FK_MAX
    cnt, mean, bound = G.zipf_bin_deviation(val, G.ZIPF_DIST_FK_MAX, theta)
    assert len(cnt) == 40
    assert (np.abs(cnt - mean) < bound).all(), (cnt, mean, bound)


def test_gen_zipf_widest_domain(ctx):
    def gen(t, w, base):
        ctx.gen_zipf(t, w, base, 2 ** 32 - 1, 0.5, G.SEED_S)
    val = column(gen, G.ZIPF_SMALL_N)
    assert int(val.max()) < 2 ** 32 - 1 and int(val.max()) >= 2 ** 31
    assert len(np.unique(val)) > 0.99 * len(val)


# ---- arguments the entries reject before any launch ----

def test_generators_reject_bad_arguments(ctx):
    import hj3d
    t = sentinel(64, 3)
    bad = [lambda: ctx.gen_fk(t, 1, 0, 0, 1),
           lambda: ctx.gen_zipf(t, 1, 0, 0, 0.8, 1),
           lambda: ctx.gen_zipf(t, 1, 0, 100, 0.0, 1),
           lambda: ctx.gen_zipf(t, 1, 0, 100, -0.5, 1),
           lambda: ctx.gen_zipf(t, 1, 0, 100, 10.0 + 1e-9, 1),
           lambda: ctx.gen_zipf(t, 1, 0, 100, float("inf"), 1),
           lambda: ctx.gen_zipf(t, 1, 0, 100, float("nan"), 1),
           lambda: ctx.expected_fk_join_gen(hj3d.Rel(t, 1), 0, 1)]
    for k, call in enumerate(bad):
        with pytest.raises(hj3d.Hj3dError) as e:
            call()
        assert e.value.status == hj3d.HJ3D_EINVAL, k
    ctx.sync()
    assert (host(t) == SENT).all()


# ---- expected_fk_join ----

def expect(ctx, build, probe, n_keys, swap, res=None):
    """hj3d_expected_fk_join by the raw entry, accumulating into `res` (a device int64[8]) when given."""
    import torch
    import hj3d
    r = res if res is not None else torch.zeros(8, dtype=torch.int64, device="cuda")
    st = hj3d.lib().hj3d_expected_fk_join(ctx.h, C.byref(build.c), C.byref(probe.c), n_keys, int(swap), r.data_ptr())
    assert st == hj3d.HJ3D_OK
    if res is not None:
        return None
    ctx.sync()
    return fields(r)


def fields(res):
    v = [int(x) & G.M64 for x in res.cpu().tolist()]
    assert v[5:] == [0, 0, 0]
    return dict(zip(G.FIELDS, v))


def rel2(keys, rows=None):
    """{key, row} tuples; without rows the second word is the sentinel (implicit rows)."""
    t = np.full((len(keys), 2), SENT, dtype=np.uint32)
    t[:, 0] = keys
    if rows is not None:
        t[:, 1] = rows
    return t


def check_join(ctx, bk, pk, n_keys, br=None, pr=None, p_base=0):
    """Device expectation == brute-force join, both orientations, through the wrapper and the raw entry."""
    import hj3d
    dB, dP = dev(rel2(bk, br)), dev(rel2(pk, pr))
    B = hj3d.Rel(dB, 0, None if br is None else 1)
    P = hj3d.Rel(dP, 0, None if pr is None else 1, row_base=p_base)
    out = {}
    for swap in (False, True):
        want = G.expected_fk(bk, np.arange(len(bk)) if br is None else br, pk,
                             np.arange(len(pk)) + p_base if pr is None else pr, n_keys, swap)
        got = ctx.expected_fk_join(B, P, n_keys, swap=swap)
        assert got == want, (swap, got, want)
        assert expect(ctx, B, P, n_keys, swap) == want, swap
        out[swap] = got
    assert np.array_equal(host(dB), rel2(bk, br)) and np.array_equal(host(dP), rel2(pk, pr))
    return out


NK = 4099


@pytest.fixture(scope="module")
def keyfk():
    """n_keys = 4099: R.k a permutation of the domain; 20 011 probe keys over [0, 1.25 n_keys), a fifth of
    them outside the domain."""
    rng = np.random.default_rng(4099)
    bk = rng.permutation(NK).astype(np.uint32)
    pk = rng.integers(0, NK + NK // 4, 20_011).astype(np.uint32)
    assert 0.17 < (pk >= NK).mean() < 0.23
    bk.setflags(write=False)
    pk.setflags(write=False)
    return bk, pk


@pytest.mark.parametrize("n_keys", [1, 2, 7])
def test_expected_tiny_domains(ctx, n_keys):
    rng = np.random.default_rng(n_keys)
    bk = rng.permutation(n_keys)
    pk = rng.integers(0, n_keys + 2, 50)
    got = check_join(ctx, bk, pk, n_keys)
    assert 0 < got[False]["n"] == int((pk < n_keys).sum()) < 50
    assert check_join(ctx, bk, pk[:0], n_keys)[True] == ZERO   # a probe of 0 rows
    assert check_join(ctx, bk[:0], pk[:0], n_keys)[False] == ZERO  # ... and a build of 0 rows with it
    assert check_join(ctx, bk, pk, 0)[False] == ZERO           # an empty domain: every key is outside


def test_expected_skips_keys_outside_the_domain(ctx, keyfk):
    bk, pk = keyfk
    got = check_join(ctx, bk, pk, NK)
    assert got[False]["n"] == int((pk < NK).sum()) < len(pk)
    assert (got[True]["n"], got[True]["sum_a"], got[True]["sum_b"]) == \
        (got[False]["n"], got[False]["sum_b"], got[False]["sum_a"])


def test_expected_explicit_and_based_rows(ctx, keyfk):
    """Row ids from a row word (a random permutation plus an offset above 2^31) on both sides, and implicit
    rows with row_base on a slice of the probe; the two forms agree where they name the same rows."""
    import hj3d
    bk, pk = keyfk
    rng = np.random.default_rng(7)
    br = (rng.permutation(NK) + 2 ** 31 + 12_345).astype(np.uint32)
    pr = (rng.permutation(len(pk)) + 2 ** 32 - len(pk) - 1).astype(np.uint32)
    got = check_join(ctx, bk, pk, NK, br=br, pr=pr)
    assert got[False]["sum_b"] >= got[False]["n"] * 2 ** 31
    lo, hi = 3001, 17_770
    base = 2 ** 32 - hi  # the slice's last row is 2^32 - 1
    based = check_join(ctx, bk, pk[lo:hi], NK, p_base=base + lo)
    named = check_join(ctx, bk, pk[lo:hi], NK, pr=np.arange(base + lo, base + hi))
    assert based == named
    # ... also as a slice of the whole probe tensor (a base that is not 16-B aligned)
    dB, dP = dev(rel2(bk)), dev(rel2(pk))
    sl = hj3d.Rel(dP[lo:hi], 0, row_base=base + lo)
    for swap in (False, True):
        assert ctx.expected_fk_join(hj3d.Rel(dB, 0), sl, NK, swap=swap) == based[swap]


def test_expected_past_one_grid_round(ctx, keyfk):
    """600 001 probe rows: the expectation kernels launch at most 8 workgroups of 256 per CU, so on up to 292 CUs
    the grid-stride loop takes a second round and the per-block sums carry over it."""
    import torch
    n = 600_001
    assert torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 < n
    bk, _ = keyfk
    pk = np.random.default_rng(600).integers(0, NK + NK // 4, n).astype(np.uint32)
    got = check_join(ctx, bk, pk, NK)
    assert got[False]["n"] == int((pk < NK).sum())


def test_expected_accumulates_into_res(ctx, keyfk):
    """Two calls for the two halves of the probe into one result == one call for the whole."""
    import torch
    import hj3d
    bk, pk = keyfk
    dB, dP = dev(rel2(bk)), dev(rel2(pk))
    B, half = hj3d.Rel(dB, 0), len(pk) // 2 + 1
    for swap in (False, True):
        want = G.expected_fk(bk, np.arange(NK), pk, np.arange(len(pk)), NK, swap)
        res = torch.zeros(8, dtype=torch.int64, device="cuda")
        expect(ctx, B, hj3d.Rel(dP[:half], 0), NK, swap, res)
        expect(ctx, B, hj3d.Rel(dP[half:], 0, row_base=half), NK, swap, res)
        ctx.sync()
        assert fields(res) == want == expect(ctx, B, hj3d.Rel(dP, 0), NK, swap), swap
        parts = [G.expected_fk(bk, np.arange(NK), pk[a:b], np.arange(a, b), NK, swap) for a, b in ((0, half), (half, len(pk)))]
        assert G.add(*parts) == want


def test_expected_with_a_partial_build_side(ctx, keyfk):
    """R holds 3000 of the 4099 keys of the domain (a rank's shard, an R shorter than n_keys): the expectation
    is the true join, so probe keys without a partner contribute nothing. (They used to count as pairs with
    build row 0xFFFFFFFF.) The same with no build row at all."""
    bk, pk = keyfk
    part = bk[:3000]
    got = check_join(ctx, part, pk, NK)
    held = np.isin(pk, part)
    assert got[False]["n"] == int(held.sum()) < int((pk < NK).sum())
    rng = np.random.default_rng(3000)
    br = (rng.permutation(3000) + 2 ** 31).astype(np.uint32)
    check_join(ctx, part, pk, NK, br=br, pr=np.arange(len(pk)) + 5)
    assert check_join(ctx, bk[:0], pk, NK)[False] == ZERO


# ---- expected_fk_join_gen ----

@pytest.mark.parametrize("n_keys,n_probe", [(1, 5000), (2, 5000), (17, 5000), (65537, 50_000), (2 ** 20 + 1, 300_000)])
def test_expected_gen_equals_the_join_on_generated_keys(ctx, n_keys, n_probe):
    """For build keys made by gen_keys(n_keys, seed): equal to expected_fk_join on that relation and to the
    model's brute-force join on the model's keys, both orientations; three probe shards summed into one
    result equal the whole."""
    import torch
    import hj3d
    seed = G.SEED_R
    rng = np.random.default_rng(n_keys)
    pk = rng.integers(0, n_keys + n_keys // 4 + 2, n_probe).astype(np.uint32)
    dR = sentinel(n_keys, 3)
    ctx.gen_keys(dR, 0, 0, n_keys, seed)
    dP = dev(rel2(pk))
    bk = G.gen_keys(n_keys, 0, n_keys, seed)
    B, P = hj3d.Rel(dR, 0), hj3d.Rel(dP, 0)
    for swap in (False, True):
        want = G.expected_fk(bk, np.arange(n_keys), pk, np.arange(n_probe), n_keys, swap)
        assert want["n"] == int((pk < n_keys).sum()) > 0
        got = ctx.expected_fk_join_gen(P, n_keys, seed, swap=swap)
        assert got == want, swap
        assert ctx.expected_fk_join(B, P, n_keys, swap=swap) == want, swap
        res = torch.zeros(8, dtype=torch.int64, device="cuda")
        for lo, hi in cuts(n_probe):
            assert ctx.expected_fk_join_gen(hj3d.Rel(dP[lo:hi], 0, row_base=lo), n_keys, seed, swap=swap, res=res) is None
        ctx.sync()
        assert fields(res) == want, swap
    # another seed is another permutation
    bk = G.gen_keys(n_keys, 0, n_keys, 2 ** 64 - 1)
    assert ctx.expected_fk_join_gen(P, n_keys, 2 ** 64 - 1) == G.expected_fk(bk, np.arange(n_keys), pk, np.arange(n_probe), n_keys, False)
    assert np.array_equal(host(dP), rel2(pk))
