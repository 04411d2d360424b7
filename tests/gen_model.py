"""What the device generators and the key/FK verifier must produce, in plain numpy (a helper module for
the tests, not a conftest).

hj3d_gen_keys, hj3d_gen_fk and hj3d_gen_zipf make the relations of every full-size run, and
hj3d_expected_fk_join / hj3d_expected_fk_join_gen decide "verified" where no fixture exists. This module
restates each of them from its definition alone:

  mix64 / pair_hash   splitmix64's finaliser; pair_hash(a, b) = mix64(a << 32 | b)
  feistel_perm / inv  4-round Feistel network over the smallest even-bit domain >= n, round function
                      mix64(x ^ (seed + golden * (round + 1))) & mask, cycle walking back into [0, n)
  gen_keys            key of global row g = feistel_perm(g) (identity when n_keys == 0), as u32
  gen_fk              ((mix64(g ^ seed) >> 32) * fk_max) >> 32
  gen_zipf            rejection-inversion (Hoermann & Derflinger 1996) in float64 over {1 .. fk_max}, minus 1,
                      attempt c of row g drawing from mix64(mix64(g ^ seed) ^ (c * golden + 0x632BE59BD9B4E019))
  zipf_pmf            the exact normalised (v + 1)^-theta
  expected_fk         a brute-force equi-join (sort + searchsorted: no inverse array, no 0xFFFFFFFF
                      convention) folded into {n, sum_a, sum_b, sum_h, xor_h} mod 2^64

The Zipf sampler takes three decisions per attempt in floating point (the rounding of x to k, the
squeeze k - x <= s, the acceptance u >= H(k + 1/2) - h(k)). Two correct implementations whose exp / log
differ by a few ulp can decide differently only when a decision is within those few ulp of flipping, so
gen_zipf also returns the rows with such an attempt ("undecided", margin ZIPF_MARGIN = 1e-9: about five
orders above an ulp-level error at x <= 1000). A device value is compared with the model on every other
row. tests/test_gen_model.py caps the share of undecided rows and pins the rest of this module on the
CPU before tests/test_gpu_generators.py judges a kernel with it.

Host only (numpy)."""
import functools

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ZIPF_STREAM = 0x632BE59BD9B4E019
ZIPF_MARGIN = 1e-9
ROUNDS = 4  # of the Feistel network
FIELDS = ("n", "sum_a", "sum_b", "sum_h", "xor_h")

SEED_R, SEED_S = 0x5eed0001, 0x5eed0002

# the cases tests/test_gpu_generators.py compares per row (and tests/test_gen_model.py caps the undecided share of)
ZIPF_SMALL_N = 200_000
ZIPF_SMALL_CASES = [(fk_max, theta) for fk_max in (1, 2, 3, 1000)
                    for theta in (0.05, 0.8, 1.0, 1.0 + 1e-9, 1.0 - 1e-12, 2.0, 10.0)]
# ... and the distribution cases
ZIPF_DIST_N, ZIPF_DIST_FK_MAX, ZIPF_DIST_THETAS = 2_000_000, 1_000_000, (0.8, 1.0, 2.0)


def _u64(x):
    """x (ints below 2^64 or an integer array) as a uint64 array of at least one dimension."""
    if isinstance(x, np.ndarray) and x.dtype == np.uint64:
        return np.atleast_1d(x)
    if isinstance(x, np.ndarray) and x.dtype.kind == "i":
        return np.atleast_1d(x.astype(np.int64).view(np.uint64))
    if isinstance(x, np.ndarray):
        return np.atleast_1d(x.astype(np.uint64))
    return np.atleast_1d(np.array(x, dtype=np.uint64))


def _c(v: int):
    return np.uint64(v & M64)


def mix64(z):
    z = _u64(z)
    z = (z ^ (z >> _c(30))) * _c(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> _c(27))) * _c(0x94d049bb133111eb)
    return z ^ (z >> _c(31))


def pair_hash(a, b):
    return mix64(((_u64(a) & _c(0xFFFFFFFF)) << _c(32)) | (_u64(b) & _c(0xFFFFFFFF)))


# ---- the key permutation ----

def feistel_geometry(n: int):
    """(half, mask): the network works on 2 * half bits, the smallest even bit count >= log2(n)."""
    bits = 0
    while bits < 64 and (1 << bits) < n:
        bits += 1
    half = max((bits + 1) // 2, 1)
    return half, (1 << half) - 1


def _round_fn(x, k, seed, mask):
    return mix64(x ^ _c(seed + GOLDEN * (k + 1))) & _c(mask)


def _enc1(x, half, mask, seed):
    L, R = x >> _c(half), x & _c(mask)
    for k in range(ROUNDS):
        L, R = R, L ^ _round_fn(R, k, seed, mask)
    return (L << _c(half)) | R


def _dec1(x, half, mask, seed):
    L, R = x >> _c(half), x & _c(mask)
    for k in reversed(range(ROUNDS)):
        L, R = R ^ _round_fn(L, k, seed, mask), L
    return (L << _c(half)) | R


def _walk(step, x, n, stats):
    """step(x), repeated on every element that fell outside [0, n) until it is back (cycle walking)."""
    y = step(x)
    rounds = 0
    out = np.flatnonzero(y >= _c(n))
    while len(out):
        y[out] = step(y[out])
        out = out[y[out] >= _c(n)]
        rounds += 1
    if stats is not None:
        stats["walk_rounds"] = max(stats.get("walk_rounds", 0), rounds)
    return y


def feistel_perm(x, n: int, seed: int, stats=None):
    """The image of x (values in [0, n)) under the seeded permutation of [0, n)."""
    x = _u64(x).copy()
    if n <= 1:
        return np.zeros_like(x)
    assert (x < _c(n)).all(), "only points of [0, n) are on a cycle that is known to return there"
    half, mask = feistel_geometry(n)
    return _walk(lambda v: _enc1(v, half, mask, seed), x, n, stats)


def feistel_inv(y, n: int, seed: int, stats=None):
    y = _u64(y).copy()
    if n <= 1:
        return np.zeros_like(y)
    assert (y < _c(n)).all()
    half, mask = feistel_geometry(n)
    return _walk(lambda v: _dec1(v, half, mask, seed), y, n, stats)


def _global_rows(n: int, row_base: int):
    return np.arange(n, dtype=np.uint64) + _c(row_base)  # (wraps mod 2^64 like the kernel's row_base + i)


def gen_keys(n: int, row_base: int, n_keys: int, seed: int) -> np.ndarray:
    g = _global_rows(n, row_base)
    k = g if n_keys == 0 else feistel_perm(g, n_keys, seed)
    return (k & _c(0xFFFFFFFF)).astype(np.uint32)


def gen_fk(n: int, row_base: int, fk_max: int, seed: int) -> np.ndarray:
    x = mix64(_global_rows(n, row_base) ^ _c(seed))
    return ((((x >> _c(32)) * _c(fk_max)) >> _c(32)) & _c(0xFFFFFFFF)).astype(np.uint32)


# ---- Zipf by rejection-inversion ----

class _Zipf:
    def __init__(self, fk_max: int, theta: float):
        self.q, self.n = float(theta), float(fk_max)
        one = np.ones(1)
        self.hx1 = float(self.H(1.5 * one)[0] - 1.0)
        self.hn = float(self.H((self.n + 0.5) * one)[0])
        self.s = float(2.0 - self.Hinv(self.H(2.5 * one) - self.h(2.0 * one))[0])

    @staticmethod
    def helper1(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.abs(x) > 1e-8, np.log1p(x) / x, 1.0 - x * (0.5 - x * (1.0 / 3.0 - 0.25 * x)))

    @staticmethod
    def helper2(x):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(np.abs(x) > 1e-8, np.expm1(x) / x, 1.0 + x * 0.5 * (1.0 + x * (1.0 / 3.0) * (1.0 + 0.25 * x)))

    def h(self, x):
        return np.exp(-self.q * np.log(x))

    def H(self, x):
        lx = np.log(x)
        return self.helper2((1.0 - self.q) * lx) * lx

    def Hinv(self, x):
        t = np.maximum(x * (1.0 - self.q), -1.0)
        with np.errstate(over="ignore"):
            return np.exp(self.helper1(t) * x)


def gen_zipf(n: int, row_base: int, fk_max: int, theta: float, seed: int, stats=None):
    """(values in [0, fk_max) as u32, undecided mask): see the module text."""
    z = _Zipf(fk_max, theta)
    key = mix64(_global_rows(n, row_base) ^ _c(seed))
    val = np.zeros(n, dtype=np.uint32)
    undecided = np.zeros(n, dtype=bool)
    todo = np.arange(n)
    c = 0
    while len(todo):
        r = mix64(key[todo] ^ _c(c * GOLDEN + ZIPF_STREAM))
        u01 = (r >> _c(11)).astype(np.float64) * 2.0 ** -53
        u = z.hn + u01 * (z.hx1 - z.hn)
        x = z.Hinv(u)
        xr = x + 0.5
        k = np.clip(np.floor(xr), 1.0, z.n)
        squeeze = k - x <= z.s
        edge = z.H(k + 0.5) - z.h(k)
        accept = squeeze | (u >= edge)
        frac = xr - np.floor(xr)
        tol = ZIPF_MARGIN * np.maximum(1.0, x)
        close = (frac < tol) | (frac > 1.0 - tol) | (np.abs(k - x - z.s) < ZIPF_MARGIN)
        close |= ~squeeze & (np.abs(u - edge) < ZIPF_MARGIN * np.maximum(1.0, np.abs(u)))
        undecided[todo[close]] = True
        val[todo[accept]] = (k[accept] - 1.0).astype(np.uint32)
        todo = todo[~accept]
        c += 1
    if stats is not None:
        stats["attempts"] = max(stats.get("attempts", 0), c)
    return val, undecided


@functools.lru_cache(maxsize=None)
def zipf_small_case(fk_max: int, theta: float):
    """The model's rows of one ZIPF_SMALL_CASES case (global rows 0 .. ZIPF_SMALL_N, seed SEED_S), computed once."""
    val, und = gen_zipf(ZIPF_SMALL_N, 0, fk_max, theta, SEED_S)
    val.setflags(write=False)
    und.setflags(write=False)
    return val, und


@functools.lru_cache(maxsize=4)
def zipf_pmf(fk_max: int, theta: float) -> np.ndarray:
    """P(v) = (v + 1)^-theta / sum, v in [0, fk_max), float64 (fk_max up to 1e7)."""
    assert 1 <= fk_max <= 10_000_000
    w = np.arange(1, fk_max + 1, dtype=np.float64) ** -float(theta)
    p = w / w.sum()
    p.setflags(write=False)
    return p


def zipf_bins(fk_max: int, singles: int = 16, logbins: int = 24) -> np.ndarray:
    """Bin edges over [0, fk_max): one bin per value below `singles`, then `logbins` log-spaced bins."""
    if fk_max <= singles:
        return np.arange(fk_max + 1, dtype=np.int64)
    tail = np.unique(np.round(np.geomspace(singles, fk_max, logbins + 1)).astype(np.int64))
    return np.concatenate([np.arange(singles, dtype=np.int64), tail])


def zipf_bin_deviation(values, fk_max: int, theta: float):
    """(count, N p, 5 sd + 1) per bin of zipf_bins for a sample of N values: the sample follows the pmf
    when |count - N p| < 5 sd + 1 everywhere, sd = sqrt(N p (1 - p))."""
    values = np.asarray(values).astype(np.int64)
    edges = zipf_bins(fk_max)
    cnt = np.histogram(values, bins=edges)[0].astype(np.float64)
    assert cnt.sum() == len(values), "values outside [0, fk_max)"
    cum = np.concatenate([[0.0], np.cumsum(zipf_pmf(fk_max, theta))])
    p = cum[edges[1:]] - cum[edges[:-1]]
    N = float(len(values))
    return cnt, N * p, 5.0 * np.sqrt(N * p * (1.0 - p)) + 1.0


# ---- the key/FK join ----

def fold(a, b) -> dict:
    """{n, sum_a, sum_b, sum_h, xor_h} of the pairs (a[i], b[i]), sums mod 2^64."""
    a, b = _u64(a) if len(a) else np.zeros(0, np.uint64), _u64(b) if len(b) else np.zeros(0, np.uint64)
    h = pair_hash(a, b) if len(a) else np.zeros(0, np.uint64)
    return {"n": len(a), "sum_a": int(a.sum(dtype=np.uint64)), "sum_b": int(b.sum(dtype=np.uint64)),
            "sum_h": int(h.sum(dtype=np.uint64)), "xor_h": int(np.bitwise_xor.reduce(h)) if len(h) else 0}


def add(*parts) -> dict:
    """The aggregates of a union of disjoint pair sets."""
    out = {"n": 0, "sum_a": 0, "sum_b": 0, "sum_h": 0, "xor_h": 0}
    for p in parts:
        for f in ("n", "sum_a", "sum_b", "sum_h"):
            out[f] = (out[f] + p[f]) & M64
        out["xor_h"] ^= p["xor_h"]
    return out


def expected_fk(build_keys, build_rows, probe_keys, probe_rows, n_keys: int, swap: bool) -> dict:
    """The aggregates of {(probe row, build row) : probe key == build key < n_keys} (swap: (build row,
    probe row)). Build keys are unique; a probe key that no build row holds joins with nothing."""
    bk, br = np.asarray(build_keys).astype(np.int64), np.asarray(build_rows).astype(np.int64)
    pk, pr = np.asarray(probe_keys).astype(np.int64), np.asarray(probe_rows).astype(np.int64)
    assert len(bk) == len(br) and len(pk) == len(pr)
    keep = bk < n_keys
    bk, br = bk[keep], br[keep]
    order = np.argsort(bk, kind="stable")
    sk, sr = bk[order], br[order]
    assert (np.diff(sk) > 0).all(), "build keys must be unique"
    if len(sk) == 0 or len(pk) == 0:
        return fold([], [])
    pos = np.minimum(np.searchsorted(sk, pk), len(sk) - 1)
    hit = (pk < n_keys) & (sk[pos] == pk)
    p, b = pr[hit].astype(np.uint64), sr[pos[hit]].astype(np.uint64)
    return fold(b, p) if swap else fold(p, b)
