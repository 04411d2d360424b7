"""Keys with chosen hashes (a helper module for the tests, not a conftest).

The join kernels hash every u32 key with murmur3's fmix32 (hj3d_device.hpp murmur32; the reference's
ht::murmur_hash<uint32_t>), a bijection on u32. Its inverse lets a test pick a key's hash exactly, so
the arithmetic on hashes (FastMod, FastDiv32, the packed {bucket-in-slice | h / NB} words, the LDS
aggregation table's `empty` marker) can be fed its edge values on purpose: hash 0, hash 0xFFFFFFFF,
the last incomplete quotient row h >= floor(2^32 / NB) * NB, the first and last bucket of every
slice / partition / owner range, and "identity" hashes h == bucket index. Random keys reach any one
of these points with probability ~ n / 2^32.

Host only (numpy)."""
import numpy as np

M32 = 0xFFFFFFFF
C1, C2 = 0x85EBCA6B, 0xC2B2AE35
C1_INV, C2_INV = pow(C1, -1, 1 << 32), pow(C2, -1, 1 << 32)


def _u64(x):
    return np.asarray(x).astype(np.uint64) & np.uint64(M32)


def fmix32(x):
    """murmur3 fmix32 of u32 values (array or scalar) as a numpy uint32 array."""
    h = _u64(x)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(C1)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(C2)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(16))
    return h.astype(np.uint32)


def unfmix32(h):
    """The key whose fmix32 is h: every step of fmix32 undone in reverse order (x ^= x >> 16 is its
    own inverse; x ^= x >> 13 is undone by x ^ (x >> 13) ^ (x >> 26); the odd multipliers by their
    inverses mod 2^32)."""
    x = _u64(h)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(C2_INV)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(13)) ^ (x >> np.uint64(26))
    x = (x * np.uint64(C1_INV)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def edge_buckets(nb, widths, lo=0, hi=None):
    """Sorted unique buckets in [0, nb): {0, 1, nb-1}; the last bucket of range k-1 and the first of
    range k (k*w - 1, k*w) for the second, third and last range of every width w in `widths`; and
    the buckets around an owned range [lo, hi) (lo, hi: one range, or sequences for several)."""
    s = {0, 1, nb - 1}
    for v in list(np.atleast_1d(lo)) + list(np.atleast_1d(nb if hi is None else hi)):
        s.update((int(v) - 1, int(v)))
    for w in widths:
        w = int(w)
        if w <= 0:
            continue
        for k in (1, 2, -(-nb // w) - 1):
            s.update((k * w - 1, k * w))
    return sorted(b for b in s if 0 <= b < nb)


def group_hashes(nb, b, group):
    """Up to `group` distinct hashes q * nb + b of bucket b: quotient 0, the largest quotient that
    fits in 32 bits, the others spread evenly between them."""
    qmax = (M32 - b) // nb
    q = np.unique(np.linspace(0, qmax, min(group, qmax + 1)).astype(np.uint64))
    q[-1] = qmax
    return (q * np.uint64(nb) + np.uint64(b)).astype(np.uint32)


def last_row_hashes(nb, count=64):
    """Up to `count` hashes of the last, incomplete quotient row h >= floor(2^32 / nb) * nb (its
    first and its last value, 0xFFFFFFFF, included). A power-of-two nb has no such row: 0xFFFFFFFF
    alone."""
    rem = (1 << 32) % nb
    if rem == 0:
        return np.array([M32], dtype=np.uint32)
    base = (1 << 32) - rem
    h = np.unique(np.linspace(base, M32, min(count, rem)).astype(np.uint64))
    h[-1] = M32
    return h.astype(np.uint32)


LITERAL_KEYS = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)


def adversarial_keys(nb, n, widths, rng, group=48, lo=0, hi=None, identity=None):
    """n distinct u32 keys for a table of nb buckets, shuffled with rng:
      (i)   identity hashes: the keys of hashes 0 .. min(nb, n // 2) - 1 (h == bucket index), or
            of 0 .. identity - 1 when `identity` is given (where n // 2 is less than nb they fill the
            lowest buckets only, which skews bucket-range partitions by up to 1.5);
      (ii)  for every bucket b of edge_buckets(nb, widths, lo, hi), `group` keys of hashes q * nb + b
            (group_hashes; 48 entries are above the 32-entry bound below which chaining buckets come
            row-sorted, and few enough not to skew a partition);
      (iii) 64 hashes of the last incomplete quotient row, 0xFFFFFFFF included;
      (iv)  the literal keys 0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF;
      (v)   uniform random full-range keys for the rest."""
    n_id = min(nb, n // 2) if identity is None else min(identity, nb, n // 2)
    parts = [unfmix32(np.arange(n_id, dtype=np.uint64))]
    for b in edge_buckets(nb, widths, lo, hi):
        parts.append(unfmix32(group_hashes(nb, b, group)))
    parts.append(unfmix32(last_row_hashes(nb)))
    parts.append(np.array(LITERAL_KEYS, dtype=np.uint32))
    keys = np.concatenate(parts)
    _, first = np.unique(keys, return_index=True)
    keys = keys[np.sort(first)]
    if len(keys) > n:
        raise ValueError(f"the chosen keys alone are {len(keys)} > n = {n}")
    while len(keys) < n:
        extra = rng.integers(0, 1 << 32, 2 * (n - len(keys)) + 16, dtype=np.uint64).astype(np.uint32)
        _, first = np.unique(extra, return_index=True)
        extra = extra[np.sort(first)]
        extra = extra[~np.isin(extra, keys)]
        keys = np.concatenate([keys, extra[: n - len(keys)]])
    return rng.permutation(keys).astype(np.uint32)
