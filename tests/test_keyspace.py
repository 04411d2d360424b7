"""CPU tests of tests/keyspace.py (keys with chosen fmix32 hashes) and the host pin of FastDiv32."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import keyspace as KS
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fmix32_round_trip_both_ways():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 32, 1_000_000, dtype=np.uint64).astype(np.uint32)
    edges = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    x = np.concatenate([x, edges])
    assert (KS.unfmix32(KS.fmix32(x)) == x).all()
    assert (KS.fmix32(KS.unfmix32(x)) == x).all()
    assert int(KS.unfmix32(0)) == 0 and int(KS.fmix32(0)) == 0
    assert int(KS.unfmix32(0xFFFFFFFF)) == 0x331DA083
    assert int(KS.fmix32(0x331DA083)) == 0xFFFFFFFF
    # murmur3's published fmix32 of 1 (the constants and shifts in the right order)
    assert int(KS.fmix32(1)) == 0x514E28B7


@pytest.mark.parametrize("nb", [7000, 100_000, 131072])
def test_group_lands_in_its_bucket_by_the_oracles_hash(nb):
    """All keys of one (ii) group share bucket b under the ORACLE's hash (not under a second copy of
    the helper's own): a chaining table at nb buckets over them alone has one collision chain of
    `group` entries and nb - 1 empty buckets."""
    group = 48
    for b in KS.edge_buckets(nb, (384, 1024, 6144), lo=nb // 3, hi=2 * nb // 3):
        keys = KS.unfmix32(KS.group_hashes(nb, b, group))
        assert len(np.unique(keys)) == group
        B = O.tuples3(keys, np.zeros(group, np.uint32))
        e = O.chain_plan(B, 0, B, 0, nb, True)
        assert e.stats["cc0_max"] == group, (nb, b)
        assert e.stats["empty"] == nb - 1, (nb, b)
        assert e.c_probe == group


def test_edge_buckets():
    assert KS.edge_buckets(10, (4,)) == [0, 1, 3, 4, 7, 8, 9]
    assert KS.edge_buckets(10, (4,), lo=5, hi=6) == [0, 1, 3, 4, 5, 6, 7, 8, 9]
    assert KS.edge_buckets(1, (64,)) == [0]
    assert KS.edge_buckets(10, (), lo=(0, 5), hi=(5, 10)) == [0, 1, 4, 5, 9]  # several owned ranges
    got = KS.edge_buckets(100_000, (384, 1024, 1536, 6144), lo=33_334, hi=66_667)
    assert got == sorted(set(got)) and got[0] == 0 and got[-1] == 99_999
    for b in (383, 384, 767, 768, 260 * 384 - 1, 260 * 384, 6143, 6144, 16 * 6144, 33_333, 33_334, 66_666, 66_667):
        assert b in got, b


def test_last_row_hashes():
    h = KS.last_row_hashes(7000)
    base = (1 << 32) // 7000 * 7000
    assert len(h) == 64 and int(h[0]) == base and int(h[-1]) == 0xFFFFFFFF and (h.astype(np.uint64) >= base).all()
    assert KS.last_row_hashes(131072).tolist() == [0xFFFFFFFF]
    assert KS.last_row_hashes(4294967291).tolist() == [4294967291 + k for k in range(5)]


@pytest.mark.parametrize("nb,n", [(7000, 100_000), (100_000, 100_000), (131072, 131072), (8192, 65536), (64, 4000)])
def test_adversarial_keys_are_n_distinct(nb, n):
    widths = (384, 1024, 1536, 6144)
    K = KS.adversarial_keys(nb, n, widths, np.random.default_rng(nb))
    assert K.dtype == np.uint32 and len(K) == n and len(np.unique(K)) == n
    h = KS.fmix32(K).astype(np.uint64)
    have = set(h.tolist())
    # every chosen part is present
    assert set(range(min(nb, n // 2))) <= have
    assert 0xFFFFFFFF in have and set(KS.last_row_hashes(nb).tolist()) <= have
    assert set(KS.LITERAL_KEYS) <= set(K.tolist())
    for b in KS.edge_buckets(nb, widths):
        assert int(((h % np.uint64(nb)) == b).sum()) >= min(48, (0xFFFFFFFF - b) // nb + 1), b
    # same seed, same keys; the keys use all 32 bits
    assert (K == KS.adversarial_keys(nb, n, widths, np.random.default_rng(nb))).all()
    assert int(K.max()) == 0xFFFFFFFF
    # a bound on the identity part leaves every other chosen hash in place
    K16 = KS.adversarial_keys(nb, n, widths, np.random.default_rng(nb), identity=16)
    h16 = set(KS.fmix32(K16).tolist())
    assert len(np.unique(K16)) == n and set(range(16)) <= h16 and set(KS.last_row_hashes(nb).tolist()) <= h16


def test_fastdiv32_host_pin(tmp_path):
    """hj3d::FastDiv32 (hj3d_device.hpp) against n / d on the host: tests/cpp/fastdiv_host.cc built
    with hipcc for gfx950 (the header is a HIP header; the program makes no HIP call) exits 0."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "fastdiv_host"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-x", "hip",
                    "-I", os.path.join(ROOT, "3d-hashjoin_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "fastdiv_host.cc"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 wrong" in r.stdout, r.stdout
