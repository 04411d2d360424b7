"""The reference drivers compiled UNCHANGED against the drop-in headers (3d-hashjoin_amd/host:
algebra.hh, ht_chaining.hh, ht_nested.hh) and linked with libhj3d.so.

CPU: the drivers compile and link against the drop-in layer (`make -C oracle dropin`, needs
/root/reference), and without a GPU they fail loudly (no CPU path).
GPU: the drop-in binaries write the same measurement CSV as the reference binaries built from
the same sources (oracle/_ref/main_experiment{1,4}.out) on the same arguments — every counter
column (scan/build/probe/unnest/top counts, c_htProbeCmp) and every hash-table statistic column
identical; only the timing columns and `reps` (time-driven, util/measure_helpers.hh:15-41) differ.
"""
import csv
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
TIME_COLS = {"reps", "t_total", "t_buildStr", "t_probeStr", "t_top", "t_build_S", "t_build_T", "t_probe_R"}


def _bin(name):
    return os.path.join(REF_DIR, name)


def _env():
    """The drop-in binaries find libhj3d.so through an rpath relative to themselves; where
    oracle/_ref/ is a link to a directory outside the tree that path leads nowhere, so the tests
    also name the tree's library directory to the loader."""
    lib = os.path.join(ROOT, "3d-hashjoin_amd", "lib")
    old = os.environ.get("LD_LIBRARY_PATH")
    return dict(os.environ, LD_LIBRARY_PATH=lib + (os.pathsep + old if old else ""))


def _have(*names):
    return all(os.path.exists(_bin(n)) for n in names)


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="reference sources absent (GPU box)")
def test_drivers_compile_against_dropin():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "dropin"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert _have("dropin_main_experiment1.out", "dropin_main_experiment4.out")


def _cpu_only():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _have("dropin_main_experiment1.out"), reason="drop-in binaries not built")
@pytest.mark.skipif(not _cpu_only(), reason="checks the no-GPU behaviour")
def test_dropin_fails_loudly_without_gpu(tmp_path):
    r = subprocess.run([_bin("dropin_main_experiment1.out"), "-R", "6", "-S", "8", "--no-skew", "-t", "0",
                        "--measure-file", str(tmp_path / "m.csv"), "-p", "Csr"],
                       capture_output=True, text=True, timeout=120, env=_env())
    assert r.returncode != 0
    assert "no CPU path" in r.stderr


def _rows(path):
    with open(path) as f:
        rows = list(csv.DictReader(f, delimiter=";"))
    return {r["plan"]: {k: v for k, v in r.items() if k not in TIME_COLS} for r in rows}


def _run_pair(tmp_path, exe, args):
    out = {}
    for tag in ("ref", "dropin"):
        m = tmp_path / f"{tag}.csv"
        name = exe if tag == "ref" else "dropin_" + exe
        r = subprocess.run([_bin(name)] + args + ["--measure-file", str(m)], capture_output=True, text=True,
                           timeout=600, cwd=str(tmp_path), env=_env())
        assert r.returncode == 0, f"{name}: {r.stderr[-2000:]}"
        out[tag] = _rows(m)
    return out["ref"], out["dropin"]


EXP1_CASES = [
    ["-R", "10", "-S", "12", "--no-skew", "-t", "0"],
    ["-R", "12", "-S", "16", "--skew", "-t", "0"],
    ["-R", "14", "-S", "18", "--no-skew", "-t", "2", "-b", "3"],
    ["-R", "16", "-S", "20", "--skew", "-t", "1", "-b", "2"],
    ["-R", "0", "-S", "3", "--no-skew", "-t", "0"],
]


@pytest.mark.gpu
@pytest.mark.skipif(not _have("main_experiment1.out", "dropin_main_experiment1.out"), reason="binaries not built")
@pytest.mark.parametrize("args", EXP1_CASES, ids=lambda a: "_".join(a).replace("-", ""))
def test_experiment1_csv_matches_reference(tmp_path, args):
    ref, got = _run_pair(tmp_path, "main_experiment1.out", args)
    assert set(got) == set(ref)
    for plan in ref:
        assert got[plan] == ref[plan], plan


EXP4_CASES = [
    ["-R", "10", "-a", "2", "-A", "2", "-b", "2", "-B", "1"],
    ["-R", "14", "-a", "3", "-A", "4", "-b", "2", "-B", "2"],
    ["-R", "16", "-a", "1", "-A", "3", "-b", "3", "-B", "5"],
]


@pytest.mark.gpu
@pytest.mark.skipif(not _have("main_experiment4.out", "dropin_main_experiment4.out"), reason="binaries not built")
@pytest.mark.parametrize("args", EXP4_CASES, ids=lambda a: "_".join(a).replace("-", ""))
def test_experiment4_csv_matches_reference(tmp_path, args):
    ref, got = _run_pair(tmp_path, "main_experiment4.out", args)
    assert set(got) == set(ref)
    for plan in ref:
        assert got[plan] == ref[plan], plan


# ---- tests/cpp/dropin_pertuple.cc: per-tuple probe API, host unnest path, relation cache ----
PERTUPLE = os.path.join(ROOT, "3d-hashjoin_amd", "bin", "dropin_pertuple")
PERTUPLE_CHECKS = ("chaining_per_tuple_walk", "nested_per_tuple_walk", "nested_host_probe_custom_consumer",
                   "relation_modified_in_place")


def test_pertuple_program_builds():
    """The per-tuple drop-in program compiles against the drop-in headers and links libhj3d."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "3d-hashjoin_amd"), "bin/dropin_pertuple"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.path.exists(PERTUPLE)


@pytest.mark.skipif(not os.path.exists(PERTUPLE), reason="per-tuple drop-in program not built")
@pytest.mark.skipif(not _cpu_only(), reason="checks the no-GPU behaviour")
def test_pertuple_fails_loudly_without_gpu():
    r = subprocess.run([PERTUPLE], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "PASS" not in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(PERTUPLE), reason="per-tuple drop-in program not built")
def test_gpu_pertuple_probe_api_and_host_unnest():
    """findDirEntryByOther / findMainNodeByOther walked tuple at a time over the host node view of
    the device table give the device probe's matches and comparisons; probe -> unnest -> a custom
    consumer yields the brute-force join's pairs in the reference's order; an in-place change of a
    relation is seen (re-upload, different result)."""
    r = subprocess.run([PERTUPLE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for name in PERTUPLE_CHECKS:
        assert f"PASS {name}" in r.stdout, r.stdout


# ---- tests/cpp/dist_join.cc: the multi-GPU strand from C++ on the C ABI (hj3d_comm_*) ----
DIST_JOIN = os.path.join(ROOT, "3d-hashjoin_amd", "bin", "dist_join")


def test_dist_join_program_builds_and_fails_loudly_without_gpu():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "3d-hashjoin_amd"), "bin/dist_join"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    if _cpu_only():
        r = subprocess.run([DIST_JOIN, "1024", "8192", "Csr"], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "no CPU path" in r.stderr


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(DIST_JOIN), reason="dist_join not built")
@pytest.mark.parametrize("plan", ["Csr", "Nsr"])
def test_gpu_dist_join_cpp_host_equals_reference(plan):
    """The C++ host's partition -> RCCL exchange (libhj3d) -> build / 3-chunk probe -> merge strand at
    world size 1, on the reference's relations: every counter, checksum and statistic equals the
    reference binary's fixture (tests/golden/exp1_R1048576_S8388608_uni.json)."""
    import json
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "exp1_R1048576_S8388608_uni.json")))
    r = subprocess.run([DIST_JOIN, str(g["nR"]), str(g["nS"]), plan, "3"], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("c_build=")]  # RCCL may print banners
    assert len(line) == 1, r.stdout[-3000:]
    got = {k: int(v) for k, v in (kv.split("=") for kv in line[0].split())}
    ref = g["plans"][plan]
    assert got["c_build"] == ref["c_build"] and got["c_top"] == ref["c_top"] and got["c_cmp"] == ref["c_cmp"]
    for k in ("n", "sum_a", "sum_b", "sum_h", "xor_h"):
        assert got[k] == ref["out"][k], k
    for k in ("nb", "empty", "entries", "cc0_min", "cc0_max", "cc0_sum", "cc0_cnt", "cc1_min", "cc1_max", "cc1_sum",
              "cc1_cnt"):
        assert got[k] == ref["stats"][k], k
