"""CPU: bench.py's command line and what --dump-outputs writes (the selection of queries, the arrays, the 64 MB cap), without a GPU."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=120)


def test_bench_options():
    p = _bench("--help")
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    for bad in (("--steps", "0"), ("--warmup", "-1")):
        p = _bench(*bad)
        assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr


def test_selection_takes_every_query_that_fits():
    assert list(bench.dump_selection(1, 50001, False)) == [0]
    assert list(bench.dump_selection(64, 20001, False)) == list(range(64))  # config 4: 64 x 20001 rows = 30.7 MB


def test_selection_samples_a_fixed_subset_under_the_cap():
    rows = 100001  # config 5: 256 Dubins queries of 100001 rows do not fit
    a = bench.dump_selection(256, rows, True)
    assert np.array_equal(a, bench.dump_selection(256, rows, True))
    assert 1 <= len(a) < 256 and len(set(a.tolist())) == len(a) and np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 256
    per_query = rows * bench.dump_row_bytes(True) + 5 * 8
    assert len(a) * per_query <= bench.DUMP_LIMIT_BYTES < (len(a) + 1) * per_query


def _fake_result(j, found, rows, rng, headings):
    r = SimpleNamespace(status=0, j=j, vgoal=j if found else 0, found=int(found))
    r.pts = rng.integers(0, 1024, size=(rows, 2)).astype(np.int32)
    r.parent = rng.integers(-1, j, size=rows).astype(np.int32)
    r.vcost = rng.uniform(0, 500, size=rows)
    if headings:
        r.head = rng.integers(0, 64, size=rows).astype(np.int32)
    return r


def test_dump_writes_the_live_rows(tmp_path):
    rng = np.random.default_rng(0)
    rows = 41
    res = [_fake_result(30, True, rows, rng, True), _fake_result(12, False, rows, rng, True)]
    nbytes = bench.dump_outputs(str(tmp_path), [3, 7], res, rows, True)
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(got) == {"query_index", "status", "j", "vgoal", "found", "pts", "parent", "vcost", "heading"}
    assert nbytes == sum(a.nbytes for a in got.values()) <= 2 * (rows * bench.dump_row_bytes(True) + 5 * 8)
    assert got["pts"].dtype == got["heading"].dtype == np.float32
    assert all(got[k].dtype == np.float64 for k in ("query_index", "status", "j", "vgoal", "found", "parent", "vcost"))
    assert got["query_index"].tolist() == [3, 7] and got["j"].tolist() == [30, 12] and got["found"].tolist() == [1, 0]
    for i, (r, live) in enumerate(zip(res, (31, 12))):
        assert np.array_equal(got["pts"][i, :live], r.pts[:live]) and np.array_equal(got["parent"][i, :live], r.parent[:live])
        assert np.array_equal(got["vcost"][i, :live], r.vcost[:live]) and np.array_equal(got["heading"][i, :live], r.head[:live])
        for k in ("pts", "parent", "vcost", "heading"):
            assert (got[k][i, live:] == -1).all(), k
