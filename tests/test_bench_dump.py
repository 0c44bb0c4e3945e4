"""bench.py --dump-outputs: the output ciphertexts of the last timed step, written so that two builds run with the same
arguments compare word for word (float64 holds every uint32 word exactly; a fixed seeded sample when over the budget)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol

ROOT = ol.ROOT
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_dump_outputs_exact_words_and_budget(tmp_path, monkeypatch):
    b = _bench_module()
    assert b.DUMP_BUDGET_BYTES <= 64 * 10**6
    words = np.random.default_rng(3).integers(0, 2**32, size=(300, ol.n + 1), dtype=np.uint64).astype(np.uint32)
    words[0, :2] = (0, 2**32 - 1)

    # within the budget: every row, float64, word for word
    b.dump_outputs(str(tmp_path / "all"), "nand", words)
    assert sorted(os.listdir(tmp_path / "all")) == ["nand_out.npy"]
    got = np.load(tmp_path / "all" / "nand_out.npy")
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), words) and np.array_equal(got, words)

    # over the budget: a fixed sample of rows (the same on every run), their gate indices beside them, all files within it
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 200_000)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), "nand", words)
    rows = np.load(tmp_path / "s1" / "nand_out_rows.npy")
    got = np.load(tmp_path / "s1" / "nand_out.npy")
    assert 0 < rows.size < words.shape[0] and np.all(np.diff(rows) > 0) and rows.dtype == np.float64
    assert np.array_equal(got, words[rows.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")) <= 200_000
    for f in ("nand_out.npy", "nand_out_rows.npy"):
        assert np.array_equal(np.load(tmp_path / "s1" / f), np.load(tmp_path / "s2" / f))

    # several ranks: one file per rank, each within its share
    monkeypatch.setattr(b, "WORLD", 4)
    monkeypatch.setattr(b, "RANK", 2)
    b.dump_outputs(str(tmp_path / "r"), "mixed", words)
    assert sorted(os.listdir(tmp_path / "r")) == ["mixed_out_rank2.npy", "mixed_out_rank2_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "r" / f) for f in os.listdir(tmp_path / "r")) <= 200_000 // 4


@pytest.mark.parametrize("args, msg", [(["--steps", "0"], "--steps"), (["--mode", "api", "--dump-outputs", "x"], "--mode ranks")])
def test_bench_rejects_bad_arguments(args, msg):
    p = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and msg in p.stderr, p.stderr[-2000:]


@pytest.mark.gpu
def test_bench_dump_is_the_timed_path_output(tmp_path):
    """The dumped words are what the HIP gate path computed on bench.py's seeded inputs: the CPU oracle's words for the same
    NAND gates, and `steps` in the line is the number of timed steps asked for."""
    gates = 64
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--gates", str(gates), "--no-extra",
                        "--no-cpu-baseline", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert line["steps"] == 3 and line["warmup"] == 1
    got = np.load(out_dir / "nand_out.npy")
    assert got.shape == (gates, ol.n + 1) and got.dtype == np.float64
    # bench.py's inputs: keys from seed 4242, rank 0's ciphertexts from seed 42
    krng, rng = np.random.default_rng(4242), np.random.default_rng(42)
    bk = krng.integers(0, 2**32, size=ol.BK_WORDS, dtype=np.uint64).astype(np.uint32)
    ksk = krng.integers(0, 2**32, size=ol.KSK_WORDS, dtype=np.uint64).astype(np.uint32)
    in0, in1 = (rng.integers(0, 2**32, size=(gates, ol.n + 1), dtype=np.uint64).astype(np.uint32) for _ in range(2))
    L = ol.load()
    ek = L.orc_evalkey_create(bk, ksk)
    want = np.zeros(gates * (ol.n + 1), np.uint32)
    L.orc_gate_batch(ek, np.array([0], np.int32), 0, 0, gates, want, in0.ravel(), in1.ctypes.data, None, min(L.orc_max_threads(), 32))
    L.orc_evalkey_destroy(ek)
    assert np.array_equal(got, want.reshape(gates, -1))
