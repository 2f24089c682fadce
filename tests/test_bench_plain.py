"""bench.py without --full: the headline figure alone (no oracle recount, no CPU baseline, no secondary figures), and what
--dump-outputs writes — one step's tables, and with --config 5 a seeded sample of the rescaling — against the C oracle
over the same records."""

import importlib.util
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
GENOME = (("chr1", 8_000_000), ("chr2", 2_000_000), ("chrS", 500))


def bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", str(ROOT / "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, str(ROOT / "bench.py")] + [str(a) for a in args]
    out = subprocess.run(cmd, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def load_dump(folder):
    return {p.stem: np.load(p) for p in sorted(pathlib.Path(folder).glob("*.npy"))}


@pytest.mark.gpu
def test_plain_line_and_dumped_tables_equal_the_oracle(tmp_path):
    from mapdamage_amd import synth
    from oracle import oracle
    n, steps = 300_000, 3
    line = run_bench(["--reads", n, "--steps", steps, "--warmup", 1, "--dump-outputs", tmp_path / "out"])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "reads/s"
    assert line["higher_is_better"] is True and line["dtype"] == "u8"
    assert not {"secondary", "cpu_baseline", "parity"} & set(line)
    got = load_dump(tmp_path / "out")
    assert set(got) == {"mis", "comp", "lgd", "n_kept"} and all(a.dtype == np.float64 for a in got.values())
    assert {k: list(v.shape) for k, v in got.items()} == line["outputs"]
    # the records of the run (bench.py: config 3, batch 0 of rank 0) and the oracle's tables of one pass over them
    ref = synth.make_genome(sizes=GENOME)
    b = synth.parallel_batch("config3_batch", ref, n, seed=3000, workers=1)
    want = oracle.tabulate(ref, b, 1, 70, 10, 0, lgd_max=4096)
    assert got["n_kept"][0] == want["n_kept"] == n
    for k in ("mis", "comp", "lgd"):
        np.testing.assert_array_equal(got[k], want[k].astype(np.float64), err_msg=k)


@pytest.mark.gpu
def test_dumped_rescaling_sample_equals_the_oracle(tmp_path):
    from mapdamage_amd import synth
    from oracle import oracle
    bench = bench_module()
    n = 300_000
    run_bench(["--config", 5, "--reads", n, "--steps", 2, "--warmup", 1, "--dump-outputs", tmp_path / "out"])
    got = load_dump(tmp_path / "out")
    assert set(got) == {"mis", "comp", "lgd", "n_kept", "rescaled_qual_sample", "mr_sample", "status_sample"}
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    ref = synth.make_genome(sizes=GENOME)
    b = bench.add_mates(synth.parallel_batch(bench.CONFIG5, ref, n, seed=5000, workers=1), 5000)
    want = oracle.tabulate(ref, b, 1, 70, 10, 0, lgd_max=4096)
    for k in ("mis", "comp", "lgd"):
        np.testing.assert_array_equal(got[k], want[k].astype(np.float64), err_msg=k)
    model, corr = bench.rescale_fixture()
    wq, wmr, wst = oracle.rescale(ref, b, corr, model.len5p, model.len3p)
    # the sample of bench.dump_outputs for one resident batch
    rng = np.random.default_rng(9000)
    ib = np.sort(rng.integers(0, wq.shape[0], min(bench.DUMP_SAMPLE, wq.shape[0])))
    ir = np.sort(rng.integers(0, n, min(bench.DUMP_SAMPLE, n)))
    np.testing.assert_array_equal(got["rescaled_qual_sample"], wq[ib].astype(np.float32))
    np.testing.assert_array_equal(got["status_sample"], wst[ir].astype(np.float32))
    np.testing.assert_array_equal(got["mr_sample"], np.where(np.isnan(wmr[ir]), -1.0, wmr[ir]))
