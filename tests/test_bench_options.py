"""bench.py's run shape: a plain run times the steps and prints the line, `--full` adds the side legs, `--dump-outputs DIR` writes
what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("e2e_scaling", "e2e", "cpu_baseline", "samples_in_flight", "exact_em", "workloads", "reference_like_for_like")


def _run(args, timeout=600):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_options_are_checked_before_any_work():
    r = _run(["--help"], timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = _run(["--steps", "0"], timeout=300)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr
    r = _run(["--workload", "class1", "--dump-outputs", "unused"], timeout=300)
    assert r.returncode != 0 and "configs1" in r.stderr


def _line(r):
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_result_and_full_computes_the_same(tmp_path):
    """A plain run: the headline fields and none of the side legs; --dump-outputs holds the last timed step's result (float64).
    The same arguments with --full (its cheap part) give the same arrays: the inputs are seeded, the timed path is the same."""
    from hisatgenotype_amd import locus as hl, synth
    common = ["--pairs", "20000", "--steps", "3", "--warmup", "1"]
    plain = _line(_run(common + ["--dump-outputs", str(tmp_path / "plain")]))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert not [k for k in SIDE_LEGS if k in plain]
    assert plain["config"]["device_front_end_batch_identical_to_host"] is None
    full = _line(_run(common + ["--dump-outputs", str(tmp_path / "full"), "--full", "--no-workloads", "--no-e2e", "--no-cpu-baseline"]))
    assert full["config"]["device_front_end_batch_identical_to_host"] is True

    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full"))
    assert {"reads_pairs.npy", "counts.npy", "counts_order.npy", "gene_prob.npy", "gene_prob_allele.npy", "em0_abundance.npy"} <= set(names)
    got = {n: np.load(str(tmp_path / "plain" / n)) for n in names}
    ref = {n: np.load(str(tmp_path / "full" / n)) for n in names}
    for n in names:
        assert got[n].dtype == np.float64 and got[n].shape == ref[n].shape, n
        if "abundance" in n or n == "gene_prob.npy":
            assert np.allclose(got[n], ref[n], rtol=0, atol=1e-9), n
        else:
            assert np.array_equal(got[n], ref[n]), n
    assert got["reads_pairs.npy"][1] == plain["config"]["pairs_per_gpu"]
    pl = hl.PackedLocus.from_synth(synth.make_hla_like_locus(n_alleles=7000, n_vars=2500, seed=101))
    assert [pl.names[int(a)] for a in got["gene_prob_allele.npy"][:2]] == plain["config"]["top2"]
