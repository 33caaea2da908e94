"""bench.py's command line on one GPU: a plain run times its steps and prints the line without the
`--full` legs, and `--dump-outputs` writes the result words of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_steps_words(orc, tmp_path):
    """c1 with 3 steps: the launches rotate over 16 batches, so the last timed step ran batch 2 (the
    sub-stream starting at packet 2 x 1,048,576); the dumped halves are the oracle's words for it.
    The plain line carries the headline fields and none of the `--full` measurements."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--ramp-ms", "0", "--workload", "c1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["metric"] == bench.METRIC and j["unit"] == "GB/s" and j["higher_is_better"] is True
    assert j["dtype"] == "u8" and j["steps"] == 3 and j["warmup"] == 1 and j["full"] is False
    assert j["value"] > 0 and j["ms_per_step"] > 0
    # value is the steps' bytes over their wall time
    c = j["config"]
    assert c["batches_rotated"] == 16
    assert j["value"] == pytest.approx(c["algorithmic_bytes_per_step_all_ranks"] / (j["ms_per_step"] * 1e-3) / 1e9,
                                       rel=1e-3)
    assert j["cpu_baseline"] is None and "pipelined_two_streams" not in j
    assert c["verify_all_packets"] is None and c["oracle_gate"] is None and c["per_launch_ms_rank0"] is None
    assert j["roofline"]["contiguous_read_GBps"] is None and j["roofline"]["launch_read_ceiling"] is None
    assert sorted(os.listdir(tmp_path)) == ["out_hi16.npy", "out_lo16.npy"]
    lo, hi = np.load(tmp_path / "out_lo16.npy"), np.load(tmp_path / "out_hi16.npy")
    assert lo.dtype == hi.dtype == np.float32 and lo.shape == hi.shape == (1 << 20,)
    synth_id, n, stride, _ = bench.WORKLOADS["c1"]
    a, d = orc.synth(n, stride, 0, synth_id, bench.SEED, 2 * n)
    want, _ = orc.process(a, d)
    assert np.array_equal(lo, (want & 0xFFFF).astype(np.float32))
    assert np.array_equal(hi, (want >> 16).astype(np.float32))
