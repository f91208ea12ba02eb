"""bench.py end to end on the tiny model: a plain run prints the headline alone and dumps the same outputs whatever the KV
pool's size; --full adds the side measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--model", "tiny", "--batch", "4", "--prompt-len", "64", "--steps", "6", "--warmup", "2"]


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *TINY, *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_same_tokens_whatever_the_pool_size(tmp_path):
    outs = []
    for blocks in ("256", "300"):
        d = tmp_path / blocks
        res = _bench("--kv-blocks", blocks, "--dump-outputs", str(d))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "prefill_tok_s"):
            assert key in res, key
        assert res["steps"] == 6 and res["warmup"] == 2 and res["config"]["kv_pool_blocks"] == int(blocks)
        assert res["value"] == pytest.approx(4 * 6 / (res["ms_per_step"] * 6 * 1e-3), rel=1e-3)
        assert not {"roofline", "cpu_baseline", "eager"} & res.keys()
        tokens = np.load(d / "tokens.npy")
        assert tokens.dtype == np.float64 and tokens.shape == (4,)
        outs.append(tokens)
    assert np.array_equal(outs[0], outs[1])


def test_full_run_adds_the_side_measurements():
    res = _bench("--kv-blocks", "256", "--full")
    assert "roofline" in res and "cpu_baseline" in res and "eager" in res
