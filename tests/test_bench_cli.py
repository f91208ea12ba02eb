"""bench.py's command line: a plain run is the headline alone (--full adds the side measurements), --steps is the number of
timed steps, --dump-outputs writes float64 arrays."""
import os
import sys

import numpy as np
import pytest

import bench


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse_args()


def test_plain_run_is_the_default(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 5, 2)
    a = _args(monkeypatch, "--full", "--dump-outputs", "out")
    assert a.full and a.dump_outputs == "out"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1")])
def test_step_counts_are_checked(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _args(monkeypatch, *argv)


def test_dump_outputs_writes_float64(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), {"tokens": [3, 128255, 0]})
    got = np.load(os.path.join(tmp_path, "d", "tokens.npy"))
    assert got.dtype == np.float64 and got.tolist() == [3.0, 128255.0, 0.0]
