"""The launches of a forward, held to the recorded ones: tools/record_layer_traces.py runs one model per engine
configuration through a fixed list of scenarios with `_hip.call` and the library GEMM replaced by recorders;
tests/golden/layer_launch_traces.json is what the commit before the layer's route decision (worker/layers/
transformer_layer.py: decide_route) launched in every cell — entry names and integer arguments. The layer's control flow may
be rewritten; what it launches, with which shapes, strides, split counts and layer ids, may not change by it."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_layer_traces as R     # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "layer_launch_traces.json"), encoding="utf-8") as _f:
    FIXTURE = R.decode_fixture(json.load(_f))


def test_the_fixture_reaches_every_launch_form_of_the_layer():
    """Over all cells the recorded traces contain every kernel form the layer's routes choose between (and the library
    GEMM), every configuration is there, and the cell that is meant to split its flash decoding does."""
    assert set(FIXTURE) == set(R.CONFIGS)
    names = {call[0] for cells in FIXTURE.values() for steps in cells.values() for step in steps for call in step}
    assert R.missing_names(names) == []
    long_cell = [call[0] for call in FIXTURE["no_rows_decode"]["decode_b1_long"][-1]]
    assert "swl_gemm_tiny_partial_from_attn" in long_cell and "swl_paged_attn_decode_qkv_rs_partials" in long_cell


@pytest.fixture(scope="module")
def model_dirs():
    dirs = {}       # (geometry, dtype) -> checkpoint directory, shared by the configurations
    yield dirs
    for path in dirs.values():
        shutil.rmtree(path, ignore_errors=True)


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(R.CONFIGS))
def test_every_cell_launches_what_the_fixture_recorded(config, model_dirs):
    cells = R.Cells(config, model_dirs)
    try:
        assert set(cells.scenarios()) == set(FIXTURE[config])
        for scenario in cells.scenarios():
            steps, _, _ = cells.run(scenario)
            want = FIXTURE[config][scenario]
            assert len(steps) == len(want), (config, scenario)
            for i, (got, exp) in enumerate(zip(steps, want)):
                if got != exp:
                    at = next((j for j, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
                    pytest.fail(f"{config} / {scenario} / forward {i}: launch {at} is {got[at:at + 1]}, recorded {exp[at:at + 1]}\n"
                                f"launched: {[c[0] for c in got]}\nrecorded: {[c[0] for c in exp]}")
    finally:
        cells.close()
