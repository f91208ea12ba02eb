"""Every entry point refuses each one-field violation of its contract (tests/_contract.py) with the documented code, and
accepts the baseline each violation was derived from.

Host validation runs before any launch and is the same code with or without a device, so it is observed where there
is none: an accepted call then comes back as SWL_ERR_LAUNCH (-3; swl_swap_blocks: SWL_ERR_RUNTIME, -4), a refused one
as -1 / -2. With a device present a baseline would launch on the table's fake host pointers, so the module skips."""
import pytest
import torch

from swiftllm_amd import _hip

if torch.cuda.is_available():
    pytest.skip("argument validation is observed without a device (a baseline would launch on host pointers)",
                allow_module_level=True)

import _contract as C  # noqa: E402


def test_every_entry_point_has_a_row_or_a_reasoned_exclusion():
    assert set(C.ROWS) | set(C.EXCLUDED) == set(_hip.SIGNATURES)
    assert not set(C.ROWS) & set(C.EXCLUDED)
    assert all(isinstance(why, str) and len(why) > 20 for why in C.EXCLUDED.values())
    for row in C.ROWS.values():
        assert row.violations, row.name
        assert list(row.args) and len(row.args) == len(_hip.SIGNATURES[row.name]), row.name


@pytest.mark.parametrize("name", sorted(C.ROWS))
def test_baseline_is_accepted(name):
    row = C.ROWS[name]
    assert row.call_baseline, f"{name}: {row.note}"
    rc = row.call(_hip.load())
    assert rc not in (C.BAD, C.UNSUP), f"{name}: the baseline itself is refused with {rc}"
    assert rc != 0, f"{name}: a non-empty call cannot succeed without a device"


@pytest.mark.parametrize("name,label,field,value,code", C.cases(), ids=[f"{c[0]}-{c[1]}" for c in C.cases()])
def test_violation_is_refused(name, label, field, value, code):
    row = C.ROWS[name]
    assert row.args[field] != value, "a violation changes its field"
    assert row.call(_hip.load(), **{field: value}) == code, f"{name}: {label} ({field} = {value})"


def test_bytes_baselines_are_what_the_library_advertises():
    """The *_bytes fields of the baselines are exact, so `one short` in a violation means one below the advertised size."""
    lib = _hip.load()
    arg = C.ROWS["swl_argmax"].args
    assert arg["scratch_bytes"] == C.ARGMAX_SCRATCH == lib.swl_argmax_scratch_bytes(arg["num_rows"])
    for name in ("swl_gemm_skinny", "swl_gemm_skinny_packed", "swl_gemm_packed_mid", "swl_gemm_packed_wide"):
        a = C.ROWS[name].args                 # explicit k_splits: k_splits * M * N fp32, never above the advertised cover
        assert a["workspace_bytes"] == a["k_splits"] * a["M"] * a["N"] * 4
    a = C.ROWS["swl_gemm_skinny"].args
    assert a["workspace_bytes"] <= 16 * a["M"] * a["N"] * 4
    assert lib.swl_gemm_skinny_workspace_bytes(a["M"], 4096, 4096) == 16 * a["M"] * 4096 * 4


def test_the_calls_that_used_to_launch():
    """The accepted calls the table was started from: each stores outside `o` on a device."""
    lib = _hip.load()
    dec, p2, var = C.ROWS["swl_paged_attn_decode"], C.ROWS["swl_paged_attn_phase2"], C.ROWS["swl_prefill_attn_varlen"]
    assert 8 < C.QW
    assert dec.call(lib, o_tok_stride=-8) == C.BAD
    assert dec.call(lib, o_tok_stride=8) == C.BAD
    assert dec.call(lib, q_tok_stride=8) == C.BAD
    assert dec.call(lib, o=dec.args["o"] + 2) == C.BAD
    assert p2.call(lib, o_tok_stride=8) == C.BAD
    assert var.call(lib, o_tok_stride=8) == C.BAD
