"""The arena harness (tests/_arena.py) catches what it is for: four fake operations written in torch on CPU tensors,
each wrong in one of the ways a kernel goes wrong, and one correct operation that passes. No kernel runs here."""
import pytest
import torch

from _arena import MIN_MARGIN, Arena, Op, run_case

CPU = torch.device("cpu")
ROWS, WIDTH, STRIDE = 3, 8, 16


def _ops(scratch=False):
    g = torch.Generator().manual_seed(0)
    ops = {"x": Op(torch.randn(ROWS, WIDTH, generator=g).to(torch.float16), skew=16, stride=STRIDE),
           "out": Op(torch.zeros(ROWS, WIDTH, dtype=torch.float16), skew=8, stride=STRIDE, out=True)}
    if scratch:
        ops["scratch"] = Op(torch.zeros(ROWS * WIDTH, dtype=torch.float32), skew=16, scratch=True)
    return ops


def _flat(view):
    """The arena (or the control's buffer) behind a strided view, from its first element on: what a kernel's raw pointer sees."""
    return view.as_strided((ROWS * STRIDE,), (1,))


def double(v):
    v["out"].copy_(v["x"] * 2)


def stores_one_element_past_its_output(v):
    double(v)
    _flat(v["out"])[(ROWS - 1) * STRIDE + WIDTH] = 1.0


def stores_into_a_padding_column(v):
    double(v)
    _flat(v["out"])[WIDTH] = 1.0


def reads_the_element_before_its_input(v):
    double(v)
    before = v["x"].as_strided((1,), (1,), v["x"].storage_offset() - 1) if v["x"].storage_offset() else torch.zeros(1)
    v["out"][0, 0] = v["out"][0, 0] + before[0].to(torch.float16)


def reads_its_scratch_before_writing_it(v):
    s = v["scratch"].view(ROWS, WIDTH)
    v["out"].copy_(v["x"] * 2 + s.to(torch.float16))      # a stale slot reaches the output
    s.copy_(v["x"].float())


def test_a_correct_operation_passes():
    want = run_case(_ops(), double, CPU)
    assert torch.equal(want["out"], _ops()["x"].data * 2)


def test_placement_honours_skew_stride_and_margins():
    arena = Arena(0xFF, CPU, Arena.capacity_for(_ops().values()))
    views = {n: arena.place(op, n) for n, op in _ops().items()}
    assert views["x"].data_ptr() % 32 == 16 and views["out"].data_ptr() % 16 == 8
    assert views["x"].stride() == (STRIDE, 1) and torch.equal(views["x"], _ops()["x"].data)
    lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + arena.buf.numel()
    for v in views.values():
        assert v.data_ptr() - lo >= MIN_MARGIN and hi - (v.data_ptr() + ROWS * STRIDE * 2) >= MIN_MARGIN
    assert abs(views["out"].data_ptr() - views["x"].data_ptr()) >= MIN_MARGIN
    assert bool((_flat(views["x"])[WIDTH:STRIDE].view(torch.uint8) == 0xFF).all()), "padding columns hold the fill"


@pytest.mark.parametrize("op,scratch,needle", [
    (stores_one_element_past_its_output, False, "outside the declared outputs"),
    (stores_into_a_padding_column, False, "a padding column"),
    (reads_the_element_before_its_input, False, "differs from the control"),
    (reads_its_scratch_before_writing_it, True, "differs from the control"),
], ids=lambda p: getattr(p, "__name__", None))
def test_a_wrong_operation_is_caught(op, scratch, needle):
    with pytest.raises(AssertionError, match=needle):
        run_case(_ops(scratch), op, CPU)
