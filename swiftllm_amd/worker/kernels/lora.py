"""Per-row low-rank adapter updates (multi-LoRA serving): the host side of csrc/lora.hip.

    y[row, :] += scale[slot] * (x[row, :] @ A[slot].T)[part columns] @ B[slot].T        for rows with slot >= 0

`build_tiles` groups a step's rows by adapter slot into tiles of <= 16 rows (numpy, no device), `LoraBatch` is that
grouping on the device (ONE upload per forward, a buffer of its own: the packed metadata of BatchPlan is not touched) plus
the fp32 `t` workspace, and `lora_apply` runs shrink + expand of one projection group on a projection's output, in place.
There is no fallback: a shape the kernels do not take is an error.
"""
import ctypes
from typing import List, Sequence, Tuple

import numpy as np
import torch

from swiftllm_amd import _hip

from ..step_logits import StagedInts

TILE_ROWS = 16
SUPPORTED_RANKS = (8, 16, 32, 64)


def build_tiles(row_slots: Sequence[int], num_slots: int) -> Tuple[np.ndarray, np.ndarray]:
    """(tile_rows int32 [num_tiles * 16], tile_slots int32 [num_tiles]) for per-row slots (-1 = no adapter). Tiles are
    ordered by slot, rows inside a slot keep their order; a slot's last tile is padded with -1. Raises ValueError for a
    slot outside [-1, num_slots): the kernels index the slot stacks with it."""
    slots = np.asarray(row_slots, dtype=np.int64).reshape(-1)
    if slots.size and (slots.min() < -1 or slots.max() >= num_slots):
        raise ValueError(f"adapter slots must be in [-1, {num_slots}), got [{int(slots.min())}, {int(slots.max())}]")
    rows_out: List[np.ndarray] = []
    tile_slots: List[int] = []
    for s in np.unique(slots[slots >= 0]):
        rows = np.nonzero(slots == s)[0].astype(np.int32)
        n_tiles = -(-rows.size // TILE_ROWS)
        padded = np.full(n_tiles * TILE_ROWS, -1, dtype=np.int32)
        padded[:rows.size] = rows
        rows_out.append(padded)
        tile_slots += [int(s)] * n_tiles
    if not rows_out:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    return np.concatenate(rows_out), np.asarray(tile_slots, dtype=np.int32)


def k_splits(k: int) -> int:
    """fp32 slabs of t for a projection with K input columns (a function of K alone)."""
    return int(_hip.load().swl_lora_k_splits(int(k)))


class LoraGroup:
    """The slot stacks of one projection group (one weight tensor of a layer): a_stack [S, P * r_max, K], b_stack
    [S, N, r_max], scale fp32 [S]; `parts` = ((n_begin, n_end, t_col_offset), ...), `names` the PEFT module of each part."""
    __slots__ = ("names", "parts", "a_stack", "b_stack", "scale", "r_max", "n", "k", "_parts_c")

    def __init__(self, names, widths, k: int, num_slots: int, r_max: int, dtype, device):
        self.names = tuple(names)
        self.r_max, self.k, self.n = int(r_max), int(k), int(sum(widths))
        parts, at = [], 0
        for i, w in enumerate(widths):
            parts.append((at, at + int(w), i * self.r_max))
            at += int(w)
        self.parts = tuple(parts)
        self.a_stack = torch.zeros((num_slots, len(parts) * self.r_max, self.k), dtype=dtype, device=device)
        self.b_stack = torch.zeros((num_slots, self.n, self.r_max), dtype=dtype, device=device)
        self.scale = torch.zeros((num_slots,), dtype=torch.float32, device=device)
        self._parts_c = (ctypes.c_int32 * (3 * len(parts)))(*[v for p in parts for v in p])

    @property
    def num_slots(self) -> int:
        return self.a_stack.shape[0]

    @property
    def r_total(self) -> int:
        return self.a_stack.shape[1]

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.a_stack, self.b_stack, self.scale))


def group_supported(k: int, widths: Sequence[int], r_max: int) -> bool:
    return r_max in SUPPORTED_RANKS and k % 128 == 0 and all(w > 0 and w % 16 == 0 for w in widths) and len(widths) <= 4


class LoraStaging(StagedInts):
    """What the LoRA steps of one model reuse from step to step: the pinned staging of the tile lists with its device twin
    (a LoRA step is eager: a twin that moves has nobody to tell) and the fp32 t workspace."""
    first_words = 4096

    def __init__(self):
        super().__init__(lambda: None)
        self.t = None


class LoraBatch:
    """A step's row grouping on the device and the t workspace the step's projections share. `staging`: the model's
    LoraStaging (one pinned buffer reused by every step); None: one of this batch's own (tests, tools)."""
    __slots__ = ("tile_rows", "tile_slots", "num_tiles", "num_tokens", "_staging")

    def __init__(self, row_slots: Sequence[int], num_slots: int, device, staging: LoraStaging = None):
        rows, slots = build_tiles(row_slots, num_slots)
        self.num_tiles, self.num_tokens = int(slots.size), len(row_slots)
        self._staging = staging = staging if staging is not None else LoraStaging()
        if self.num_tiles == 0:
            self.tile_rows = self.tile_slots = None
            return
        words = np.concatenate([slots, rows])       # one buffer, one H2D copy
        staging.ensure(max(words.size, staging.first_words))
        staging.begin()[:words.size] = words
        staging.ship([(0, words.size)])
        self.tile_slots, self.tile_rows = staging.staged[:self.num_tiles], staging.staged[self.num_tiles:words.size]

    def workspace(self, floats: int, device) -> torch.Tensor:
        keep = self._staging
        if keep.t is None or keep.t.numel() < floats:
            keep.t = torch.empty(floats, dtype=torch.float32, device=device)
        return keep.t


def _row_stride(t: torch.Tensor) -> int:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("lora kernels take 2-D activations whose rows are contiguous")
    return int(t.stride(0))


def lora_shrink(x: torch.Tensor, group: LoraGroup, batch: LoraBatch) -> torch.Tensor:
    """t [k_splits, T, r_total] fp32 (rows without an adapter are not written)."""
    _hip.require_gpu_tensor(x, "x")
    tokens, k = x.shape
    if k != group.k or tokens != batch.num_tokens:
        raise ValueError(f"x is {tuple(x.shape)}, the group takes K = {group.k} and the batch has {batch.num_tokens} rows")
    ks = k_splits(k)
    t = batch.workspace(ks * tokens * group.r_total, x.device)[:ks * tokens * group.r_total].view(ks, tokens, group.r_total)
    _hip.call("swl_lora_shrink", t.data_ptr(), x.data_ptr(), group.a_stack.data_ptr(), _hip.ptr(batch.tile_rows),
              _hip.ptr(batch.tile_slots), batch.num_tiles, tokens, k, group.r_total, group.num_slots, _row_stride(x),
              _hip.dtype_code(x.dtype), _hip.stream())
    return t


def lora_expand(y: torch.Tensor, t: torch.Tensor, group: LoraGroup, batch: LoraBatch) -> None:
    """y += scale[slot] * t[part columns] @ B[slot].T for the rows of the batch's tiles, in place (one rounding)."""
    _hip.require_gpu_tensor(y, "y")
    tokens, n = y.shape
    if n != group.n or tokens != batch.num_tokens:
        raise ValueError(f"y is {tuple(y.shape)}, the group has N = {group.n} and the batch has {batch.num_tokens} rows")
    _hip.call("swl_lora_expand", y.data_ptr(), t.data_ptr(), group.b_stack.data_ptr(), group.scale.data_ptr(),
              _hip.ptr(batch.tile_rows), _hip.ptr(batch.tile_slots), ctypes.addressof(group._parts_c), len(group.parts),
              batch.num_tiles, tokens, n, group.r_max, group.r_total, t.shape[0], group.num_slots, _row_stride(y),
              _hip.dtype_code(y.dtype), _hip.stream())


def lora_apply(x: torch.Tensor, y: torch.Tensor, group: LoraGroup, batch: LoraBatch) -> None:
    """The adapter update of one projection: y = linear(x, W) on entry, y + delta(x) for the adapter rows on return."""
    if batch.num_tiles == 0:
        return
    lora_expand(y, lora_shrink(x, group, batch), group, batch)
