"""Arena harness: run an operation with every operand placed inside ONE allocation, at its minimum legal alignment and
with padded strides, and check where it wrote and what it let into its outputs.

An Arena is one uint8 tensor filled with a single byte. `place()` copies an operand in at a base address that is `skew`
modulo 256 (an operand legal at 16 bytes sits at 16 mod 32, one legal at 8 at 8 mod 16, one legal at 2 at 2 mod 4), with
a margin of fill bytes before and after it, and returns a view with the requested row stride. Outputs (and in/out
operands, and scratch) are declared as regions of rows x width bytes with a stride; `assert_untouched()` compares every
other byte of the arena — the padding columns between output rows included — with a copy taken before the call.

`run_case()` runs one operation three times on the same data: on plain tensors (the control; scratch zero-filled), in
a 0xFF arena and in a 0x00 arena (scratch pre-filled with 0xFF in both, at exactly its advertised size). 0xFF is NaN in
fp16 / bf16 / fp32 and -1 in every integer type, so a value from beyond an input or from an unwritten scratch slot that
reaches an output changes it between the runs; the outputs of the three runs must be bit-identical.

Margins are a condition of the method, not a knob: each is at least 256 KiB and larger than one outer-dimension step of
any indexed operand of the case (for a KV pool: one block), so an index read from the fill (-1) dereferences one step in
front of its buffer, which is still inside the arena. No test built on this may make a kernel touch memory outside its
one allocation.

What this cannot see: a read outside an operand whose value never reaches an output (a prefetch that is discarded, a
clamped row that is masked later) leaves no trace here.
"""
import torch

MIN_MARGIN = 256 * 1024


class Op:
    """One operand of a case.

    data    CPU tensor holding the input values; dim 0 is the row dimension when `stride` is given
    skew    minimum legal alignment of the base address in bytes (the base sits at skew mod 2 * skew)
    stride  row stride in elements (None: contiguous)
    out     the operation may write it (in/out operands too): compared with the control, and a declared region
    scratch contents are undefined before and after the call: zero-filled in the control, 0xFF-filled in the arenas, sized
            exactly as given; a declared region, never compared
    """

    def __init__(self, data, skew=16, stride=None, out=False, scratch=False):
        assert data.is_contiguous()
        self.data, self.skew, self.stride, self.out, self.scratch = data, skew, stride, out or scratch, scratch
        if stride is not None:
            assert data.dim() >= 2 and stride >= data[0].numel()

    @property
    def row_elems(self):
        return self.data[0].numel() if self.stride is not None else self.data.numel()

    @property
    def rows(self):
        return self.data.shape[0] if self.stride is not None else 1

    @property
    def span_bytes(self):
        """First to last byte the operand's elements occupy."""
        e = self.data.element_size()
        if self.stride is None:
            return self.data.numel() * e
        return ((self.rows - 1) * self.stride + self.row_elems) * e


class Arena:
    def __init__(self, fill, device, capacity, margin=MIN_MARGIN):
        assert margin >= MIN_MARGIN and 0 <= fill <= 255
        self.fill, self.margin = fill, margin
        self.buf = torch.full((capacity + 512,), fill, dtype=torch.uint8, device=device)
        self._origin = (-self.buf.data_ptr()) % 256       # offset of the first 256-byte aligned address
        self._cursor = self._origin + margin
        self.regions = []                                  # (name, offset, rows, width_bytes, stride_bytes)
        self._snap = None

    @staticmethod
    def capacity_for(ops, margin=MIN_MARGIN):
        return margin + sum(op.span_bytes + 512 + margin for op in ops)

    def place(self, op, name="?"):
        """Copy `op` in; return the view the operation gets."""
        skew, e = op.skew, op.data.element_size()
        assert skew in (1, 2, 4, 8, 16, 32, 64, 128) and skew % e == 0, (name, skew, e)
        off = self._origin + (self._cursor - self._origin + 255) // 256 * 256 + (skew % 256)
        assert (self.buf.data_ptr() + off) % 256 == skew % 256
        end = off + op.span_bytes
        assert end + self.margin <= self.buf.numel(), "arena too small for its operands and margins"
        self._cursor = end + self.margin
        flat = self.buf[off:end].view(op.data.dtype)
        if op.stride is None:
            view = flat.view(op.data.shape)
        else:
            inner = op.data[0].contiguous().stride() if op.data.dim() > 1 else ()
            view = flat.as_strided(op.data.shape, (op.stride,) + tuple(inner))
        if op.scratch:
            self.buf[off:end] = 0xFF
        else:
            view.copy_(op.data.to(self.buf.device))
        if op.out:
            self.declare_output(name, off, op.rows, op.row_elems * e, (op.stride or op.row_elems) * e)
        return view

    def declare_output(self, name, offset, rows, width_bytes, stride_bytes):
        self.regions.append((name, offset, rows, width_bytes, stride_bytes))

    def snapshot(self):
        self._snap = self.buf.clone()

    def assert_untouched(self):
        assert self._snap is not None, "snapshot() before the call"
        free = torch.ones(self.buf.numel(), dtype=torch.bool, device=self.buf.device)
        for _, off, rows, width, stride in self.regions:
            free[off:off + (rows - 1) * stride + width].as_strided((rows, width), (stride, 1)).fill_(False)
        changed = ((self.buf != self._snap) & free).nonzero().flatten()
        if changed.numel():
            first = int(changed[0])
            near = min(self.regions, key=lambda r: min(abs(first - r[1]), abs(first - (r[1] + (r[2] - 1) * r[4] + r[3]))),
                       default=None)
            where = ""
            if near is not None:
                name, off, rows, width, stride = near
                rel = first - off
                where = (f"; nearest region {name!r}: byte {rel} from its base (rows {rows} x {width} B, stride {stride} B"
                         f"{', a padding column' if 0 <= rel < (rows - 1) * stride + width else ''})")
            raise AssertionError(f"{changed.numel()} bytes outside the declared outputs changed (fill 0x{self.fill:02X}), "
                                 f"first at arena offset {first}{where}")


def _bits(t):
    return t.contiguous().view(torch.uint8)


def run_case(ops, call, device, margin=MIN_MARGIN, sync=None, same_path=True, check=None):
    """ops: {name: Op}; call(views): runs the operation on {name: tensor}; returns nothing.

    Control on plain tensors (contiguous unless a stride is given: then the same padded stride, zero padding), then the
    0xFF and the 0x00 arena. Outputs must be bit-identical across the three runs and nothing outside them may change. With
    same_path=False (an entry that picks another code path by alignment) `check(name, control, got)` judges an output
    whose bits differ instead. Returns the control's outputs {name: CPU tensor}."""
    margin = max(margin, MIN_MARGIN)
    sync = sync or (lambda: None)

    def plain(op):
        if op.stride is None:
            t = torch.zeros(op.data.shape, dtype=op.data.dtype, device=device)
        else:
            rows = op.data.shape[0]
            t = torch.zeros(rows * op.stride, dtype=op.data.dtype, device=device)
            inner = op.data[0].contiguous().stride() if op.data.dim() > 1 else ()
            t = t.as_strided(op.data.shape, (op.stride,) + tuple(inner))
        if not op.scratch:
            t.copy_(op.data.to(device))
        return t

    control = {name: plain(op) for name, op in ops.items()}
    call(control)
    sync()
    want = {name: control[name].cpu().clone() for name, op in ops.items() if op.out and not op.scratch}
    for fill in (0xFF, 0x00):
        arena = Arena(fill, device, Arena.capacity_for(ops.values(), margin), margin)
        views = {name: arena.place(op, name) for name, op in ops.items()}
        arena.snapshot()
        call(views)
        sync()
        for name, ref in want.items():
            got = views[name].cpu()
            if torch.equal(_bits(got), _bits(ref)):
                continue
            if not same_path and check is not None:
                check(name, ref, got)
                continue
            diff = (_bits(got) != _bits(ref)).nonzero()
            raise AssertionError(f"output {name!r} in the 0x{fill:02X} arena differs from the control in "
                                 f"{diff.shape[0]} bytes, first at {diff[0].tolist()}")
        arena.assert_untouched()
    return want
