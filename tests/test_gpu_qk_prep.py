"""swl_qk_prep_rotary (csrc/qk_prep.hip: projection bias + per-head QK RMSNorm + rotary, one launch, in place) against the
fp64 restatement of its contract in tests/_families_ref.py.

Bound per element of q and k: |out - y| <= 0.5 ulp_dtype(y) + 2^-18 (|a| + |b|), a and b the two products of the element's
rotation in fp64 and ulp floored at the dtype's smallest subnormal. The first term is the one rounding the contract allows;
the second is the fp32 chain's budget — about 16 roundings of 2^-24 relative to the terms is 2^-20, with a factor 4 over it:
1/64 of a float16 half-ulp. A biased v is bit-equal to the torch expression. Everything that is not an operand keeps its bits."""
from types import SimpleNamespace

import pytest
import torch

from _families_ref import qk_prep_ref, ulp_of

pytestmark = pytest.mark.gpu

HEADS = [(4, 2), (5, 1), (8, 8)]        # (5, 1) at D 32: a token is 12 lanes, not a divisor of 64
ROWS = 64                               # rope table rows
SENTINEL = 0x7B5A                       # a finite 16-bit pattern in both dtypes
EPS = 1e-6


class Case:
    """q / k / v as column slices of one fused buffer whose row pitch is larger than the row, with guard rows around it."""

    def __init__(self, dtype, D, H, KVH, T, form, seed, pos="inert"):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        self.dtype, self.D, self.H, self.KVH, self.T = dtype, D, H, KVH, T
        self.row = (H + 2 * KVH) * D
        self.pitch = self.row + 24                  # 16-byte aligned, larger than the row
        buf = torch.full((T + 2, self.pitch), SENTINEL, dtype=torch.int16).view(dtype)
        buf[1:T + 1, :self.row] = (rnd(T, self.row) * 1.5).to(dtype)
        self.host = buf
        inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
        freqs = torch.outer(torch.arange(ROWS, dtype=torch.float32), inv)
        self.cos, self.sin = torch.cos(freqs).to(dtype), torch.sin(freqs).to(dtype)
        if pos == "null":
            self.pos = None
        else:
            self.pos = torch.randint(0, ROWS, (T,), generator=g, dtype=torch.int32)
            if pos == "inert" and T > 2:
                self.pos[3] = self.pos[T - 1] = -1
        norm, bias = form in ("norm", "bias+norm"), form in ("bias", "bias+norm")
        vec = lambda n, mean, std: (mean + std * rnd(n)).to(dtype)     # noqa: E731
        self.q_norm, self.k_norm = (vec(D, 1.0, 0.2), vec(D, 1.0, 0.2)) if norm else (None, None)
        self.q_bias, self.k_bias, self.v_bias = ((vec(H * D, 0, 0.5), vec(KVH * D, 0, 0.5), vec(KVH * D, 0, 0.5)) if bias
                                                 else (None, None, None))

    def views(self, buf):
        H, KVH, D, T = self.H, self.KVH, self.D, self.T
        body = buf[1:T + 1]
        return (body[:, :H * D].view(T, H, D), body[:, H * D:(H + KVH) * D].view(T, KVH, D),
                body[:, (H + KVH) * D:self.row].view(T, KVH, D))

    def vectors(self, dev=None):
        names = ("q_bias", "k_bias", "v_bias", "q_norm", "k_norm")
        return {n: (getattr(self, n) if dev is None or getattr(self, n) is None else getattr(self, n).to(dev)) for n in names}

    def state(self, dev):
        n = self.T if self.pos is None else ROWS
        return SimpleNamespace(position_cos=self.cos[:n].to(dev), position_sin=self.sin[:n].to(dev),
                               position_indices=None if self.pos is None else self.pos.to(dev))

    def run(self, buf=None):
        """One launch on a device copy of the buffer; returns the device buffer."""
        from swiftllm_amd.worker.kernels.rotary_emb import qk_prep_rotary_inplace
        buf = self.host.cuda() if buf is None else buf
        q, k, v = self.views(buf)
        qk_prep_rotary_inplace(q, k, v, self.state(buf.device), eps=EPS, **self.vectors(buf.device))
        return buf

    def check(self, out):
        """The bound on q and k, the bit-equality of v, and the bits of everything that is not an operand."""
        out = out.cpu()
        q0, k0, v0 = self.views(self.host)
        ref = qk_prep_ref(q0, k0, v0, self.cos, self.sin, self.pos, eps=EPS, **self.vectors())
        q, k, v = self.views(out)
        worst = 0.0
        for name, got in (("q", q), ("k", k)):
            y, mag = ref[name], ref[name + "_mag"]
            bound = 0.5 * ulp_of(y, self.dtype) + 2.0 ** -18 * mag
            live = ref["live"][:, None, None].expand_as(y)
            err = (got.double() - y).abs()
            worst = max(worst, float((err / bound)[live].max()) if bool(live.any()) else 0.0)
            assert bool((err <= bound)[live].all()), (name, float((err / bound)[live].max()))
            assert torch.equal(got.view(torch.int16)[~live], getattr(self, "views")(self.host)[0 if name == "q" else 1]
                               .view(torch.int16)[~live]), f"inert rows of {name} moved"
        if self.v_bias is not None:
            want = (v0.float() + self.v_bias.float().view(1, self.KVH, self.D)).to(self.dtype)
            want = torch.where(ref["live"][:, None, None], want, v0)
            assert torch.equal(v.view(torch.int16), want.view(torch.int16)), "v + bias is not the torch expression"
        else:
            assert torch.equal(v.view(torch.int16), v0.view(torch.int16)), "v moved without a bias"
        bits, before = out.view(torch.int16), self.host.view(torch.int16)
        assert torch.equal(bits[0], before[0]) and torch.equal(bits[-1], before[-1]), "a guard row moved"
        assert torch.equal(bits[:, self.row:], before[:, self.row:]), "the padding between rows moved"
        return worst


@pytest.mark.parametrize("form", ["norm", "bias", "bias+norm", "neither"])
@pytest.mark.parametrize("D", [32, 64, 128, 256])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_against_the_fp64_contract(dtype, D, form):
    worst = 0.0
    for (H, KVH), T in ((hk, t) for hk in HEADS for t in (1, 37)):
        case = Case(dtype, D, H, KVH, T, form, seed=1000 * D + 10 * H + T)
        worst = max(worst, case.check(case.run()))
    print(f"qk_prep {form} D={D} {dtype}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("form", ["bias+norm", "neither"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_null_positions_take_row_t(dtype, form):
    for D in (32, 128):
        case = Case(dtype, D, 5, 1, 37, form, seed=D, pos="null")
        case.check(case.run())


@pytest.mark.parametrize("D,H,KVH", [(32, 5, 1), (64, 4, 2), (128, 8, 8), (256, 4, 2)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_a_row_does_not_depend_on_the_batch_or_the_launch(dtype, D, H, KVH):
    case = Case(dtype, D, H, KVH, 37, "bias+norm", seed=7 * D)
    first, second = case.run().cpu(), case.run().cpu()
    assert torch.equal(first.view(torch.int16), second.view(torch.int16)), "two launches differ"
    for r in (0, 20, 35):       # live rows (3 and 36 are inert)
        alone = Case(dtype, D, H, KVH, 1, "bias+norm", seed=7 * D)
        for name in ("q_bias", "k_bias", "v_bias", "q_norm", "k_norm"):
            setattr(alone, name, getattr(case, name))
        alone.host[1] = case.host[1 + r]
        alone.pos = case.pos[r:r + 1].clone()
        got = alone.run().cpu()
        assert torch.equal(got.view(torch.int16)[1], first.view(torch.int16)[1 + r]), f"row {r} alone differs"
    # a batch of one inert row: nothing moves
    inert = Case(dtype, D, H, KVH, 1, "bias+norm", seed=3)
    inert.pos[0] = -1
    assert torch.equal(inert.run().cpu().view(torch.int16), inert.host.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
def test_a_captured_graph_replays_to_the_eager_bits(dtype):
    case = Case(dtype, 128, 4, 2, 37, "bias+norm", seed=11)
    eager = case.run().cpu()
    dev = case.host.cuda()
    pristine = dev.clone()
    vecs, state = case.vectors(dev.device), case.state(dev.device)
    from swiftllm_amd.worker.kernels.rotary_emb import qk_prep_rotary_inplace
    q, k, v = case.views(dev)
    warm = torch.cuda.Stream()
    warm.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(warm):
        qk_prep_rotary_inplace(q, k, v, state, eps=EPS, **vecs)
    torch.cuda.current_stream().wait_stream(warm)
    graph = torch.cuda.CUDAGraph()
    # under inference mode, as LlamaModel captures its decode graphs: torch's capture updates the generator's graph state
    # in place, and that state is an inference tensor once a model of an earlier test has captured a graph
    with torch.inference_mode(), torch.cuda.graph(graph):
        qk_prep_rotary_inplace(q, k, v, state, eps=EPS, **vecs)
    for _ in range(2):
        dev.copy_(pristine)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(dev.cpu().view(torch.int16), eager.view(torch.int16))
