"""The variants of varlen prefill attention at head size 128 give the same BITS: the register-staged kernel
(SWL_PREFILL_ATTN=v1) against the LDS-DMA kernel, and the LDS-DMA kernel under every heads-per-workgroup split
(SWL_PREFILL_HPW = 1 / 2 / 4). The kernels share one tile body and one epilogue (csrc/prefill_tile.h); what differs is
how K/V reach LDS and which wave owns which 32 rows, and neither may change a row's arithmetic.

One varlen batch whose lengths cross the 32-row wave, the 64-key tile, the 64- and 128-row workgroup blocks and leave a
last tile of every kind; q/k/v are views of one fused [T, (H + 2 KVH) D] buffer (the strided form the layer uses). The
longest sequence has scores that RISE along the keys (key row j scaled by 1 + j / 32), so its running maximum moves by
more than kLazyMax in late tiles and the rescale branch runs there too, not on the first tiles only.

Both switches are read once per process: the parent computes the default outputs in-process and starts one fresh child
per variant, one after another, each under its own time limit; this file is the child's program.
Reference semantics of the operator: swiftllm/worker/kernels/prefill_attn.py:102-139.
"""
import os
import subprocess
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = [(32, 8), (8, 8)]
DTYPES = [torch.float16, torch.bfloat16]
D = 128
LENS = [1, 17, 64, 65, 129, 700]
RISING = LENS.index(700)
# (name, environment, which (H, KVH) are compared)
VARIANTS = [("v1", {"SWL_PREFILL_ATTN": "v1"}, lambda G: True),
            ("hpw1", {"SWL_PREFILL_HPW": "1"}, lambda G: True),
            ("hpw4", {"SWL_PREFILL_HPW": "4"}, lambda G: G % 4 == 0)]


def _outputs():
    """{case name: o as int16 [T, H, D] on the CPU} of every case, through the library this process loaded."""
    from swiftllm_amd.worker.kernels.prefill_attn import prefill_attention
    T = sum(LENS)
    cu = torch.zeros(len(LENS) + 1, dtype=torch.int32)
    cu[1:] = torch.cumsum(torch.tensor(LENS, dtype=torch.int32), 0)
    st = types.SimpleNamespace(num_prefill_seqs=len(LENS), max_prefill_len=max(LENS), softmax_scale=D ** -0.5,
                               prefill_seq_start_locs_with_end=cu.cuda())
    outs = {}
    for H, KVH in HEADS:
        for dtype in DTYPES:
            g = torch.Generator().manual_seed(1000 * H + KVH)
            fused = torch.randn(T, H + 2 * KVH, D, generator=g)
            lo = int(cu[RISING])
            fused[lo:lo + LENS[RISING], H:H + KVH] *= (1 + torch.arange(LENS[RISING]) / 32.0)[:, None, None]
            fused = fused.to(dtype).cuda()
            q, k, v = fused[:, :H], fused[:, H:H + KVH], fused[:, H + KVH:]
            o = torch.zeros(T, H, D, dtype=dtype, device="cuda")
            mc = types.SimpleNamespace(num_q_heads=H, num_kv_heads=KVH, head_dim=D)
            prefill_attention(q, k, v, o, mc, None, st)
            torch.cuda.synchronize()
            outs[f"H{H}_KVH{KVH}_{str(dtype).split('.')[-1]}"] = o.view(torch.int16).cpu()
    return outs


def test_register_staged_and_every_heads_per_workgroup_split_give_the_bits_of_the_default(tmp_path):
    assert not {"SWL_PREFILL_ATTN", "SWL_PREFILL_HPW"} & set(os.environ), "the parent runs with the default switches"
    want = _outputs()
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests")
    for name, switches, compared in VARIANTS:
        out = tmp_path / f"{name}.pt"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], cwd=ROOT, env=dict(env, **switches),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stderr[-3000:]}"
        got = torch.load(out)
        assert got.keys() == want.keys()
        n = 0
        for H, KVH in HEADS:
            if not compared(H // KVH):
                continue
            for dtype in DTYPES:
                case = f"H{H}_KVH{KVH}_{str(dtype).split('.')[-1]}"
                same = torch.equal(got[case], want[case])
                rows = (got[case] != want[case]).flatten(1).any(1).nonzero().flatten().tolist()
                assert same, f"{name} {case}: {len(rows)} token rows differ from the default, first {rows[:8]}"
                n += 1
        print(f"\n[prefill variants] {name}: {n} outputs bit-equal to the default")


if __name__ == "__main__":
    torch.save(_outputs(), sys.argv[1])
