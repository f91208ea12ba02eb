"""Dense block-scaled FP8 projections at 65..256 tokens (csrc/gemm_fp8_block_wide.hip; `wide=True` of kernels/linear_fp8.py;
EngineConfig.dense_fp8_wide). The weights, the bound and the model are tests/test_gpu_gemm_fp8_block.py's: every element
against fp64 on the dequantised weights with a = (2^-18 + F 2^-24) sum |x w|, F = ceil(K / 128) + k_splits - 1 for the split
the launch ran (split 0: the WIDE chooser's for the weight rows it streams). The kernel keeps the 64-row kernel's chain, so
at a forced split a row's bits are those of that row sent alone through the 64-row kernel. M: 65 is one row in a fifth
token tile, 129 the first row past any half split of sixteen tiles, 256 every tile full; 200 rows take the 4-tile form
with a partly filled last wave. Every test fails on a tree without the `wide` argument, the option or the entries."""
import json
import os

import pytest
import torch

from swiftllm_amd.worker.kernels import linear_fp8 as L
from swiftllm_amd.worker.weight import dequantise_blocks

import _moe_ref as R
from _families_ref import make_hf_checkpoint
from test_gpu_gemm_fp8_block import DEV, DTYPES, GEOMETRIES, KINDS, STEPS, a_of, splits_of, weights
from test_gpu_model_families import TORCH_DTYPE, _generate, _hf_at_our_positions, _load
from test_gpu_moe_fp8 import bits
from test_gpu_moe_fp8_block import to_block_fp8

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M", [65, 129, 256])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("segments, K", [GEOMETRIES[1], GEOMETRIES[3], GEOMETRIES[4]])
def test_every_element_meets_the_derived_bound(segments, K, dtype, M):
    codes, bscale, deq = weights(segments, K)
    x = torch.randn((M, K), generator=torch.Generator().manual_seed(700 + M + K)).to(dtype)
    xd, h = x.double(), lambda v: 0.5 * R.ulp_of(v, dtype)      # noqa: E731
    ref, mag = xd @ deq.T, xd.abs() @ deq.abs().T
    for ks in splits_of(segments, K):
        a = a_of(mag, K, ks or L.choose_splits_wide(sum(segments), K), None)    # (both forms stream all the weight rows)
        got = L.linear_fp8_block(x.to(DEV), codes, bscale, segments, k_splits=ks, wide=True).cpu().double()
        worst = float(((got - ref).abs() / (h(ref.abs() + a) + a)).max())
        print(f"\n[wide gemm {segments} K={K} M={M} ks={ks} {dtype}] error / bound {worst:.3f}")
        assert float(got.abs().max()) > 0 and worst <= 1.0, (segments, K, M, ks, worst)
        if len(segments) != 2:
            continue
        inter = segments[0]
        act = L.linear_silu_gate_fp8_block(x.to(DEV), codes, bscale, inter, k_splits=ks, wide=True).cpu().double()
        (up, gate), (au, ag) = (ref[:, :inter], ref[:, inter:]), (a[:, :inter], a[:, inter:])
        du, dg, s = au + h(up.abs() + au), ag + h(gate.abs() + ag), R.silu(gate)    # the up_gate_silu bound of the 64-row test
        ds = 1.1 * dg + 2.0 ** -21 * s.abs() + h(s.abs() + 1.1 * dg)
        e = up.abs() * ds + s.abs() * du + du * ds
        worst = float(((act - up * s).abs() / (e + h((up * s).abs() + e))).max())
        print(f"[wide silu_gate ks={ks}] error / bound {worst:.3f}")
        assert float(act.abs().max()) > 0 and worst <= 1.0, (segments, K, M, ks, worst)


def forms_of(segments, K):
    codes, bscale, _ = weights(segments, K)
    forms = [lambda v, ks, wide: L.linear_fp8_block(v, codes, bscale, segments, k_splits=ks, wide=wide)]
    if len(segments) == 2:
        forms.append(lambda v, ks, wide: L.linear_silu_gate_fp8_block(v, codes, bscale, segments[0], k_splits=ks, wide=wide))
    return forms


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("segments, K", [GEOMETRIES[1], GEOMETRIES[3]])
def test_a_row_has_the_bits_of_the_64_row_kernel_and_launches_repeat(segments, K, dtype):
    x = torch.randn((200, K), generator=torch.Generator().manual_seed(71)).to(dtype).to(DEV)
    for form in forms_of(segments, K):
        for ks in (1, L.max_splits(K)):
            full = form(x, ks, True)
            assert torch.equal(bits(full), bits(form(x, ks, True)))
            for t in (0, 64, 128, 199):
                assert torch.equal(bits(form(x[t:t + 1], ks, False)), bits(full[t:t + 1])), (ks, t)


@pytest.mark.parametrize("M", [64, 257])
def test_the_option_leaves_the_other_row_counts_on_their_routes(M):
    segments, K = GEOMETRIES[3]
    x = torch.randn((M, K), generator=torch.Generator().manual_seed(72)).to(torch.bfloat16).to(DEV)
    for form in forms_of(segments, K):
        assert torch.equal(bits(form(x, 0, True)), bits(form(x, 0, False)))


# ---- model ---------------------------------------------------------------------------------------------------------------
_CHECKPOINTS = {}


def checkpoint(tmp_path_factory, dtype):
    """(path, HF fp32 model holding the DEQUANTISED projections) of the 64-row module's tiny `llama` kind, once per dtype."""
    if dtype not in _CHECKPOINTS:
        name, overrides, seed = KINDS["llama"]
        path = str(tmp_path_factory.mktemp(f"dense_fp8_wide_{dtype}"))
        hf = make_hf_checkpoint(path, name, TORCH_DTYPE[dtype], seed, **overrides)
        file = to_block_fp8(path)
        with open(os.path.join(path, "config.json"), encoding="utf-8") as f:
            config = dict(json.load(f), model_type="llama", architectures=["LlamaForCausalLM"])
        with open(os.path.join(path, "config.json"), "w", encoding="utf-8") as f:
            json.dump(config, f)
        for key, p in hf.named_parameters():
            if key + "_scale_inv" in file:
                p.data.copy_(dequantise_blocks(file[key], file[key + "_scale_inv"], TORCH_DTYPE[dtype]).float())
        _CHECKPOINTS[dtype] = (path, hf)
    return _CHECKPOINTS[dtype]


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_model_steps_of_80_and_130_tokens_run_fp8_kernels_only_and_stay_within_the_gate(tmp_path_factory, dtype):
    path, hf = checkpoint(tmp_path_factory, dtype)
    g = torch.Generator().manual_seed(73)
    prompts = [torch.randint(3, hf.config.vocab_size, (n,), generator=g).tolist() for n in (80, 130)]
    L._scratch.clear()
    model = _load(path, dtype, dense_weight_dtype="fp8_block", dense_fp8_wide=True)
    (scratch,) = L._scratch.values()                        # still reserved at load: steps above 256 tokens need it
    with torch.inference_mode():
        scratch.fill_(float("nan"))
    runs = [_generate(model, [p], steps=STEPS, seq_ids=[i]) for i, p in enumerate(prompts)]    # a prefill of 80, one of 130
    assert bool(torch.isnan(scratch).all()), "a projection took the dequantising route"
    streams, logits = [r[0][0] for r in runs], torch.cat([r[1] for r in runs], dim=1)
    lg32 = _hf_at_our_positions(hf, prompts, streams, torch.float32)
    lg16 = _hf_at_our_positions(hf, prompts, streams, TORCH_DTYPE[dtype])
    d_ours, d_ref16 = (logits - lg32).abs().max().item(), (lg16 - lg32).abs().max().item()
    print(f"\n[dense fp8 wide {dtype}] d_ours {d_ours:.3e}  d_ref16 {d_ref16:.3e}  ratio {d_ours / d_ref16:.2f}")
    assert lg32.shape == logits.shape and d_ours <= 1.5 * d_ref16, (d_ours, d_ref16)


def test_graph_replay_of_72_sequences_gives_the_bits_of_eager_launches(tmp_path_factory):
    path, hf = checkpoint(tmp_path_factory, "bfloat16")
    g = torch.Generator().manual_seed(74)
    prompts = [torch.randint(3, hf.config.vocab_size, (3,), generator=g).tolist() for _ in range(72)]
    kw = dict(num_blocks=96, dense_weight_dtype="fp8_block", dense_fp8_wide=True, max_batch_size=96, max_seqs_in_block_table=96)
    got = {}
    for graph in (True, False):                             # decode steps of 72 rows: replayed in the 96 bucket, eager as 72
        model = _load(path, "bfloat16", use_hip_graph=graph, **kw)
        got[graph] = _generate(model, prompts, steps=STEPS)
        assert (model.replay.captures >= 1) == graph
    assert got[True][0] == got[False][0] and torch.equal(got[True][1], got[False][1])
