"""Seeded sampling on CPU: the Philox known answers of the reference helper, SamplingParams validation, the C ABI's
argument checks, the HTTP fields, and how the engine hands per-request parameters to the data plane."""
import asyncio
import types

import numpy as np
import pytest

from swiftllm_amd import SamplingParams, _hip
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.server import Engine, RawRequest, Request
from swiftllm_amd.worker.kernels.sampling import pack_params

from _sampling_ref import philox4x32_10, sample_row, uniforms


def _cfg(**kw):
    base = dict(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=64,
                max_seqs_in_block_table=16, max_blocks_per_seq=64, max_batch_size=4, max_tokens_in_batch=100)
    base.update(kw)
    return EngineConfig(**base)


@pytest.mark.parametrize("key,ctr,want", [
    ((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(key, ctr, want):
    got = philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert " ".join(f"{w:08x}" for w in got) == want


def test_uniforms_strictly_inside_the_unit_interval():
    u = uniforms(12345, 7, 4096)
    assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24
    assert np.float32(u.max()) < 1.0      # exact in fp32 too: the noise is always finite


def test_reference_sampler_greedy_and_filters():
    f = np.array([1.0, 3.0, 3.0, np.nan, -np.inf, 2.0])
    assert sample_row(f, 0.0, 0, 1.0, 1, 1)[0] == 1          # lowest index among equal maxima, NaN skipped
    assert sample_row(np.array([np.nan, -np.inf]), 0.7, 0, 1.0, 1, 1)[0] == 0
    for seed in range(64):
        assert sample_row(f, 1.0, 2, 1.0, seed, 5)[0] in (1, 2)      # top-2: the tied pair only
        assert sample_row(f, 5.0, 0, 0.3, seed, 5)[0] in (1, 2)      # their mass alone exceeds 0.3


def test_sampling_params_validation():
    assert SamplingParams().greedy and SamplingParams(0.0, top_k=5).greedy
    SamplingParams(0.8, top_k=40, top_p=0.95, seed=2 ** 64 - 1)
    for kw in (dict(temperature=-0.1), dict(temperature=float("nan")), dict(temperature=float("inf")),
               dict(temperature="1"), dict(temperature=True), dict(top_k=-1), dict(top_k=1.5), dict(top_k=True),
               dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan")), dict(seed=-1), dict(seed=2 ** 64),
               dict(seed=1.0)):
        with pytest.raises(ValueError):
            SamplingParams(**kw)
    a = SamplingParams(1.0)
    s1, s2 = a.with_seed(), a.with_seed()
    assert s1.seed is not None and s1.seed != s2.seed and s1.with_seed() is s1


def test_swiftllm_alias_exports_sampling_params():
    import swiftllm
    assert swiftllm.SamplingParams is SamplingParams


def test_pack_params_layout():
    buf = pack_params([None, SamplingParams(0.5, 3, 0.9, seed=(7 << 32) | 5), SamplingParams(0.0)],
                      np.full(5 * 4, -1, dtype=np.int32))
    seeds = buf[:8].reshape(4, 2)
    assert seeds.tolist() == [[0, 0], [5, 7], [0, 0], [0, 0]]
    assert buf[8:12].view(np.float32).tolist() == [0.0, 0.5, 0.0, 0.0]      # greedy rows and padding: T = 0
    assert buf[12:16].tolist() == [0, 3, 0, 0]
    assert np.allclose(buf[16:20].view(np.float32), [1.0, 0.9, 1.0, 1.0])


def test_sample_abi_rejects_bad_arguments_without_a_gpu():
    lib = _hip.load()
    p = 16      # any non-null pointer value: validation happens before anything is dereferenced or launched
    args = lambda **kw: [kw.get(k, d) for k, d in (("out", p), ("x", p), ("rows", 4), ("n", 1000), ("stride", 1000),
                                                   ("dtype", _hip.SWL_BF16), ("t", p), ("k", p), ("pp", p), ("s", p),
                                                   ("pos", p), ("stream", None))]
    assert lib.swl_sample(*args(rows=0)) == 0                       # empty batch: no launch
    assert lib.swl_sample(*args(rows=-1)) == -1
    assert lib.swl_sample(*args(n=0)) == -1
    assert lib.swl_sample(*args(stride=999)) == -1                  # row stride below the width
    assert lib.swl_sample(*args(dtype=7)) == -1
    assert lib.swl_sample(*args(x=None)) == -1
    assert lib.swl_sample(*args(s=None)) == -1
    assert lib.swl_sample(*args(pos=None)) == -1
    assert lib.swl_sample(*args(x=17)) == -1                        # 16-bit elements need 2-byte alignment


# ---- engine and HTTP with a fake data plane ------------------------------------------------------------------------------
class ThreeArgModel:
    """The data plane as the existing fakes have it: forward takes exactly three arguments."""
    num_blocks = 8

    def __init__(self):
        self.model_config = types.SimpleNamespace()
        self.calls = 0

    def forward(self, input_ids, seq_ids, decoding_lens):
        self.calls += 1
        return [len(x) % 97 for x in input_ids]

    def swap_in_seqs(self, ids):
        pass

    def swap_out_seqs(self, ids):
        pass

    def free_seqs_resources(self, ids):
        pass


class SamplingModel(ThreeArgModel):
    """Records the sampling_params of every call; the token is (seed + position) % 97 for a sampled row."""

    def __init__(self):
        super().__init__()
        self.seen = []      # (seq_id, position, SamplingParams or None)

    def forward(self, input_ids, seq_ids, decoding_lens, sampling_params=None):
        assert sampling_params is not None and len(sampling_params) == len(input_ids)
        n_pre = len(input_ids) - len(decoding_lens)
        lens = [len(x) for x in input_ids[:n_pre]] + list(decoding_lens)
        out = []
        for sid, n, sp in zip(seq_ids, lens, sampling_params):
            self.seen.append((sid, n, sp))
            out.append(0 if sp is None else (sp.seed + n) % 97)
        return out


def _run(model, raws, **cfg):
    async def run():
        eng = Engine(_cfg(**cfg), model=model)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        done = await asyncio.wait_for(asyncio.gather(*(eng.add_request_and_wait(r) for r in raws)), timeout=20)
        loops.cancel()
        return eng, done
    return asyncio.run(run())


def test_engine_keeps_the_three_argument_call_for_greedy_batches():
    model = ThreeArgModel()
    _, done = _run(model, [RawRequest("", 3, [1, 2]), RawRequest("", 2, [5], sampling_params=SamplingParams(0.0)),
                           RawRequest("", 2, [6, 6, 6], sampling_params=None)])
    assert model.calls > 0 and all(req.error is None for req, _ in done)


def test_engine_passes_aligned_params_for_mixed_batches():
    model = SamplingModel()
    greedy = RawRequest("", 3, [1, 2])
    hot = RawRequest("", 3, [4, 4, 4], sampling_params=SamplingParams(0.7, top_p=0.9, seed=1000))
    cold = RawRequest("", 3, [9], sampling_params=SamplingParams(1.2))
    _, done = _run(model, [greedy, hot, cold])
    (rg, tg), (rh, th), (rc, tc) = done
    assert tg == [0, 0, 0]
    assert th == [(1000 + 3 + i) % 97 for i in range(3)]       # position = prompt 3, then 4, 5
    assert rc.sampling_params.seed is not None                   # resolved once, at enqueue
    assert tc == [(rc.sampling_params.seed + 1 + i) % 97 for i in range(3)]
    by_seq = {}
    for sid, n, sp in model.seen:
        by_seq.setdefault(sid, set()).add(None if sp is None else sp.seed)
    assert {frozenset(v) for v in by_seq.values()} == {frozenset({None}), frozenset({1000}),
                                                       frozenset({rc.sampling_params.seed})}


def test_request_seed_survives_swap_out_and_in():
    """Two long requests overflow an 8-block pool: one is swapped out and back in; its seed never changes and the
    positions it samples at continue where they stopped."""
    model = SamplingModel()
    swaps = []
    orig_out, orig_in = model.swap_out_seqs, model.swap_in_seqs
    model.swap_out_seqs = lambda ids: (swaps.append(("out", list(ids))), orig_out(ids))
    model.swap_in_seqs = lambda ids: (swaps.append(("in", list(ids))), orig_in(ids))
    raws = [RawRequest("", 40, list(range(31)), sampling_params=SamplingParams(0.9)) for _ in range(2)]
    model.num_blocks = 8     # 5 blocks each by the end: one request is swapped out
    eng, done = _run(model, raws, max_tokens_in_batch=1000)
    assert all(req.error is None for req, _ in done)
    assert eng.num_swapped_out > 0 and eng.num_swapped_in > 0 and ("out", [1]) in swaps
    for req, toks in done:
        sid_rows = [(n, sp) for _, n, sp in model.seen if sp is not None and sp.seed == req.sampling_params.seed]
        assert [n for n, _ in sid_rows] == list(range(31, 71))     # one draw per position, in order
        assert toks == [(req.sampling_params.seed + n) % 97 for n, _ in sid_rows]


def test_request_resolves_seed_once():
    r = Request(RawRequest("", 2, [1], sampling_params=SamplingParams(0.5)))
    assert r.sampling_params.seed is not None
    assert Request(RawRequest("", 2, [1], sampling_params=SamplingParams(0.0))).sampling_params is None
    assert Request(RawRequest("", 2, [1], sampling_params=SamplingParams(0.5, seed=3))).sampling_params.seed == 3


def test_api_sampling_fields():
    from fastapi.testclient import TestClient
    from swiftllm_amd.server.api_server import build_app

    model = SamplingModel()

    async def boot():
        eng = Engine(_cfg(), model=model)
        await eng.initialize()
        return eng
    loop = asyncio.new_event_loop()
    eng = loop.run_until_complete(boot())
    app = build_app(eng)

    @app.on_event("startup")
    async def start_loops():
        eng.event_loop = asyncio.get_running_loop()
        asyncio.ensure_future(eng.start_all_event_loops())
    base = {"prompt_token_ids": [4, 5], "output_len": 3}
    with TestClient(app) as client:
        for bad in (dict(temperature=-1), dict(temperature="0.5"), dict(temperature=True),
                    dict(top_k=-1), dict(top_k=2.5), dict(top_k="3"), dict(top_p=0), dict(top_p=1.5),
                    dict(top_p="0.9"), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5), dict(seed=False)):
            r = client.post("/generate", json={**base, **bad})
            assert r.status_code == 400 and "error" in r.json(), bad
        body = {**base, "temperature": 0.8, "top_k": 50, "top_p": 0.9, "seed": 2 ** 64 - 1}
        r = client.post("/generate", json=body)
        assert r.status_code == 200 and r.json() == {"output_token_ids": [(2 ** 64 - 1 + n) % 97 for n in (2, 3, 4)]}
        r = client.post("/generate", json={**body, "stream": True})
        assert [int(x) for x in r.text.split()] == [(2 ** 64 - 1 + n) % 97 for n in (2, 3, 4)]
        r = client.post("/generate", json={**base, "temperature": 1, "top_p": 1})
        assert r.status_code == 200
    assert any(sp is not None and sp.top_k == 50 and sp.top_p == 0.9 for _, _, sp in model.seen)
