"""Multi-LoRA serving on the host: the PEFT loader and the slot stacks (on CPU tensors), the configuration, the tile
builder, and the engine / scheduler / HTTP layer over a fake data plane. No device is touched."""
import argparse
import asyncio
import threading
import types

import pytest
import torch

from oracle import synth
from swiftllm_amd import LlamaModelConfig
from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.server import Engine, RawRequest, Request, Scheduler
from swiftllm_amd.worker.kernels.lora import build_tiles
from swiftllm_amd.worker.lora import LoraError, LoraStore, rows_of_sequences

import _lora as L

CFG = synth.make_config(**synth.TINY)       # hidden 128, 4 q / 2 kv heads of 32, FFN 256, 2 layers


def _store(max_loras=2, r_max=16, fuse_qkv=True, dtype=torch.float16):
    return LoraStore(LlamaModelConfig(CFG), max_loras, r_max, dtype, "cpu", fuse_qkv=fuse_qkv)


# ---- the loader -------------------------------------------------------------------------------------------------------------
def test_a_peft_directory_loads_into_the_slot_stacks(tmp_path):
    store = _store()
    modules = ("q_proj", "v_proj", "up_proj", "gate_proj", "down_proj")         # k_proj and o_proj are absent
    adapter = L.random_adapter(CFG, 8, seed=1, modules=modules)
    path = L.write_peft_dir(str(tmp_path / "a"), adapter, L.adapter_config(8, alpha=32, modules=modules))
    assert store.load("a", path) == 0 and store.names() == {"a": 0}
    for layer in range(2):
        g = store.layers[layer]
        qkv, o, ug, down = g.qkv_proj, g.o_proj, g.up_gate_proj, g.down_proj
        assert qkv.a_stack.shape == (2, 48, 128) and qkv.b_stack.shape == (2, 256, 16) and qkv.scale.dtype == torch.float32
        assert qkv.parts == ((0, 128, 0), (128, 192, 16), (192, 256, 32))
        assert ug.a_stack.shape == (2, 32, 128) and ug.b_stack.shape == (2, 512, 16) and ug.parts == ((0, 256, 0), (256, 512, 16))
        assert down.a_stack.shape == (2, 16, 256) and down.b_stack.shape == (2, 128, 16)
        # q: rows [0, 8) of its part hold A, the rank padding [8, 16) is zero; B fills columns [0, 8) of the q rows
        assert torch.equal(qkv.a_stack[0, 0:8], adapter[L.peft_key(layer, "q_proj", "A")])
        assert not qkv.a_stack[0, 8:16].any()
        assert torch.equal(qkv.b_stack[0, 0:128, :8], adapter[L.peft_key(layer, "q_proj", "B")])
        assert not qkv.b_stack[0, :, 8:].any()
        # k is absent: its part stays zero; v sits in the third part
        assert not qkv.a_stack[0, 16:32].any() and not qkv.b_stack[0, 128:192].any()
        assert torch.equal(qkv.a_stack[0, 32:40], adapter[L.peft_key(layer, "v_proj", "A")])
        assert torch.equal(qkv.b_stack[0, 192:256, :8], adapter[L.peft_key(layer, "v_proj", "B")])
        assert not o.a_stack.any() and not o.b_stack.any()
        # [up ; gate], as the weight tensor
        assert torch.equal(ug.a_stack[0, 0:8], adapter[L.peft_key(layer, "up_proj", "A")])
        assert torch.equal(ug.a_stack[0, 16:24], adapter[L.peft_key(layer, "gate_proj", "A")])
        assert torch.equal(ug.b_stack[0, 256:512, :8], adapter[L.peft_key(layer, "gate_proj", "B")])
        assert torch.equal(down.b_stack[0, :, :8], adapter[L.peft_key(layer, "down_proj", "B")])
        for grp in (qkv, o, ug, down):
            assert grp.scale.tolist() == [4.0, 0.0]                 # alpha / r; the free slot stays zero
            assert not grp.a_stack[1].any() and not grp.b_stack[1].any()


def test_unfused_qkv_has_one_group_per_projection():
    store = _store(fuse_qkv=False)
    adapter = L.random_adapter(CFG, 16, seed=2)
    store.load("a", state_dict=adapter, config=L.adapter_config(16))
    g = store.layers[1]
    assert set(g.groups) == {"q_proj", "k_proj", "v_proj", "o_proj", "up_gate_proj", "down_proj"}
    assert g.k_proj.a_stack.shape == (2, 16, 128) and g.k_proj.b_stack.shape == (2, 64, 16)
    assert torch.equal(g.k_proj.a_stack[0], adapter[L.peft_key(1, "k_proj", "A")])
    assert torch.equal(g.v_proj.b_stack[0], adapter[L.peft_key(1, "v_proj", "B")])
    assert g.q_proj.scale.tolist() == [1.0, 0.0]


def test_unload_zeroes_the_slot_and_frees_it():
    store = _store()
    a, b = L.random_adapter(CFG, 16, seed=3), L.random_adapter(CFG, 4, seed=4)
    assert store.load("a", state_dict=a, config=L.adapter_config(16)) == 0
    assert store.load("b", state_dict=b, config=L.adapter_config(4)) == 1
    assert store.unload("a") == 0 and store.names() == {"b": 1}
    for layer in store.layers:
        for grp in layer.groups.values():
            assert not grp.a_stack[0].any() and not grp.b_stack[0].any() and grp.scale[0] == 0
            assert grp.a_stack[1].any() and grp.scale[1] == 1.0
    with pytest.raises(LoraError, match="unknown LoRA adapter 'a'"):
        store.slot_of("a")
    # the freed slot takes the next adapter; what the rank-16 one left beyond rank 4 is gone
    assert store.load("c", state_dict=b, config=L.adapter_config(4)) == 0
    assert not store.layers[0].o_proj.a_stack[0, 4:].any() and store.layers[0].o_proj.a_stack[0, :4].any()


def _refused(store, match, adapter=None, name="x", **config):
    adapter = L.random_adapter(CFG, 8, seed=5) if adapter is None else adapter
    cfg = L.adapter_config(config.pop("r", 8))
    cfg.update(config)
    before = {k: v for k, v in store.names().items()}
    with pytest.raises(LoraError, match=match):
        store.load(name, state_dict=adapter, config=cfg)
    assert store.names() == before
    assert isinstance(LoraError("x"), ValueError)


def test_everything_the_lora_path_cannot_serve_is_refused_with_a_reason(tmp_path):
    store = _store(max_loras=2, r_max=16)
    _refused(store, "rank 32 exceeds max_lora_rank", adapter=L.random_adapter(CFG, 32, seed=5), r=32)
    _refused(store, "unknown target module", target_modules=["q_proj", "router"])
    _refused(store, "embedding / lm_head", target_modules=["q_proj", "lm_head"])
    _refused(store, "embedding / lm_head", target_modules=["embed_tokens"])
    _refused(store, "modules_to_save", modules_to_save=["lm_head"])
    _refused(store, "use_dora", use_dora=True)
    _refused(store, "use_rslora", use_rslora=True)
    _refused(store, "bias='all'", bias="all")
    emb = L.random_adapter(CFG, 8, seed=5)
    emb["base_model.model.model.embed_tokens.lora_embedding_A"] = torch.zeros(8, 256)
    _refused(store, "embedding / lm_head", adapter=emb)
    odd = L.random_adapter(CFG, 8, seed=5)
    odd["base_model.model.model.layers.0.mlp.router.lora_A.weight"] = torch.zeros(8, 128)
    _refused(store, "unknown target module", adapter=odd)
    deep = {k.replace("layers.1.", "layers.7."): v for k, v in L.random_adapter(CFG, 8, seed=5).items()}
    _refused(store, "names layer 7", adapter=deep)
    wrong = L.random_adapter(CFG, 8, seed=5)
    wrong[L.peft_key(0, "k_proj", "B")] = torch.zeros(128, 8, dtype=torch.float16)          # k has 64 outputs
    _refused(store, "this model needs", adapter=wrong)
    wrong = L.random_adapter(CFG, 8, seed=5)
    wrong[L.peft_key(1, "down_proj", "A")] = torch.zeros(8, 128, dtype=torch.float16)       # down reads 256 inputs
    _refused(store, "this model needs", adapter=wrong)
    half = L.random_adapter(CFG, 8, seed=5)
    del half[L.peft_key(0, "o_proj", "B")]
    _refused(store, "only one of lora_A / lora_B", adapter=half)
    for layer in store.layers:                      # nothing was written by any refusal
        assert not any(g.a_stack.any() or g.b_stack.any() for g in layer.groups.values())
    with pytest.raises(LoraError, match="not a PEFT adapter directory"):
        store.load("x", str(tmp_path / "nowhere"))
    good = L.random_adapter(CFG, 8, seed=5)
    store.load("a", state_dict=good, config=L.adapter_config(8))
    _refused(store, "already loaded", name="a")
    store.load("b", state_dict=good, config=L.adapter_config(8))
    _refused(store, "no free LoRA slot", name="c")
    with pytest.raises(LoraError, match="max_lora_rank must be one of"):
        _store(r_max=24)
    odd_model = synth.make_config(**dict(synth.TINY, hidden_size=96, num_attention_heads=3, num_key_value_heads=3))
    with pytest.raises(LoraError, match="multiple of 128"):
        LoraStore(LlamaModelConfig(odd_model), 1, 16, torch.float16, "cpu")


# ---- configuration ----------------------------------------------------------------------------------------------------------
def _cfg(**kw):
    base = dict(model_path="", use_dummy=True, block_size=16, gpu_mem_utilization=0.9, num_cpu_blocks=64,
                max_seqs_in_block_table=16, max_blocks_per_seq=64, max_batch_size=4, max_tokens_in_batch=100)
    base.update(kw)
    return EngineConfig(**base)


def test_engine_config_defaults_refusals_and_cli_round_trip():
    c = _cfg()
    assert (c.max_loras, c.max_lora_rank, c.lora_modules) == (0, 16, None)
    with pytest.raises(ValueError, match="fp8_e4m3"):
        _cfg(max_loras=2, kv_cache_dtype="fp8_e4m3")
    with pytest.raises(ValueError, match="decode_engine"):
        _cfg(max_loras=2, tuning={"decode_engine": True})
    _cfg(max_loras=0, kv_cache_dtype="fp8_e4m3")            # (off: nothing to refuse)
    with pytest.raises(ValueError, match="max_lora_rank"):
        _cfg(max_loras=2, max_lora_rank=24)
    with pytest.raises(ValueError, match="max_loras"):
        _cfg(max_loras=-1)
    with pytest.raises(ValueError, match="needs max_loras"):
        _cfg(lora_modules=["a=/x"])
    with pytest.raises(ValueError, match="NAME=PATH"):
        _cfg(max_loras=2, lora_modules=["a"])
    with pytest.raises(ValueError, match="twice"):
        _cfg(max_loras=2, lora_modules=["a=/x", "a=/y"])
    with pytest.raises(ValueError, match="names 3 adapters"):
        _cfg(max_loras=2, lora_modules=["a=/x", "b=/y", "c=/z"])
    ap = argparse.ArgumentParser()
    EngineConfig.add_cli_args(ap)
    args = ap.parse_args(["--model-path", "/m", "--max-loras", "3", "--max-lora-rank", "32", "--lora", "a=/x", "--lora",
                          "b=/y=z"])
    c = EngineConfig(**vars(args))
    assert (c.max_loras, c.max_lora_rank, c.lora_modules) == (3, 32, ["a=/x", "b=/y=z"])
    c = EngineConfig(**vars(ap.parse_args(["--model-path", "/m"])))
    assert (c.max_loras, c.max_lora_rank, c.lora_modules) == (0, 16, None)
    from swiftllm_amd.worker.lora import parse_lora_modules
    assert parse_lora_modules(["a=/x", "b=/y=z"]) == {"a": "/x", "b": "/y=z"} and parse_lora_modules(None) == {}
    from swiftllm_amd.server.router import lora_passthrough
    assert lora_passthrough(2, 32, ["a=/x"]) == ["--max-loras", "2", "--max-lora-rank", "32", "--lora", "a=/x"]
    assert lora_passthrough(None, None, None) == []
    with pytest.raises(SystemExit):
        lora_passthrough(None, None, ["a=/x"])


# ---- the tile builder -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 16, 17])
def test_tiles_group_rows_by_slot(t):
    def check(row_slots):
        rows, slots = build_tiles(row_slots, 4)
        assert rows.dtype.name == "int32" and slots.dtype.name == "int32" and rows.size == 16 * slots.size
        seen = []
        for i, s in enumerate(slots.tolist()):
            tile = rows[16 * i:16 * i + 16].tolist()
            real = [r for r in tile if r >= 0]
            assert real and tile == real + [-1] * (16 - len(real))              # padding at the end only
            assert all(row_slots[r] == s for r in real) and real == sorted(real)
            seen += real
        assert sorted(seen) == [i for i, s in enumerate(row_slots) if s >= 0] and len(seen) == len(set(seen))
        assert slots.tolist() == sorted(slots.tolist())
        per_slot = {s: sum(1 for x in row_slots if x == s) for s in set(row_slots) - {-1}}
        assert slots.size == sum(-(-n // 16) for n in per_slot.values())
        return rows, slots
    check([(0, 1, 3)[i % 3] for i in range(t)])                     # interleaved row by row
    check([0] * (t // 2) + [3] * (t - t // 2))                      # runs
    check([-1 if i % 3 == 0 else 1 for i in range(t)])              # rows without an adapter
    rows, slots = check([2] * t)
    assert slots.tolist() == [2] * (-(-t // 16))
    rows, slots = build_tiles([-1] * t, 4)
    assert rows.size == 0 and slots.size == 0


def test_rows_of_a_step_take_their_sequences_slot():
    # two prompts (3 and 2 tokens) and two decoding sequences
    assert rows_of_sequences([1, -1, 0, -1], [3, 2]) == [1, 1, 1, -1, -1, 0, -1]
    assert rows_of_sequences([2, 2], []) == [2, 2]


# ---- engine, scheduler, HTTP ------------------------------------------------------------------------------------------------
class LoraFakeModel:
    """The engine's calls over a deterministic data plane: the token after t is t % 3 + 1 (so the prompt 1 2 3 1 2 3 ...
    continues itself and the prompt-lookup proposer finds drafts). Records every forward's keyword arguments."""
    num_blocks = 64
    max_draft_tokens = 3

    def __init__(self, loras=("a", "b")):
        self.model_config = types.SimpleNamespace()
        self._loras = {n: i for i, n in enumerate(loras)}
        self.calls, self.verify_calls, self.freed, self.lora_threads = [], [], [], []

    def forward(self, input_ids, seq_ids, decoding_lens, **kw):
        self.calls.append((list(seq_ids), kw))
        return [ids[-1] % 3 + 1 for ids in input_ids]

    def forward_verify(self, input_ids, seq_ids, ctx_lens):
        self.verify_calls.append(list(seq_ids))
        return [[t % 3 + 1 for t in ids] for ids in input_ids]

    def loras(self):
        return dict(self._loras)

    def load_lora(self, name, path=None, **kw):
        self.lora_threads.append(threading.current_thread().name)
        self._loras[name] = len(self._loras)
        return self._loras[name]

    def unload_lora(self, name):
        self.lora_threads.append(threading.current_thread().name)
        return self._loras.pop(name)

    def swap_in_seqs(self, ids):
        pass

    def swap_out_seqs(self, ids):
        pass

    def free_seqs_resources(self, ids):
        self.freed.extend(ids)


PATTERN = [1, 2, 3] * 4


def _serve(model, raws, **cfg):
    async def run():
        eng = Engine(_cfg(**cfg), model=model, piggyback=True)
        await eng.initialize()
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        done = await asyncio.wait_for(asyncio.gather(*(eng.add_request_and_wait(r) for r in raws)), timeout=20)
        loops.cancel()
        return eng, done
    return asyncio.run(run())


def test_plain_batches_keep_the_three_argument_call_and_mixed_batches_pass_an_aligned_list():
    model = LoraFakeModel()
    _serve(model, [RawRequest("", 4, [5, 6]), RawRequest("", 3, [7])])
    assert model.calls and all(kw == {} for _, kw in model.calls)
    model = LoraFakeModel()
    eng, done = _serve(model, [RawRequest("", 5, [5, 6], lora="a"), RawRequest("", 5, [7]), RawRequest("", 5, [8, 9], lora="b")])
    ids = {req.lora: req.request_id for req, _ in done}
    assert all(req.error is None and len(toks) == 5 for req, toks in done)
    mixed = 0
    for seq_ids, kw in model.calls:
        want = [next(name for name, rid in ids.items() if rid == s) for s in seq_ids]
        if any(n is not None for n in want):
            assert kw.get("lora") == want                   # aligned with the batch
            mixed += len(set(want)) > 1
        else:
            assert "lora" not in kw
    assert mixed >= 1


def test_a_lora_request_is_never_speculated():
    plain = LoraFakeModel()
    _serve(plain, [RawRequest("", 8, list(PATTERN))], speculative_ngram=3)
    assert plain.verify_calls                               # (the proposer finds drafts in this prompt)
    model = LoraFakeModel()
    eng, done = _serve(model, [RawRequest("", 8, list(PATTERN), lora="a")], speculative_ngram=3)
    assert eng.speculative_k == 3 and model.verify_calls == []
    assert done[0][1] == [1, 2, 3, 1, 2, 3, 1, 2]
    assert all(kw.get("lora") == ["a"] for _, kw in model.calls) and len(model.calls) == 8
    # a batch that holds a LoRA request is a plain forward for everyone in it
    model = LoraFakeModel()
    eng, done = _serve(model, [RawRequest("", 8, list(PATTERN), lora="a"), RawRequest("", 8, list(PATTERN))],
                       speculative_ngram=3)
    lora_id = next(req.request_id for req, _ in done if req.lora == "a")
    assert all(lora_id not in seqs for seqs in model.verify_calls)
    assert sum(lora_id in seqs for seqs, _ in model.calls) == 8         # every one of its tokens came from a plain forward


def test_an_unknown_adapter_is_rejected_and_not_queued():
    s = Scheduler(None, _cfg(), num_gpu_blocks=10)
    named = Request(RawRequest("", 3, [1, 2], lora="a"))
    assert "not loaded" in s.why_unservable(named)          # (a data plane without adapters serves none)
    s.lora_names = lambda: {"a": 0}.keys()
    assert s.why_unservable(named) is None
    assert "'zz' is not loaded" in s.why_unservable(Request(RawRequest("", 3, [1, 2], lora="zz")))
    assert s.why_unservable(Request(RawRequest("", 3, [1, 2]))) is None
    model = LoraFakeModel()
    eng, done = _serve(model, [RawRequest("", 3, [1, 2], lora="zz"), RawRequest("", 3, [4], lora="b")])
    (bad, bad_toks), (good, good_toks) = done
    assert bad.error and "not loaded" in bad.error and bad_toks == []
    assert good.error is None and len(good_toks) == 3
    assert all(kw.get("lora") == ["b"] for _, kw in model.calls)


def test_unload_is_refused_while_in_use_and_allowed_afterwards():
    async def run():
        model = LoraFakeModel()
        eng = Engine(_cfg(), model=model)
        await eng.initialize()
        req = Request(RawRequest("", 3, [1, 2], lora="a"))
        eng.scheduler.on_requests_arrival([req])
        with pytest.raises(ValueError, match="in use"):
            eng.unload_lora("a")                            # waiting
        assert eng.unload_lora("b") == 1                    # nobody names b
        assert await eng.step()
        with pytest.raises(ValueError, match="in use"):
            eng.unload_lora("a")                            # running
        while await eng.step():
            pass
        assert req.is_finished() and model.freed == [req.request_id]
        assert eng.unload_lora("a") == 0 and model.loras() == {}
        assert "not loaded" in eng.scheduler.why_unservable(Request(RawRequest("", 3, [1, 2], lora="a")))
        assert eng.load_lora("c", "/somewhere") == 0
        assert eng.scheduler.why_unservable(Request(RawRequest("", 3, [1, 2], lora="c"))) is None
        # while the serving loop runs, both commands execute on the model thread
        del model.lora_threads[:]
        loops = asyncio.ensure_future(eng.start_all_event_loops())
        await asyncio.sleep(0.05)
        loop = asyncio.get_running_loop()
        assert await asyncio.wait_for(loop.run_in_executor(None, eng.load_lora, "d", "/x"), 10) == 1
        _, toks = await asyncio.wait_for(eng.add_request_and_wait(RawRequest("", 2, [3], lora="d")), 10)
        assert len(toks) == 2
        assert await asyncio.wait_for(loop.run_in_executor(None, eng.unload_lora, "d"), 10) == 1
        loops.cancel()
        await asyncio.gather(loops, return_exceptions=True)
        return model
    model = asyncio.run(run())
    assert model.lora_threads == ["swiftllm-model", "swiftllm-model"]


def test_an_adapter_unloaded_between_the_check_and_the_arrival_is_answered_not_forwarded():
    """The name is checked on the event loop when the request arrives and AGAIN on the model thread when the arrival is
    moved into the scheduler: a request that passed the first check while an unload was running gets an error there."""
    async def run():
        model = LoraFakeModel()
        eng = Engine(_cfg(), model=model)
        await eng.initialize()
        late = Request(RawRequest("", 3, [1, 2], lora="a"))
        keep = Request(RawRequest("", 3, [4], lora="b"))
        assert eng.scheduler.why_unservable(late) is None          # passed the check ...
        eng._live.update([late, keep])
        model.unload_lora("a")                                      # ... the adapter goes ...
        eng._inbox.put([late, keep])                                # ... and only then the arrival is queued
        while await eng.step():
            pass
        await asyncio.sleep(0)
        assert late.error and "not loaded" in late.error and late.finished_event.is_set() and late.output_token_ids == []
        assert late not in eng._live and await late.output_q.get() is None
        assert keep.error is None and len(keep.output_token_ids) == 3
        assert all(kw.get("lora") == ["b"] for _, kw in model.calls) and model.calls
    asyncio.run(run())


def test_generate_validates_the_lora_field_and_answers_as_before_without_it():
    from fastapi.testclient import TestClient
    from swiftllm_amd.server.api_server import build_app
    model = LoraFakeModel()

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
    with TestClient(app) as client:
        r = client.post("/generate", json={"prompt_token_ids": [4, 5], "output_len": 3})
        assert r.status_code == 200 and r.json() == {"output_token_ids": [3, 1, 2]}        # exactly today's JSON
        r = client.post("/generate", json={"prompt_token_ids": [4, 5], "output_len": 3, "lora": "a"})
        assert r.status_code == 200 and r.json() == {"output_token_ids": [3, 1, 2]}
        assert model.calls[-1][1] == {"lora": ["a"]}
        for bad in ("", 7, None, ["a"], {"name": "a"}, True):
            r = client.post("/generate", json={"prompt_token_ids": [4, 5], "output_len": 3, "lora": bad})
            assert r.status_code == 400 and "lora" in r.json()["error"], bad
        r = client.post("/generate", json={"prompt_token_ids": [4, 5], "output_len": 3, "lora": "zz"})
        assert r.status_code == 400 and "not loaded" in r.json()["error"]


def test_the_router_forwards_the_lora_field_unchanged():
    import socket
    import time
    import fastapi
    import uvicorn
    from fastapi.responses import JSONResponse
    from fastapi.testclient import TestClient
    from swiftllm_amd.server.router import ReplicaRouter, build_app
    seen = []
    replica = fastapi.FastAPI()

    @replica.post("/generate")
    async def generate(req: fastapi.Request):
        seen.append(await req.json())
        return JSONResponse({"output_token_ids": [1]})
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    server = uvicorn.Server(uvicorn.Config(replica, host="127.0.0.1", port=port, log_level="error"))
    threading.Thread(target=server.run, daemon=True).start()
    deadline = time.time() + 10
    while not server.started:
        assert time.time() < deadline, "the fake replica did not start"
        time.sleep(0.02)
    try:
        with TestClient(build_app(ReplicaRouter([f"http://127.0.0.1:{port}"]))) as client:
            body = {"prompt_token_ids": [1, 2, 3], "output_len": 1, "lora": "tenant-7"}
            assert client.post("/generate", json=body).json() == {"output_token_ids": [1]}
            plain = {"prompt_token_ids": [1, 2, 3], "output_len": 1}
            client.post("/generate", json=plain)
        assert seen == [body, plain]
    finally:
        server.should_exit = True
