"""Offline generation straight on the data plane (no engine, no scheduler) — the flow of the reference's
examples/offline.py against this implementation: build the model, size the KV pool from free HBM,
prefill a few prompts in one batch, then decode greedily step by step.

    python examples/offline.py --model-path /path/to/llama [--dtype bfloat16] [--steps 20] [--speculative-ngram 3]
                               [--logprobs 3] [--guided-regex '[0-9]{4}-[0-9]{2}-[0-9]{2}']

With a HuggingFace tokenizer in the model directory the prompts are text; otherwise (e.g. the random-init
checkpoints written by oracle/synth.py) random token ids are used and ids are printed.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import swiftllm  # noqa: E402

PROMPTS = ["Life blooms like a flower, far away", "one two three four five",
           "A B C D E F G H I J K L M N O P Q R S T U V", "To be or not to be,"]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--model-path", required=True)
    ap.add_argument("--dtype", default="float16", choices=["float16", "bfloat16"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--use-dummy", action="store_true")
    ap.add_argument("--kv-cache-dtype", default="auto", choices=["auto", "fp8_e4m3"])
    ap.add_argument("--speculative-ngram", type=int, default=0,
                    help="prompt-lookup speculative decoding: n-gram drafts per sequence per step (0 = off)")
    ap.add_argument("--max-loras", type=int, default=0, help="multi-LoRA serving: adapter slots (0 = off)")
    ap.add_argument("--max-lora-rank", type=int, default=16, choices=[8, 16, 32, 64])
    ap.add_argument("--lora", action="append", default=None, metavar="NAME=PATH",
                    help="a PEFT adapter directory (repeatable): prompt i runs with adapter i, the prompts beyond the "
                         "adapters with the base model")
    ap.add_argument("--logprobs", type=int, default=None, metavar="N",
                    help="report every generated token's log-probability, rank and N most likely alternatives (0..20)")
    ap.add_argument("--guided-regex", default=None, metavar="PATTERN",
                    help="guided decoding: the bytes every prompt's output spells fullmatch this pattern (the byte-level "
                         "subset of swiftllm_amd/guided/regex.py; needs tokenizer.json in --model-path); a sequence is "
                         "printed up to the token that completes the pattern")
    args = ap.parse_args()

    cfg = swiftllm.EngineConfig(model_path=args.model_path, use_dummy=args.use_dummy, block_size=16,
                                gpu_mem_utilization=0.9, num_cpu_blocks=0, max_seqs_in_block_table=128,
                                max_blocks_per_seq=2048, max_batch_size=16, max_tokens_in_batch=2048 * 16,
                                dtype=args.dtype, use_hip_graph=True, kv_cache_dtype=args.kv_cache_dtype,
                                speculative_ngram=args.speculative_ngram, max_loras=args.max_loras,
                                max_lora_rank=args.max_lora_rank, lora_modules=args.lora,
                                guided_max_states=1024 if args.guided_regex is not None else 0)
    t0 = time.perf_counter()
    model = swiftllm.LlamaModel(cfg)
    model.load_weights()
    num_blocks = model.profile_num_blocks()
    model.init_kvcache_and_swap(min(num_blocks, 4096))
    print(f"model ready in {time.perf_counter() - t0:.2f} s; {num_blocks} KV blocks fit, using {model.num_blocks}")

    tokenizer = None
    if any(n.startswith("tokenizer") for n in os.listdir(args.model_path)):
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(args.model_path)
        input_ids = tokenizer(PROMPTS)["input_ids"]
    else:
        import random
        rng = random.Random(0)
        vocab = model.model_config.vocab_size
        input_ids = [[rng.randrange(vocab) for _ in range(n)] for n in (9, 5, 22, 6)]

    seq_ids = list(range(len(input_ids)))
    if args.speculative_ngram > 0:
        return generate_speculative(model, input_ids, seq_ids, args, tokenizer)
    # one adapter per prompt, in the order of --lora; None (the base model) for the rest; no --lora: the call of always
    names = list(model.loras())
    kw = {"lora": [names[i] if i < len(names) else None for i in seq_ids]} if names else {}
    if args.logprobs is not None:       # (no --logprobs: the call of always; last_logprobs is None then)
        kw["sampling_params"] = [swiftllm.SamplingParams(logprobs=args.logprobs)] * len(seq_ids)
    # --guided-regex: one cursor per sequence through one shared guide; the caller advances them with the returned tokens
    # (no --guided-regex: the call of always). A sequence whose pattern is complete rides on unguided and is cut below.
    cursors, done_at = None, {}
    if args.guided_regex is not None:
        from swiftllm_amd.guided import GuideCursor, guide_key
        key = guide_key("regex", args.guided_regex)
        cursors = [GuideCursor(model.guide_store.acquire(key)) for _ in seq_ids]

    def step(ids, lens):
        if cursors is None:
            return model.forward(ids, seq_ids, lens, **kw)
        guides = [None if i in done_at else c for i, c in enumerate(cursors)]
        toks = model.forward(ids, seq_ids, lens, guides=guides, **kw)
        for i, (c, t) in enumerate(zip(guides, toks)):
            if c is not None:
                c.advance(t)
                if c.complete:
                    done_at[i] = len(outputs) + 1
        return toks
    outputs = []
    outputs.append(step(input_ids, []))
    scores = [model.last_logprobs]
    lens = [len(x) for x in input_ids]
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lens = [n + 1 for n in lens]
        outputs.append(step([[t] for t in outputs[-1]], lens))
        scores.append(model.last_logprobs)
    dt = time.perf_counter() - t0
    print(f"{args.steps} decode steps x {len(seq_ids)} sequences: {dt / args.steps * 1e3:.2f} ms/step")
    for i in seq_ids:
        toks = [out[i] for out in outputs][:done_at.get(i)]
        print(f"[{i}]", tokenizer.decode(toks, skip_special_tokens=True) if tokenizer else toks)
        if args.logprobs is not None:
            for scored in scores[:done_at.get(i)]:
                lp = scored[i]
                top = ", ".join(f"{t}: {v:.3f}" for t, v in lp.top)
                print(f"      {lp.token_id}: {lp.logprob:.3f} (rank {lp.rank})" + (f"  top: {top}" if top else ""))
    for c in cursors or ():
        model.guide_store.release(c.guide)
    model.free_seqs_resources(seq_ids)


def generate_speculative(model, input_ids, seq_ids, args, tokenizer):
    """The same greedy streams with prompt-lookup drafts: a step feeds every sequence's last token and up to k tokens that
    followed the most recent earlier occurrence of its last n-gram, and keeps what the model confirms (+ one token)."""
    from swiftllm_amd.server.speculative import NgramProposer, accept
    k = min(args.speculative_ngram, model.max_draft_tokens)
    want = args.steps + 1
    outs = [[t] for t in model.forward(input_ids, seq_ids, [])]
    props = [NgramProposer(p) for p in input_ids]
    forwards = proposed = accepted = 0
    t0 = time.perf_counter()
    while any(len(o) < want for o in outs):
        live = [i for i in seq_ids if len(outs[i]) < want]
        drafts = []
        for i in live:
            props[i].sync(input_ids[i], outs[i])
            drafts.append(props[i].propose(min(k, want - len(outs[i]) - 1)))
        ctx = [len(input_ids[i]) + len(outs[i]) - 1 for i in live]
        if any(drafts):
            targets = model.forward_verify([[outs[i][-1]] + d for i, d in zip(live, drafts)], live, ctx)
        else:
            targets = [[t] for t in model.forward([[outs[i][-1]] for i in live], live, [c + 1 for c in ctx])]
        forwards += 1
        for i, d, tgt in zip(live, drafts, targets):
            a = accept(d, tgt)
            proposed, accepted = proposed + len(d), accepted + a
            outs[i].extend(tgt[:a + 1])
    dt = time.perf_counter() - t0
    print(f"{args.steps} tokens x {len(seq_ids)} sequences in {forwards} forwards ({dt / forwards * 1e3:.2f} ms each); "
          f"drafts accepted {accepted} / {proposed} (k = {k})")
    for i in seq_ids:
        print(f"[{i}]", tokenizer.decode(outs[i], skip_special_tokens=True) if tokenizer else outs[i])
    model.free_seqs_resources(seq_ids)


if __name__ == "__main__":
    main()
