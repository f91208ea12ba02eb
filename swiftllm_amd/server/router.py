"""Request-sharded data parallelism for serving: N independent replicas on the N GPUs of one node.

    python -m swiftllm_amd.server.router --num-replicas 8 --model-path DIR [--port 8000] [engine flags]

Each replica is an `api_server` process pinned to one GPU (HIP_VISIBLE_DEVICES=i, so it sees its GPU as
device 0 like a single-GPU run) with its own weights, KV pool and scheduler. This process only routes:
a request goes to the replica with the fewest outstanding tokens and stays there for its whole life —
no KV migration, no collective, nothing on xGMI (the reference has no multi-GPU mode).
"""
import argparse
import asyncio
import os
import subprocess
import sys
from typing import List

from swiftllm_amd import dp


class ReplicaRouter:
    """Least-outstanding-tokens routing over a fixed set of replica URLs (pure bookkeeping)."""

    def __init__(self, urls: List[str]):
        self.urls = list(urls)
        self.outstanding = [0] * len(urls)

    def acquire(self, cost: int) -> int:
        i = dp.least_loaded(self.outstanding)
        self.outstanding[i] += cost
        return i

    def release(self, i: int, cost: int):
        self.outstanding[i] -= cost


def request_cost(body: dict) -> int:
    ids = body.get("prompt_token_ids")
    return int(body.get("output_len", 0)) + (len(ids) if ids else len(str(body.get("prompt", "")).split()))


def build_app(router: ReplicaRouter):
    import aiohttp
    import fastapi
    from fastapi.responses import JSONResponse, StreamingResponse
    app = fastapi.FastAPI()
    no_limit = aiohttp.ClientTimeout(total=None)    # a queued long generation may take longer than aiohttp's 300 s

    @app.post("/generate")
    async def generate(req: fastapi.Request):
        body = await req.json()
        cost = request_cost(body)
        i = router.acquire(cost)
        url = router.urls[i] + "/generate"
        if body.get("stream", False):
            async def relay():
                try:
                    async with aiohttp.ClientSession(timeout=no_limit) as s, s.post(url, json=body) as r:
                        async for chunk in r.content.iter_any():
                            yield chunk
                finally:
                    router.release(i, cost)
            return StreamingResponse(relay(), media_type="text/plain")
        try:
            async with aiohttp.ClientSession(timeout=no_limit) as s, s.post(url, json=body) as r:
                return JSONResponse(await r.json(), status_code=r.status)
        finally:
            router.release(i, cost)

    @app.get("/load")
    async def load():
        return JSONResponse({"outstanding_tokens": router.outstanding})

    return app


def spawn_replicas(num: int, base_port: int, passthrough: List[str]) -> List[subprocess.Popen]:
    procs = []
    for i in range(num):
        env = dict(os.environ, HIP_VISIBLE_DEVICES=str(i), HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "swiftllm_amd.server.api_server", "--port", str(base_port + 1 + i)] + passthrough
        cpus = dp.cpus_for_local_rank(i, num)      # NUMA-local cores of GPU i, disjoint from the other replicas'

        def pin(cpus=cpus):
            try:
                os.sched_setaffinity(0, cpus)
            except OSError:
                pass
        procs.append(subprocess.Popen(cmd, env=env, preexec_fn=pin))
    return procs


def lora_passthrough(max_loras, max_lora_rank, loras) -> List[str]:
    """The replicas' flags for the router's LoRA options; refuses what every replica would refuse, before any is spawned."""
    if loras and not max_loras:
        raise SystemExit("--lora needs --max-loras > 0")
    for spec in loras or ():
        name, sep, path = spec.partition("=")
        if not sep or not name or not path:
            raise SystemExit(f"--lora takes NAME=PATH, got {spec!r}")
    out: List[str] = []
    if max_loras is not None:
        out += ["--max-loras", str(max_loras)]
    if max_lora_rank is not None:
        out += ["--max-lora-rank", str(max_lora_rank)]
    for spec in loras or ():
        out += ["--lora", spec]
    return out


async def wait_until_ready(urls: List[str], timeout_s: float = 1800.0, procs=None) -> None:
    """Poll every replica's GET /load until it answers (weights loaded, KV pool profiled). `procs` (the replicas'
    subprocess.Popen objects, same order as `urls`): a replica whose process has exited fails the wait at once
    instead of being polled until the timeout."""
    import aiohttp
    deadline = asyncio.get_event_loop().time() + timeout_s
    async with aiohttp.ClientSession(timeout=aiohttp.ClientTimeout(total=5)) as s:
        for i, url in enumerate(urls):
            while True:
                if procs is not None and procs[i].poll() is not None:
                    raise RuntimeError(f"replica {url} exited with code {procs[i].returncode} before it came up")
                try:
                    async with s.get(url + "/load") as r:
                        if r.status == 200:
                            break
                except (aiohttp.ClientError, asyncio.TimeoutError):
                    pass
                if asyncio.get_event_loop().time() > deadline:
                    raise RuntimeError(f"replica {url} did not come up within {timeout_s:.0f} s")
                await asyncio.sleep(0.5)


def main():
    ap = argparse.ArgumentParser(description="swiftllm_amd replica router (request-sharded DP)")
    ap.add_argument("--num-replicas", type=int, default=8)
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    # checked here, before eight replicas load their weights, and handed on to every one of them
    ap.add_argument("--kv-cache-dtype", default=None, choices=["auto", "fp8_e4m3"],
                    help="element type of every replica's KV pools (api_server --kv-cache-dtype)")
    # multi-LoRA serving: every replica loads the same adapters (a request's "lora" field is relayed like every field)
    ap.add_argument("--max-loras", type=int, default=None, help="adapter slots of every replica (api_server --max-loras)")
    ap.add_argument("--max-lora-rank", type=int, default=None, choices=[8, 16, 32, 64])
    ap.add_argument("--lora", action="append", default=None, metavar="NAME=PATH",
                    help="a PEFT adapter directory every replica loads at start-up (repeatable)")
    # guided decoding: every replica keeps a mask pool of this many rows (a request's "guided_regex", "guided_choice" and
    # "allowed_token_ids" fields are relayed like every field)
    ap.add_argument("--guided-max-states", type=int, default=None,
                    help="rows of every replica's guide mask pool (api_server --guided-max-states; 0 = off)")
    args, passthrough = ap.parse_known_args()
    if args.guided_max_states is not None:
        if args.guided_max_states < 0:
            raise SystemExit("--guided-max-states must be >= 0")
        passthrough = list(passthrough) + ["--guided-max-states", str(args.guided_max_states)]
    if args.kv_cache_dtype is not None:
        passthrough = list(passthrough) + ["--kv-cache-dtype", args.kv_cache_dtype]
    passthrough = list(passthrough) + lora_passthrough(args.max_loras, args.max_lora_rank, args.lora)
    procs = spawn_replicas(args.num_replicas, args.port, passthrough)
    router = ReplicaRouter([f"http://127.0.0.1:{args.port + 1 + i}" for i in range(args.num_replicas)])
    try:
        import uvicorn
        asyncio.run(wait_until_ready(router.urls, procs=procs))      # accept traffic only when every replica can serve it
        uvicorn.run(build_app(router), host=args.host, port=args.port, log_level="warning")
    finally:
        for p in procs:
            p.terminate()


if __name__ == "__main__":
    main()
