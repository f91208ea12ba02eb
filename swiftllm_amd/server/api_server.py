"""HTTP front-end of one engine replica.

    python -m swiftllm_amd.server.api_server --model-path DIR [--port 8000] [engine flags]

`POST /generate` with JSON {prompt | prompt_token_ids, output_len, stream?, decode?} — the request
format of the reference's swiftllm/server/api_server.py:16-84, plus optional sampling fields (temperature,
top_k, top_p, seed; repetition_penalty, presence_penalty, frequency_penalty, min_p, logit_bias = {"id": bias},
stop_token_ids, min_tokens; absent = greedy to output_len, as in the reference) and "lora": the name of a loaded LoRA
adapter (--max-loras / --lora NAME=PATH; absent = the base model): non-streaming answers
{"output_token_ids": [...]} (or {"output": text} with decode), streaming sends one line per token.
"guided_regex": pattern, "guided_choice": [strings] or "allowed_token_ids": [ids] (at most one; --guided-max-states > 0)
hold the output to a shape: its bytes fullmatch the pattern (the byte-level subset of swiftllm_amd/guided/regex.py), are one
of the choices, or every token is one of the ids; "stop_token_ids" are the guide's end ids. A pattern outside the subset is
answered with 400, a guide store whose rows are all held by live requests with 503; a request whose guide reaches a state
in which no token is allowed ends with {"error": ...} (400) as well.
"logprobs": N (0..20) asks for every generated token's log-probability, rank and N most likely alternatives: the
non-streaming answer gains "logprobs": [{"token_id", "logprob", "rank", "top": [[id, logprob], ...]}, ...] and a stream
sends one such JSON object per line (with "text" under decode); values that are not finite are sent as null.
`GET /load` reports outstanding tokens (used by the replica router). Any engine failure takes the
process down (reference api_server.py:114-119) so a supervisor can restart the replica.
"""
import argparse
import asyncio
import json
import math
import os
import traceback

import fastapi
import uvicorn
from fastapi.responses import JSONResponse, StreamingResponse

from swiftllm_amd.engine_config import EngineConfig
from swiftllm_amd.sampling_params import MAX_LOGPROBS, SamplingParams
from .engine import Engine
from .structs import RawRequest


def _validate_body(body) -> "str | None":
    """Shape checks the engine must never have to survive (it dies on any exception, taking every in-flight
    request with it): types only — ranges (vocabulary, rotary positions, pool size) are the scheduler's
    `why_unservable`, answered with the same 400."""
    if not isinstance(body, dict):
        return "body must be a JSON object"
    n = body.get("output_len")
    if not isinstance(n, int) or isinstance(n, bool):
        return "output_len must be an integer"
    ids = body.get("prompt_token_ids")
    if ids is not None:
        if not isinstance(ids, list) or not all(isinstance(t, int) and not isinstance(t, bool) for t in ids):
            return "prompt_token_ids must be a list of integers"
        if len(ids) == 0:
            return "prompt_token_ids must not be empty"
        if any(t < 0 or t >= 2 ** 31 for t in ids):
            return "prompt_token_ids out of range"
    if not isinstance(body.get("prompt", ""), str):    # also when token ids are given: the handler still touches it
        return "prompt must be a string"
    if "lora" in body and (not isinstance(body["lora"], str) or not body["lora"]):
        return "lora must be a non-empty string (the name of a loaded adapter)"
    return _validate_sampling(body)


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _is_finite_number(v) -> bool:
    """An int or a float that is finite AS A FLOAT (a JSON integer of hundreds of digits is not: float() overflows)."""
    if not (_is_int(v) or isinstance(v, float)):
        return False
    try:
        return math.isfinite(v)
    except OverflowError:
        return False


def _validate_sampling(body) -> "str | None":
    t = body.get("temperature")
    if t is not None and (not _is_finite_number(t) or t < 0):
        return "temperature must be a finite number >= 0"
    k = body.get("top_k")
    if k is not None and (not _is_int(k) or k < 0 or k >= 2 ** 31):
        return "top_k must be an integer >= 0"
    p = body.get("top_p")
    if p is not None and (not _is_finite_number(p) or not 0 < p <= 1):
        return "top_p must be a number in (0, 1]"
    s = body.get("seed")
    if s is not None and (not _is_int(s) or not 0 <= s < 2 ** 64):
        return "seed must be an integer in [0, 2**64)"

    number = _is_finite_number
    r = body.get("repetition_penalty")
    if r is not None and (not number(r) or r <= 0):
        return "repetition_penalty must be a finite number > 0"
    for name in ("presence_penalty", "frequency_penalty"):
        v = body.get(name)
        if v is not None and not number(v):
            return f"{name} must be a finite number"
    m = body.get("min_p")
    if m is not None and (not number(m) or not 0 <= m < 1):
        return "min_p must be a number in [0, 1)"
    bias = body.get("logit_bias")
    if bias is not None:
        if not isinstance(bias, dict):
            return "logit_bias must be an object of token id -> bias"
        for key, v in bias.items():
            # (the length first: int() refuses strings of thousands of digits with a ValueError of its own)
            if not (isinstance(key, str) and 0 < len(key) <= 10 and key.isascii() and key.isdigit() and int(key) < 2 ** 31):
                return "logit_bias keys must be decimal token ids"
            if not number(v):
                return "logit_bias values must be finite numbers"
        if len({int(key) for key in bias}) != len(bias):
            return "logit_bias names a token id twice"
    stops = body.get("stop_token_ids")
    if stops is not None and (not isinstance(stops, list) or not all(_is_int(t) and 0 <= t < 2 ** 31 for t in stops)):
        return "stop_token_ids must be a list of integers >= 0"
    n = body.get("min_tokens")
    if n is not None and (not _is_int(n) or n < 0):
        return "min_tokens must be an integer >= 0"
    lp = body.get("logprobs")
    if lp is not None and (not _is_int(lp) or not 0 <= lp <= MAX_LOGPROBS):
        return f"logprobs must be an integer in [0, {MAX_LOGPROBS}]"
    if sum(body.get(f) is not None for f in _GUIDED_FIELDS) > 1:
        return "at most one of guided_regex, guided_choice and allowed_token_ids may be set"
    g = body.get("guided_regex")
    if g is not None and not isinstance(g, str):
        return "guided_regex must be a string"
    g = body.get("guided_choice")
    if g is not None and (not isinstance(g, list) or not g or not all(isinstance(c, str) and c for c in g)
                          or len(set(g)) != len(g)):
        return "guided_choice must be a non-empty list of distinct non-empty strings"
    g = body.get("allowed_token_ids")
    if g is not None and (not isinstance(g, list) or not g or not all(_is_int(t) and 0 <= t < 2 ** 31 for t in g)):
        return "allowed_token_ids must be a non-empty list of integers >= 0"
    if any(body.get(f) is not None for f in _GUIDED_FIELDS) and (n or 0) > 0:
        return "min_tokens cannot be combined with guided_regex, guided_choice or allowed_token_ids"
    return None


_SAMPLING_FIELDS = ("temperature", "top_k", "top_p", "seed")
_GUIDED_FIELDS = ("guided_regex", "guided_choice", "allowed_token_ids")
_PROCESSING_FIELDS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "min_p", "logit_bias",
                      "stop_token_ids", "min_tokens")


def _sampling_params(body) -> "SamplingParams | None":
    if all(body.get(f) is None for f in _SAMPLING_FIELDS + _PROCESSING_FIELDS + ("logprobs",) + _GUIDED_FIELDS):
        return None
    kw = {}
    if any(body.get(f) is not None for f in _GUIDED_FIELDS):            # (none of them: the params of always)
        choice, allowed = body.get("guided_choice"), body.get("allowed_token_ids")
        kw = dict(guided_regex=body.get("guided_regex"), guided_choice=tuple(choice) if choice is not None else None,
                  allowed_token_ids=tuple(allowed) if allowed is not None else None,
                  stop_token_ids=tuple(body.get("stop_token_ids") or ()))
    if any(body.get(f) is not None for f in _PROCESSING_FIELDS):       # (none of them: the params of always)
        def num(name, default):
            return float(body[name]) if body.get(name) is not None else default
        bias = body.get("logit_bias")
        kw.update(repetition_penalty=num("repetition_penalty", 1.0), presence_penalty=num("presence_penalty", 0.0),
                  frequency_penalty=num("frequency_penalty", 0.0), min_p=num("min_p", 0.0),
                  logit_bias={int(k): float(v) for k, v in bias.items()} if bias else None,
                  stop_token_ids=tuple(body.get("stop_token_ids") or ()), min_tokens=int(body.get("min_tokens") or 0))
    return SamplingParams(temperature=float(body.get("temperature") or 0.0), top_k=int(body.get("top_k") or 0),
                          top_p=float(body.get("top_p") if body.get("top_p") is not None else 1.0),
                          seed=body.get("seed"), logprobs=body.get("logprobs"), **kw)


def _finite_or_none(v: float) -> "float | None":
    """JSON has no NaN / Infinity (JSONResponse refuses them): such a value is sent as null."""
    return v if math.isfinite(v) else None


def _logprob_json(lp) -> dict:
    """A TokenLogprob as the object both answer forms carry."""
    return {"token_id": lp.token_id, "logprob": _finite_or_none(lp.logprob), "rank": lp.rank,
            "top": [[i, _finite_or_none(v)] for i, v in lp.top]}


def build_app(engine: Engine) -> fastapi.FastAPI:
    app = fastapi.FastAPI()
    state = {"outstanding_tokens": 0}

    @app.post("/generate")
    async def generate(req: fastapi.Request):
        try:
            body = await req.json()
        except Exception:     # noqa: BLE001 — malformed JSON is the client's problem, not the engine's
            return JSONResponse({"error": "body must be a JSON object"}, status_code=400)
        problem = _validate_body(body)
        if problem is not None:
            return JSONResponse({"error": problem}, status_code=400)
        raw = RawRequest(body.get("prompt", ""), body["output_len"], body.get("prompt_token_ids"),
                         sampling_params=_sampling_params(body), lora=body.get("lora"))
        want_text = bool(body.get("decode", False))
        want_logprobs = body.get("logprobs") is not None
        cost = raw.output_len + len(raw.prompt_token_ids or raw.prompt.split())
        state["outstanding_tokens"] += cost
        if body.get("stream", False):
            async def lines():
                try:
                    async for step in engine.add_request_and_stream(raw):
                        if want_logprobs and step.logprobs is not None:
                            obj = _logprob_json(step.logprobs)
                            if want_text:
                                obj["text"] = await engine.tokenization_engine.decode([step.token_id])
                            yield json.dumps(obj, allow_nan=False) + "\n"
                        elif want_text:
                            yield await engine.tokenization_engine.decode([step.token_id]) + "\n"
                        else:
                            yield f"{step.token_id}\n"
                finally:
                    state["outstanding_tokens"] -= cost
            return StreamingResponse(lines(), media_type="text/plain")
        try:
            request, token_ids = await engine.add_request_and_wait(raw)
        finally:
            state["outstanding_tokens"] -= cost
        if request.error is not None:
            # a request the engine can never serve is the client's error (400); an engine whose model thread is gone is
            # the server's (503: a router in front retries on another replica)
            dead = getattr(engine, "_dead", None) is not None and request.error == engine._dead
            retry = dead or getattr(request, "error_retryable", False)      # (a full guide store passes: try again later)
            return JSONResponse({"error": request.error}, status_code=503 if retry else 400)
        answer = ({"output": await engine.tokenization_engine.decode(token_ids)} if want_text else
                  {"output_token_ids": token_ids})
        if want_logprobs:
            answer["logprobs"] = [_logprob_json(lp) for lp in request.output_logprobs if lp is not None]
        return JSONResponse(answer)

    @app.get("/load")
    async def load():
        return JSONResponse(state)

    return app


async def _serve(args):
    fields = {f for f in EngineConfig.__dataclass_fields__}
    engine = Engine(EngineConfig(**{k: v for k, v in vars(args).items() if k in fields}),
                    piggyback=args.piggyback)
    await engine.initialize()
    server = uvicorn.Server(uvicorn.Config(build_app(engine), host=args.host, port=args.port, log_level="warning"))

    async def guarded_loops():
        try:
            await engine.start_all_event_loops()
        except Exception:     # noqa: BLE001 — a dead engine must not leave a zombie HTTP server behind
            traceback.print_exc()
            os._exit(1)
    await asyncio.gather(server.serve(), guarded_loops())


def main():
    ap = argparse.ArgumentParser(description="swiftllm_amd API server (one replica)")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=8000)
    ap.add_argument("--piggyback", action="store_true", help="let decodes ride along with prefill batches")
    EngineConfig.add_cli_args(ap)
    asyncio.run(_serve(ap.parse_args()))


if __name__ == "__main__":
    main()
