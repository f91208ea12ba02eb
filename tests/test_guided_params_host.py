"""SamplingParams: the three guided-decoding fields, their validation and what they do to `plain` / `processes_logits`."""
import dataclasses

import pytest

from swiftllm_amd import SamplingParams
from swiftllm_amd.server.structs import RawRequest, Request


def test_default_params_are_what_they_were():
    sp = SamplingParams()
    assert (sp.guided_regex, sp.guided_choice, sp.allowed_token_ids) == (None, None, None)
    assert not sp.guided and sp.plain and sp.greedy and not sp.processes_logits and sp.guide_spec() is None
    # the fields of before, with their defaults, in their order, and the three new ones behind them
    names = [f.name for f in dataclasses.fields(SamplingParams)]
    assert names == ["temperature", "top_k", "top_p", "seed", "repetition_penalty", "presence_penalty", "frequency_penalty",
                     "min_p", "logit_bias", "stop_token_ids", "min_tokens", "logprobs", "guided_regex", "guided_choice",
                     "allowed_token_ids"]
    assert dataclasses.astuple(sp)[:12] == (0.0, 0, 1.0, None, 1.0, 0.0, 0.0, 0.0, None, (), 0, None)
    assert Request(RawRequest("", 4, [1, 2], sampling_params=sp)).sampling_params is None      # plain: what None means


def test_each_field_alone_makes_a_guided_request():
    a = SamplingParams(guided_regex="[0-9]+")
    b = SamplingParams(guided_choice=["yes", "no"])
    c = SamplingParams(allowed_token_ids=[7, 3, 7, 5])
    assert a.guide_spec() == ("regex", "[0-9]+")
    assert b.guided_choice == ("yes", "no") and b.guide_spec() == ("choice", ("yes", "no"))
    assert c.allowed_token_ids == (3, 5, 7) and c.guide_spec() == ("tokens", (3, 5, 7))        # sorted, unique
    for sp in (a, b, c):
        assert sp.guided and not sp.plain
        assert not sp.processes_logits                   # unchanged: a guided request needs no token history
        req = Request(RawRequest("", 4, [1, 2], sampling_params=sp))
        assert req.sampling_params is sp and req.guide_cursor is None
    assert SamplingParams(guided_regex="a", temperature=0.7, seed=3, logprobs=2, min_p=0.1, stop_token_ids=(2,)).guided
    assert SamplingParams(guided_regex="a", min_p=0.1, temperature=1.0).processes_logits


def test_the_three_fields_are_mutually_exclusive():
    for kw in (dict(guided_regex="a", guided_choice=["a"]), dict(guided_regex="a", allowed_token_ids=[1]),
               dict(guided_choice=["a"], allowed_token_ids=[1]),
               dict(guided_regex="a", guided_choice=["a"], allowed_token_ids=[1])):
        with pytest.raises(ValueError, match="at most one"):
            SamplingParams(**kw)


@pytest.mark.parametrize("kw", [dict(guided_regex=5), dict(guided_regex=b"a"), dict(guided_choice="yes"),
                                dict(guided_choice=[]), dict(guided_choice=["a", ""]), dict(guided_choice=["a", "a"]),
                                dict(guided_choice=["a", 3]), dict(guided_choice=7), dict(allowed_token_ids=[]),
                                dict(allowed_token_ids=[-1]), dict(allowed_token_ids=[1.5]), dict(allowed_token_ids=[True]),
                                dict(allowed_token_ids=[2 ** 31]), dict(allowed_token_ids="12"), dict(allowed_token_ids=3)])
def test_bad_values_are_refused(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw)


def test_min_tokens_with_a_guide_is_refused():
    for kw in (dict(guided_regex="a+"), dict(guided_choice=["a"]), dict(allowed_token_ids=[1, 2])):
        with pytest.raises(ValueError, match="min_tokens"):
            SamplingParams(min_tokens=1, stop_token_ids=(2,), **kw)
        SamplingParams(min_tokens=0, stop_token_ids=(2,), **kw)
    SamplingParams(min_tokens=1, stop_token_ids=(2,))    # without a guide: as before


def test_a_pattern_is_not_compiled_by_the_params():
    # the syntax is checked where the request is submitted (the engine answers through request.error), not here
    assert SamplingParams(guided_regex="a(?=b)").guided


def test_the_http_fields_become_the_params():
    from swiftllm_amd.server.api_server import _sampling_params, _validate_sampling
    body = {"guided_regex": "[0-9]+", "stop_token_ids": [2]}
    assert _validate_sampling(body) is None
    sp = _sampling_params(body)
    assert sp.guided_regex == "[0-9]+" and sp.stop_token_ids == (2,) and sp.greedy and not sp.processes_logits
    sp = _sampling_params({"guided_choice": ["yes", "no"], "temperature": 0.5, "seed": 1})
    assert sp.guided_choice == ("yes", "no") and not sp.greedy
    sp = _sampling_params({"allowed_token_ids": [9, 4, 4], "min_p": 0.1, "temperature": 1.0})
    assert sp.allowed_token_ids == (4, 9) and sp.min_p == 0.1
    assert _sampling_params({}) is None
    for bad in ({"guided_regex": 3}, {"guided_choice": []}, {"guided_choice": ["a", "a"]}, {"guided_choice": "yes"},
                {"allowed_token_ids": []}, {"allowed_token_ids": [-1]}, {"allowed_token_ids": [1.5]},
                {"guided_regex": "a", "guided_choice": ["a"]}, {"guided_regex": "a", "min_tokens": 2, "stop_token_ids": [1]}):
        assert _validate_sampling(bad) is not None, bad
