"""CPU tier: batch_generate_ids and serve_requests (1, 2 and 16 staging slots) ask of the engine what they asked before they shared one
scheduler core (tiny_llm_hip/scheduler.py) -- call for call, argument for argument -- and return what they returned.

tests/golden/scheduler_traces.json holds, for every scenario of tests/scheduler_recorder.py, the full call list of a recording engine,
the returned value (the finished list, or the ServingMetrics as a dict) and the error text where one is expected, written by
tests/golden/make_scheduler_traces.py from the three hand-copied loops at the commit the file names.  It is never regenerated from the
code under test.  DecodeEngine.generate shares the settings record with batch_generate_ids: its setter sequence is checked here too."""

import json
from pathlib import Path

import pytest

from scheduler_recorder import fake_grammar, fake_stop_set, scenarios

GOLDEN = json.loads((Path(__file__).parent / "golden" / "scheduler_traces.json").read_text())
SCENARIOS = scenarios()


def test_the_fixture_covers_every_scenario_and_names_its_commit():
    assert sorted(GOLDEN["traces"]) == sorted(SCENARIOS)
    assert len(GOLDEN["commit"]) == 40


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_trace_is_the_pinned_one(name):
    want, got = GOLDEN["traces"][name], SCENARIOS[name]()
    assert got["error"] == want["error"]
    for k, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, f"call {k}: {a} != {b} (after {got['calls'][max(k - 3, 0):k]})"
    assert len(got["calls"]) == len(want["calls"])
    assert got["result"] == want["result"]


def _generate_calls(**kw):
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.stop import StopState

    class Stub(DecodeEngine):
        """DecodeEngine.generate over stubbed slot calls: the log holds the setters' names in call order."""
        prefix_cache_enabled, vocab_size, max_prefill_rows = False, 1000, 64

        def __init__(self):
            self.log = []

        def __getattribute__(self, name):
            if name.startswith("set_"):
                return lambda *a, **k: self.log.append(name)
            return object.__getattribute__(self, name)

        def begin(self, slot=0):
            pass

        release = begin

        def prefill(self, slot, tokens, **k):
            pass

        def decode(self, steps, batch=None, use_graph=True):
            pass

        def stop_state(self, slot):
            return StopState("length", 0, 3, 8, 0, 0)

        def read_tokens(self, slot, count):
            return [7] * count

        def read_logprobs(self, slot, count):
            return [None] * count

    eng = Stub()
    eng.generate([1, 2, 3, 4, 5], 3, **kw)
    return eng.log


def test_generate_applies_a_request_with_every_option_in_the_documented_order_and_defaults_make_no_call():
    from tiny_llm_hip.engine import RequestSettings

    every = dict(lora=1, temperature=0.8, seed=3, repetition_penalty=1.1, logit_bias={5: 1.0}, grammar=fake_grammar("g", [9]), logprobs=2,
                 stop=fake_stop_set("s"))
    assert _generate_calls(min_p=0.1, top_k=40, **every) == ["set_lora", "set_sampling", "set_truncation", "set_penalties", "set_logit_bias",
                                                              "set_grammar", "set_logprobs", "set_stop"]
    assert _generate_calls(mirostat_tau=5.0, **every) == ["set_lora", "set_sampling", "set_mirostat", "set_penalties", "set_logit_bias",
                                                           "set_grammar", "set_logprobs", "set_stop"]
    assert _generate_calls() == []
    assert RequestSettings.apply.__doc__ and "lora, sampling, truncation / Mirostat, penalties, bias, grammar, logprobs, stop" in RequestSettings.apply.__doc__
