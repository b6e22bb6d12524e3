"""GPU tier: the per-slot settings across the lifecycle with every feature on at once (csrc/slot_settings.h, applied by csrc/engine.hip).
One slot samples under Mirostat with penalties, a logit bias, a regex grammar, log-probability records, a stop budget and a LoRA adapter;
what fork, move and park / unpark must carry is READ back through the API (no decode step in between, no token stream compared), and
what move and release must reset reads as the defaults."""

import math

import pytest

import lora_oracle as L
from helpers import TINY_CFG
from test_zz_stop_gpu import EngineDevice

pytestmark = pytest.mark.gpu

PROMPT = [7, 300, 301, 302, 9, 11, 500, 44, 3]


def _state(eng, slot):
    """Everything the API lets one read of the slot's settings and of the words that evolve on the device."""
    return {"mu": eng.mirostat_mu(slot), "grammar": eng.grammar_state(slot), "stop": tuple(eng.stop_state(slot)),
            "logprob": repr(eng.read_pending_logprobs(slot + 1)[slot]), "pending": eng.read_pending(slot + 1)[slot], "lora": eng.slot_lora(slot),
            "context": eng.context_len(slot)}


def _reads_as_defaults(eng, slot):
    assert math.isnan(eng.mirostat_mu(slot))
    with pytest.raises(RuntimeError, match="fewer tokens have been produced since logprobs were switched on"):
        eng.read_logprobs(slot, 1)
    with pytest.raises(RuntimeError, match="the slot has no grammar"):
        eng.grammar_state(slot)
    stop = eng.stop_state(slot)
    assert (stop.reason, stop.index, stop.generated, stop.text_bytes, stop.cut_bytes) == ("none", 0, 0, 0, 0)
    assert eng.slot_lora(slot) == -1 and eng.context_len(slot) == 0
    assert len(eng.verify(slot, PROMPT[:3])) == 3  # greedy verification refuses a slot that samples or processes: this one does neither
    assert eng.context_len(slot) == 3


def test_every_setting_travels_and_resets_through_the_lifecycle():
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    edev = EngineDevice()
    eng = DecodeEngine(synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda"), page_size=16, num_pages=64, max_batch=4, max_prefill_rows=64)
    try:
        eng.set_swap_space(4)  # two slots of up to two pages
        # (the smallest rank the engine loads is 8)
        adapter = eng.load_lora(L.to_lora_adapter(L.make_adapter(TINY_CFG, 8, seed=0, sigma=0.05, scale=1.0)))
        eng.begin(0)
        eng.set_sampling(0, 0.8, seed=11)
        eng.set_mirostat(0, 3.0, 0.1)
        eng.set_penalties(0, 1.3, 0.5, 0.25)
        eng.set_logit_bias(0, {97: 1.5, 98: -2.0})
        eng.set_grammar(0, edev.words)
        eng.set_logprobs(0, 3)
        eng.set_stop(0, None, 64)
        eng.set_lora(0, adapter)
        eng.prefill(0, PROMPT)
        eng.decode(4, batch=1)
        want = _state(eng, 0)
        assert want["context"] == len(PROMPT) + 4 and want["lora"] == adapter and not math.isnan(want["mu"])
        assert want["stop"][0] == "none" and want["stop"][2] == 5  # (the prefill's first token and four steps were checked)

        eng.fork(0, 1)
        assert _state(eng, 1) == want and _state(eng, 0) == want
        eng.move(1, 2)
        assert _state(eng, 2) == want
        eng.park(2)
        eng.unpark(2)
        assert _state(eng, 2) == want and _state(eng, 0) == want

        eng.begin(1)  # the slot the move left
        _reads_as_defaults(eng, 1)
        eng.release(2)
        eng.begin(2)
        _reads_as_defaults(eng, 2)

        eng.decode(1, batch=3)
        eng.synchronize()
        assert eng.context_len(0) == want["context"] + 1 and eng.context_len(1) == eng.context_len(2) == 4
        with pytest.raises(RuntimeError, match="engine_rewind: the slot processes its logits"):
            eng.rewind(0, 1)
        with pytest.raises(RuntimeError, match="engine_set_token: the slot processes its logits"):
            eng.set_token(0, 5)
    finally:
        eng.close()
