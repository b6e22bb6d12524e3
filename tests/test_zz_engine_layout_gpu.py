"""GPU tier: the engine on the layout of csrc/engine_layout.h is the engine it was (DESIGN.md "The engine's memory layout").

tests/golden/engine_layout.json was recorded before the header existed: the written-once checker's report of a decode step over 1 .. 24 rows
of a 24-slot engine (a slot count that is no multiple of the 16-row fragment block: weighted rows of 17 - 24 sequences fill a second block
partly -- the sizing bug of round 5), and what tl_engine_get_stats reports of the engine's memory after create, after the first
verify_batch (its scratch with a matmul workspace of its own, or the engine's) and after tl_engine_set_moe_layer.  TINY shapes."""

import json
import pathlib

import numpy as np
import pytest

from helpers import TINY_CFG

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((pathlib.Path(__file__).resolve().parent / "golden" / "engine_layout.json").read_text())
CASES = {case["name"]: case for case in GOLDEN["cases"]}


def _prompts(n, vocab, seed):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(2, vocab, size=5 + i % 3)] for i in range(n)]


@pytest.fixture(scope="module")
def tiny():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert GOLDEN["cfgs"]["tiny"] == TINY_CFG
    return synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda")


def test_a_step_of_any_row_count_writes_every_hand_over_address_once(tiny):
    from tiny_llm_hip.engine import DecodeEngine

    rec = GOLDEN["check_step_24_slots"]
    eng = DecodeEngine(tiny, **rec["engine_args"])
    try:
        assert eng.replay_route() == "aql"
        for i, p in enumerate(_prompts(24, eng.vocab_size, rec["prompt_seed"])):
            eng.begin(i)
            eng.prefill(i, p)
        assert sorted(map(int, rec["reports"])) == [1, 4, 5, 16, 17, 24]
        for b, want in sorted(rec["reports"].items(), key=lambda kv: int(kv[0])):
            eng.decode(rec["steps_before_check"], batch=int(b))
            rep = eng.check_step(int(b))
            assert rep["double_writes"] == 0, (b, rep)
            assert {k: rep[k] for k in want} == want, (b, rep)
    finally:
        eng.close()


def _stats(eng):
    return {k: eng.stats()[k] for k in ("workspace_bytes", "kv_bytes")}


def test_the_memory_the_engine_reports_is_what_it_was(tiny, tmp_path):
    """After create and after the first verify_batch (tiny-b1-r8: the scratch brings its own matmul workspace; the others use the engine's),
    then a model with MoE layers after tl_engine_set_moe_layer."""
    from checkpoint_fixture import MOE_CFG_OVERRIDES, make_moe_weights, write_checkpoint
    from tiny_llm_hip import load
    from tiny_llm_hip.engine import DecodeEngine

    for name in ("tiny-b1-r8", "tiny-b24-r512", "tiny-b24-r512-fp8"):
        case = CASES[name]
        own = [r["verify"]["own_ws"] for r in case["records"] if r["what"] == "verify_alloc"]
        assert own == [1 if name == "tiny-b1-r8" else 0]
        eng = DecodeEngine(tiny, **case["engine_args"])
        try:
            assert _stats(eng) == case["stats_after_create"], name
            n = min(2, case["engine_args"]["max_batch"])
            for i, p in enumerate(_prompts(n, eng.vocab_size, 5)):
                eng.begin(i)
                eng.prefill(i, p)
            eng.verify_batch([(i, [7 + i, 9, 11]) for i in range(n)], commit=False)
            assert _stats(eng) == case["stats_after_verify"], name
        finally:
            eng.close()

    cfg = dict(TINY_CFG, **MOE_CFG_OVERRIDES)
    assert GOLDEN["moe_cfg"] == cfg
    path = write_checkpoint(tmp_path / "ckpt", cfg, make_moe_weights(cfg, seed=21), vocab_words=[f"w{i}" for i in range(cfg["vocab_size"] - 2)])
    model, _ = load(str(path))
    case = CASES["moe-b24-r8"]
    assert [r["what"] for r in case["records"]] == ["create", "set_moe_layer", "set_moe_layer"]
    eng = DecodeEngine(model, **case["engine_args"])  # (the constructor hands over the MoE layers)
    try:
        assert _stats(eng) == case["records"][-1]["stats"] == case["stats_after_create"]
    finally:
        eng.close()
