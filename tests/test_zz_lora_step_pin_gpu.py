"""GPU tier: a decode step under LoRA adapters launches and produces what it did when tests/golden/engine_lora_steps.json was recorded.

tests/test_zz_engine_step_launches_gpu.py pins the launches of the base program, tests/test_zz_lora_gpu.py holds an adapter step
against the truth within a tolerance.  Neither sees host code that builds the adapter plan differently -- a projection on another
kernel, another buffer, another field of a call record -- while the logits stay inside the tolerance.  So the mixed batch of
test_mixed_batches_eager_and_captured (adapters X, none, Y, X, none over the slots) is held bit for bit against a table recorded by
tests/golden/make_engine_lora_steps.py (the same `record` runs here): TINY_CFG dense and with a Qwen3-MoE layer, at 1, 4, 5 and 17
rows; per case the launches per kind of tl_engine_profile_step and its split count, tl_engine_check_step's launch count and plan
flag, tl_engine_replay_route's text, the ids of 4 greedy captured steps for every slot and the SHA-256 of the logits' bf16 bits.
A deliberate change of the adapter plan regenerates the table (see the generator's docstring) and says so."""

import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_engine_lora_steps", GOLDEN / "make_engine_lora_steps.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def recorded(recorder, tmp_path_factory):
    return recorder.record(recorder.models(tmp_path_factory.mktemp("lora_steps")))


def test_the_table_holds_adapter_plans(recorder):
    """What the table is for: every case is an adapter plan -- never written-once, on hipGraphLaunch because of the adapter -- with its
    shrink / expand launches counted by no kind (the kinds' launches are the base projections')."""
    want = json.loads((GOLDEN / "engine_lora_steps.json").read_text())
    assert sorted(want) == sorted(f"{m}/{b}" for m in recorder.MODELS for b in recorder.BATCHES)
    for key, case in want.items():
        assert case["written_once_plan"] == 0, key
        assert "LoRA" in case["replay_route"] and case["replay_route"].startswith("hipgraph"), key
        assert len(case["ids"]) == int(key.split("/")[1]) and all(len(ids) == recorder.STEPS for ids in case["ids"]), key
        assert case["graph_replays"] == recorder.STEPS, key  # every recorded id came from a captured step


def test_every_adapter_step_is_the_recorded_one(recorder, recorded):
    want = json.loads((GOLDEN / "engine_lora_steps.json").read_text())
    assert sorted(recorded) == sorted(want)
    differ = {key: (recorded[key], want[key]) for key in want if recorded[key] != want[key]}
    assert not differ, "adapter steps that differ from the recorded table (got, recorded): " + json.dumps(differ, indent=1)
