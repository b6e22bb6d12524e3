"""GPU tier: a decode step is made of the launches it was made of when tests/golden/engine_step_launches.json was recorded.

The parity tests pin what a step computes, tl_engine_check_step that a step planned as written-once writes every hand-over address once.
Neither sees a projection that silently moved to another kernel, or a step that silently left the per-layer buffers (and with them the
AQL replay route): the numbers stay right, only the speed goes.  So the routing of a step -- launches per kind of tl_engine_profile_step,
its split count, tl_engine_check_step's launch count and `written_once_plan` -- is held against a table recorded by
tests/golden/make_engine_step_launches.py (the same `record` runs here): two layers of the Qwen3-4B widths with the default options,
"qmm6" = 0, "qmm3" = 0 and without per-layer buffers (TL_AQL=0), TINY_CFG, and TINY_CFG with a Qwen3-MoE layer, at 1 .. 64 rows.
A deliberate change of a route regenerates the table (see the generator's docstring) and says so."""

import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_engine_step_launches", GOLDEN / "make_engine_step_launches.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def recorded(recorder, tmp_path_factory):
    return recorder.record(recorder.models(tmp_path_factory.mktemp("step_launches")))


def test_the_table_holds_every_kind_of_step():
    """What the table is for: a fused-GEMV step and a batched step on the per-layer buffers, a batched step on the shared ones, a MoE step."""
    want = json.loads((GOLDEN / "engine_step_launches.json").read_text())
    assert all("error" not in case for case in want.values()), [k for k, case in want.items() if "error" in case]
    assert want["qwen4b_2_layers/default/1"]["written_once_plan"] == 1 and want["qwen4b_2_layers/default/16"]["written_once_plan"] == 1
    assert want["qwen4b_2_layers/shared_buffers/16"]["written_once_plan"] == 0
    assert want["qwen4b_2_layers/shared_buffers/16"]["launches"] == want["qwen4b_2_layers/default/16"]["launches"]
    assert want["tiny_moe/default/16"]["launches"][2] == 1, "the MoE layer's expert launches carry no stamps: one gate|up launch (the dense layer's)"


def test_every_step_is_made_of_the_recorded_launches(recorder, recorded):
    want = json.loads((GOLDEN / "engine_step_launches.json").read_text())
    assert sorted(recorded) == sorted(want) == sorted(f"{m}/{label}/{b}" for m, label, _, _ in recorder.SETUPS for b in recorder.BATCHES)
    differ = {key: (recorded[key], want[key]) for key in want if recorded[key] != want[key]}
    assert not differ, "steps whose launches or plan differ from the recorded table (got, recorded): " + json.dumps(differ, indent=1)
