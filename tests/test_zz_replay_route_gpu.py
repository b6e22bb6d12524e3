"""GPU tier: every decode call of the scripted runs takes the route it took when tests/golden/replay_routes.json was recorded.

The parity tests pin what a step computes on either route; they do not see a call that silently left the AQL queue, captured a plan
twice, never flushed the plan cache or reported another sentence.  tests/golden/make_replay_routes.py (the same `record` runs here; its
docstring lists the scenarios) records per call the counters it moved and tl_engine_replay_route(), per step the attention plan, the
feature set and whether a slot entered a new page -- TINY_CFG, 8 slots on 128-token pages, both TL_AQL settings -- and asserts while
recording that the plan cache flushed and that a call rode the queue exactly when its plans want a program.  The same table feeds the
host-only model of the route (tests/test_replay_route_cpu.py)."""

import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("make_replay_routes", GOLDEN / "make_replay_routes.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def recorded(recorder):
    return recorder.record(recorder.model())


@pytest.mark.parametrize("scenario", ["calls", "flush"])
@pytest.mark.parametrize("aql", ["1", "0"])
def test_every_call_takes_the_recorded_route(recorder, recorded, scenario, aql):
    want = json.loads((GOLDEN / "replay_routes.json").read_text())
    assert sorted(recorded) == sorted(want) == sorted(f"{s}/TL_AQL={a}" for s in recorder.SCENARIOS for a in recorder.ROUTES)
    key = f"{scenario}/TL_AQL={aql}"
    got, run = recorded[key], want[key]
    assert {k: v for k, v in got.items() if k != "calls"} == {k: v for k, v in run.items() if k != "calls"}
    assert [c["label"] for c in got["calls"]] == [c["label"] for c in run["calls"]]
    differ = [(g, w) for g, w in zip(got["calls"], run["calls"]) if g != w]
    assert not differ, "calls whose route differs from the recorded table (got, recorded): " + json.dumps(differ[:3], indent=1)
