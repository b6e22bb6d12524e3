"""CPU tier: the replay route of tl_engine_decode without a device (csrc/replay_route.h; DESIGN.md, "The replay route").

tests/replay_route_check.cpp is a stand-alone program over the header the library itself uses, built with AddressSanitizer and UBSan and
run as its own process.  `check` walks random decode calls with injected failures through tl_engine_decode's loop over a fake device and
holds every action to the route's properties; `trace` replays the calls of tests/golden/replay_routes.json -- recorded on the GPU before
the header existed (tests/golden/make_replay_routes.py) -- and must arrive at the recorded counters and route texts."""

import json
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "replay_route_check.cpp"
GOLDEN = ROOT / "tests" / "golden" / "replay_routes.json"
HEADER = ROOT / "tiny-llm_amd" / "csrc" / "replay_route.h"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tiny-llm_amd" / "csrc")]
# the bit order of the driver's feature masks (features_of)
FEATURES = ("samples", "logprobs", "processes", "grammar", "stack_grammar", "truncates", "mirostat", "lora", "stop", "dry")
COUNTERS = ("decode_steps", "graph_captures", "graph_replays", "aql_steps", "graph_cache_flushes")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("replay_route") / "replay_route_check"
    subprocess.run([*FLAGS, str(DRIVER), "-o", str(out)], check=True)
    return out


def _mask(names):
    return sum(1 << FEATURES.index(n) for n in names)


def test_every_action_of_a_random_walk_keeps_the_route(exe):
    done = subprocess.run([str(exe), "check"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    m = re.fullmatch(r"ok calls=(\d+) steps=(\d+) checks=(\d+)", done.stdout.strip())
    assert m and int(m.group(1)) >= 100_000 and int(m.group(2)) >= int(m.group(1)) and int(m.group(3)) >= int(m.group(2)), done.stdout[-400:]


def test_the_golden_holds_what_it_is_for():
    golden = json.loads(GOLDEN.read_text())
    assert sorted(golden) == ["calls/TL_AQL=0", "calls/TL_AQL=1", "flush/TL_AQL=0", "flush/TL_AQL=1"]
    for name, run in golden.items():
        on = name.endswith("=1")
        assert run["aql_on"] == run["written_once"] == int(on)
        total = {k: sum(c["counters"][k] for c in run["calls"]) for k in COUNTERS}
        assert (total["aql_steps"] > 0) == on and total["graph_cache_flushes"] == int(name.startswith("flush")), (name, total)
        decodes = [c for c in run["calls"] if c["kind"] == "decode"]
        assert any(s["new_page"] for c in decodes for s in c["steps"][1:]), f"{name}: no call crosses a page in mid-call"
    calls = golden["calls/TL_AQL=1"]["calls"]
    assert {c["kind"] for c in calls} == {"decode", "profile", "check"} and any(not c["use_graph"] for c in calls if c["kind"] == "decode")
    assert {c["batch"] for c in calls} >= {1, 4, 5, 8}
    armed = [c for c in calls if "stop" in c["live_features"]]
    assert armed and all(c["counters"]["aql_steps"] == 0 and c["route"].startswith("hipgraph: a slot is armed") for c in armed)
    assert any("samples" in c["live_features"] and c["counters"]["aql_steps"] > 0 and c["route"] == "aql" for c in calls)


def test_the_header_reproduces_the_recorded_routes(exe):
    golden = json.loads(GOLDEN.read_text())
    for name, run in golden.items():
        lines = [f"engine {run['aql_on']} {run['written_once']} {run['aql_why']}".rstrip()]
        for call in run["calls"]:
            lines.append(f"call {int(call['kind'] != 'decode')} {call['batch']} {call['use_graph']} {len(call['steps'])} {_mask(call['live_features'])}")
            lines += [f"step {s['plan'][0]} {s['plan'][1]} {s['plan'][2]} {_mask(s['features'])} {s['new_page']}" for s in call["steps"]]
        done = subprocess.run([str(exe), "trace"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        got = done.stdout.splitlines()
        assert len(got) == len(run["calls"])
        for call, line in zip(run["calls"], got):
            counters, _, route = line.partition("|")
            assert dict(zip(COUNTERS, map(int, counters.split()))) == call["counters"] and route == call["route"], (name, call["label"], line)


def test_the_route_header_is_host_only():
    text = HEADER.read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text
    assert re.findall(r'#include "([^"]+)"', text) == ["slot_settings.h"]  # StepFeatures, and nothing else of the project
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-I", str(HEADER.parent), str(HEADER)], check=True)


def test_the_engine_keeps_no_route_state_of_its_own():
    engine = (ROOT / "tiny-llm_amd" / "csrc" / "engine.hip").read_text()
    assert not re.search(r"\bon_queue\b|\bdrop_plans\b", engine) and engine.count("call.finish()") >= 2 and "ReplayCallEnd end{" in engine
