"""Writes tests/golden/scheduler_traces.json: what batch_generate_ids and serve_requests (1, 2 and 16 staging slots) ask of the engine,
call for call, and what they return, in the scenarios of tests/scheduler_recorder.py.

The fixture pins the schedulers' behaviour at ONE commit -- the one before the three loops became one scheduler core
(tiny_llm_hip/scheduler.py); its hash is stored in the file.  It is the yardstick tests/test_scheduler_traces_cpu.py holds later code
against, so it is never regenerated from the code under test: run this script only in a checkout of that commit (with the test helper
tests/scheduler_recorder.py copied in), after building the library.

    python tests/golden/make_scheduler_traces.py
"""

import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for extra in (ROOT, ROOT / "tests", ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(extra))

from scheduler_recorder import scenarios  # noqa: E402


def main() -> None:
    traces = {name: run() for name, run in scenarios().items()}
    # scenario 5 must not go vacuous: the traces hold a staging request that gave way, a park, an unpark and a hole-closing move of a parked slot
    swap = [c for name, t in traces.items() if name.startswith("5_swap") and "lone" not in name for c in t["calls"]]
    assert any(c[0] == "park" for c in swap) and any(c[0] == "unpark" for c in swap)
    assert any(c[0] == "move" and c[-1] == "parked" for c in swap), "no parked slot was moved into a hole"
    for name, t in traces.items():
        calls = t["calls"]
        if name.startswith("5_swap") and "lone" not in name:
            assert t["error"] is None, (name, t["error"])
        if name.startswith("5_swap/"):
            batch = 3  # (every request wants more than one token: a staging slot is only released when its request gives way)
            assert any(c[0] == "release" and c[1] >= batch for c in calls), f"{name}: no staging request was requeued"
        if name.startswith("5_swap_lone"):
            assert "KV page pool exhausted" in t["error"], (name, t["error"])
        if name.startswith("10_check"):
            assert t["error"] and t["error"].startswith("ValueError") and calls == [], (name, t["error"], calls[:3])
        elif "lone" not in name:
            assert t["error"] is None and calls, (name, t["error"])
        if name.startswith("6_holes/"):
            assert any(c[0] == "move" and c[1] < 16 for c in calls), f"{name}: no hole was closed"
        if name.startswith("8_stop_block_4"):
            assert any(c[0] == "decode" and c[1] == 4 for c in calls), f"{name}: no multi-step block ran"
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    out = Path(__file__).with_name("scheduler_traces.json")
    out.write_text(json.dumps({"commit": commit, "traces": traces}, separators=(",", ":")) + "\n")
    print(f"{out}: {len(traces)} traces, {sum(len(t['calls']) for t in traces.values())} calls, {out.stat().st_size} bytes, commit {commit}")


if __name__ == "__main__":
    main()
