"""Writes tests/golden/request_cli.json: the parser surface of main.py and batch_main.py, what both scripts make of the command lines
of tests/request_cli_recorder.py (the refusal's text, or the entry points reached with their arguments, every settings call of every
engine with its values and a digest of the engine's whole call log, the notes and the printed text), and what request_settings and DecodeEngine.generate make of the ``sampling`` arguments there.

The fixture pins that behaviour at ONE commit -- the one before the request settings got their table (tiny_llm_hip/request.py); its
hash is stored in the file.  It is the yardstick tests/test_request_cli_cpu.py holds later code against, so it is never regenerated
from the code under test: run this script only in a checkout of that commit (with tests/request_cli_recorder.py, tests/golden/request_cli_prompts.txt and
the ``set_dry`` line of tests/scheduler_recorder.py copied in), after building the library.

    python tests/golden/make_request_cli.py
"""

import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for extra in (ROOT, ROOT / "tests", ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(extra))

from request_cli_recorder import record  # noqa: E402


def main() -> None:
    data = record()
    cli = {script: {name: data["pool"][k] for name, k in data[script].items()} for script in ("main", "batch_main")}
    # the scenarios must not go vacuous: every route is reached, every check refuses something, every setter is called somewhere
    entries = {e[0] for script in cli.values() for t in script.values() for e in t.get("entries", [])}
    assert entries >= {"DecodeEngine", "generate", "batch_generate_ids", "speculative_generate_ids", "batch_speculative_generate_ids", "beam_search_ids",
                       "simple_generate_with_kv_cache", "speculative_generate"}, entries
    calls = {c[0] for script in cli.values() for t in script.values() for _, log, _ in t.get("engines", []) for c in log}
    assert calls >= {"set_sampling", "set_truncation", "set_mirostat", "set_penalties", "set_grammar", "set_dry", "set_logprobs", "set_stop", "set_lora",
                     "load_lora"}, calls
    errors = [t["error"] for script in cli.values() for t in script.values() if t["error"]]
    for needle in ("Mirostat excludes", "--num-beams cannot be combined with", "--num-beams must be", "apply with --num-beams only", "must not exceed 32",
                   "--draft-model runs greedy", "--proposal-length must be", "ValueError: min_p"):
        assert any(needle in e for e in errors), needle
    notes = {n for t in cli["main"].values() for n in t.get("notes", [])}
    assert len(notes) >= 10, sorted(notes)
    assert len(cli["main"]["stop id matched"]["printed"][0].split()) == 2, "the scripted stop id did not end the answer at its third token"
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    out = Path(__file__).with_name("request_cli.json")
    out.write_text(json.dumps({"commit": commit, **data}, separators=(",", ":")) + "\n")
    print(f"{out}: {sum(len(v) for v in cli.values())} command lines, {len(data['settings'])} sampling arguments, {len(data['generate'])} generate calls, "
          f"{out.stat().st_size} bytes, commit {commit}")


if __name__ == "__main__":
    main()
