"""CPU tier: the engine's per-slot settings without a device (csrc/slot_settings.h; DESIGN.md "The slot settings").

tests/slot_settings_model_check.cpp is a stand-alone program over the header the library itself runs: a seeded random walk over five slots
and every operation of the record, with host byte arrays standing for the device blocks.  They are made from the layouts' own fill rules
and change only by the edits a call reports; after every operation they are compared with what the mirrors say the device must hold.
Built with AddressSanitizer and UBSan and run as its own process."""

import pathlib
import re
import subprocess

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "slot_settings_model_check.cpp"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tiny-llm_amd" / "csrc")]
STEPS = 50_000
FEATURES = ("sampling", "logprobs", "processing", "truncation", "lora", "stop", "flags")
REFUSALS = ("sampling.temperature", "sampling.top_k", "sampling.top_p", "sampling.mirostat", "truncation.min_p", "truncation.typical_p",
            "truncation.mirostat", "mirostat.tau", "mirostat.eta", "mirostat.excludes", "penalties.repetition", "penalties.presence", "bias.count",
            "bias.null", "bias.id", "bias.twice", "bias.value", "logprobs.top_n", "stop.budget")


def test_the_device_follows_the_mirrors_through_a_random_walk(tmp_path):
    exe = tmp_path / "slot_settings_model_check"
    subprocess.run([*FLAGS, str(DRIVER), "-o", str(exe)], check=True)
    lines = []
    for seed in ("1", "7"):
        done = subprocess.run([str(exe), str(STEPS), seed], capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        line = done.stdout.strip()
        assert line.startswith(f"ok steps={STEPS} "), line
        counts = {k: int(v) for k, v in re.findall(r"([\w.]+)=(\d+)\b", line)}
        # served calls per (lifecycle operation, feature its slot had on), and calls per kind of refusal
        for op in ("carry", "fork", "move", "park", "unpark", "reset"):
            for feature in FEATURES:
                assert counts.get(f"{op}.{feature}", 0) >= 100, (op, feature, line)
        for kind in REFUSALS:
            assert counts.get(f"refused.{kind}", 0) >= 100, (kind, line)
        for setter in ("sampling", "truncation", "mirostat", "penalties", "logit_bias", "grammar", "logprobs", "lora", "stop"):
            assert counts.get(f"set_{setter}", 0) >= 100, (setter, line)
        assert counts["asked"] >= 100 and counts["reconciled"] >= 100, line
        lines.append(line)
    assert lines[0] != lines[1]  # the seed is read


def test_the_settings_header_is_host_only():
    text = (ROOT / "tiny-llm_amd" / "csrc" / "slot_settings.h").read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text
    assert '#include "' not in text  # nothing of the project's device code either
