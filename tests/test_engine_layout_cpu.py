"""CPU tier: the engine's memory layout without a device (csrc/engine_layout.h; DESIGN.md "The engine's memory layout").

tests/engine_layout_check.cpp is a stand-alone program over the header the library itself uses, built with AddressSanitizer and UBSan and
run as its own process.  `check` walks a grid of configurations and holds every piece to what its writers write; `layout` prints the four
layouts of the configurations it reads, and tests/golden/engine_layout.json holds the offsets, totals and inputs the engine had before the
header existed (recorded on the device from the hand-written carve / cast pairs): the header must reproduce every one of them."""

import json
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "engine_layout_check.cpp"
GOLDEN = ROOT / "tests" / "golden" / "engine_layout.json"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tiny-llm_amd" / "csrc")]
CFG_FIELDS = ("hidden_size", "num_layers", "num_heads", "num_kv_heads", "head_dim", "intermediate_size", "vocab_size", "page_size", "num_pages",
              "max_batch", "max_pages_per_seq", "max_prefill_rows")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("engine_layout") / "engine_layout_check"
    subprocess.run([*FLAGS, str(DRIVER), "-o", str(out)], check=True)
    return out


def test_every_piece_holds_what_its_writers_write(exe):
    done = subprocess.run([str(exe), "check"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    m = re.fullmatch(r"ok configs=(\d+) checks=(\d+)", done.stdout.strip())
    assert m and int(m.group(1)) >= 4000 and int(m.group(2)) >= 1_000_000, done.stdout[-400:]


def _line(rec):
    c, i = rec["cfg"], rec["inputs"]
    nums = [c[k] for k in CFG_FIELDS] + [i["attn_ws_bytes"], i["attn_ws_pad"], i["qm3_ss"], *i["plane_bytes"], i["matmul_ws_need"], i["matmul_ws_engine"],
                                         i["aql"], i["ring_cap"], i["tile_max_bytes"], i["verify_ws_rows"], i["verify_head_dim"], i["verify_result_bytes"],
                                         i["moe_k"], i["moe_e"], i["moe_i"]]
    return " ".join(str(int(n)) for n in nums)


def test_the_header_reproduces_the_recorded_offsets(exe):
    golden = json.loads(GOLDEN.read_text())
    records = [(case["name"], rec) for case in golden["cases"] for rec in case["records"]]
    models = {case["model"] for case in golden["cases"]}
    assert len(records) >= 50 and models >= {"tiny", "wide", "tiny_d64", "tiny_d32", "moe"}
    done = subprocess.run([str(exe), "layout"], input="\n".join(_line(rec) for _, rec in records) + "\n", capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    got_all = [json.loads(line) for line in done.stdout.splitlines()]
    assert len(got_all) == len(records)
    seen = {"layer": 0, "verify_own": 0, "verify_engine": 0, "moe": 0, "graph": 0}
    for (name, rec), got in zip(records, got_all):
        what = f"{name} ({rec['what']})"
        assert got["arena"] == rec["arena"], what  # every offset, act_off and the total
        if rec["inputs"]["aql"] == 0:
            assert got["layer"] == {"rows": 0, "bytes": 0} and rec["layer"]["rows"] == 0, what
            seen["graph"] += 1
        if rec["layer"]["rows"] > 0:  # (a model with MoE layers has given its per-layer block back)
            want, layers = rec["layer"], rec["cfg"]["num_layers"]
            assert {k: v for k, v in got["layer"].items() if k not in ("rows", "bytes")} == {k: want[k] for k in got["layer"] if k not in ("rows", "bytes")}, what
            assert got["layer"]["rows"] == want["rows"] and got["layer"]["bytes"] == want["stride"], what
            assert want["bytes"] == want["stride"] * layers and want["last_layer_base"] == want["stride"] * (layers - 1), what
            assert got["layer"]["plane0"] - got["layer"]["attn_ws"] == want["ws_bytes"], what
            seen["layer"] += 1
        if rec["verify"]["bytes"] > 0:
            want = rec["verify"]
            assert got["verify"]["own_ws"] == want["own_ws"] and got["verify"]["bytes"] == want["bytes"], what
            assert want["matmul_ws"] == (got["verify"]["matmul_ws"] if want["own_ws"] else -1), what
            for k, v in got["verify"].items():
                if k not in ("own_ws", "bytes", "matmul_ws"):
                    assert v == want[k], (what, k)
            assert want["ws_bytes"] == (rec["inputs"]["matmul_ws_need"] if want["own_ws"] else rec["inputs"]["matmul_ws_engine"]), what
            seen["verify_own" if want["own_ws"] else "verify_engine"] += 1
        if rec["moe"]["bytes"] > 0:
            assert got["moe"] == rec["moe"], what
            seen["moe"] += 1
    assert all(n > 0 for n in seen.values()), seen


def test_the_layout_header_is_host_only():
    text = (ROOT / "tiny-llm_amd" / "csrc" / "engine_layout.h").read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text
    assert '#include "' not in text  # nothing of the project's device code either
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", "-include", "stddef.h", str(ROOT / "tiny-llm_amd" / "csrc" / "engine_layout.h")], check=True)
