"""CPU tier: the plans of the decode projections without a device (csrc/linear_plan.h).

tests/linear_plan_check.cpp is a stand-alone program over the header the library itself uses, built with AddressSanitizer and UBSan and
run as its own process.  `check` sweeps row counts, reductions, tile counts, CU counts, grids and knob sets and holds every plan to what a
launch of it needs and every layer's route to kernels whose plans exist; `plans` prints the records of the requests it reads, and
tests/golden/linear_plans.json holds what the planners and the routing predicates answered when they sat in the kernel headers and in
decode_linear.h (tests/golden/make_linear_plans.py; digests, and the lines around the difference spelled out): the header must reproduce
every record -- but for the one intended difference, the
register-resident matmul's plan for 19 groups per wave at 33 .. 48 rows, which did not exist."""

import importlib.util
import json
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "linear_plan_check.cpp"
GOLDEN = ROOT / "tests" / "golden" / "linear_plans.json"
HEADER = ROOT / "tiny-llm_amd" / "csrc" / "linear_plan.h"
CSRC = ROOT / "tiny-llm_amd" / "csrc"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(CSRC)]


def _maker():
    spec = importlib.util.spec_from_file_location("make_linear_plans", ROOT / "tests" / "golden" / "make_linear_plans.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("linear_plan") / "linear_plan_check"
    subprocess.run([*FLAGS, str(DRIVER), "-o", str(out)], check=True)
    return out


def ask(exe, requests):
    done = subprocess.run([str(exe), "plans"], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    lines = done.stdout.splitlines()
    assert len(lines) == len(requests)
    return lines


def test_every_plan_is_a_launch_the_kernels_take(exe):
    done = subprocess.run([str(exe), "check"], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    m = re.fullmatch(r"ok plans=(\d+) checks=(\d+)", done.stdout.strip())
    assert m and int(m.group(1)) >= 1_000_000 and int(m.group(2)) >= int(m.group(1)), done.stdout[-400:]


def _hole(rows, cols, M):
    """the plans that did not exist: 19 groups per wave (reductions of 33 .. 76 groups) have one candidate, 16-row blocks; at 33 .. 48 rows its
    three row blocks share 256 CUs, 85 workgroups each at most, and where the tiles deal out to 81 .. 85 of them the count rounds up to 88
    (a multiple of 8): 264 workgroups, which the one-workgroup-per-CU rule (at most 256 + 7) turned away"""
    tiles = rows // 16
    tpw = -(-tiles // min(tiles, 256 // 3))
    return 33 <= M <= 48 and 32 < cols // 128 <= 76 and (-(-tiles // tpw) + 7) // 8 * 8 * 3 > 256 + 7


def test_the_header_reproduces_the_recorded_plans(exe):
    """The golden file keeps a digest per (shape, record, row range) and (knob set, model, row range); the ranges in which the parent's
    qmm6_plan refused a shape within its reach -- and the routes of the models that own such a shape -- are spelled out, so that the one
    intended difference is compared line by line."""
    golden, maker = json.loads(GOLDEN.read_text()), _maker()
    assert golden["cus"] == 256 and golden["models"] == {m: list(v) for m, v in maker.MODEL_SHAPES.items()}
    assert golden["row_ranges"] == [list(r) for r in maker.ROW_RANGES] == [[1, 16], [17, 32], [33, 48], [49, 64]]
    assert len(golden["models"]) == 7 and len(golden["plans"]) == len(maker.shapes()) and set(golden["knob_sets"]) == set(maker.KNOB_SETS)
    records, spelled, changed = 0, 0, []
    for rows, cols in maker.shapes():
        recorded = golden["plans"][f"{rows} {cols}"]
        for name, requests in maker.plan_requests(rows, cols):
            parts = maker.chunks(ask(exe, requests))
            assert len(recorded[name]) == len(parts)
            for (first, _), want, have in zip(maker.ROW_RANGES, recorded[name], parts):
                records += len(have)
                if isinstance(want, str):  # a digest: the whole range as recorded
                    assert maker.digest(have) == want, f"{name} {rows} x {cols} from {first} rows: {have[0]} ..."
                    continue
                assert len(want) == len(have)
                spelled += len(want)
                for M, (w, h) in enumerate(zip(want, have), start=first):
                    if w == h:
                        continue
                    # the one intended difference: a plan where there was none, (MB 1, GPW 19, three row blocks); nothing that was ok moved
                    assert name.startswith("qmm6") and _hole(rows, cols, M) and w.split()[-1] == "0", f"{name} {rows} x {cols} at {M} rows: {h} against {w}"
                    MB, GPW, sets, row_blocks, wgs, tpw, lds, ok = (int(v) for v in h.split())
                    assert (MB, GPW, sets, row_blocks, ok) == (1, 19, 1, 3, 1) and wgs * row_blocks > 256 + 7, f"{name} {rows} x {cols} at {M} rows: {h}"
                    changed.append((rows, cols, M))
    assert records >= 13000 and spelled >= 96
    # ... and every plan of the hole changed: gate|up and lm_head of the 5,120-wide models (Qwen3-14B / 32B)
    assert {(r, c) for r, c, _ in changed} == {(r, c) for r, c in maker.shapes() if _hole(r, c, 40)} and len(changed) == 2 * 16 * len({(r, c) for r, c, _ in changed})
    routes = 0
    for knob_set, knobs in golden["knob_sets"].items():
        assert knobs == maker.knobs(knob_set)
        for model in golden["models"]:
            parts = maker.chunks(ask(exe, maker.route_requests(knob_set, model)))
            for (first, _), want, have in zip(maker.ROW_RANGES, golden["routes"][knob_set][model], parts):
                routes += len(have)
                if isinstance(want, str):
                    assert maker.digest(have) == want, f"{knob_set} {model} from {first} rows: {have[0]} ..."
                    continue
                spelled += len(want)
                for batch, (want_line, have_line) in enumerate(zip(want, have), start=first):
                    if want_line == have_line:
                        continue
                    # what the hole took with it: gate|up and lm_head of a 5,120-wide model off the register-resident matmul at 33 .. 48 rows
                    assert golden["models"][model][0] == 5120 and 33 <= batch <= 48 and knobs[1] == 1 and knobs[4] == 0, f"{knob_set} {model} at {batch} rows: {have_line} against {want_line}"
                    w, h = want_line.split(" | "), have_line.split(" | ")
                    assert (w[0], w[2], w[3], w[5]) == (h[0], h[2], h[3], h[5]) and w[1].split()[:2] == h[1].split()[:2]
                    assert [p[0] for p in w[1].split()[2:]] == ["0", "0", "0"] and [p[0] for p in h[1].split()[2:]] == ["1", "0", "1"], f"{knob_set} {model} at {batch} rows: {have_line} against {want_line}"
    assert routes >= 6000 and spelled >= 600


def test_the_batched_matmul_has_a_plan_wherever_its_reduction_fits(exe):
    """ADVICE.md (round 6): the one-workgroup-per-CU rule of qmm6_plan rejected the only candidate there is at 19 groups per wave, 33 .. 48 rows
    and 81 tiles or more -- gate|up of a 5,120-wide model silently left the batched route.  Every projection of MODEL_SHAPES whose reduction fits
    4 waves x 19 groups has a plan at 5 .. 64 rows."""
    maker = _maker()
    shapes = [(rows, cols) for rows, cols in maker.shapes() if cols // 128 <= 4 * 19]
    assert len(shapes) >= 25 and (2 * 17408, 5120) in shapes and (5120, 17408) not in shapes
    for rows, cols in shapes:
        for line, M in zip(ask(exe, [f"qmm6 0 {M} {rows} {cols}" for M in range(5, 65)]), range(5, 65)):
            MB, GPW, sets, row_blocks, wgs, tpw, lds, ok = (int(v) for v in line.split())
            assert ok == 1 and 4 * GPW >= cols // 128 and MB * row_blocks >= (M + 15) // 16, f"{rows} x {cols} at {M} rows: {line}"
    assert ask(exe, ["qmm6 0 33 34816 5120", "qmm6 0 48 1360 5120"]) == ["1 19 1 3 88 26 136000 1", "1 19 1 3 88 1 136000 1"]


def test_the_plan_header_is_host_only():
    text = HEADER.read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text and "__host__" not in text
    assert '#include "' not in text  # nothing of the project's device code either
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", str(HEADER)], check=True)
    # ... and the only place that plans: no planner, table predicate, LDS size or routing predicate is defined anywhere else under csrc/
    defined = re.compile(r"^\s*(?:static |inline |constexpr |__host__ |__device__ )*(?:bool|int|size_t|\w+Plan|LayerRoute)\s+"
                         r"(\w+_plan|\w+_has_variant|\w+_lds_bytes|gemv_takes_rows|qmm6_takes|takes_skinny_matmul|weighted_rows_apply|wo_merge_applicable|plan_layer|"
                         r"rows_travel_in_fragment_order)\s*\(", re.M)
    for path in sorted(CSRC.glob("*")):
        if path.suffix not in (".h", ".hip", ".cpp", ".inc") or path == HEADER:
            continue
        names = {n for n in defined.findall(path.read_text()) if not n.startswith(("gemm8", "attn", "fa_", "tl_"))}
        assert not names, f"{path.name} defines {sorted(names)}"
    for table in ("Q3_TABLE", "Q3_MERGE_TABLE", "QM3_TABLE", "QM3P_TABLE", "QM6_TABLE", "QM7_TABLE"):
        spelled = [p.name for p in sorted(CSRC.glob("*")) if p.is_file() and re.search(rf"#define {table}\(", p.read_text(errors="ignore"))]
        assert spelled == [HEADER.name], f"{table} is spelled in {spelled}"
