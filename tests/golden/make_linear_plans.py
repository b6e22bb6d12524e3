"""Generates tests/golden/linear_plans.json: what the decode projections' planners and routing predicates answered BEFORE
csrc/linear_plan.h existed -- the planners at the bottom of qmv.h / qmv3.h / qmm3.h / qmm6.h / qmm7.h and the predicates of decode_linear.h.

The recorder below is a throwaway program over those headers: it is compiled with hipcc (the headers hold kernels) and linked against the
built library, which supplies qmm3_num_cus -- 256 without a device -- and the three *_variant_in_table functions; it launches nothing.
It reads requests, one per line, and prints one record per request, in the formats tests/linear_plan_check.cpp (`plans`) prints from the new header:

  qmv  M rows cols            -> MR WN RPL RB blocks lds
  qmv3 M rows cols            -> MR KS CW LM blocks lds ok
  qmm3 mode M rows cols       -> MB TW LM slices tile_groups grid_x persistent tiles_per_wg NU  full_slices wgs_full tpw_full last_groups
                                 wgs_last tpw_last  lds partial_bytes ok
  qmm6 frag M rows cols       -> MB GPW NSETS row_blocks wgs tiles_per_wg lds ok
  qmm7 M rows cols            -> MB T GPW wgs row_blocks lds ok
  route <10 knobs> hidden q_dim qkv_dim intermediate vocab batch
                              -> gemv_takes_rows | (qmm6_takes, takes_skinny_matmul) of qkv, wo, gate|up, w_down, lm_head | weighted_rows_apply(wo,
                                 gate|up) | wo_merge_applicable at 2, 4, 8 attention splits | LayerRoute: batched qkv6 wo6 down gemv_weighted
                                 batched_written_once | rows_travel_in_fragment_order
  knobs: use_qmm3 use_qmm6 use_qmm7 force_qmm7 force_linear qmm3_min_rows qmm3_mode fuse_norm gemv_weighted_rows gemv_producer_ss

The grid: every distinct projection shape of MODEL_SHAPES (tests/test_decode_plans_cpu.py) x M = 1 .. 64 (the GEMV planners: 1 .. 8), both row
orders of qmm6, the three grids of qmm3; every model x batch 1 .. 64 under the knob sets KNOB_SETS.  The file keeps a digest of every
(shape, record, row range) and (knob set, model, row range) and spells out the ranges in which qmm6_plan refused a shape within its reach.
tl_decode_gemv_plan, tl_decode_batched_plan and tl_decode_streaming_plan of the same library are asked the same questions and must agree with the recorder.

Needs hipcc and the built library, no GPU.  Run from the repository root at the commit whose planners are to be recorded:
    python tests/golden/make_linear_plans.py [--out tests/golden/linear_plans.json]"""

import argparse
import ctypes
import hashlib
import json
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
CSRC = ROOT / "tiny-llm_amd" / "csrc"
LIBDIR = ROOT / "tiny-llm_amd" / "extensions_hip" / "tiny_llm_ext_hip"

# (hidden, Hq * D, (Hq + 2 Hkv) * D, intermediate, vocab): tests/test_decode_plans_cpu.py MODEL_SHAPES
MODEL_SHAPES = {
    "qwen3-0.6b": (1024, 2048, 4096, 3072, 151936), "qwen3-1.7b": (2048, 2048, 4096, 6144, 151936),
    "qwen3-4b": (2560, 4096, 6144, 9728, 151936), "qwen3-8b": (4096, 4096, 6144, 12288, 151936),
    "qwen3-14b": (5120, 5120, 7168, 17408, 151936), "qwen3-32b": (5120, 8192, 10240, 25600, 151936),
    "qwen2-7b": (3584, 3584, 4608, 18944, 152064),
}
KNOB_NAMES = ("use_qmm3", "use_qmm6", "use_qmm7", "force_qmm7", "force_linear", "qmm3_min_rows", "qmm3_mode", "fuse_norm",
              "gemv_weighted_rows", "gemv_producer_ss")
DEFAULT = dict(use_qmm3=1, use_qmm6=1, use_qmm7=1, force_qmm7=0, force_linear=0, qmm3_min_rows=5, qmm3_mode=-1, fuse_norm=1,
               gemv_weighted_rows=1, gemv_producer_ss=1)
# what tl_engine_set_option, TL_QMM3_MIN_M and the kernel numbers of tl_decode_linear can produce
KNOB_SETS = {
    "default": {}, "qmm6=0": {"use_qmm6": 0}, "qmm7=0": {"use_qmm7": 0}, "qmm3=0": {"use_qmm3": 0}, "TL_QMM3_MIN_M=9": {"qmm3_min_rows": 9},
    "force_linear=1": {"force_linear": 1}, "force_linear=2": {"force_linear": 2},
    "one-shot grid": {"qmm3_mode": 0}, "persistent grid": {"qmm3_mode": 1},
    "force_linear=2, one-shot grid": {"force_linear": 2, "qmm3_mode": 0}, "force_linear=2, persistent grid": {"force_linear": 2, "qmm3_mode": 1},
    "kernel 6": {"use_qmm7": 0, "force_qmm7": 1},
    "fuse_norm=0": {"fuse_norm": 0}, "gemv_weighted_rows=0": {"gemv_weighted_rows": 0}, "gemv_producer_ss=0": {"gemv_producer_ss": 0},
}


def projections(model):
    hidden, q_dim, qkv_dim, inter, vocab = MODEL_SHAPES[model]
    return {"qkv": (qkv_dim, hidden), "wo": (hidden, q_dim), "gate_up": (2 * inter, hidden), "down": (hidden, inter), "lm_head": (vocab, hidden)}


def shapes():
    """every distinct (rows, cols) of the models' projections, in a fixed order"""
    seen = []
    for model in MODEL_SHAPES:
        for shape in projections(model).values():
            if shape not in seen:
                seen.append(shape)
    return seen


def knobs(name):
    return [dict(DEFAULT, **KNOB_SETS[name])[k] for k in KNOB_NAMES]


def plan_requests(rows, cols):
    """(record name, request lines) of one shape"""
    yield "qmv", [f"qmv {M} {rows} {cols}" for M in range(1, 9)]
    yield "qmv3", [f"qmv3 {M} {rows} {cols}" for M in range(1, 9)]
    for mode in (-1, 0, 1):
        yield f"qmm3 mode {mode}", [f"qmm3 {mode} {M} {rows} {cols}" for M in range(1, 65)]
    for frag in (0, 1):
        yield f"qmm6 frag {frag}", [f"qmm6 {frag} {M} {rows} {cols}" for M in range(1, 65)]
    yield "qmm7", [f"qmm7 {M} {rows} {cols}" for M in range(1, 65)]


def route_requests(knob_set, model):
    k = " ".join(str(v) for v in knobs(knob_set))
    return [f"route {k} {' '.join(str(v) for v in MODEL_SHAPES[model])} {batch}" for batch in range(1, 65)]


RECORDER = r"""
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "decode_linear.h"
using namespace tl;

static tl_w4 fake(int id, int rows, int cols) {
    tl_w4 w{};
    w.weight_dev = reinterpret_cast<const uint32_t *>((uintptr_t)0x1000 * (id + 1));
    w.rows = rows, w.cols = cols;
    return w;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        in >> what;
        int M = 0, rows = 0, cols = 0, x = 0;
        if (what == "qmv") {
            in >> M >> rows >> cols;
            const QmvPlan p = qmv_plan(M, cols, rows);
            printf("%d %d %d %d %d %zu\n", p.MR, p.WN, p.RPL, p.RB, p.blocks, p.lds);
        } else if (what == "qmv3") {
            in >> M >> rows >> cols;
            const Qmv3Plan p = qmv3_plan(M, cols, rows);
            printf("%d %d %d %d %d %zu %d\n", p.MR, p.KS, p.CW, p.LM, p.blocks, p.lds, (int)p.ok);
        } else if (what == "qmm3") {
            in >> x >> M >> rows >> cols;
            const Qmm3Plan p = qmm3_plan(M, cols, rows, x);
            const Qmm3pGrid &g = p.pgrid;
            printf("%d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d  %zu %zu %d\n", p.MB, p.TW, p.LM, p.slices, p.tile_groups, p.grid_x, p.persistent,
                   p.tiles_per_wg, p.NU, g.full_slices, g.wgs_full, g.tpw_full, g.last_groups, g.wgs_last, g.tpw_last, p.lds, p.partial_bytes, (int)p.ok);
        } else if (what == "qmm6") {
            in >> x >> M >> rows >> cols;
            const Qmm6Plan p = qmm6_plan(M, cols, rows, x != 0);
            printf("%d %d %d %d %d %d %zu %d\n", p.MB, p.GPW, p.NSETS, p.row_blocks, p.wgs, p.tiles_per_wg, p.lds, (int)p.ok);
        } else if (what == "qmm7") {
            in >> M >> rows >> cols;
            const Qmm7Plan p = qmm7_plan(M, cols, rows);
            printf("%d %d %d %d %d %zu %d\n", p.MB, p.T, p.GPW, p.wgs, p.row_blocks, p.lds, (int)p.ok);
        } else if (what == "route") {
            int k[10], hidden, q_dim, qkv_dim, inter, vocab, batch;
            for (int &v : k) in >> v;
            in >> hidden >> q_dim >> qkv_dim >> inter >> vocab >> batch;
            LinearCtx ctx;
            ctx.use_qmm3 = k[0], ctx.use_qmm6 = k[1], ctx.use_qmm7 = k[2], ctx.force_qmm7 = k[3], ctx.force_linear = k[4], ctx.qmm3_min_rows = k[5];
            ctx.qmm3_mode = k[6], ctx.fuse_norm = k[7], ctx.gemv_weighted_rows = k[8], ctx.gemv_producer_ss = k[9];
            tl_layer_weights w{};
            w.wqkv = fake(0, qkv_dim, hidden), w.wo = fake(1, hidden, q_dim), w.wgu = fake(2, 2 * inter, hidden), w.wdown = fake(3, hidden, inter);
            const tl_w4 head = fake(4, vocab, hidden);
            const tl_w4 *all[5] = {&w.wqkv, &w.wo, &w.wgu, &w.wdown, &head};
            for (const tl_w4 *m : all) ctx.tiled[m->weight_dev] = TiledW4{};
            printf("%d |", (int)gemv_takes_rows(ctx, batch));
            for (const tl_w4 *m : all) printf(" %d%d", (int)qmm6_takes(ctx, *m, batch), (int)takes_skinny_matmul(ctx, *m, batch));
            printf(" | %d |", (int)weighted_rows_apply(ctx, w.wo, w.wgu, batch));
            for (int ns : {2, 4, 8}) printf(" %d", (int)wo_merge_applicable(ctx, w.wo, batch, ns, 128, q_dim / 128));
            const LayerRoute r = plan_layer(ctx, w, batch, false);
            printf(" | %d %d %d %d %d %d | %d\n", (int)r.batched, (int)r.qkv6, (int)r.wo6, (int)r.down, (int)r.gemv_weighted, (int)r.batched_written_once(),
                   (int)rows_travel_in_fragment_order(ctx, w, batch));
        } else {
            fprintf(stderr, "unknown request: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
"""


def build_recorder(tmp):
    src, exe = Path(tmp) / "linear_plan_recorder.hip", Path(tmp) / "linear_plan_recorder"
    src.write_text(RECORDER)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-I", str(CSRC),
                    str(src), "-o", str(exe), "-L", str(LIBDIR), "-ltinyllm_hip", f"-Wl,-rpath,{LIBDIR}"], check=True)
    return exe


def ask(exe, requests):
    done = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True, check=True)
    lines = done.stdout.splitlines()
    assert len(lines) == len(requests), (len(lines), len(requests), done.stderr[-2000:])
    return [" ".join(line.split()) for line in lines]


def cross_check(plans):
    """the three planners the C ABI exposes answer as the recorder did"""
    lib = ctypes.CDLL(str(LIBDIR / "libtinyllm_hip.so"))
    out = (ctypes.c_int * 6)()
    for (rows, cols) in shapes():
        rec = plans[f"{rows} {cols}"]
        for M in range(1, 65):
            if M <= 8:
                ok = lib.tl_decode_gemv_plan(M, rows, cols, out)
                got = rec["qmv3"][M - 1].split()
                assert [str(v) for v in out[:5]] + [str(ok)] == got[:5] + got[6:], (rows, cols, M)
            ok = lib.tl_decode_batched_plan(M, rows, cols, out)
            got = rec["qmm6 frag 0"][M - 1].split()
            assert [str(v) for v in out[:6]] + [str(ok)] == got[:6] + got[7:], (rows, cols, M)
            ok = lib.tl_decode_streaming_plan(M, rows, cols, out)
            got = rec["qmm7"][M - 1].split()
            assert [str(v) for v in out[:4]] + [str(ok)] == got[:4] + got[6:], (rows, cols, M)


ROW_RANGES = ((1, 16), (17, 32), (33, 48), (49, 64))  # one to four 16-row blocks


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def chunks(lines):
    """the records of one request list by row range (the GEMV planners' 8 records: one chunk)"""
    return [lines] if len(lines) == 8 else [lines[a - 1:b] for a, b in ROW_RANGES]


def refused_in_reach(rows, cols, lines):
    """a qmm6 record that says `not ok` although the reduction fits 4 waves x 19 groups and the shape is the kernel's"""
    return cols // 128 <= 4 * 19 and any(line.split()[-1] == "0" for line in lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "linear_plans.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_recorder(tmp)
        plans = {f"{rows} {cols}": {name: ask(exe, reqs) for name, reqs in plan_requests(rows, cols)} for rows, cols in shapes()}
        routes = {ks: {model: ask(exe, route_requests(ks, model)) for model in MODEL_SHAPES} for ks in KNOB_SETS}
    cross_check(plans)
    # The file holds a digest per (shape, record, row range) and per (knob set, model, row range).  Spelled out instead, line by line: the row
    # ranges in which qmm6_plan refuses a shape within its reach, with the routes of the models that own such a shape -- and, as a sample, the
    # default routes of Qwen3-4B.
    holes = {(shape, c) for shape, rec in plans.items() for c, lines in enumerate(chunks(rec["qmm6 frag 0"]))
             if refused_in_reach(*map(int, shape.split()), lines)}
    plan_doc = {shape: {name: [part if name.startswith("qmm6") and (shape, c) in holes else digest(part) for c, part in enumerate(chunks(lines))]
                        for name, lines in rec.items()} for shape, rec in plans.items()}
    owns = {model: {c for rows, cols in projections(model).values() for c in range(len(ROW_RANGES)) if (f"{rows} {cols}", c) in holes} for model in MODEL_SHAPES}
    route_doc = {ks: {model: [part if c in owns[model] or (ks, model) == ("default", "qwen3-4b") else digest(part) for c, part in enumerate(chunks(lines))]
                      for model, lines in per.items()} for ks, per in routes.items()}
    head = {"cus": 256, "models": {m: list(v) for m, v in MODEL_SHAPES.items()}, "knob_names": list(KNOB_NAMES),
            "knob_sets": {ks: knobs(ks) for ks in KNOB_SETS}, "row_ranges": [list(r) for r in ROW_RANGES]}
    one = lambda v: json.dumps(v, separators=(",", ":"))
    text = "{\n" + "".join(f"{one(k)}:{one(v)},\n" for k, v in head.items())
    text += '"plans":{\n' + ",\n".join(f"{one(k)}:{one(v)}" for k, v in plan_doc.items()) + '},\n"routes":{\n'
    text += ",\n".join(f"{one(k)}:{one(v)}" for k, v in route_doc.items()) + "}}\n"
    assert json.loads(text)["plans"] == plan_doc
    Path(args.out).write_text(text)
    spelled = sum(len(e) for doc in (plan_doc, route_doc) for per in doc.values() for v in per.values() for e in v if isinstance(e, list))
    print(f"{args.out}: {sum(len(v) for p in plans.values() for v in p.values())} plan records, "
          f"{sum(len(v) for r in routes.values() for v in r.values())} routing records, {spelled} of them spelled out")


if __name__ == "__main__":
    main()
