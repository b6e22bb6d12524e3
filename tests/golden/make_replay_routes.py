"""Generates tests/golden/replay_routes.json: which route every decode call of a scripted run took, per call and per step.

tl_engine_decode decides, step by step, who owns the work of a call -- the HIP stream (an eager step, a capture, hipGraphLaunch) or the
engine's own AQL queue -- and what must happen at every change of owner (csrc/replay_route.h).  The parity tests pin
what the steps COMPUTE on both routes; this table pins what the decision WAS: per call the counters it moved (decode_steps,
graph_captures, graph_replays, aql_steps, graph_cache_flushes) and tl_engine_replay_route() behind it, per step the attention plan
(n_splits, tokens_per_split, heads per workgroup: with the batch and the feature set, the key of the captured plan), the feature set and
whether a slot entered a new page.  tests/replay_route_check.cpp (mode `trace`) replays the table through the header's record without a
device and must arrive at the same counters and sentences.

Scenarios (tests/test_zz_replay_route_gpu.py runs the same `record`), each with TL_AQL=1 and TL_AQL=0: TINY_CFG, 8 slots on 128-token
pages behind prompts that end 3 .. 10 tokens short of a page, so calls cross pages in mid-call.
  calls: a warm call; multi-step calls at 1, 4, 5 and 8 sequences with a profiled and a checked step between them; a call with
         use_graph=0; slot 0 armed with a stop set (the plans leave the queue), disarmed, sampling (back on the queue), greedy again
  flush: 2 steps at every batch 1 .. 8 under every combination of sampling, logprobs and penalties on slot 0 -- 64 keys and more
         against a cache of 48: graph_cache_flushes reaches 1 (asserted here)
In all of them a plan has a program exactly when the route is on, the step was written once and no feature keeps the graph (a dense
model, contexts under 600 tokens): asserted here, call by call, through aql_steps.

Needs the GPU.  Run from the repository root at the commit whose routing is to be recorded:
    python tests/golden/make_replay_routes.py [--out tests/golden/replay_routes.json]"""

import argparse
import itertools
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for extra in (ROOT, ROOT / "tests", ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(extra) not in sys.path:
        sys.path.insert(0, str(extra))

PAGE = 128
LENGTHS = (125, 250, 120, 377, 246, 118, 123, 249)  # 3, 6, 8, 7, 10, 10, 5 and 7 tokens short of a page
COUNTERS = ("decode_steps", "graph_captures", "graph_replays", "aql_steps", "graph_cache_flushes")
GRAPH_ONLY = ("stop", "lora", "mirostat", "dry")  # the features whose plans never become a program (graph_only_reason)
SCENARIOS = ("calls", "flush")
ROUTES = ("1", "0")  # TL_AQL


def model():
    import tiny_llm_ext_hip as ext
    from helpers import TINY_CFG
    from tiny_llm_hip.synthetic import synthetic_qwen3

    ext.load_library(str(ROOT))
    return TINY_CFG, synthetic_qwen3(TINY_CFG, seed=12, sigma=0.05, device="cuda")


class _Run:
    """One engine and the host's own account of it: contexts, what each slot has switched on, the calls so far."""

    def __init__(self, cfg, mdl, aql):
        from tiny_llm_hip.engine import DecodeEngine

        self.cfg = cfg
        old = os.environ.get("TL_AQL")
        os.environ["TL_AQL"] = aql
        try:
            n = len(LENGTHS)
            pages = sum(ln // PAGE + 4 for ln in LENGTHS) + 2
            self.eng = DecodeEngine(mdl, page_size=PAGE, num_pages=pages, max_batch=n, max_prefill_rows=128)
        finally:
            if old is None:
                os.environ.pop("TL_AQL", None)
            else:
                os.environ["TL_AQL"] = old
        rng = np.random.default_rng(7)
        for slot, ln in enumerate(LENGTHS):
            self.eng.begin(slot)
            self.eng.prefill(slot, [int(t) for t in rng.integers(2, cfg["vocab_size"], size=ln)])
        self.on = [set() for _ in LENGTHS]  # per slot: the features it has switched on
        route = self.eng.replay_route()
        self.aql_on = route == "aql"
        self.written_once = None  # what tl_engine_check_step says of the steps of this engine
        self.out = {"aql_on": int(self.aql_on), "aql_why": route.partition(": ")[2], "calls": []}
        self.before = self.eng.stats()

    def features(self, batch):
        return sorted(set().union(*self.on[:batch]))

    def _plan(self, batch, context):
        import ctypes

        import tiny_llm_ext_hip as ext

        out3 = (ctypes.c_int * 3)()
        assert ext.lib().tl_decode_attention_plan(batch, context, self.cfg["num_attention_heads"], self.cfg["num_key_value_heads"], out3) == 1
        return list(out3)

    def _close_call(self, label, kind, batch, steps, use_graph, contexts):
        eng = self.eng
        feats = self.features(batch)
        after = eng.stats()
        assert [eng.context_len(s) for s in range(batch)] == [c + steps for c in contexts], f"{label}: a slot stopped in mid-call"
        call = {"label": label, "kind": kind, "batch": batch, "use_graph": int(use_graph),
                "steps": [{"plan": self._plan(batch, max(contexts) + i), "features": feats, "new_page": int(any((c + i) % PAGE == 0 for c in contexts))}
                          for i in range(steps)],
                "counters": {k: after[k] - self.before[k] for k in COUNTERS}, "live_features": self.features(len(LENGTHS)),
                "route": eng.replay_route()}
        self.before = after
        self.out["calls"].append(call)
        return call

    def decode(self, label, batch, steps, use_graph=True):
        contexts = [self.eng.context_len(s) for s in range(batch)]
        self.eng.decode(steps, batch=batch, use_graph=use_graph)
        call = self._close_call(label, "decode", batch, steps, use_graph, contexts)
        # a plan has a program iff the route is on, the step was written once and no feature keeps the graph: every replayed step of
        # such a call rode the queue, no step of any other call did
        wanted = self.aql_on and self.written_once is not False and not set(call["steps"][0]["features"]) & set(GRAPH_ONLY)
        c = call["counters"]
        assert c["decode_steps"] == steps and c["aql_steps"] == (c["graph_replays"] if wanted else 0), (label, c)
        return call

    def profile(self, label, batch):
        contexts = [self.eng.context_len(s) for s in range(batch)]
        self.eng.profile_step(batch)
        self._close_call(label, "profile", batch, 1, False, contexts)

    def check(self, label, batch):
        contexts = [self.eng.context_len(s) for s in range(batch)]
        rep = self.eng.check_step(batch)
        assert rep["written_once_plan"] == int(self.aql_on), (label, rep)
        self.written_once = bool(rep["written_once_plan"])
        self._close_call(label, "check", batch, 1, False, contexts)

    def close(self):
        self.out["written_once"] = int(bool(self.written_once))
        self.eng.close()
        return self.out


def _calls(run):
    eng = run.eng
    run.decode("warm", 1, 1)
    for batch in (1, 4, 5, 8):
        run.decode(f"batch {batch}", batch, 6)
        run.profile(f"profiled step at {batch}", batch)
        run.check(f"checked step at {batch}", batch)
        run.decode(f"batch {batch} again", batch, 3)
    run.decode("use_graph=0", 4, 3, use_graph=False)
    stop = eng.make_stop_set(ids=[1])
    eng.set_stop(0, stop, max_new_tokens=4000)
    run.on[0].add("stop")
    run.decode("slot 0 armed, batch 4", 4, 4)
    run.decode("slot 0 armed, batch 1", 1, 2)
    eng.set_stop(0, None, 0)
    run.on[0].discard("stop")
    run.decode("disarmed", 4, 3)
    eng.set_sampling(0, temperature=0.8, top_k=20, seed=5)
    run.on[0].add("samples")
    run.decode("slot 0 samples, batch 4", 4, 4)
    run.decode("slot 0 samples, batch 8", 8, 2)
    eng.set_sampling(0, temperature=0.0)
    run.on[0].discard("samples")
    run.decode("greedy again", 8, 3)


def _flush(run):
    eng = run.eng
    run.decode("warm", 1, 1)
    run.check("checked step at 1", 1)
    for samples, logprobs, penalties in itertools.product((False, True), repeat=3):
        eng.set_sampling(0, temperature=0.8 if samples else 0.0, seed=5)
        eng.set_logprobs(0, 0 if logprobs else None)
        eng.set_penalties(0, repetition=1.1 if penalties else 1.0)
        run.on[0] = {name for name, on in (("samples", samples), ("logprobs", logprobs), ("processes", penalties)) if on}
        for batch in range(1, len(LENGTHS) + 1):
            run.decode(f"samples={int(samples)} logprobs={int(logprobs)} penalties={int(penalties)} batch {batch}", batch, 2)
    assert eng.stats()["graph_cache_flushes"] >= 1, "64 keys and more did not flush a cache of 48 plans"


def record(cfg_model, log=None) -> dict:
    """{"<scenario>/TL_AQL=<0|1>": {"aql_on", "aql_why", "written_once", "calls": [...]}}"""
    cfg, mdl = cfg_model
    out = {}
    for name, aql in itertools.product(SCENARIOS, ROUTES):
        run = _Run(cfg, mdl, aql)
        try:
            {"calls": _calls, "flush": _flush}[name](run)
        finally:
            out[f"{name}/TL_AQL={aql}"] = run.close()
        if log:
            for call in out[f"{name}/TL_AQL={aql}"]["calls"]:
                log(f"{name}/TL_AQL={aql}: {call['label']}: {call['counters']} {call['route']}")
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "replay_routes.json"))
    args = ap.parse_args()
    table = record(model(), log=lambda s: print(s, flush=True))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(table, indent=None, sort_keys=True, separators=(",", ":")).replace('},{"label"', '},\n{"label"') + "\n")
    print(f"wrote {args.out} ({sum(len(v['calls']) for v in table.values())} calls)")


if __name__ == "__main__":
    main()
