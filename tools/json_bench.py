"""JSON mode (csrc/grammar_stack.h: the stack twin of the processing launch) against the regex twin and the plans without a grammar,
on one Qwen3-4B-shaped synthetic engine (the weights bench.py builds) and tools/grammar_bench.py's synthetic 151,936-token vocabulary
with brackets added.  Settings alternated in one process; at 1 and 64 slots, all of them set alike, ms per decode step (one step per
call).  Every slot is led into one configuration by a scripted logit bias and held there by a bias on a token that loops in it (the
tool asserts that all slots end in one and the same configuration):

    off            no processing slot
    bias           bias-only processing slots (the list every variant below carries too)
    regex_light    [ ]*"[^"\\\\]*" in its start state (few tokens can be walked); the regex twin
    regex_heavy    the same inside the string (most tokens, the long ones included, stay alive)
    json_light     compile_json("value", "free") in its start state; the stack twin (116 states: the current row in LDS, the rest through L2)
    json_heavy     the same inside a string
    json_pops      the same after `[[[[1`: the state in which tokens that begin with `]` or `,` are walked through the pop table

and the kind-7 kernel time of tl_engine_profile_step (the processing launch + the step end; `off` is the step end alone).

    python tools/json_bench.py [--steps 32] [--rounds 3] [--slots 1,64]                      -> profiles/json_bench.json, "stack_twin"
    python tools/json_bench.py --unchanged LABEL [--root TREE]                                -> the same file, "unchanged"[LABEL]

--unchanged LABEL measures only the plans this feature must not change (off, bias, regex_light, regex_heavy) and stores them under LABEL;
--root TREE imports the library from another checkout (a build of the parent commit), so that one command can alternate
this_1 / parent_1 / this_2 / parent_2 and the file shows this commit's times inside the parent's own run-to-run spread."""

import argparse
import json
import math
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent.parent


def _root():
    for i, a in enumerate(sys.argv):
        if a == "--root" and i + 1 < len(sys.argv):
            return Path(sys.argv[i + 1]).resolve()
    return HERE


ROOT = _root()
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip", HERE / "tools"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from grammar_bench import CFG, synthetic_vocabulary  # noqa: E402

UNCHANGED = ("off", "bias", "regex_light", "regex_heavy")
VARIANTS = UNCHANGED + ("json_light", "json_heavy", "json_pops")
STRING = rb'[ ]*"[^"\\]*"'
# variant -> (grammar, tokens that lead into the configuration, the token that loops in it)
SCRIPTS = {"off": (None, [], None), "bias": (None, [], b"x"), "regex_light": ("regex", [], b" "), "regex_heavy": ("regex", [b'"'], b"x"),
           "json_light": ("json", [], b" "), "json_heavy": ("json", [b'"'], b"x"), "json_pops": ("json", [b"[", b"[", b"[", b"[", b"1"], b" ")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", default="1,64")
    ap.add_argument("--unchanged", default=None, metavar="LABEL")
    ap.add_argument("--root", default=None)
    ap.add_argument("--out", default=str(HERE / "profiles" / "json_bench.json"))
    args = ap.parse_args()
    from tiny_llm_hip import grammar as G
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "json_bench needs a GPU"
    V = CFG["vocab_size"]
    slots = [int(s) for s in args.slots.split(",")]
    B = max(slots)
    variants = UNCHANGED if args.unchanged else VARIANTS
    tokens = synthetic_vocabulary(V)
    edge = [b"],[", b"}}", b'{"a":[', b"]]]]", b"]]", b"[[", b"[1,2,3,4,5,6,7,8,9]", b'"abcdefghijklmno"', b"[" * 17]
    tokens[300:300 + len(edge)] = edge
    rng = np.random.default_rng(1)
    for j in rng.choice(np.arange(400, V - 4), 20000, replace=False):  # brackets in one token of eight: a BPE vocabulary's share is smaller
        t = bytearray(tokens[int(j)])
        if t:
            t[int(rng.integers(0, len(t)))] = b"[]{}"[int(rng.integers(0, 4))]
            tokens[int(j)] = bytes(t)
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    eng = DecodeEngine(model, page_size=128, num_pages=3 * B + 8, max_batch=B, max_prefill_rows=128)
    eng.make_vocab(*G.vocabulary_bytes_from_strings(tokens))
    eos = [V - 1, V - 2]
    dfas = {"regex": G.compile_regex(STRING)}
    if not args.unchanged:
        dfas["json"] = G.compile_json("value", "free")
    grammars = {k: eng.make_grammar(d, eos) for k, d in dfas.items()}
    prompt = [(7 * i + 3) % V for i in range(128)]

    ids = {t: tokens.index(t) for _, lead, loop in SCRIPTS.values() for t in lead + [loop] if t is not None}

    def bias_on(token):
        return {ids[token]: 50.0, **{t: -math.inf for t in eos}}

    def start(n, variant):
        """n slots led into the variant's configuration, holding a pending token that loops in it"""
        kind, lead, loop = SCRIPTS[variant]
        script = lead + [loop] if loop is not None else []
        for i in range(n):
            eng.begin(i)
            if script:
                eng.set_logit_bias(i, bias_on(script[0]))
            if kind is not None:
                eng.set_grammar(i, grammars[kind])
            eng.prefill(i, prompt)
        for token in script[1:]:
            for i in range(n):
                eng.set_logit_bias(i, bias_on(token))
            eng.decode(1, batch=n)

    def held(n, variant):
        """the one configuration all n slots are in (None without a grammar)"""
        kind = SCRIPTS[variant][0]
        if kind is None:
            return None
        read = eng.grammar_config if kind == "json" else eng.grammar_state
        seen = sorted({tuple(read(i)) for i in range(n)})
        assert len(seen) == 1 and seen[0][0] >= 0, f"{variant}: the slots are not held in one configuration: {seen[:4]}"
        return list(seen[0])

    def stop(n):
        eng.synchronize()
        for i in range(n):
            eng.release(i)

    def step_ms(n, variant):
        start(n, variant)
        eng.decode(2, batch=n)
        before = held(n, variant)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.decode(1, batch=n)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        assert held(n, variant) == before, f"{variant}: the slots moved while they were timed"
        stop(n)
        return ms, before

    def kind7_us(n, variant, repeats=5):
        start(n, variant)
        eng.decode(2, batch=n)
        best = min(eng.profile_step(n)["kinds"][eng.PROFILE_KINDS[7]]["us"] for _ in range(repeats))
        held(n, variant)
        stop(n)
        return best

    result = {"route": eng.replay_route(), "states": {k: int(d.n_states) for k, d in dfas.items()}, "slots": {}}
    for n in slots:
        res = {v: [] for v in variants}
        seen = {}
        for _ in range(args.rounds):
            for v in variants:  # alternated: every round visits every setting
                ms, cfg = step_ms(n, v)
                res[v].append(ms)
                if cfg is not None:
                    seen[v] = cfg
        entry = {"step_ms": {v: round(min(t), 4) for v, t in res.items()}, "step_ms_rounds": {v: [round(x, 4) for x in t] for v, t in res.items()},
                 "held_in": seen}
        if not args.unchanged:
            entry["kind7_us"] = {v: round(kind7_us(n, v), 2) for v in variants}
            ms = entry["step_ms"]
            entry["stack_twin_over_regex_twin_us"] = {"light": round((ms["json_light"] - ms["regex_light"]) * 1e3, 1),
                                                      "heavy": round((ms["json_heavy"] - ms["regex_heavy"]) * 1e3, 1),
                                                      "pops_over_regex_heavy": round((ms["json_pops"] - ms["regex_heavy"]) * 1e3, 1)}
        result["slots"][str(n)] = entry
    eng.close()
    path = Path(args.out)
    out = json.loads(path.read_text()) if path.exists() else {}
    out.update({"tool": "tools/json_bench.py", "measured": True,
                "unit": "ms per decode step, best of rounds (step_ms_rounds: every round); kind7_us: processing launch + step end, best of 5"})
    if args.unchanged:
        out.setdefault("unchanged", {})[args.unchanged] = result
    else:
        out["stack_twin"] = result
    path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({args.unchanged or "stack_twin": result}))


if __name__ == "__main__":
    main()
