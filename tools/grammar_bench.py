"""Regex-constrained decoding (csrc/grammar.h) against the same decode without it, on one Qwen3-4B-shaped synthetic engine (the weights
bench.py builds) and a synthetic 151,936-token vocabulary (the single bytes, strings of 1-16 bytes, ~200 tokens of 64-200 bytes, 16
empty ones), settings alternated in one process.  At 1 / 8 / 64 slots, all of them set alike, ms per decode step (one step per call):

    off            no processing slot
    bias           bias-only processing slots (+50 on the token "x", the EOS ids banned: the list every variant below carries too, so
                   that every slot keeps producing "x" and its automaton stays in the start state, which the tool asserts)
    small_light    a small automaton ([xy]*: LDS table): a state few tokens can be walked from
    small_heavy    a small automaton ([^"]*): a state most tokens, the long ones included, stay alive in
    large_light    [xy]*"(enum of random words), > 2,048 states (current row in LDS, the rest through L2), light start state
    large_heavy    [^"]*"(enum): the same size, in the state that keeps most tokens alive

and, for the processing variants, the kind-7 kernel time of tl_engine_profile_step (the processing launch + the step end; `off` is the
step end alone).  Writes profiles/grammar_bench.json and prints it as one JSON line.

    python tools/grammar_bench.py [--steps 32] [--rounds 3] [--slots 1,8,64] [--profile-rows N]

--profile-rows N: only N rows, a few steps of every variant -- for `rocprofv3 --kernel-trace --stats -- python tools/grammar_bench.py
--profile-rows 8` (the launch is logit_process_kernel<true>)."""

import argparse
import json
import math
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
VARIANTS = ("off", "bias", "small_light", "small_heavy", "large_light", "large_heavy")


def synthetic_vocabulary(V, seed=0):
    rng = np.random.default_rng(seed)
    pieces = [bytes([c]) for c in b'0123456789abcdefghijklmnopqrstuvwxyz{}":,.- '] + [u.encode() for u in "éüñ€日本"]
    tokens = [bytes([b]) for b in range(256)]
    for _ in range(V - 256):
        tokens.append(b"".join(pieces[int(k)] for k in rng.integers(0, len(pieces), int(rng.integers(1, 17))))[:16])
    letters = [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz ,.-0123456789"]
    for j in rng.choice(np.arange(256, V - 4), 200, replace=False):
        n = int(rng.integers(64, 201))
        tokens[int(j)] = b"".join(letters[int(k)] for k in rng.integers(0, len(letters), n)) if rng.random() < 0.7 else b" " * n
    for j in rng.choice(np.arange(256, V - 4), 12, replace=False):
        tokens[int(j)] = b""
    tokens[V - 4:] = [b""] * 4
    return tokens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", default="1,8,64")
    ap.add_argument("--profile-rows", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grammar_bench.json"))
    args = ap.parse_args()
    from tiny_llm_hip import grammar as G
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "grammar_bench needs a GPU"
    V = CFG["vocab_size"]
    slots = [args.profile_rows] if args.profile_rows else [int(s) for s in args.slots.split(",")]
    B = max(slots)
    model = synthetic_qwen3(CFG, seed=0, sigma=0.02, device="cuda")
    eng = DecodeEngine(model, page_size=128, num_pages=3 * B + 8, max_batch=B, max_prefill_rows=128)
    vocab = eng.make_vocab(*G.vocabulary_bytes_from_strings(synthetic_vocabulary(V)))
    eos = [V - 1, V - 2]
    rng = np.random.default_rng(5)
    words = sorted({bytes(rng.choice(list(b"abcdefghijklmnopqrstuvwxyz0123456789 "), int(rng.integers(5, 14))).tolist()) for _ in range(700)})
    patterns = {"small_light": rb"[xy]*", "small_heavy": rb'[^"]*', "large_light": rb'[xy]*"' + G.choice(words),
                "large_heavy": rb'[^"]*"' + G.choice(words)}
    dfas = {k: G.compile_regex(p) for k, p in patterns.items()}
    grammars = {k: eng.make_grammar(d, eos) for k, d in dfas.items()}
    ban_eos = {ord("x"): 50.0, **{t: -math.inf for t in eos}}
    prompt = [(7 * i + 3) % V for i in range(128)]

    def start(n, variant):
        for i in range(n):
            eng.begin(i)
            if variant != "off":
                eng.set_logit_bias(i, ban_eos)
            if variant in grammars:
                eng.set_grammar(i, grammars[variant])
            eng.prefill(i, prompt)

    def stop(n):
        eng.synchronize()
        for i in range(n):
            eng.release(i)

    if args.profile_rows:
        for variant in VARIANTS:
            start(B, variant)
            eng.decode(8, batch=B)
            stop(B)
        print(json.dumps({"profile_rows": B}))
        return

    def step_ms(n, variant):
        start(n, variant)
        eng.decode(2, batch=n)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.decode(1, batch=n)
        eng.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        states = sorted({eng.grammar_state(i)[0] for i in range(n)}) if variant in grammars else None
        assert states in (None, [dfas[variant].start] if variant in dfas else None), f"{variant}: the slots left the start state: {states}"
        stop(n)
        return ms, states

    def kind7_us(n, variant, repeats=5):
        start(n, variant)
        eng.decode(2, batch=n)
        best = min(eng.profile_step(n)["kinds"][eng.PROFILE_KINDS[7]]["us"] for _ in range(repeats))
        if variant in grammars:
            assert {eng.grammar_state(i)[0] for i in range(n)} == {dfas[variant].start}, f"{variant}: the slots left the start state"
        stop(n)
        return best

    out = {"tool": "tools/grammar_bench.py", "unit": "ms per step (best of rounds); kind7_us: processing launch + step end, best of 5",
           "states": {k: int(d.n_states) for k, d in dfas.items()}, "route": eng.replay_route(), "slots": {}}
    for n in slots:
        res = {v: [] for v in VARIANTS}
        seen = {}
        for _ in range(args.rounds):
            for v in VARIANTS:  # alternated: every round visits every setting
                ms, states = step_ms(n, v)
                res[v].append(ms)
                if states is not None:
                    seen[v] = states[:4]
        out["slots"][str(n)] = {"step_ms": {v: round(min(t), 4) for v, t in res.items()},
                                "kind7_us": {v: round(kind7_us(n, v), 2) for v in VARIANTS}, "states_at_end": seen}
    eng.close()
    Path(args.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
