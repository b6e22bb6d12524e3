"""Text embeddings (csrc/pool.h; tiny_llm_hip.embedding.embed_ids) against the prefill passes they ride on, on one Qwen3-4B-shaped
synthetic engine (the weights bench.py builds): 128 texts of 128 .. 1,024 tokens (the serving bench's distribution), 16 slots,
4,096-row passes.  In ONE process, on ONE engine, per pooling mode ("last", "mean"):

    embed      embed_ids over the texts: embedded tokens per second of wall clock
    yardstick  the SAME begin / pass / release sequence with every pass through prefill_packed, want_logits = 0 -- what the engine
               could do before it had embeddings: the K / V of the texts and no vector
    added      1 - yardstick / embed: the share of the embed run that the final RMSNorm, the pooling launches and the copy of the
               vectors with its synchronise add to the passes

and the pooling launches alone (tiny_llm_ext_hip.pool_rows over a 4,096 x 2,560 chunk of 16 sequences, HIP events).  Nothing is
asserted about the times; the vectors are checked to be unit length.  Writes profiles/embedding.json ("measured": true) and prints it
as one JSON line.

    python tools/embedding_bench.py [--texts 128] [--min-len 128] [--max-len 1024] [--layers 36] [--repeats 3]"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path
from random import Random

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = dict(hidden_size=2560, num_hidden_layers=36, num_attention_heads=32, num_key_value_heads=8, head_dim=128, intermediate_size=9728,
           vocab_size=151936, rope_theta=1000000, rms_norm_eps=1e-6, max_position_embeddings=40960, tie_word_embeddings=True)
PAGE, SLOTS, ROWS = 128, 16, 4096


class Recorder:
    """The engine as embed_ids sees it, with every begin / pass / release written down."""

    def __init__(self, engine):
        self._engine, self.log = engine, []

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def begin(self, slot):
        self.log.append(("begin", slot))
        self._engine.begin(slot)

    def release(self, slot):
        self.log.append(("release", slot))
        self._engine.release(slot)

    def embed_packed(self, chunks, **kw):
        self.log.append(("pass", [(slot, list(tokens), False) for slot, tokens, _ in chunks]))
        return self._engine.embed_packed(chunks, **kw)


def replay(engine, log):
    for op, arg in log:
        if op == "pass":
            engine.prefill_packed(arg)
        else:
            getattr(engine, op)(arg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=128)
    ap.add_argument("--min-len", type=int, default=128)
    ap.add_argument("--max-len", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=CFG["num_hidden_layers"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "embedding.json"))
    args = ap.parse_args()
    import tiny_llm_ext_hip as ext
    from tiny_llm_hip.embedding import embed_ids
    from tiny_llm_hip.engine import DecodeEngine
    from tiny_llm_hip.synthetic import synthetic_qwen3

    assert torch.cuda.is_available(), "embedding_bench needs a GPU"
    cfg = dict(CFG, num_hidden_layers=args.layers)
    rng, nrng = Random(args.seed), np.random.default_rng(args.seed)
    lens = [rng.randint(args.min_len, args.max_len) for _ in range(args.texts)]
    texts = [[int(t) for t in nrng.integers(256, cfg["vocab_size"] - 1, n)] for n in lens]
    tokens = sum(lens)
    per_seq = -(-args.max_len // PAGE)
    model = synthetic_qwen3(cfg, seed=0, sigma=0.02, device="cuda")
    eng = DecodeEngine(model, page_size=PAGE, num_pages=per_seq * SLOTS + 2, max_batch=SLOTS, max_pages_per_seq=per_seq, max_prefill_rows=ROWS)

    def timed(fn):
        eng.synchronize()
        t0 = time.perf_counter()
        out = fn()
        eng.synchronize()
        return time.perf_counter() - t0, out

    result = {"tool": "tools/embedding_bench.py", "measured": True,
              "shape": {"texts": args.texts, "tokens": tokens, "min_len": args.min_len, "max_len": args.max_len, "layers": args.layers,
                        "slots": SLOTS, "max_prefill_rows": ROWS, "page_size": PAGE, "repeats": args.repeats},
              "unit": "median seconds of wall clock per run over all texts; tokens/s = tokens / seconds",
              "yardstick": "the same begin / pass / release sequence through prefill_packed with want_logits = 0, same process, same engine"}
    for pooling in ("last", "mean"):
        rec = Recorder(eng)
        _, vectors = timed(lambda: embed_ids(rec, texts, pooling=pooling))  # warm: first-use allocations; the log of its passes
        norms = np.linalg.norm(vectors.astype(np.float64), axis=1)
        assert vectors.shape == (args.texts, cfg["hidden_size"]) and np.allclose(norms, 1.0, atol=1e-4), (vectors.shape, norms.min(), norms.max())
        passes = [arg for op, arg in rec.log if op == "pass"]
        timed(lambda: replay(eng, rec.log))  # warm
        embed_s, yard_s = [], []
        for _ in range(args.repeats):  # interleaved: a drift of the clocks hits both alike
            embed_s.append(timed(lambda: embed_ids(eng, texts, pooling=pooling))[0])
            yard_s.append(timed(lambda: replay(eng, rec.log))[0])
        e, y = statistics.median(embed_s), statistics.median(yard_s)
        result[pooling] = {"passes": len(passes), "rows_per_pass_mean": round(tokens / len(passes), 1),
                           "sequences_per_pass_mean": round(sum(len(p) for p in passes) / len(passes), 2),
                           "embed_seconds": round(e, 4), "embed_seconds_all": [round(v, 4) for v in embed_s],
                           "yardstick_seconds": round(y, 4), "yardstick_seconds_all": [round(v, 4) for v in yard_s],
                           "embed_tokens_per_s": round(tokens / e, 1), "yardstick_tokens_per_s": round(tokens / y, 1),
                           "embed_vs_yardstick": round(y / e, 4), "added_share_of_embed_time": round(1.0 - y / e, 4)}
    assert eng.stats()["pages_in_use"] == 0
    eng.close()

    # the pooling launches alone: 16 sequences of 256 rows in a 4,096 x 2,560 chunk
    rows = torch.randn((ROWS, cfg["hidden_size"]), device="cuda").to(torch.bfloat16)
    seqs = [(i * (ROWS // SLOTS), ROWS // SLOTS) for i in range(SLOTS)]
    micro = {}
    for pooling in ("last", "mean"):
        sums = torch.zeros((SLOTS, cfg["hidden_size"]), dtype=torch.float32, device="cuda")
        times = []
        for i in range(12):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ext.pool_rows(rows, seqs, pooling=pooling, sums=sums if pooling == "mean" else None)
            b.record()
            b.synchronize()
            if i >= 2:
                times.append(a.elapsed_time(b) * 1e3)
        micro[pooling] = {"launches": 1 if pooling == "last" else 2, "us_median": round(statistics.median(times), 2), "us_min": round(min(times), 2)}
    result["pool_rows_4096x2560_16_sequences"] = micro
    for pooling in ("last", "mean"):
        per_pass = result[pooling]["embed_seconds"] / result[pooling]["passes"] * 1e6
        result[pooling]["pooling_launches_share_of_a_pass"] = round(micro[pooling]["us_median"] / per_pass, 5)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
