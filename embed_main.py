#!/usr/bin/env python3
"""Text-embedding CLI over the fused engine: one text per line in, one vector per line out.

  python embed_main.py --model <checkpoint dir> --texts-file f [--pooling last|mean] [--dim N] [--no-normalize]
                       [--instruct TASK] [--prefix-cache [PAGES]] [--similarity]

Every text is tokenised, ended with the tokenizer's <|endoftext|> id (what Qwen3-Embedding models pool on) and embedded through
tiny_llm_hip.embedding.embed_ids: the model's final-norm rows, pooled ("last": the last token's row), cut to --dim components and
L2-normalised.  --instruct TASK wraps every text as a query, "Instruct: TASK\\nQuery:text" (documents are embedded bare: run them
without it).  Output: one JSON object per line {"index", "tokens", "embedding"}, or with --similarity the cosine-similarity matrix
of the texts, one row per line.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


def cosine_matrix(vectors):
    """[n, n] cosine similarities of the rows of ``vectors`` in float64 (a zero row is similar to nothing: 0)."""
    import numpy as np

    v = np.asarray(vectors, dtype=np.float64)
    norms = np.linalg.norm(v, axis=1, keepdims=True)
    unit = np.divide(v, norms, out=np.zeros_like(v), where=norms > 0)
    return unit @ unit.T


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--texts-file", required=True, help="one text per line (empty lines are skipped)")
    ap.add_argument("--pooling", default="last", choices=["last", "mean"])
    ap.add_argument("--dim", type=int, default=None, help="keep the first DIM components (default: the hidden size)")
    ap.add_argument("--no-normalize", action="store_true", help="leave the pooled vector as it is (default: divide by its Euclidean norm)")
    ap.add_argument("--instruct", default=None, metavar="TASK", help="embed every text as a query of the Qwen3-Embedding instruction format")
    ap.add_argument("--prefix-cache", nargs="?", type=int, const=0, default=None, metavar="PAGES",
                    help="reuse the K / V of a shared prefix (the instruction) across texts; last-token pooling only; PAGES caps the retained pages")
    ap.add_argument("--similarity", action="store_true", help="print the cosine-similarity matrix instead of the vectors")
    ap.add_argument("--kv-format", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--max-seq-len", type=int, default=8192, help="longest text in tokens")
    ap.add_argument("--prefill-rows", type=int, default=4096, help="tokens per pass (max_prefill_rows)")
    ap.add_argument("--batch-size", type=int, default=16, help="texts per pass, at most 16")
    args = ap.parse_args(argv)
    if not 1 <= args.batch_size <= 16:
        ap.error("--batch-size must be 1 .. 16")

    from tiny_llm_hip import load
    from tiny_llm_hip.embedding import embed_ids, text_ids
    from tiny_llm_hip.engine import DecodeEngine

    model, tokenizer = load(args.model)
    texts = [l for l in Path(args.texts_file).read_text().splitlines() if l.strip()]
    encoded = [text_ids(tokenizer, t, task=args.instruct) for t in texts]
    longest = max((len(ids) for ids in encoded), default=0)
    if longest > args.max_seq_len:
        raise ValueError(f"a text of {longest} tokens exceeds max_seq_len {args.max_seq_len}")
    pages_per_seq = -(-max(longest, 1) // 128)
    cache_pages = 0 if args.prefix_cache is None else (args.prefix_cache or pages_per_seq)
    engine = DecodeEngine(model, page_size=128, num_pages=pages_per_seq * args.batch_size + cache_pages + 1, max_batch=args.batch_size,
                          max_pages_per_seq=pages_per_seq, max_prefill_rows=args.prefill_rows, kv_format=args.kv_format,
                          prefix_cache=False if args.prefix_cache is None else (args.prefix_cache or True))
    try:
        vectors = embed_ids(engine, encoded, pooling=args.pooling, normalize=not args.no_normalize, dim=args.dim)
    finally:
        engine.close()
    if args.similarity:
        for row in cosine_matrix(vectors):
            print(" ".join(f"{x:.4f}" for x in row))
    else:
        for i, (ids, v) in enumerate(zip(encoded, vectors)):
            print(json.dumps({"index": i, "tokens": len(ids), "embedding": [float(x) for x in v]}))
    return vectors


if __name__ == "__main__":
    main()
