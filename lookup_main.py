#!/usr/bin/env python3
"""Generation with prompt-lookup speculative decoding: no draft model, the proposals come from the sequence itself.

  python lookup_main.py <checkpoint dir> [PROMPT ...] [--prompts-file f] [--proposal-length 4] [--max-ngram 3] [--min-ngram 1]
                        [--max-seq-len 512] [--raw-prompts] [--sampler-temp T] [--sampler-top-k K] [--sampler-top-p P] [--sampler-seed S]

Every round the engine looks, on the device, for the last --max-ngram .. --min-ngram ids of each sequence earlier in that sequence
(prompt included) and proposes the up to --proposal-length ids that followed; one batched verification pass accepts what the model
itself would have produced (tiny_llm_hip.engine.lookup_generate_ids).  The answers are the model's greedy answers; what changes is the
number of passes, which the last line reports.  Prompts that are quoted, edited or summarised in the answer gain the most.
With --sampler-temp above 0 the requests sample on the device (main.py's flags; request i draws from --sampler-seed + i) and the
proposals are verified by speculative sampling: the answers are distributed exactly as the sampler's own, only the passes change.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

DEFAULT_PROMPTS = ["Repeat this sentence three times, word for word: the quick brown fox jumps over the lazy dog."]


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("model", help="checkpoint directory")
    ap.add_argument("prompts", nargs="*", help="the prompts (default: --prompts-file, or one built-in prompt)")
    ap.add_argument("--prompts-file", default=None, help="one prompt per line, in addition to the positional ones")
    ap.add_argument("--proposal-length", type=int, default=4, help="ids proposed per sequence and round (1 .. 7)")
    ap.add_argument("--max-ngram", type=int, default=3, help="the longest match looked for (1 .. 16)")
    ap.add_argument("--min-ngram", type=int, default=1, help="the shortest match that yields a proposal (1 .. --max-ngram)")
    ap.add_argument("--max-seq-len", type=int, default=512, help="prompt plus answer, in tokens")
    ap.add_argument("--prefill-step", type=int, default=128)
    ap.add_argument("--kv-format", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--enable-thinking", action="store_true")
    ap.add_argument("--raw-prompts", action="store_true", help="do not wrap the prompts in the chat template")
    ap.add_argument("--sampler-temp", type=float, default=0.0, help="0 = greedy; else sample on the device, proposals verified by speculative sampling")
    ap.add_argument("--sampler-top-k", type=int, default=None, help="sample among the K most likely tokens")
    ap.add_argument("--sampler-top-p", type=float, default=None, help="sample among the likeliest tokens whose mass reaches this")
    ap.add_argument("--sampler-seed", type=int, default=0, help="the device's seed: request i draws from seed + i")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not 1 <= args.proposal_length <= 7:
        ap.error("--proposal-length must be between 1 and 7 (8 verification rows per request)")
    if not 1 <= args.max_ngram <= 16:
        ap.error("--max-ngram must be between 1 and 16")
    if not 1 <= args.min_ngram <= args.max_ngram:
        ap.error("--min-ngram must be between 1 and --max-ngram")
    if args.sampler_temp < 0.0:
        ap.error("--sampler-temp must be >= 0")

    from tiny_llm_hip import load, request
    from tiny_llm_hip.engine import DecodeEngine, lookup_generate_ids

    model, tokenizer = load(args.model)
    prompts = list(args.prompts)
    if args.prompts_file:
        prompts += [l for l in Path(args.prompts_file).read_text().splitlines() if l.strip()]
    prompts = prompts or DEFAULT_PROMPTS
    encoded, limits = [], []
    for text in prompts:
        full = text if args.raw_prompts else request.chat_prompt(tokenizer, text, args.enable_thinking)
        ids = tokenizer.encode(full, add_special_tokens=False)
        if len(ids) >= args.max_seq_len:
            raise ValueError(f"prompt of {len(ids)} tokens exceeds max_seq_len {args.max_seq_len}")
        encoded.append(ids)
        limits.append(args.max_seq_len - len(ids))
    wave = min(len(encoded), 64 // (args.proposal_length + 1))
    pages_per_seq = args.max_seq_len // 128 + 2
    engine = DecodeEngine(model, page_size=128, num_pages=pages_per_seq * wave + 2, max_batch=wave, max_pages_per_seq=pages_per_seq,
                          max_prefill_rows=args.prefill_step, kv_format=args.kv_format)
    stats = {}
    sampled = {}
    if args.sampler_temp > 0.0:
        sampled = {"sampling": {"temperature": args.sampler_temp, "top_k": args.sampler_top_k, "top_p": args.sampler_top_p},
                   "base_seed": args.sampler_seed}
    try:
        answers = lookup_generate_ids(engine, encoded, limits, proposal_length=args.proposal_length, max_ngram=args.max_ngram,
                                      min_ngram=args.min_ngram, eos_token_id=tokenizer.eos_token_id, stats=stats, **sampled)
    finally:
        engine.close()
    results = []
    for idx, ids in enumerate(answers):
        text = tokenizer.decode(ids)
        results.append((idx, text))
        print(f"--- {idx} ---\nQ: {prompts[idx]}\nA: {text}")
    stats["tokens"] = sum(len(a) for a in answers)
    print(json.dumps(stats))
    return results


if __name__ == "__main__":
    main()
