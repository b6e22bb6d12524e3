#!/usr/bin/env python3
"""Continuous-batching CLI over the fused engine (counterpart of the reference batch-main.py:62-101).

  python batch_main.py --model <checkpoint dir> [--batch-size 5] [--prefill-step 128] [--max-seq-len 512] [--prompts-file f] [--prefix-cache [PAGES]] [--swap-pages N]
                       [--draft-model <checkpoint dir> [--proposal-length 4]]
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

DEFAULT_PROMPTS = ["What is the capital of France?", "Where is New York City?", "Where is Tokyo?",
                   "What is the capital of China?", "Give me a short introduction to large language model."]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--batch-size", type=int, default=5)
    ap.add_argument("--prefill-step", type=int, default=128)
    ap.add_argument("--max-seq-len", type=int, default=512)
    ap.add_argument("--kv-format", default="bf16", choices=["bf16", "fp8"],
                    help="K / V pages as bfloat16 (the reference's cache) or FP8 E4M3 codes + power-of-two row scales (extension)")
    ap.add_argument("--enable-thinking", action="store_true")
    ap.add_argument("--raw-prompts", action="store_true", help="do not wrap the prompts in the chat template")
    ap.add_argument("--sampler-temp", type=float, default=0.0, help="0 = greedy; otherwise the device sampler per request")
    ap.add_argument("--sampler-top-p", type=float, default=None)
    ap.add_argument("--sampler-top-k", type=int, default=None)
    ap.add_argument("--sampler-seed", type=int, default=0, help="request i draws from seed + i")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, help="per request, on the device; over prompt and output (1 = off)")
    ap.add_argument("--presence-penalty", type=float, default=0.0, help="per request, on the device; over the output (0 = off)")
    ap.add_argument("--frequency-penalty", type=float, default=0.0, help="per request, on the device; times the count in the output (0 = off)")
    ap.add_argument("--dry-multiplier", type=float, default=0.0,
                    help="per request, on the device: DRY -- subtract multiplier * base ** (L - allowed_length) from the token that would "
                         "extend a verbatim repeat of L tokens (0 = off)")
    ap.add_argument("--dry-base", type=float, default=1.75, help="DRY's base (>= 1)")
    ap.add_argument("--dry-allowed-length", type=int, default=2, help="the longest repeat DRY leaves alone, plus one (>= 1)")
    ap.add_argument("--dry-range", type=int, default=0, help="DRY looks for repeats in the last N tokens (0 = all)")
    ap.add_argument("--dry-breaker", action="append", default=[], metavar="STRING",
                    help="a repeat never runs across the last token of STRING's encoding; repeatable (64)")
    ap.add_argument("--no-repeat-ngram", type=int, default=0, metavar="N",
                    help="per request, on the device: ban the token that would complete an N-gram the text already holds (0 = off, else 2 .. 64)")
    ap.add_argument("--sampler-min-p", type=float, default=0.0, help="per sampling request, on the device: keep tokens with p >= min_p * p_max (0 = off)")
    ap.add_argument("--sampler-typical-p", type=float, default=None, help="... locally typical sampling with this mass (1 = off)")
    ap.add_argument("--mirostat-tau", type=float, default=0.0,
                    help="... Mirostat v2 with this target surprise in bits (0 = off); excludes top-k, top-p, min-p and typical-p")
    ap.add_argument("--mirostat-eta", type=float, default=0.1, help="Mirostat's learning rate, in (0, 1]")
    constraint = ap.add_mutually_exclusive_group()
    constraint.add_argument("--regex", default=None, metavar="PATTERN",
                            help="every answer must match PATTERN in full (tiny_llm_hip.grammar's dialect), enforced on the device per request")
    constraint.add_argument("--json", default=None, choices=["object", "value"],
                            help="JSON mode: every answer is one JSON object (or any JSON value), enforced on the device per request")
    constraint.add_argument("--json-schema", default=None, metavar="FILE",
                            help="every answer is compact JSON that conforms to the schema in FILE (tiny_llm_hip.grammar.schema_regex)")
    ap.add_argument("--stop", action="append", default=[], metavar="STRING",
                    help="end an answer where its text holds STRING (matched on the device, across token boundaries); repeatable (16)")
    ap.add_argument("--stop-id", action="append", type=int, default=[], metavar="N", help="end an answer at token id N; repeatable")
    ap.add_argument("--prefix-cache", nargs="?", type=int, const=0, default=None, metavar="PAGES",
                    help="keep the K / V of finished requests and reuse it for later prompts that start with the same tokens (the chat "
                         "template, a shared system prompt); PAGES caps the retained pages (default: no cap)")
    ap.add_argument("--swap-pages", type=int, default=0, metavar="N",
                    help="room for N KV pages in pinned host memory: under page pressure the youngest request is preempted (its K / V "
                         "swapped out, or its prefill redone) instead of the run failing with 'KV page pool exhausted' (default 0: off)")
    ap.add_argument("--prompts-file", default=None, help="one prompt per line (default: five built-in questions)")
    ap.add_argument("--lora", action="append", default=[], metavar="DIR",
                    help="a LoRA adapter directory (PEFT or mlx_lm layout; tiny_llm_hip.lora) to keep resident beside the frozen weights; "
                         "repeat the flag for several adapters (up to 32), which then share decode steps")
    ap.add_argument("--lora-assign", default="round-robin", choices=["round-robin", "first"],
                    help="which request runs under which adapter: round-robin = request i under adapter i mod n; first = request 0 under "
                         "the first adapter, every other request on the base model")
    ap.add_argument("--draft-model", default=None, metavar="DIR",
                    help="greedy speculative decoding in batch: the checkpoint in DIR proposes for every request, the model verifies all of "
                         "them in one pass per round (tiny_llm_hip.engine.batch_speculative_generate_ids); the answers are the same ids")
    ap.add_argument("--proposal-length", type=int, default=4, help="tokens the draft model proposes per request and round (1 .. 7)")
    return ap


def check_draft_flags(ap: argparse.ArgumentParser, args, truncates: bool) -> None:
    """--draft-model verifies raw logits greedily, one adapter-free model: refuse every flag that would not apply."""
    if not args.draft_model:
        return
    clashes = [name for name, on in (
        ("--sampler-temp / --sampler-top-p / --sampler-top-k", bool(args.sampler_temp) or args.sampler_top_p is not None or args.sampler_top_k is not None),
        ("--sampler-min-p / --sampler-typical-p / --mirostat-tau", truncates),
        ("--repetition-penalty / --presence-penalty / --frequency-penalty",
         (args.repetition_penalty, args.presence_penalty, args.frequency_penalty) != (1.0, 0.0, 0.0)),
        ("--regex / --json / --json-schema", bool(args.regex or args.json or args.json_schema)),
        ("--stop / --stop-id", bool(args.stop or args.stop_id)),
        ("--lora", bool(args.lora)),
        ("--dry-multiplier / --dry-base / --dry-allowed-length / --dry-range / --dry-breaker / --no-repeat-ngram",
         args.dry_multiplier > 0 or args.no_repeat_ngram > 0),
    ) if on]
    if clashes:
        ap.error("--draft-model runs greedy speculative decoding over the raw logits of one model; it does not combine with " + ", ".join(clashes))
    if not 1 <= args.proposal_length <= 7:
        ap.error("--proposal-length must be between 1 and 7 (8 verification rows per request)")


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    from main import check_truncation_flags

    truncates = check_truncation_flags(ap, args)
    check_draft_flags(ap, args, truncates)

    from tiny_llm_hip import load
    from tiny_llm_hip.engine import DecodeEngine, batch_generate_ids, batch_speculative_generate_ids
    from main import chat_prompt

    model, tokenizer = load(args.model)
    prompts = [l for l in Path(args.prompts_file).read_text().splitlines() if l.strip()] if args.prompts_file else DEFAULT_PROMPTS
    encoded, limits = [], []
    for text in prompts:
        full = text if args.raw_prompts else chat_prompt(tokenizer, text, args.enable_thinking)
        ids = tokenizer.encode(full, add_special_tokens=False)
        if len(ids) >= args.max_seq_len:
            raise ValueError(f"prompt of {len(ids)} tokens exceeds max_seq_len {args.max_seq_len}")
        encoded.append(ids)
        limits.append(args.max_seq_len - len(ids))
    pages_per_seq = args.max_seq_len // 128 + 2
    engine = DecodeEngine(model, page_size=128, num_pages=pages_per_seq * (args.batch_size + 1) + 2,
                          max_batch=args.batch_size + 1, max_prefill_rows=args.prefill_step, kv_format=args.kv_format,
                          prefix_cache=False if args.prefix_cache is None else (args.prefix_cache or True), swap_pages=args.swap_pages)
    sampling = {}
    if args.sampler_temp:
        sampling.update(temperature=args.sampler_temp, top_k=args.sampler_top_k, top_p=args.sampler_top_p)
        if truncates:
            sampling.update(min_p=args.sampler_min_p, typical_p=args.sampler_typical_p, mirostat_tau=args.mirostat_tau, mirostat_eta=args.mirostat_eta)
    if (args.repetition_penalty, args.presence_penalty, args.frequency_penalty) != (1.0, 0.0, 0.0):
        sampling.update(repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty,
                        frequency_penalty=args.frequency_penalty)
    from main import dry_settings

    sampling.update(dry_settings(args, tokenizer))
    stops = {tokenizer.eos_token_id}
    try:
        from tiny_llm_hip.grammar import cli_grammar
        from tiny_llm_hip.lora import assign_adapters

        if args.lora:
            sampling["lora"] = assign_adapters(len(encoded), [engine.load_lora(d) for d in args.lora], args.lora_assign)

        grammar = cli_grammar(engine, tokenizer, args.regex, args.json, args.json_schema)
        if grammar is not None:
            sampling["grammar"] = grammar
            stops |= set(grammar.eos_ids)
        from tiny_llm_hip.stop import cli_stop_set, cut_text

        stop, token_bytes = cli_stop_set(engine, tokenizer, args.stop, args.stop_id, sorted(i for i in stops if i is not None))
        stops |= set(args.stop_id)
        if args.draft_model:
            draft_model, draft_tok = load(args.draft_model)
            if draft_tok.get_vocab() != tokenizer.get_vocab():
                raise ValueError("draft and target tokenizers use different token ids")
            draft = DecodeEngine(draft_model, page_size=128, num_pages=pages_per_seq * (args.batch_size + 1) + 2,
                                 max_batch=args.batch_size + 1, max_prefill_rows=args.prefill_step)
            try:
                answers = batch_speculative_generate_ids(engine, draft, encoded, limits, proposal_length=args.proposal_length,
                                                         eos_token_id=tokenizer.eos_token_id)
            finally:
                draft.close()
            done = list(enumerate(answers))
        elif stop is not None:  # the device ends every request: at a stop string, a stop id (the EOS ids among them) or its budget
            done = batch_generate_ids(engine, encoded, limits, batch_size=args.batch_size, prefill_step=args.prefill_step,
                                      sampling=sampling or None, base_seed=args.sampler_seed, stop=stop)
        else:
            done = batch_generate_ids(engine, encoded, limits, batch_size=args.batch_size, prefill_step=args.prefill_step,
                                      eos_token_id=tokenizer.eos_token_id, sampling=sampling or None, base_seed=args.sampler_seed)
    finally:
        engine.close()
    results = []
    for idx, ids in done:
        if ids and ids[-1] in stops:
            ids = ids[:-1]
        text = cut_text(ids, token_bytes, args.stop) if args.stop else tokenizer.decode(ids)
        results.append((idx, text))
        print(f"--- {idx} ---\nQ: {prompts[idx]}\nA: {text}")
    return results


if __name__ == "__main__":
    main()
