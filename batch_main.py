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


from tiny_llm_hip import request  # noqa: E402


def build_parser() -> argparse.ArgumentParser:
    """The request flags come from tiny_llm_hip.request's table (shared with main.py) and hold per request; the rest are this script's own."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--batch-size", type=int, default=5)
    ap.add_argument("--prefill-step", type=int, default=128)
    ap.add_argument("--max-seq-len", type=int, default=512)
    ap.add_argument("--kv-format", default="bf16", choices=["bf16", "fp8"],
                    help="K / V pages as bfloat16 (the reference's cache) or FP8 E4M3 codes + power-of-two row scales (extension)")
    ap.add_argument("--enable-thinking", action="store_true")
    ap.add_argument("--raw-prompts", action="store_true", help="do not wrap the prompts in the chat template")
    request.add_request_flags(ap, "batch_main")
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
    flags = request.switched(args)
    clashes = [name for name, on in (
        ("--sampler-temp / --sampler-top-p / --sampler-top-k", bool(flags.given & {"--sampler-temp", "--sampler-top-p", "--sampler-top-k"})),
        ("--sampler-min-p / --sampler-typical-p / --mirostat-tau", truncates),
        ("--repetition-penalty / --presence-penalty / --frequency-penalty", "penalties" in flags.groups),
        ("--regex / --json / --json-schema", "grammar" in flags.groups),
        ("--stop / --stop-id", "stop" in flags.groups),
        ("--lora", bool(args.lora)),
        ("--dry-multiplier / --dry-base / --dry-allowed-length / --dry-range / --dry-breaker / --no-repeat-ngram", "dry" in flags.groups),
    ) if on]
    if clashes:
        ap.error("--draft-model runs greedy speculative decoding over the raw logits of one model; it does not combine with " + ", ".join(clashes))
    if not 1 <= args.proposal_length <= 7:
        ap.error("--proposal-length must be between 1 and 7 (8 verification rows per request)")


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    truncates = request.check_truncation_flags(ap, args)
    check_draft_flags(ap, args, truncates)

    from tiny_llm_hip import load
    from tiny_llm_hip.engine import DecodeEngine, batch_generate_ids, batch_speculative_generate_ids

    model, tokenizer = load(args.model)
    prompts = [l for l in Path(args.prompts_file).read_text().splitlines() if l.strip()] if args.prompts_file else DEFAULT_PROMPTS
    encoded, limits = [], []
    for text in prompts:
        full = text if args.raw_prompts else request.chat_prompt(tokenizer, text, args.enable_thinking)
        ids = tokenizer.encode(full, add_special_tokens=False)
        if len(ids) >= args.max_seq_len:
            raise ValueError(f"prompt of {len(ids)} tokens exceeds max_seq_len {args.max_seq_len}")
        encoded.append(ids)
        limits.append(args.max_seq_len - len(ids))
    pages_per_seq = args.max_seq_len // 128 + 2
    engine = DecodeEngine(model, page_size=128, num_pages=pages_per_seq * (args.batch_size + 1) + 2,
                          max_batch=args.batch_size + 1, max_prefill_rows=args.prefill_step, kv_format=args.kv_format,
                          prefix_cache=False if args.prefix_cache is None else (args.prefix_cache or True), swap_pages=args.swap_pages)
    sampling = request.sampling_dict(args, tokenizer, request.switched(args).groups)
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
