#!/usr/bin/env python3
"""Single-prompt generation CLI over the HIP path (counterpart of the reference main.py:9-190; same flag names where the
feature exists here).

  python main.py --model <checkpoint dir or cached repo> --prompt "..." [--solution engine|ops] [--draft-model <dir>]

--solution engine  fused decode engine (tl_engine_*): greedy, or speculative with --draft-model (speculative sampling with a nonzero
                   --sampler-temp: the answer is distributed as the model's own samples), or beam search with --num-beams
--solution ops     the op-by-op Week-3 model on the HIP operators (reference call structure); supports the sampler flags
Checkpoints are MLX-format 4-bit directories (tiny_llm_hip.load); there is no network, so --model must exist locally.
"""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent
for p in (ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))


from tiny_llm_hip import request  # noqa: E402
from tiny_llm_hip.request import chat_prompt, check_truncation_flags, dry_settings  # noqa: E402,F401  (dry_settings: the --dry-* flags as sampling keys)


def build_parser() -> argparse.ArgumentParser:
    """The request flags come from tiny_llm_hip.request's table (shared with batch_main.py); the rest are this script's own.  A request
    flag that exists on the device only applies with --solution engine."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", required=True)
    ap.add_argument("--draft-model", default=None)
    ap.add_argument("--prompt", default="Give me a short introduction to large language model.")
    ap.add_argument("--solution", default="engine", choices=["engine", "ops"])
    request.add_request_flags(ap, "main")
    ap.add_argument("--enable-thinking", action="store_true")
    ap.add_argument("--raw-prompt", action="store_true", help="do not wrap the prompt in the chat template")
    ap.add_argument("--max-new-tokens", type=int, default=256)
    ap.add_argument("--logprobs", type=int, default=None, metavar="N",
                    help="with --solution engine (greedy or device sampling): print each generated token with its log-probability "
                         "and its N (0-20) most likely alternatives")
    ap.add_argument("--proposal-length", type=int, default=4)
    ap.add_argument("--num-beams", type=int, default=None, metavar="N",
                    help="with --solution engine: beam search over N (1-8) beams, candidates ranked on the device; prints the best "
                         "hypothesis.  Excludes the sampler, penalty, grammar, --stop, --logprobs, --lora and draft options (--stop-id ids count "
                         "as EOS ids)")
    ap.add_argument("--length-penalty", type=float, default=1.0,
                    help="with --num-beams: a hypothesis scores sum of log-probabilities / length ** this")
    ap.add_argument("--early-stopping", action="store_true", help="with --num-beams: stop as soon as N hypotheses have finished")
    ap.add_argument("--lora", default=None, metavar="DIR",
                    help="with --solution engine: run the request under the LoRA adapter in DIR (a PEFT or an mlx_lm adapter directory; "
                         "tiny_llm_hip.lora), applied on the device beside the frozen weights")
    return ap


def check_beam_flags(ap, args) -> None:
    """--num-beams runs plain greedy slots (tl_engine_beam_select refuses any other): what it excludes is an error before anything is loaded."""
    if args.num_beams is None:
        if args.length_penalty != 1.0 or args.early_stopping:
            ap.error("--length-penalty and --early-stopping apply with --num-beams only")
        return
    if not 1 <= args.num_beams <= 8:
        ap.error("--num-beams must be 1 .. 8")
    if (2 + len(set(args.stop_id))) * args.num_beams > 32:
        ap.error("--num-beams: (1 + number of EOS ids) * beams must not exceed 32 (the EOS id and every --stop-id count)")
    flags = request.switched(args)
    sampler = {f.option for s in request.SETTINGS if s.group in ("sampling", "truncation") for f in s.flags}
    excluded = {
        "--solution ops": args.solution != "engine",
        "--draft-model": args.draft_model is not None,
        "the sampler options": bool(flags.given & sampler),
        "the penalty options": "penalties" in flags.groups,
        "--regex / --json / --json-schema": "grammar" in flags.groups,
        "--stop": "--stop" in flags.given,
        "--logprobs": args.logprobs is not None,
        "--lora": args.lora is not None,
        "the DRY / --no-repeat-ngram options": "dry" in flags.groups,
    }
    clash = [name for name, on in excluded.items() if on]
    if clash:
        ap.error("--num-beams cannot be combined with " + ", ".join(clash) + ": beam slots are plain greedy slots")


def main(argv=None) -> str:
    ap = build_parser()
    args = ap.parse_args(argv)
    check_truncation_flags(ap, args)
    check_beam_flags(ap, args)
    on = request.switched(args).groups
    from tiny_llm_hip import load

    model, tokenizer = load(args.model)
    prompt = args.prompt if args.raw_prompt else chat_prompt(tokenizer, args.prompt, args.enable_thinking)
    if args.solution == "ops":
        from tiny_llm_hip import Qwen3ModelWeek3, make_sampler, simple_generate_with_kv_cache, speculative_generate

        net = Qwen3ModelWeek3(model)
        if args.draft_model:
            draft, draft_tok = load(args.draft_model)
            return speculative_generate(Qwen3ModelWeek3(draft), net, draft_tok, tokenizer, prompt,
                                        proposal_length=args.proposal_length)
        if on & {"penalties", "grammar"}:
            print("note: the penalty flags, --regex, --json and --json-schema apply to --solution engine only")
        if "dry" in on:
            print("note: the --dry-* flags and --no-repeat-ngram apply to --solution engine only")
        if args.sampler_temp:
            print("note: the KV-cache loop is greedy like the reference's; sampler flags apply to --solution engine only")
        _ = make_sampler  # sampler surface kept importable for callers of the library
        return simple_generate_with_kv_cache(net, tokenizer, prompt, max_new_tokens=args.max_new_tokens)

    from tiny_llm_hip.engine import DecodeEngine, speculative_generate_ids

    ids = tokenizer.encode(prompt, add_special_tokens=False)
    pages = (len(ids) + args.max_new_tokens) // 128 + 2
    if args.num_beams is not None:
        return beam_search_with_engine(model, tokenizer, ids, pages, args)
    engine = DecodeEngine(model, page_size=128, num_pages=pages, max_batch=1, max_prefill_rows=4096)
    eos = tokenizer.eos_token_id
    records = grammar = lora = stop = token_bytes = None
    try:
        if args.lora:
            if args.draft_model:
                print("note: --lora does not apply with a draft model")
            else:
                lora = engine.load_lora(args.lora)
        if not args.draft_model:
            from tiny_llm_hip.grammar import cli_grammar

            grammar = cli_grammar(engine, tokenizer, args.regex, args.json, args.json_schema)
            from tiny_llm_hip.stop import cli_stop_set

            # (the EOS ids join the set: the device ends the request at whichever comes first)
            stop, token_bytes = cli_stop_set(engine, tokenizer, args.stop, args.stop_id, [eos, *(grammar.eos_ids if grammar is not None else ())])
        elif "stop" in on:
            print("note: --stop and --stop-id do not apply with a draft model")
        if args.draft_model:
            draft_model, draft_tok = load(args.draft_model)
            if draft_tok.get_vocab() != tokenizer.get_vocab():
                raise ValueError("draft and target tokenizers use different token ids")
            if on & {"penalties", "grammar"}:
                print("note: speculative decoding verifies the raw logits; the penalty flags, --regex, --json and --json-schema do not "
                      "apply with a draft model")
            if "dry" in on:
                print("note: speculative decoding verifies the raw logits; the --dry-* flags and --no-repeat-ngram do not apply with a draft model")
            if "truncation" in on:
                print("note: speculative sampling verifies under temperature, top-k and top-p; --sampler-min-p, --sampler-typical-p and "
                      "--mirostat-tau do not apply with a draft model")
            if args.sampler_temp and args.sampler_seed is None:
                print("note: a draft model with a nonzero --sampler-temp selects the device sampler; no --sampler-seed given: seed 0")
            draft = DecodeEngine(draft_model, page_size=128, num_pages=pages, max_batch=1, max_prefill_rows=4096)
            try:
                # --sampler-temp 0: greedy speculative decoding; > 0: speculative sampling, both engines drawing on the device
                out = speculative_generate_ids(engine, draft, ids, args.max_new_tokens,
                                               proposal_length=min(args.proposal_length, 7), eos_token_id=eos,
                                               temperature=args.sampler_temp, top_k=args.sampler_top_k, top_p=args.sampler_top_p,
                                               seed=args.sampler_seed or 0)
            finally:
                draft.close()
        elif args.sampler_temp and not (args.sampler_seed is not None or lora is not None or grammar is not None or stop is not None
                                        or on & {"penalties", "truncation", "dry"}):
            out = sample_with_engine(engine, ids, args, eos)
        else:
            # greedy, or the per-slot sampler on the device (the whole generation in one prefill + one decode(N) call), which every flag
            # that exists on the device only selects: the penalties, the grammar, min-p, typical-p, Mirostat, DRY, the stop set, the adapter
            if args.sampler_temp and args.sampler_seed is None:
                print("note: the penalty, truncation and Mirostat flags and --regex select the device sampler; no --sampler-seed given: seed 0")
            # (a sampling request hands the truncation flags over at neutral values too: one that is out of range is refused, not ignored)
            out = engine.generate(ids, args.max_new_tokens, seed=args.sampler_seed or 0, logprobs=args.logprobs, grammar=grammar, lora=lora, stop=stop,
                                  **request.sampling_dict(args, tokenizer, on | {"truncation"}))
            if args.logprobs is not None:
                out, records = out
            out = cut_at_eos(out, eos, grammar)
        ended = engine.last_stop_state if stop is not None else None
    finally:
        engine.close()
    if records is not None:
        for t, r in zip(out, records):
            alts = " ".join(f"{tokenizer.decode([i])!r}:{v:.4f}" for i, v in r.top)
            print(f"{tokenizer.decode([t])!r}\t{r.logprob:.4f}\t{alts}")
    elif args.logprobs is not None:
        print("note: --logprobs applies to the engine's greedy decode and its device sampler (--sampler-seed) only")
    if ended is not None and ended.reason == "string":  # the text up to the matched string, as the device counted it
        from tiny_llm_hip.stop import cut_text

        text = cut_text(out, token_bytes, cut_bytes=ended.cut_bytes)
    else:
        text = tokenizer.decode(out[:-1] if ended is not None and ended.reason == "id" and out and out[-1] in args.stop_id else out)
    print(text)
    return text


def beam_search_with_engine(model, tokenizer, ids, pages, args) -> str:
    """--num-beams: the best hypothesis of tiny_llm_hip.beam.beam_search_ids (every beam may hold a tail and fresh pages of its own)."""
    from tiny_llm_hip.beam import beam_search_ids
    from tiny_llm_hip.engine import DecodeEngine

    eos = sorted({tokenizer.eos_token_id, *args.stop_id})
    engine = DecodeEngine(model, page_size=128, num_pages=pages * args.num_beams, max_batch=args.num_beams, max_prefill_rows=4096)
    try:
        best, score = beam_search_ids(engine, ids, args.num_beams, args.max_new_tokens, eos_ids=eos, length_penalty=args.length_penalty,
                                      early_stopping=args.early_stopping)[0]
    finally:
        engine.close()
    text = tokenizer.decode(best[:-1] if best and best[-1] in eos else best)
    print(text)
    return text


def cut_at_eos(out, eos, grammar=None):
    """The ids before the first EOS id: the tokenizer's, or any of the grammar's."""
    stops = set(grammar.eos_ids) if grammar is not None else set()
    stops.add(eos)
    cut = next((k for k, t in enumerate(out) if t in stops), len(out))
    return out[:cut]


def sample_with_engine(engine, ids, args, eos):
    """Temperature / top-k / top-p sampling: logits come from the engine, the sampler (tiny_llm_hip.make_sampler, reference
    sampler.py:5-25) runs on them, the sampled id is fed back with set_token."""
    import torch
    from tiny_llm_hip import make_sampler

    sample = make_sampler(args.sampler_temp, top_p=args.sampler_top_p, top_k=args.sampler_top_k)
    out = []
    engine.begin(0)
    try:
        engine.prefill(0, ids)
        for _ in range(args.max_new_tokens):
            logits = engine.logits(1).float()
            token = int(sample(logits - torch.logsumexp(logits, dim=-1, keepdim=True))[0])
            if token == eos:
                break
            out.append(token)
            engine.set_token(0, token)
            engine.decode(1, batch=1)
    finally:
        engine.release(0)
    return out


if __name__ == "__main__":
    main()
