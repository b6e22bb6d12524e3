"""The scenarios behind tests/golden/request_cli.json (tests/test_request_cli_cpu.py): what main.py and batch_main.py make of their
command lines, and what request_settings makes of a ``sampling`` argument.

Nothing here touches a device.  ``tiny_llm_hip.load`` hands out a named stand-in model and a word-level tokenizer, ``cli_grammar`` and
``cli_stop_set`` hand out scheduler_recorder's fake grammar and stop set (named after their arguments), and ``DecodeEngine`` is
``CliEngine``: scheduler_recorder's RecordingEngine behind the real constructor's keywords.  The real ``DecodeEngine.generate``,
``batch_generate_ids``, ``request_settings`` and ``RequestSettings.apply`` run over it, so a scenario's engine log holds every setter
the command line led to, with its values.  The other entry points a script can hand a request to -- ``speculative_generate_ids``,
``batch_speculative_generate_ids``, ``beam_search_ids`` and the op-by-op model's two loops -- are recorded with their arguments.

``record()`` returns {"parsers", "pool", "main", "batch_main", "settings", "generate"} in JSON's value types.  tests/golden/make_request_cli.py wrote the fixture from
it at the commit named in the file; the test runs it through the code under test and compares.
"""

from __future__ import annotations

import contextlib
import hashlib
import io
import json
from pathlib import Path
from types import SimpleNamespace
from unittest import mock

from scheduler_recorder import VOCAB, RecordingEngine, fake_grammar, fake_stop_set, plain

EOS = 2
PROMPTS = str(Path(__file__).parent / "golden" / "request_cli_prompts.txt")  # three short prompts: batch_main's logs stay short


def digest(x) -> str:
    """What stands in the fixture for a value too long to keep: its length and a hash of its JSON text."""
    text = json.dumps(x)
    return f"{len(text)}:{hashlib.sha256(text.encode()).hexdigest()[:16]}"


def engine_log(calls: list) -> list:
    """An engine's call log as the fixture keeps it: every settings call with its values, and the digest of the whole log."""
    return [[c for c in calls if c[0].startswith("set_") or c[0] == "load_lora"], digest(calls)]


class WordTokenizer:
    """One token per whitespace-separated word; its id follows from the word's bytes."""
    eos_token_id, name = EOS, "tokenizer"

    def encode(self, text, add_special_tokens=False):
        return [10 + sum(w.encode()) % 900 for w in text.split()]

    def decode(self, ids):
        return " ".join(f"t{int(i)}" for i in ids)

    def apply_chat_template(self, messages, tokenize=False, add_generation_prompt=True, enable_thinking=False):
        return "chat " + messages[-1]["content"] + (" think" if enable_thinking else "")

    def get_vocab(self):
        return {"word": 10}


class _Always(dict):
    """RecordingEngine.stop_at for "every armed request's stop set matches at its n-th token"."""

    def __init__(self, n):
        super().__init__()
        self.n = n

    def get(self, key, default=None):
        return self.n


class Session:
    """One run of a script's ``main``: the entry points it reached, in order, and the engines it built."""

    def __init__(self, stop_at=None):
        self.entries: list = []
        self.engines: list = []
        self.stop_at = stop_at
        self.tokenizer = WordTokenizer()

    def entry(self, name, *args, **kwargs):
        self.entries.append([name, plain(args), plain(kwargs)])

    def recorded(self, name, result):
        def call(*args, **kwargs):
            self.entry(name, *args, **kwargs)
            return result(*args, **kwargs) if callable(result) else result
        return call

    def engine_class(self):
        from tiny_llm_hip.engine import DecodeEngine, TokenLogprob

        session = self

        class CliEngine(RecordingEngine):
            def __init__(self, model, **kw):
                super().__init__(kw["max_batch"])
                if session.stop_at is not None:
                    self.stop_at = _Always(session.stop_at)
                self.name = f"engine{len(session.engines)}:{model.name}"
                session.entry("DecodeEngine", model, **kw)
                session.engines.append(self)
                self.loras = 0

            def generate(self, *args, **kw):  # (the keywords are the script's own business: what they lead to is in the log)
                session.entries.append(["generate"])
                return DecodeEngine.generate(self, *args, **kw)

            def load_lora(self, adapter):
                self.loras += 1
                self._log("load_lora", adapter, result=self.loras - 1)
                return self.loras - 1

            def close(self):
                self._log("close")

            def set_token(self, slot, token):
                self._log("set_token", slot, int(token))

            def read_logprobs(self, slot, count):
                out = [TokenLogprob(-0.5, [(t, -0.5), (t + 1, -1.5)]) for t in self._ids(slot, count)]
                self._log("read_logprobs", slot, count, result=out)
                return out

            def logits(self, rows=1):  # one id holds all the mass: the host sampler's draw does not depend on its random stream
                import torch

                self._log("logits", rows)
                out = torch.full((rows, VOCAB), -1.0e9)
                out[:, 5 + len([c for c in self.calls if c[0] == "logits"])] = 0.0
                return out

        return CliEngine

    def patches(self):
        def load(path):
            return SimpleNamespace(name=f"model:{path}"), self.tokenizer

        def grammar(engine, tokenizer, regex=None, json_top=None, json_schema_file=None):
            given = [f"{k}={v}" for k, v in (("regex", regex), ("json", json_top), ("schema", json_schema_file)) if v]
            return fake_grammar("grammar:" + ",".join(given), [7]) if given else None

        def stop_set(engine, tokenizer, strings=(), ids=(), also_ids=()):
            if not strings and not ids:
                return None, None
            return fake_stop_set(f"stop:{list(strings)}:{list(ids)}:{list(also_ids)}"), [f"t{i} ".encode() for i in range(VOCAB)]

        def batch_speculative(target, draft, prompts, limits, **kw):
            return [[30 + i, 40 + i, EOS] for i in range(len(prompts))]

        import tiny_llm_hip.engine as engine_mod

        real_batch = engine_mod.batch_generate_ids

        def batch_generate(*args, **kw):
            self.entries.append(["batch_generate_ids"])
            return real_batch(*args, **kw)

        return [
            mock.patch("tiny_llm_hip.load", load),
            mock.patch("tiny_llm_hip.grammar.cli_grammar", grammar),
            mock.patch("tiny_llm_hip.stop.cli_stop_set", stop_set),
            mock.patch("tiny_llm_hip.engine.DecodeEngine", self.engine_class()),
            mock.patch("tiny_llm_hip.engine.batch_generate_ids", batch_generate),
            mock.patch("tiny_llm_hip.engine.speculative_generate_ids", self.recorded("speculative_generate_ids", [11, 12, 13])),
            mock.patch("tiny_llm_hip.engine.batch_speculative_generate_ids", self.recorded("batch_speculative_generate_ids", batch_speculative)),
            mock.patch("tiny_llm_hip.beam.beam_search_ids", self.recorded("beam_search_ids", [([21, 22, 9], -1.5)])),
            mock.patch("tiny_llm_hip.Qwen3ModelWeek3", lambda model: SimpleNamespace(name=f"week3:{model.name}")),
            mock.patch("tiny_llm_hip.simple_generate_with_kv_cache", self.recorded("simple_generate_with_kv_cache", "kv-cache text")),
            mock.patch("tiny_llm_hip.speculative_generate", self.recorded("speculative_generate", "speculative text")),
        ]


def run_cli(script: str, argv: list, stop_at=None) -> dict:
    """``script``.main(argv) under the stand-ins: {"error"} for a refused command line or a raised error, else the entry points reached
    with their arguments, every engine's log (engine_log), the ``note:`` lines and everything else printed, and the returned value's digest."""
    import importlib

    module = importlib.import_module(script)
    session = Session(stop_at)
    out, err = io.StringIO(), io.StringIO()
    result, error = None, None
    with contextlib.ExitStack() as stack:
        for p in session.patches():
            stack.enter_context(p)
        stack.enter_context(contextlib.redirect_stdout(out))
        stack.enter_context(contextlib.redirect_stderr(err))
        try:
            result = module.main(list(argv))
        except SystemExit:  # ap.error: usage (which names the program), then "<program>: error: <text>"
            error = "ap.error: " + err.getvalue().split(": error: ", 1)[1].strip()
        except (ValueError, RuntimeError, TypeError) as exc:
            error = f"{type(exc).__name__}: {exc}"
    lines = out.getvalue().splitlines()
    done = {"error": error, "entries": session.entries, "engines": [[e.name, *engine_log(e.calls)] for e in session.engines],
            "notes": [l for l in lines if l.startswith("note:")], "printed": [l for l in lines if not l.startswith("note:")], "result": digest(plain(result))}
    return json.loads(json.dumps({"error": error} if error is not None and error.startswith("ap.error") else done))


def parser_surface(script: str) -> dict:
    """Every option of ``script``.build_parser() but --help, by its first option string; help texts are left out."""
    import importlib

    parser = importlib.import_module(script).build_parser()
    exclusive = {}
    for group in parser._mutually_exclusive_groups:
        members = sorted(a.option_strings[0] for a in group._group_actions)
        for a in group._group_actions:
            exclusive[a.option_strings[0]] = members
    out = {}
    for a in parser._actions:
        if a.dest == "help":
            continue
        every = {"options": list(a.option_strings), "dest": a.dest, "type": getattr(a.type, "__name__", None), "default": a.default, "nargs": a.nargs,
                 "const": a.const, "choices": None if a.choices is None else list(a.choices), "action": type(a).__name__, "metavar": a.metavar,
                 "required": a.required, "exclusive": exclusive.get(a.option_strings[0])}
        out[a.option_strings[0]] = {k: v for k, v in every.items() if v is not None and (k, v) != ("required", False)}  # (left out: None; not required)
    return json.loads(json.dumps(out))


# ---- the command lines ----------------------------------------------------------------------------------------------------------------
# every shared request flag at a value that is not its default
SHARED = [["--sampler-temp", "0.7"], ["--sampler-top-p", "0.9"], ["--sampler-top-k", "40"], ["--sampler-seed", "5"], ["--repetition-penalty", "1.3"],
          ["--presence-penalty", "0.4"], ["--frequency-penalty", "0.2"], ["--dry-multiplier", "0.8"], ["--dry-base", "2.0"], ["--dry-allowed-length", "3"],
          ["--dry-range", "64"], ["--dry-breaker", "word"], ["--no-repeat-ngram", "3"], ["--sampler-min-p", "0.05"], ["--sampler-typical-p", "0.9"],
          ["--mirostat-tau", "4.0"], ["--mirostat-eta", "0.3"], ["--regex", "a+"], ["--json", "object"], ["--json-schema", "no-such-file"],
          ["--stop", "END"], ["--stop-id", "9"], ["--enable-thinking"], ["--proposal-length", "3"]]
INERT_ALONE = ("--sampler-top-p", "--sampler-top-k", "--sampler-seed", "--sampler-min-p", "--sampler-typical-p", "--mirostat-tau", "--mirostat-eta")
MIROSTAT_OTHERS = [["--sampler-top-k", "40"], ["--sampler-top-p", "0.9"], ["--sampler-min-p", "0.05"], ["--sampler-typical-p", "0.9"]]
DRY = ["--dry-multiplier", "0.8", "--dry-base", "2.0", "--dry-allowed-length", "3", "--dry-range", "64", "--dry-breaker", "word", "--dry-breaker", "two words",
       "--dry-breaker", "word", "--no-repeat-ngram", "4"]
PENALTIES = ["--repetition-penalty", "1.3", "--presence-penalty", "0.4", "--frequency-penalty", "0.2"]
EVERY_GROUP = ["--sampler-temp", "0.8", "--sampler-top-p", "0.9", "--sampler-top-k", "40", "--sampler-seed", "7", "--sampler-min-p", "0.05",
               "--sampler-typical-p", "0.9", *PENALTIES, *DRY, "--regex", "a+", "--stop", "END", "--stop-id", "9", "--stop-id", "12"]


def main_vectors() -> dict:
    base = ["--model", "m", "--max-new-tokens", "6"]
    out = {"plain": base, "defaults": ["--model", "m"]}
    for flag in SHARED:
        out["alone " + " ".join(flag)] = base + flag
        if flag[0] in INERT_ALONE and flag[0] != "--sampler-seed":
            out["sampled " + " ".join(flag)] = base + ["--sampler-temp", "0.8", "--sampler-seed", "3"] + flag
    # check_truncation_flags
    for other in MIROSTAT_OTHERS:
        out["mirostat with " + other[0]] = base + ["--sampler-temp", "0.8", "--mirostat-tau", "5"] + other
    out["mirostat with neutral others"] = base + ["--sampler-temp", "0.8", "--sampler-seed", "1", "--mirostat-tau", "5", "--sampler-top-p", "1.0",
                                                   "--sampler-typical-p", "1.0", "--sampler-top-k", "0", "--sampler-min-p", "0"]
    # check_beam_flags
    beams = base + ["--num-beams", "2"]
    out["beam: length penalty alone"] = base + ["--length-penalty", "0.8"]
    out["beam: early stopping alone"] = base + ["--early-stopping"]
    out["beam: 0 beams"] = base + ["--num-beams", "0"]
    out["beam: 9 beams"] = base + ["--num-beams", "9"]
    out["beam: too many eos ids"] = base + ["--num-beams", "8", "--stop-id", "1", "--stop-id", "2", "--stop-id", "3"]
    for extra in ([["--solution", "ops"], ["--draft-model", "d"], ["--logprobs", "2"], ["--lora", "dir"], ["--sampler-typical-p", "1.0"]] + SHARED):
        out["beam with " + " ".join(extra)] = beams + extra
    out["beam with everything"] = beams + ["--solution", "ops", "--draft-model", "d", "--logprobs", "0", "--lora", "dir"] + EVERY_GROUP
    out["beam"] = base + ["--num-beams", "3", "--length-penalty", "0.8", "--early-stopping", "--stop-id", "9", "--stop-id", "9", "--raw-prompt"]
    # the routes, each with the flags that make it print a note
    out["ops"] = base + ["--solution", "ops"]
    out["ops with notes"] = base + ["--solution", "ops", "--sampler-temp", "0.8", *PENALTIES, *DRY]
    out["ops with a grammar"] = base + ["--solution", "ops", "--json", "value"]
    out["ops with a draft"] = base + ["--solution", "ops", "--draft-model", "d", "--proposal-length", "5", *PENALTIES]
    out["draft greedy"] = base + ["--draft-model", "d"]
    out["draft greedy with notes"] = base + ["--draft-model", "d", "--lora", "dir", "--stop", "END", *PENALTIES, *DRY, "--regex", "a+", "--proposal-length", "9"]
    out["draft greedy with a stop id"] = base + ["--draft-model", "d", "--stop-id", "9"]
    out["draft sampled without a seed"] = base + ["--draft-model", "d", "--sampler-temp", "0.8", "--sampler-top-k", "40", "--sampler-top-p", "0.9",
                                                   "--sampler-min-p", "0.05"]
    out["draft sampled with a seed"] = base + ["--draft-model", "d", "--sampler-temp", "0.8", "--sampler-seed", "11", "--mirostat-tau", "4"]
    out["draft sampled, typical-p 1"] = base + ["--draft-model", "d", "--sampler-temp", "0.8", "--sampler-seed", "0", "--sampler-typical-p", "1.0"]
    out["device sampler with a seed"] = base + ["--sampler-temp", "0.8", "--sampler-seed", "11", "--sampler-top-k", "40", "--sampler-top-p", "0.9"]
    out["device sampler, seed 0"] = base + ["--sampler-temp", "0.8", "--sampler-seed", "0"]
    for name, extra in (("penalties", PENALTIES), ("dry", DRY), ("a grammar", ["--json-schema", "file"]), ("a lora", ["--lora", "dir"]),
                        ("a stop string", ["--stop", "END"]), ("min-p", ["--sampler-min-p", "0.1"]), ("mirostat", ["--mirostat-tau", "4", "--mirostat-eta", "0.2"])):
        out["device sampler without a seed, by " + name] = base + ["--sampler-temp", "0.8"] + extra
    out["device sampler with logprobs"] = base + ["--sampler-temp", "0.8", "--sampler-seed", "3", "--logprobs", "1"]
    out["device sampler with everything"] = base + EVERY_GROUP + ["--lora", "dir", "--logprobs", "2", "--enable-thinking"]
    out["device sampler, a neutral flag out of range"] = base + ["--sampler-temp", "0.8", "--sampler-seed", "1", "--sampler-min-p", "-0.5"]
    out["device sampler, neutral eta out of range"] = base + ["--sampler-temp", "0.8", "--sampler-seed", "1", "--mirostat-eta", "5"]
    out["host sampler"] = base + ["--sampler-temp", "0.8", "--sampler-top-k", "40", "--sampler-top-p", "0.9"]
    out["host sampler with logprobs"] = base + ["--sampler-temp", "0.8", "--logprobs", "1"]
    out["host sampler, typical-p 1"] = base + ["--sampler-temp", "0.8", "--sampler-typical-p", "1.0"]
    out["greedy with logprobs"] = base + ["--logprobs", "3"]
    out["greedy with everything"] = base + [a for a in EVERY_GROUP if a not in ("--sampler-temp", "0.8")] + ["--lora", "dir", "--logprobs", "0", "--raw-prompt",
                                                                                                               "--prompt", "one two three"]
    out["greedy, truncation flags ignored"] = base + ["--sampler-min-p", "0.1", "--mirostat-eta", "5", "--sampler-top-k", "40"]
    out["greedy, dry out of range"] = base + ["--dry-multiplier", "0.5", "--dry-base", "0.5"]
    return out


def batch_vectors() -> dict:
    base = ["--model", "m", "--max-seq-len", "8", "--prompts-file", PROMPTS]
    out = {"plain": base, "built-in prompts": ["--model", "m", "--max-seq-len", "20"], "batch of 2": base + ["--batch-size", "2", "--prefill-step", "4", "--raw-prompts"],
           "engine flags": base + ["--kv-format", "fp8", "--prefix-cache", "--swap-pages", "4"], "prefix cache cap": base + ["--prefix-cache", "8"],
           "prompt too long": ["--model", "m", "--max-seq-len", "4"]}
    for flag in SHARED:
        out["alone " + " ".join(flag)] = base + flag
        if flag[0] in INERT_ALONE:
            out["sampled " + " ".join(flag)] = base + ["--sampler-temp", "0.8"] + flag
    for other in MIROSTAT_OTHERS:
        out["mirostat with " + other[0]] = base + ["--sampler-temp", "0.8", "--mirostat-tau", "5"] + other
    out["mirostat with neutral others"] = base + ["--sampler-temp", "0.8", "--mirostat-tau", "5", "--mirostat-eta", "0.2", "--sampler-top-p", "1.0",
                                                   "--sampler-typical-p", "1.0", "--sampler-top-k", "0"]
    # check_draft_flags
    draft = base + ["--draft-model", "d"]
    out["draft"] = draft + ["--proposal-length", "5"]
    for extra in SHARED + [["--lora", "dir"], ["--sampler-typical-p", "1.0"], ["--proposal-length", "0"], ["--proposal-length", "8"]]:
        if extra[0] != "--proposal-length" or extra[1] != "3":
            out["draft with " + " ".join(extra)] = draft + extra
    out["draft with everything"] = draft + EVERY_GROUP + ["--lora", "a", "--mirostat-eta", "0.5"]
    out["draft with mirostat"] = draft + ["--sampler-temp", "0.8", "--mirostat-tau", "4"]
    # lora, stop, every group
    for assign in ("round-robin", "first"):
        out["two loras, " + assign] = base + ["--lora", "a", "--lora", "b", "--lora-assign", assign]
    out["stop strings and ids"] = base + ["--stop", "END", "--stop", "t9", "--stop-id", "9", "--json", "object"]
    out["every group"] = base + EVERY_GROUP + ["--lora", "a", "--batch-size", "3"]
    out["every group, mirostat"] = base + ["--sampler-temp", "0.8", "--sampler-seed", "100", "--mirostat-tau", "4", "--mirostat-eta", "0.2", *PENALTIES, *DRY]
    out["a neutral flag out of range"] = base + ["--sampler-temp", "0.8", "--sampler-min-p", "-0.5"]
    out["dry out of range"] = base + ["--no-repeat-ngram", "1"]
    return out


def record_cli() -> dict:
    out = {"main": {name: run_cli("main", argv) for name, argv in main_vectors().items()},
           "batch_main": {name: run_cli("batch_main", argv) for name, argv in batch_vectors().items()}}
    for script in out:
        out[script]["stop id matched"] = run_matched_stop(script)
    return out


def run_matched_stop(script: str) -> dict:
    """Stop conditions that match (scripted: every armed request's set matches at a fixed count): the answer ends at the stopping id,
    which is not printed."""
    if script == "main":
        return run_cli("main", ["--model", "m", "--max-new-tokens", "40", "--stop-id", str(_third_id_of_main())], stop_at=3)
    return run_cli("batch_main", ["--model", "m", "--max-seq-len", "8", "--prompts-file", PROMPTS, "--stop-id", "9", "--stop", "END"], stop_at=2)


def _third_id_of_main() -> int:
    """The third id the recording engine produces for main.py's default prompt (so that --stop-id names the id the answer ends with)."""
    from scheduler_recorder import produced_id

    tok = WordTokenizer()
    prompt = tok.apply_chat_template([{"role": "user", "content": "Give me a short introduction to large language model."}])
    return produced_id(sum(tok.encode(prompt)), 3)


# ---- request_settings -----------------------------------------------------------------------------------------------------------------
def settings_cases() -> dict:
    gram = fake_grammar("grammar", [7, 9])
    stop = fake_stop_set("stop")
    every = {"temperature": 0.8, "top_k": 40, "top_p": 0.9, "seed": 11, "min_p": 0.05, "typical_p": 0.9, "mirostat_tau": 0.0, "mirostat_eta": 0.3,
             "repetition_penalty": 1.1, "presence_penalty": 0.2, "frequency_penalty": 0.1, "logit_bias": {5: 1.0, 2: -4.0}, "grammar": gram, "lora": 1,
             "dry_multiplier": 0.8, "dry_base": 2.0, "dry_allowed_length": 3, "dry_range": 64, "dry_breakers": [4, 6], "no_repeat_ngram": 3}
    out = {"none": dict(sampling=None, n_prompts=2), "none with base_seed": dict(sampling=None, n_prompts=3, base_seed=100),
           "empty dict": dict(sampling={}, n_prompts=2, base_seed=2 ** 64 - 1), "every key": dict(sampling=every, n_prompts=2, vocab_size=VOCAB),
           "every key, mirostat": dict(sampling={**every, "top_k": None, "top_p": None, "min_p": 0.0, "typical_p": None, "mirostat_tau": 4.0}, n_prompts=1),
           "a list": dict(sampling=[{"temperature": 0.5}, {}, {"seed": 3, "lora": 2}, every], n_prompts=4, base_seed=10, vocab_size=VOCAB),
           "lora list in one dict": dict(sampling={"lora": [0, None, -1]}, n_prompts=3),
           "logprobs, stop and limits": dict(sampling={"temperature": 1.0}, n_prompts=2, logprobs=2, stop=[stop, None], limits=[4, 5]),
           "one stop, one limit": dict(sampling=None, n_prompts=2, logprobs=0, stop=stop, limits=7),
           "explicit neutral values": dict(sampling={"temperature": 0.0, "top_k": 0, "top_p": 1.0, "seed": 0, "min_p": 0.0, "typical_p": 1.0, "mirostat_tau": 0.0,
                                                     "mirostat_eta": 0.1, "repetition_penalty": 1.0, "presence_penalty": 0.0, "frequency_penalty": 0.0,
                                                     "logit_bias": None, "grammar": None, "lora": None, "dry_multiplier": 0.0, "dry_base": 1.75,
                                                     "dry_allowed_length": 2, "dry_range": 0, "dry_breakers": (), "no_repeat_ngram": 0}, n_prompts=1, base_seed=9)}
    for key, value in every.items():
        out[f"alone {key}"] = dict(sampling={key: value}, n_prompts=2, base_seed=5, vocab_size=VOCAB)
    nan, inf = float("nan"), float("inf")
    bad = {"temperature": [-1.0, nan, inf, "1", True], "top_k": [-1, 1.5, True], "top_p": [0.0, 1.5, "x", True], "seed": [-1, 2 ** 64, 1.0, True],
           "min_p": [-0.1, 1.5, "x", nan, True], "typical_p": [0.0, 1.5, "x", inf], "mirostat_tau": [-1.0, nan, "x"], "mirostat_eta": [0.0, 1.5, nan],
           "repetition_penalty": [0.0, -1.0, nan, "x", True], "presence_penalty": [nan, "x"], "frequency_penalty": [inf, None],
           "logit_bias": [{VOCAB: 1.0}, {-1: 1.0}, [1, 2], {1: nan}], "grammar": ["a+", 3], "lora": [32, -2, 1.0, True, [0]],
           "dry_multiplier": [-0.5, nan, "x", True], "dry_base": [0.5, inf, None], "dry_allowed_length": [0, 1.5, True], "dry_range": [-1, 2.0],
           "dry_breakers": [[VOCAB], [-1], [3, 3], [1.5], list(range(65))], "no_repeat_ngram": [1, 65, -2, 2.0, True]}
    for key, values in bad.items():
        for k, value in enumerate(values):
            base = {"mirostat_tau": 1.0} if key == "mirostat_eta" else {}
            out[f"bad {key} {k}"] = dict(sampling={**base, key: value}, n_prompts=2, vocab_size=VOCAB)
    out["unknown key"] = dict(sampling={"temp": 1.0, "beams": 2}, n_prompts=1)
    out["entry is no dict"] = dict(sampling=[{}, 3], n_prompts=2)
    out["too few dicts"] = dict(sampling=[{}], n_prompts=2)
    for name, extra in (("top_k", {"top_k": 40}), ("top_p", {"top_p": 0.9}), ("min_p", {"min_p": 0.1}), ("typical_p", {"typical_p": 0.9})):
        out[f"mirostat with {name}"] = dict(sampling={"temperature": 1.0, "mirostat_tau": 5.0, **extra}, n_prompts=1)
    out["mirostat with neutral others"] = dict(sampling={"temperature": 1.0, "mirostat_tau": 5.0, "top_k": 0, "top_p": 1.0, "min_p": 0.0, "typical_p": 1.0}, n_prompts=1)
    out["bad logprobs"] = dict(sampling=None, n_prompts=1, logprobs=21)
    out["bad logprobs type"] = dict(sampling=None, n_prompts=1, logprobs=True)
    out["bad stop"] = dict(sampling=None, n_prompts=2, stop=[stop])
    return out


def run_settings(kw: dict) -> dict:
    from tiny_llm_hip.engine import request_settings

    kw = dict(kw)
    try:
        return {"error": None, "settings": json.loads(json.dumps(plain([list(s) for s in request_settings(kw.pop("sampling"), kw.pop("n_prompts"), **kw)])))}
    except (ValueError, TypeError) as exc:
        return {"error": f"{type(exc).__name__}: {exc}"}


def generate_cases() -> dict:
    """DecodeEngine.generate(**kw) over the recording engine: the settings as keywords."""
    cases = settings_cases()
    out = {"defaults": {}, "chunk and slot": dict(slot=1, chunk=2), "stop in blocks": dict(stop=fake_stop_set("stop"), decode_block=2, logprobs=1),
           "bad decode_block": dict(stop=fake_stop_set("stop"), decode_block=0)}
    for name in ("every key", "every key, mirostat", "explicit neutral values", "bad top_p 1", "bad dry_breakers 2", "mirostat with top_k", "bad lora 0",
                 "lora list in one dict"):
        out[name] = dict(cases[name]["sampling"])
    for key, value in cases["every key"]["sampling"].items():
        out[f"alone {key}"] = {key: value}
    return out


def run_generate(kw: dict) -> dict:
    session = Session()
    engine = session.engine_class()(SimpleNamespace(name="model"), max_batch=2)
    result, error = None, None
    try:
        result = engine.generate([3, 4, 5, 6, 7], 4, **kw)
    except (ValueError, TypeError) as exc:
        error = f"{type(exc).__name__}: {exc}"
    return json.loads(json.dumps({"error": error, "calls": engine_log(engine.calls), "result": plain(result)}))


def record() -> dict:
    """Everything above; equal outcomes are kept once, in "pool", and a scenario holds its outcome's index there."""
    cli = record_cli()
    named = {"main": cli["main"], "batch_main": cli["batch_main"], "settings": {name: run_settings(kw) for name, kw in settings_cases().items()},
             "generate": {name: run_generate(kw) for name, kw in generate_cases().items()}}
    pool: list = []
    for section in named.values():
        for name, outcome in section.items():
            if outcome not in pool:
                pool.append(outcome)
            section[name] = pool.index(outcome)
    return {"parsers": {script: parser_surface(script) for script in ("main", "batch_main")}, "pool": pool, **named}
