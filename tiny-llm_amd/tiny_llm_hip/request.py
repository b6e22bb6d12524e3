"""What a request can set on its slot, declared once: the Python counterpart of csrc/slot_settings.h (DESIGN.md has the steps to add one).

``SETTINGS`` is the table: per key of a ``sampling`` dict (and of ``DecodeEngine.generate``'s keywords) its neutral default, its validator
group and the command-line flags that set it.  From it follow ``SETTINGS_KEYS``, the defaults of the validators, of ``RequestSettings``
and of ``request_settings``, ``DRY_OFF``, the flags main.py and batch_main.py share (``add_request_flags``), what a command line switches on
(``switched``) and the ``sampling`` dict it stands for (``sampling_dict``).  Host logic only: no torch, no device.
"""

from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Any, Callable, NamedTuple, Sequence

from ._ext import tiny_llm_ext_hip as _ext

# a flag's predicates over (its value, its setting's default)
_never, _set, _truthy = (lambda v, d: False), (lambda v, d: v is not None), (lambda v, d: bool(v))
_positive, _below_one, _differs = (lambda v, d: v > 0), (lambda v, d: v is not None and v < 1), (lambda v, d: v != d)


class Flag(NamedTuple):
    """One command-line flag of a setting.  ``given``: the command line names the flag (what --num-beams refuses); ``on``: its value is
    not the neutral one (--sampler-typical-p 1.0 is given and off).  ``leads``: an ``on`` value switches the flag's group on -- top-k and
    top-p narrow a sampling request, they do not make one.  ``defaults``: the parser default per script where it is not the setting's."""
    option: str
    help: str
    kw: dict = {}  # add_argument's type / action / metavar / choices
    given: Callable[[Any, Any], bool] = _never
    on: Callable[[Any, Any], bool] = _never
    leads: bool = True
    exclusive: bool = False  # the exclusive flags of a setting form one mutually exclusive group
    defaults: dict = {}

    @property
    def dest(self) -> str:
        return self.option[2:].replace("-", "_")


class Setting(NamedTuple):
    key: str      # as ``sampling`` dicts and generate spell it
    default: Any  # the neutral value
    group: str    # the validator that takes it: sampling, truncation (with Mirostat), penalties, bias, dry, grammar, lora
    flags: tuple = ()


_F, _I, _N, _STRINGS = {"type": float}, {"type": int}, {"type": int, "metavar": "N"}, {"action": "append", "metavar": "STRING"}
SETTINGS = (
    Setting("temperature", 0.0, "sampling", (Flag("--sampler-temp", "0 = greedy; else sample (on the device or, main.py, on the host)", _F, _truthy, _truthy),)),
    Setting("top_k", None, "sampling", (Flag("--sampler-top-k", "sample among the K most likely tokens", _I, _set, _truthy, leads=False),)),
    Setting("top_p", None, "sampling", (Flag("--sampler-top-p", "sample among the likeliest tokens whose mass reaches this", _F, _set, _below_one, leads=False),)),
    Setting("seed", None, "sampling", (Flag("--sampler-seed", "the device's seed (main.py: selects the device sampler; batch_main.py: request i draws from seed + i)",
                                            _I, _set, defaults={"main": None, "batch_main": 0}),)),  # (no seed: request i of a call draws from base_seed + i)
    Setting("min_p", 0.0, "truncation", (Flag("--sampler-min-p", "sampling on the device: keep tokens with p >= min_p * p_max (0 = off)", _F, _positive, _positive),)),
    Setting("typical_p", None, "truncation", (Flag("--sampler-typical-p", "... keep the tokens nearest the entropy up to this mass (1 = off)", _F, _set, _below_one),)),
    Setting("mirostat_tau", 0.0, "truncation", (Flag("--mirostat-tau", "... Mirostat v2 with this target surprise (bits) (0 = off); excludes top-k, top-p, min-p, typical-p",
                                                     _F, _positive, _positive),)),
    Setting("mirostat_eta", 0.1, "truncation", (Flag("--mirostat-eta", "Mirostat's learning rate, in (0, 1]", _F),)),
    Setting("repetition_penalty", 1.0, "penalties", (Flag("--repetition-penalty", "on the device, over prompt and output (1 = off)", _F, _differs, _differs),)),
    Setting("presence_penalty", 0.0, "penalties", (Flag("--presence-penalty", "on the device, over the output (0 = off)", _F, _differs, _differs),)),
    Setting("frequency_penalty", 0.0, "penalties", (Flag("--frequency-penalty", "on the device, times the count in the output (0 = off)", _F, _differs, _differs),)),
    Setting("logit_bias", None, "bias"),
    Setting("grammar", None, "grammar", (
        Flag("--regex", "the answer must match PATTERN in full (tiny_llm_hip.grammar's dialect), on the device", {"metavar": "PATTERN"}, _truthy, _truthy, exclusive=True),
        Flag("--json", "the answer is one JSON object (or any value), up to 32 levels, on the device", {"choices": ["object", "value"]}, _truthy, _truthy, exclusive=True),
        Flag("--json-schema", "the answer is compact JSON that fits the schema in FILE (grammar.schema_regex)", {"metavar": "FILE"}, _truthy, _truthy, exclusive=True))),
    Setting("lora", None, "lora"),  # (--lora is each script's own: one adapter there, several here)
    Setting("dry_multiplier", 0.0, "dry", (Flag("--dry-multiplier", "DRY, on the device: the token that would extend a verbatim repeat of L tokens loses multiplier * "
                                                "base ** (L - allowed_length) (0 = off)", _F, _positive, _positive),)),
    Setting("dry_base", 1.75, "dry", (Flag("--dry-base", "DRY's base (>= 1)", _F),)),
    Setting("dry_allowed_length", 2, "dry", (Flag("--dry-allowed-length", "the longest repeat DRY leaves alone, plus one (>= 1)", _I),)),
    Setting("dry_range", 0, "dry", (Flag("--dry-range", "DRY looks for repeats in the last N tokens (0 = all)", _I),)),
    Setting("dry_breakers", (), "dry", (Flag("--dry-breaker", "a repeat never runs across the last token of STRING's encoding; repeatable (64)", _STRINGS),)),
    Setting("no_repeat_ngram", 0, "dry", (Flag("--no-repeat-ngram", "on the device: no N-gram twice (0 = off, else 2 .. 64)", _N, _positive, _positive),)),
)
# stop conditions are an argument of their own (``stop=``: a StopSet over the engine's vocabulary), not a ``sampling`` key; their flags are shared all the same
STOP_FLAGS = (Flag("--stop", "end an answer where its text holds STRING (matched on the device, across token boundaries); repeatable (16)", _STRINGS, _truthy, _truthy),
              Flag("--stop-id", "end an answer at token id N (not printed); repeatable", {"action": "append", **_N}, _truthy, _truthy))
FLAGS = [(s.group, s.default, f) for s in SETTINGS for f in s.flags] + [("stop", (), f) for f in STOP_FLAGS]
SETTINGS_KEYS = {s.key for s in SETTINGS}
_D = {s.key: s.default for s in SETTINGS}


# ---- the validators: one per group, named after the tl_engine_set_* call that takes its tuple ------------------------------------------
def logprobs_arg(top_n: int | None) -> int:
    """tl_engine_set_logprobs' top_n: None -> -1 (off), else an int in [0, 20]."""
    if top_n is None:
        return -1
    if isinstance(top_n, bool) or not isinstance(top_n, int) or not 0 <= top_n <= _ext.TL_MAX_TOP_LOGPROBS:
        raise ValueError(f"logprobs must be None or an int in [0, {_ext.TL_MAX_TOP_LOGPROBS}], got {top_n!r}")
    return top_n


def sampling_args(temperature: float = _D["temperature"], top_k: int | None = _D["top_k"], top_p: float | None = _D["top_p"],
                  seed: int = 0) -> tuple[float, int, float, int]:
    """Validated (temperature, top_k, top_p, seed) for tl_engine_set_sampling: temperature finite and >= 0 (0 = greedy); top_k None
    or 0 = no top-k, else a positive int (beyond the vocabulary: none); top_p None = no top-p, else in (0, 1] (1 = none); seed an
    int in [0, 2^64)."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature < 0:
        raise ValueError(f"temperature must be a finite number >= 0, got {temperature!r}")
    if top_k is None:
        top_k = 0
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 0:
        raise ValueError(f"top_k must be None or an int >= 0, got {top_k!r}")
    if top_p is None:
        top_p = 1.0
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not (0.0 < top_p <= 1.0):
        raise ValueError(f"top_p must be None or in (0, 1], got {top_p!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an int in [0, 2**64), got {seed!r}")
    return float(temperature), min(int(top_k), 2**31 - 1), float(top_p), int(seed)


def truncation_args(min_p: float = _D["min_p"], typical_p: float | None = _D["typical_p"], mirostat_tau: float = _D["mirostat_tau"],
                    mirostat_eta: float = _D["mirostat_eta"], *, top_k: int = 0, top_p: float = 1.0) -> tuple[float, float, float, float]:
    """Validated (min_p, typical_p, tau, eta) for tl_engine_set_truncation / tl_engine_set_mirostat: min_p in [0, 1] (0 = off),
    typical_p None or in (0, 1] (1 = off), mirostat_tau finite and >= 0 (0 = off), mirostat_eta in (0, 1].  Mirostat excludes every
    other truncation: with tau > 0, min_p, typical_p and the request's ``top_k`` / ``top_p`` (as sampling_args returns them) must be off."""
    if typical_p is None:
        typical_p = 1.0
    for name, v in (("min_p", min_p), ("typical_p", typical_p), ("mirostat_tau", mirostat_tau), ("mirostat_eta", mirostat_eta)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if not 0.0 <= min_p <= 1.0:
        raise ValueError(f"min_p must be in [0, 1], got {min_p!r}")
    if not 0.0 < typical_p <= 1.0:
        raise ValueError(f"typical_p must be None or in (0, 1], got {typical_p!r}")
    if mirostat_tau < 0:
        raise ValueError(f"mirostat_tau must be >= 0, got {mirostat_tau!r}")
    if not 0.0 < mirostat_eta <= 1.0:
        raise ValueError(f"mirostat_eta must be in (0, 1], got {mirostat_eta!r}")
    if mirostat_tau > 0 and (min_p > 0 or typical_p < 1 or top_k > 0 or top_p < 1):
        raise ValueError("Mirostat excludes every other truncation (top_k, top_p, min_p, typical_p)")
    return float(min_p), float(typical_p), float(mirostat_tau), float(mirostat_eta) if mirostat_tau > 0 else 0.0


def penalty_args(repetition: float = _D["repetition_penalty"], presence: float = _D["presence_penalty"],
                 frequency: float = _D["frequency_penalty"]) -> tuple[float, float, float]:
    """Validated (repetition, presence, frequency) for tl_engine_set_penalties: repetition finite and > 0 (1 = off), presence and
    frequency finite (0 = off; negative values encourage repetition)."""
    for name, v in (("repetition_penalty", repetition), ("presence_penalty", presence), ("frequency_penalty", frequency)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if not repetition > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {repetition!r}")
    return float(repetition), float(presence), float(frequency)


def dry_args(multiplier: float = _D["dry_multiplier"], base: float = _D["dry_base"], allowed_length: int = _D["dry_allowed_length"],
             range: int = _D["dry_range"], no_repeat_ngram: int = _D["no_repeat_ngram"], breakers: Sequence[int] = _D["dry_breakers"],  # noqa: A002
             vocab_size: int = 0) -> tuple:
    """Validated (multiplier, base, allowed_length, range, no_repeat_ngram, breakers) for tl_engine_set_dry: multiplier finite and >= 0
    (0 = off), base finite and >= 1, allowed_length >= 1, range >= 0 (0 = everything recorded), no_repeat_ngram 0 (off) or 2 .. 64,
    breakers up to 64 distinct ids (inside ``vocab_size`` where that is given)."""
    for name, v in (("dry_multiplier", multiplier), ("dry_base", base)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if multiplier < 0:
        raise ValueError(f"dry_multiplier must be >= 0, got {multiplier!r}")
    if base < 1:
        raise ValueError(f"dry_base must be >= 1, got {base!r}")
    for name, v in (("dry_allowed_length", allowed_length), ("dry_range", range), ("no_repeat_ngram", no_repeat_ngram)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if allowed_length < 1:
        raise ValueError(f"dry_allowed_length must be >= 1, got {allowed_length!r}")
    if range < 0:
        raise ValueError(f"dry_range must be >= 0, got {range!r}")
    if no_repeat_ngram != 0 and not 2 <= no_repeat_ngram <= _ext.TL_DRY_MAX_MATCH:
        raise ValueError(f"no_repeat_ngram must be 0 (off) or 2 .. {_ext.TL_DRY_MAX_MATCH}, got {no_repeat_ngram!r}")
    ids = tuple(breakers or ())
    if any(isinstance(t, bool) or not isinstance(t, int) or t < 0 or (vocab_size and t >= vocab_size) for t in ids):
        raise ValueError("dry_breakers must be token ids inside the vocabulary")
    if len(set(ids)) != len(ids):
        raise ValueError("dry_breakers: a token id appears twice")
    if len(ids) > _ext.TL_MAX_DRY_BREAKERS:
        raise ValueError(f"dry_breakers takes at most {_ext.TL_MAX_DRY_BREAKERS} ids, got {len(ids)}")
    return float(multiplier), float(base), allowed_length, range, no_repeat_ngram, ids


def dry_breaker_ids(tokenizer, strings: Sequence[str]) -> list[int]:
    """The breaker ids of ``strings`` as text-generation-webui derives them: each string gives the LAST id of its encoding (a breaker is
    one token); duplicates are dropped, the order kept."""
    out: list[int] = []
    for s in strings:
        try:
            ids = tokenizer.encode(s, add_special_tokens=False)
        except TypeError:
            ids = tokenizer.encode(s)
        ids = getattr(ids, "ids", ids)
        if len(ids) and int(ids[-1]) not in out:
            out.append(int(ids[-1]))
    return out


DRY_OFF = dry_args()  # of a request with neither DRY nor the n-gram ban
PENALTIES_OFF = penalty_args()


class RequestSettings(NamedTuple):
    """Everything one request sets on its slot, validated (request_settings builds it from a ``sampling`` dict); the defaults are a plain
    greedy request: the validators' answers to the table's defaults."""
    sampling: tuple = sampling_args()            # temperature, top_k, top_p, seed
    truncation: tuple = truncation_args()        # min_p, typical_p, mirostat tau, eta
    penalties: tuple = PENALTIES_OFF             # repetition, presence, frequency
    bias: dict = {}                              # logit bias {token id: value}
    grammar: "Grammar | None" = None
    lora: int = -1                               # a resident adapter's id; -1: the base model
    top_n: int = logprobs_arg(None)              # alternatives per recorded token; -1: no records
    armed: bool = False                          # stop conditions on the device: the slot is armed with ``stop`` and ``budget``
    stop: Any = None                             # a StopSet or None
    budget: int = 0                              # the request's max_new_tokens
    dry: tuple = DRY_OFF                         # multiplier, base, allowed_length, range, no_repeat_ngram, breaker ids

    def apply(self, engine, slot: int) -> None:
        """The one setter sequence, on a freshly begun slot and before its prompt's first chunk:
        lora, sampling, truncation / Mirostat, penalties, bias, grammar, logprobs, stop.
        A neutral value makes no call.  The order is free but for one rule: each setter rewrites only its own per-slot record
        (csrc/engine.hip), and the one cross-check -- truncation / Mirostat against the slot's top_k / top_p -- needs sampling first.
        Any order that keeps that rule leaves the slot in the same end state."""
        if self.lora >= 0:
            engine.set_lora(slot, self.lora)
        if self.sampling[0] > 0.0:
            engine.set_sampling(slot, *self.sampling)
        if self.truncation[0] > 0.0 or self.truncation[1] < 1.0:
            engine.set_truncation(slot, self.truncation[0], self.truncation[1])
        if self.truncation[2] > 0.0:
            engine.set_mirostat(slot, self.truncation[2], self.truncation[3])
        if self.penalties != PENALTIES_OFF:
            engine.set_penalties(slot, *self.penalties)
        if self.bias:
            engine.set_logit_bias(slot, self.bias)
        if self.grammar is not None:
            engine.set_grammar(slot, self.grammar)
        if self.dry[0] > 0.0 or self.dry[4] > 0:
            engine.set_dry(slot, *self.dry)
        if self.top_n >= 0:
            engine.set_logprobs(slot, self.top_n)
        if self.armed:
            engine.set_stop(slot, self.stop, self.budget)


def request_settings(sampling, n_prompts: int, base_seed: int = 0, vocab_size: int = 0, logprobs: int | None = None, stop=None,
                     limits: int | Sequence[int] = 0) -> list[RequestSettings]:
    """One RequestSettings per prompt.  ``sampling``: None (greedy), one dict for every request or one dict per prompt, with keys of
    SETTINGS, each group through its validator: sampling_args (a request without a seed gets base_seed + its prompt index, so requests
    do not share a random stream), truncation_args (exclusivity against the same dict's top_k / top_p included), penalty_args,
    logit_bias_arg over ``vocab_size``, dry_args, a Grammar or None, lora.request_loras (also one list for all in a single dict).
    ``logprobs``: logprobs_arg, for every request.  ``stop``: stop.request_stops; a request is armed when it is not None.  ``limits``:
    max_new_tokens, one for all or one per prompt.  ValueError for anything else."""
    from .engine import Grammar
    from .lora import request_loras
    from .stop import request_stops

    stops = request_stops(stop, n_prompts)
    limits = [limits] * n_prompts if isinstance(limits, int) else list(limits)
    dicts = [{}] * n_prompts if sampling is None else [sampling] * n_prompts if isinstance(sampling, dict) else list(sampling)
    if len(dicts) != n_prompts:
        raise ValueError("sampling needs one dict per prompt (or one dict for all)")
    out = []
    for i, d in enumerate(dicts):
        if not isinstance(d, dict):
            raise ValueError("sampling entries must be dicts")
        unknown = set(d) - SETTINGS_KEYS
        if unknown:
            raise ValueError(f"unknown sampling keys: {sorted(unknown)}")
        d = {**_D, **d}
        smp = sampling_args(d["temperature"], d["top_k"], d["top_p"], (base_seed + i) & 0xFFFFFFFFFFFFFFFF if d["seed"] is None else d["seed"])
        bias = d["logit_bias"]
        _ext.logit_bias_arg(bias, vocab_size)
        pen = penalty_args(d["repetition_penalty"], d["presence_penalty"], d["frequency_penalty"])
        grammar = d["grammar"]
        if grammar is not None and not isinstance(grammar, Grammar):
            raise ValueError("sampling['grammar'] must be a Grammar (DecodeEngine.make_grammar) or None")
        trn = truncation_args(d["min_p"], d["typical_p"], d["mirostat_tau"], d["mirostat_eta"], top_k=smp[1], top_p=smp[2])
        dry = dry_args(d["dry_multiplier"], d["dry_base"], d["dry_allowed_length"], d["dry_range"], d["no_repeat_ngram"], d["dry_breakers"], vocab_size)
        out.append(RequestSettings(sampling=smp, truncation=trn, penalties=pen, bias=dict(bias) if bias else {}, grammar=grammar, dry=dry,
                                   armed=stops is not None, stop=stops[i] if stops is not None else None, budget=limits[i]))
    loras = request_loras(sampling, n_prompts) or [-1] * n_prompts
    top_n = logprobs_arg(logprobs)
    return [s._replace(lora=lora, top_n=top_n) for s, lora in zip(out, loras)]


# ---- the command line: the flags main.py and batch_main.py share ------------------------------------------------------------------------
def add_request_flags(ap, script: str) -> None:
    """Add every flag of the table (and --stop / --stop-id) to ``ap``; ``script`` ("main" or "batch_main") picks the per-script defaults."""
    exclusive = {}
    for group, default, flag in FLAGS:
        default = flag.defaults.get(script, default)
        if flag.exclusive and group not in exclusive:
            exclusive[group] = ap.add_mutually_exclusive_group()
        (exclusive[group] if flag.exclusive else ap).add_argument(flag.option, default=list(default) if flag.kw.get("action") == "append" else default,
                                                                  help=flag.help, **flag.kw)


def switched(args) -> SimpleNamespace:
    """What a command line (of a parser with add_request_flags) asks for, flags by their option strings: ``given`` -- the flags it names;
    ``on`` -- those whose value is not neutral; ``groups`` -- the groups these switch on ("stop" for --stop / --stop-id)."""
    on = {f.option for _, d, f in FLAGS if f.on(getattr(args, f.dest), d)}
    return SimpleNamespace(on=on, given={f.option for _, d, f in FLAGS if f.given(getattr(args, f.dest), d)},
                           groups={g for g, _, f in FLAGS if f.leads and f.option in on})


def check_truncation_flags(ap, args) -> bool:
    """The exclusivity rule of the engine (tl_engine_set_mirostat), raised before anything is loaded; True when a truncation flag is set."""
    flags = switched(args)
    if "--mirostat-tau" in flags.on and flags.on & {"--sampler-top-k", "--sampler-top-p", "--sampler-min-p", "--sampler-typical-p"}:
        ap.error("Mirostat excludes every other truncation (--sampler-top-k, --sampler-top-p, --sampler-min-p, --sampler-typical-p)")
    return "truncation" in flags.groups


def sampling_dict(args, tokenizer, groups) -> dict:
    """The ``sampling`` dict of the flags' values for ``groups`` (switched(args).groups: a neutral group contributes nothing): the keys of
    sampling (but the seed, which goes as base_seed or generate's own), truncation -- only where the request samples --, penalties and dry,
    whose --dry-breaker strings become ids under ``tokenizer``.  A grammar, an adapter and a stop set need an engine: the scripts add those."""
    groups = set(groups) & {"sampling", "penalties", "dry"} | ({"truncation"} if {"sampling", "truncation"} <= set(groups) else set())
    out = {s.key: getattr(args, s.flags[0].dest) for s in SETTINGS if s.group in groups and s.key != "seed"}
    if "dry_breakers" in out:
        out["dry_breakers"] = tuple(dry_breaker_ids(tokenizer, out["dry_breakers"]))
    return out


def dry_settings(args, tokenizer) -> dict:
    """The --dry-* / --no-repeat-ngram flags as the keys of engine.generate / a sampling dict ({} when both are off)."""
    return sampling_dict(args, tokenizer, switched(args).groups & {"dry"})


def chat_prompt(tokenizer, text: str, enable_thinking: bool) -> str:
    messages = [{"role": "system", "content": "You are a helpful assistant."}, {"role": "user", "content": text}]
    return tokenizer.apply_chat_template(messages, tokenize=False, add_generation_prompt=True, enable_thinking=enable_thinking)
