"""A recording engine and the scenarios behind tests/golden/scheduler_traces.json (tests/test_scheduler_traces_cpu.py).

``RecordingEngine`` is benches/serving.py's ScheduleOnlyEngine with a log: every call a scheduler makes, with its arguments and (for
the calls that answer) its result, in order.  It scripts what the real engine would decide -- the ids a slot produces, the stop state
of an armed slot (which freezes inside a multi-step block), log-probability records that name their token -- so that a trace pins a
front-end's whole behaviour: ``batch_generate_ids`` and ``serve_requests`` with 1, 2 and 16 staging slots.

``scenarios()`` returns {name: thunk}; a thunk runs one scenario on a fresh engine and returns {"calls", "result", "error"} in JSON's
value types.  tests/golden/make_scheduler_traces.py wrote the fixture from these thunks at the commit named in the file; the test runs
the same thunks through the code under test and compares.
"""

from __future__ import annotations

import dataclasses
import json
from types import SimpleNamespace

from benches.serving import ScheduleOnlyEngine, serve_requests

VOCAB = 1000


def produced_id(context_sum: int, k: int) -> int:
    """The k-th id (k = 1, 2, ...) of a sequence whose prompt tokens sum to ``context_sum``."""
    return (context_sum * 7 + 3 * k) % 991 + 5


def plain(x):
    """``x`` in JSON's value types: a scripted object by its name, a mapping as sorted pairs."""
    if hasattr(x, "name") and not isinstance(x, (str, bytes)):
        return f"<{x.name}>"
    if isinstance(x, dict):
        return [[plain(k), plain(v)] for k, v in sorted(x.items())]
    if isinstance(x, (list, tuple, set)):
        return [plain(v) for v in (sorted(x) if isinstance(x, set) else x)]
    return x


def fake_stop_set(name: str):
    """A StopSet that never saw the library: the schedulers only pass it on (request_stops checks its type)."""
    from tiny_llm_hip.stop import StopSet

    s = StopSet.__new__(StopSet)
    s.ids, s.strings, s.vocab, s._h, s.name = [1], [], None, None, name
    return s


def fake_grammar(name: str, eos_ids):
    from tiny_llm_hip.engine import Grammar

    g = Grammar.__new__(Grammar)
    g._h, g.eos_ids, g.name = None, tuple(eos_ids), name
    return g


class RecordingEngine(ScheduleOnlyEngine):
    def __init__(self, slots: int, page_size: int = 16, stop_at: dict | None = None, **kw):
        """``stop_at``: {first prompt token: generated count at which the request's stop set matches (reason "id")}; an armed slot
        without an entry stops at its budget (reason "length")."""
        super().__init__(slots, page_size=page_size, **kw)
        self.max_batch, self.vocab_size = slots, VOCAB
        self.calls: list = []
        self.seq: list = [None] * slots  # per live slot: {"first", "sum", "n", "stop": None | {"budget", "reason"}}
        self.stop_at = dict(stop_at or {})

    def _log(self, name, *args, result=None):
        self.calls.append([name, *plain(args)] + ([] if result is None else ["->", plain(result)]))

    # ---- what a slot produces ---------------------------------------------------------------------------------------------
    def _fed(self, slot, tokens):
        s = self.seq[slot]
        if s["first"] is None and len(tokens) > 0:
            s["first"] = int(tokens[0])
        s["sum"] += sum(int(t) for t in tokens)

    def _produce(self, slot):
        s = self.seq[slot]
        st = s["stop"]
        if st is not None and st["reason"] != "none":
            return  # frozen at its stopping token
        s["n"] += 1
        if st is not None:
            if self.stop_at.get(s["first"]) == s["n"]:
                st["reason"] = "id"
            elif st["budget"] and s["n"] >= st["budget"]:
                st["reason"] = "length"

    def _ids(self, slot, count):
        s = self.seq[slot]
        return [produced_id(s["sum"], k) for k in range(s["n"] - count + 1, s["n"] + 1)]

    # ---- the slot interface, logged ---------------------------------------------------------------------------------------
    def begin(self, slot):
        self._log("begin", slot)
        super().begin(slot)
        self.seq[slot] = {"first": None, "sum": 0, "n": 0, "stop": None}

    def release(self, slot):
        self._log("release", slot)
        super().release(slot)
        self.seq[slot] = None

    def move(self, src, dst):
        self._log("move", src, dst, *(["parked"] if src in self.parked_slots else []))
        super().move(src, dst)
        self.seq[dst], self.seq[src] = self.seq[src], None

    def park(self, slot):
        self._log("park", slot)
        super().park(slot)

    def unpark(self, slot):
        self._log("unpark", slot)
        super().unpark(slot)

    def is_parked(self, slot):
        out = super().is_parked(slot)
        self._log("is_parked", slot, result=out)
        return out

    def step_pages(self, batch=None):
        out = super().step_pages(batch)
        self._log("step_pages", batch, result=out)
        return out

    def context_len(self, slot):
        out = super().context_len(slot)
        self._log("context_len", slot, result=out)
        return out

    def swap_stats(self):
        out = super().swap_stats()
        self._log("swap_stats", result=out)
        return out

    def stats(self):
        self._log("stats")
        return super().stats()

    def synchronize(self):
        self._log("synchronize")

    def step_bytes(self, batch=None):
        out = super().step_bytes(batch)
        self._log("step_bytes", batch, result=out)
        return out

    def prefix_attach(self, slot, tokens):
        matched = super().prefix_attach(slot, tokens)
        self._log("prefix_attach", slot, list(tokens), result=matched)
        self._fed(slot, list(tokens)[:matched])
        return matched

    def prefix_extend(self, slot, tokens):
        self._log("prefix_extend", slot, list(tokens))
        super().prefix_extend(slot, tokens)

    def prefill(self, slot, tokens, chunk=None, want_logits=True):
        self._log("prefill", slot, list(tokens), chunk, bool(want_logits))
        super().prefill(slot, tokens, chunk, want_logits)
        self._fed(slot, tokens)
        if want_logits:
            self._produce(slot)

    def prefill_packed(self, chunks):
        self._log("prefill_packed", [[s, list(t), bool(last)] for s, t, last in chunks])
        super().prefill_packed(chunks)
        for slot, tokens, last in chunks:
            self._fed(slot, tokens)
            if last:
                self._produce(slot)

    def decode(self, steps, batch=None):
        self._log("decode", steps, batch)
        super().decode(steps, batch)
        for i in range(batch):
            if self.seq[i] is not None and i not in self.parked_slots:
                for _ in range(steps):
                    self._produce(i)

    def read_tokens(self, slot, count):
        out = self._ids(slot, count)
        self._log("read_tokens", slot, count, result=out)
        return out

    def read_pending(self, count=None):
        out = [self._ids(i, 1)[0] if self.seq[i] is not None else -1 for i in range(count)]
        self._log("read_pending", count, result=out)
        return out

    def read_logprobs(self, slot, count):
        out = [("lp", t) for t in self._ids(slot, count)]
        self._log("read_logprobs", slot, count, result=out)
        return out

    def read_pending_logprobs(self, count=None):
        out = [("lp", self._ids(i, 1)[0]) if self.seq[i] is not None else ("lp", -1) for i in range(count)]
        self._log("read_pending_logprobs", count, result=out)
        return out

    def stop_state(self, slot):
        from tiny_llm_hip.stop import StopState

        s = self.seq[slot]
        st = StopState(s["stop"]["reason"] if s["stop"] else "none", 0, s["n"], self.slots[slot], 0, 0)
        self._log("stop_state", slot, result=[st.reason, st.generated])
        return st

    # ---- per-slot settings: logged, and what the script needs of them kept ------------------------------------------------
    def set_stop(self, slot, stop=None, max_new_tokens=0):
        self._log("set_stop", slot, stop, max_new_tokens)
        self.seq[slot]["stop"] = {"budget": max_new_tokens, "reason": "none"}

    def set_lora(self, slot, adapter):
        self._log("set_lora", slot, adapter)

    def set_sampling(self, slot, *args):
        self._log("set_sampling", slot, *args)

    def set_truncation(self, slot, *args):
        self._log("set_truncation", slot, *args)

    def set_mirostat(self, slot, *args):
        self._log("set_mirostat", slot, *args)

    def set_penalties(self, slot, *args):
        self._log("set_penalties", slot, *args)

    def set_logit_bias(self, slot, bias):
        self._log("set_logit_bias", slot, bias)

    def set_grammar(self, slot, grammar):
        self._log("set_grammar", slot, grammar)

    def set_logprobs(self, slot, top_n):
        self._log("set_logprobs", slot, top_n)

    def set_dry(self, slot, *args):
        self._log("set_dry", slot, *args)


def trace(eng: RecordingEngine, call) -> dict:
    """Run ``call()`` and return what it did to ``eng`` and what came of it, as JSON would hand it back."""
    result, error = None, None
    try:
        result = call()
    except (ValueError, RuntimeError, TypeError) as exc:
        error = f"{type(exc).__name__}: {exc}"
    if dataclasses.is_dataclass(result):
        result = dataclasses.asdict(result)
    return json.loads(json.dumps({"calls": eng.calls, "result": plain(result), "error": error}))


STAGING = (1, 2, 16)  # serve_requests: the reference's one-at-a-time admission, packed admission, the packed pass's 16-slot limit


def _batch(prompts, limits, batch, step, eng_kw=None, on_step=False, **kw):
    def run():
        from tiny_llm_hip.engine import batch_generate_ids

        eng = RecordingEngine(batch + 1, **(eng_kw or {}))
        if on_step:
            kw["on_step"] = lambda active: eng._log("on_step", active)
        return trace(eng, lambda: batch_generate_ids(eng, prompts, limits, batch_size=batch, prefill_step=step, **kw))

    return run


def _serve(prompts, limits, batch, step, staging, eng_kw=None, loras=None, **kw):
    def run():
        eng = RecordingEngine(batch + min(staging, 16), **(eng_kw or {}))
        reqs = [SimpleNamespace(prompt_token_ids=p, max_new_tokens=n, **({} if loras is None or loras[i] is None else {"lora": loras[i]}))
                for i, (p, n) in enumerate(zip(prompts, limits))]
        return trace(eng, lambda: serve_requests(eng, reqs, batch_size=batch, prefill_step=step, page_size=eng.page_size, clock=eng.clock,
                                                 staging_slots=staging, **kw))

    return run


def _prompts(lengths):
    return [[10 + 3 * i + (j % 5) for j in range(n)] for i, n in enumerate(lengths)]


def scenarios() -> dict:
    out = {}

    def both(name, prompts, limits, batch, step, eng_kw=None, batch_kw=None, serve_kw=None):
        out[f"{name}/batch_generate_ids"] = _batch(prompts, limits, batch, step, eng_kw, **(batch_kw or {}))
        for st in STAGING:
            out[f"{name}/serve_requests_{st}"] = _serve(prompts, limits, batch, step, st, eng_kw, **(serve_kw or {}))

    # 1. plain greedy: a prompt shorter than a chunk, one of exactly a chunk, limits of 1 (retired from staging); request 4 produces the eos id
    p1, l1 = _prompts([5, 16, 23, 40, 1, 33, 17]), [3, 1, 4, 2, 5, 1, 6]
    both("1_plain", p1, l1, 3, 16, batch_kw=dict(eos_token_id=produced_id(sum(p1[4]), 3), on_step=True))
    # 2. more requests than slots: prefilled requests wait in staging for a decode slot
    both("2_stall", _prompts([4, 9, 3, 7, 2, 6, 5, 8]), [10, 7, 9, 12, 8, 10, 6, 11], 2, 16)
    # 3. the prefill budget: a short last chunk, then the next request admitted and prefilled in the same turn
    p3, l3 = _prompts([20, 5, 18, 35, 3, 16, 9]), [4, 3, 1, 5, 2, 6, 3]
    for st in STAGING:
        for budget in (16, 64):
            out[f"3_budget_{budget}/serve_requests_{st}"] = _serve(p3, l3, 3, 16, st, prefill_budget=budget)
    # 4. prefix cache on, shared prefixes (tests/test_prefix_cache_schedule_cpu.py)
    shared = list(range(100, 140))
    p4 = [shared + [200 + i, 300 + i, 400 + i] for i in range(6)]
    both("4_prefix_cache", p4, [6] * 6, 3, 16, dict(prefix_cache=True), batch_kw=dict(sampling={"temperature": 0.5}), serve_kw=dict(prefill_budget=32))
    # 5. a tight pool with swap space (tests/test_kv_swap_schedule_cpu.py), and the lone request that does not fit
    p5 = [[1 + i] * 6 for i in range(5)]
    both("5_swap", p5, [12] * 5, 3, 4, dict(page_size=4, num_pages=9, swap_pages=12), serve_kw=dict(prefill_budget=8))
    p5b = [[1 + i] * (3 + 2 * (i % 3)) for i in range(8)]
    both("5_swap_holes", p5b, [5, 14, 3, 16, 4, 12, 9, 15], 4, 4, dict(page_size=4, num_pages=11, swap_pages=16), serve_kw=dict(prefill_budget=8))
    both("5_swap_lone", p5[:1], [12], 3, 4, dict(page_size=4, num_pages=3, swap_pages=8), serve_kw=dict(prefill_budget=8))
    # 6. hole closing: 16 slots, staggered limits (tests/test_host_logic_cpu.py); and serve_requests with compact=False
    p6 = [[i + 1] * (3 + i % 5) for i in range(12)]
    l6 = [2 + (i * 3) % 7 for i in range(12)]
    both("6_holes", p6, l6, 16, 4, serve_kw=dict(prefill_budget=16))
    for st in (1, 2):
        out[f"6_holes_no_compact/serve_requests_{st}"] = _serve(p6, l6, 16, 4, st, prefill_budget=16, compact=False)
    # 7. per-prompt sampling that uses every key, with logprobs; "lora" in its other form (one dict, a list of ids)
    p7 = _prompts([7, 20, 3, 18, 9, 33])
    gram = fake_grammar("grammar", [produced_id(sum(p7[4]), 3), 999])
    every = {"temperature": 1.0, "top_k": 0, "top_p": 1.0, "seed": 11, "min_p": 0.0, "typical_p": 1.0, "mirostat_tau": 4.0, "mirostat_eta": 0.3,
             "repetition_penalty": 1.1, "presence_penalty": 0.2, "frequency_penalty": 0.1, "logit_bias": {5: 1.0, 2: -4.0}, "grammar": gram, "lora": 1}
    s7 = [{"temperature": 0.8, "top_k": 40, "top_p": 0.9, "seed": 7}, {"temperature": 1.0, "min_p": 0.05, "typical_p": 0.9}, every,
          {"repetition_penalty": 1.2, "logit_bias": {3: -5.0}}, {"grammar": gram, "lora": 2}, {}]
    out["7_sampling_list/batch_generate_ids"] = _batch(p7, [4, 3, 5, 1, 6, 4], 3, 16, sampling=s7, logprobs=2, base_seed=100)
    out["7_sampling_one_dict/batch_generate_ids"] = _batch(p7, 4, 3, 16, sampling={"temperature": 0.7, "presence_penalty": 0.5, "lora": [0, None, 1, -1, 0, 2]},
                                                          logprobs=0, base_seed=5)
    # 8. stop conditions on the device: request 1 stops on its set inside a block, the others at their budgets (one in staging)
    p8 = _prompts([6, 19, 4, 11])
    stop_at = {p8[1][0]: 6, p8[2][0]: 2}
    sets = [fake_stop_set("stop_a"), fake_stop_set("stop_b"), None, fake_stop_set("stop_a")]
    for block in (1, 4):
        out[f"8_stop_block_{block}/batch_generate_ids"] = _batch(p8, [9, 12, 1, 7], 3, 16, dict(stop_at=stop_at), on_step=True, stop=sets, decode_block=block,
                                                                 logprobs=1)
    out["8_stop_one_set/batch_generate_ids"] = _batch(p8, 5, 2, 16, dict(stop_at=stop_at), stop=sets[0], decode_block=4)
    # 9. serve_requests with requests that carry a ``lora`` attribute
    for st in STAGING:
        out[f"9_lora/serve_requests_{st}"] = _serve(_prompts([5, 5, 20, 3, 17, 8]), [3, 1, 4, 3, 2, 5], 4, 16, st, loras=[0, None, 1, 1, -1, 0])
    # 10. every argument check of batch_generate_ids (serve_requests has none): the error's text, before any engine call
    p10 = _prompts([4, 6])
    bad = {"decode_block_type": dict(decode_block=True), "decode_block_zero": dict(decode_block=0, stop=sets[0]), "decode_block_without_stop": dict(decode_block=2),
           "stop_and_eos": dict(stop=sets[0], eos_token_id=3), "stop_length": dict(stop=[sets[0]]), "stop_type": dict(stop=["x", None]),
           "sampling_length": dict(sampling=[{}]), "sampling_entry": dict(sampling=[{}, 3]), "sampling_key": dict(sampling={"temp": 1.0}),
           "temperature": dict(sampling={"temperature": -1.0}), "top_k": dict(sampling={"top_k": -1}), "top_p": dict(sampling=[{}, {"top_p": 2.0}]),
           "seed": dict(sampling={"seed": -1}), "min_p": dict(sampling={"min_p": 2.0}), "typical_p": dict(sampling={"typical_p": 0.0}),
           "mirostat_tau": dict(sampling={"mirostat_tau": -1.0}), "mirostat_eta": dict(sampling={"mirostat_tau": 1.0, "mirostat_eta": 2.0}),
           "mirostat_exclusive": dict(sampling={"temperature": 1.0, "mirostat_tau": 5.0, "top_p": 0.9}), "truncation_type": dict(sampling={"min_p": "x"}),
           "repetition_penalty": dict(sampling={"repetition_penalty": 0.0}), "presence_penalty": dict(sampling={"presence_penalty": float("nan")}),
           "logit_bias_id": dict(sampling={"logit_bias": {VOCAB: 1.0}}), "logit_bias_type": dict(sampling={"logit_bias": [1, 2]}),
           "grammar": dict(sampling={"grammar": "a+"}), "lora_value": dict(sampling={"lora": 32}), "lora_length": dict(sampling={"lora": [0]}),
           "logprobs": dict(logprobs=21), "logprobs_type": dict(logprobs=True)}
    for name, kw in bad.items():
        out[f"10_check_{name}/batch_generate_ids"] = _batch(p10, 3, 2, 16, **kw)
    out["10_check_batch_size/batch_generate_ids"] = _batch(p10, 3, 0, 16)
    out["10_check_prefill_step/batch_generate_ids"] = _batch(p10, 3, 2, 0)

    def too_few_slots():
        from tiny_llm_hip.engine import batch_generate_ids

        eng = RecordingEngine(2)
        return trace(eng, lambda: batch_generate_ids(eng, p10, 3, batch_size=2, prefill_step=16))

    out["10_check_slots/batch_generate_ids"] = too_few_slots
    return out
