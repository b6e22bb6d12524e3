"""CPU tier: the three schedulers -- batch_generate_ids, serve_requests one prompt at a time, serve_requests with packed admission --
use the prefix cache the way include/tinyllm_engine.h "Prefix cache" asks: one attach per request, after its settings and before its
first chunk; chunks start at the matched offset; the fed answer tokens are declared before the release; and with the cache off the
call sequence is what it was.  The engine is ScheduleOnlyEngine (a page-granular model of the cache) behind a recorder."""

from types import SimpleNamespace

import pytest

from benches.serving import ScheduleOnlyEngine, serve_requests

PAGE = 16
SHARED = list(range(100, 140))                      # 40 tokens: two full pages and half of a third
PROMPTS = [SHARED + [200 + i, 300 + i, 400 + i] for i in range(6)]
NEW_TOKENS = 6                                      # 43 prompt tokens + 5 fed answer tokens fill the third page


class Recorder:
    """Every call the scheduler makes, in order, passed on to a ScheduleOnlyEngine; produced ids are 7, 8, 9, ... per slot."""

    def __init__(self, slots, cache):
        self.inner = ScheduleOnlyEngine(slots, prefix_cache=cache, page_size=PAGE)
        self.prefix_cache_enabled = cache
        self.max_batch, self.vocab_size = slots, 1000
        self.calls = []
        self.produced = [0] * slots

    def begin(self, slot):
        self.calls.append(("begin", slot))
        self.produced[slot] = 0
        self.inner.begin(slot)

    def set_sampling(self, slot, *args):
        self.calls.append(("settings", slot))

    def prefix_attach(self, slot, tokens):
        matched = self.inner.prefix_attach(slot, tokens)
        self.calls.append(("attach", slot, tuple(tokens), matched))
        return matched

    def prefix_extend(self, slot, tokens):
        self.calls.append(("extend", slot, tuple(tokens)))
        self.inner.prefix_extend(slot, tokens)

    def prefill(self, slot, tokens, chunk=None, want_logits=True):
        self.calls.append(("prefill", slot, tuple(tokens), bool(want_logits)))
        self.inner.prefill(slot, tokens)
        self.produced[slot] += bool(want_logits)

    def prefill_packed(self, chunks):
        for slot, tokens, last in chunks:
            self.calls.append(("prefill", slot, tuple(tokens), bool(last)))
            self.produced[slot] += bool(last)
        self.inner.prefill_packed(chunks)

    def move(self, src, dst):
        self.calls.append(("move", src, dst))
        self.inner.move(src, dst)
        self.produced[dst], self.produced[src] = self.produced[src], 0

    def decode(self, steps, batch=None):
        self.calls.append(("decode", batch))
        self.inner.decode(steps, batch=batch)
        for i in range(batch):
            if self.inner.slots[i] is not None:
                self.produced[i] += steps

    def read_tokens(self, slot, count):
        return [6 + self.produced[slot]] * count

    def read_pending(self, count=None):
        return [6 + self.produced[i] for i in range(count)]

    def release(self, slot):
        self.calls.append(("release", slot))
        self.inner.release(slot)

    def synchronize(self):
        pass

    def stats(self):
        return self.inner.stats()


def run_batch_generate(cache):
    from tiny_llm_hip.engine import batch_generate_ids

    eng = Recorder(4, cache)
    done = batch_generate_ids(eng, PROMPTS, NEW_TOKENS, batch_size=3, prefill_step=PAGE, sampling={"temperature": 0.5})
    assert sorted(i for i, _ in done) == list(range(len(PROMPTS)))
    assert all(out == [7, 8, 9, 10, 11, 12] for _, out in done)
    return eng


def run_serve(cache, staging_slots):
    eng = Recorder(3 + staging_slots, cache)
    reqs = [SimpleNamespace(prompt_token_ids=p, max_new_tokens=NEW_TOKENS) for p in PROMPTS]
    m = serve_requests(eng, reqs, batch_size=3, prefill_step=PAGE, prefill_budget=2 * PAGE, page_size=PAGE, clock=eng.inner.clock,
                       staging_slots=staging_slots)
    assert m.generated_tokens == len(PROMPTS) * NEW_TOKENS
    return eng


SCHEDULERS = {"batch_generate_ids": run_batch_generate, "serve_requests": lambda cache: run_serve(cache, 1),
              "serve_requests_packed": lambda cache: run_serve(cache, 2)}


def lifetimes(calls):
    """The calls of each request, in order: from a begin until the release of the slot the request then lives in."""
    where, out = {}, []
    for c in calls:
        kind = c[0]
        if kind == "begin":
            where[c[1]] = [c]
            continue
        if kind == "decode":
            continue
        if kind == "move":
            where[c[2]] = where.pop(c[1]) + [c]
            continue
        where[c[1]].append(c)
        if kind == "release":
            out.append(where.pop(c[1]))
    assert not where
    return out


@pytest.mark.parametrize("name", list(SCHEDULERS))
def test_cache_on_attaches_once_prefills_from_the_match_and_declares_the_answer(name):
    eng = SCHEDULERS[name](True)
    lives = lifetimes(eng.calls)
    assert len(lives) == len(PROMPTS)
    hits = 0
    for life in lives:
        kinds = [c[0] for c in life]
        assert kinds.count("attach") == 1 and kinds.count("extend") == 1 and kinds[0] == "begin" and kinds[-1] == "release"
        attach = kinds.index("attach")
        first_chunk = kinds.index("prefill")
        assert attach < first_chunk                                   # before the first chunk ...
        if "settings" in kinds:
            assert kinds.index("settings") < attach                   # ... and after the request's settings
        _, _, prompt, matched = life[attach]
        assert 0 <= matched <= len(prompt) - 1
        chunks = [c for c in life if c[0] == "prefill"]
        fed = [t for c in chunks for t in c[2]]
        assert fed == list(prompt[matched:])                          # chunks start at `matched`, nothing is prefilled twice
        assert [c[3] for c in chunks] == [False] * (len(chunks) - 1) + [True]
        assert kinds[-2] == "extend"                                  # the answer is declared right before the release
        assert life[-2][2] == (7, 8, 9, 10, 11)                               # out[:-1]: the last produced token was never fed
        hits += matched > 0
    matched_all = [life[[c[0] for c in life].index("attach")][3] for life in lives]
    # the first request finds nothing; every request admitted after its shared pages were published finds the two full pages and, once
    # a third page is cached, the 8 shared tokens of it as well
    assert matched_all[0] == 0 and hits >= len(PROMPTS) - 3 and max(matched_all) == len(SHARED)
    assert all(m in (0, 2 * PAGE, len(SHARED)) for m in matched_all), matched_all
    stats = eng.inner.prefix_stats()
    assert stats["lookups"] == len(PROMPTS) and stats["tokens_matched"] == sum(matched_all)
    # the virtual clock's prefill work: only the tokens actually prefilled
    assert eng.inner.prefilled_tokens == sum(len(p) for p in PROMPTS) - sum(matched_all)


@pytest.mark.parametrize("name", list(SCHEDULERS))
def test_cache_off_keeps_the_call_sequence(name):
    eng = SCHEDULERS[name](False)
    kinds = {c[0] for c in eng.calls}
    assert "attach" not in kinds and "extend" not in kinds
    for life in lifetimes(eng.calls):
        chunks = [c for c in life if c[0] == "prefill"]
        assert [t for c in chunks for t in c[2]] == PROMPTS[0][:len(SHARED)] + list(chunks[-1][2][-3:])
    assert eng.inner.prefilled_tokens == sum(len(p) for p in PROMPTS)

    class Bare:  # an engine that has never heard of the cache (no attribute, no methods) is served as before
        def __init__(self, inner):
            self._inner = inner

        def __getattr__(self, item):
            if item.startswith("prefix"):
                raise AttributeError(item)
            return getattr(self._inner, item)

    bare = Recorder(5, False)
    reqs = [SimpleNamespace(prompt_token_ids=p, max_new_tokens=NEW_TOKENS) for p in PROMPTS]
    serve_requests(Bare(bare), reqs, batch_size=3, prefill_step=PAGE, prefill_budget=2 * PAGE, page_size=PAGE, clock=bare.inner.clock, staging_slots=2)
    same = run_serve(False, 2)
    assert bare.calls == same.calls


def test_follow_up_turn_finds_prompt_and_answer():
    """Retirement declares out[:-1]: a second turn whose prompt is the first prompt + its answer + new text matches all of it but
    what lies in the last, partly filled page beyond the cached rows."""
    eng = ScheduleOnlyEngine(3, prefix_cache=True, page_size=4)

    class R(SimpleNamespace):
        pass

    first = list(range(50, 61))  # 11 tokens
    serve_requests(eng, [R(prompt_token_ids=first, max_new_tokens=6)], batch_size=2, prefill_step=8, page_size=4, clock=eng.clock)
    # the slot held 11 prompt tokens + 5 fed answer tokens (ids 0 in the model) = 16 = four full pages, all declared
    turn2 = first + [0] * 5 + [70, 71, 72]
    eng.begin(0)
    assert eng.prefix_attach(0, turn2) == 16
    eng.release(0)
