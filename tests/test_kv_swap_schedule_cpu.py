"""CPU tier: the preemption policy (tiny_llm_hip/preempt.py) in the three schedulers -- batch_generate_ids, serve_requests one prompt at
a time, serve_requests with packed admission -- against ScheduleOnlyEngine's page pool and swap space (benches/serving.py).

A recording engine notes every call with the pool's state at that moment, so the rules are checked where they are applied:
  victim order   a staging request that holds pages gives way first (released, admitted again before anybody else); only then is a
                 running request parked, and it is the one admitted last;
  resume rule    the oldest parked request first, and only when obtainable >= its pages + one per running request;
  admission      nothing begins while a request is parked;
  old error      one request that cannot fit raises "KV page pool exhausted", swap space or not;
  no pressure    on a pool that never runs short the call trace with swap space is the trace without it."""

from types import SimpleNamespace

import pytest

from benches.serving import ScheduleOnlyEngine, serve_requests

PAGE, BATCH = 4, 3
PROMPTS = [[1 + i] * 6 for i in range(5)]  # 2 pages each
NEW_TOKENS = 12                            # a finished request holds 17 tokens: 5 pages


class Recorder(ScheduleOnlyEngine):
    """ScheduleOnlyEngine that logs (call, arguments, state before the call)."""

    def __init__(self, slots, **kw):
        super().__init__(slots, page_size=PAGE, **kw)
        self.max_batch = slots
        self.vocab_size = 100
        self.calls = []
        self.order = {}      # slot -> admission number of the running request in it
        self.admissions = 0

    def _log(self, name, *args):
        staging = [i for i in range(BATCH, len(self.slots)) if self.slots[i] is not None]
        self.calls.append(SimpleNamespace(
            name=name, args=args, pages=self.step_pages(BATCH), parked=set(self.parked_slots), order=dict(self.order),
            contexts=list(self.slots), staging_tokens=sum(self.slots[i] for i in staging)))

    def begin(self, slot):
        self._log("begin", slot)
        super().begin(slot)

    def prefill(self, slot, tokens, chunk=None, want_logits=True):
        self._log("prefill", slot, len(tokens), tokens[0])
        super().prefill(slot, tokens, chunk, want_logits)

    def prefill_packed(self, chunks):
        self._log("prefill_packed", tuple((c[0], len(c[1]), c[1][0]) for c in chunks))
        super().prefill_packed(chunks)

    def move(self, src, dst):
        self._log("move", src, dst)
        super().move(src, dst)
        if src >= BATCH:
            self.order[dst] = self.admissions
            self.admissions += 1
        else:
            self.order[dst] = self.order.pop(src)

    def decode(self, steps, batch=None):
        self._log("decode", batch)
        super().decode(steps, batch)

    def park(self, slot):
        self._log("park", slot)
        super().park(slot)

    def unpark(self, slot):
        self._log("unpark", slot)
        super().unpark(slot)

    def release(self, slot):
        self._log("release", slot)
        super().release(slot)
        self.order.pop(slot, None)


def run_batch_generate(eng_kw, prompts=PROMPTS, new_tokens=NEW_TOKENS):
    from tiny_llm_hip.engine import batch_generate_ids

    eng = Recorder(BATCH + 1, **eng_kw)
    done = batch_generate_ids(eng, prompts, new_tokens, batch_size=BATCH, prefill_step=PAGE)
    assert sorted(i for i, _ in done) == list(range(len(prompts)))
    assert all(len(out) == new_tokens for _, out in done)
    return eng, None


def run_serve(eng_kw, staging_slots, prompts=PROMPTS, new_tokens=NEW_TOKENS):
    eng = Recorder(BATCH + staging_slots, **eng_kw)
    reqs = [SimpleNamespace(prompt_token_ids=p, max_new_tokens=new_tokens) for p in prompts]
    m = serve_requests(eng, reqs, batch_size=BATCH, prefill_step=PAGE, prefill_budget=2 * PAGE, page_size=PAGE, clock=eng.clock,
                       staging_slots=staging_slots)
    assert m.generated_tokens == len(prompts) * new_tokens
    return eng, m


SCHEDULERS = {"batch_generate_ids": run_batch_generate, "serve_requests": lambda kw, **a: run_serve(kw, 1, **a),
              "serve_requests_packed": lambda kw, **a: run_serve(kw, 2, **a)}
# three requests of 5 pages want 15: 9 pages run short once two are long, and the third is still being admitted
TIGHT = dict(num_pages=9, swap_pages=12)


@pytest.fixture(scope="module", params=sorted(SCHEDULERS))
def tight(request):
    eng, metrics = SCHEDULERS[request.param](TIGHT)
    return eng, metrics


def pages(tokens):
    return (tokens + PAGE - 1) // PAGE


def test_pressure_is_answered_by_preemption_and_everything_is_freed(tight):
    eng, metrics = tight
    names = [c.name for c in eng.calls]
    assert "park" in names and "unpark" in names
    assert names.count("park") == names.count("unpark")  # every parked request came back
    assert all(s is None for s in eng.slots) and not eng.parked_slots
    stats = eng.swap_stats()
    assert stats["host_pages_in_use"] == 0 and stats["pages_out"] == stats["pages_in"] > 0
    if metrics is not None:
        requeued = sum(1 for c in eng.calls if c.name == "release" and c.args[0] >= BATCH and c.contexts[c.args[0]] < len(PROMPTS[0]) + 1
                       and c.pages[0] > c.pages[1])
        assert metrics.preemptions == names.count("park") + metrics.recomputed and metrics.recomputed >= requeued
        assert metrics.pages_swapped == stats["pages_out"] + stats["pages_in"]


def test_the_victim_is_the_staging_request_first_then_the_running_request_admitted_last(tight):
    eng, _ = tight
    for c in (c for c in eng.calls if c.name == "park"):
        need, obtainable = c.pages
        assert need > obtainable                      # only under pressure
        assert c.staging_tokens == 0                  # a staging request that held pages had given way before
        running = {s: n for s, n in c.order.items() if s not in c.parked}
        assert len(running) >= 2                      # the last running request is never parked
        assert c.args[0] == max(running, key=running.get)
    # a staging request that gives way is released under pressure while it holds pages, and its prompt is the next one to begin
    def prompt_in(slot, calls):  # the prompt (by its first token) of the last chunk prefilled into `slot`
        for c in reversed(calls):
            if c.name == "prefill" and c.args[0] == slot:
                return c.args[2]
            if c.name == "prefill_packed":
                for st, _, first in c.args[0]:
                    if st == slot:
                        return first
        return None

    calls = eng.calls
    for k, c in enumerate(calls):
        if not (c.name == "release" and c.args[0] >= BATCH):
            continue
        assert c.pages[0] > c.pages[1] or (c.parked and not any(s not in c.parked for s in c.order))  # under pressure, or to let a parked one resume
        assert c.contexts[c.args[0]] > 0
        gave_way = prompt_in(c.args[0], calls[:k])
        begin = next(j for j in range(k + 1, len(calls)) if calls[j].name == "begin")
        slot = calls[begin].args[0]
        stop = next(j for j in range(begin + 1, len(calls)) if calls[j].name in ("release", "move") and calls[j].args[0] == slot)
        assert prompt_in(slot, calls[begin + 1:stop]) == gave_way  # the first chunks into the slot begun next are that prompt's


def test_resume_is_oldest_first_and_leaves_a_page_per_running_request(tight):
    eng, _ = tight
    for c in (c for c in eng.calls if c.name == "unpark"):
        slot = c.args[0]
        assert c.order[slot] == min(c.order[s] for s in c.parked)
        running = sum(1 for s in c.order if s not in c.parked)
        assert c.pages[1] >= pages(c.contexts[slot]) + running


def test_nothing_is_admitted_while_a_request_is_parked(tight):
    eng, _ = tight
    assert all(not c.parked for c in eng.calls if c.name == "begin")


@pytest.mark.parametrize("scheduler", sorted(SCHEDULERS))
@pytest.mark.parametrize("swap", [0, 8])
def test_a_single_request_that_cannot_fit_raises_the_old_error(scheduler, swap):
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        SCHEDULERS[scheduler](dict(num_pages=3, swap_pages=swap), prompts=PROMPTS[:1])  # 17 tokens want 5 pages


@pytest.mark.parametrize("scheduler", sorted(SCHEDULERS))
def test_without_swap_space_a_short_pool_still_fails_as_before(scheduler):
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        SCHEDULERS[scheduler](dict(num_pages=TIGHT["num_pages"]))


@pytest.mark.parametrize("scheduler", sorted(SCHEDULERS))
def test_a_pool_that_never_runs_short_sees_the_same_calls_with_and_without_swap_space(scheduler):
    def trace(kw):
        eng, metrics = SCHEDULERS[scheduler](kw)
        return [(c.name, c.args) for c in eng.calls], eng.now, metrics

    plain, t_plain, m_plain = trace(dict(num_pages=64))
    swap, t_swap, m_swap = trace(dict(num_pages=64, swap_pages=16))
    assert swap == plain and t_swap == t_plain
    assert not any(name in ("park", "unpark") for name, _ in swap)
    if m_swap is not None:
        assert (m_swap.preemptions, m_swap.recomputed, m_swap.pages_swapped) == (0, 0, 0)
        assert m_swap.turns == m_plain.turns and m_swap.prefill_chunks == m_plain.prefill_chunks
