"""Continuous batching: the one scheduler behind ``engine.batch_generate_ids`` and benches/serving.py's ``serve_requests``.

Pure host logic over the engine's duck-typed slot interface (``begin`` / ``prefill`` / ``prefill_packed`` / ``move`` / ``decode`` /
``release``, ``prefix_attach`` / ``prefix_extend`` with a prefix cache, what tiny_llm_hip.preempt asks with swap space; DecodeEngine,
or benches/serving.py's ScheduleOnlyEngine): no torch, no device.  Decode slots are [0, batch_size), staging slots follow them.

One turn of ``Scheduler.run``:

  stage     admit waiting requests into free staging slots (``begin``, the front-end's settings, ``prefix_attach``), prefill, and let
            every request whose prompt is in the cache leave staging: retired if it is already finished, else moved into the lowest
            free decode slot -- or it waits for one.  Two admission policies: ``_stage_one`` (the reference's, one request at a time
            through ``engine.prefill``; batch.py:48-76) and ``_stage_packed`` (several staged prompts' chunks in one
            ``engine.prefill_packed`` pass).  One staging slot is the ``staged`` list with at most one entry.
  preempt   ``Preemption.before_step`` resumes parked requests and makes room for the step; a staged request that has to give way is
            released and put at the front of the queue (``_requeue``).
  compact   ``close_holes``.
  step      one decode call over the row bucket of the occupied prefix, then collect and retire (``prefix_extend``, ``release``).

and a ``finally`` that releases every slot still live.

What the two front-ends differ in is the ``Frontend`` below, and nowhere else: each difference is one attribute or one hook, with the
reason beside it.  None of them is decided here: a step's arithmetic follows its row count, so even the row rule can move token ids.
"""

from __future__ import annotations

from .preempt import Preemption
from .request import RequestSettings  # noqa: F401  (what a front-end's ``admit`` applies; benches/serving.py takes it from here)

# decode row counts the schedulers use: exact up to 4 rows (fused GEMV), then the row-block sizes of the skinny matmul; the engine
# keeps one captured graph per row count, and the buckets bound their number
ROW_BUCKETS = (1, 2, 3, 4, 8, 16, 32, 48, 64, 96, 128, 192, 256)

parked = Preemption.parked


def row_bucket(n: int, batch_size: int) -> int:
    return min(next((b for b in ROW_BUCKETS if b >= n), batch_size), batch_size)


def close_holes(engine, slots: list, live: set) -> None:
    """Move the highest live decode slots into the holes finished requests left, when that lowers the step's row bucket.

    The engine decodes the occupied PREFIX of the slots and a step's cost follows its row count (a staircase in 16-row blocks:
    17-32 rows 1.77 ms, 33-64 rows 2.5 ms on the Qwen3-4B shape); with holes, 27 live requests spread over 48 slots pay for 48
    rows.  A move hands over a block-table row, a context length and the pending token (tl_engine_move: no K/V byte moves; a parked
    slot's host records move with it).  The reference decodes all ``batch_size`` rows of its batch cache every step
    (batch.py:136-285): slot numbers are invisible to it, to the results and to every counter of the report."""
    count = sum(s is not None for s in slots)
    top = max((i for i, s in enumerate(slots) if s is not None), default=-1)
    if count == 0 or row_bucket(count, len(slots)) >= row_bucket(top + 1, len(slots)):
        return
    lo, hi = 0, len(slots) - 1
    while True:
        while lo < hi and slots[lo] is not None:
            lo += 1
        while hi > lo and slots[hi] is None:
            hi -= 1
        if lo >= hi:
            return
        engine.move(hi, lo)
        slots[lo], slots[hi] = slots[hi], None
        live.discard(hi)
        live.add(lo)


class Frontend:
    """What a front-end decides and what it sees: the seam of ``Scheduler``.  A request's state is a dict the scheduler makes --
    ``req`` (what the front-end queued), ``staging`` (its staging slot), ``tokens`` (the prompt), ``offset`` (prompt tokens in the
    cache) and ``out`` (produced ids, which ``prefix_extend`` declares at retirement) -- and the front-end adds its own keys."""

    # Chunks per turn.  None: exactly one pass of ``_stage_one`` -- admit, ONE chunk, leave staging -- the reference scheduler's turn,
    # which batch_generate_ids promises.  An int: a turn spends up to that many prompt tokens, and after a short last chunk goes on to
    # adopt, admit the next request and prefill its first chunk (on an MI355X one chunk per turn starves a 64-slot batch).
    prefill_budget: int | None = None
    # Rows of a step.  True: the bucket of the highest OCCUPIED slot, parked ones included (batch_generate_ids).  False: of the highest
    # slot that runs (serve_requests).  Not unified: the ids of a step follow its row count, and both front-ends' ids are pinned by tests.
    rows_cover_parked = False
    # Steps per decode call: above 1 only where the device decides when a request is finished (batch_generate_ids with stop=), and
    # only while nothing waits to be admitted, staged or resumed -- a slot that stops inside the block freezes at its stopping token.
    decode_block = 1
    # False leaves the holes open (serve_requests(compact=False): the A/B switch of the hole-closing measurement).
    compact = True

    def admit(self, slot: int, state: dict) -> None:
        """The request ``state["req"]`` has just begun in ``slot``: apply its settings, set ``state["tokens"]``."""
        raise NotImplementedError

    def before_prefill(self) -> None:
        """A prefill pass is about to be issued (measurement: serve_requests starts its timer)."""

    def prefilled(self, chunks: list) -> None:
        """The pass over ``chunks`` = [(state, tokens fed, ends the prompt)] was issued: read back what the front-end keeps of a
        request's first token; measurement."""

    def finished_in_staging(self, slot: int, state: dict) -> bool:
        """Is the request, prefilled and still in its staging slot, already finished (it then never enters the batch)?"""
        raise NotImplementedError

    def before_step(self, rows: int) -> None:
        """A decode call over ``rows`` rows is about to be issued (measurement)."""

    def stepped(self, rows: int, active: list, steps: int) -> None:
        """The decode call was issued over the running slots ``active``: read back what the front-end needs after a step
        (batch_generate_ids: the pending ids, every step; serve_requests: only what the prefix cache must be told); measurement."""

    def collect(self, slot: int, state: dict) -> bool:
        """After ``stepped``, per running slot in slot order: take the slot's new tokens; is the request finished?
        (batch_generate_ids: the host's limit / EOS comparison, or the device's stop state; serve_requests: a token count.)"""
        raise NotImplementedError

    def requeued(self, state: dict) -> None:
        """A staged request gave way to page pressure and will be prefilled again (measurement: its tokens are not counted twice)."""

    def idle(self) -> None:
        """A turn without a decode step (measurement: idle time is not a completion gap)."""


class Scheduler:
    def __init__(self, engine, frontend: Frontend, requests, *, batch_size: int, prefill_step: int, staging_slots: int = 1):
        self.engine, self.frontend, self.requests = engine, frontend, requests
        self.batch_size, self.prefill_step = batch_size, prefill_step
        self.cached = bool(getattr(engine, "prefix_cache_enabled", False))
        self.pre = Preemption(engine)  # (every answer is "go ahead" on an engine without swap space)
        self.slots: list[dict | None] = [None] * batch_size  # running requests by decode slot
        self.staged: list[dict] = []                         # admission order; each state holds its staging slot
        self.free_staging = list(range(batch_size, batch_size + min(staging_slots, 16)))  # (a packed pass takes 16 chunks)
        self.next_idx = 0
        self.front: list = []        # requests a preemption put back: they are admitted before requests[next_idx]
        self.live: set[int] = set()  # every slot that holds a sequence: released in run's finally
        self.finished: list[dict] = []  # retired requests' states, in retirement order
        self.turns = 0

    def waiting(self) -> bool:
        return bool(self.front) or self.next_idx < len(self.requests)

    def run(self) -> None:
        stage = self._stage_packed if len(self.free_staging) > 1 else self._stage_one
        slots, pre = self.slots, self.pre
        try:
            while self.waiting() or self.staged or any(s is not None for s in slots):
                self.turns += 1
                stage()
                if pre.active and any(s is not None for s in slots):
                    pre.before_step(slots, lambda: self.batch_size, [(p["staging"], p) for p in self.staged], self._requeue)
                self._step()
        finally:
            for slot in list(self.live):
                try:
                    self.engine.release(slot)
                except RuntimeError:
                    pass

    # ---- staging ----------------------------------------------------------------------------------------------------------
    def _admit(self) -> None:
        slot = self.free_staging.pop(0)
        self.engine.begin(slot)
        self.live.add(slot)
        if self.front:
            request = self.front.pop(0)
        else:
            request = self.requests[self.next_idx]
            self.next_idx += 1
        state = {"req": request, "staging": slot, "offset": 0, "out": []}
        self.frontend.admit(slot, state)
        if self.cached and len(state["tokens"]) > 0:  # after the settings, before the first chunk: the prompt starts behind the cached prefix
            state["offset"] = self.engine.prefix_attach(slot, state["tokens"])
        self.staged.append(state)

    def _stage_one(self) -> None:
        budget = self.frontend.prefill_budget  # (None: one pass; else passes until the budget is spent or staging stalls)
        while True:
            spent = self._stage_one_pass()
            if spent is None or budget is None:
                return
            budget -= spent
            if budget <= 0:
                return

    def _stage_one_pass(self) -> int | None:
        """Admit if the staging slot is free, prefill one chunk, leave staging if the prompt is complete.  Returns the prompt tokens
        prefilled; None where staging stalls for this turn (decoding goes on, and slots and pages come back)."""
        if not self.staged:
            if not self.waiting() or not self.pre.may_admit(self.slots):
                return None
            self._admit()
        p = self.staged[0]
        spent = 0
        left = len(p["tokens"]) - p["offset"]
        if left > 0:
            if not self.pre.may_prefill(p["staging"], min(self.prefill_step, left), self.slots):
                return None  # the pool cannot hold the chunk yet
            chunk = p["tokens"][p["offset"]:p["offset"] + self.prefill_step]
            spent = len(chunk)
            self.frontend.before_prefill()
            self.engine.prefill(p["staging"], chunk, chunk=spent, want_logits=spent >= left)
            p["offset"] += spent
            self.frontend.prefilled([(p, spent, spent >= left)])
            if spent < left:
                return spent
        return spent if self._leave_staging(p) else None

    def _stage_packed(self) -> None:
        """Admit into every free staging slot, send the next chunk of every staged prompt through ONE packed pass (at most
        ``prefill_budget`` rows together, ``prefill_step`` per prompt), then let the prompts that are complete leave staging in
        admission order: the first one that finished takes the first free slot."""
        pre, slots = self.pre, self.slots
        while self.free_staging and self.waiting() and pre.may_admit(slots):
            self._admit()
        budget = self.frontend.prefill_budget
        chunks = []
        promised = 0  # pages of the chunks already in this pass (only counted by an engine with swap space)
        for p in self.staged:
            rem = len(p["tokens"]) - p["offset"]
            if rem <= 0 or budget <= 0:
                continue
            n = min(self.prefill_step, rem, budget)
            if not pre.may_prefill(p["staging"], n, slots, promised):
                continue  # the pool cannot hold this chunk beside the pass's earlier ones yet
            promised += pre.chunk_pages(p["staging"], n)
            chunks.append((p, p["tokens"][p["offset"]:p["offset"] + n], n >= rem))
            budget -= n
        if chunks:
            self.frontend.before_prefill()
            self.engine.prefill_packed([(p["staging"], chunk, last) for p, chunk, last in chunks])
            for p, chunk, _ in chunks:
                p["offset"] += len(chunk)
            self.frontend.prefilled([(p, len(chunk), last) for p, chunk, last in chunks])
        for p in list(self.staged):
            if p["offset"] >= len(p["tokens"]):
                self._leave_staging(p)

    def _leave_staging(self, p: dict) -> bool:
        """The prompt of ``p`` is in the cache: retire it if it is finished, else move it into the lowest free decode slot.  False:
        prefilled and waiting for a slot."""
        staging = p["staging"]
        if self.frontend.finished_in_staging(staging, p):
            self._retire(staging, p)
        else:
            free = next((i for i, s in enumerate(self.slots) if s is None), None)
            if free is None:
                return False
            self.engine.move(staging, free)
            self.live.discard(staging)
            self.live.add(free)
            self.slots[free] = p
            self.pre.admitted(p)
        self.free_staging.append(staging)
        self.staged.remove(p)
        return True

    def _requeue(self, slot: int, state: dict) -> None:
        """Preemption.before_step's callback: the staged request gives way -- released, admitted again first."""
        self.engine.release(slot)
        self.live.discard(slot)
        self.free_staging.append(slot)
        self.staged.remove(state)
        self.frontend.requeued(state)
        self.front.insert(0, state["req"])

    def _retire(self, slot: int, state: dict) -> None:
        if self.cached:  # the answer's fed tokens are declared first (the last produced one was never fed)
            self.engine.prefix_extend(slot, state["out"][:-1])
        self.engine.release(slot)
        self.live.discard(slot)
        self.finished.append(state)

    # ---- the decode step --------------------------------------------------------------------------------------------------
    def _step(self) -> None:
        fe, slots = self.frontend, self.slots
        if fe.compact:
            close_holes(self.engine, slots, self.live)
        # (after Preemption.before_step a parked request always has a running one beside it, so "nothing runs" is "nothing is there")
        active = [i for i, s in enumerate(slots) if s is not None and not parked(s)]
        if not active:
            fe.idle()
            return
        # slots fill lowest-first, so rows above the highest occupied one are idle: decode only a bucket that covers the occupied
        # prefix; idle rows inside it carry context 0 and produce nothing
        top = max(i for i, s in enumerate(slots) if s is not None) if fe.rows_cover_parked else active[-1]
        rows = row_bucket(top + 1, self.batch_size)
        steps = fe.decode_block if fe.decode_block > 1 and not (self.waiting() or self.staged or self.pre.active) else 1
        fe.before_step(rows)
        self.engine.decode(steps, batch=rows)
        fe.stepped(rows, active, steps)
        for i in active:
            if fe.collect(i, slots[i]):
                self._retire(i, slots[i])
                slots[i] = None
