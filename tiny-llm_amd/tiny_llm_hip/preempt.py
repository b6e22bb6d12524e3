"""Preemption under KV page pressure: the policy of the one scheduler (tiny_llm_hip/scheduler.py) behind ``batch_generate_ids`` and
``serve_requests``.

Pure host logic over the engine's duck-typed slot interface (``step_pages`` / ``park`` / ``unpark`` / ``context_len`` / ``swap_stats``;
DecodeEngine(swap_pages=N), or benches/serving.py's ScheduleOnlyEngine): no torch, no extension.  The policy is vLLM's: when the next
decode step needs more pages than the pool can give, the youngest sequence gives way.

  victim   before a decode step, while ``need > obtainable`` (engine.step_pages):
           1. the staging request, if it holds pages (the youngest staged one first): it is RELEASED and put back at the front of the
              queue -- recomputation is cheapest for the youngest, and the prefix cache helps it;
           2. else the running request admitted last: it is PARKED in place (its K/V goes to host memory, every per-slot setting stays);
              holes are closed as before with ``move`` (scheduler.close_holes), which carries a parked slot's records.
           With one running request left that still does not fit, nothing is done: the step raises the engine's own
           "KV page pool exhausted".
  resume   the oldest parked request first, when ``obtainable >= its pages + one per running request``.
  admission  nothing new is admitted while anything is parked (``may_admit``), and a staged prompt's next chunk waits a turn when the
           pool cannot hold it while other requests are alive to free pages (``may_prefill``) -- a lone request goes ahead and gets the
           engine's error.

Running requests are the scheduler's state dicts: the helper stamps ``state["admitted"]`` (admission order) and ``state["parked"]``.
An engine without swap space makes every method a no-op that answers "go ahead": the scheduler is then the program it was.
"""

from __future__ import annotations


class Preemption:
    def __init__(self, engine):
        self.engine = engine
        self.active = bool(getattr(engine, "swap_enabled", False))
        self.page_size = int(getattr(engine, "page_size", 0) or 0)
        self.preemptions = 0   # parks + recomputations
        self.recomputed = 0    # staging requests released and re-queued
        self._admissions = 0
        self._pages_before = self._pages_swapped() if self.active else 0

    def _pages_swapped(self) -> int:
        s = self.engine.swap_stats()
        return int(s["pages_out"]) + int(s["pages_in"])

    @staticmethod
    def parked(state) -> bool:
        return state is not None and bool(state.get("parked"))

    def _pages(self, tokens: int) -> int:
        return (tokens + self.page_size - 1) // self.page_size

    def admitted(self, state) -> None:
        """The request enters a decode slot: later ones are preempted first."""
        state["admitted"] = self._admissions
        self._admissions += 1

    def may_admit(self, slots) -> bool:
        return not (self.active and any(self.parked(s) for s in slots))

    def chunk_pages(self, slot: int, tokens: int) -> int:
        """Pages ``slot`` takes for ``tokens`` more tokens."""
        if not self.active:
            return 0
        ctx = max(self.engine.context_len(slot), 0)
        return self._pages(ctx + tokens) - self._pages(ctx)

    def may_prefill(self, slot: int, tokens: int, slots, promised: int = 0) -> bool:
        """Can ``slot`` take ``tokens`` more tokens now, with ``promised`` pages already given to other chunks of the same pass?  False:
        wait a turn (somebody else is alive and will free or be made to free pages)."""
        if not self.active:
            return True
        _, obtainable = self.engine.step_pages(1)
        return self.chunk_pages(slot, tokens) + promised <= obtainable or not any(s is not None for s in slots)

    def before_step(self, slots, rows_of, staged, requeue) -> None:
        """Resume what fits, then make room for the step over ``rows_of()`` rows.  ``slots``: the running requests' states by decode
        slot (None: free).  ``staged``: [(slot, state)] of the staging requests, oldest first.  ``requeue(slot, state)``: the loop
        releases that staging request and puts it back at the front of its queue."""
        if not self.active:
            return
        eng = self.engine
        staged = list(staged)

        def give_way(slot, state):
            staged.remove((slot, state))
            requeue(slot, state)
            self.recomputed += 1
            self.preemptions += 1

        while True:  # resume, oldest parked first
            waiting = sorted((s["admitted"], i) for i, s in enumerate(slots) if self.parked(s))
            if not waiting:
                break
            slot = waiting[0][1]
            running = sum(1 for s in slots if s is not None and not self.parked(s))
            _, obtainable = eng.step_pages(rows_of())
            if obtainable >= self._pages(eng.context_len(slot)) + running:
                eng.unpark(slot)
                slots[slot]["parked"] = False
                continue
            if running > 0:
                break  # pages come back as the running requests finish
            holding = [(st, state) for st, state in staged if eng.context_len(st) > 0]
            if not holding:
                raise RuntimeError("engine: KV page pool exhausted (a parked request cannot resume into an idle pool)")
            give_way(*holding[-1])  # nobody runs: only a staged request can still hold the pages
        while True:
            need, obtainable = eng.step_pages(rows_of())
            if need <= obtainable:
                return
            holding = [(slot, state) for slot, state in staged if eng.context_len(slot) > 0]
            if holding:
                give_way(*holding[-1])
                continue
            running = sorted((s["admitted"], i) for i, s in enumerate(slots) if s is not None and not self.parked(s))
            if len(running) <= 1:
                return  # the step raises the engine's own error
            slot = running[-1][1]
            eng.park(slot)
            slots[slot]["parked"] = True
            self.preemptions += 1

    def report(self, metrics) -> None:
        """The counts into a ServingMetrics (benches/serving.py)."""
        metrics.preemptions = self.preemptions
        metrics.recomputed = self.recomputed
        metrics.pages_swapped = self._pages_swapped() - self._pages_before if self.active else 0
