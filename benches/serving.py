"""Continuous-batching serving loop over the decode engine, with the reference harness's report
(reference: benches/bench.py:35-62 ServingMetrics, :351-572 run_batch_requests_serving, :787-830 report lines).

The loop itself is tiny_llm_hip/scheduler.py's (one scheduler, shared with tiny_llm_hip.engine.batch_generate_ids); ``serve_requests``
adds what is this front-end's own: a request is finished by its token count, and every engine call is timed and counted.

One loop turn = (a) prefill work for the request being admitted, (b) hand it to a free decode slot once its prompt is
in the cache, (c) ONE batched decode step over the occupied slots, (d) retire finished requests.  The reference does
exactly one prefill chunk per turn; on an MI355X that makes admission the bottleneck of a 64-slot batch (a decode
step takes ~4 ms, a 128-token chunk ~7 ms, and requests finish as fast as they are admitted: 21 of 64 slots busy).
``prefill_budget`` therefore lets a turn spend up to that many prompt tokens on admission (default = one chunk, the
reference's schedule), which is what lets config 4 ("64 concurrent requests") actually reach 64.

An engine whose ``prefix_cache_enabled`` is true (DecodeEngine(prefix_cache=...)) has every admitted request attach the cached
prefix of its prompt (``prefix_attach`` right after ``begin``: the prompt then starts at the matched offset) and declare the answer
tokens it fed at retirement (``prefix_extend(slot, out[:-1])`` before ``release``); the loop then also keeps the produced ids.  With
the cache off the call sequence is unchanged.

An engine whose ``swap_enabled`` is true (DecodeEngine(swap_pages=N), ScheduleOnlyEngine(num_pages=..., swap_pages=N)) is preempted
under page pressure instead of failing with "KV page pool exhausted": before a decode step the youngest staging request is released
and re-queued, or the running request admitted last is parked (its K/V swapped to host memory); parked requests resume oldest first
and nothing new is admitted while one is parked (tiny_llm_hip.preempt, shared with batch_generate_ids).  Without swap space the
call sequence is unchanged, error included.

The engine is duck-typed (begin / prefill / move / decode / release / synchronize / stats): ``ScheduleOnlyEngine``
runs the same schedule against a cost model instead of a GPU (capacity planning, and the CPU tests of the scheduler
and of the multi-replica dealer).
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field


def __getattr__(name):
    if name == "ROW_BUCKETS":  # the decode row counts the engine keeps captured graphs for: they live with the scheduler
        from tiny_llm_hip.scheduler import ROW_BUCKETS

        return ROW_BUCKETS
    raise AttributeError(name)


@dataclass
class ServingMetrics:
    """Field names are the reference's (benches/bench.py:35-62): drivers read them from the JSON payload.  Pages here are
    ENGINE pages (one id spans every layer's K and V: kv_bytes_per_page bytes); the growth / copy counters are zero by
    construction -- the pools are sized once, nothing is ever copied to grow (288 GB of HBM)."""
    generated_tokens: int = 0
    decode_tokens: int = 0
    prefill_time: float = 0.0
    decode_time: float = 0.0
    peak_active_requests: int = 0
    peak_live_pages: int = 0
    peak_capacity_pages: int = 0
    peak_tail_waste_slots: int = 0
    peak_tail_waste_live_slots: int = 0
    peak_tail_waste_bytes: int = 0
    peak_tail_waste_fraction: float = 0.0
    peak_kv_bytes: int = 0
    decode_step_count: int = 0
    decode_step_median_ms: float = 0.0
    decode_step_p95_ms: float = 0.0
    decode_step_max_ms: float = 0.0
    decode_gap_count: int = 0
    decode_gap_median_ms: float = 0.0
    decode_gap_p95_ms: float = 0.0
    decode_gap_max_ms: float = 0.0
    reused_page_allocations: int = 0
    storage_growths: int = 0
    copied_pages_on_growth: int = 0
    paged_growth_copy_bytes: int = 0
    dense_growth_copy_bytes: int = 0
    dense_staging_copy_bytes: int = 0
    # not in the reference: what the scheduler did
    prefill_chunks: int = 0
    turns: int = 0
    preemptions: int = 0    # requests that gave way under page pressure: parked, or released and re-queued (tiny_llm_hip.preempt)
    recomputed: int = 0     # ... of which released from the staging slot and prefilled again
    pages_swapped: int = 0  # KV pages moved to host memory and back (engine.swap_stats: pages_out + pages_in)
    decode_bytes: int = 0  # algorithmic HBM bytes of all decode steps: per step W + 147,456 B x sum of live contexts
    decode_step_ms: list = field(default_factory=list, repr=False)


def nearest_rank(values, q: float) -> float:
    """Nearest-rank percentile, the reference's definition (benches/bench.py:579-585)."""
    if not values:
        return 0.0
    ordered = sorted(values)
    rank = max(1, min(len(ordered), -int(-q * len(ordered) // 1)))
    return ordered[rank - 1]


def median(values) -> float:
    if not values:
        return 0.0
    ordered = sorted(values)
    mid = len(ordered) // 2
    return ordered[mid] if len(ordered) % 2 else 0.5 * (ordered[mid - 1] + ordered[mid])


def serve_requests(engine, requests, *, batch_size: int, prefill_step: int, prefill_budget: int | None = None,
                   page_size: int = 128, kv_bytes_per_page: int = 0, capacity_pages: int = 0,
                   clock=time.perf_counter, staging_slots: int = 1, compact: bool = True) -> ServingMetrics:
    """Serve ``requests`` (objects with prompt_token_ids, max_new_tokens) through ``engine`` with ``batch_size`` decode slots
    and ``staging_slots`` staging slots (indices batch_size ..).  Timers wrap a synchronised engine, like the reference's
    mx.eval inside them.  One staging slot = the reference's policy (one request prefilled at a time, batch.py:48-76);
    several = the admitted prompts' chunks go through ONE packed multi-token pass per turn (engine.prefill_packed), at most
    ``prefill_budget`` rows together.  ``compact``: close the holes in the decode slots before a step whenever that lowers its row
    bucket (tiny_llm_hip.scheduler.close_holes).  The turn is tiny_llm_hip.scheduler.Scheduler's, shared with batch_generate_ids
    (pure host logic: no GPU needed to import it); what is this front-end's own -- a request is finished by its token count, and the
    whole measurement -- is the class below."""
    from tiny_llm_hip.scheduler import Frontend, RequestSettings, Scheduler

    m = ServingMetrics()
    cached = bool(getattr(engine, "prefix_cache_enabled", False))
    has_step_bytes = hasattr(engine, "step_bytes")
    gaps_ms: list[float] = []

    class Serving(Frontend):
        t0 = 0.0
        last_completion: float | None = None

        def admit(self, slot, state):
            request = state["req"]
            state["tokens"], state["count"] = request.prompt_token_ids, 0
            lora = getattr(request, "lora", None)  # the id of a resident LoRA adapter (DecodeEngine.load_lora); such a request bypasses the prefix cache
            if lora is not None and lora >= 0:
                RequestSettings(lora=lora).apply(engine, slot)
            dry = getattr(request, "dry", None)  # DRY / the n-gram ban: a dict with the keys of DecodeEngine.set_dry
            if dry:
                from tiny_llm_hip.engine import dry_args

                RequestSettings(dry=dry_args(dry.get("multiplier", 0.0), dry.get("base", 1.75), dry.get("allowed_length", 2), dry.get("range", 0),
                                             dry.get("no_repeat_ngram", 0), dry.get("breakers") or ())).apply(engine, slot)

        def before_prefill(self):
            self.t0 = clock()

        def prefilled(self, chunks):
            engine.synchronize()
            m.prefill_time += clock() - self.t0
            m.prefill_chunks += len(chunks)
            for state, _, last in chunks:
                if last:
                    state["count"] = 1
                    m.generated_tokens += 1
                    if cached:  # the produced ids are only kept for prefix_extend
                        state["out"].append(engine.read_tokens(state["staging"], 1)[0])
            self.snapshot()

        def finished_in_staging(self, slot, state):  # a one-token request never enters the batch
            return state["count"] >= state["req"].max_new_tokens

        def before_step(self, rows):
            m.decode_bytes += int(engine.step_bytes(rows)) if has_step_bytes else 0
            self.t0 = clock()

        def stepped(self, rows, active, steps):
            engine.synchronize()
            now = clock()
            m.decode_time += now - self.t0
            m.decode_step_ms.append((now - self.t0) * 1e3)
            if self.last_completion is not None:
                gaps_ms.append((now - self.last_completion) * 1e3)
            self.last_completion = now
            produced = engine.read_pending(rows) if cached else None
            slots = sched.slots
            for i in active:
                slots[i]["count"] += 1
                if produced is not None:
                    slots[i]["out"].append(produced[i])
            m.generated_tokens += len(active)
            m.decode_tokens += len(active)
            self.snapshot()

        def collect(self, slot, state):
            return state["count"] >= state["req"].max_new_tokens

        def requeued(self, state):
            m.generated_tokens -= state["count"]

        def idle(self):
            self.last_completion = None  # idle time without an active decode request is not a fairness gap

        def snapshot(self):
            # context lengths: a running request holds its prompt and every produced token but the last, a staged one what was prefilled
            ctx = [s["offset"] + s["count"] - 1 for s in sched.slots if s is not None] + [s["offset"] for s in sched.staged]
            m.peak_active_requests = max(m.peak_active_requests, len(ctx))
            pages = sum((c + page_size - 1) // page_size for c in ctx)
            waste = sum((-c) % page_size for c in ctx if c > 0)
            m.peak_live_pages = max(m.peak_live_pages, pages)
            m.peak_capacity_pages = max(m.peak_capacity_pages, capacity_pages)
            m.peak_kv_bytes = max(m.peak_kv_bytes, capacity_pages * kv_bytes_per_page)
            if waste > m.peak_tail_waste_slots:
                m.peak_tail_waste_slots = waste
                m.peak_tail_waste_live_slots = pages * page_size
                m.peak_tail_waste_bytes = waste * (kv_bytes_per_page // page_size if page_size else 0)
                m.peak_tail_waste_fraction = waste / (pages * page_size) if pages else 0.0

    fe = Serving()
    fe.prefill_budget, fe.compact = prefill_step if prefill_budget is None else prefill_budget, compact
    sched = Scheduler(engine, fe, requests, batch_size=batch_size, prefill_step=prefill_step, staging_slots=staging_slots)
    sched.run()
    m.turns = sched.turns
    sched.pre.report(m)
    stats = engine.stats() if hasattr(engine, "stats") else {}
    m.reused_page_allocations = int(stats.get("reused_page_allocations", 0))
    m.decode_step_count = len(m.decode_step_ms)
    m.decode_step_median_ms = median(m.decode_step_ms)
    m.decode_step_p95_ms = nearest_rank(m.decode_step_ms, 0.95)
    m.decode_step_max_ms = max(m.decode_step_ms, default=0.0)
    m.decode_gap_count = len(gaps_ms)
    m.decode_gap_median_ms = median(gaps_ms)
    m.decode_gap_p95_ms = nearest_rank(gaps_ms, 0.95)
    m.decode_gap_max_ms = max(gaps_ms, default=0.0)
    return m


def report_lines(num_seqs: int, prompt_tokens: int, total_time: float, m: ServingMetrics) -> list[str]:
    """The report exactly as the reference prints it (benches/bench.py:765-830; drivers regex these lines,
    benches/bench_course_progression.py:103-105)."""
    def div(a, b):
        return a / b if b else 0.0

    gen = m.generated_tokens
    return [
        f"Requests: {num_seqs}, Prompt tokens: {prompt_tokens}, Generated tokens: {gen}",
        f"Time: {total_time:.2f}s, Output throughput: {div(gen, total_time):.2f} tok/s",
        f"Total throughput (prompt+output): {div(prompt_tokens + gen, total_time):.2f} tok/s",
        f"Prefill throughput: {div(prompt_tokens, m.prefill_time):.2f} tok/s",
        f"Decode throughput: {div(m.decode_tokens, m.decode_time):.2f} tok/s",
        f"Request throughput: {div(num_seqs, total_time):.2f} req/s",
        f"Peak active requests: {m.peak_active_requests}",
        f"Peak KV bytes: {m.peak_kv_bytes}",
        f"Peak live KV pages: {m.peak_live_pages}",
        f"Peak KV capacity pages: {m.peak_capacity_pages}",
        f"Peak tail waste slots: {m.peak_tail_waste_slots}",
        f"Tail-waste snapshot live slots: {m.peak_tail_waste_live_slots}",
        f"Tail-waste snapshot bytes: {m.peak_tail_waste_bytes}",
        f"Tail-waste snapshot fraction: {m.peak_tail_waste_fraction:.6f}",
        f"Decode step latency ms (median/p95/max): {m.decode_step_median_ms:.3f}/{m.decode_step_p95_ms:.3f}/{m.decode_step_max_ms:.3f}",
        f"Decode completion gap ms (median/p95/max): {m.decode_gap_median_ms:.3f}/{m.decode_gap_p95_ms:.3f}/{m.decode_gap_max_ms:.3f}",
        f"Reused page allocations: {m.reused_page_allocations}",
        f"Page-pool growths: {m.storage_growths}",
        f"Pages copied during pool growth: {m.copied_pages_on_growth}",
        f"Dense KV bytes copied during growth: {m.dense_growth_copy_bytes}",
        f"Dense KV bytes copied into batch tensors: {m.dense_staging_copy_bytes}",
        f"Paged KV bytes copied during pool growth: {m.paged_growth_copy_bytes}",
    ]


class ScheduleOnlyEngine:
    """The engine's slot interface against a COST MODEL instead of a GPU: a virtual clock advances by
    ``prefill_ms_per_token`` per prompt token and ``decode_ms(rows)`` per batched step.  Enforces the slot protocol (a slot
    is begun once, moved into a free slot, released once) so that scheduler bugs surface without hardware."""

    def __init__(self, slots: int, prefill_ms_per_token: float = 0.055, decode_ms=lambda rows: 1.1 + 0.07 * rows,
                 prefix_cache: bool = False, page_size: int = 128, num_pages: int | None = None, swap_pages: int = 0,
                 swap_ms_per_page: float = 0.05):
        """``num_pages``: a page POOL of that many pages (None, the default: no pool, nothing ever runs short): every unparked slot holds
        ceil(context / page_size) private pages, and a prefill or decode step that needs more than the pool has left raises the
        engine's "KV page pool exhausted" with nothing changed.  ``swap_pages``: swap space of that many host records (include/
        tinyllm_engine.h "KV swap"): park / unpark / is_parked / step_pages / swap_stats as the engine has them, each moved page
        costing ``swap_ms_per_page`` on the virtual clock.
        ``prefix_cache``: a page-granular model of the engine's prefix cache (include/tinyllm_engine.h "Prefix cache"): the full
        pages of every token sequence a slot is known to hold are remembered (no eviction: the model has no pool), prefix_attach
        matches whole pages plus the longest partial page, never more than len(tokens) - 1, and the virtual clock charges only the
        tokens that are actually prefilled.  Produced ids are 0 (read_tokens / read_pending), so answers cache like prompts."""
        self.slots = [None] * slots  # context length per live slot
        self.now = 0.0
        self.prefill_ms_per_token = prefill_ms_per_token
        self.decode_ms = decode_ms
        self.page_allocations = 0
        self.prefix_cache_enabled = bool(prefix_cache)
        self.page_size = page_size
        self.known = [None] * slots            # token ids the engine knows per live slot (prompt chunks, declared answers)
        self.cached_pages: set[tuple] = set()  # every cached chain of full pages, as the tuple of its tokens
        self.prefilled_tokens = 0
        self.counters = {"lookups": 0, "hits": 0, "tokens_matched": 0, "tail_rows_copied": 0, "pages_registered": 0}
        self.num_pages = num_pages
        self.swap_pages = int(swap_pages)
        self.swap_enabled = self.swap_pages > 0
        self.swap_ms_per_page = swap_ms_per_page
        self.parked_slots: set[int] = set()
        self.swap_counters = {"parks": 0, "unparks": 0, "pages_out": 0, "pages_in": 0}

    # ---- the page pool and the swap space (only with num_pages / swap_pages) ---------------------------------------------
    def _pages(self, tokens: int) -> int:
        return (tokens + self.page_size - 1) // self.page_size

    def _free_pages(self) -> int:
        held = sum(self._pages(c) for i, c in enumerate(self.slots) if c is not None and i not in self.parked_slots)
        return (self.num_pages if self.num_pages is not None else 1 << 30) - held

    def _take(self, pages: int) -> None:
        if pages > self._free_pages():
            raise RuntimeError("engine: KV page pool exhausted")

    def _unparked(self, slot, what):
        if self.slots[slot] is None:
            raise RuntimeError("slot holds no sequence")
        if slot in self.parked_slots:
            raise RuntimeError(f"{what}: the slot is parked")

    def context_len(self, slot) -> int:
        return -1 if self.slots[slot] is None else self.slots[slot]

    def is_parked(self, slot) -> bool:
        return slot in self.parked_slots

    def step_pages(self, batch=None):
        rows = range(batch or len(self.slots))
        need = sum(self._pages(self.slots[i] + 1) - self._pages(self.slots[i]) for i in rows if self.slots[i] is not None and i not in self.parked_slots)
        return need, self._free_pages()

    def park(self, slot):
        self._unparked(slot, "park")
        pages = self._pages(self.slots[slot])
        in_use = sum(self._pages(self.slots[i]) for i in self.parked_slots)
        if self.slots[slot] < 1 or pages > self.swap_pages - in_use:
            raise RuntimeError("engine_park: not enough free host records")
        self.parked_slots.add(slot)
        self.swap_counters["parks"] += 1
        self.swap_counters["pages_out"] += pages
        self.now += pages * self.swap_ms_per_page * 1e-3

    def unpark(self, slot):
        if slot not in self.parked_slots:
            raise RuntimeError("engine_unpark: the slot is not parked")
        pages = self._pages(self.slots[slot])
        if pages > self._free_pages():
            raise RuntimeError("engine_unpark: KV page pool exhausted")
        self.parked_slots.discard(slot)
        self.swap_counters["unparks"] += 1
        self.swap_counters["pages_in"] += pages
        self.now += pages * self.swap_ms_per_page * 1e-3

    def swap_stats(self):
        return {"host_pages": self.swap_pages, "host_pages_in_use": sum(self._pages(self.slots[i]) for i in self.parked_slots), **self.swap_counters}

    def clock(self) -> float:
        return self.now

    def begin(self, slot):
        if self.slots[slot] is not None:
            raise RuntimeError("slot already holds a sequence")
        self.slots[slot] = 0
        self.known[slot] = []

    def _append(self, slot, tokens):
        self._unparked(slot, "prefill")
        self._take(self._pages(self.slots[slot] + len(tokens)) - self._pages(self.slots[slot]))
        if self.prefix_cache_enabled and len(self.known[slot]) == self.slots[slot]:
            self.known[slot].extend(int(t) for t in tokens)
            self._publish(slot)
        self.slots[slot] += len(tokens)
        self.prefilled_tokens += len(tokens)

    def _publish(self, slot):
        known, P = self.known[slot], self.page_size
        for end in range(P, len(known) + 1, P):
            chain = tuple(known[:end])
            if chain not in self.cached_pages:
                self.cached_pages.add(chain)
                self.counters["pages_registered"] += 1

    def prefix_attach(self, slot, tokens) -> int:
        if self.slots[slot] != 0:
            raise RuntimeError("prefix_attach needs a freshly begun slot")
        if not self.prefix_cache_enabled:
            return 0
        tokens, P = [int(t) for t in tokens], self.page_size
        limit = len(tokens) - 1
        self.counters["lookups"] += 1
        full = 0
        while (full + 1) * P <= limit and tuple(tokens[:(full + 1) * P]) in self.cached_pages:
            full += 1
        head, tail = tuple(tokens[:full * P]), 0
        for chain in self.cached_pages:  # the longest partial page among the children of the last matched page
            if len(chain) == (full + 1) * P and chain[:full * P] == head:
                rows = 0
                while rows < min(P, limit - full * P) and chain[full * P + rows] == tokens[full * P + rows]:
                    rows += 1
                tail = max(tail, rows)
        matched = full * P + tail
        self.counters["hits"] += matched > 0
        self.counters["tokens_matched"] += matched
        self.counters["tail_rows_copied"] += tail
        self.slots[slot] = matched
        self.known[slot] = tokens[:matched]
        return matched

    def prefix_extend(self, slot, tokens):
        if self.slots[slot] is None:
            raise RuntimeError("slot holds no sequence")
        if not self.prefix_cache_enabled or not tokens:
            return
        if len(self.known[slot]) + len(tokens) > self.slots[slot]:
            raise RuntimeError("prefix_extend declares more tokens than the slot holds")
        self.known[slot].extend(int(t) for t in tokens)
        self._publish(slot)

    def prefix_stats(self):
        return {**self.counters, "entries": len(self.cached_pages), "enabled": int(self.prefix_cache_enabled)}

    def read_tokens(self, slot, count):
        return [0] * count

    def read_pending(self, count=None):
        return [0] * (count or len(self.slots))

    def prefill(self, slot, tokens, chunk=None, want_logits=True):
        self._append(slot, tokens)
        self.now += len(tokens) * self.prefill_ms_per_token * 1e-3

    def prefill_packed(self, chunks):
        """One pass over several slots' chunks: rows cost the same, the fixed per-pass overhead is paid once."""
        if len({c[0] for c in chunks}) != len(chunks):
            raise RuntimeError("a slot appears twice in a packed prefill")
        self._take(sum(self._pages(self.slots[s] + len(t)) - self._pages(self.slots[s]) for s, t, _ in chunks if self.slots[s] is not None))
        for slot, tokens, _last in chunks:
            self._append(slot, tokens)
        self.now += sum(len(c[1]) for c in chunks) * self.prefill_ms_per_token * 1e-3

    def move(self, src, dst):
        if self.slots[src] is None or self.slots[dst] is not None:
            raise RuntimeError("bad move")
        self.slots[dst], self.slots[src] = self.slots[src], None
        self.known[dst], self.known[src] = self.known[src], None
        if src in self.parked_slots:  # the parked records move with the slot
            self.parked_slots.discard(src)
            self.parked_slots.add(dst)

    def decode(self, steps, batch=None):
        rows = [i for i in range(batch) if self.slots[i] is not None and i not in self.parked_slots]
        self._take(sum(self._pages(self.slots[i] + steps) - self._pages(self.slots[i]) for i in rows))
        for i in rows:
            self.slots[i] += steps
        self.now += steps * self.decode_ms(batch) * 1e-3

    def release(self, slot):
        if self.slots[slot] is None:
            raise RuntimeError("slot holds no sequence")
        self.slots[slot] = None
        self.known[slot] = None
        self.parked_slots.discard(slot)

    def synchronize(self):
        pass

    def step_bytes(self, batch=None):
        """W + 147,456 B x the live contexts of the step (Qwen3-4B W4: W = 2,136,832,000 B)."""
        return 2_136_832_000 + 147_456 * sum(c for i, c in enumerate(self.slots[:batch]) if c is not None and i not in self.parked_slots)

    def stats(self):
        return {"reused_page_allocations": 0, "pages_in_use": 0}
