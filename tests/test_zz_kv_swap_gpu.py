"""GPU tier: KV swap in the decode engine (include/tinyllm_engine.h "KV swap"; csrc/kv_swap.h, csrc/slot_table.h,
tiny_llm_hip/preempt.py).

A parked and resumed sequence reads back the bytes it wrote, so it must equal -- torch.equal on bf16 logits rows, == on ids -- an
UNINTERRUPTED control: a fresh engine, same slot, same batch, same chunks.  The round trip first holds the control to that standard
against itself (`control_is_reproducible`): if two uninterrupted runs do not give equal bits, the test says so and does not blame the swap.

TINY_CFG, 16-token pages, 64-row prefill chunks, 8 - 16 pages, three slots: contexts of 1 token, 32 (ending on a page boundary) and 51
(three pages and three rows), each on both replay routes and once with FP8 pages; the kernels alone against numpy on pools whose rows
are 256, 256, 4 and 6 bytes (the 16-byte, the 4-byte and the byte path)."""

import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import TINY_CFG, to_mlx_shaped
from oracle import tiny_oracle as O

pytestmark = pytest.mark.gpu
PAGE = 16
V = TINY_CFG["vocab_size"]
RNG = np.random.default_rng(4242)
LONG = [int(t) for t in RNG.integers(0, V, 51)]    # three full pages and three rows
OTHER = [int(t) for t in RNG.integers(0, V, 128)]  # eight full pages: takes a whole 8-page pool
SECOND = [int(t) for t in RNG.integers(0, V, 23)]
T2 = [int(t) for t in RNG.integers(0, V, 9)]
TL_ERR_INVALID = -1


@pytest.fixture(scope="module")
def ext():
    import tiny_llm_ext_hip

    tiny_llm_ext_hip.load_library(".")
    return tiny_llm_ext_hip


@pytest.fixture(scope="module")
def model():
    return to_mlx_shaped(TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=11, sigma=0.05))


@pytest.fixture()
def make(model):
    from tiny_llm_hip.engine import DecodeEngine

    made = []

    def build(swap=0, num_pages=8, route="aql", **kw):
        old = os.environ.pop("TL_AQL", None)
        if route == "hipgraph":
            os.environ["TL_AQL"] = "0"
        try:
            eng = DecodeEngine(model, page_size=PAGE, num_pages=num_pages, max_batch=3, max_prefill_rows=64, swap_pages=swap, **kw)
        finally:
            os.environ.pop("TL_AQL", None)
            if old is not None:
                os.environ["TL_AQL"] = old
        assert eng.replay_route().startswith(route), eng.replay_route()
        eng.num_pages = num_pages
        made.append(eng)
        return eng

    yield build
    for eng in made:
        eng.close()


def prefill(eng, slot, tokens, want_logits=True):
    eng.prefill(slot, tokens, chunk=64, want_logits=want_logits)


def rows_and_ids(eng, slot, steps=3, batch=None, processed=False, first_row=True):
    """The logits row behind the prompt's last token (first_row), then `steps` decode steps' rows, and the ids the steps produced."""
    batch = batch or slot + 1
    rows = [eng.logits(1)[0].clone()] if first_row else []
    for _ in range(steps):
        eng.decode(1, batch=batch)
        rows.append((eng.processed_logits(batch) if processed else eng.logits(batch))[slot].clone())
    return rows, eng.read_tokens(slot, steps)


def assert_same(got, want, what):
    (g_rows, g_ids), (w_rows, w_ids) = got, want
    assert g_ids == w_ids, f"{what}: ids {g_ids} != {w_ids}"
    assert len(g_rows) == len(w_rows)
    for i, (g, w) in enumerate(zip(g_rows, w_rows)):
        assert torch.equal(g, w), f"{what}: logits row {i} differs in {int((g != w).sum())} entries"


def snapshot(eng, slot):
    return eng.stats(), eng.swap_stats(), eng.context_len(slot)


def identity(eng):
    st = eng.stats()
    retained = eng.prefix_stats()["pages_retained"]
    assert st["pages_in_use"] + st["pages_free"] + retained == eng.num_pages, (st, retained)
    return st


# ---- the two launches against numpy ------------------------------------------------------------------------------------------------
ROW_BYTES = (256, 256, 4, 6)
POOL_PAGES, HEADS = 6, 2
SENTINEL = 0xA5


@pytest.mark.parametrize("tail_rows", [1, 7, 16])
def test_gather_and_scatter_move_the_named_rows_and_nothing_else(ext, tail_rows):
    gen = torch.Generator().manual_seed(tail_rows)
    src = [torch.randint(0, 256, (POOL_PAGES, HEADS, PAGE, rb), dtype=torch.uint8, generator=gen).cuda() for rb in ROW_BYTES]
    dst = [torch.full((POOL_PAGES, HEADS, PAGE, rb), SENTINEL, dtype=torch.uint8).cuda() for rb in ROW_BYTES]
    src_before = [p.clone() for p in src]

    def table(pools):
        t = (ext.TlKvPoolDesc * len(pools))(*[ext.TlKvPoolDesc(p.data_ptr(), rb) for p, rb in zip(pools, ROW_BYTES)])
        return t, torch.frombuffer(bytearray(bytes(t)), dtype=torch.uint8).cuda()

    host_table, src_table = table(src)
    _, dst_table = table(dst)
    record = ext.lib().tl_kv_page_record_bytes(host_table, len(ROW_BYTES), HEADS, PAGE)
    assert record == HEADS * PAGE * sum(ROW_BYTES)
    offsets = np.cumsum([0] + [HEADS * PAGE * rb for rb in ROW_BYTES[:-1]]).astype(np.uint64)
    offsets_dev = torch.from_numpy(offsets.view(np.int64)).cuda()
    out_ids, in_ids = [3, 0, 4], [1, 5, 2]
    out_dev, in_dev = torch.tensor(out_ids, dtype=torch.int32).cuda(), torch.tensor(in_ids, dtype=torch.int32).cuda()
    staging = torch.full((4 * record,), SENTINEL, dtype=torch.uint8).cuda()  # one record more than the launch writes
    torch.cuda.synchronize()
    args = (len(ROW_BYTES), HEADS, PAGE)
    ext.check(ext.lib().tl_kv_gather_pages(src_table.data_ptr(), offsets_dev.data_ptr(), *args, out_dev.data_ptr(), 3, tail_rows, staging.data_ptr(), record, None))
    torch.cuda.synchronize()
    want = np.full(4 * record, SENTINEL, dtype=np.uint8)
    for j, page in enumerate(out_ids):
        rows = tail_rows if j == 2 else PAGE
        for i, rb in enumerate(ROW_BYTES):
            for h in range(HEADS):
                at = j * record + int(offsets[i]) + h * PAGE * rb
                want[at:at + rows * rb] = src_before[i][page, h, :rows].cpu().numpy().reshape(-1)
    assert torch.equal(staging.cpu(), torch.from_numpy(want)), "the staging records differ from the named rows, or a byte outside them changed"
    for got, was in zip(src, src_before):
        assert torch.equal(got, was), "gather wrote into a pool"
    ext.check(ext.lib().tl_kv_scatter_pages(dst_table.data_ptr(), offsets_dev.data_ptr(), *args, in_dev.data_ptr(), 3, tail_rows, staging.data_ptr(), record, None))
    torch.cuda.synchronize()
    for i, got in enumerate(dst):
        expect = torch.full_like(got, SENTINEL)
        for j, (page_out, page_in) in enumerate(zip(out_ids, in_ids)):
            rows = tail_rows if j == 2 else PAGE
            expect[page_in, :, :rows] = src_before[i][page_out, :, :rows]
        assert torch.equal(got, expect), f"pool {i}: the named rows did not arrive, or a byte outside them changed"
    assert torch.equal(staging.cpu(), torch.from_numpy(want)), "scatter wrote into the staging buffer"


# ---- round trip -----------------------------------------------------------------------------------------------------------------
def control(make, prompt, **kw):
    eng = make(0, **kw)
    eng.begin(0)
    prefill(eng, 0, prompt)
    out = rows_and_ids(eng, 0)
    eng.release(0)
    return out


def parked_round_trip(make, prompt, **kw):
    """prefill; park; another slot takes and overwrites every freed page; release it; unpark."""
    eng = make(8, **kw)
    eng.begin(0)
    prefill(eng, 0, prompt)
    held = eng.stats()["pages_in_use"]
    assert held == (len(prompt) + PAGE - 1) // PAGE
    eng.park(0)
    assert eng.is_parked(0) and eng.context_len(0) == len(prompt)
    st, sw = eng.stats(), eng.swap_stats()
    assert (st["pages_in_use"], st["pages_free"]) == (0, 8) and sw["host_pages_in_use"] == held and sw["pages_out"] == held
    eng.begin(1)
    prefill(eng, 1, OTHER, want_logits=False)  # (no logits: the row behind slot 0's prompt stays where it is)
    after = eng.stats()
    assert after["pages_in_use"] == 8 and after["pages_free"] == 0  # every page of the pool, the freed ones among them ...
    assert after["reused_page_allocations"] - st["reused_page_allocations"] >= held  # ... taken again and written
    eng.release(1)
    eng.unpark(0)
    assert not eng.is_parked(0)
    st, sw = eng.stats(), eng.swap_stats()
    assert st["pages_in_use"] == held and st["pages_in_use"] + st["pages_free"] == 8
    assert (sw["host_pages_in_use"], sw["parks"], sw["unparks"], sw["pages_in"]) == (0, 1, 1, held)
    out = rows_and_ids(eng, 0)
    eng.release(0)
    return out


@pytest.fixture()
def control_is_reproducible(make):
    a, b = control(make, LONG), control(make, LONG)
    if a[1] != b[1] or not all(torch.equal(x, y) for x, y in zip(a[0], b[0])):
        pytest.fail("the UNINTERRUPTED path is not reproducible on this machine: two runs of the same chunks differ; the swap is not at fault")
    return a


@pytest.mark.parametrize("route", ["aql", "hipgraph"])
@pytest.mark.parametrize("context", [1, 32, 51])
def test_a_parked_sequence_resumes_bit_for_bit(make, control_is_reproducible, context, route):
    want = control(make, LONG[:context], route=route)
    if context == 51 and route == "aql":
        assert_same(control_is_reproducible, want, "control against control")
    assert_same(parked_round_trip(make, LONG[:context], route=route), want, f"context {context}, {route}")


def test_a_parked_sequence_resumes_bit_for_bit_with_fp8_pages(make):
    want = control(make, LONG, kv_format="fp8")
    assert_same(control(make, LONG, kv_format="fp8"), want, "control against control")
    assert_same(parked_round_trip(make, LONG, kv_format="fp8"), want, "fp8 pages")


# ---- state stays with the slot -----------------------------------------------------------------------------------------------------
def tiny_vocabulary():
    """ids 0-255 the single bytes, then two-letter lower-case words; the last id is EOS (empty)."""
    letters = b"abcdefghijklmnopqrstuvwxyz"
    words = [bytes([a, b]) for a in letters for b in letters + b" "] + [bytes([a, b, 101]) for a in letters for b in letters]
    return [bytes([b]) for b in range(256)] + words[:V - 257] + [b""]


def settings(eng, slot, grammar):
    eng.set_sampling(slot, temperature=0.8, seed=1234)
    eng.set_penalties(slot, repetition=1.3, presence=0.4, frequency=0.2)
    eng.set_grammar(slot, grammar)
    eng.set_logprobs(slot, 3)


def test_every_setting_stays_with_a_parked_slot(make):
    from tiny_llm_hip import grammar as G

    dfa = G.compile_regex(rb"[a-z]+( [a-z]+)*")

    def run(swap):
        eng = make(8 if swap else 0)
        eng.make_vocab(tiny_vocabulary())
        grammar = eng.make_grammar(dfa, [V - 1])
        eng.begin(0)
        settings(eng, 0, grammar)
        prefill(eng, 0, LONG)
        if swap:
            eng.park(0)
            eng.begin(1)
            prefill(eng, 1, OTHER, want_logits=False)
            eng.release(1)
            eng.unpark(0)
        rows, _ = rows_and_ids(eng, 0, processed=True, first_row=False)
        out = rows, eng.read_tokens(0, 4), eng.grammar_state(0), eng.read_logprobs(0, 4)
        eng.release(0)
        return out

    want, got = run(False), run(True)
    assert got[1] == want[1], f"ids {got[1]} != {want[1]}"
    for i, (g, w) in enumerate(zip(got[0], want[0])):
        assert torch.equal(g, w), f"processed row {i} differs"
    assert got[2] == want[2], "grammar state"
    assert got[3] == want[3], "log-probability records"


# ---- a parked slot inside the decoded range ------------------------------------------------------------------------------------------
def test_a_parked_slot_inside_the_range_is_left_alone(make):
    def slot0(eng):
        eng.begin(0)
        eng.set_sampling(0, temperature=0.8, seed=99)
        eng.set_penalties(0, repetition=1.2, presence=0.3, frequency=0.1)  # the step's processing launch must not count for a parked row
        eng.set_logprobs(0, 2)
        prefill(eng, 0, LONG)

    def slot1(eng):  # it processes too, so the step's processing launch runs over both rows
        eng.begin(1)
        eng.set_penalties(1, repetition=1.1)
        prefill(eng, 1, SECOND)

    kv_bytes_per_token = 2 * TINY_CFG["num_hidden_layers"] * TINY_CFG["num_key_value_heads"] * TINY_CFG["head_dim"] * 2
    eng = make(8, num_pages=12)
    slot0(eng)
    slot1(eng)
    bytes_both = eng.step_bytes(2)
    eng.park(0)
    before = snapshot(eng, 0)
    assert bytes_both - eng.step_bytes(2) == kv_bytes_per_token * len(LONG)  # a parked slot's context is not read by a step
    assert eng.step_pages(2) == (0, 12 - 2)                                  # ... and takes no page
    got1 = rows_and_ids(eng, 1, batch=2, first_row=False)
    assert eng.context_len(0) == len(LONG) and eng.swap_stats() == before[1]
    eng.release(1)
    eng.unpark(0)
    rows, ids = rows_and_ids(eng, 0, processed=True, first_row=False)
    got0 = rows, eng.read_tokens(0, 4), eng.read_logprobs(0, 4)
    eng.release(0)

    ctl = make(0, num_pages=12)  # the controls, in the order the engine above decoded: slot 1 beside an EMPTY slot 0, then slot 0 alone
    slot1(ctl)
    assert_same(got1, rows_and_ids(ctl, 1, batch=2, first_row=False), "slot 1 beside a parked slot 0")
    ctl.release(1)
    slot0(ctl)
    rows, ids = rows_and_ids(ctl, 0, processed=True, first_row=False)
    want0 = rows, ctl.read_tokens(0, 4), ctl.read_logprobs(0, 4)
    ctl.release(0)
    assert got0[1] == want0[1] and got0[2] == want0[2]
    for i, (g, w) in enumerate(zip(got0[0], want0[0])):
        assert torch.equal(g, w), f"slot 0, processed row {i} differs"


# ---- move, fork, cache -------------------------------------------------------------------------------------------------------------
def test_a_parked_slot_moves_with_its_records(make):
    def run(swap):
        eng = make(8 if swap else 0)
        eng.begin(0)
        prefill(eng, 0, LONG)
        if swap:
            eng.park(0)
        eng.move(0, 2)
        if swap:
            assert eng.is_parked(2) and eng.context_len(2) == len(LONG) and eng.context_len(0) == -1
            assert eng.swap_stats()["host_pages_in_use"] == 4
            eng.unpark(2)
        out = rows_and_ids(eng, 2, batch=3, first_row=False)
        eng.release(2)
        assert eng.stats()["pages_in_use"] == 0 and eng.swap_stats()["host_pages_in_use"] == 0
        return out

    assert_same(run(True), run(False), "moved while parked")


def test_a_forked_child_parks_while_the_parent_decodes(make):
    def run(swap):
        eng = make(8 if swap else 0, num_pages=12)
        eng.begin(0)
        prefill(eng, 0, LONG)
        eng.fork(0, 1)
        assert eng.stats()["pages_in_use"] == 5  # three shared pages and two tails
        if swap:
            eng.park(1)
            st = eng.stats()
            assert (st["pages_in_use"], st["pages_free"]) == (4, 8)  # only the child's own tail was freed: the shared pages stay
        parent = rows_and_ids(eng, 0, batch=1, first_row=False)
        if swap:
            eng.unpark(1)
            assert eng.stats()["pages_in_use"] == 4 + 4 + 0  # the parent's four (one more token each step stays inside its tail) + four private
        child = rows_and_ids(eng, 1, batch=2, first_row=False)
        eng.release(0)
        eng.release(1)
        assert eng.stats()["pages_in_use"] == 0
        return parent, child

    got, want = run(True), run(False)
    assert_same(got[0], want[0], "parent beside a parked child")
    assert_same(got[1], want[1], "child after unpark")


def test_with_the_prefix_cache_the_identity_holds_and_a_follow_up_hits(make):
    eng = make(8, num_pages=16, prefix_cache=True)
    eng.begin(0)
    identity(eng)
    prefill(eng, 0, LONG)
    identity(eng)
    eng.park(0)
    st = identity(eng)
    assert st["pages_in_use"] == 0 and eng.prefix_stats()["pages_retained"] == 3  # the indexed pages are retained, the tail is free
    eng.unpark(0)
    st = identity(eng)
    assert st["pages_in_use"] == 4
    eng.decode(3, batch=1)
    identity(eng)
    ids = eng.read_tokens(0, 4)
    eng.prefix_extend(0, ids[:-1])
    identity(eng)
    eng.release(0)
    identity(eng)
    request = LONG[:48] + T2
    eng.begin(0)
    assert eng.prefix_attach(0, request) == 48
    identity(eng)
    prefill(eng, 0, request[48:])
    got = rows_and_ids(eng, 0)
    eng.release(0)
    identity(eng)

    def cold():
        c = make(0, num_pages=16)
        c.begin(0)
        prefill(c, 0, LONG)  # the publisher's chunk and its three decode steps, then back to the 48 tokens the follow-up shares
        c.decode(3, batch=1)
        c.rewind(0, 6)
        prefill(c, 0, T2)
        out = rows_and_ids(c, 0)
        c.release(0)
        return out

    want = cold()
    assert_same(cold(), want, "cold against cold")
    assert_same(got, want, "follow-up hit after park and unpark")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(make, ext):
    lib = ext.lib()
    eng = make(3)  # 51 tokens want four records: one too few
    eng.begin(0)
    prefill(eng, 0, LONG)
    before = snapshot(eng, 0)
    assert lib.tl_engine_park(eng._h, 0) == TL_ERR_INVALID
    assert snapshot(eng, 0) == before and not eng.is_parked(0)
    assert lib.tl_engine_unpark(eng._h, 0) == TL_ERR_INVALID  # not parked
    assert lib.tl_engine_park(eng._h, 1) == TL_ERR_INVALID    # no sequence
    assert snapshot(eng, 0) == before
    eng.release(0)

    eng = make(8)
    assert lib.tl_engine_swap_stats  # (bound)
    eng.begin(0)
    prefill(eng, 0, LONG)
    eng.park(0)
    assert lib.tl_engine_swap_space(eng._h, 0) == TL_ERR_INVALID  # while a slot is parked
    eng.begin(1)
    prefill(eng, 1, OTHER[:80], want_logits=False)  # five of eight pages: three are left, the parked slot wants four
    before = snapshot(eng, 0)
    assert lib.tl_engine_unpark(eng._h, 0) == TL_ERR_INVALID
    assert snapshot(eng, 0) == before and eng.is_parked(0)
    # every call that would read or write the parked slot's K/V
    tokens = (ctypes.c_int32 * 4)(1, 2, 3, 4)
    out_ids, out_lp, matched = (ctypes.c_int32 * 4)(), (ctypes.c_float * 4)(), ctypes.c_int(0)
    one, four = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(4)
    refused = {
        "park": lambda: lib.tl_engine_park(eng._h, 0),
        "prefill": lambda: lib.tl_engine_prefill(eng._h, 0, tokens, 4, 1),
        "prefill_packed": lambda: lib.tl_engine_prefill_packed(eng._h, 1, one, tokens, four, (ctypes.c_int * 1)(1)),
        "score": lambda: lib.tl_engine_score(eng._h, 0, tokens, 4, -1, out_lp, None),
        "verify": lambda: lib.tl_engine_verify(eng._h, 0, tokens, 4, out_ids),
        "fork": lambda: lib.tl_engine_fork(eng._h, 0, 2),
        "rewind": lambda: lib.tl_engine_rewind(eng._h, 0, 1),
        "reserve": lambda: lib.tl_engine_reserve(eng._h, 0, 64),
        "prefix_attach": lambda: lib.tl_engine_prefix_attach(eng._h, 0, tokens, 4, ctypes.byref(matched)),
        "prefix_extend": lambda: lib.tl_engine_prefix_extend(eng._h, 0, tokens, 4),
        "begin": lambda: lib.tl_engine_begin(eng._h, 0),
    }
    for name, call in refused.items():
        assert call() == TL_ERR_INVALID, name
        assert snapshot(eng, 0) == before and eng.is_parked(0), name
    assert eng.context_len(2) == -1
    # ... while the per-slot settings and the read calls still work
    eng.set_sampling(0, temperature=0.5, seed=3)
    eng.set_logprobs(0, 1)
    assert eng.read_tokens(0, 1) == [eng.read_pending(1)[0]]
    eng.release(1)
    eng.unpark(0)
    eng.release(0)
    st, sw = eng.stats(), eng.swap_stats()
    assert (st["pages_in_use"], st["pages_free"], sw["host_pages_in_use"]) == (0, 8, 0)
    eng.set_swap_space(0)
    assert eng.swap_stats()["host_pages"] == 0


def test_releasing_a_parked_slot_returns_its_records(make):
    eng = make(4)
    eng.begin(0)
    prefill(eng, 0, LONG)
    eng.park(0)
    assert eng.swap_stats()["host_pages_in_use"] == 4
    eng.release(0)
    assert eng.swap_stats()["host_pages_in_use"] == 0 and eng.context_len(0) == -1 and not eng.is_parked(0)
    eng.begin(0)  # the slot and the arena serve the next request
    prefill(eng, 0, LONG)
    eng.park(0)
    eng.unpark(0)
    eng.release(0)
    assert eng.stats()["pages_in_use"] == 0


# ---- the scheduler -----------------------------------------------------------------------------------------------------------------
def test_batch_generate_ids_preempts_instead_of_failing():
    """Six prompts through two decode slots on 8 pages: without swap space the pool runs out; with it every prompt gets the ids of a run
    on a pool that never runs short.  The peaked checkpoint of tests/test_zz_prefix_generator_gpu.py: row-count buckets change when a
    request leaves the batch, so only a checkpoint whose top-2 margin dwarfs rounding allows id equality."""
    from tiny_llm_hip.engine import DecodeEngine, batch_generate_ids
    from tiny_llm_hip.synthetic import synthetic_qwen3

    peaked = synthetic_qwen3(TINY_CFG, seed=21, sigma=0.05, device="cuda", embed_sigma=0.5, residual_gain=0.5, head_permutation=(5, 11))
    rng = np.random.default_rng(77)
    prompts = [[int(t) for t in rng.integers(0, V, n)] for n in (20, 9, 33, 17, 26, 12)]

    def run(num_pages, swap):
        eng = DecodeEngine(peaked, page_size=PAGE, num_pages=num_pages, max_batch=3, max_prefill_rows=64, swap_pages=swap)
        try:
            done = sorted(batch_generate_ids(eng, prompts, 40, batch_size=2, prefill_step=16))
            st = eng.stats()
            assert st["pages_in_use"] == 0 and st["pages_free"] == num_pages
            return done, eng.swap_stats()
        finally:
            eng.close()

    want, _ = run(16, 0)
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        run(8, 0)
    got, sw = run(8, 12)
    assert sw["parks"] >= 1 and sw["parks"] == sw["unparks"] and sw["host_pages_in_use"] == 0
    assert [i for i, _ in got] == list(range(6))
    for (i, g), (_, w) in zip(got, want):
        assert g == w, f"prompt {i}: {g} != {w}"
