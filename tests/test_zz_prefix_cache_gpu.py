"""GPU tier: cross-request prefix caching in the decode engine (include/tinyllm_engine.h "Prefix cache"; csrc/prefix_cache.h,
csrc/kv_copy.h).

A hit reads the publisher's K/V bytes, so it must equal -- torch.equal on bf16 logits rows, == on ids -- a COLD control engine (cache
off, same slot, same batch) whose prefix went through the publisher's chunks.  Every case first holds the cold path to that standard
(`cold_is_reproducible`): if a cold control run twice does not give equal bits, the test says so and does not blame the cache.

TINY_CFG, 16-token pages, 64-row prefill chunks, 8 - 32 pages: the smallest shapes at which the page arithmetic can go wrong (a
prefix of whole pages, a tail inside a page, a prompt that ends on a page boundary, a rewind into an indexed page, a pool that must
evict)."""

import numpy as np
import pytest
import torch

from helpers import TINY_CFG, to_mlx_shaped
from oracle import tiny_oracle as O

pytestmark = pytest.mark.gpu
PAGE = 16
RNG = np.random.default_rng(2024)
S = [int(t) for t in RNG.integers(0, TINY_CFG["vocab_size"], 32)]     # two full pages
T1 = [int(t) for t in RNG.integers(0, TINY_CFG["vocab_size"], 7)]
T2 = [int(t) for t in RNG.integers(0, TINY_CFG["vocab_size"], 9)]
LONG = [int(t) for t in RNG.integers(0, TINY_CFG["vocab_size"], 51)]  # three full pages and three rows
OTHER = [int(t) for t in RNG.integers(0, TINY_CFG["vocab_size"], 112)]


@pytest.fixture(scope="module")
def model():
    return to_mlx_shaped(TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=11, sigma=0.05))


@pytest.fixture()
def make(model):
    from tiny_llm_hip.engine import DecodeEngine

    made = []

    def build(cache=False, num_pages=16, **kw):
        eng = DecodeEngine(model, page_size=PAGE, num_pages=num_pages, max_batch=3, max_prefill_rows=64, prefix_cache=cache, **kw)
        eng.num_pages = num_pages
        made.append(eng)
        return eng

    yield build
    for eng in made:
        eng.close()


def chunks(eng, slot, parts, logits_last=True):
    """Prefill the parts as one chunk each; only the last may produce logits."""
    for i, part in enumerate(parts):
        eng.prefill(slot, part, chunk=len(part), want_logits=logits_last and i == len(parts) - 1)


def rows_and_ids(eng, slot, steps=3, processed=False):
    """The logits row behind the prompt's last token, then `steps` decode steps' rows, and the ids produced."""
    rows = [eng.logits(1)[0].clone()]
    for _ in range(steps):
        eng.decode(1, batch=slot + 1)
        rows.append((eng.processed_logits(slot + 1) if processed else eng.logits(slot + 1))[slot].clone())
    return rows, eng.read_tokens(slot, steps + 1)


def assert_same(got, want, what):
    (g_rows, g_ids), (w_rows, w_ids) = got, want
    assert g_ids == w_ids, f"{what}: ids {g_ids} != {w_ids}"
    for i, (g, w) in enumerate(zip(g_rows, w_rows)):
        assert torch.equal(g, w), f"{what}: logits row {i} differs in {int((g != w).sum())} entries"


def cold(make, parts, rewind=0, tail=None, **kw):
    """A cold control: cache off, slot 0, batch 1.  The prefix in the given chunks, an optional rewind, then the request's remainder."""
    eng = make(False, **kw)
    eng.begin(0)
    chunks(eng, 0, parts, logits_last=tail is None)
    if rewind:
        eng.rewind(0, rewind)
    if tail is not None:
        eng.prefill(0, tail, chunk=len(tail))
    out = rows_and_ids(eng, 0)
    st = eng.stats()
    eng.release(0)
    return out, st


@pytest.fixture()
def cold_is_reproducible(make):
    a, _ = cold(make, [S], tail=T2)
    b, _ = cold(make, [S], tail=T2)
    if a[1] != b[1] or not all(torch.equal(x, y) for x, y in zip(a[0], b[0])):
        pytest.fail("the COLD path is not reproducible on this machine: two cache-off runs of the same chunks differ; the prefix cache is not at fault")
    return a


def totals(eng):
    """Both sets of counters, with the page-count identity checked."""
    st, ps = eng.stats(), eng.prefix_stats()
    assert st["pages_in_use"] + st["pages_free"] + ps["pages_retained"] == eng.num_pages
    return st, ps


def full_pages_case(make, want, **kw):
    eng = make(True, **kw)
    eng.begin(0)
    chunks(eng, 0, [S, T1])
    eng.release(0)
    st, ps = totals(eng)
    assert (ps["pages_retained"], st["pages_in_use"], st["pages_free"]) == (2, 0, 14)
    assert ps["pages_registered"] == 2 and ps["entries"] == 2
    eng.begin(0)
    assert eng.prefix_attach(0, S + T2) == 32
    assert eng.context_len(0) == 32
    st, ps = totals(eng)
    assert (ps["pages_retained"], st["pages_in_use"]) == (0, 2)
    eng.prefill(0, T2, chunk=len(T2))
    got = rows_and_ids(eng, 0)
    assert_same(got, want[0], "full pages")
    assert eng.stats()["prefill_tokens"] == 48 and want[1]["prefill_tokens"] == 41
    ps = eng.prefix_stats()
    assert (ps["lookups"], ps["hits"], ps["tokens_matched"], ps["tail_rows_copied"]) == (1, 1, 32, 0)
    eng.release(0)
    totals(eng)


def test_a_full_pages(make, cold_is_reproducible):
    want = cold(make, [S], tail=T2)
    assert_same(cold_is_reproducible, want[0], "cold against cold")
    full_pages_case(make, want)


def test_b_tail_rows(make, cold_is_reproducible):
    parts = [LONG[:32], LONG[32:48], LONG[48:51]]
    request = LONG[:41] + [(t + 1) % TINY_CFG["vocab_size"] for t in LONG[41:47]]
    eng = make(True)
    eng.begin(0)
    chunks(eng, 0, parts)
    eng.release(0)
    assert eng.prefix_stats()["pages_retained"] == 3
    eng.begin(0)
    assert eng.prefix_attach(0, request) == 41
    st, ps = totals(eng)
    assert ps["tail_rows_copied"] == 9 and st["pages_in_use"] == 3 and ps["pages_retained"] == 1  # 2 shared pages + 1 private copy
    eng.prefill(0, request[41:], chunk=len(request) - 41)
    got = rows_and_ids(eng, 0)
    eng.release(0)
    want, _ = cold(make, parts[:2], rewind=7, tail=request[41:])
    assert_same(got, want, "tail rows")
    # a prompt that ends exactly on a cached page boundary: all but its last token
    eng.begin(0)
    assert eng.prefix_attach(0, LONG[:48]) == 47
    assert eng.prefix_stats()["tail_rows_copied"] == 9 + 15
    eng.prefill(0, LONG[47:48], chunk=1)
    got = rows_and_ids(eng, 0)
    eng.release(0)
    totals(eng)
    want, _ = cold(make, parts[:2], rewind=1, tail=LONG[47:48])
    assert_same(got, want, "prompt ending on a page boundary")


def test_c_rewind_into_an_indexed_page(make, cold_is_reproducible):
    x = T1[:5]
    eng = make(True)
    eng.begin(0)
    chunks(eng, 0, [S], logits_last=False)
    assert eng.prefix_stats()["entries"] == 2
    eng.rewind(0, 8)  # lands inside the second, indexed page: the slot gets a private copy, the entry keeps its bytes
    st, ps = totals(eng)
    assert (st["pages_in_use"], ps["pages_retained"], st["page_allocations"]) == (2, 1, 3)
    eng.prefill(0, T2[:8], chunk=8, want_logits=False)  # 8 other tokens over rows 8 .. 15 of the copy
    assert eng.prefix_stats()["entries"] == 3  # the rewritten page is a sibling entry
    eng.release(0)
    eng.begin(0)
    assert eng.prefix_attach(0, S + x) == 32
    eng.prefill(0, x, chunk=len(x))
    got = rows_and_ids(eng, 0)
    eng.release(0)
    totals(eng)
    want, _ = cold(make, [S], tail=x)
    assert_same(got, want, "after a rewind into an indexed page")


def test_d_eviction_and_cap(make, cold_is_reproducible):
    pub = LONG[:48]
    eng = make(True, num_pages=8)
    eng.begin(0)
    chunks(eng, 0, [pub], logits_last=False)
    eng.release(0)
    st, ps = totals(eng)
    assert (ps["pages_retained"], st["pages_free"]) == (3, 5)
    eng.begin(0)
    assert eng.prefix_attach(0, OTHER) == 0
    chunks(eng, 0, [OTHER[:64], OTHER[64:]], logits_last=False)  # 7 pages: 5 free ones, then the two youngest leaves of the publisher
    st, ps = totals(eng)
    assert (st["pages_in_use"], st["pages_free"], ps["pages_retained"], ps["pages_evicted"]) == (7, 0, 1, 2)
    eng.begin(1)
    assert eng.prefix_attach(1, pub) == 16  # leaf first: the publisher's first page survived, and only it
    st, ps = totals(eng)
    assert (st["pages_in_use"], ps["pages_retained"]) == (8, 0)
    before = (eng.stats(), eng.prefix_stats(), eng.context_len(1))
    with pytest.raises(RuntimeError, match="KV page pool exhausted"):
        eng.prefill(1, pub[16:40], chunk=24)  # nothing evictable left
    assert (eng.stats(), eng.prefix_stats(), eng.context_len(1)) == before
    eng.release(0)
    eng.prefill(1, pub[16:40], chunk=24)  # the block-table row was left as it was: the slot goes on from its 16 cached tokens
    got = rows_and_ids(eng, 1)
    eng.release(1)
    totals(eng)
    ctl = make(False, num_pages=8)
    ctl.begin(1)
    chunks(ctl, 1, [pub], logits_last=False)
    ctl.rewind(1, 32)
    ctl.prefill(1, pub[16:40], chunk=24)
    assert_same(got, rows_and_ids(ctl, 1), "after a refused reservation")
    # the cap: at most 2 retained pages, so the publisher's leaf goes as soon as it is let go
    capped = make(2, num_pages=8)
    capped.begin(0)
    chunks(capped, 0, [pub], logits_last=False)
    capped.release(0)
    st, ps = totals(capped)
    assert (ps["pages_retained"], ps["pages_evicted"], ps["max_retained_pages"], st["pages_free"]) == (2, 1, 2, 6)
    capped.begin(0)
    assert capped.prefix_attach(0, pub) == 32
    capped.release(0)


def test_e_slot_settings(make, cold_is_reproducible):
    eng = make(True)
    eng.begin(0)
    chunks(eng, 0, [S, T1])
    eng.release(0)
    ctl = make(False)
    # penalties set before the attach: the matched tokens are prompt tokens of the history
    for e, hit in ((eng, True), (ctl, False)):
        e.begin(0)
        e.set_penalties(0, 1.3, 0.0, 0.0)
        if hit:
            assert e.prefix_attach(0, S + T2) == 32
        else:
            e.prefill(0, S, chunk=32, want_logits=False)
        e.prefill(0, T2, chunk=len(T2))
    got, want = rows_and_ids(eng, 0, processed=True), rows_and_ids(ctl, 0, processed=True)
    assert_same((got[0][1:], got[1]), (want[0][1:], want[1]), "penalised slot")
    eng.release(0), ctl.release(0)
    # a sampling slot: the Philox position is the context length
    for e, hit in ((eng, True), (ctl, False)):
        e.begin(0)
        e.set_sampling(0, 0.8, None, None, 5)
        if hit:
            assert e.prefix_attach(0, S + T2) == 32
        else:
            e.prefill(0, S, chunk=32, want_logits=False)
        e.prefill(0, T2, chunk=len(T2))
    assert_same(rows_and_ids(eng, 0), rows_and_ids(ctl, 0), "sampling slot")
    eng.release(0), ctl.release(0)
    # set_token + decode straight after an attach of whole pages, as after a fork
    for e, hit in ((eng, True), (ctl, False)):
        e.begin(0)
        if hit:
            assert e.prefix_attach(0, S + T2[:1]) == 32
        else:
            e.prefill(0, S, chunk=32, want_logits=False)
        e.set_token(0, T2[0])
        e.decode(1, batch=1)
    assert torch.equal(eng.logits(1), ctl.logits(1)) and eng.read_tokens(0, 1) == ctl.read_tokens(0, 1)
    eng.release(0), ctl.release(0)
    totals(eng)


def test_f_packed_admission(make, cold_is_reproducible):
    eng, ctl = make(True), make(False)
    eng.begin(2)
    eng.prefill(2, S, chunk=32, want_logits=False)  # a live publisher
    for slot, t in ((0, T1), (1, T2)):
        eng.begin(slot)
        assert eng.prefix_attach(slot, S + t) == 32
        ctl.begin(slot)
        ctl.prefill(slot, S, chunk=32, want_logits=False)
    for e in (eng, ctl):
        e.prefill_packed([(0, T1, True), (1, T2, True)])
    assert torch.equal(eng.logits(2), ctl.logits(2))
    assert eng.read_pending(2) == ctl.read_pending(2)
    st, _ = totals(eng)
    assert st["pages_in_use"] == 2 + 2 and ctl.stats()["pages_in_use"] == 4 + 2  # 2 shared pages where the control holds 4
    for e in (eng, ctl):
        e.decode(2, batch=2)
    assert torch.equal(eng.logits(2), ctl.logits(2))
    for slot in (0, 1, 2):
        eng.release(slot)
    totals(eng)


def test_g_fp8_pages(make, cold_is_reproducible):
    want = cold(make, [S], tail=T2, kv_format="fp8")
    again = cold(make, [S], tail=T2, kv_format="fp8")
    if want[0][1] != again[0][1] or not all(torch.equal(x, y) for x, y in zip(want[0][0], again[0][0])):
        pytest.fail("the COLD FP8 path is not reproducible: two cache-off runs differ; the prefix cache is not at fault")
    full_pages_case(make, want, kv_format="fp8")
    # ... and a tail over code and scale pools
    eng = make(True, kv_format="fp8")
    eng.begin(0)
    chunks(eng, 0, [S, T1 + T2], logits_last=False)  # 48 tokens: the third page is full
    eng.release(0)
    assert T2[0] != T1[4]
    request = S + T1[:4] + T2
    eng.begin(0)
    assert eng.prefix_attach(0, request) == 36
    assert totals(eng)[1]["tail_rows_copied"] == 4
    eng.prefill(0, T2, chunk=len(T2))
    got = rows_and_ids(eng, 0)
    ctl, _ = cold(make, [S, T1 + T2], rewind=12, tail=T2, kv_format="fp8")
    assert_same(got, ctl, "FP8 tail rows")


def test_h_cache_off(make):
    eng = make(False)
    assert eng.prefix_stats() == {"lookups": 0, "hits": 0, "tokens_matched": 0, "tail_rows_copied": 0, "pages_registered": 0,
                                  "pages_evicted": 0, "entries": 0, "pages_retained": 0, "max_retained_pages": 0, "enabled": 0}
    eng.begin(0)
    assert eng.prefix_attach(0, S + T2) == 0 and eng.context_len(0) == 0 and eng.stats()["pages_in_use"] == 0
    chunks(eng, 0, [S, T1])
    eng.prefix_extend(0, [1, 2, 3])  # does nothing
    eng.release(0)
    eng.begin(0)
    assert eng.prefix_attach(0, S + T2) == 0
    eng.release(0)
    st = eng.stats()
    assert (st["pages_free"], st["pages_in_use"]) == (16, 0) and eng.prefix_stats()["lookups"] == 0
    # bad input with the cache on: refused, nothing changed
    on = make(True)
    on.begin(0)
    on.prefill(0, S, chunk=32, want_logits=False)
    with pytest.raises(RuntimeError, match="already holds"):
        on.prefix_attach(0, S + T2)
    with pytest.raises(RuntimeError, match="more tokens than the slot holds"):
        on.prefix_extend(0, [1])
    with pytest.raises(RuntimeError):
        on.prefix_attach(1, S)  # not live
    assert on.prefix_stats()["lookups"] == 0
    on.release(0)
    on.prefix_clear()
    st = on.stats()
    assert (st["pages_free"], on.prefix_stats()["pages_retained"], on.prefix_stats()["entries"]) == (16, 0, 0)
