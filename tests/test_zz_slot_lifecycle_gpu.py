"""GPU tier: one sequence through the whole slot lifecycle (csrc/slot_table.h as the engine applies its edits: block-table writes,
tail-page copies, park and unpark transfers) with the prefix cache off and on.

16-token pages, 12 pages, 3 slots, 8 host records.  A 21-token prompt (one full page and a partial tail) is prefilled into slot 0, then:
fork 0 -> 1, two decode steps, slot 1 rewound by 3, moved to slot 2 and parked, slot 0 decoded alone for 12 steps across a page
boundary, slot 2 unparked, both decoded, everything released.  Every id of each sequence must equal an undisturbed single-slot control on
a fresh engine -- for the rewound one the control is fed the 20 kept tokens and the 21st as its pending token -- and after every call
pages_in_use + pages_free + retained pages == num_pages; at the end no page and no host record is held.  The peaked checkpoint of
tests/test_zz_kv_swap_gpu.py's scheduler test: the sequences are decoded beside each other here and alone in the controls, and only a
checkpoint whose top-2 margin dwarfs rounding allows id equality across row counts."""

import numpy as np
import pytest

from helpers import TINY_CFG
from test_zz_kv_swap_gpu import PAGE, V

pytestmark = pytest.mark.gpu
NUM_PAGES, RECORDS = 12, 8
PROMPT = [int(t) for t in np.random.default_rng(2121).integers(0, V, 21)]
ALONE, TOGETHER = 12, 4  # decode steps of slot 0 alone (context 23 -> 35: past the boundary at 32), then of both


@pytest.fixture(scope="module")
def peaked():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=21, sigma=0.05, device="cuda", embed_sigma=0.5, residual_gain=0.5, head_permutation=(5, 11))


def engine(model, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    return DecodeEngine(model, page_size=PAGE, num_pages=NUM_PAGES, max_batch=3, max_prefill_rows=64, **kw)


@pytest.fixture(scope="module")
def controls(peaked):
    """(ids of the prompt's sequence, ids of the sequence that keeps 20 tokens and is fed the 21st), each alone in slot 0."""
    eng = engine(peaked)
    try:
        eng.begin(0)
        eng.prefill(0, PROMPT, chunk=64)
        eng.decode(2 + ALONE + TOGETHER, batch=1)
        whole = eng.read_tokens(0, 1 + 2 + ALONE + TOGETHER)
        eng.release(0)
        eng.begin(0)
        eng.prefill(0, PROMPT[:20], chunk=64, want_logits=False)
        eng.set_token(0, PROMPT[20])
        eng.decode(TOGETHER, batch=1)
        kept = eng.read_tokens(0, TOGETHER)
        eng.release(0)
        return whole, kept
    finally:
        eng.close()


@pytest.mark.parametrize("prefix_cache", [False, True])
def test_fork_rewind_move_park_unpark_keep_every_sequence(peaked, controls, prefix_cache):
    whole, kept = controls
    eng = engine(peaked, swap_pages=RECORDS, prefix_cache=prefix_cache)

    def call(fn, *args, **kw):
        out = fn(*args, **kw)
        st, retained = eng.stats(), eng.prefix_stats()["pages_retained"]
        assert st["pages_in_use"] + st["pages_free"] + retained == NUM_PAGES, (fn.__name__, st, retained)
        return out

    try:
        call(eng.begin, 0)
        call(eng.prefill, 0, PROMPT, chunk=64)
        call(eng.fork, 0, 1)
        assert eng.stats()["pages_in_use"] == 3  # the full page shared, two tails
        call(eng.decode, 2, batch=2)
        first = eng.read_tokens(0, 3)
        assert eng.read_tokens(1, 2) == whole[1:3]  # the child draws what the parent draws
        call(eng.rewind, 1, 3)
        assert eng.context_len(1) == 20
        eng.set_token(1, PROMPT[20])
        call(eng.move, 1, 2)
        call(eng.park, 2)
        assert eng.is_parked(2) and eng.context_len(1) == -1 and eng.swap_stats()["host_pages_in_use"] == 2
        call(eng.decode, ALONE, batch=1)
        assert eng.context_len(0) == 21 + 2 + ALONE and eng.context_len(2) == 20
        alone = eng.read_tokens(0, ALONE)
        call(eng.unpark, 2)
        call(eng.decode, TOGETHER, batch=3)
        assert first + alone + eng.read_tokens(0, TOGETHER) == whole
        assert eng.read_tokens(2, TOGETHER) == kept
        call(eng.release, 0)
        call(eng.release, 2)
        assert eng.stats()["pages_in_use"] == 0 and eng.swap_stats()["host_pages_in_use"] == 0
    finally:
        eng.close()
