"""GPU tier: beam search (include/tinyllm_engine.h "Beam search").

* tl_beam_rows (csrc/beam.h) against the float64 restatement of its definition (tests/beam_oracle.py): which (parent, token) pairs, in
  which order, with which scores.  The seeds are chosen (on the CPU) so that no two adjacent candidates the device must tell apart lie
  within 2 TOL of each other, and every case asserts that about the oracle's scores before it looks at the device's.
* tl_engine_beam_reorder against a second engine that reaches the same genealogy in the same slots with fork / move / release /
  set_token over spare slots: the group's logits rows must agree bit for bit after every step, for bf16 and FP8 pages, with a partial
  and with a full tail page.
* beam_search_ids end to end on the peaked checkpoint against the same policy over host-side float64 selection."""

import math

import numpy as np
import pytest
import torch

import beam_oracle as BO
from helpers import TINY_CFG

pytestmark = pytest.mark.gpu

TOL = 2e-4  # the project's log-probability tolerance (tests/test_zz_logprobs_gpu.py)
PAGE = 16
V = TINY_CFG["vocab_size"]

# (vocab, rows) -> the seed of the case's logits and scores: the first for which the oracle's adjacent candidates among the first 33 are
# more than 2 TOL apart (equal logits of one row aside: those tie exactly and the lower id goes first)
SEEDS = {(vocab, rows): 1 for vocab in (8, 1000, 8197, 151936) for rows in (1, 3, 8)}
SEEDS.update(tie=1, edges=1)


def case_rows(vocab, rows, seed):
    """Logits 4 N(0, 1) in bf16 (equal logits inside a row are common) and cumulative scores in [-3, 0] (so that every row competes)."""
    rng = np.random.default_rng(seed)
    logits = torch.from_numpy((rng.standard_normal((rows, vocab)) * 4.0).astype(np.float32)).bfloat16()
    scores = (-3.0 * rng.random(rows)).astype(np.float32)
    return logits, scores


def assert_apart(ranked):
    """On the oracle's float64 scores: adjacent distinct candidates are more than 2 TOL apart.  Two candidates are not distinct when
    they are equal logits of one row, or (the tie case below) equal logits of rows that are bit-identical with equal scores: those
    have exactly equal scores on the device too, and the order is the definition's (parent, then token)."""
    real = [c for c in ranked if c[0] >= 0 and c[2] > -math.inf]
    for a, b in zip(real, real[1:]):
        assert a[2] - b[2] > 2 * TOL or (a[2] == b[2] and a[4] == b[4]), (a, b)


def check_against_oracle(got, logits, scores, n_cand):
    rows64 = logits.float().numpy().astype(np.float64)
    want = BO.beam_select(rows64, scores, n_cand + 1, with_logits=True)
    assert_apart(want)
    want = want[:n_cand]
    assert [c[:2] for c in got] == [c[:2] for c in want]  # across rows: the oracle's list exactly
    for p in range(len(rows64)):  # within a parent: exactly the row's first tokens in (logit descending, lower id first) order
        mine = [c[1] for c in got if c[0] == p]
        assert mine == BO.row_order(rows64[p])[:len(mine)].tolist()
    for g, w in zip(got, want):
        if w[0] < 0:
            assert g == BO.EMPTY
            continue
        for mine, theirs in ((g[2], w[2]), (g[3], w[3])):
            assert mine == theirs == -math.inf or abs(mine - theirs) <= TOL + abs(theirs) * 2.0 ** -23, (g, w)
        assert g[2] == float(np.float32(np.float32(scores[g[0]]) + np.float32(g[3])))  # the score is ONE fp32 addition


_cases = {}


def shared_case(vocab, rows):
    if (vocab, rows) not in _cases:
        logits, scores = case_rows(vocab, rows, SEEDS[(vocab, rows)])
        _cases[(vocab, rows)] = (logits, scores, logits.cuda())
    return _cases[(vocab, rows)]


@pytest.mark.parametrize("n_cand", [1, 2, 16, 32])
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("vocab", [8, 1000, 8197, 151936])  # 8: fewer pairs than candidates; 8,197: one past a pass of 8,192
def test_beam_rows_match_the_oracle(vocab, rows, n_cand):
    import tiny_llm_ext_hip as ext

    logits, scores, dev = shared_case(vocab, rows)
    got = ext.beam_rows(dev, scores, n_cand)
    check_against_oracle(got, logits, scores, n_cand)
    if vocab * rows < n_cand:
        assert got[vocab * rows:] == [BO.EMPTY] * (n_cand - vocab * rows)
    assert ext.beam_rows(dev, scores, n_cand) == got  # two calls agree bit for bit


def test_bit_identical_rows_tie_exactly_and_the_lower_parent_goes_first():
    import tiny_llm_ext_hip as ext

    logits, _ = case_rows(1000, 3, SEEDS["tie"])
    logits[2] = logits[0]
    scores = np.array([-1.5, -0.25, -1.5], dtype=np.float32)
    got = ext.beam_rows(logits.cuda(), scores, 32)
    check_against_oracle(got, logits, scores, 32)
    from_0, from_2 = [c for c in got if c[0] == 0], [c for c in got if c[0] == 2]
    assert len(from_0) >= 4 and len(from_0) - len(from_2) in (0, 1)
    for a, b in zip(from_0, from_2):
        assert a[1:] == b[1:] and got.index(b) == got.index(a) + 1  # the same token with the same score bits, right behind


def test_dead_nan_and_infinite_rows_contribute_nothing():
    import tiny_llm_ext_hip as ext

    logits, scores = case_rows(1000, 5, SEEDS["edges"])
    scores[1] = -np.inf                # a dead beam
    logits[2] = float("nan")           # a row of NaN
    logits[3, 77] = float("inf")       # a row holding +inf
    logits[4, ::3] = float("nan")      # NaN logits inside a live row: never ranked
    logits[4, 5] = float("-inf")
    dev = logits.cuda()
    got = ext.beam_rows(dev, scores, 32)
    check_against_oracle(got, logits, scores, 32)
    assert {c[0] for c in got} == {0, 4} and all(c[1] % 3 != 0 for c in got if c[0] == 4)
    assert ext.beam_rows(dev, scores, 32) == got
    assert ext.beam_rows(dev[1:4].contiguous(), scores[1:4], 4) == [BO.EMPTY] * 4
    lonely = torch.full((1, 40), float("-inf")).bfloat16()
    lonely[0, 9] = 2.0
    lonely[0, 30] = float("nan")
    got = ext.beam_rows(lonely.cuda(), [-2.0], 3)  # one finite logit: log-probability 0; then the -inf logits by id
    assert got == [(0, 9, -2.0, 0.0), (0, 0, -math.inf, -math.inf), (0, 1, -math.inf, -math.inf)]


# ---- the reorder ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def peaked():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=21, sigma=0.05, device="cuda", embed_sigma=0.5, residual_gain=0.5, head_permutation=(5, 11))


def make_engine(model, num_pages=24, max_batch=6, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    return DecodeEngine(model, page_size=PAGE, num_pages=num_pages, max_batch=max_batch, max_prefill_rows=64, **kw)


def pages(eng, num_pages):
    st = eng.stats()
    assert st["pages_in_use"] + st["pages_free"] == num_pages, st  # (the prefix cache is off: nothing is retained)
    return st["pages_in_use"]


def same_rows(a, b, rows, what):
    assert torch.equal(a.logits(rows), b.logits(rows)), what


@pytest.mark.parametrize("kv_format", ["bf16", "fp8"])
@pytest.mark.parametrize("n_prompt", [PAGE + 3, 2 * PAGE])  # a partial tail page; a full one
def test_reorder_equals_fork_move_release_over_spare_slots(peaked, kv_format, n_prompt):
    prompt = [int(t) for t in np.random.default_rng(n_prompt).integers(0, V, n_prompt)]
    partial = n_prompt % PAGE != 0
    eng, ctl = make_engine(peaked, kv_format=kv_format), make_engine(peaked, kv_format=kv_format)

    def tokens(ids):
        for slot, t in enumerate(ids):
            ctl.set_token(slot, t)

    try:
        for e in (eng, ctl):
            e.begin(0)
            e.prefill(0, prompt)
        assert pages(eng, 24) == 2
        # one source to three slots
        eng.beam_reorder(0, 1, [0, 0, 0], [11, 500, 1023])
        ctl.fork(0, 1), ctl.fork(0, 2), tokens([11, 500, 1023])
        assert pages(eng, 24) == pages(ctl, 24) == (4 if partial else 2)  # the full pages shared; a partial tail copied twice
        assert [eng.context_len(s) for s in range(4)] == [n_prompt] * 3 + [-1]
        assert eng.read_pending(3) == [11, 500, 1023]
        for e in (eng, ctl):
            e.decode(1, batch=3)
        same_rows(eng, ctl, 3, "after [0, 0, 0]")
        # [2, 2, 0]: slot 2's sequence twice, slot 0's once, slot 1's let go
        eng.beam_reorder(0, 3, [2, 2, 0], [7, 8, 9])
        ctl.move(0, 3), ctl.move(2, 0), ctl.release(1), ctl.fork(0, 1), ctl.move(3, 2), tokens([7, 8, 9])
        assert pages(eng, 24) == pages(ctl, 24)
        for e in (eng, ctl):
            e.decode(1, batch=3)
        same_rows(eng, ctl, 3, "after [2, 2, 0]")
        # the permutation [1, 0] of the first two slots: no page changes hands with the pool
        before = pages(eng, 24)
        eng.beam_reorder(0, 2, [1, 0], [300, 301])
        ctl.move(0, 3), ctl.move(1, 0), ctl.move(3, 1), tokens([300, 301])
        assert pages(eng, 24) == before
        for e in (eng, ctl):
            e.decode(1, batch=3)
        same_rows(eng, ctl, 3, "after the permutation [1, 0]")
        # a shrink from 3 to 2
        eng.beam_reorder(0, 3, [2, 0], [40, 41])
        ctl.release(1), ctl.move(0, 1), ctl.move(2, 0), tokens([40, 41])
        assert pages(eng, 24) == pages(ctl, 24) and eng.context_len(2) == -1
        for e in (eng, ctl):
            e.decode(2, batch=2)
        same_rows(eng, ctl, 2, "after the shrink [2, 0]")
        assert eng.read_tokens(0, 2) == ctl.read_tokens(0, 2) and eng.read_tokens(1, 2) == ctl.read_tokens(1, 2)
        for slot in (0, 1):
            eng.release(slot)
        assert pages(eng, 24) == 0  # releasing the group returns every page
    finally:
        eng.close()
        ctl.close()


def test_a_reorder_the_pool_cannot_serve_changes_nothing(peaked):
    prompt = [int(t) for t in np.random.default_rng(5).integers(0, V, PAGE + 3)]
    filler = [int(t) for t in np.random.default_rng(6).integers(0, V, 2 * PAGE)]
    eng, ctl = make_engine(peaked, num_pages=4), make_engine(peaked, num_pages=4)
    try:
        for e in (eng, ctl):
            e.begin(0)
            e.prefill(0, prompt)
            e.begin(5)
            e.prefill(5, filler)  # the other two pages: no page is obtainable
        before = eng.stats()
        assert before["pages_free"] == 0
        with pytest.raises(RuntimeError, match="KV page pool exhausted"):
            eng.beam_reorder(0, 1, [0, 0], [3, 4])  # the second child needs a copy of the tail
        after = eng.stats()
        assert (after["pages_in_use"], after["pages_free"], after["page_allocations"]) == (4, 0, before["page_allocations"])
        assert [eng.context_len(s) for s in (0, 1, 5)] == [PAGE + 3, -1, 2 * PAGE]
        assert eng.read_pending(1) == ctl.read_pending(1)
        eng.beam_reorder(0, 1, [0], [3])  # one child inherits: no page needed
        ctl.set_token(0, 3)
        for e in (eng, ctl):
            e.decode(1, batch=1)
        same_rows(eng, ctl, 1, "the step after a refused reorder")
    finally:
        eng.close()
        ctl.close()


def test_the_lora_adapter_travels_with_the_parent(peaked):
    import lora_oracle as L

    adapter = L.to_lora_adapter(L.make_adapter(TINY_CFG, 16, seed=0, sigma=0.05, scale=1.0))
    prompt = [int(t) for t in np.random.default_rng(9).integers(0, V, PAGE + 5)]
    eng, ctl = make_engine(peaked), make_engine(peaked)
    try:
        for e in (eng, ctl):
            x = e.load_lora(adapter)
            for slot, lora in ((0, x), (1, None)):
                e.begin(slot)
                e.set_lora(slot, lora)
                e.prefill(slot, prompt)
        # slot 0 <- the base sequence; slots 1 and 2 <- the adapter's, with its adapter
        eng.beam_reorder(0, 2, [1, 0, 0], [21, 22, 23])
        ctl.move(0, 3), ctl.move(1, 0), ctl.move(3, 1), ctl.fork(1, 2)
        for slot, t in enumerate([21, 22, 23]):
            ctl.set_token(slot, t)
        assert [eng.slot_lora(s) for s in range(4)] == [ctl.slot_lora(s) for s in range(4)] == [-1, x, x, -1]
        for e in (eng, ctl):
            e.decode(2, batch=3)
        same_rows(eng, ctl, 3, "adapter and base beams after a reorder")
        rows = eng.logits(3)
        assert not torch.equal(rows[0], rows[1])  # (the adapter moves the logits: the two sequences hold the same tokens)
        eng.beam_reorder(0, 3, [0], [5])  # a shrink to the base beam: the slots that are released lose the adapter
        assert [eng.slot_lora(s) for s in range(3)] == [-1, -1, -1] and pages(eng, 24) == 2
    finally:
        eng.close()
        ctl.close()


def test_select_and_reorder_refuse_slots_that_are_not_plain(peaked):
    eng = make_engine(peaked)
    try:
        eng.begin(0)
        eng.prefill(0, [1, 2, 3])
        assert len(eng.beam_select(0, 1, [0.0], 4)) == 4
        with pytest.raises(RuntimeError, match="most recent logits"):
            eng.beam_select(0, 2, [0.0, 0.0], 4)  # a prefill leaves one row
        with pytest.raises(RuntimeError, match="most recent logits"):
            eng.beam_select(1, 1, [0.0], 4)
        eng.set_sampling(0, temperature=0.7, seed=1)
        with pytest.raises(RuntimeError, match="samples"):
            eng.beam_select(0, 1, [0.0], 4)
        with pytest.raises(RuntimeError, match="samples"):
            eng.beam_reorder(0, 1, [0, 0], [1, 2])
        eng.set_sampling(0)
        eng.set_logprobs(0, 2)
        with pytest.raises(RuntimeError, match="log-probabilities"):
            eng.beam_select(0, 1, [0.0], 4)
        eng.set_logprobs(0, None)
        eng.begin(2)
        with pytest.raises(RuntimeError, match="already holds"):
            eng.beam_reorder(0, 1, [0, 0, 0], [1, 2, 3])  # slot 2 is not free
        with pytest.raises(RuntimeError, match="out of range"):
            eng.beam_reorder(0, 1, [0, 1], [1, 2])
        assert eng.context_len(1) == -1 and eng.context_len(0) == 3
        eng.decode(1, batch=2)
        assert len(eng.beam_select(0, 1, [0.0], 2)) == 2  # after a decode step row i is slot i
        with pytest.raises(RuntimeError, match="holds no sequence"):
            eng.beam_select(0, 2, [0.0, 0.0], 2)
    finally:
        eng.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
E2E_PROMPT_SEED, E2E_PROMPT_LEN, NEW = 16, 21, 12


def host_beam_run(eng, prompt, num_beams, eos, length_penalty=1.0, early_stopping=False):
    """The policy over float64 selection on the host from copy_logits_into rows; with it the smallest gap, on those scores, at any
    place where a rounding of the device's fp32 scores could change what the search keeps: between the candidates ranked B and B + 1
    (who may finish), K and K + 1 (who is selected), the B-th and the next candidate that goes on (who runs); and the smallest gap
    between the returned hypotheses' scores (their order).  A kept and a dropped candidate that are equal logits of ONE row are no such
    place: their scores are the same number on the host and the same number on the device (one lse, one addition), and both sides
    cut between them by the lower token id.  On this checkpoint, whose rows hold one dominant logit over a tail of coarse bf16 values,
    such pairs sit at most cuts: over 72 prompts of 9, 21 and 37 tokens and three choices of EOS ids each, the smallest gap with those
    pairs counted was 0.0 every time; without them it is 0.0625 or 0.125 (one or two bf16 steps of a tail logit) for the prompt used."""
    from tiny_llm_hip.beam import beam_search

    buf = eng.logits_buffer(eng.max_batch)
    state = {"width": 0, "step": 0}
    gaps = []

    def select(scores, n_cand):
        rows = len(scores)
        eng.copy_logits_into(buf, rows)
        eng.synchronize()
        ranked = BO.beam_select(buf[:rows].float().cpu().numpy().astype(np.float64), scores, n_cand + 1)
        state["step"] += 1
        last = state["step"] >= NEW
        go_on = [c for c in ranked if not (last or c[1] in eos)]
        cuts = [(ranked, num_beams), (ranked, n_cand)] + ([(go_on, num_beams)] if len(go_on) > num_beams else [])
        for among, cut in cuts:
            kept, dropped = among[cut - 1], among[cut]
            if not (kept[0] == dropped[0] and kept[3] == dropped[3]):  # (equal logits of one row: see the docstring)
                gaps.append(kept[2] - dropped[2])
        return ranked[:n_cand]

    def advance(parents, tokens):
        eng.beam_reorder(0, max(state["width"], 1), parents, tokens)
        state["width"] = len(parents)
        eng.decode(1, batch=state["width"])

    eng.begin(0)
    try:
        eng.prefill(0, prompt)
        out = beam_search(select, advance, num_beams=num_beams, max_new_tokens=NEW, eos_ids=eos, length_penalty=length_penalty,
                          early_stopping=early_stopping)
    finally:
        for slot in range(max(state["width"], 1)):
            eng.release(slot)
    return out, min(gaps or [math.inf]), min([a[1] - b[1] for a, b in zip(out, out[1:])] or [math.inf])


@pytest.fixture(scope="module")
def e2e(peaked):
    """Two engines of 8 slots, the prompt, its greedy ids and the EOS ids: tokens the greedy continuation meets at its fifth and eighth
    step, so that hypotheses end on them before the length limit."""
    a, b = make_engine(peaked, num_pages=64, max_batch=8), make_engine(peaked, num_pages=64, max_batch=8)
    prompt = [int(t) for t in np.random.default_rng(E2E_PROMPT_SEED).integers(0, V, E2E_PROMPT_LEN)]
    greedy = a.generate(prompt, NEW)
    yield a, b, prompt, greedy, sorted({greedy[4], greedy[7]})
    a.close()
    b.close()


def test_one_beam_is_greedy_generation(e2e):
    from tiny_llm_hip.beam import beam_search_ids

    eng, _, prompt, greedy, _ = e2e
    (ids, score), = beam_search_ids(eng, prompt, 1, NEW)
    assert ids == greedy and score <= 0.0  # (the peaked checkpoint's greedy tokens have probability 1 to fp32)
    assert eng.stats()["pages_in_use"] == 0


@pytest.mark.parametrize("num_beams", [4, 8])
def test_device_selection_finds_the_hypotheses_of_host_selection(e2e, num_beams):
    from tiny_llm_hip.beam import beam_search_ids

    eng, host, prompt, _, eos = e2e
    want, gap, order_gap = host_beam_run(host, prompt, num_beams, eos)
    print(f"beams={num_beams} smallest kept/dropped gap {gap:.6f}, between hypotheses {order_gap:.6f}: {[(ids, round(s, 4)) for ids, s in want]}")
    assert gap > 2 * TOL * NEW, gap  # (about the host run: the device's fp32 scores cannot change what the search keeps)
    assert order_gap > 2 * TOL, order_gap  # (a hypothesis' score is its sum over its length: each side is within TOL)
    got = beam_search_ids(eng, prompt, num_beams, NEW, eos_ids=eos)
    assert [ids for ids, _ in got] == [ids for ids, _ in want]
    for (_, mine), (ids, theirs) in zip(got, want):
        assert abs(mine - theirs) <= TOL * NEW, (mine, theirs)
    assert any(ids[-1] in eos and len(ids) < NEW for ids, _ in got)  # a hypothesis ends on an EOS id before the limit
    assert eng.stats()["pages_in_use"] == 0 and host.stats()["pages_in_use"] == 0


def test_cli_num_beams_on_a_written_checkpoint(tmp_path, capsys):
    """main.py --num-beams: one beam prints what the greedy path prints; four beams with the other two flags print a hypothesis."""
    from checkpoint_fixture import write_checkpoint
    from oracle import tiny_oracle as O
    import main as cli

    words = [f"w{i}" for i in range(V - 2)]
    path = str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05), vocab_words=words))
    base = ["--model", path, "--prompt", "w5 w17 w400 w3", "--raw-prompt", "--max-new-tokens", "10"]
    greedy = cli.main(base)
    assert cli.main(base + ["--num-beams", "1"]) == greedy
    best = cli.main(base + ["--num-beams", "4", "--length-penalty", "0.6", "--early-stopping"])
    assert isinstance(best, str) and 1 <= len(best.split()) <= 10
    capsys.readouterr()
