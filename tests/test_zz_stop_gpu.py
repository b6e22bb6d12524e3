"""GPU tier: stop conditions on the device (tl_stop_create, tl_engine_set_stop, tl_engine_stop_state, tl_stop_rows; csrc/stop.h,
csrc/stop_set.h) against the plain-Python restatement of their definition (tests/stop_oracle.py).  Everything is exact: a stop record is
integers, and a slot that froze must stand where a run that made exactly that many tokens stands, bit for bit."""

import functools
import math
import os

import numpy as np
import pytest
import torch

from helpers import TINY_CFG
from stop_oracle import ID, LENGTH, NONE, STRING, stop_oracle

pytestmark = pytest.mark.gpu

REASON = {"none": NONE, "id": ID, "string": STRING, "length": LENGTH}


# -- tl_stop_rows against the oracle ------------------------------------------------------------------------------------------------
def _abc(rng, n):
    return bytes(rng.choice(list(b"abc"), n).tolist())


@functools.lru_cache(maxsize=None)
def rows_vocabulary():
    """Tokens of 0, 1, 3, 63, 64, 65 and 200 bytes over a three-letter alphabet (overlaps are dense), and two long tokens with a marker."""
    rng = np.random.default_rng(11)
    v = [b"", b"a", b"b", b"c", b"abc", b"cab", b"bca", _abc(rng, 63), _abc(rng, 64), _abc(rng, 65), _abc(rng, 200), b"ab", b"ca",
         b"q" * 120 + b"STOP" + b"r" * 76,   # 13: a match inside a 200-byte token
         b"ST", b"OP" + b"r" * 198,          # 14, 15: a match that ends in the second byte of a 200-byte token
         b"r" * 63 + b"ST", b"OP",           # 16, 17: ... and one that starts in the last bytes of a 65-byte token
         b"xyz", b"zz"]
    assert sorted({len(t) for t in v}) == [0, 1, 2, 3, 63, 64, 65, 200]
    return v


class RowsDevice:
    def __init__(self):
        from tiny_llm_hip.engine import Vocab
        from tiny_llm_hip.grammar import vocabulary_bytes_from_strings

        self.tokens = rows_vocabulary()
        self.vocab = Vocab(*vocabulary_bytes_from_strings(self.tokens))

    def stop_set(self, ids, strings, with_vocab=True):
        from tiny_llm_hip.stop import StopSet

        return StopSet(ids, strings, self.vocab if with_vocab else None, vocab_size=len(self.tokens)) if ids or strings else None


@pytest.fixture(scope="module")
def rows_dev():
    return RowsDevice()


def _run_rows(dev, ids, strings, sequences, rows, shift=0, with_vocab=True):
    """Row r follows sequences[(r + shift) % n] = (tokens, budget), one launch per token position; after every launch every row's
    record equals the oracle on the tokens so far.  Text is counted in the set's vocabulary: without a set, or with one made without
    a vocabulary, no token has bytes."""
    import tiny_llm_ext_hip as ext

    stop = dev.stop_set(ids, strings, with_vocab)
    texts = dev.tokens if stop is not None and with_vocab else [b""] * len(dev.tokens)
    seqs = [sequences[(r + shift) % len(sequences)] for r in range(rows)]
    steps = max(len(t) for t, _ in seqs)
    seqs = [(list(t) + [0] * (steps - len(t)), b) for t, b in seqs]  # (padded with the token that has no bytes)
    states = torch.zeros(rows, 6, dtype=torch.int32, device="cuda")
    automaton = torch.zeros(rows, dtype=torch.int32, device="cuda")
    budgets = torch.tensor([b for _, b in seqs], dtype=torch.int32, device="cuda")
    for k in range(steps):
        tokens = torch.tensor([t[k] for t, _ in seqs], dtype=torch.int32, device="cuda")
        ext.stop_rows(stop._h if stop is not None else None, tokens, states, automaton, budgets)
        got = states.cpu().numpy()
        for r, (t, b) in enumerate(seqs):
            want = stop_oracle(t[:k + 1], texts, ids, strings, b)
            assert tuple(int(x) for x in got[r][[0, 1, 2, 4, 5]]) == want, (ids, strings, t[:k + 1], b, r, got[r].tolist())
            assert got[r][3] == 0  # the context field is the engine's
    return states.cpu().numpy()


def _big_set():
    """16 strings of 64 bytes, 1,024 together: 15 random ones and one that lies inside the random 200-byte token."""
    rng = np.random.default_rng(5)
    strings = [rows_vocabulary()[10][100:164]]
    while len(strings) < 16:
        s = _abc(rng, 64)
        if s not in strings:
            strings.append(s)
    return strings


ROW_CASES = {
    # name: (ids, strings, [(tokens, budget)])
    "string over three tokens": ([], [b"abc"], [([1, 2, 5], 0), ([1, 0, 2, 0, 3], 0)]),
    "ends in mid-token": ([], [b"zc"], [([18, 5], 0)]),
    "two strings end on one byte": ([], [b"b", b"zab", b"yzab"], [([18, 11], 0), ([19, 11], 0)]),
    "aab and aaab": ([], [b"aab", b"aaab"], [([1, 1, 1, 2], 0), ([2, 1, 1, 2], 0), ([1, 1, 1, 1, 1, 11], 0)]),
    "inside the 200-byte token": ([], [b"STOP"], [([1, 13, 2], 0), ([14, 15], 0), ([16, 17], 0), ([16, 0, 17], 0), ([14, 1, 15], 0)]),
    "long tokens, short strings": ([], [b"abca", b"cc", b"bab"], [([7], 0), ([8], 0), ([9], 0), ([10], 0), ([3, 7, 8, 9, 10], 0)]),
    "16 ids": (list(range(4, 20)), [], [([1, 2, 3, 19], 0), ([0, 4], 0), ([3, 3, 3], 0)]),
    "the 1,024-byte set": ([], "big", [([1, 10, 2], 0), ([7, 8, 9], 0), ([9, 10], 0)]),
    "id and budget on one token": ([2], [], [([1, 2], 2)]),
    "string and budget on one token": ([], [b"ab"], [([1, 2], 2), ([3, 11], 2)]),
    "budget 1": ([], [b"zz"], [([4], 1), ([19], 1)]),
    "budget alone": ([], [], [([4, 4, 4], 2), ([1, 1, 1], 0)]),
    "an id whose bytes would complete a string": ([9, 2], [b"ab"], [([1, 2], 0), ([1, 1, 2, 11], 0)]),
}


@pytest.mark.parametrize("name", list(ROW_CASES))
def test_stop_rows_match_the_oracle(rows_dev, name):
    ids, strings, sequences = ROW_CASES[name]
    strings = _big_set() if strings == "big" else strings
    final = None
    for shift in range(len(sequences)):
        final = _run_rows(rows_dev, ids, strings, sequences, 1, shift)
    _run_rows(rows_dev, ids, strings, sequences, 2)
    final = _run_rows(rows_dev, ids, strings, sequences, 65)
    if not strings:  # a set of ids made without a vocabulary: the same stops, no text
        _run_rows(rows_dev, ids, strings, sequences, 65, with_vocab=False)
    if name not in ("budget alone", "16 ids"):
        assert (final[:, 0] != NONE).any(), "the case never stops"


def test_stop_rows_random_sets_and_sequences(rows_dev):
    rng = np.random.default_rng(3)
    V = len(rows_dev.tokens)
    for _ in range(12):
        strings = []
        while len(strings) < int(rng.integers(1, 6)):
            s = _abc(rng, int(rng.integers(1, 7 if rng.random() < 0.7 else 40)))
            if s not in strings:
                strings.append(s)
        ids = [int(t) for t in rng.choice(V, int(rng.integers(0, 4)), replace=False)]
        sequences = [([int(t) for t in rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], int(rng.integers(1, 7)))], int(rng.integers(0, 6))) for _ in range(13)]
        _run_rows(rows_dev, ids, strings, sequences, 65)


def test_stop_rows_leave_unarmed_and_stopped_rows_alone(rows_dev):
    import tiny_llm_ext_hip as ext

    stop = rows_dev.stop_set([2], [b"ab"])
    rows = 6
    states = torch.tensor([[0, 0, 0, 9, 0, 0], [ID, 3, 4, 5, 6, 6], [0, 7, 7, 7, 7, 7], [STRING, 1, 2, 3, 9, 4], [LENGTH, 0, 5, 5, 5, 5], [0, 0, 1, 0, 1, 1]],
                          dtype=torch.int32, device="cuda")
    automaton = torch.tensor([0, 1, 1, 1, 0, 1], dtype=torch.int32, device="cuda")  # (state 1: "a" has been seen)
    armed = torch.tensor([1, 1, 0, 1, 1, 1], dtype=torch.int32, device="cuda")
    before, before_a = states.clone(), automaton.clone()
    ext.stop_rows(stop._h, torch.full((rows,), 2, dtype=torch.int32, device="cuda"), states, automaton, torch.zeros(rows, dtype=torch.int32, device="cuda"), armed)
    got = states.cpu().numpy()
    for r in (1, 2, 3, 4):  # stopped before, or unarmed: bit-identical
        assert np.array_equal(got[r], before[r].cpu().numpy()) and int(automaton[r]) == int(before_a[r]), r
    assert got[0].tolist() == [ID, 0, 1, 9, 0, 0]  # token 2 is the stop id; the context field is not touched
    assert got[5].tolist() == [ID, 0, 2, 0, 1, 1]   # ... and wins over "ab", which its byte would complete


# -- the engine ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda")


@functools.lru_cache(maxsize=None)
def engine_vocabulary():
    """1,024 tokens: the single bytes, then seeded strings of 2-6 lowercase letters and spaces, the last four empty (the grammar's EOS)."""
    rng = np.random.default_rng(1024)
    letters = list(b"abcdefghijklmnopqrstuvwxyz ")
    tokens = [bytes([b]) for b in range(256)]
    tokens += [bytes(rng.choice(letters, int(rng.integers(2, 7))).tolist()) for _ in range(1020 - 256)] + [b""] * 4
    return tokens


class EngineDevice:
    def __init__(self):
        from tiny_llm_hip import grammar as G
        from tiny_llm_hip.engine import Grammar, Vocab
        from tiny_llm_hip.grammar import vocabulary_bytes_from_strings

        self.tokens = engine_vocabulary()
        self.vocab = Vocab(*vocabulary_bytes_from_strings(self.tokens))
        self.words = Grammar(self.vocab, G.compile_regex(rb"[a-z]+( [a-z]+)*"), [1023, 1022])

    def stop_set(self, ids=(), strings=()):
        from tiny_llm_hip.stop import StopSet

        return StopSet(ids, strings, self.vocab, vocab_size=len(self.tokens))


@pytest.fixture(scope="module")
def edev():
    return EngineDevice()


def _engine(model, n, route=None, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    old = os.environ.pop("TL_AQL", None)
    if route == "hipgraph":
        os.environ["TL_AQL"] = "0"
    try:
        return DecodeEngine(model, page_size=16, num_pages=16 * n + 32, max_batch=n, max_prefill_rows=64, **kw)
    finally:
        os.environ.pop("TL_AQL", None)
        if old is not None:
            os.environ["TL_AQL"] = old


PROMPTS = [[5, 17, 900, 33, 2], [7, 300, 301, 302, 9, 11, 500, 44, 3], [400 + i for i in range(12)], [600 + 7 * i for i in range(15)]]
KINDS = ("greedy", "sampled", "constrained", "mirostat")
STEPS, EXTRA = 24, 4


def _configure(eng, edev, slot, kind):
    if kind == "sampled":
        eng.set_sampling(slot, 0.8, seed=11)
    elif kind == "constrained":  # sampled + penalties + regex grammar + logprobs 3
        eng.set_penalties(slot, 1.3, 0.4, 0.2)
        eng.set_grammar(slot, edev.words)
        eng.set_sampling(slot, 0.8, seed=12)
        eng.set_logprobs(slot, 3)
    elif kind == "mirostat":
        eng.set_sampling(slot, 1.0, seed=13)
        eng.set_mirostat(slot, 3.0, 0.3)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().copy()


def _slot_state(eng, slot, kind):
    mu = eng.mirostat_mu(slot)
    return (eng.context_len(slot), None if math.isnan(mu) else mu, eng.grammar_config(slot) if kind == "constrained" else None)


def _step_rows(eng, n, kinds):
    rows = {"ids": eng.read_pending(n), "logits": _bits(eng.logits(n))}
    if "constrained" in kinds:
        rows["processed"] = _bits(eng.processed_logits(n))
    if "mirostat" in kinds:
        rows["filtered"] = _bits(eng.filtered_logits(n))
    return rows


def _begin_all(eng, edev, kinds, arm=None):
    for slot, kind in enumerate(kinds):
        eng.begin(slot)
        _configure(eng, edev, slot, kind)
        if arm is not None:
            eng.set_stop(slot, *arm[slot])
        eng.prefill(slot, PROMPTS[slot])


def _reference(eng, edev, kinds, steps):
    """The unarmed run, one step per call: per slot the ids, per step the rows of every kind and every slot's state; state[k] and
    rows[k] stand after k decode steps (rows[0]: none)."""
    n = len(kinds)
    _begin_all(eng, edev, kinds)
    out = [[t] for t in eng.read_pending(n)]
    states, rows = [[_slot_state(eng, s, kinds[s]) for s in range(n)]], [None]
    for _ in range(steps):
        eng.decode(1, batch=n)
        rows.append(_step_rows(eng, n, kinds))
        for s in range(n):
            out[s].append(rows[-1]["ids"][s])
        states.append([_slot_state(eng, s, kinds[s]) for s in range(n)])
    records = {s: eng.read_logprobs(s, steps + 1) for s in range(n) if kinds[s] == "constrained"}
    for s in range(n):
        eng.release(s)
    return out, states, rows, records


def _derive(out, tokens, first_choice):
    """A stop spec from the slot's own ids: (ids, strings, budget).  id: an id whose first occurrence is at step >= 3; string: the bytes
    from the middle of one produced token to the middle of the one after next; budget: 6."""
    id_at = next((k for k in range(3, len(out) - EXTRA) if out[k] not in out[:k]), None)
    str_at = next((k for k in range(2, len(out) - EXTRA - 2) if len(tokens[out[k]]) >= 2 and len(tokens[out[k + 2]]) >= 2), None)
    specs = {"budget": ((), (), 6)}
    if id_at is not None:
        specs["id"] = ((out[id_at],), (), 0)
    if str_at is not None:
        a, b, c = (tokens[out[str_at + j]] for j in range(3))
        specs["string"] = ((), (a[len(a) // 2:] + b + c[:max(1, len(c) // 2)],), 0)
    return next(specs[k] for k in first_choice if k in specs)


def _logprob_key(rec):
    return (np.float32(rec.logprob).tobytes(), tuple((i, np.float32(v).tobytes()) for i, v in rec.top))


def _freeze_check(model, edev, kinds, orders, **kw):
    n = len(kinds)
    eng = _engine(model, n, **kw)
    out, states, rows, records = _reference(eng, edev, kinds, STEPS + EXTRA)
    specs = [_derive(out[s][:STEPS + 1], edev.tokens, orders[s]) for s in range(n)]
    # (a budget alone arms the slot without a set, so without a vocabulary: no token has bytes there)
    texts = [edev.tokens if specs[s][0] or specs[s][1] else [b""] * len(edev.tokens) for s in range(n)]
    want = [stop_oracle(out[s][:STEPS + 1], texts[s], *specs[s]) for s in range(n)]
    print("specs", specs, "oracle", want)
    sets = [edev.stop_set(ids, strings) if ids or strings else None for ids, strings, _ in specs]
    # the armed run: one call
    _begin_all(eng, edev, kinds, arm=[(sets[s], specs[s][2]) for s in range(n)])
    assert "stop" in eng.replay_route()
    eng.decode(STEPS, batch=n)
    for s in range(n):
        st = eng.stop_state(s)
        g = want[s][2]
        assert (REASON[st.reason], st.index, st.generated, st.text_bytes, st.cut_bytes) == want[s], (s, st, want[s])
        assert st.context == states[g - 1][s][0] == eng.context_len(s)
        assert eng.read_tokens(s, g) == out[s][:g]
        assert eng.read_pending(n)[s] == out[s][g - 1]
        if kinds[s] == "constrained":
            assert [_logprob_key(r) for r in eng.read_logprobs(s, g)] == [_logprob_key(r) for r in records[s][:g]]
        assert _slot_state(eng, s, kinds[s]) == states[g - 1][s], (s, _slot_state(eng, s, kinds[s]), states[g - 1][s])
    # disarmed, every slot goes on from where its text really ended: the next EXTRA steps are the reference's, bit for bit
    for s in range(n):
        eng.set_stop(s, None, 0)
        assert eng.stop_state(s).reason == "none"
    for j in range(1, EXTRA + 1):
        eng.decode(1, batch=n)
        got = _step_rows(eng, n, kinds)
        for s in range(n):
            ref = rows[want[s][2] - 1 + j]
            assert got["ids"][s] == ref["ids"][s], (s, j)
            for key in ("logits", "processed", "filtered"):
                if key in got:
                    assert np.array_equal(got[key][s], ref[key][s]), (s, j, key)
    for s in range(n):
        assert _slot_state(eng, s, kinds[s]) == states[want[s][2] - 1 + EXTRA][s]
        eng.release(s)
    eng.close()
    return want


def test_a_stopped_slot_freezes_where_its_text_ended(tiny, edev):
    """Four slots (greedy; sampled; sampled + penalties + grammar + logprobs; Mirostat), each armed from the unarmed run's own ids."""
    want = _freeze_check(tiny, edev, KINDS, [("id", "string", "budget"), ("string", "id", "budget"), ("budget",), ("id", "string", "budget")])
    assert {w[0] for w in want} == {ID, STRING, LENGTH}, want
    assert all(w[2] <= STEPS for w in want)


def test_freeze_on_fp8_kv_pages(tiny, edev):
    want = _freeze_check(tiny, edev, KINDS[:1], [("id", "string", "budget")], kv_format="fp8")
    assert want[0][0] in (ID, STRING) and want[0][2] >= 3


def test_the_first_token_can_stop(tiny, edev):
    eng = _engine(tiny, 2)
    eng.begin(0)
    eng.prefill(0, PROMPTS[0])
    first = eng.read_tokens(0, 1)[0]
    eng.release(0)
    stop = edev.stop_set([3, first])
    for slot in (0, 1):
        eng.begin(slot)
        eng.set_stop(slot, stop if slot == 0 else None, 0 if slot == 0 else 9)
        eng.prefill(slot, PROMPTS[0])
    st = eng.stop_state(0)
    assert (st.reason, st.index, st.generated, st.context, st.text_bytes, st.cut_bytes) == ("id", 1, 1, len(PROMPTS[0]), 0, 0)
    eng.decode(4, batch=2)
    assert eng.stop_state(0) == st and eng.read_tokens(0, 1) == [first] and eng.context_len(0) == len(PROMPTS[0])
    assert eng.read_pending(2)[0] == first
    assert eng.stop_state(1).generated == 5 and eng.context_len(1) == len(PROMPTS[0]) + 4  # the neighbour ran
    eng.release(0)
    eng.release(1)
    eng.close()


def _snapshot(eng, slot, g):
    return (eng.stop_state(slot), eng.read_tokens(slot, g), eng.context_len(slot), eng.read_pending(slot + 1)[slot])


def test_a_stopped_slot_is_inert_and_slot_calls_carry_the_state(tiny, edev):
    eng = _engine(tiny, 4, swap_pages=16)
    base = {k: eng.stats()[k] for k in ("pages_in_use", "pages_free")}
    for slot in (0, 1):
        eng.begin(slot)
        if slot == 0:
            eng.set_stop(0, None, 3)
        eng.prefill(slot, PROMPTS[slot])
    eng.decode(6, batch=4)
    snap = _snapshot(eng, 0, 3)
    assert (snap[0].reason, snap[0].generated, snap[2]) == ("length", 3, len(PROMPTS[0]) + 2)
    assert eng.context_len(1) == len(PROMPTS[1]) + 6
    eng.decode(3, batch=4)
    assert _snapshot(eng, 0, 3) == snap and eng.context_len(1) == len(PROMPTS[1]) + 9
    ids = snap[1]
    # move carries, fork copies (the ring restarts with a move, so the ids are read through the pending token and the state)
    eng.move(0, 2)
    eng.fork(2, 3)
    eng.decode(2, batch=4)
    for slot in (2, 3):
        assert eng.stop_state(slot) == snap[0] and eng.context_len(slot) == snap[2] and eng.read_pending(4)[slot] == ids[-1], slot
    # park / unpark keep it
    eng.park(2)
    eng.decode(1, batch=4)
    eng.unpark(2)
    eng.decode(1, batch=4)
    assert eng.stop_state(2) == snap[0] and eng.context_len(2) == snap[2] and eng.read_pending(4)[2] == ids[-1]
    # feeding a stopped slot is refused, nothing changed; a rewind and set_token work
    with pytest.raises(RuntimeError, match="stopped"):
        eng.prefill(2, [5, 6])
    with pytest.raises(RuntimeError, match="stopped"):
        eng.prefill_packed([(2, [5], True)])
    assert eng.stop_state(2) == snap[0] and eng.context_len(2) == snap[2]
    eng.rewind(3, 1)
    eng.set_token(3, 77)
    assert eng.stop_state(3).reason == "length" and eng.context_len(3) == snap[2] - 1
    # resumed, the moved slot is the sequence it was: its next token is the one an unarmed engine makes after the same three
    eng.set_stop(2, None, 0)
    eng.decode(1, batch=4)
    nxt = eng.read_pending(3)[2]
    for slot in (1, 2, 3):
        eng.release(slot)
    eng.begin(2)
    st = eng.stop_state(2)
    assert (st.reason, st.generated, st.text_bytes) == ("none", 0, 0)
    eng.prefill(2, PROMPTS[0])
    eng.decode(3, batch=4)
    assert eng.read_tokens(2, 4) == ids + [nxt]
    eng.release(2)
    assert {k: eng.stats()[k] for k in base} == base
    eng.close()


def _route_run(eng, edev, arm):
    eng.begin(0)
    if arm:
        eng.set_stop(0, *arm)
    eng.prefill(0, PROMPTS[1])
    eng.decode(8, batch=1)
    g = eng.stop_state(0).generated if arm else 9
    out = (eng.read_tokens(0, g), eng.stop_state(0))
    eng.release(0)
    return out


def test_routes_and_plans(tiny, edev):
    never = _engine(tiny, 1)
    _route_run(never, edev, None)
    plain = (never.replay_route(), never.stats()["graph_captures"], never.stats()["aql_steps"])
    never.close()
    eng = _engine(tiny, 1)
    eng.begin(0)
    eng.set_stop(0, None, 5)
    eng.set_stop(0, None, 0)  # armed and disarmed before anything ran: the engine it was
    eng.release(0)
    ids_plain, _ = _route_run(eng, edev, None)
    assert (eng.replay_route(), eng.stats()["graph_captures"], eng.stats()["aql_steps"]) == plain
    # one armed slot: a plan of its own, and the route says why
    stop = edev.stop_set([ids_plain[5]])
    eng.begin(0)
    eng.set_stop(0, stop, 0)
    assert eng.replay_route().startswith("hipgraph") and "stop" in eng.replay_route()
    eng.release(0)
    assert eng.replay_route() == plain[0]
    ids_armed, st = _route_run(eng, edev, (stop, 0))
    captures = eng.stats()["graph_captures"]
    assert captures == plain[1] + 1 and eng.stats()["aql_steps"] == plain[2]
    assert st.reason == "id" and ids_armed == ids_plain[:st.generated] and ids_armed[-1] == ids_plain[5]
    # disarmed again: the unarmed plan, nothing captured anew
    assert _route_run(eng, edev, None)[0] == ids_plain
    assert eng.stats()["graph_captures"] == captures and eng.replay_route() == plain[0]
    eng.close()
    # the other route: identical ids and states
    other = _engine(tiny, 1, route="hipgraph")
    assert _route_run(other, edev, None)[0] == ids_plain
    got = _route_run(other, edev, (stop, 0))
    assert got == (ids_armed, st)
    other.close()


# -- Python ---------------------------------------------------------------------------------------------------------------------------
def test_generate_with_stop_returns_the_prefix(tiny, edev):
    eng = _engine(tiny, 1)
    prompt = PROMPTS[1]
    full, full_lp = eng.generate(prompt, 25, logprobs=2)
    id_spec = _derive(full, edev.tokens, ("id",))
    str_spec = _derive(full, edev.tokens, ("string",))
    for ids, strings, _ in (id_spec, str_spec):
        want = stop_oracle(full, edev.tokens, ids, strings, 25)
        assert want[0] in (ID, STRING)
        got, got_lp = eng.generate(prompt, 25, logprobs=2, stop=eng.make_stop_set(ids, strings, vocab=edev.vocab), decode_block=4)
        assert got == full[:want[2]]
        assert [_logprob_key(r) for r in got_lp] == [_logprob_key(r) for r in full_lp[:want[2]]]
    # the budget alone ends the call where the plain call ends
    absent = next(t for t in range(1024) if t not in full)
    assert eng.generate(prompt, 7, stop=eng.make_stop_set([absent]), decode_block=32) == full[:7]
    assert eng.stats()["pages_in_use"] == 0
    eng.close()


@pytest.mark.parametrize("cache", [False, True])
def test_batch_generate_ids_with_device_stops_equals_the_host_comparison(tiny, edev, cache):
    from tiny_llm_hip.engine import batch_generate_ids

    rng = np.random.default_rng(2)
    prompts = [[int(t) for t in rng.integers(0, 1000, int(rng.integers(5, 14)))] for _ in range(6)]
    eng = _engine(tiny, 4, prefix_cache=cache)
    free = dict(batch_generate_ids(eng, prompts, 12, batch_size=3, prefill_step=8))
    # an id that ends some requests early and leaves others to their budget
    counts = {}
    for ids in free.values():
        for t in set(ids[2:10]):
            counts[t] = counts.get(t, 0) + 1
    eos = min(counts, key=lambda t: (abs(counts[t] - 3), t))
    if cache:
        eng.prefix_clear()
    want = batch_generate_ids(eng, prompts, 12, batch_size=3, prefill_step=8, eos_token_id=eos)
    assert any(len(ids) < 12 for _, ids in want) and all(ids[-1] == eos or len(ids) == 12 for _, ids in want)
    stop = eng.make_stop_set([eos])
    for block in (1, 8):
        if cache:
            eng.prefix_clear()
        got = batch_generate_ids(eng, prompts, 12, batch_size=3, prefill_step=8, stop=stop, decode_block=block)
        assert dict(got) == dict(want), block
        if block == 1:
            assert got == want
        assert eng.stats()["pages_in_use"] == 0
    eng.close()


def test_cli_stop_flags_on_a_written_checkpoint(tmp_path, capsys):
    """main.py / batch_main.py --stop-id and --stop on a checkpoint directory with a word-level tokenizer (token i + 2 spells "w<i>")."""
    from checkpoint_fixture import write_checkpoint
    from oracle import tiny_oracle as O
    import batch_main
    import main as cli

    words = [f"w{i}" for i in range(TINY_CFG["vocab_size"] - 2)]
    path = str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05), vocab_words=words))
    base = ["--model", path, "--prompt", "w5 w17 w400 w3", "--raw-prompt", "--max-new-tokens", "10"]
    greedy = cli.main(base).split()
    assert len(greedy) >= 4 and all(w in words for w in greedy), greedy
    k = next(i for i in range(1, len(greedy)) if greedy[i] not in greedy[:i])
    # a stop id ends the answer ahead of that token; another id that never comes changes nothing
    assert cli.main(base + ["--stop-id", str(words.index(greedy[k]) + 2), "--stop-id", "1"]).split() == greedy[:k]
    # a stop string cuts the text -- the tokens' bytes, which this tokenizer spells without spaces -- ahead of its first match
    raw = "".join(greedy)
    assert cli.main(base + ["--stop", greedy[k], "--stop", "never"]) == raw[:raw.find(greedy[k])]
    assert cli.main(base + ["--stop", "never"]).split() == greedy  # (no match: the budget ends it, the tokenizer spells the answer)
    # the device sampler takes the set too
    sampled = cli.main(base + ["--sampler-temp", "0.8", "--sampler-seed", "3"]).split()
    j = next(i for i in range(1, len(sampled)) if sampled[i] not in sampled[:i])
    assert cli.main(base + ["--sampler-temp", "0.8", "--sampler-seed", "3", "--stop-id", str(words.index(sampled[j]) + 2)]).split() == sampled[:j]
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("w5 w6 w7\nw8 w9\nw10 w11 w12 w13\n")
    batch = ["--model", path, "--batch-size", "2", "--prefill-step", "16", "--max-seq-len", "24", "--raw-prompts", "--prompts-file", str(prompts)]
    plain = dict(batch_main.main(batch))
    word = plain[0].split()[1]
    done = dict(batch_main.main(batch + ["--stop-id", str(words.index(word) + 2)]))
    assert sorted(done) == [0, 1, 2] and all(word not in text.split() for text in done.values())
    assert done[0].split() == plain[0].split()[:1]  # (request 0 runs the same steps up to there: admitted first, nothing retires earlier)
    cut = dict(batch_main.main(batch + ["--stop", word]))
    assert sorted(cut) == [0, 1, 2] and all(word not in text for text in cut.values()) and cut[0] == plain[0].split()[0]
    capsys.readouterr()
