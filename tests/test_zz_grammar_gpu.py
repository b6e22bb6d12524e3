"""GPU tier: regex-constrained decoding on the device (tl_vocab_create, tl_grammar_create, tl_engine_set_grammar,
tl_engine_grammar_state, tl_grammar_mask_rows; csrc/grammar.h, csrc/logit_process.h) against the plain-Python restatement of its
definition (tests/grammar_oracle.py), with the choice on the processed row checked by tests/sampling_oracle.py -- a produced id must
equal the oracle's unless the sampling oracle flags the draw ambiguous, and at most 10 % of the draws a test checks may be flagged, as in
tests/test_zz_logit_processing_gpu.py -- and, end to end, against Python's ``re``.

The tests keep every slot's automaton state and history on the host by the header's rule: the pending token advances the state (and is
counted) at the start of the decode step that feeds it back."""

import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import grammar_oracle as GO
import logit_processing_oracle as P
import sampling_oracle as S
from helpers import QWEN4B_CFG, TINY_CFG

pytestmark = pytest.mark.gpu

NEUTRAL = (1.0, 0.0, 0.0)
NUMBER = rb"-?(0|[1-9][0-9]{0,5})(\.[0-9]{1,3})?"
JSONISH = rb'\{"id": [0-9]{1,4}, "ok": (true|false)\}'
RECORD = rb'\{"name": "[^"]*", "n": -?(0|[1-9][0-9]{0,5})\}'  # small (< 64 states), with a state most tokens stay alive in
WORDS = rb"[a-z]+( [a-z]+)*"
ALPHABET = b'0123456789abcdefghijklmnopqrstuvwxyz{}":,.- '
UTF8 = ["é", "ü", "ñ", "€", "日", "本"]


# -- vocabularies and automata ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vocabulary(V):
    """V = 1,024: ids 0-255 the single bytes, 256-1,019 seeded random strings of 2-6 bytes over ALPHABET plus a few 2-3-byte UTF-8
    characters, 1,020-1,023 empty.  Larger V: the single bytes, strings of 1-16 bytes, ~200 tokens of 64-200 bytes, a few of 15-18, 16 empty ones
    (the last four among them).  EOS = {V - 1, V - 2}."""
    rng = np.random.default_rng(V)
    pieces = [bytes([c]) for c in ALPHABET] + [u.encode() for u in UTF8]

    def text(lo, hi):
        out = b""
        n = int(rng.integers(lo, hi + 1))
        while len(out) < n:
            out += pieces[int(rng.integers(0, len(pieces)))]
        return out[:hi]

    tokens = [bytes([b]) for b in range(256)]
    if V == 1024:
        tokens += [text(2, 6) for _ in range(1020 - 256)] + [b""] * 4
    else:
        tokens += [text(1, 16) for _ in range(V - 256)]
        letters = [bytes([c]) for c in b"abcdefghijklmnopqrstuvwxyz ,.-0123456789"]
        for j in rng.choice(np.arange(256, V - 4), 200, replace=False):
            n = int(rng.integers(64, 201))
            tokens[int(j)] = b"".join(letters[int(k)] for k in rng.integers(0, len(letters), n)) if rng.random() < 0.7 else b" " * n
        for j in rng.choice(np.arange(256, V - 4), 12, replace=False):
            tokens[int(j)] = b""
        tokens[V - 4:] = [b""] * 4
        # around the length above which the engine looks a token up instead of walking it (16 bytes)
        tokens[300:306] = [b"a" * 16, b"a" * 17, b"abcdefghijklmnop\"", b"abcdefghijklmno\"", b" " * 18, b"x" * 15 + b"\xc3\xa9"]
    assert len(tokens) == V
    return tokens


def eos_ids(V):
    return [V - 1, V - 2]


@functools.lru_cache(maxsize=None)
def big_choice():
    """An enum of random words whose minimal DFA has more than 2,048 states: beyond any table an LDS budget holds."""
    from tiny_llm_hip import grammar as G

    rng = np.random.default_rng(5)
    words = sorted({bytes(rng.choice(list(b"abcdefghijklmnopqrstuvwxyz0123456789 "), int(rng.integers(5, 14))).tolist()) for _ in range(700)})
    return G.choice(words), words


@functools.lru_cache(maxsize=None)
def dfa_of(pattern):
    from tiny_llm_hip import grammar as G

    return G.compile_regex(pattern)


@functools.lru_cache(maxsize=None)
def oracle_of(pattern, V):
    d = dfa_of(pattern)
    return GO.Grammar(d.table, d.accepting, d.start, vocabulary(V), eos_ids(V))


class Device:
    """The device side of a vocabulary and the grammars made over it, kept alive while engines use them."""

    def __init__(self, V):
        from tiny_llm_hip.engine import Grammar, Vocab
        from tiny_llm_hip.grammar import vocabulary_bytes_from_strings

        self.V = V
        self.vocab = Vocab(*vocabulary_bytes_from_strings(vocabulary(V)))
        self._make = lambda pattern: Grammar(self.vocab, dfa_of(pattern), eos_ids(V))
        self.grammars = {}

    def grammar(self, pattern):
        if pattern not in self.grammars:
            self.grammars[pattern] = self._make(pattern)
        return self.grammars[pattern]

    def close(self):
        for g in self.grammars.values():
            g.close()
        self.vocab.close()


@pytest.fixture(scope="module")
def dev_tiny():
    d = Device(1024)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev_big():
    d = Device(151936)
    yield d
    d.close()


@pytest.fixture(scope="module")
def tiny():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(TINY_CFG, seed=3, sigma=0.05, device="cuda")


@pytest.fixture(scope="module")
def q4b():
    from tiny_llm_hip.synthetic import synthetic_qwen3

    return synthetic_qwen3(dict(QWEN4B_CFG, num_hidden_layers=2), seed=11, sigma=0.02, device="cuda")


def text_of(ids, V):
    tokens = vocabulary(V)
    return b"".join(tokens[t] for t in ids)


def before_eos(ids, V):
    """(ids before the first EOS id, whether an EOS id was produced)"""
    for k, t in enumerate(ids):
        if t in eos_ids(V):
            return list(ids[:k]), True
    return list(ids), False


def follows(g, ids):
    """whether every id is allowed in the state the ids before it lead to"""
    state = g.start
    for t in ids:
        if not g.allowed(state)[t]:
            return False
        state = g.advance(state, t)
    return True


# -- 1. the kernel, bit for bit -----------------------------------------------------------------------------------------------------
def _states(g, pattern):
    """start, END, an accepting state, a non-accepting one, the state after a long walk -- 8 rows"""
    accepting = next(s for s in range(len(g.accepting)) if g.accepting[s])
    plain = next(s for s in range(len(g.accepting)) if not g.accepting[s] and s != g.start)
    if pattern == RECORD:
        deep = g.alive(b'{"name": "some words, 42 of them')   # inside [^"]*: most long tokens stay alive
        late = g.alive(b'{"name": "x", "n": -12')
    else:
        word = big_choice()[1][17]
        deep, late = g.alive(word[:len(word) - 1]), g.alive(word)
    assert deep is not GO.DEAD and late is not GO.DEAD
    return [g.start, GO.END, accepting, plain, deep, late, g.start, deep]


@pytest.mark.parametrize("V", [1024, 151936, 151941])
@pytest.mark.parametrize("which", ["small", "large"])
def test_mask_rows_bit_for_bit(V, which):
    import tiny_llm_ext_hip as ext

    pattern = RECORD if which == "small" else big_choice()[0]
    g = oracle_of(pattern, V)
    assert (len(g.accepting) < 64) if which == "small" else (len(g.accepting) >= 2048)
    dev = Device(V)
    try:
        rng = np.random.default_rng(V)
        states = _states(g, pattern)
        rows = []
        for i in range(len(states)):
            l = rng.standard_normal(V).astype(np.float32) * 2.0
            at = rng.choice(V, 600, replace=False)
            l[at[:150]], l[at[150:300]], l[at[300:450]], l[at[450:]] = np.nan, np.inf, -np.inf, -0.0
            if i == 0:  # specials on allowed and on disallowed tokens alike: the single bytes and the EOS ids
                l[0:256:4], l[1:256:4], l[2:256:4] = np.nan, -0.0, np.inf
                l[V - 2] = np.nan
            rows.append(P.bf16_round(l))
        logits = torch.from_numpy(np.stack(rows)).bfloat16().cuda()
        raw = logits.view(torch.int16).cpu().numpy().view(np.uint16)
        out = torch.empty_like(logits)
        st = torch.tensor(states, dtype=torch.int32, device="cuda")
        ext.check(ext.lib().tl_grammar_mask_rows(dev.grammar(pattern)._h, logits.data_ptr(), len(states), st.data_ptr(), out.data_ptr(), None))
        torch.cuda.synchronize()
        got = out.view(torch.int16).cpu().numpy().view(np.uint16)
        for i, s in enumerate(states):
            ok = g.allowed(s)
            want = P.bits(GO.mask_row(P.from_bits(raw[i]), g, s))  # the element itself (NaN payloads and -0.0 included), else -inf
            assert np.array_equal(want, np.where(ok, raw[i], np.uint16(0xFF80)))
            bad = np.flatnonzero(got[i] != want)
            assert bad.size == 0, (f"V {V}, row {i}, state {s}: {bad.size} elements differ, first at {bad[:4]} (tokens "
                                   f"{[vocabulary(V)[j] for j in bad[:4]]}): got {got[i][bad[:4]]}, want {want[bad[:4]]}")
            if s == GO.END:
                assert sorted(np.flatnonzero(ok)) == sorted(eos_ids(V))
            else:
                assert ok[eos_ids(V)].all() == bool(g.accepting[s]) and not ok[V - 3]
        # the rows discriminate: the start state allows something, and not everything
        assert 0 < g.allowed(states[0]).sum() < V
        if which == "small":
            long_alive = [j for j in np.flatnonzero(g.allowed(states[4])) if len(vocabulary(V)[j]) >= 64]
            assert V == 1024 or len(long_alive) >= 50, "the deep state keeps long tokens alive"
    finally:
        dev.close()


# -- the engine beside the oracle ---------------------------------------------------------------------------------------------------
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


def _cfg(pen=NEUTRAL, bias=None, smp=(0.0, 0, 1.0, 0), grammar=None):
    return {"pen": pen, "bias": dict(bias or {}), "smp": smp, "grammar": grammar}


def _mixed(i, V, small=True):
    """Slot i's settings by i % 6: no grammar; grammar greedy; grammar sampled; grammar + penalties + bias, sampled; a different grammar
    (the large automaton); bias only.  The sampler settings are those of tests/test_zz_logit_processing_gpu.py."""
    rng = np.random.default_rng(1000 + i)
    bias = {int(t): float(np.float32(v)) for t, v in zip(rng.choice(V, 16, replace=False), rng.standard_normal(16) * 2.0)}
    bias[int(rng.integers(0, V))] = -math.inf
    bias[ord("{")] = 3.0  # ... and entries on tokens the grammar decides about: allowed at the start of RECORD, disallowed later
    bias[ord("z")] = 100.0
    smp = [(0.8, 50, 1.0), (0.8, 20, 0.8), (0.8, 0, 1.0) if small else (0.7, 40, 1.0)][(i // 6) % 3]
    kind = i % 6
    if kind == 0:
        return _cfg()
    if kind == 1:
        return _cfg(grammar=RECORD)
    if kind == 2:
        return _cfg(grammar=[RECORD, NUMBER, JSONISH][(i // 6) % 3], smp=(*smp, 100 + i))
    if kind == 3:
        return _cfg(pen=(1.2, 0.4, 0.1), bias=bias, smp=(*smp, 100 + i), grammar=RECORD)
    if kind == 4:
        return _cfg(grammar=big_choice()[0], smp=(0.0, 0, 1.0, 0) if (i // 6) % 2 == 0 else (*smp, 100 + i))
    return _cfg(bias=bias)


class Sim:
    """An engine and, beside it, what the header says it holds: per slot the settings, the history, the automaton state (without the
    pending token) and the pending token."""

    def __init__(self, model, n, dev, route=None, **kw):
        self.eng = _engine(model, n, route, **kw)
        self.dev = dev
        self.V = self.eng.vocab_size
        self.cfg, self.hist, self.state, self.pending, self.out = {}, {}, {}, {}, {}
        self.draws = self.ambiguous = 0

    def close(self):
        self.eng.close()

    def grammar(self, slot):
        p = self.cfg[slot]["grammar"]
        return oracle_of(p, self.V) if p is not None else None

    def processes(self, slot):
        c = self.cfg[slot]
        return bool(P.processes(*c["pen"], c["bias"])) or c["grammar"] is not None

    def configure(self, slot, cfg):
        """the engine calls of a fresh slot's settings (before its prefill)"""
        self.cfg[slot] = cfg
        if cfg["grammar"] is not None:
            self.eng.set_grammar(slot, self.dev.grammar(cfg["grammar"]))
            self.state[slot] = self.grammar(slot).start
        if cfg["pen"] != NEUTRAL:
            self.eng.set_penalties(slot, *cfg["pen"])
        if cfg["bias"]:
            self.eng.set_logit_bias(slot, cfg["bias"])
        T, k, p, seed = cfg["smp"]
        if T > 0:
            self.eng.set_sampling(slot, T, k or None, p if p < 1 else None, seed)
        self.hist[slot] = P.History(self.V)

    def check(self, slot, got, raw_row, position):
        c = self.cfg[slot]
        g = self.grammar(slot)
        if self.processes(slot):
            row = GO.process(raw_row, self.hist[slot].prompt, self.hist[slot].count, *c["pen"], c["bias"], grammar=g,
                             state=self.state.get(slot))
        else:
            row = raw_row
        want, amb = S.sample(row, *c["smp"][:3], c["smp"][3], position)
        self.draws += 1
        self.ambiguous += bool(amb)
        assert got == want or amb, (slot, got, want, c["smp"], self.state.get(slot))
        if g is not None:
            assert g.allowed(self.state[slot])[got], f"slot {slot} produced token {got} that state {self.state[slot]} does not allow"
            state, accepting = self.eng.grammar_state(slot)
            after = g.advance(self.state[slot], got)
            assert state == after and accepting == (after == GO.END or g.accepting[after]), (slot, state, after, accepting)

    def start(self, slot, cfg, prompt, chunk=None):
        self.eng.begin(slot)
        self.configure(slot, cfg)
        self.eng.prefill(slot, prompt, chunk=chunk)
        self.consumed(slot, prompt)
        self.first_token(slot)

    def consumed(self, slot, tokens):
        if self.processes(slot):
            self.hist[slot].consume_prompt(tokens)

    def first_token(self, slot, row=0, rows=1):
        got = self.eng.read_tokens(slot, 1)[0]
        raw = self.eng.logits(rows).float().cpu().numpy()[row]
        self.check(slot, got, raw, self.eng.context_len(slot))
        self.pending[slot] = got
        self.out[slot] = [got]

    def feed(self, live):
        """the step's input token is counted, and advances the state, before the step's row is processed"""
        for i in live:
            if self.processes(i):
                self.hist[i].feed(self.pending[i])
            if self.cfg[i]["grammar"] is not None:
                self.state[i] = self.grammar(i).advance(self.state[i], self.pending[i])

    def step(self, n, use_graph=True, check=True):
        live = [i for i in range(n) if i in self.cfg and self.eng.context_len(i) >= 0]
        ctx = {i: self.eng.context_len(i) for i in live}
        self.feed(live)
        self.eng.decode(1, batch=n, use_graph=use_graph)
        got = self.eng.read_pending(n)
        raw = self.eng.logits(n).float().cpu().numpy() if check else None
        for i in live:
            if check:
                self.check(i, got[i], raw[i], ctx[i] + 1)
            self.pending[i] = got[i]
            self.out[i].append(got[i])
        return raw

    def assert_few_ambiguous(self):
        assert self.draws > 0 and self.ambiguous <= 0.1 * self.draws, f"{self.ambiguous} of {self.draws} draws flagged ambiguous"


def _mixed_run(model, n, steps, dev, small=True, route=None, use_graph=True, check=True, first=0, **kw):
    sim = Sim(model, n, dev, route, **kw)
    try:
        rng = np.random.default_rng(n)
        for i in range(n):
            sim.start(i, _mixed(i + first, sim.V, small), rng.integers(0, 1000, 5 + i % 11).tolist())
        for _ in range(steps):
            sim.step(n, use_graph=use_graph, check=check)
        return sim
    except Exception:
        sim.close()
        raise


# -- 2. the engine step by step, both routes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 17, 64])
def test_engine_every_step_matches_oracle(tiny, dev_tiny, n):
    first = 3 if n == 1 else 0  # one slot: grammar + penalties + bias, sampled
    a = _mixed_run(tiny, n, 24, dev_tiny, first=first)
    b = c = None
    try:
        assert a.eng.replay_route() == "aql"
        a.assert_few_ambiguous()
        sa = a.eng.stats()
        assert sa["graph_replays"] == 23 and sa["aql_steps"] == sa["graph_replays"], sa  # the grammar plan replays as AQL packets
        b = _mixed_run(tiny, n, 24, dev_tiny, first=first, route="hipgraph", check=False)
        c = _mixed_run(tiny, n, 24, dev_tiny, first=first, use_graph=False, check=False)
        assert b.eng.replay_route().startswith("hipgraph") and b.eng.stats()["aql_steps"] == 0
        assert a.out == b.out == c.out
        for i in range(n):  # what the constrained slots wrote is text of their language, so far
            if a.cfg[i]["grammar"] is not None:
                ids, ended = before_eos(a.out[i], a.V)
                g = a.grammar(i)
                s = g.alive(text_of(ids, a.V))
                assert s is not GO.DEAD and (not ended or g.accepting[s]), (i, text_of(ids, a.V))
    finally:
        for s in (a, b, c):
            if s is not None:
                s.close()


# -- 3. end to end against Python's re ----------------------------------------------------------------------------------------------
def _generate(model, dev, pattern, smp, steps, prompt, **kw):
    eng = _engine(model, 2, **kw)
    try:
        eng.begin(0)
        if pattern is not None:
            eng.set_grammar(0, dev.grammar(pattern))
        if smp[0] > 0:
            eng.set_sampling(0, smp[0], smp[1] or None, smp[2] or None, smp[3])
        eng.prefill(0, prompt)
        eng.decode(steps, batch=1)
        return eng.read_tokens(0, steps + 1)
    finally:
        eng.close()


@pytest.mark.parametrize("pattern", [NUMBER, JSONISH, "choice"])
def test_bounded_patterns_fullmatch(tiny, dev_tiny, pattern):
    if pattern == "choice":
        from tiny_llm_hip import grammar as G

        pattern = G.choice(["red", "green", "dark blue", "0.5", "é-ü", '{"a": 1}'])
    prompt = list(range(100, 112))
    for smp in ((0.0, 0, 0.0, 0), (0.9, 40, 0.0, 7), (1.5, 0, 0.0, 8)):
        ids = _generate(tiny, dev_tiny, pattern, smp, 32, prompt)
        text, ended = before_eos(ids, 1024)
        assert ended, "a bounded language forces an EOS id within 32 steps"
        assert re.fullmatch(pattern, text_of(text, 1024)), (smp, text_of(text, 1024))
        # after an EOS id is fed the slot only produces EOS ids
        assert all(t in eos_ids(1024) for t in ids[len(text):])
        # the discriminating control: the same slot without a grammar writes something else
        free, _ = before_eos(_generate(tiny, dev_tiny, None, smp, 32, prompt), 1024)
        assert not re.fullmatch(pattern, text_of(free, 1024))


def test_unbounded_pattern_stays_viable(tiny, dev_tiny):
    g = oracle_of(WORDS, 1024)
    for smp in ((0.0, 0, 0.0, 0), (1.0, 0, 0.0, 3)):
        ids = _generate(tiny, dev_tiny, WORDS, smp, 24, list(range(50, 60)))
        text, ended = before_eos(ids, 1024)
        s = g.alive(text_of(text, 1024))
        assert s is not GO.DEAD and len(text) > 0
        assert not ended or re.fullmatch(WORDS, text_of(text, 1024))
        # the control: without the grammar the slot produces ids the automaton does not allow (tokens that leave the language, or
        # empty ones, which no state allows)
        free = _generate(tiny, dev_tiny, None, smp, 24, list(range(50, 60)))
        assert not follows(g, free) and follows(g, ids)


# -- 4. step splitting and prefill paths --------------------------------------------------------------------------------------------
def test_step_splitting(tiny, dev_tiny):
    def run(calls):
        sim = Sim(tiny, 3, dev_tiny)
        try:
            for i in range(3):
                sim.start(i, _mixed(i + 2, sim.V), list(range(20 + i, 30 + 2 * i)))
            for c in calls:
                sim.eng.decode(c, batch=3)
            return [sim.eng.read_tokens(i, 13) for i in range(3)], [sim.eng.grammar_state(i) for i in range(3)]
        finally:
            sim.close()

    assert run([6, 6]) == run([1] * 12)


def test_prefill_paths(tiny, dev_tiny):
    sim = Sim(tiny, 4, dev_tiny)
    try:
        prompt = [int(t) for t in np.random.default_rng(9).integers(0, 1000, 33)]
        cfg = _cfg(pen=(1.4, 0.3, 0.2), bias={5: 1.5, ord("{"): -1.0}, grammar=RECORD)
        sim.start(0, cfg, prompt, chunk=8)  # chunked: the first token is masked with the start state
        assert sim.out[0][0] == ord("{")
        # packed, two slots, one with a grammar, the other in two passes
        sim.eng.begin(1), sim.eng.begin(2)
        sim.configure(1, _cfg(grammar=JSONISH, smp=(0.8, 50, 1.0, 5)))
        sim.configure(2, _cfg(bias={7: 2.0}))
        sim.eng.prefill_packed([(1, prompt[:20], True), (2, prompt[:10], False)])
        sim.consumed(1, prompt[:20]), sim.consumed(2, prompt[:10])
        sim.first_token(1)
        assert sim.out[1][0] == ord("{")
        sim.eng.prefill_packed([(2, prompt[10:], True)])
        sim.consumed(2, prompt[10:])
        sim.first_token(2)
        sim.start(3, _cfg(grammar=NUMBER), prompt[:9])
        for _ in range(14):
            sim.step(4)
        # the NUMBER slot has ended by now (at most 11 bytes): only EOS ids since
        ids, ended = before_eos(sim.out[3], 1024)
        assert ended and all(t in eos_ids(1024) for t in sim.out[3][len(ids):]) and re.fullmatch(NUMBER, text_of(ids, 1024))
        assert sim.eng.grammar_state(3) == (GO.END, True)
        sim.assert_few_ambiguous()
    finally:
        sim.close()


# -- 5. life cycle ------------------------------------------------------------------------------------------------------------------
def test_life_cycle(tiny, dev_tiny, dev_big):
    sim = Sim(tiny, 4, dev_tiny)
    eng = sim.eng
    try:
        cfg = _cfg(pen=(1.5, 1.0, 0.5), bias={11: 2.0}, grammar=WORDS, smp=(0.9, 30, 1.0, 5))
        sim.start(2, cfg, list(range(30, 40)))
        for _ in range(3):
            sim.step(3)
        # move mid-generation: grammar and state go with the sequence
        eng.move(2, 0)
        for d in (sim.cfg, sim.hist, sim.state, sim.pending, sim.out):
            d[0] = d.pop(2)
        for _ in range(2):
            sim.step(1)
        # fork: the child starts from the parent's state, then both go their own way under different seeds
        eng.fork(0, 1)
        sim.cfg[1], sim.hist[1], sim.state[1] = dict(sim.cfg[0], smp=(0.9, 30, 1.0, 77)), sim.hist[0].copy(), sim.state[0]
        sim.pending[1], sim.out[1] = sim.pending[0], list(sim.out[0])
        eng.set_sampling(1, 0.9, 30, None, 77)
        assert eng.grammar_state(1) == eng.grammar_state(0)
        for _ in range(8):
            sim.step(2)
        assert sim.out[0] != sim.out[1]
        g = sim.grammar(0)
        for i in (0, 1):
            ids, ended = before_eos(sim.out[i], 1024)
            assert g.alive(text_of(ids, 1024)) is not GO.DEAD
        # verify / rewind / set_token refuse a grammar slot ...
        eng.begin(3)
        eng.set_grammar(3, dev_tiny.grammar(NUMBER))
        eng.prefill(3, [1, 2, 3])
        for call in (lambda: eng.verify(3, [1, 2]), lambda: eng.rewind(3, 1), lambda: eng.set_token(3, 5)):
            with pytest.raises(RuntimeError):
                call()
        # ... a vocabulary of another size is refused, the slot keeps its grammar ...
        with pytest.raises(RuntimeError):
            eng.set_grammar(3, dev_big.grammar(NUMBER))
        with pytest.raises(RuntimeError):
            eng.grammar_state(2)  # (no live sequence there)
        assert eng.grammar_state(3)[0] != GO.END
        # ... and they work again once the grammar is cleared
        eng.set_grammar(3, None)
        with pytest.raises(RuntimeError):
            eng.grammar_state(3)
        eng.rewind(3, 1)
        eng.set_token(3, 5)
        assert len(eng.verify(3, [1, 2])) == 2
        eng.release(3)
        # set_grammar(None) on a slot with penalties leaves the penalties working
        eng.set_grammar(0, None)
        sim.cfg[0] = dict(sim.cfg[0], grammar=None)
        for _ in range(3):
            sim.step(2)
        # release + begin clear the grammar: the slot is free again, and a fresh grammar starts at its start state
        eng.release(1)
        del sim.cfg[1]
        sim.start(1, _cfg(), list(range(30, 40)))
        with pytest.raises(RuntimeError):
            eng.grammar_state(1)
        eng.release(1)
        del sim.cfg[1]
        sim.start(1, _cfg(grammar=JSONISH), list(range(30, 40)))
        assert sim.out[1][0] == ord("{")
        sim.step(2)
        sim.assert_few_ambiguous()
    finally:
        sim.close()


def test_grammar_set_on_a_slot_with_a_pending_token(tiny, dev_tiny):
    """the pending token is fed by the next step and advances the new grammar's state then; grammar_state includes it at once"""
    eng = _engine(tiny, 1)
    try:
        g = oracle_of(WORDS, 1024)
        eng.begin(0)
        eng.set_logit_bias(0, {ord("q"): 100.0})
        eng.prefill(0, list(range(10, 20)))
        assert eng.read_tokens(0, 1) == [ord("q")]
        eng.set_grammar(0, dev_tiny.grammar(WORDS))
        want = g.advance(g.start, ord("q"))
        assert eng.grammar_state(0) == (want, True)
        eng.decode(1, batch=1)
        assert eng.grammar_state(0) == (g.advance(want, ord("q")), True)
    finally:
        eng.close()


def test_grammar_create_refuses_bad_input(dev_tiny):
    """the table, start and EOS validation needs a vocabulary, which lives on the device"""
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    d = dfa_of(NUMBER)
    S_ = d.n_states

    def create(n_states=S_, table=None, start=0, eos=(1023, 1022), n_eos=None, vocab=dev_tiny.vocab._h):
        table = np.ascontiguousarray(d.table if table is None else table, dtype=np.uint16)
        acc = np.ascontiguousarray(d.accepting, dtype=np.uint8)
        arr = (ctypes.c_int32 * 9)(*eos)
        out = ctypes.c_void_p()
        rc = lib.tl_grammar_create(vocab, n_states, table.ctypes.data, acc.ctypes.data, start, arr, len(eos) if n_eos is None else n_eos,
                                   None, ctypes.byref(out))
        if rc == 0:
            lib.tl_grammar_destroy(out)
        else:
            assert not out.value
        return rc

    assert create() == 0
    INVALID = create(start=S_)
    assert INVALID != 0 and create(start=-1) == INVALID
    bad = d.table.copy()
    bad[S_ - 1, 200] = S_  # a transition outside the table that is not 0xFFFF
    assert create(table=bad) == INVALID
    assert create(eos=(1023, 1023)) == INVALID and create(eos=(1024,)) == INVALID and create(eos=(-1,)) == INVALID
    assert create(eos=(), n_eos=0) == INVALID and create(eos=tuple(range(9)), n_eos=9) == INVALID
    assert create(n_states=0) == INVALID and create(n_states=32769) == INVALID
    assert create(vocab=None) == INVALID


# -- 6. unchanged programs ----------------------------------------------------------------------------------------------------------
def test_programs_without_a_grammar_are_unchanged(tiny, dev_tiny):
    prompt, steps = list(range(100, 112)), 10

    def run(setup, bias=None):
        eng = _engine(tiny, 2)
        try:
            setup(eng)
            eng.begin(0)
            if bias:
                eng.set_logit_bias(0, bias)
            eng.prefill(0, prompt)
            eng.decode(steps, batch=1)
            return eng.read_tokens(0, steps + 1), eng.logits(1).float().cpu(), eng.stats()["graph_captures"], eng.stats()["workspace_bytes"]
        finally:
            eng.close()

    fresh = run(lambda eng: None)  # before any engine of this test holds a grammar
    other = _engine(tiny, 1)  # an engine of its own that holds a grammar from here on
    try:
        other.begin(0)
        other.set_grammar(0, dev_tiny.grammar(RECORD))
        other.prefill(0, prompt)
        other.decode(2, batch=1)
        beside = run(lambda eng: None)
        assert beside[0] == fresh[0] and torch.equal(beside[1], fresh[1]) and beside[2:] == fresh[2:], "nothing is allocated or captured anew"

        def released(eng):  # the engine's only grammar slot was released (and another one cleared) before the run
            eng.begin(1)
            eng.set_grammar(1, dev_tiny.grammar(NUMBER))
            eng.prefill(1, prompt[:5])
            eng.release(1)
            eng.begin(1)
            eng.set_grammar(1, dev_tiny.grammar(NUMBER))
            eng.set_grammar(1, None)
            eng.release(1)

        after = run(released)
        assert after[0] == fresh[0] and torch.equal(after[1], fresh[1]) and after[2] == fresh[2]
        # ... and a processing plan without a grammar is the processing plan it was
        bias = {t: -math.inf for t in set(fresh[0])}
        banned, banned_after = run(lambda eng: None, bias), run(released, bias)
        assert banned[0] == banned_after[0] and torch.equal(banned[1], banned_after[1]) and banned[2] == banned_after[2]
        assert not set(banned[0]) & set(fresh[0])
    finally:
        other.close()


# -- 7. written once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_written_once_grammar_plans(tiny, dev_tiny, n):
    def check(with_grammar):
        sim = Sim(tiny, n, dev_tiny)
        try:
            for i in range(n):
                cfg = _mixed(i + 1, sim.V)  # slot 0 holds a grammar at every n
                if not with_grammar and cfg["grammar"] is not None:  # the corresponding processing plan: a bias entry instead
                    cfg = dict(cfg, grammar=None, bias={**cfg["bias"], 7: 1.0})
                sim.start(i, cfg, list(range(3 + i % 7, 12 + i % 7)))
            sim.step(n)
            c = sim.eng.check_step(n)
            assert np.isfinite(sim.eng.logits(n).float().cpu().numpy()).all()
            return c
        finally:
            sim.close()

    grammar, processing = check(True), check(False)
    assert grammar["double_writes"] == 0, grammar
    assert processing["double_writes"] == 0, processing
    assert grammar["written_once_plan"] == processing["written_once_plan"], (grammar, processing)
    assert grammar["launches"] == processing["launches"], "the grammar twin replaces the processing launch, it adds none"


# -- 8. the Qwen3-4B vocabulary width -----------------------------------------------------------------------------------------------
def test_engine_qwen4b_shapes(q4b, dev_big):
    sim = Sim(q4b, 4, dev_big)
    try:
        rng = np.random.default_rng(44)
        for i in range(4):
            sim.start(i, _mixed(i + 1, sim.V, small=False), rng.integers(0, 1000, 6 + i).tolist())  # kinds 1, 2, 3, 4
        for _ in range(6):
            sim.step(4)
        sim.assert_few_ambiguous()
    finally:
        sim.close()


# -- 9. FP8 pages -------------------------------------------------------------------------------------------------------------------
def test_fp8_pages(tiny, dev_tiny):
    for smp in ((0.0, 0, 0.0, 0), (0.9, 40, 0.0, 7)):
        ids = _generate(tiny, dev_tiny, JSONISH, smp, 32, list(range(100, 112)), kv_format="fp8")
        text, ended = before_eos(ids, 1024)
        assert ended and re.fullmatch(JSONISH, text_of(text, 1024)), text_of(text, 1024)


# -- 10. continuous batching --------------------------------------------------------------------------------------------------------
def test_batch_generate_grammar(tiny, dev_tiny):
    from tiny_llm_hip.engine import batch_generate_ids

    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, 1000, int(rng.integers(4, 30))).tolist() for _ in range(7)]
    patterns = [NUMBER, JSONISH, None, NUMBER, JSONISH, NUMBER, None]
    sampling = [dict({"grammar": dev_tiny.grammar(p)} if p else {}, **({"temperature": 0.9, "top_k": 40} if i % 2 else {}),
                     **({"repetition_penalty": 1.3} if i == 3 else {})) for i, p in enumerate(patterns)]

    def run():
        eng = _engine(tiny, 5)
        try:
            return sorted(batch_generate_ids(eng, prompts, 34, batch_size=4, prefill_step=16, sampling=sampling))
        finally:
            eng.close()

    a = run()
    assert a == run()
    for idx, ids in a:
        if patterns[idx] is None:
            assert len(ids) == 34
            continue
        text, ended = before_eos(ids, 1024)
        assert ended and len(ids) == len(text) + 1, "a request with a grammar ends with its first EOS id"
        assert re.fullmatch(patterns[idx], text_of(text, 1024)), (idx, text_of(text, 1024))
