"""GPU tier: stack grammars -- JSON mode -- on the device (tl_grammar_create_stack, tl_engine_grammar_config,
tl_grammar_mask_rows_stack; csrc/grammar_stack.h) against the plain-Python restatement of their definition
(tests/stack_grammar_oracle.py).  Every decode step's processed rows are compared with the oracle's bit for bit, for the stack slots and
for the regex-grammar, penalty-only and plain slots that share the step with them; the choice on the processed row is checked by
tests/sampling_oracle.py under the rule of tests/test_zz_logit_processing_gpu.py (a produced id equals the oracle's unless the draw is
flagged ambiguous; at most 10 % of the checked draws may be).

The engine harness is the one of tests/test_zz_grammar_gpu.py (its Sim keeps every slot's settings, history, automaton state and pending
token on the host by the header's rule); here a slot's "state" is a configuration (state, depth, stack) where its grammar has a stack."""

import ctypes
import functools
import json
import math

import numpy as np
import pytest
import torch

import grammar_oracle as GO
import logit_processing_oracle as P
import sampling_oracle as S
import stack_grammar_oracle as SO
import test_zz_grammar_gpu as RG
from helpers import QWEN4B_CFG, TINY_CFG

pytestmark = pytest.mark.gpu

NEUTRAL = RG.NEUTRAL
RECORD = RG.RECORD
ALPHABET = b'0123456789abcdefghijklmnopqrstuvwxyz{}[]()<>":,.- '
# tokens made to cross stack edges, at ids EDGE_AT ..: pops below the start of the token followed by a push; 16- and 17-byte tokens
# (17 bytes is LONG: never walked in a step) with and without a closing bracket, for either automaton; pushes that meet the depth limit
EDGE = [b"],[", b"}}", b'{"a":[', b"]]]]", b"[[", b"[" * 16, b"[" * 17,
        b'"abcdefghijklmn"', b'"abcdefghijklm"]', b'"abcdefghijklmno"', b'"abcdefghijklmn"]',
        b"abcdefghijklmnop", b"abcdefghijklmno]", b"abcdefghijklmnopq", b"abcdefghijklmnop]",
        b"(abcdefghijklmnop)", b"[1,2,3,4,5,6,7,8,9]", b"]]", b")(", b">}])", b"(((((((([[[[[[[[", b"]["]
EDGE_AT = 300
assert [len(t) for t in EDGE[7:15]] == [16, 16, 17, 17, 16, 16, 17, 17]


def tok(text):
    """the id of an EDGE token or of a single byte, in every vocabulary"""
    return EDGE_AT + EDGE.index(text) if text in EDGE else bytes(range(256)).index(text)


# -- vocabularies and automata ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def vocabulary(V):
    """tests/test_zz_grammar_gpu.py's vocabulary(V) with brackets of four kinds in the alphabet, and the EDGE tokens."""
    rng = np.random.default_rng(V)
    pieces = [bytes([c]) for c in ALPHABET] + [u.encode() for u in RG.UTF8]

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
        for j in rng.choice(np.arange(400, V - 4), 200, replace=False):
            n = int(rng.integers(64, 201))
            tokens[int(j)] = b"".join(letters[int(k)] for k in rng.integers(0, len(letters), n)) if rng.random() < 0.7 else b" " * n
        for j in rng.choice(np.arange(400, V - 4), 12, replace=False):
            tokens[int(j)] = b""
        tokens[V - 4:] = [b""] * 4
        tokens[340:346] = [b"a" * 16, b"a" * 17, b"abcdefghijklmnop\"", b"abcdefghijklmno\"", b" " * 18, b"x" * 15 + b"\xc3\xa9"]
    tokens[EDGE_AT:EDGE_AT + len(EDGE)] = EDGE
    assert len(tokens) == V
    return tokens


def eos_ids(V):
    return [V - 1, V - 2]


POP_ROWS = [5, 40, 66, 69]  # "brackets-pops": the pop entry of each closer, two of them past the 64 entries the kernels keep in LDS


def bracket_automaton(many_pops=False):
    """Four stack symbols, five states (< 16: in LDS whole): the state is what is on top of the stack (4: nothing); letters, digits
    and spaces stay, an opener pushes its kind, the closer of the kind on top pops; the text may end where nothing is open.
    many_pops: the same language over a pop table of 70 entries (more than 64: read through L2, not from LDS) -- every closer has an
    entry of its own, POP_ROWS, and every other entry leads to a wrong state, so that a lookup of the wrong entry shows."""
    from tiny_llm_hip import grammar as G

    opens, closes = b"([{<", b")]}>"
    table = np.full((5, 256), 0xFFFF, dtype=np.uint16)
    ops = np.zeros((5, 256), dtype=np.uint8)
    for s in range(5):
        for b in b"abcdefghijklmnopqrstuvwxyz0123456789 ":
            table[s, b] = s
        for a in range(4):
            table[s, opens[a]], ops[s, opens[a]] = a, 1 + a
        if s < 4:
            table[s, closes[s]], ops[s, closes[s]] = (POP_ROWS[s] if many_pops else 0), 5
    pops = [[0, 1, 2, 3, 4] if r in POP_ROWS else [(r + 1) % 4, (r + 2) % 4, 4, 0xFFFF, r % 4] for r in range(70)] if many_pops else [[0, 1, 2, 3, 4]]
    return G.StackDFA(table, ops, pops, [0, 0, 0, 0, 1], 4)


@functools.lru_cache(maxsize=None)
def automaton(key):
    """"brackets", "brackets-pops" (the same over a large pop table), "json" (any value, free whitespace), "json-object" (compact), or a
    regex pattern (bytes)"""
    from tiny_llm_hip import grammar as G

    if key in ("brackets", "brackets-pops"):
        return bracket_automaton(many_pops=key == "brackets-pops")
    if key == "json":
        return G.compile_json("value", "free")
    if key == "json-object":
        return G.compile_json("object", "compact")
    return G.compile_regex(key)


@functools.lru_cache(maxsize=None)
def oracle_of(key, V):
    d = automaton(key)
    if isinstance(key, bytes):
        return GO.Grammar(d.table, d.accepting, d.start, vocabulary(V), eos_ids(V))
    return SO.StackGrammar(d.table, d.ops, d.pop_table, d.accepting, d.start, vocabulary(V), eos_ids(V))


def has_stack(g):
    return isinstance(g, SO.StackGrammar)


class Device:
    """The device side of a vocabulary and the grammars made over it, kept alive while engines use them."""

    def __init__(self, V):
        from tiny_llm_hip.engine import Vocab
        from tiny_llm_hip.grammar import vocabulary_bytes_from_strings

        self.V = V
        self.vocab = Vocab(*vocabulary_bytes_from_strings(vocabulary(V)))
        self.grammars = {}

    def grammar(self, key):
        from tiny_llm_hip.engine import Grammar

        if key not in self.grammars:
            self.grammars[key] = Grammar(self.vocab, automaton(key), eos_ids(self.V))
        return self.grammars[key]

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
    for k, t in enumerate(ids):
        if t in eos_ids(V):
            return list(ids[:k]), True
    return list(ids), False


def bits_of(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


# -- 1. the kernel over caller rows, bit for bit ------------------------------------------------------------------------------------
def _configurations(g, key, V):
    """(configuration, {token text: allowed?} that the row must show) -- END, depth 0, depth 32, depth 31 with a token that pushes twice,
    states reached mid-string, and both sides of the long-token rule"""
    if key in ("brackets", "brackets-pops"):
        rng = np.random.default_rng(7)
        full = [int(a) for a in rng.integers(0, 4, 32)]
        full[31], full[30] = 1, 1  # '[' on top, '[' under it

        def cfg(symbols):
            return (symbols[-1] if symbols else 4, len(symbols), sum(a << (2 * i) for i, a in enumerate(symbols)))

        return [
            (g.start, {b"[[": True, b"]": False, b"abcdefghijklmnopq": True, b"abcdefghijklmnop]": False, b"(abcdefghijklmnop)": True, b"[" * 17: True,
                       b"abcdefghijklmno]": False, b")(": False}),
            (SO.END, {}),
            (cfg(full), {b"[": False, b"]": True, b"]]": True, b"][": True, b"[[": False, b"abcdefghijklmnopq": True, b"(abcdefghijklmnop)": False,
                         b"abcdefghijklmnop]": False, b"abcdefghijklmno]": True}),
            (cfg(full[:31]), {b"[": True, b"[[": False, b"][": True, b"],[": False, b"(abcdefghijklmnop)": True}),
            (cfg([0, 1, 2, 3]), {b">}])": True, b")(": False, b"]]]]": False, b"(((((((([[[[[[[[": True, b"[" * 17: True}),
            (cfg(full[:15]), {b"[" * 17: True, b"[" * 16: True, b"(((((((([[[[[[[[": True}),
            (cfg(full[:16]), {b"[" * 17: False, b"[" * 16: True, b"(((((((([[[[[[[[": True}),
            (cfg(full[:17]), {b"[" * 17: False, b"[" * 16: False, b"(((((((([[[[[[[[": False}),
            (cfg([1, 1, 1, 1]), {b"]]]]": True, b"]]": True, b">}])": False}),
        ]
    at = lambda text: g.alive(text)
    return [
        (g.start, {b'{"a":[': True, b"[" * 17: True, b'"abcdefghijklmno"': True, b'"abcdefghijklmn"]': False, b"[1,2,3,4,5,6,7,8,9]": True, b"]": False,
                   b'"abcdefghijklmn"': True, b'"abcdefghijklm"]': False}),
        (SO.END, {}),
        (at(b"[" * 32), {b"[": False, b"]": True, b"]]]]": True, b'"abcdefghijklmno"': True, b"[1,2,3,4,5,6,7,8,9]": False, b'"abcdefghijklm"]': True,
                         b'"abcdefghijklmn"]': False, b"1": True, b"{": False}),
        (at(b"[" * 31), {b"[": True, b"[[": False, b'{"a":[': False, b"{": True, b"[1,2,3,4,5,6,7,8,9]": True}),
        (at(b'{"a":["x'), {b"abcdefghijklmnopq": True, b"]": True, b'"abcdefghijklmn"]': False, b"[" * 17: True}),
        (at(b'[{"k":"\\'), {b"n": True, b"u": True, b"x": False, b'"abcdefghijklmn"': True}),
        (at(b"[[1"), {b"],[": True, b"]]": True, b"]]]]": False, b"}}": False, b",": True}),
        (at(b'{"a":{"b":1'), {b"}}": True, b"]]": False, b"],[": False}),
        (at(b"[[[[[1"), {b"]]]]": True, b"],[": True}),
        (at(b"[" * 15), {b"[" * 17: True, b"[" * 16: True}),
        (at(b"[" * 16), {b"[" * 17: False, b"[" * 16: True}),
        (at(b'[{"a":-1.5e'), {b"+": True, b"1": True, b"]": False, b",": False}),
    ]


@pytest.mark.parametrize("V", [1024, 151936, 151941])
@pytest.mark.parametrize("key", ["brackets", "json"])
def test_mask_rows_stack_bit_for_bit(V, key):
    _check_mask_rows_stack(V, key)


def test_mask_rows_stack_pop_table_past_lds():
    """more than 64 pop entries: the one path on which the pop lookups of a walk go through L2 (GRS_LDS_POPS)"""
    assert automaton("brackets-pops").n_pop > 64 and max(POP_ROWS) >= 64
    _check_mask_rows_stack(1024, "brackets-pops")


def _check_mask_rows_stack(V, key):
    import tiny_llm_ext_hip as ext

    g = oracle_of(key, V)
    assert (len(g.accepting) < 16) if key.startswith("brackets") else (len(g.accepting) > 100)
    dev = Device(V)
    try:
        rng = np.random.default_rng(V)
        rows_of = _configurations(g, key, V)
        rows = []
        for i in range(len(rows_of)):
            l = rng.standard_normal(V).astype(np.float32) * 2.0
            at = rng.choice(V, 600, replace=False)
            l[at[:150]], l[at[150:300]], l[at[300:450]], l[at[450:]] = np.nan, np.inf, -np.inf, -0.0
            if i == 0:  # specials on allowed and on disallowed tokens alike: the single bytes and the EOS ids
                l[0:256:4], l[1:256:4], l[2:256:4] = np.nan, -0.0, np.inf
                l[V - 2] = np.nan
            rows.append(P.bf16_round(l))
        logits = torch.from_numpy(np.stack(rows)).bfloat16().cuda()
        raw = bits_of(logits)
        out = torch.empty_like(logits)
        cfgs = [c for c, _ in rows_of]
        assert all(c is not SO.DEAD for c in cfgs)
        st = torch.tensor([c[0] for c in cfgs], dtype=torch.int32, device="cuda")
        dp = torch.tensor([c[1] for c in cfgs], dtype=torch.int32, device="cuda")
        sk = torch.from_numpy(np.array([c[2] for c in cfgs], dtype=np.uint64).view(np.int64)).cuda()
        ext.check(ext.lib().tl_grammar_mask_rows_stack(dev.grammar(key)._h, logits.data_ptr(), len(cfgs), st.data_ptr(), dp.data_ptr(), sk.data_ptr(),
                                                       out.data_ptr(), None))
        torch.cuda.synchronize()
        got = bits_of(out)
        for i, (c, expect) in enumerate(rows_of):
            ok = g.allowed(c)
            for text, allowed in expect.items():  # the rows cover what they are meant to cover (by the oracle, before the device is asked)
                assert bool(ok[tok(text)]) == allowed, (key, c, text, allowed)
            want = P.bits(SO.mask_row(P.from_bits(raw[i]), g, c))
            assert np.array_equal(want, np.where(ok, raw[i], np.uint16(0xFF80)))
            bad = np.flatnonzero(got[i] != want)
            assert bad.size == 0, (f"{key}, V {V}, row {i}, configuration {c}: {bad.size} elements differ, first at {bad[:4]} (tokens "
                                   f"{[vocabulary(V)[j] for j in bad[:4]]}): got {got[i][bad[:4]]}, want {want[bad[:4]]}")
            if c == SO.END:
                assert sorted(np.flatnonzero(ok)) == sorted(eos_ids(V))
            else:
                assert ok[eos_ids(V)].all() == bool(g.accepting[c[0]]) and not ok[V - 3]
        assert 0 < g.allowed(cfgs[0]).sum() < V
        if V > 1024:  # long tokens on both sides of the rule, beyond the hand-made ones
            long_ids = [j for j, t in enumerate(vocabulary(V)) if len(t) > 16]
            alive = [sum(bool(g.allowed(c)[j]) for j in long_ids) for c in cfgs if c != SO.END]
            assert len(long_ids) >= 200 and max(alive) >= 50 and min(alive) < len(long_ids) - 50, alive
    finally:
        dev.close()


def test_create_refuses_bad_input(dev_tiny):
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    d = automaton("json")
    S_ = d.n_states

    def create(n_states=S_, table=None, ops=None, pops=None, n_pop=None, start=None, eos=(1023, 1022)):
        table = np.ascontiguousarray(d.table if table is None else table, dtype=np.uint16)
        ops = np.ascontiguousarray(d.ops if ops is None else ops, dtype=np.uint8)
        pops = np.ascontiguousarray(d.pop_table if pops is None else pops, dtype=np.uint16)
        acc = np.ascontiguousarray(d.accepting, dtype=np.uint8)
        arr = (ctypes.c_int32 * 9)(*eos)
        out = ctypes.c_void_p()
        rc = lib.tl_grammar_create_stack(dev_tiny.vocab._h, n_states, table.ctypes.data, ops.ctypes.data, pops.shape[0] if n_pop is None else n_pop,
                                         pops.ctypes.data, acc.ctypes.data, d.start if start is None else start, arr, len(eos), None, ctypes.byref(out))
        if rc == 0:
            lib.tl_grammar_destroy(out)
        else:
            assert not out.value
        return rc

    assert create() == 0
    INVALID = create(start=S_)
    assert INVALID != 0 and create(start=-1) == INVALID
    free = np.argwhere(d.table == 0xFFFF)[0]
    push = np.argwhere(d.ops == 1)[0]
    pop = np.argwhere(d.ops == 5)[0]
    bad = d.ops.copy()
    bad[pop[0], pop[1]] = 6  # an op byte that is none of 0 .. 5
    assert create(ops=bad) == INVALID
    bad[pop[0], pop[1]] = 255
    assert create(ops=bad) == INVALID
    bad = d.table.copy()
    bad[pop[0], pop[1]] = 1  # a pop entry >= n_pop (a valid state number)
    assert create(table=bad) == INVALID
    bad = d.table.copy()
    bad[push[0], push[1]] = S_  # a push entry outside the table
    assert create(table=bad) == INVALID
    bad = d.pop_table.copy()
    bad[0, 2] = S_  # a pop_table entry >= n_states that is not 0xFFFF
    assert create(pops=bad) == INVALID
    assert create(n_pop=-1) == INVALID and create(n_pop=65536) == INVALID
    assert create(n_states=0) == INVALID and create(eos=(1023, 1023)) == INVALID
    ok = d.ops.copy()
    ok[free[0], free[1]] = 9  # (the op of an entry without a transition is validated too)
    assert create(ops=ok) == INVALID
    # tl_grammar_mask_rows refuses a stack grammar, tl_grammar_mask_rows_stack a regex grammar
    rows = torch.zeros((1, 1024), dtype=torch.bfloat16, device="cuda")
    out = torch.empty_like(rows)
    zero = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.tl_grammar_mask_rows(dev_tiny.grammar("json")._h, rows.data_ptr(), 1, zero.data_ptr(), out.data_ptr(), None) == INVALID
    assert lib.tl_grammar_mask_rows_stack(dev_tiny.grammar(RECORD)._h, rows.data_ptr(), 1, zero.data_ptr(), zero.data_ptr(), zero.data_ptr(),
                                          out.data_ptr(), None) == INVALID
    torch.cuda.synchronize()


# -- the engine beside the oracle ---------------------------------------------------------------------------------------------------
_cfg = RG._cfg


def _mixed(i, V):
    """Slot i's settings by i % 6: nothing; penalties and bias only; a regex grammar, sampled; the bracket automaton, greedy; JSON with
    penalties and bias, sampled; JSON with a bias that favours brackets, greedy."""
    rng = np.random.default_rng(2000 + i)
    bias = {int(t): float(np.float32(v)) for t, v in zip(rng.choice(V, 16, replace=False), rng.standard_normal(16) * 2.0)}
    bias[int(rng.integers(0, V))] = -math.inf
    bias[ord("[")] = 4.0  # ... and entries on tokens the grammar decides about
    bias[ord("z")] = 100.0
    smp = [(0.8, 50, 1.0), (0.8, 20, 0.8), (0.8, 0, 1.0)][(i // 6) % 3]
    kind = i % 6
    if kind == 0:
        return _cfg()
    if kind == 1:
        return _cfg(pen=(1.2, 0.4, 0.1), bias=bias)
    if kind == 2:
        return _cfg(grammar=RECORD, smp=(*smp, 100 + i))
    if kind == 3:
        return _cfg(grammar="brackets", bias={ord("("): 8.0, ord("<"): 8.5, ord(">"): 9.0, tok(b")("): 12.0, tok(b"(abcdefghijklmnop)"): 8.75})
    if kind == 4:
        return _cfg(pen=(1.2, 0.4, 0.1), bias=bias, smp=(*smp, 100 + i), grammar="json")
    return _cfg(grammar="json", bias={ord("["): 6.0, ord("{"): 5.0, tok(b"],["): 8.0, tok(b"]]"): 5.0, tok(b'{"a":['): 7.0})


class Sim(RG.Sim):
    """tests/test_zz_grammar_gpu.py's Sim over this file's vocabulary and automata; self.state[slot] is a configuration for a stack
    grammar.  A checked step also compares the processed row of every live slot with the oracle's."""

    deepest = 0  # the deepest stack a checked step started from

    def grammar(self, slot):
        key = self.cfg[slot]["grammar"]
        return oracle_of(key, self.V) if key is not None else None

    def oracle_row(self, slot, raw_row):
        c, g = self.cfg[slot], self.grammar(slot)
        if not self.processes(slot):
            return raw_row
        h = self.hist[slot]
        if has_stack(g):
            return SO.process(raw_row, h.prompt, h.count, *c["pen"], c["bias"], grammar=g, cfg=self.state[slot])
        return GO.process(raw_row, h.prompt, h.count, *c["pen"], c["bias"], grammar=g, state=self.state.get(slot))

    def check(self, slot, got, raw_row, position, processed=None):
        c, g = self.cfg[slot], self.grammar(slot)
        row = self.oracle_row(slot, raw_row)
        if processed is not None:
            bad = np.flatnonzero(P.bits(row) != processed)
            assert bad.size == 0, (f"slot {slot} ({c['grammar']}, {self.state.get(slot)}): {bad.size} elements of the processed row differ, first "
                                   f"at {bad[:4]}: got {processed[bad[:4]]}, want {P.bits(row)[bad[:4]]}")
        want, amb = S.sample(row, *c["smp"][:3], c["smp"][3], position)
        self.draws += 1
        self.ambiguous += bool(amb)
        if has_stack(g) and self.state[slot] != SO.END:
            self.deepest = max(self.deepest, self.state[slot][1])
        assert got == want or amb, (slot, got, want, c["smp"], self.state.get(slot))
        if c["smp"][0] == 0 and np.isfinite(np.nanmax(row)):
            assert got == int(np.flatnonzero(row == np.nanmax(row))[0]), "a greedy slot's id is the first maximum of the processed row"
        if g is None:
            return
        assert g.allowed(self.state[slot])[got], f"slot {slot} produced token {got} that {self.state[slot]} does not allow"
        after = g.advance(self.state[slot], got)
        if has_stack(g):
            accepting = after == SO.END or g.accepting[after[0]]
            assert self.eng.grammar_config(slot) == (*after, accepting), (slot, self.eng.grammar_config(slot), after)
            assert self.eng.grammar_state(slot) == (after[0], accepting)
        else:
            accepting = after == GO.END or g.accepting[after]
            assert self.eng.grammar_state(slot) == (after, accepting)
            assert self.eng.grammar_config(slot) == (after, 0, 0, accepting)

    def step(self, n, use_graph=True, check=True):
        live = [i for i in range(n) if i in self.cfg and self.eng.context_len(i) >= 0]
        ctx = {i: self.eng.context_len(i) for i in live}
        self.feed(live)
        self.eng.decode(1, batch=n, use_graph=use_graph)
        got = self.eng.read_pending(n)
        if check:
            raw = P.from_bits(bits_of(self.eng.logits(n)))
            processed = bits_of(self.eng.processed_logits(n)) if any(self.processes(i) for i in live) else None
        for i in live:
            if check:
                self.check(i, got[i], raw[i], ctx[i] + 1, None if processed is None else processed[i])
            self.pending[i] = got[i]
            self.out[i].append(got[i])


def _mixed_run(model, n, steps, dev, route=None, use_graph=True, check=True, first=0, **kw):
    sim = Sim(model, n, dev, route, **kw)
    try:
        rng = np.random.default_rng(n)
        for i in range(n):
            sim.start(i, _mixed(i + first, sim.V), rng.integers(0, 1000, 5 + i % 11).tolist())
        for _ in range(steps):
            sim.step(n, use_graph=use_graph, check=check)
        return sim
    except Exception:
        sim.close()
        raise


def viable(sim, i):
    """what a constrained slot wrote is, so far, text its automaton can still accept -- and accepts, where an EOS id ended it"""
    g = sim.grammar(i)
    ids, ended = before_eos(sim.out[i], sim.V)
    s = g.alive(text_of(ids, sim.V))
    assert s is not None, (i, text_of(ids, sim.V))
    assert not ended or g.accepting[s[0] if has_stack(g) else s], (i, text_of(ids, sim.V))


# -- 2. every step against the oracle, both replay routes ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 17, 64])
def test_engine_every_step_matches_oracle(tiny, dev_tiny, n):
    first = 4 if n == 1 else 0  # one slot: JSON with penalties and bias, sampled
    a = _mixed_run(tiny, n, 8, dev_tiny, first=first)
    b = c = None
    try:
        assert a.eng.replay_route() == "aql"
        a.assert_few_ambiguous()
        sa = a.eng.stats()
        assert sa["graph_replays"] == 7 and sa["aql_steps"] == sa["graph_replays"], sa  # the stack plan replays as AQL packets
        b = _mixed_run(tiny, n, 8, dev_tiny, first=first, route="hipgraph", check=False)
        c = _mixed_run(tiny, n, 8, dev_tiny, first=first, use_graph=False, check=False)
        assert b.eng.replay_route().startswith("hipgraph") and b.eng.stats()["aql_steps"] == 0
        assert a.out == b.out == c.out
        for i in range(n):
            if a.cfg[i]["grammar"] is not None:
                viable(a, i)
                assert b.eng.grammar_config(i) == a.eng.grammar_config(i) == c.eng.grammar_config(i)
        assert n < 4 or a.deepest >= (4 if n >= 6 else 1), "the stack slots did push: the run is about stacks"
    finally:
        for s in (a, b, c):
            if s is not None:
                s.close()


# -- 3. scripted documents ----------------------------------------------------------------------------------------------------------
def _scripted(model, dev, key, script, then_eos=False):
    """Before every step a logit bias of +30,000 on the step's scripted token; returns (engine, ids produced), stopping at the first id
    that is not the scripted one."""
    V = 1024
    ids = [tok(t) for t in script] + ([eos_ids(V)[0]] if then_eos else [])
    eng = RG._engine(model, 1)
    out = []
    try:
        eng.begin(0)
        eng.set_grammar(0, dev.grammar(key))
        for k, t in enumerate(ids):
            eng.set_logit_bias(0, {t: 30000.0})
            if k == 0:
                eng.prefill(0, [5, 6, 7])
                out.append(eng.read_tokens(0, 1)[0])
            else:
                if then_eos and k == len(ids) - 1:  # after the last scripted token, before EOS is asked for
                    state, depth, stack, accepting = eng.grammar_config(0)
                    assert accepting and depth == 0 and stack == 0 and state >= 0
                eng.decode(1, batch=1)
                out.append(eng.read_pending(1)[0])
            if out[-1] != t:
                break
        return eng, out, ids
    except Exception:
        eng.close()
        raise


@pytest.mark.parametrize("script", [
    [b'{"a":[', b"[", b"1", b"],[", b'"abcdefghijklm"]', b",", b"{", b'"', b"b", b'"', b":", b"{", b"}}", b"]", b"}"],
    [b"[[", b'"abcdefghijklmno"', b",", b" ", b"[[", b"0", b"]]]]"],
    [b"[1,2,3,4,5,6,7,8,9]"],
])
def test_scripted_document_is_produced(tiny, dev_tiny, script):
    eng, out, ids = _scripted(tiny, dev_tiny, "json", script, then_eos=True)
    try:
        assert out == ids, (out, ids)
        text = text_of(out[:-1], 1024)
        assert text == b"".join(script)
        json.loads(text)
        assert eng.grammar_config(0) == (-1, 0, 0, True)
    finally:
        eng.close()


@pytest.mark.parametrize("script", [
    [b"{", b'"', b"a", b'"', b":", b"1", b"]"],   # ']' closing an object
    [b"[["] * 16 + [b"["],                        # a 33rd '['
    [b"1", b","],                                 # ',' at top level
    [b"[", b'"abcdefghijklmn"]'],                 # a long token that closes a container opened before it
])
def test_scripted_error_is_not_produced(tiny, dev_tiny, script):
    eng, out, ids = _scripted(tiny, dev_tiny, "json", script)
    try:
        assert len(out) == len(ids) and out[:-1] == ids[:-1] and out[-1] != ids[-1], (out, ids)
        g = oracle_of("json", 1024)
        assert g.alive(text_of(before_eos(out, 1024)[0], 1024)) is not None
        assert g.alive(text_of(ids, 1024)) is None or len(vocabulary(1024)[ids[-1]]) > 16
    finally:
        eng.close()


# -- 4. step splitting and life cycle -----------------------------------------------------------------------------------------------
def test_step_splitting(tiny, dev_tiny):
    def run(calls):
        sim = Sim(tiny, 4, dev_tiny)
        try:
            for i in range(4):
                sim.start(i, _mixed(i + 2, sim.V), list(range(20 + i, 30 + 2 * i)))  # regex, brackets, JSON sampled, JSON greedy
            for c in calls:
                sim.eng.decode(c, batch=4)
            return [sim.eng.read_tokens(i, 9) for i in range(4)], [sim.eng.grammar_config(i) for i in range(4)]
        finally:
            sim.close()

    assert run([8]) == run([3, 5]) == run([1] * 8)


def test_life_cycle(tiny, dev_tiny):
    sim = Sim(tiny, 4, dev_tiny)
    eng = sim.eng
    try:
        sim.start(2, _mixed(5, sim.V), list(range(30, 40)))  # JSON, greedy, brackets favoured
        for _ in range(4):
            sim.step(3)
        assert eng.grammar_config(2)[1] >= 1, "the slot is inside a container"
        # move mid-generation: grammar and configuration go with the sequence
        before = eng.grammar_config(2)
        eng.move(2, 0)
        assert eng.grammar_config(0) == before
        for d in (sim.cfg, sim.hist, sim.state, sim.pending, sim.out):
            d[0] = d.pop(2)
        with pytest.raises(RuntimeError):
            eng.grammar_config(2)
        for _ in range(2):
            sim.step(1)
        # fork: the child starts from the parent's configuration, then both go their own way
        eng.fork(0, 1)
        sim.cfg[1], sim.hist[1], sim.state[1] = dict(sim.cfg[0], smp=(0.9, 30, 1.0, 77)), sim.hist[0].copy(), sim.state[0]
        sim.pending[1], sim.out[1] = sim.pending[0], list(sim.out[0])
        eng.set_sampling(1, 0.9, 30, None, 77)
        assert eng.grammar_config(1) == eng.grammar_config(0)
        for _ in range(6):
            sim.step(2)
        viable(sim, 0), viable(sim, 1)
        # verify / rewind / set_token refuse the slot ...
        eng.begin(3)
        eng.set_grammar(3, dev_tiny.grammar("brackets"))
        eng.prefill(3, [1, 2, 3])
        for call in (lambda: eng.verify(3, [1, 2]), lambda: eng.rewind(3, 1), lambda: eng.set_token(3, 5)):
            with pytest.raises(RuntimeError):
                call()
        # ... and work again once the grammar is cleared
        eng.set_grammar(3, None)
        with pytest.raises(RuntimeError):
            eng.grammar_config(3)
        eng.rewind(3, 1)
        eng.set_token(3, 5)
        eng.release(3)
        # release + begin clear the grammar; a fresh one starts at (start, 0, 0), whatever the slot held before
        eng.release(1)
        del sim.cfg[1]
        sim.start(1, _cfg(), list(range(30, 40)))
        with pytest.raises(RuntimeError):
            eng.grammar_config(1)
        eng.release(1)
        del sim.cfg[1]
        eng.begin(1)
        eng.set_grammar(1, dev_tiny.grammar("json"))
        g = oracle_of("json", 1024)
        assert eng.grammar_config(1) == (*g.start, False)
        eng.release(1)
        sim.assert_few_ambiguous()
    finally:
        sim.close()


def test_grammar_set_on_a_slot_with_a_pending_token(tiny, dev_tiny):
    """the pending token is fed by the next step and advances the new grammar's configuration then; grammar_config includes it at once"""
    eng = RG._engine(tiny, 1)
    try:
        g = oracle_of("json", 1024)
        eng.begin(0)
        eng.set_logit_bias(0, {tok(b'{"a":['): 100.0})
        eng.prefill(0, list(range(10, 20)))
        assert eng.read_tokens(0, 1) == [tok(b'{"a":[')]
        eng.set_grammar(0, dev_tiny.grammar("json"))
        want = g.advance(g.start, tok(b'{"a":['))
        assert want[1] == 2 and eng.grammar_config(0) == (*want, False)
        eng.decode(1, batch=1)
        assert eng.grammar_config(0) == (*g.advance(want, tok(b'{"a":[')), False)  # ('{' opens the array's first element)
        assert eng.grammar_config(0)[1] == 4
    finally:
        eng.close()


# -- 5. unchanged programs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grammar", [None, RECORD])
def test_programs_without_a_stack_grammar_are_unchanged(tiny, dev_tiny, grammar):
    prompt, steps = list(range(100, 112)), 10

    def run(setup):
        eng = RG._engine(tiny, 2)
        try:
            setup(eng)
            eng.begin(0)
            if grammar is not None:
                eng.set_grammar(0, dev_tiny.grammar(grammar))
            eng.prefill(0, prompt)
            eng.decode(steps, batch=1)
            ids, logits, stats = eng.read_tokens(0, steps + 1), eng.logits(1).float().cpu(), eng.stats()
            return ids, logits, stats["graph_captures"], eng.check_step(1)["launches"], stats["workspace_bytes"]
        finally:
            eng.close()

    fresh = run(lambda eng: None)
    other = RG._engine(tiny, 1)  # an engine of its own that holds a stack grammar from here on
    try:
        other.begin(0)
        other.set_grammar(0, dev_tiny.grammar("json"))
        other.prefill(0, prompt)
        other.decode(2, batch=1)
        beside = run(lambda eng: None)
        assert beside[0] == fresh[0] and torch.equal(beside[1], fresh[1]) and beside[2:] == fresh[2:], "nothing is allocated or captured anew"

        def released(eng):  # the engine's only stack slot was released (and another one cleared) before the run
            eng.begin(1)
            eng.set_grammar(1, dev_tiny.grammar("json"))
            eng.prefill(1, prompt[:5])
            eng.release(1)
            eng.begin(1)
            eng.set_grammar(1, dev_tiny.grammar("brackets"))
            eng.set_grammar(1, None)
            eng.release(1)

        after = run(released)
        assert after[0] == fresh[0] and torch.equal(after[1], fresh[1]) and after[2:4] == fresh[2:4]
    finally:
        other.close()


def test_a_step_goes_back_to_its_old_plan_when_the_stack_slot_is_released(tiny, dev_tiny):
    def run(with_stack_slot):
        eng = RG._engine(tiny, 2)
        try:
            eng.begin(0)
            eng.set_grammar(0, dev_tiny.grammar(RECORD))
            eng.prefill(0, list(range(100, 112)))
            eng.decode(3, batch=2)  # (eager warm step, then the regex twin's plan)
            captures = eng.stats()["graph_captures"]
            if with_stack_slot:
                eng.begin(1)
                eng.set_grammar(1, dev_tiny.grammar("json"))
                eng.prefill(1, [1, 2, 3])
                eng.decode(2, batch=2)
                assert eng.stats()["graph_captures"] == captures + 1, "the stack twin's plan is a plan of its own"
                eng.release(1)
            eng.decode(4, batch=2)
            return eng.read_tokens(0, 10 if with_stack_slot else 8), eng.stats()["graph_captures"] - captures
        finally:
            eng.close()

    with_slot, without = run(True), run(False)
    assert without[1] == 0 and with_slot[1] == 1, "after the release the step replays the plan it had before: nothing is captured again"
    eng = RG._engine(tiny, 2)
    try:  # the regex slot's ids do not depend on the company it had
        eng.begin(0)
        eng.set_grammar(0, dev_tiny.grammar(RECORD))
        eng.prefill(0, list(range(100, 112)))
        eng.decode(9, batch=2)
        assert eng.read_tokens(0, 10) == with_slot[0]
    finally:
        eng.close()


# -- 6. written once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5, 64])
def test_written_once_stack_plans(tiny, dev_tiny, n):
    def check(with_stack):
        sim = Sim(tiny, n, dev_tiny)
        try:
            for i in range(n):
                cfg = _mixed(i + 4, sim.V)  # slot 0 holds JSON at every n
                if not with_stack and cfg["grammar"] in ("json", "brackets"):
                    cfg = dict(cfg, grammar=RECORD)  # the corresponding regex twin's plan
                sim.start(i, cfg, list(range(3 + i % 7, 12 + i % 7)))
            sim.step(n)
            c = sim.eng.check_step(n)
            assert np.isfinite(sim.eng.logits(n).float().cpu().numpy()).all()
            return c, sim.eng.replay_route()
        finally:
            sim.close()

    (stack, route_s), (regex, route_r) = check(True), check(False)
    assert stack["double_writes"] == 0, stack
    assert regex["double_writes"] == 0, regex
    assert stack["written_once_plan"] == regex["written_once_plan"] and route_s == route_r, (stack, regex, route_s, route_r)
    assert stack["launches"] == regex["launches"], "the stack twin replaces the processing launch, it adds none"


# -- 7. the Qwen3-4B vocabulary width; FP8 pages ------------------------------------------------------------------------------------
def test_engine_qwen4b_shapes(q4b, dev_big):
    sim = Sim(q4b, 4, dev_big)
    try:
        rng = np.random.default_rng(44)
        for i in range(4):
            sim.start(i, _mixed(i + 2, sim.V), rng.integers(0, 1000, 6 + i).tolist())  # regex, brackets, JSON sampled, JSON greedy
        for _ in range(4):
            sim.step(4)
        sim.assert_few_ambiguous()
        for i in range(4):
            viable(sim, i)
    finally:
        sim.close()


def test_fp8_pages(q4b, dev_big):
    sim = _mixed_run(q4b, 4, 4, dev_big, first=2, kv_format="fp8")
    try:
        sim.assert_few_ambiguous()
        for i in range(4):
            viable(sim, i)
    finally:
        sim.close()


# -- 8. continuous batching ---------------------------------------------------------------------------------------------------------
def test_batch_generate_json(tiny, dev_tiny):
    from tiny_llm_hip.engine import batch_generate_ids

    rng = np.random.default_rng(8)
    prompts = [rng.integers(0, 1000, int(rng.integers(4, 30))).tolist() for _ in range(6)]
    constrained = [True, False, True, False, True, False]
    sampling = [dict({"grammar": dev_tiny.grammar("json-object")} if c else {}, **({"temperature": 0.9, "top_k": 40} if i % 3 == 2 else {}))
                for i, c in enumerate(constrained)]

    def run():
        eng = RG._engine(tiny, 5)
        try:
            return sorted(batch_generate_ids(eng, prompts, 24, batch_size=4, prefill_step=16, sampling=sampling))
        finally:
            eng.close()

    a = run()
    assert a == run()
    g = oracle_of("json-object", 1024)
    for idx, ids in a:
        if not constrained[idx]:
            assert len(ids) == 24
            continue
        text, ended = before_eos(ids, 1024)
        assert text and text_of(text, 1024)[:1] == b"{"
        assert g.alive(text_of(text, 1024)) is not None, (idx, text_of(text, 1024))
        if ended:
            assert len(ids) == len(text) + 1
            assert isinstance(json.loads(text_of(text, 1024)), dict)
        else:
            assert len(ids) == 24
