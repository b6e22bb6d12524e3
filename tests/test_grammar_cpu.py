"""CPU tier: the regex compiler of tiny_llm_hip/grammar.py against Python's ``re`` (full match over bytes), its helpers, and the
host-side validation of the grammar ABI through the built library (no device is touched: bad input is refused before any allocation)."""

import ctypes
import random
import re

import numpy as np
import pytest

from tiny_llm_hip import grammar as G

NUMBER = rb"-?(0|[1-9][0-9]{0,5})(\.[0-9]{1,3})?"
JSONISH = rb'\{"id": [0-9]{1,4}, "ok": (true|false)\}'

PATTERNS = [
    NUMBER,
    JSONISH,
    G.choice(["red", "green", "blue", "dark red", "a+b", "x|y", "tab\there"]),
    rb'"[^"\\]*"',                      # a negated class
    "café|naïve|日本".encode(),   # UTF-8 literals
    "é+x",                         # a str pattern: the quantifier binds the last BYTE, as in a bytes pattern
    rb"abc",
    rb"a|b|cd",
    rb"(ab)*c",
    rb"(?:ab)+c?",
    rb"a*b+c?d",
    rb"a{3}",
    rb"a{2,}b",
    rb"(ab){1,3}",
    rb"[a-c]{0,2}x{,2}",
    rb"\d+\.\d*",
    rb"\w+\s\w+",
    rb"\D\W\S",
    rb"[\d\s]+",
    rb"[^\w]+",
    rb"a.c",
    rb".*",
    rb"line\n\ttab\r",
    rb"\x41\x00[\x80-\xff]+",
    rb"\.\*\+\?\(\)\[\]\{\}\|\\",
    rb"[]a]+",
    rb"[a\-z]+",
    rb"[a-]+",
    rb"[^]]x",
    rb"a{b",                            # a brace that is no quantifier is a literal
    rb"(a|)b",
    rb"((a|b)(c|d))*",
    rb"[a-z]+( [a-z]+)*",
    rb"(0|1(01*0)*1)*",                 # multiples of three in binary
    rb"x(y(z)?)?",
    rb"[+-]?[0-9]+(e[+-]?[0-9]{1,2})?",
]


def _pattern_bytes(p):
    return p.encode("utf-8") if isinstance(p, str) else p


def _alphabet(dfa, pattern):
    used = np.flatnonzero((dfa.table != G.DEAD).any(axis=0)).tolist()
    extra = [b for b in pattern if b < 0x80][:8]
    return sorted(set(used[:40] + used[-8:] + extra + [0x00, 0x0A, 0x20, 0x61, 0xFF]))


def _samples(dfa, pattern, rng, want=2000):
    """Accepted strings and viable prefixes by random walks on the DFA, random strings over the pattern's alphabet, and single-byte
    mutations of accepted strings."""
    out, accepted = set(), []
    alpha = _alphabet(dfa, pattern)
    moves = [np.flatnonzero(dfa.table[s] != G.DEAD) for s in range(dfa.n_states)]
    tries = 0
    while len(out) < want and tries < 40 * want:
        tries += 1
        kind = tries % 4
        if kind in (0, 1):  # a walk that stops in an accepting state with some probability, or is cut short (kind 1)
            s, data = dfa.start, bytearray()
            limit = rng.randrange(1, 24)
            while len(data) < limit and len(moves[s]):
                if dfa.accepting[s] and rng.random() < 0.3:
                    break
                b = int(moves[s][rng.randrange(len(moves[s]))])
                data.append(b)
                s = int(dfa.table[s, b])
            data = bytes(data)
            if kind == 1 and data:
                data = data[:rng.randrange(0, len(data) + 1)]
            if dfa.accepting[dfa.walk(dfa.start, data)]:
                accepted.append(data)
        elif kind == 2 or not accepted:
            data = bytes(rng.choice(alpha) for _ in range(rng.randrange(0, 12)))
        else:
            data = bytearray(accepted[rng.randrange(len(accepted))])
            op = rng.randrange(3)
            at = rng.randrange(len(data) + 1)
            if op == 0 and data:
                data[min(at, len(data) - 1)] = rng.choice(alpha)
            elif op == 1:
                data.insert(at, rng.choice(alpha))
            elif data:
                del data[min(at, len(data) - 1)]
            data = bytes(data)
        out.add(data)
    return sorted(out)


@pytest.mark.parametrize("index", range(len(PATTERNS)))
def test_compile_regex_agrees_with_re_fullmatch(index):
    pattern = PATTERNS[index]
    raw = _pattern_bytes(pattern)
    dfa = G.compile_regex(pattern)
    ref = re.compile(raw)
    rng = random.Random(index)
    strings = _samples(dfa, raw, rng)
    assert len(strings) >= 2000, (pattern, len(strings))
    hits = 0
    for data in strings:
        want = ref.fullmatch(data) is not None
        hits += want
        assert dfa.accepts(data) == want, (pattern, data, want)
    assert hits > 0, "the sample holds accepted strings"
    # trimmed: every state is reachable from the start and can reach acceptance
    S = dfa.n_states
    assert dfa.start == 0 and dfa.table.shape == (S, 256) and dfa.accepting.shape == (S,)
    succ = [set(int(t) for t in dfa.table[s] if t != G.DEAD) for s in range(S)]
    seen, stack = {dfa.start}, [dfa.start]
    while stack:
        for t in succ[stack.pop()]:
            if t not in seen:
                seen.add(t)
                stack.append(t)
    assert seen == set(range(S)), "unreachable states"
    can = {s for s in range(S) if dfa.accepting[s]}
    grew = True
    while grew:
        grew = False
        for s in range(S):
            if s not in can and succ[s] & can:
                can.add(s)
                grew = True
    assert can == set(range(S)), "a state that cannot reach acceptance"


def test_minimal():
    assert G.compile_regex(rb"(a|b)*abb").n_states == 4
    assert G.compile_regex(rb"[^\"]*").n_states == 1
    assert G.compile_regex(rb"a|a|a").n_states == 2
    assert G.compile_regex(rb"(0|1(01*0)*1)*").n_states == 3


@pytest.mark.parametrize("bad", [rb"^a", rb"a$", rb"a*?", rb"a+?", rb"a??", rb"a{2}?", rb"a*+", rb"(?=a)b", rb"(?!a)b", rb"(?<=a)b",
                                 rb"(a)\1", rb"(?P<n>a)", rb"(?i)a", rb"\bword", rb"\Aa", rb"a\Z", rb"a**", rb"*a", rb"(a", rb"a)",
                                 rb"[a", rb"[z-a]", rb"a{3,2}", rb"\xg0", rb"\p", rb"a\\"[:-1], rb"[\d-z]", rb"[^\x00-\xff]", 12])
def test_unsupported_syntax_raises(bad):
    with pytest.raises(ValueError):
        G.compile_regex(bad)


def test_choice_and_escape():
    words = ["a.b", "x*", "café", "(", "", "tab\t"]
    dfa = G.compile_regex(G.choice(words))
    for w in words:
        assert dfa.accepts(w.encode())
    for w in (b"aXb", b"x", b"xx", b"caf", b"()"):
        assert not dfa.accepts(w)
    assert re.fullmatch(G.escape("a.b|c"), b"a.b|c") and not re.fullmatch(G.escape("a.b"), b"aXb")
    with pytest.raises(ValueError):
        G.choice([])


def test_check_vocabulary():
    dfa = G.compile_regex(JSONISH)
    full = [bytes([b]) for b in range(256)] + [b"true", b'"id"', b""]
    G.compile_regex(NUMBER).check_vocabulary(*G.vocabulary_bytes_from_strings(full))
    dfa.check_vocabulary(*G.vocabulary_bytes_from_strings(full))
    lacking = [t for t in full if t != b":"]  # no token can produce the colon: the state after "id" is stuck
    with pytest.raises(ValueError, match="state"):
        dfa.check_vocabulary(*G.vocabulary_bytes_from_strings(lacking))
    # a multi-byte token alone does not help when it walks out of the language
    with pytest.raises(ValueError, match="state"):
        G.compile_regex(rb"ab").check_vocabulary(*G.vocabulary_bytes_from_strings([b"a", b"bb", b"ba"]))
    G.compile_regex(rb"ab").check_vocabulary(*G.vocabulary_bytes_from_strings([b"a", b"b"]))


def test_vocabulary_bytes_from_strings():
    offsets, data = G.vocabulary_bytes_from_strings([b"ab", b"", b"\xff\x00c"])
    assert offsets.dtype == np.int32 and offsets.tolist() == [0, 2, 2, 5] and data.tobytes() == b"ab\xff\x00c"


class _FakeTokenizer:
    """A byte-level BPE vocabulary as GPT-2 / Qwen write it: every byte through the byte <-> unicode table."""

    def __init__(self):
        to_unicode = {b: ch for ch, b in G.gpt2_unicode_to_byte().items()}
        self.words = [bytes([b]) for b in range(256)] + [b" the", b"\n\n", "été".encode(), b"\x00\xff "]
        self.vocab = {"".join(to_unicode[b] for b in w): i for i, w in enumerate(self.words)}
        self.added = {"<|endoftext|>": len(self.words), "<|im_start|>": len(self.words) + 1}
        self.vocab.update(self.added)

    def get_vocab(self):
        return dict(self.vocab)

    def get_added_vocab(self):
        return dict(self.added)


def test_vocabulary_bytes_round_trips_every_byte():
    table = G.gpt2_unicode_to_byte()
    assert len(table) == 256 and sorted(table.values()) == list(range(256))
    assert table["Ġ"] == 0x20 and table["Ċ"] == 0x0A and table["!"] == 0x21  # the well-known entries: space and newline
    tok = _FakeTokenizer()
    offsets, data = G.vocabulary_bytes(tok, vocab_size=270)
    assert len(offsets) == 271
    got = [data[offsets[j]:offsets[j + 1]].tobytes() for j in range(270)]
    assert got[:len(tok.words)] == tok.words
    assert all(t == b"" for t in got[len(tok.words):]), "added tokens and ids without a token are empty"


# -- ABI validation, host only ------------------------------------------------------------------------------------------------------
def test_vocab_create_refuses_bad_input(built_libs):
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    data = (ctypes.c_uint8 * 8)(*b"abcdefgh")

    def create(vocab, offsets):
        arr = (ctypes.c_int32 * len(offsets))(*offsets)
        out = ctypes.c_void_p()
        rc = lib.tl_vocab_create(vocab, arr, data, None, ctypes.byref(out))
        assert rc != 0 and not out.value
        return rc

    INVALID = create(0, [0])  # (TL_ERR_INVALID: the code every refusal below shares)
    assert create(3, [1, 2, 3, 4]) == INVALID        # offsets[0] != 0
    assert create(3, [0, 4, 2, 8]) == INVALID        # decreasing
    assert create(3, [0, -1, 2, 8]) == INVALID
    assert create(-1, [0]) == INVALID
    assert create(1 << 20, [0]) == INVALID           # beyond the sampler's vocabulary limit
    out = ctypes.c_void_p()
    assert lib.tl_vocab_create(3, None, data, None, ctypes.byref(out)) == INVALID
    assert lib.tl_vocab_create(3, (ctypes.c_int32 * 4)(0, 1, 2, 3), None, None, ctypes.byref(out)) == INVALID
    # the other entry points refuse null handles before anything else
    assert lib.tl_grammar_create(None, 1, None, None, 0, None, 1, None, ctypes.byref(out)) == INVALID
    assert lib.tl_grammar_mask_rows(None, None, 1, None, None, None) == INVALID
    assert lib.tl_engine_set_grammar(None, 0, None) != 0
    lib.tl_vocab_destroy(None)
    lib.tl_grammar_destroy(None)


def test_request_dicts_accept_a_grammar():
    from tiny_llm_hip import engine as E

    pens = E.request_settings([{"grammar": None, "repetition_penalty": 1.2}], 1, vocab_size=1024)
    assert [(s.penalties, s.bias) for s in pens] == [((1.2, 0.0, 0.0), {})]
    assert [s.grammar for s in E.request_settings([{"grammar": None}, {}], 2)] == [None, None]
    assert [s.grammar for s in E.request_settings(None, 3)] == [None] * 3
    with pytest.raises(ValueError):
        E.request_settings({"grammar": "a+"}, 1)
    assert E.request_settings({"grammar": None, "temperature": 0.5}, 1)[0].sampling[0] == 0.5
