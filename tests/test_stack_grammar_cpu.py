"""CPU tier: JSON mode on the host (tiny_llm_hip/grammar.py: StackDFA, compile_json, schema_regex) against Python's ``json`` and
``re``, and StackDFA.walk against the plain-Python restatement of the header's definition (tests/stack_grammar_oracle.py)."""

import functools
import json
import random
import re

import numpy as np
import pytest

import stack_grammar_oracle as SO
from tiny_llm_hip import grammar as G


@functools.lru_cache(maxsize=None)
def dfa(top="value", whitespace="free"):
    return G.compile_json(top, whitespace)


def _refuse(_):
    raise ValueError("NaN / Infinity are not JSON")


def nesting(text: bytes) -> int:
    """the deepest bracket nesting outside strings (of a text json.loads accepted)"""
    depth = deepest = 0
    in_string = escaped = False
    for b in text:
        if in_string:
            if escaped:
                escaped = False
            elif b == 0x5C:
                escaped = True
            elif b == 0x22:
                in_string = False
        elif b == 0x22:
            in_string = True
        elif b in b"[{":
            depth += 1
            deepest = max(deepest, depth)
        elif b in b"]}":
            depth -= 1
    return deepest


def strict_json(text: bytes) -> bool:
    """RFC 8259 as Python reads it: the bytes are strict UTF-8 (json.loads on bytes would also guess UTF-16 / 32 and skip a BOM), no
    NaN / Infinity, no raw control character in a string; nesting within the engine's 32 levels."""
    try:
        json.loads(text.decode("utf-8"), parse_constant=_refuse)
    except (ValueError, RecursionError):
        return False
    return nesting(text) <= 32


# -- JSON acceptance ----------------------------------------------------------------------------------------------------------------
def test_every_short_string():
    """every byte string of up to 5 bytes over the alphabet (N and I stay out: json.loads reads NaN and Infinity)"""
    d = dfa()
    alphabet = b'{}[]",:-01.eE\\utfna '
    assert len(set(alphabet)) == 20
    checked = accepted = 0
    bad = []

    def visit(prefix, cfg):
        nonlocal checked, accepted
        got = cfg is not None and bool(d.accepting[cfg[0]])
        checked += 1
        accepted += got
        if got != strict_json(prefix):
            bad.append(prefix)
        if len(prefix) == 5:
            return
        for b in alphabet:
            visit(prefix + bytes([b]), d.walk(cfg, bytes([b])) if cfg is not None else None)

    visit(b"", (d.start, 0, 0))
    assert checked == sum(20 ** k for k in range(6)) and accepted > 500
    assert not bad, bad[:10]


def random_value(rng, depth=0):
    kind = rng.randrange(9 if depth < 5 else 7)
    if kind == 0:
        return rng.choice([None, True, False])
    if kind == 1:
        return rng.randrange(-10 ** rng.randrange(1, 12), 10 ** rng.randrange(1, 12))
    if kind == 2:
        return rng.choice([0.0, -0.0, 1.5, -2.25e-7, 6.02e23, 1e-300, rng.uniform(-1e6, 1e6), float(rng.randrange(1000))])
    if kind < 7:
        chars = 'abc xyz019_"\\/\b\f\n\r\t\x00\x1f\x7f\u00e9\u00fc\u00f1\u20ac\u65e5\u672c\U0001f600\ud7ff\uffff'
        return "".join(rng.choice(chars) for _ in range(rng.randrange(0, 9)))
    if kind == 7:
        return [random_value(rng, depth + 1) for _ in range(rng.randrange(0, 4))]
    return {rng.choice(["k%d", "\u00e9%d", 'q"%d', "%d"]) % i: random_value(rng, depth + 1) for i in range(rng.randrange(0, 4))}


@functools.lru_cache(maxsize=None)
def documents():
    rng = random.Random(8259)
    docs = []
    for i in range(2000):
        v = random_value(rng)
        style = i % 4
        if style == 0:
            docs.append(json.dumps(v, ensure_ascii=False).encode())
        elif style == 1:
            docs.append(json.dumps(v).encode())
        elif style == 2:
            docs.append(json.dumps(v, ensure_ascii=False, separators=(",", ":")).encode())
        else:
            docs.append(json.dumps(v, ensure_ascii=False, indent=rng.choice([1, 2, "\t"])).encode())
    return docs


def test_random_documents():
    d = dfa()
    docs = documents()
    assert sum(any(b >= 0x80 for b in x) for x in docs) > 200, "non-ASCII strings are among them"
    assert max(nesting(x) for x in docs) >= 4
    for x in docs:
        assert strict_json(x) and d.accepts(x), x


def test_mutated_documents():
    """one byte deleted, replaced or inserted: the automaton agrees with json.loads on what is left"""
    d = dfa()
    rng = random.Random(1)
    pool = b'{}[]",:-01.eE\\utfna \n\x00\x1f\x7f\x80\xbf\xc0\xc3\xe0\xed\xf0\xf4\xf5\xff9+'
    rejected = 0
    for x in documents():
        for kind in range(3):
            at = rng.randrange(len(x) + (kind == 2))
            new = bytes([rng.choice(pool)])
            y = x[:at] + (b"" if kind == 0 else new) + x[at + (kind != 2):]
            want = strict_json(y)
            rejected += not want
            assert d.accepts(y) == want, (x, y, want)
    assert rejected > 2000


def test_edge_cases():
    d = dfa()
    for k in (1, 31, 32):
        assert d.accepts(b"[" * k + b"]" * k) and d.accepts(b'{"a":' * k + b"1" + b"}" * k)
    assert d.accepts(b'[{"a":' * 16 + b"null" + b"}]" * 16)
    assert not d.accepts(b"[" * 33 + b"]" * 33) and not d.accepts(b'{"a":' * 33 + b"1" + b"}" * 33)
    assert not d.accepts(b'[{"a":' * 16 + b"[]" + b"}]" * 16)
    assert d.walk((d.start, 0, 0), b"[" * 32) is not None and d.walk((d.start, 0, 0), b"[" * 33) is None
    # UTF-8: every class of malformation (Unicode table 3-7)
    good = ["\u00e9", "\u20ac", "\u65e5", "\U0001f600", "\u07ff", "\u0800", "\ud7ff", "\ue000", "\uffff", "\U00010000", "\U0010ffff", "\x7f"]
    for ch in good:
        assert d.accepts(b'"' + ch.encode() + b'"'), ch
    bad = [b"\x80", b"\xbf", b"\xc3", b"\xc3\x28", b"\xe2\x82", b"\xe2\x28\xa1", b"\xf0\x9f\x98",  # stray / missing continuation bytes
           b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xf0\x80\x80\x80", b"\xf0\x8f\xbf\xbf",  # overlong forms
           b"\xed\xa0\x80", b"\xed\xbf\xbf",  # surrogates
           b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xfe", b"\xff"]  # above U+10FFFF
    for raw in bad:
        assert not d.accepts(b'"' + raw + b'"') and not d.accepts(b'"a' + raw + b'b"'), raw
    for b in range(0x20):
        assert not d.accepts(b'"' + bytes([b]) + b'"')
    # escapes
    for text in [rb'"\""', rb'"\\"', rb'"\/"', rb'"\b\f\n\r\t"', rb'"\u00e9"', rb'"\ud83d\ude00"', rb'"\ud800"', rb'"\uABcd"']:
        assert d.accepts(text) and strict_json(text), text
    for text in [rb'"\u"', rb'"\u1"', rb'"\u12"', rb'"\u123"', rb'"\u123g"', rb'"\U0041"', rb'"\a"', rb'"\x41"', rb'"\'"', rb'"\u 041"', b'"\\']:
        assert not d.accepts(text) and not strict_json(text), text
    # numbers
    for text in [b"0", b"-0", b"10", b"-1.5", b"0.0", b"1e5", b"1E+5", b"1.25e-10", b"0e0"]:
        assert d.accepts(text) and strict_json(text), text
    for text in [b"00", b"01", b"-01", b"-", b"+1", b".5", b"1.", b"1.e5", b"1e", b"1e+", b"0x10", b"1_0", b"--1", b"1 2", b"Infinity", b"NaN"]:
        assert not d.accepts(text), text
    for text in [b"true", b"false", b"null", b" \t\n\r[ 1 , 2 ]\n", b'{ "a" : [ ] , "b" : { } }', b"[]", b"{}", b'""']:
        assert d.accepts(text) and strict_json(text), text
    for text in [b"", b" ", b"True", b"nul", b"[1,]", b"[,1]", b'{"a":1,}', b"{1:2}", b'{"a"}', b'{"a":}', b"[1 2]", b"[1]]", b"[}", b'{"a":1]',
                 b"[1],", b"1,", b"\xef\xbb\xbf1", b"1\x00", b"[1\x0b]", b"'a'"]:
        assert not d.accepts(text) and not strict_json(text), text
    # top="object" refuses a top-level scalar or array; what it accepts is what "value" accepts among objects
    o = dfa("object", "free")
    for text in [b"1", b'"a"', b"null", b"[]", b"[{}]", b""]:
        assert not o.accepts(text), text
    for text in [b"{}", b' {"a": [1, {"b": null}]} ', b'{"a":' * 32 + b"1" + b"}" * 32]:
        assert o.accepts(text), text
    # an accepting state implies an empty stack: no configuration reached by a prefix with open brackets is accepting
    for prefix in [b"[", b"[1", b'{"a":1', b"[[]", b'[{"a":[]}', b"[1 "]:
        cfg = d.walk((d.start, 0, 0), prefix)
        assert cfg is not None and cfg[1] > 0 and not d.accepting[cfg[0]]
    with pytest.raises(ValueError):
        G.compile_json("array")
    with pytest.raises(ValueError):
        G.compile_json("value", "pretty")
    with pytest.raises(ValueError):
        G.compile_json("value", "free", max_depth=8)
    for top in ("value", "object"):
        for mode in ("free", "compact"):
            assert 64 < dfa(top, mode).n_states <= 250 and dfa(top, mode).n_pop == 1


def test_compact_mode():
    for top in ("value", "object"):
        c = dfa(top, "compact")
        for x in documents()[:600]:
            v = json.loads(x)
            if top == "object" and not isinstance(v, dict):
                assert not c.accepts(json.dumps(v, separators=(",", ":")).encode())
                continue
            tight, loose = json.dumps(v, ensure_ascii=False, separators=(",", ":")).encode(), json.dumps(v, separators=(", ", ": ")).encode()
            assert c.accepts(tight) and c.accepts(loose), (tight, loose)
    c = dfa("value", "compact")
    assert c.accepts(b'{"a": [1, 2],"b":{"c": null}}')
    for text in [b'{"a":  1}', b"[1,  2]", b" 1", b"1 ", b"[ 1]", b"[1 ]", b'{ "a":1}', b'{"a" :1}', b'{"a":1 }', b"[1,\n2]", b"[1,\t2]", b"[ ]", b"{ }"]:
        assert not c.accepts(text) and dfa().accepts(text), text


# -- schema_regex -------------------------------------------------------------------------------------------------------------------
SCHEMAS = [
    ({"type": "object", "properties": {"id": {"type": "integer"}, "ok": {"type": "boolean"}}, "required": ["id", "ok"]},
     [{"id": 7, "ok": True}, {"id": -120, "ok": False}, {"id": 0, "ok": True}],
     [{"ok": True, "id": 7}, {"id": 7}, {"id": 1.5, "ok": True}, {"id": 7, "ok": None}, {"id": 7, "ok": True, "x": 1}, [], 7]),
    ({"type": "object", "properties": {"name": {"type": "string", "maxLength": 6}, "colour": {"type": "string", "enum": ["red", "dark blue", "é"]},
                                       "v": {"const": "1.0"}}},
     [{"name": "", "colour": "red", "v": "1.0"}, {"name": "a \"b\"", "colour": "dark blue", "v": "1.0"}, {"name": "日本語", "colour": "é", "v": "1.0"}],
     [{"name": "toolong", "colour": "red", "v": "1.0"}, {"name": "a", "colour": "blue", "v": "1.0"}, {"name": "a", "colour": "red", "v": "1"},
      {"name": 5, "colour": "red", "v": "1.0"}]),
    ({"type": "array", "items": {"type": "number"}, "minItems": 1, "maxItems": 3},
     [[1], [1.5, -2], [0, 1e300, -0.25], [6.02e+23]],
     [[], [1, 2, 3, 4], ["1"], [None], 1, [[1]]]),
    ({"anyOf": [{"type": "null"}, {"type": "integer"}, {"type": "array", "items": {"type": "object", "properties": {"p": {"type": "boolean"}}}}]},
     [None, 5, [], [{"p": True}], [{"p": False}, {"p": True}, {"p": True}, {"p": False}]],
     [True, "x", 1.5, [5], [{"p": 1}], [{}], {"p": True}]),
    ({"type": "object", "properties": {"user": {"type": "object", "properties": {"id": {"type": "integer"},
                                                                                  "tags": {"type": "array", "items": {"type": "string", "maxLength": 3}, "maxItems": 2}}},
                                       "score": {"anyOf": [{"type": "number"}, {"type": "null"}]}}},
     [{"user": {"id": 1, "tags": []}, "score": None}, {"user": {"id": 22, "tags": ["a", "bcd"]}, "score": 0.5}],
     [{"user": {"id": 1, "tags": ["a", "b", "c"]}, "score": 1}, {"user": {"id": 1, "tags": ["abcd"]}, "score": 1}, {"user": {"id": 1}, "score": 1},
      {"user": {"tags": [], "id": 1}, "score": 1}, {"user": {"id": 1, "tags": []}, "score": "1"}]),
]


@pytest.mark.parametrize("k", range(len(SCHEMAS)))
def test_schema_regex(k):
    schema, good, bad = SCHEMAS[k]
    pattern = G.schema_regex(schema)
    compiled = G.compile_regex(pattern)
    assert compiled.n_states < 32768
    for doc, want in [(x, True) for x in good] + [(x, False) for x in bad]:
        text = json.dumps(doc, separators=(",", ":")).encode()
        assert bool(re.fullmatch(pattern, text)) == want, (text, want)
        assert compiled.accepts(text) == want, (text, want)
        assert dfa("value", "compact").accepts(text), "what a schema admits is JSON"


def test_schema_regex_refuses_what_it_does_not_support():
    for schema, word in [({"type": "string", "pattern": "a+"}, "pattern"), ({"type": "integer", "minimum": 0}, "minimum"),
                         ({"$ref": "#/definitions/x"}, "$ref"), ({"type": "object", "properties": {"a": {"type": "string", "format": "date"}}}, "format"),
                         ({"type": "array", "items": {"type": "integer"}, "uniqueItems": True}, "uniqueItems"), ({"type": "tuple"}, "type"),
                         ({"type": "object", "properties": {"a": {"type": "null"}}, "required": []}, "required"),
                         ({"type": "object", "properties": {}, "additionalProperties": True}, "additionalProperties"), ({"oneOf": [{"type": "null"}]}, "oneOf")]:
        with pytest.raises(ValueError, match=re.escape(word)):
            G.schema_regex(schema)


# -- the oracle against StackDFA ----------------------------------------------------------------------------------------------------
def bracket_automaton():
    """five states, four stack symbols: state = what is on top (4: nothing); an opener pushes, the matching closer pops"""
    opens, closes = b"([{<", b")]}>"
    table = np.full((5, 256), 0xFFFF, dtype=np.uint16)
    ops = np.zeros((5, 256), dtype=np.uint8)
    for s in range(5):
        for b in b"abcdefghijklmnopqrstuvwxyz0123456789 ":
            table[s, b] = s
        for a in range(4):
            table[s, opens[a]], ops[s, opens[a]] = a, 1 + a
        if s < 4:
            table[s, closes[s]], ops[s, closes[s]] = 0, 5
    return G.StackDFA(table, ops, [[0, 1, 2, 3, 4]], [0, 0, 0, 0, 1], 4)


@pytest.mark.parametrize("which", ["brackets", "json"])
def test_walk_equals_the_oracle(which):
    d = bracket_automaton() if which == "brackets" else dfa()
    rng = random.Random(3)
    pieces = [bytes([b]) for b in b'()[]{}<>ab01 ",:-.e\\'] + [b"],[", b"}}", b'{"a":[', b"]]]]", b"[" * 17, b"true", b'"k":', b"[[", "\u00e9".encode()]
    tokens = [b"".join(rng.choice(pieces) for _ in range(rng.randrange(1, 5))) for _ in range(300)] + [b"[" * 33, b"]" * 33, b""]
    o = SO.StackGrammar(d.table, d.ops, d.pop_table, d.accepting, d.start, tokens, [len(tokens) - 1])
    # states a text can be in (a random state of the JSON automaton is mostly one a few bytes can leave), under random stacks
    prefixes = [b"", b"[", b"[1", b'{"a":', b'{"a":1', b'["x', b'[{"k":"v"', b"[[", b'{"a":[1,2', b"[tru", b'{"a":{', b"[-1.5e", b"[ ", b'{"a"']
    states = list(range(d.n_states)) if which == "brackets" else [d.walk((d.start, 0, 0), p)[0] for p in prefixes]
    died = lived = below = full = 0
    for _ in range(4000):
        depth = rng.choice([0, 0, 1, 2, 5, 31, 32, rng.randrange(33)])
        cfg = (rng.choice(states), depth, rng.getrandbits(2 * depth) if depth else 0)
        j = rng.randrange(len(tokens) - 1)
        want = o.alive(tokens[j], cfg)
        got = d.walk(cfg, tokens[j])
        assert got == want, (cfg, tokens[j], got, want)
        died += want is None
        lived += want is not None
        if want is None:  # which edge killed it: a pop below the start of the token, or a push at depth 32
            c = cfg
            for b in tokens[j]:
                nxt = o.byte(c, b)
                if nxt is None:
                    t, op = int(d.table[c[0], b]), int(d.ops[c[0], b])
                    below += t != 0xFFFF and op == 5 and c[1] == 0
                    full += t != 0xFFFF and 1 <= op <= 4 and c[1] == 32
                    break
                c = nxt
    assert died > 500 and lived > 300 and below > 20 and full > 20, (died, lived, below, full)
    assert d.accepts(b"") == (which == "brackets")
    if which == "brackets":
        assert d.accepts(b"a(b[c]{<>})") and not d.accepts(b"(]") and not d.accepts(b"(") and not d.accepts(b")")


def test_check_vocabulary():
    d = dfa("value", "compact")  # (with free whitespace every state can at least produce a space)
    single = [bytes([b]) for b in range(256)]
    d.check_vocabulary(*G.vocabulary_bytes_from_strings(single))
    with pytest.raises(ValueError, match="state"):
        d.check_vocabulary(*G.vocabulary_bytes_from_strings([b for b in single if b != b":"]))


def test_cli_takes_one_constraint():
    import main

    parser = main.build_parser()
    assert parser.parse_args(["--model", "m", "--json", "object"]).json == "object"
    assert parser.parse_args(["--model", "m", "--json-schema", "s.json"]).json_schema == "s.json"
    for argv in (["--json", "value", "--regex", "a+"], ["--json-schema", "s.json", "--regex", "a+"], ["--json", "object", "--json-schema", "s.json"],
                 ["--json", "array"]):
        with pytest.raises(SystemExit):
            parser.parse_args(["--model", "m"] + argv)
