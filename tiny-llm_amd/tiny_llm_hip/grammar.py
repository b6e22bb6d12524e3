"""Host side of regex-constrained decoding (include/tinyllm_engine.h "grammars"): a regular expression becomes a byte-level DFA, a
tokenizer's vocabulary becomes byte strings; the decode engine uploads both once (DecodeEngine.make_vocab / make_grammar) and masks
every logits row of a constrained slot on the device.

``compile_regex`` is Thompson NFA -> subset construction -> removal of states that cannot reach acceptance -> minimisation, so every
state of the result still has a way to finish.  Matching is FULL-match.  The dialect is Python ``re`` over a BYTES pattern (a ``str``
pattern is UTF-8 encoded first), restricted to

    literals and backslash-escaped punctuation       \\d \\w \\s \\D \\W \\S (ASCII, as for bytes patterns)   \\n \\t \\r \\xHH
    .  (any byte but \\n)                             [...] and [^...] with ranges and the escapes above
    ( ) and (?: )          |          * + ? {m} {m,} {m,n}

Anything else raises ValueError: anchors, look-around, back-references, named groups, lazy and possessive quantifiers, flags, other
backslash-letter escapes.  LIMITATION: everything is over bytes.  A negated class (and ``.``, ``\\D \\W \\S``) admits any byte outside its
set, so it can admit a partial or invalid UTF-8 sequence; a non-ASCII character inside a class stands for its separate bytes.  Spell
multi-byte characters as literals or alternations where that matters."""

from __future__ import annotations

from typing import Iterable, Sequence

import numpy as np

DEAD = 0xFFFF
MAX_STATES = 32768
_ALL = (1 << 256) - 1


def _mask(byte_values: Iterable[int]) -> int:
    m = 0
    for b in byte_values:
        m |= 1 << b
    return m


_DIGIT = _mask(range(0x30, 0x3A))
_WORD = _DIGIT | _mask(range(0x41, 0x5B)) | _mask(range(0x61, 0x7B)) | (1 << 0x5F)
_SPACE = _mask(b" \t\n\r\f\v")
_CLASS_ESCAPES = {ord("d"): _DIGIT, ord("w"): _WORD, ord("s"): _SPACE, ord("D"): _ALL & ~_DIGIT, ord("W"): _ALL & ~_WORD,
                  ord("S"): _ALL & ~_SPACE}
_CHAR_ESCAPES = {ord("n"): 0x0A, ord("t"): 0x09, ord("r"): 0x0D}
_HEX = b"0123456789abcdefABCDEF"
_MAX_REPEAT = 1000


class _Parser:
    """Pattern bytes -> a tree of ("set", mask) / ("cat", [..]) / ("alt", [..]) / ("rep", node, m, n or None)."""

    def __init__(self, pattern: bytes):
        self.p, self.i = pattern, 0

    def error(self, what: str):
        return ValueError(f"compile_regex: {what} at position {self.i} of {self.p!r}")

    def peek(self) -> int:
        return self.p[self.i] if self.i < len(self.p) else -1

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            raise self.error("unbalanced parenthesis")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == ord("|"):
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() not in (-1, ord("|"), ord(")")):
            items.append(self.repeat())
        return ("cat", items)

    def repeat(self):
        node = self.atom()
        q = self.quantifier()
        if q is None:
            return node
        nxt = self.peek()
        if nxt == ord("?"):
            raise self.error("lazy quantifiers are not supported")
        if nxt == ord("+"):
            raise self.error("possessive quantifiers are not supported")
        if nxt == ord("*") or (nxt == ord("{") and self.braces(self.i) is not None):
            raise self.error("multiple repeat")
        return ("rep", node, q[0], q[1])

    def braces(self, at: int):
        """{m} {m,} {m,n} {,n} at p[at:] -> (m, n or None, end), else None (the brace is then a literal, as in ``re``)."""
        j = at + 1
        lo = j
        while j < len(self.p) and 0x30 <= self.p[j] <= 0x39:
            j += 1
        m_txt = self.p[lo:j]
        if j < len(self.p) and self.p[j] == ord("}"):
            return (int(m_txt), int(m_txt), j + 1) if m_txt else None
        if j >= len(self.p) or self.p[j] != ord(","):
            return None
        j += 1
        lo = j
        while j < len(self.p) and 0x30 <= self.p[j] <= 0x39:
            j += 1
        n_txt = self.p[lo:j]
        if j >= len(self.p) or self.p[j] != ord("}") or (not m_txt and not n_txt):
            return None
        return (int(m_txt) if m_txt else 0, int(n_txt) if n_txt else None, j + 1)

    def quantifier(self):
        c = self.peek()
        if c == ord("*"):
            self.i += 1
            return (0, None)
        if c == ord("+"):
            self.i += 1
            return (1, None)
        if c == ord("?"):
            self.i += 1
            return (0, 1)
        if c == ord("{"):
            b = self.braces(self.i)
            if b is None:
                return None
            m, n, end = b
            if (n is not None and n < m) or m > _MAX_REPEAT or (n is not None and n > _MAX_REPEAT):
                raise self.error(f"bad repeat interval (counts up to {_MAX_REPEAT})")
            self.i = end
            return (m, n)
        return None

    def escape(self, in_class: bool):
        """After a backslash: ("set", mask) for a class escape, else the byte value."""
        c = self.peek()
        if c == -1:
            raise self.error("bad escape (end of pattern)")
        self.i += 1
        if c in _CLASS_ESCAPES:
            return ("set", _CLASS_ESCAPES[c])
        if c in _CHAR_ESCAPES:
            return _CHAR_ESCAPES[c]
        if c == ord("x"):
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or h[0] not in _HEX or h[1] not in _HEX:
                raise self.error("incomplete escape \\x")
            self.i += 2
            return int(h, 16)
        if (0x30 <= c <= 0x39) or (0x41 <= c <= 0x5A) or (0x61 <= c <= 0x7A):
            raise self.error(f"unsupported escape \\{chr(c)}")
        return c

    def atom(self):
        c = self.peek()
        self.i += 1
        if c == ord("("):
            if self.peek() == ord("?"):
                if self.p[self.i:self.i + 2] != b"?:":
                    raise self.error("only (?: ) groups are supported (no look-around, flags or named groups)")
                self.i += 2
            node = self.alt()
            if self.peek() != ord(")"):
                raise self.error("missing )")
            self.i += 1
            return node
        if c == ord("["):
            return self.char_class()
        if c == ord("."):
            return ("set", _ALL & ~(1 << 0x0A))
        if c == ord("\\"):
            e = self.escape(False)
            return e if isinstance(e, tuple) else ("set", 1 << e)
        if c in (ord("^"), ord("$")):
            self.i -= 1
            raise self.error("anchors are not supported (matching is full-match)")
        if c in (ord("*"), ord("+"), ord("?")):
            self.i -= 1
            raise self.error("nothing to repeat")
        return ("set", 1 << c)

    def char_class(self):
        negate = False
        if self.peek() == ord("^"):
            negate = True
            self.i += 1
        mask, first = 0, True
        while True:
            c = self.peek()
            if c == -1:
                raise self.error("unterminated character set")
            if c == ord("]") and not first:
                self.i += 1
                break
            first = False
            self.i += 1
            lo = self.escape(True) if c == ord("\\") else c
            if isinstance(lo, tuple):
                if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                    raise self.error("bad character range (a class escape as an end point)")
                mask |= lo[1]
                continue
            if self.peek() == ord("-") and self.i + 1 < len(self.p) and self.p[self.i + 1] != ord("]"):
                self.i += 1
                c2 = self.peek()
                self.i += 1
                hi = self.escape(True) if c2 == ord("\\") else c2
                if isinstance(hi, tuple) or hi < lo:
                    raise self.error("bad character range")
                mask |= _mask(range(lo, hi + 1))
            else:
                mask |= 1 << lo
        if negate:
            mask = _ALL & ~mask
        return ("set", mask)


class _NFA:
    def __init__(self):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple[int, int]]] = []  # (mask, target)

    def new(self) -> int:
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> tuple[int, int]:
        """Thompson fragment of `node`: (entry, exit)."""
        kind = node[0]
        if kind == "set":
            a, b = self.new(), self.new()
            if node[1]:
                self.edges[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = self.new()
            cur = a
            for item in node[1]:
                s, t = self.build(item)
                self.eps[cur].append(s)
                cur = t
            return a, cur
        if kind == "alt":
            a, b = self.new(), self.new()
            for item in node[1]:
                s, t = self.build(item)
                self.eps[a].append(s)
                self.eps[t].append(b)
            return a, b
        _, sub, m, n = node
        a = self.new()
        cur = a
        for _ in range(m):
            s, t = self.build(sub)
            self.eps[cur].append(s)
            cur = t
        if n is None:  # a loop behind the mandatory copies
            s, t = self.build(sub)
            hub = self.new()
            self.eps[cur].append(hub)
            self.eps[hub].append(s)
            self.eps[t].append(hub)
            return a, hub
        end = self.new()
        for _ in range(n - m):  # optional copies, each of which may be skipped to the end
            self.eps[cur].append(end)
            s, t = self.build(sub)
            self.eps[cur].append(s)
            cur = t
        self.eps[cur].append(end)
        return a, end


def _bits(mask: int, cache: dict) -> list[int]:
    got = cache.get(mask)
    if got is None:
        got = cache[mask] = [b for b in range(256) if mask >> b & 1]
    return got


class ByteDFA:
    """A trimmed, minimal DFA over bytes: ``table`` uint16 [S, 256] (next state, 0xFFFF = none), ``accepting`` uint8 [S], ``start``."""

    def __init__(self, table: np.ndarray, accepting: np.ndarray, start: int):
        self.table = np.ascontiguousarray(table, dtype=np.uint16)
        self.accepting = np.ascontiguousarray(accepting, dtype=np.uint8)
        self.start = int(start)

    @property
    def n_states(self) -> int:
        return self.table.shape[0]

    def walk(self, state: int, data: bytes) -> int | None:
        """The state after feeding `data` from `state`; None once a byte has no transition."""
        t = self.table
        for b in data:
            state = int(t[state, b])
            if state == DEAD:
                return None
        return state

    def accepts(self, data: bytes) -> bool:
        s = self.walk(self.start, data)
        return s is not None and bool(self.accepting[s])

    def check_vocabulary(self, offsets: Sequence[int], data) -> None:
        """Raises ValueError, naming a state, if some non-accepting state (all states are reachable) has no token of the vocabulary
        that can be walked from it: a constrained slot in that state would have nothing to produce."""
        offsets = np.asarray(offsets, dtype=np.int64)
        data = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
        by_first: dict[int, list[bytes]] = {}
        for j in range(len(offsets) - 1):
            tok = data[offsets[j]:offsets[j + 1]]
            if tok:
                by_first.setdefault(tok[0], []).append(tok)
        for toks in by_first.values():
            toks.sort(key=len)
        for s in range(self.n_states):
            if self.accepting[s]:
                continue
            ok = False
            for b in np.nonzero(self.table[s] != DEAD)[0]:
                if any(self.walk(s, tok) is not None for tok in by_first.get(int(b), ())):
                    ok = True
                    break
            if not ok:
                raise ValueError(f"check_vocabulary: no token of the vocabulary can be produced in state {s} (not accepting)")


def compile_regex(pattern: str | bytes) -> ByteDFA:
    """The minimal trimmed byte-level DFA of `pattern` under full-match semantics (dialect and limitation: the module docstring)."""
    if isinstance(pattern, str):
        pattern = pattern.encode("utf-8")
    if not isinstance(pattern, (bytes, bytearray)):
        raise ValueError("compile_regex takes a str or bytes pattern")
    tree = _Parser(bytes(pattern)).parse()
    nfa = _NFA()
    entry, exit_ = nfa.build(tree)

    closure_cache: dict[int, frozenset] = {}

    def closure(states) -> frozenset:
        out, stack = set(states), list(states)
        while stack:
            for t in nfa.eps[stack.pop()]:
                if t not in out:
                    out.add(t)
                    stack.append(t)
        return frozenset(out)

    def closure1(state: int) -> frozenset:
        got = closure_cache.get(state)
        if got is None:
            got = closure_cache[state] = closure([state])
        return got

    # subset construction
    bit_cache: dict[int, list[int]] = {}
    start_set = closure1(entry)
    index = {start_set: 0}
    order = [start_set]
    rows: list[list[int]] = []
    k = 0
    while k < len(order):
        cur = order[k]
        k += 1
        per_byte: dict[int, set] = {}
        for s in cur:
            for mask, t in nfa.edges[s]:
                for b in _bits(mask, bit_cache):
                    per_byte.setdefault(b, set()).add(t)
        row = [-1] * 256
        seen_targets: dict[frozenset, int] = {}
        for b, targets in per_byte.items():
            key = frozenset(targets)
            idx = seen_targets.get(key)
            if idx is None:
                full = frozenset().union(*(closure1(t) for t in key))
                idx = index.get(full)
                if idx is None:
                    idx = index[full] = len(order)
                    order.append(full)
                    if len(order) > 4 * MAX_STATES:
                        raise ValueError("compile_regex: the automaton is too large")
                seen_targets[key] = idx
            row[b] = idx
        rows.append(row)
    n = len(order)
    table = np.asarray(rows, dtype=np.int64)
    acc = np.fromiter((exit_ in st for st in order), dtype=bool, count=n)

    # states that can reach acceptance (backwards over the transitions); everything else becomes "no transition"
    live = acc.copy()
    while True:
        reach = np.concatenate([live, [False]])[table]  # [-1] reads the appended False
        grown = live | reach.any(axis=1)
        if (grown == live).all():
            break
        live = grown
    if not live[0]:
        raise ValueError("compile_regex: the pattern matches nothing")
    table = np.where(np.concatenate([live, [False]])[table], table, -1)
    # keep the live states only (the start stays state 0); one sink stands for "no transition"
    keep = np.nonzero(live)[0]
    renum = np.full(n + 1, -1, dtype=np.int64)
    renum[keep] = np.arange(len(keep))
    table = renum[table[keep]]  # (-1 reads renum[n] = -1)
    acc = acc[keep]
    n = len(keep)
    live = np.ones(n, dtype=bool)

    # minimisation (Moore): refine the partition {accepting, not, sink} until the signatures stop splitting it
    sink = n
    t2 = np.concatenate([np.where(table < 0, sink, table), np.full((1, 256), sink, dtype=np.int64)])
    labels = np.concatenate([acc.astype(np.int64), [2]])
    count = len(np.unique(labels))
    while True:
        sig = np.concatenate([labels[:, None], labels[t2]], axis=1)
        _, new = np.unique(sig, axis=0, return_inverse=True)
        labels = new.reshape(-1).astype(np.int64)
        new_count = int(labels.max()) + 1
        if new_count == count:
            break
        count = new_count

    # renumber the live classes breadth-first from the start (state 0); the sink is dropped
    sink_label = int(labels[n])
    rep_of: dict[int, int] = {}
    for s in range(n):
        if live[s]:
            rep_of.setdefault(int(labels[s]), s)
    new_id = {int(labels[0]): 0}
    queue = [int(labels[0])]
    out_rows, out_acc = [], []
    qi = 0
    while qi < len(queue):
        lab = queue[qi]
        qi += 1
        s = rep_of[lab]
        row = np.full(256, DEAD, dtype=np.int64)
        for b in range(256):
            t = int(table[s, b])
            if t < 0:
                continue
            tl = int(labels[t])
            if tl == sink_label:
                continue
            if tl not in new_id:
                new_id[tl] = len(queue)
                queue.append(tl)
            row[b] = new_id[tl]
        out_rows.append(row)
        out_acc.append(1 if acc[s] else 0)
    if len(out_rows) > MAX_STATES:
        raise ValueError(f"compile_regex: {len(out_rows)} states, more than the engine's {MAX_STATES}")
    return ByteDFA(np.asarray(out_rows, dtype=np.uint16), np.asarray(out_acc, dtype=np.uint8), 0)


def escape(data: str | bytes) -> bytes:
    """`data` as a pattern that matches exactly it (every byte that is not an ASCII letter, digit or underscore as \\xHH)."""
    if isinstance(data, str):
        data = data.encode("utf-8")
    return b"".join(bytes([b]) if _WORD >> b & 1 else b"\\x%02x" % b for b in data)


def choice(strings: Iterable[str | bytes]) -> bytes:
    """The pattern of an enum: the alternation of the escaped literals."""
    parts = [escape(s) for s in strings]
    if not parts:
        raise ValueError("choice needs at least one string")
    return b"(?:" + b"|".join(parts) + b")"


def vocabulary_bytes_from_strings(tokens: Sequence[bytes]) -> tuple[np.ndarray, np.ndarray]:
    """(offsets int32 [V + 1], bytes uint8) of a list of V byte strings (token id = index)."""
    lens = np.fromiter((len(t) for t in tokens), dtype=np.int64, count=len(tokens))
    offsets = np.zeros(len(tokens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    if offsets[-1] >= 2**31:
        raise ValueError("vocabulary larger than 2 GiB")
    return offsets.astype(np.int32), np.frombuffer(b"".join(bytes(t) for t in tokens), dtype=np.uint8).copy()


def gpt2_unicode_to_byte() -> dict[str, int]:
    """The inverse of the GPT-2 byte <-> unicode table byte-level BPE vocabularies are written in."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, extra = {}, 0
    for b in range(256):
        if b in keep:
            table[chr(b)] = b
        else:
            table[chr(256 + extra)] = b
            extra += 1
    return table


def vocabulary_bytes(tokenizer, vocab_size: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(offsets, bytes) from a byte-level BPE tokenizer's ``get_vocab()``: every token string is mapped back through the GPT-2
    byte <-> unicode table.  Added / special tokens (``get_added_vocab()``), tokens that hold a character outside the table and ids no
    token has become empty strings: never allowed under a grammar.  ``vocab_size``: the model's (it may exceed the tokenizer's)."""
    vocab = tokenizer.get_vocab()
    added = set(getattr(tokenizer, "get_added_vocab", dict)().values())
    size = max(vocab.values()) + 1 if vocab else 0
    size = max(size, vocab_size or 0)
    inverse = gpt2_unicode_to_byte()
    tokens = [b""] * size
    for text, j in vocab.items():
        if j in added or j < 0:
            continue
        try:
            tokens[j] = bytes(inverse[ch] for ch in text)
        except KeyError:
            tokens[j] = b""
    return vocabulary_bytes_from_strings(tokens)


def tokenizer_eos_ids(tokenizer) -> list[int]:
    """The tokenizer's EOS ids (``eos_token_ids`` where it has several, else ``eos_token_id``), at most the engine's 8."""
    ids = getattr(tokenizer, "eos_token_ids", None)
    ids = list(ids) if ids else [tokenizer.eos_token_id]
    return sorted({int(t) for t in ids if t is not None})[:8]


def regex_grammar(engine, tokenizer, pattern: str | bytes, check: bool = True):
    """A Grammar for ``engine`` from a loaded byte-level BPE tokenizer: its vocabulary as bytes (padded to the model's vocabulary size),
    the pattern's DFA and the tokenizer's EOS ids.  ``check``: refuse a pattern some state of which no token can continue."""
    dfa = compile_regex(pattern)
    offsets, data = vocabulary_bytes(tokenizer, engine.vocab_size)
    if len(offsets) - 1 != engine.vocab_size:
        raise ValueError(f"the tokenizer has {len(offsets) - 1} ids, the model {engine.vocab_size}")
    if check:
        dfa.check_vocabulary(offsets, data)
    vocab = engine.make_vocab(offsets, data)
    return engine.make_grammar(dfa, tokenizer_eos_ids(tokenizer), vocab)
