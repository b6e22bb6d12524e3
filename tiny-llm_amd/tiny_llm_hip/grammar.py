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


# ---- stack grammars: JSON mode (include/tinyllm_engine.h "stack grammars") ------------------------------------------------------------
# Nested JSON is not regular.  A StackDFA is a byte-level DFA with a bounded stack of 2-bit symbols beside the state; the engine keeps
# the configuration (state, depth, stack) per slot on the device, as it keeps a regex grammar's state.

MAX_DEPTH = 32
OP_POP = 5
_EMPTY = 4  # pop_table column: the stack became empty


class StackDFA:
    """``table`` uint16 [S, 256] (0xFFFF = none; else the next state or, for a pop, a row of ``pop_table``), ``ops`` uint8 [S, 256]
    (0 none, 1 .. 4 push symbol op - 1, 5 pop), ``pop_table`` uint16 [P, 5] (the state after a pop by the new top 0 .. 3, column 4 =
    the stack became empty; 0xFFFF = dead), ``accepting`` uint8 [S], ``start``.  A configuration is (state, depth, stack): depth in
    0 .. 32, stack an int with the symbol of level i (0 = bottom) in bits 2i, 2i + 1."""

    def __init__(self, table, ops, pop_table, accepting, start: int):
        self.table = np.ascontiguousarray(table, dtype=np.uint16)
        self.ops = np.ascontiguousarray(ops, dtype=np.uint8)
        self.pop_table = np.ascontiguousarray(pop_table, dtype=np.uint16).reshape(-1, 5)
        self.accepting = np.ascontiguousarray(accepting, dtype=np.uint8)
        self.start = int(start)
        if self.table.ndim != 2 or self.table.shape[1] != 256 or self.ops.shape != self.table.shape or self.accepting.shape != (self.table.shape[0],):
            raise ValueError("StackDFA: table and ops must be [S, 256], accepting [S]")

    @property
    def n_states(self) -> int:
        return self.table.shape[0]

    @property
    def n_pop(self) -> int:
        return self.pop_table.shape[0]

    def walk(self, config, data: bytes):
        """The configuration after feeding `data` from `config`; None once a byte has no transition, pushes onto a full stack or pops
        an empty one."""
        state, depth, stack = config
        for b in data:
            t, op = int(self.table[state, b]), int(self.ops[state, b])
            if t == DEAD:
                return None
            if op == 0:
                state = t
            elif op < OP_POP:
                if depth == MAX_DEPTH:
                    return None
                stack |= (op - 1) << (2 * depth)
                depth += 1
                state = t
            else:
                if depth == 0:
                    return None
                depth -= 1
                stack &= (1 << (2 * depth)) - 1
                state = int(self.pop_table[t, (stack >> (2 * (depth - 1))) & 3 if depth else _EMPTY])
                if state == DEAD:
                    return None
        return state, depth, stack

    def accepts(self, data: bytes) -> bool:
        c = self.walk((self.start, 0, 0), data)
        return c is not None and bool(self.accepting[c[0]])

    def check_vocabulary(self, offsets: Sequence[int], data) -> None:
        """Raises ValueError, naming a state, if from some non-accepting state no token of the vocabulary can be walked whatever is
        on the stack (tried: the empty stack and every stack of one or two symbols)."""
        offsets = np.asarray(offsets, dtype=np.int64)
        data = bytes(data) if not isinstance(data, np.ndarray) else data.tobytes()
        by_first: dict[int, list[bytes]] = {}
        for j in range(len(offsets) - 1):
            tok = data[offsets[j]:offsets[j + 1]]
            if tok:
                by_first.setdefault(tok[0], []).append(tok)
        for toks in by_first.values():
            toks.sort(key=len)
        stacks = [(0, 0)] + [(1, a) for a in range(4)] + [(2, a | b << 2) for a in range(4) for b in range(4)]
        for s in range(self.n_states):
            if self.accepting[s]:
                continue
            firsts = [int(b) for b in np.nonzero(self.table[s] != DEAD)[0]]
            if not any(self.walk((s, d, st), tok) is not None for b in firsts for tok in by_first.get(b, ()) for d, st in stacks):
                raise ValueError(f"check_vocabulary: no token of the vocabulary can be produced in state {s} (not accepting)")


def compile_json(top: str = "object", whitespace: str = "compact", max_depth: int = MAX_DEPTH) -> StackDFA:
    """RFC 8259 JSON as a StackDFA.  ``top``: "value" (any JSON text) or "object" (the text must be an object).  ``whitespace``: "free"
    (RFC whitespace wherever the RFC has it) or "compact" (none, but at most one space after ``:`` and ``,`` -- what
    ``json.dumps`` writes with either pair of separators).  Strings are well-formed UTF-8 (no overlong forms, no surrogates, nothing
    above U+10FFFF) without raw bytes below 0x20; escapes are ``\\" \\\\ \\/ \\b \\f \\n \\r \\t \\uXXXX``.  Stack symbols: 0 = object,
    1 = array; the kind of the innermost container is part of the state, so an accepting state implies an empty stack.  Containers
    nest up to the engine's 32 levels (``max_depth`` must be 32: the bound is the device's stack, not the automaton's)."""
    if top not in ("object", "value") or whitespace not in ("compact", "free"):
        raise ValueError('compile_json: top is "object" or "value", whitespace "compact" or "free"')
    if max_depth != MAX_DEPTH:
        raise ValueError("compile_json: max_depth must be 32 (the depth of the engine's stack)")
    free = whitespace == "free"
    ws = b" \t\n\r" if free else b""
    names: dict[str, int] = {}
    table: list[list[int]] = []
    ops: list[list[int]] = []
    accepting: list[int] = []

    def state(name: str) -> int:
        if name not in names:
            names[name] = len(table)
            table.append([DEAD] * 256)
            ops.append([0] * 256)
            accepting.append(0)
        return names[name]

    def edge(src: str, byte_values, dst: str | int, op: int = 0) -> None:
        s, d = state(src), dst if isinstance(dst, int) else state(dst)
        for b in byte_values:
            assert table[s][b] == DEAD, (src, b)
            table[s][b], ops[s][b] = d, op

    digits, digits19, hexes = b"0123456789", b"123456789", b"0123456789abcdefABCDEF"

    def spaced(name: str) -> str:
        """the state entered after ':' or ',': `name` itself with free whitespace, else a state that also takes one space"""
        return name if free else name + ".sp"

    def after_value(src: str, ctx: str) -> None:
        edge(src, ws, "AV." + ctx)
        if ctx == "O":
            edge(src, b",", spaced("KX"))
            edge(src, b"}", 0, OP_POP)
        elif ctx == "A":
            edge(src, b",", spaced("V.A"))
            edge(src, b"]", 0, OP_POP)

    def value_start(src: str, ctx: str) -> None:
        edge(src, b'"', f"S.{ctx}")
        edge(src, b"-", f"NM.{ctx}")
        edge(src, b"0", f"NZ.{ctx}")
        edge(src, digits19, f"NI.{ctx}")
        for word in (b"true", b"false", b"null"):
            edge(src, word[:1], f"L.{ctx}.{word[:1].decode()}")
        edge(src, b"{", "O0", 1)
        edge(src, b"[", "A0", 2)

    def string(p: str, exit_: str) -> None:
        edge(p, [b for b in range(0x20, 0x80) if b not in b'"\\'], p)
        edge(p, b'"', exit_)
        edge(p, b"\\", p + ".esc")
        edge(p, range(0xC2, 0xE0), p + ".c1")
        edge(p, [0xE0], p + ".e0")
        edge(p, [b for b in range(0xE1, 0xF0) if b != 0xED], p + ".c2")
        edge(p, [0xED], p + ".ed")
        edge(p, [0xF0], p + ".f0")
        edge(p, range(0xF1, 0xF4), p + ".c3")
        edge(p, [0xF4], p + ".f4")
        edge(p + ".c1", range(0x80, 0xC0), p)
        edge(p + ".c2", range(0x80, 0xC0), p + ".c1")
        edge(p + ".e0", range(0xA0, 0xC0), p + ".c1")
        edge(p + ".ed", range(0x80, 0xA0), p + ".c1")
        edge(p + ".c3", range(0x80, 0xC0), p + ".c2")
        edge(p + ".f0", range(0x90, 0xC0), p + ".c2")
        edge(p + ".f4", range(0x80, 0x90), p + ".c2")
        edge(p + ".esc", b'"\\/bfnrt', p)
        edge(p + ".esc", b"u", p + ".h1")
        for k in (1, 2, 3):
            edge(f"{p}.h{k}", hexes, f"{p}.h{k + 1}")
        edge(p + ".h4", hexes, p)

    start = "V.T" if top == "value" else "START"
    state(start)
    if top == "value":
        edge("V.T", ws, "V.T")
        value_start("V.T", "T")
    else:
        edge("START", ws, "START")
        edge("START", b"{", "O0", 1)
    for ctx in ("T", "O", "A"):
        after_value("AV." + ctx, ctx)
        string("S." + ctx, "AV." + ctx)
        edge(f"NM.{ctx}", b"0", f"NZ.{ctx}")
        edge(f"NM.{ctx}", digits19, f"NI.{ctx}")
        edge(f"NI.{ctx}", digits, f"NI.{ctx}")
        for n in ("NZ", "NI"):
            edge(f"{n}.{ctx}", b".", f"NF0.{ctx}")
        edge(f"NF0.{ctx}", digits, f"NF.{ctx}")
        edge(f"NF.{ctx}", digits, f"NF.{ctx}")
        for n in ("NZ", "NI", "NF"):
            edge(f"{n}.{ctx}", b"eE", f"NE0.{ctx}")
        edge(f"NE0.{ctx}", b"+-", f"NE1.{ctx}")
        for n in ("NE0", "NE1", "NE"):
            edge(f"{n}.{ctx}", digits, f"NE.{ctx}")
        for n in ("NZ", "NI", "NF", "NE"):
            after_value(f"{n}.{ctx}", ctx)
        for word in (b"true", b"false", b"null"):
            for k in range(1, len(word)):
                edge(f"L.{ctx}.{word[:k].decode()}", word[k:k + 1], f"L.{ctx}.{word[:k + 1].decode()}" if k + 1 < len(word) else f"AV.{ctx}")
    for n in ("AV", "NZ", "NI", "NF", "NE"):
        accepting[state(n + ".T")] = 1
    # containers: O0 / A0 just opened; KX a key after ','; COL the ':' after a key; V.O / V.A a value after ':' / ','
    edge("O0", ws, "O0")
    edge("O0", b'"', "KS")
    edge("O0", b"}", 0, OP_POP)
    edge("KX", ws, "KX")
    edge("KX", b'"', "KS")
    string("KS", "COL")
    edge("COL", ws, "COL")
    edge("COL", b":", spaced("V.O"))
    edge("A0", ws, "A0")
    value_start("A0", "A")
    edge("A0", b"]", 0, OP_POP)
    for ctx in ("O", "A"):
        edge("V." + ctx, ws, "V." + ctx)
        value_start("V." + ctx, ctx)
    if not free:
        edge("KX.sp", b" ", "KX")
        edge("KX.sp", b'"', "KS")
        for ctx in ("O", "A"):
            edge(f"V.{ctx}.sp", b" ", "V." + ctx)
            value_start(f"V.{ctx}.sp", ctx)
    pop_table = [[names["AV.O"], names["AV.A"], DEAD, DEAD, names["AV.T"]]]
    # drop what cannot be reached from the start (top="object": the values of the top level)
    seen, todo = {names[start]}, [names[start]]
    while todo:
        s = todo.pop()
        for b in range(256):
            if table[s][b] == DEAD:
                continue
            for d in ([x for x in pop_table[table[s][b]] if x != DEAD] if ops[s][b] == OP_POP else [table[s][b]]):
                if d not in seen:
                    seen.add(d)
                    todo.append(d)
    order = sorted(seen)
    new = {s: i for i, s in enumerate(order)}
    out_table = np.full((len(order), 256), DEAD, dtype=np.uint16)
    out_ops = np.zeros((len(order), 256), dtype=np.uint8)
    for s in order:
        for b in range(256):
            if table[s][b] != DEAD:
                out_table[new[s], b] = table[s][b] if ops[s][b] == OP_POP else new[table[s][b]]
                out_ops[new[s], b] = ops[s][b]
    out_pop = np.asarray([[new.get(x, DEAD) if x != DEAD else DEAD for x in row] for row in pop_table], dtype=np.uint16)
    return StackDFA(out_table, out_ops, out_pop, np.asarray([accepting[s] for s in order], dtype=np.uint8), new[names[start]])


_SCHEMA_ANNOTATIONS = {"title", "description", "$schema", "$id", "default", "examples"}
_JSON_CHAR = b'(?:[^"\\\\\\x00-\\x1f]|\\\\(?:["\\\\/bfnrt]|u[0-9a-fA-F]{4}))'
_JSON_INT = b"-?(?:0|[1-9][0-9]*)"
_JSON_NUMBER = _JSON_INT + b"(?:\\.[0-9]+)?(?:[eE][+-]?[0-9]+)?"


def schema_regex(schema: dict) -> bytes:
    """A pattern (for compile_regex; also a valid ``re`` bytes pattern) of the COMPACT JSON texts -- ``json.dumps(x, separators=(",",
    ":"))`` -- that conform to a non-recursive JSON-Schema subset: ``type`` object (``properties`` in the given order, all of them
    required), string (``enum``, ``const``, ``maxLength``), integer, number, boolean, null, array (``items``, ``minItems``,
    ``maxItems``), ``anyOf``, ``enum`` / ``const`` of scalars, nested freely.  Any other keyword raises ValueError naming it."""
    import json

    if not isinstance(schema, dict):
        raise ValueError("schema_regex: a schema is a dict")

    def only(allowed):
        for key in schema:
            if key not in allowed and key not in _SCHEMA_ANNOTATIONS:
                raise ValueError(f"schema_regex: unsupported keyword {key!r}")

    def literal(value) -> bytes:
        if isinstance(value, (dict, list)):
            raise ValueError("schema_regex: unsupported keyword 'enum' / 'const' with a value that is not a scalar")
        return escape(json.dumps(value))

    if "anyOf" in schema:
        only({"anyOf"})
        return b"(?:" + b"|".join(schema_regex(s) for s in schema["anyOf"]) + b")"
    if "const" in schema:
        only({"const", "type"})
        return literal(schema["const"])
    if "enum" in schema:
        only({"enum", "type"})
        if not schema["enum"]:
            raise ValueError("schema_regex: unsupported keyword 'enum' without values")
        return b"(?:" + b"|".join(literal(v) for v in schema["enum"]) + b")"
    kind = schema.get("type")
    if kind is None:
        only(set())
        raise ValueError("schema_regex: a schema needs 'type', 'enum', 'const' or 'anyOf'")
    if kind == "string":
        only({"type", "maxLength"})
        return b'"' + _JSON_CHAR + (b"{0,%d}" % int(schema["maxLength"]) if "maxLength" in schema else b"*") + b'"'
    if kind in ("integer", "number", "boolean", "null"):
        only({"type"})
        return {"integer": _JSON_INT, "number": _JSON_NUMBER, "boolean": b"(?:true|false)", "null": b"null"}[kind]
    if kind == "array":
        only({"type", "items", "minItems", "maxItems"})
        if "items" not in schema:
            raise ValueError("schema_regex: unsupported keyword 'array' without 'items'")
        item, lo, hi = schema_regex(schema["items"]), int(schema.get("minItems", 0)), schema.get("maxItems")
        if hi is not None and (int(hi) < lo or int(hi) < 0):
            raise ValueError("schema_regex: unsupported keyword 'maxItems' below 'minItems'")
        if hi is not None and int(hi) == 0:
            return b"\\[\\]"
        more = b"(?:," + item + b")" + (b"{%d,}" % max(lo - 1, 0) if hi is None else b"{%d,%d}" % (max(lo - 1, 0), int(hi) - 1))
        return b"\\[" + (b"(?:" + item + more + b")?" if lo == 0 else item + more) + b"\\]"
    if kind == "object":
        only({"type", "properties", "required", "additionalProperties"})
        props = schema.get("properties", {})
        if "required" in schema and set(schema["required"]) != set(props):
            raise ValueError("schema_regex: unsupported keyword 'required' that does not list every property")
        if schema.get("additionalProperties", False) is not False:
            raise ValueError("schema_regex: unsupported keyword 'additionalProperties' other than false")
        return b"\\{" + b",".join(escape(json.dumps(k)) + b":" + schema_regex(v) for k, v in props.items()) + b"\\}"
    raise ValueError(f"schema_regex: unsupported keyword 'type': {kind!r}")


def json_grammar(engine, tokenizer, top: str = "object", whitespace: str = "compact", check: bool = True):
    """regex_grammar's companion for JSON mode: a Grammar for ``engine`` from a loaded byte-level BPE tokenizer and compile_json."""
    dfa = compile_json(top, whitespace)
    offsets, data = vocabulary_bytes(tokenizer, engine.vocab_size)
    if len(offsets) - 1 != engine.vocab_size:
        raise ValueError(f"the tokenizer has {len(offsets) - 1} ids, the model {engine.vocab_size}")
    if check:
        dfa.check_vocabulary(offsets, data)
    vocab = engine.make_vocab(offsets, data)
    return engine.make_grammar(dfa, tokenizer_eos_ids(tokenizer), vocab)


def cli_grammar(engine, tokenizer, regex=None, json_top=None, json_schema_file=None):
    """The Grammar of main.py's and batch_main.py's --regex PATTERN / --json object|value / --json-schema FILE (at most one of them), or
    None."""
    if json_top:
        return json_grammar(engine, tokenizer, top=json_top)
    if json_schema_file:
        import json

        with open(json_schema_file, encoding="utf-8") as f:
            return regex_grammar(engine, tokenizer, schema_regex(json.load(f)))
    return regex_grammar(engine, tokenizer, regex) if regex else None
