"""Plain-Python / numpy restatement of stack grammars as include/tinyllm_engine.h ("stack grammars") defines them: one byte of a
byte-level DFA with a bounded stack, the walk of a token's bytes, the allowed set of a configuration (with the rule for tokens of more
than 16 bytes), the advance of a slot's configuration, and the processed row (tests/logit_processing_oracle.py's row, then the mask
line).  It shares no code with tiny_llm_hip/grammar.py: an automaton is taken as plain arrays (table [S, 256] with 0xFFFF = no
transition, ops [S, 256], pop_table [P, 5], accepting [S], start), a vocabulary as a list of byte strings.

A configuration is a tuple (state, depth, stack): depth in 0 .. 32, stack an int with the symbol of level i (0 = bottom) in bits
2i, 2i + 1 and zero above bit 2 * depth."""

import numpy as np

import logit_processing_oracle as P

END = (-1, 0, 0)
DEAD = None
NONE = 0xFFFF
DEPTH = 32
LONG = 16
POP = 5


class StackGrammar:
    def __init__(self, table, ops, pop_table, accepting, start, tokens, eos_ids):
        self.table = np.asarray(table).astype(np.int64).tolist()
        self.ops = np.asarray(ops).astype(np.int64).tolist()
        self.pop_table = np.asarray(pop_table).astype(np.int64).reshape(-1, 5).tolist()
        self.accepting = [bool(a) for a in np.asarray(accepting).tolist()]
        self.start = (int(start), 0, 0)
        self.tokens = [bytes(t) for t in tokens]
        self.eos = [int(t) for t in eos_ids]
        self._allowed = {}
        self._long = {}

    def byte(self, cfg, b):
        """One byte b from (s, d, stack)."""
        s, d, stack = cfg
        t, op = self.table[s][b], self.ops[s][b]
        if t == NONE:
            return DEAD
        if op == 0:
            return (t, d, stack)
        if 1 <= op <= 4:  # push symbol op - 1
            if d == DEPTH:
                return DEAD
            return (t, d + 1, stack | (op - 1) << (2 * d))
        assert op == POP
        if d == 0:
            return DEAD
        d -= 1
        stack &= (1 << (2 * d)) - 1
        top = (stack >> (2 * (d - 1))) & 3 if d > 0 else 4
        s2 = self.pop_table[t][top]
        return DEAD if s2 == NONE else (s2, d, stack)

    def alive(self, data, cfg=None):
        """The configuration after the bytes `data` from the start (or `cfg`); DEAD when they leave the language's prefixes."""
        cfg = self.start if cfg is None else cfg
        for b in data:
            cfg = self.byte(cfg, b)
            if cfg is DEAD:
                return DEAD
        return cfg

    def walk(self, cfg, j):
        """Feed token j's bytes from cfg: the configuration reached or DEAD; an empty string is DEAD.  Any token length."""
        data = self.tokens[j]
        return self.alive(data, cfg) if data else DEAD

    def advance(self, cfg, token):
        """The configuration after the slot fed `token` back: the real stack, at any token length."""
        if token in self.eos or cfg == END:
            return END
        c = self.walk(cfg, token)
        return END if c is DEAD else c

    def long_depth(self, state, j):
        """The byte of (state, long token j): the largest depth of the token's walk from (state, empty stack), or DEAD where that walk
        dies (no transition, a pop below the starting level, a 33rd level)."""
        key = (state, j)
        if key not in self._long:
            cfg, m = (state, 0, 0), 0
            for b in self.tokens[j]:
                cfg = self.byte(cfg, b)
                if cfg is DEAD:
                    break
                m = max(m, cfg[1])
            self._long[key] = DEAD if cfg is DEAD else m
        return self._long[key]

    def allowed(self, cfg):
        """bool [V]: the tokens the slot may produce in `cfg`."""
        got = self._allowed.get(cfg)
        if got is not None:
            return got
        ok = np.zeros(len(self.tokens), dtype=bool)
        if cfg == END:
            ok[self.eos] = True
        else:
            state, depth, _ = cfg
            first = self.table[state]
            for j, data in enumerate(self.tokens):
                if not data or first[data[0]] == NONE:
                    continue
                if len(data) > LONG:
                    m = self.long_depth(state, j)
                    ok[j] = m is not DEAD and depth + m <= DEPTH
                else:
                    ok[j] = self.walk(cfg, j) is not DEAD
            ok[self.eos] = self.accepting[state]  # acceptance by final state
        self._allowed[cfg] = ok
        return ok


def mask_row(logits, grammar, cfg):
    """tl_grammar_mask_rows_stack: the row itself where the token is allowed, -inf elsewhere (float32 array of bf16 values)."""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    return np.where(grammar.allowed(cfg), l, np.float32(-np.inf)).astype(np.float32)


def process(logits, prompt, count, repetition=1.0, presence=0.0, frequency=0.0, bias=None, grammar=None, cfg=None):
    """The processed row of a slot with a stack grammar: the processing definition, then `if not allowed[j]: v = -inf`.  The slot
    PROCESSES: with neutral parameters the row still goes through every line (v / 1, v - 0, v + 0.0: -0.0 comes out as +0.0)."""
    if grammar is None:
        return P.process(logits, prompt, count, repetition, presence, frequency, bias)
    if P.processes(repetition, presence, frequency, bias):
        v = P.process(logits, prompt, count, repetition, presence, frequency, bias)
    else:
        l = np.ascontiguousarray(logits, dtype=np.float32)
        with np.errstate(all="ignore"):
            v = P.bf16_round(((l - np.float32(0.0)).astype(np.float32) + np.float32(0.0)).astype(np.float32))
    return np.where(grammar.allowed(cfg), v, np.float32(-np.inf)).astype(np.float32)
