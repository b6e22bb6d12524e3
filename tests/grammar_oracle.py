"""Plain-Python / numpy restatement of regex-constrained decoding as include/tinyllm_engine.h ("grammars") defines it: the walk of a
token's bytes through a byte-level DFA, the allowed set of a state, the advance of a slot's state, and the processed row
(tests/logit_processing_oracle.py's row, then the mask line).  It shares no code with tiny_llm_hip/grammar.py: an automaton is taken
as plain arrays (table [S, 256] with 0xFFFF = no transition, accepting [S], start), a vocabulary as a list of byte strings."""

import numpy as np

import logit_processing_oracle as P

END = -1
DEAD = None
NONE = 0xFFFF


class Grammar:
    def __init__(self, table, accepting, start, tokens, eos_ids):
        self.table = np.asarray(table).astype(np.int64).tolist()  # (lists: the walks below index it once per byte)
        self.accepting = [bool(a) for a in np.asarray(accepting).tolist()]
        self.start = int(start)
        self.tokens = [bytes(t) for t in tokens]
        self.eos = [int(t) for t in eos_ids]
        self._rows = None
        self._allowed = {}

    def walk(self, s, j):
        """Feed token j's bytes from state s: the state reached, DEAD if a step has no transition; an empty string is DEAD."""
        data = self.tokens[j]
        if not data:
            return DEAD
        for b in data:
            s = self.table[s][b]
            if s == NONE:
                return DEAD
        return s

    def advance(self, state, token):
        """The state after the slot fed `token` back."""
        if token in self.eos or state == END:
            return END
        s = self.walk(state, token)
        return END if s is DEAD else s

    def allowed(self, state):
        """bool [V]: the tokens the slot may produce in `state`."""
        got = self._allowed.get(state)
        if got is not None:
            return got
        V = len(self.tokens)
        ok = np.zeros(V, dtype=bool)
        if state == END:
            ok[self.eos] = True
        else:
            # token by token, byte by byte; tokens are grouped by their first byte only to skip those that die at once
            first = self.table[state]
            for j, data in enumerate(self.tokens):
                if data and first[data[0]] != NONE and self.walk(state, j) is not DEAD:
                    ok[j] = True
            ok[self.eos] = self.accepting[state]
        self._allowed[state] = ok
        return ok

    def alive(self, data, state=None):
        """The state after the bytes `data` from the start (or `state`); DEAD when they leave the language's prefixes."""
        s = self.start if state is None else state
        for b in data:
            s = self.table[s][b]
            if s == NONE:
                return DEAD
        return s


def mask_row(logits, grammar, state):
    """tl_grammar_mask_rows: the row itself where the token is allowed, -inf elsewhere (float32 array of bf16 values)."""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    return np.where(grammar.allowed(state), l, np.float32(-np.inf)).astype(np.float32)


def process(logits, prompt, count, repetition=1.0, presence=0.0, frequency=0.0, bias=None, grammar=None, state=None):
    """The processed row of a slot: the processing definition, then `if not allowed[j]: v = -inf`.  A slot with a grammar PROCESSES:
    with neutral parameters the row still goes through every line (v / 1, v - 0, v + 0.0: -0.0 comes out as +0.0)."""
    if grammar is None:
        return P.process(logits, prompt, count, repetition, presence, frequency, bias)
    if P.processes(repetition, presence, frequency, bias):
        v = P.process(logits, prompt, count, repetition, presence, frequency, bias)
    else:
        l = np.ascontiguousarray(logits, dtype=np.float32)
        with np.errstate(all="ignore"):
            v = P.bf16_round(((l - np.float32(0.0)).astype(np.float32) + np.float32(0.0)).astype(np.float32))
    return np.where(grammar.allowed(state), v, np.float32(-np.inf)).astype(np.float32)
