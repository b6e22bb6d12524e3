"""Stop conditions of the decode engine (include/tinyllm_engine.h "Stop conditions"): the ids and byte strings that end a sequence.

A ``StopSet`` is a tl_stop: validated here (so that a bad argument is a ValueError before anything reaches the device), built and
uploaded once by the library, immutable and shareable between slots.  ``DecodeEngine.set_stop(slot, stop_set, max_new_tokens)`` arms a
slot with it; ``DecodeEngine.stop_state(slot)`` reads the slot's record as a ``StopState``."""

from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

MAX_STOP_IDS = 16       # TL_MAX_STOP_IDS
MAX_STOP_STRINGS = 16   # TL_MAX_STOP_STRINGS
MAX_STOP_BYTES = 1024   # TL_MAX_STOP_BYTES
REASONS = ("none", "id", "string", "length")  # TL_STOP_NONE, TL_STOP_ID, TL_STOP_STRING, TL_STOP_LENGTH


class StopState(NamedTuple):
    """tl_stop_state: ``reason`` (one of REASONS), ``index`` (which id / string), ``generated`` (tokens examined since arming, the
    stopping one included), ``context`` (the slot's context length), ``text_bytes`` (bytes of text since arming, the stopping token's
    included unless it is a stop id) and ``cut_bytes`` (the text bytes ahead of the matched string; == text_bytes otherwise)."""
    reason: str
    index: int
    generated: int
    context: int
    text_bytes: int
    cut_bytes: int

    @property
    def stopped(self) -> bool:
        return self.reason != "none"


def stop_args(ids=(), strings=(), vocab_size: int | None = None) -> tuple[list[int], list[bytes]]:
    """The checked arguments of a stop set: ids (ints, distinct, in [0, vocab_size) where that is known) and strings (``bytes``, or
    ``str`` -> UTF-8; non-empty, distinct, at most 1,024 bytes together).  ValueError / TypeError otherwise."""
    if isinstance(ids, (int,)) or isinstance(strings, (str, bytes, bytearray)):
        raise TypeError("stop ids and stop strings are sequences (a single string would be taken apart letter by letter)")
    out_ids = []
    for t in ids:
        if isinstance(t, bool) or not isinstance(t, int) and not hasattr(t, "__index__"):
            raise TypeError(f"stop id {t!r} is not an integer")
        t = int(t)
        if t < 0 or (vocab_size is not None and t >= vocab_size):
            raise ValueError(f"stop id {t} out of range")
        if t in out_ids:
            raise ValueError(f"stop id {t} appears twice")
        out_ids.append(t)
    out_strings = []
    for s in strings:
        if isinstance(s, str):
            s = s.encode("utf-8")
        elif isinstance(s, (bytes, bytearray, memoryview)):
            s = bytes(s)
        else:
            raise TypeError(f"stop string {s!r} is neither bytes nor str")
        if not s:
            raise ValueError("a stop string is empty")
        if s in out_strings:
            raise ValueError(f"stop string {s!r} appears twice")
        out_strings.append(s)
    if len(out_ids) > MAX_STOP_IDS:
        raise ValueError(f"at most {MAX_STOP_IDS} stop ids")
    if len(out_strings) > MAX_STOP_STRINGS:
        raise ValueError(f"at most {MAX_STOP_STRINGS} stop strings")
    if sum(len(s) for s in out_strings) > MAX_STOP_BYTES:
        raise ValueError(f"the stop strings hold more than {MAX_STOP_BYTES} bytes")
    if not out_ids and not out_strings:
        raise ValueError("a stop set needs an id or a string (a budget alone needs no set)")
    return out_ids, out_strings


class StopSet:
    """tl_stop over ``ids`` and ``strings`` (stop_args).  Strings need ``vocab``, a ``tiny_llm_hip.engine.Vocab`` of the engine's
    vocabulary; a set of ids needs none, but a slot's text is counted in the set's vocabulary: without one text_bytes stays 0.  Keep it (and its Vocab) alive while a slot is armed with it."""

    def __init__(self, ids: Sequence[int] = (), strings: Sequence[bytes | str] = (), vocab=None, vocab_size: int | None = None):
        size = vocab.size if vocab is not None else vocab_size
        self.ids, self.strings = stop_args(ids, strings, size)
        if self.strings and vocab is None:
            raise ValueError("StopSet: stop strings need a Vocab (DecodeEngine.make_vocab)")
        self.vocab = vocab
        self._h = None
        from ._ext import tiny_llm_ext_hip as _ext

        data = b"".join(self.strings)
        offsets = [0]
        for s in self.strings:
            offsets.append(offsets[-1] + len(s))
        handle = ctypes.c_void_p()
        _ext.check(_ext.lib().tl_stop_create(
            vocab._h if vocab is not None else None, (ctypes.c_int32 * max(len(self.ids), 1))(*self.ids), len(self.ids),
            ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p) if data else None, (ctypes.c_int32 * len(offsets))(*offsets), len(self.strings), None,
            ctypes.byref(handle)))
        self._h = handle

    def close(self) -> None:
        if getattr(self, "_h", None):
            from ._ext import tiny_llm_ext_hip as _ext

            _ext.lib().tl_stop_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cli_stop_set(engine, tokenizer, strings=(), ids=(), also_ids=()):
    """The StopSet of main.py's and batch_main.py's ``--stop STRING`` / ``--stop-id N`` (both repeatable) with the token byte strings
    it was made over, or (None, None) when neither flag is given.  The vocabulary comes from the loaded tokenizer
    (grammar.vocabulary_bytes).  ``also_ids``: ids that end a request anyway (the tokenizer's EOS, a grammar's), joined to the set."""
    if not strings and not ids:
        return None, None
    from .grammar import vocabulary_bytes

    offsets, data = vocabulary_bytes(tokenizer, engine.vocab_size)
    vocab = engine.make_vocab(offsets, data)
    every = list(dict.fromkeys([int(i) for i in ids] + [int(i) for i in also_ids if i is not None]))
    data = bytes(bytearray(data))
    return engine.make_stop_set(every, list(strings), vocab), [data[offsets[t]:offsets[t + 1]] for t in range(len(offsets) - 1)]


def cut_text(ids, token_bytes, strings=(), cut_bytes=None) -> str:
    """The text the token ``ids`` spell, as bytes, cut at ``cut_bytes`` (a stop record's) or, where that is unknown, ahead of the
    first stop string it holds."""
    raw = b"".join(token_bytes[t] for t in ids)
    if cut_bytes is None:
        found = [k for k in (raw.find(bytes(s, "utf-8") if isinstance(s, str) else s) for s in strings) if k >= 0]
        cut_bytes = min(found) if found else len(raw)
    return raw[:cut_bytes].decode("utf-8", "replace")


def request_stops(stop, n_prompts: int) -> list["StopSet | None"] | None:
    """The ``stop`` argument of batch_generate_ids: None, one StopSet for every request, or a sequence with one (or None) per request."""
    if stop is None:
        return None
    if isinstance(stop, StopSet):
        return [stop] * n_prompts
    stops = list(stop)
    if len(stops) != n_prompts or any(s is not None and not isinstance(s, StopSet) for s in stops):
        raise ValueError("stop: one StopSet, or a sequence with a StopSet or None per prompt")
    return stops
