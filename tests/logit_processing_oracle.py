"""numpy restatement of the decode engine's logit processing (include/tinyllm_engine.h tl_engine_set_penalties / tl_engine_set_logit_bias,
csrc/logit_process.h).  Per element, in float32, one IEEE-754 single-precision operation per line (numpy's float32 array operations are
exactly that: no fused multiply-add, a correctly rounded division):

    v = float(l[j])
    if prompt[j] or count[j] > 0:  v = v / r  if v > 0 else  v * r
    v = v - (f * float(count[j]))
    if count[j] > 0:               v = v - p
    v = v + bias[j]
    out[j] = bf16 round to nearest even of v

`process` works on float32 arrays holding bf16 values; `bits` / `from_bits` convert to and from the 16-bit patterns, `pack_history` builds
the device's uint16 history (bit 15 = prompt, bits 0-14 = count saturated at 32,767)."""

import numpy as np

COUNT_MAX = 32767
MAX_LOGIT_BIAS = 1024


def bf16_round(v):
    """float32 -> the nearest bf16 value (ties to even) as float32; NaN stays NaN."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    out = (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32).copy()
    out[np.isnan(v)] = np.nan
    return out


def bits(v):
    """bf16 values held in float32 -> their uint16 patterns."""
    return (np.ascontiguousarray(v, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def pack_history(prompt, count):
    """uint16 per token: bit 15 = prompt flag, bits 0-14 = min(count, 32,767)."""
    c = np.minimum(np.asarray(count, dtype=np.int64), COUNT_MAX).astype(np.uint16)
    return c | (np.asarray(prompt, dtype=bool).astype(np.uint16) << 15)


def processes(repetition=1.0, presence=0.0, frequency=0.0, bias=None):
    return np.float32(repetition) != 1 or np.float32(presence) != 0 or np.float32(frequency) != 0 or bool(bias)


def process(logits, prompt, count, repetition=1.0, presence=0.0, frequency=0.0, bias=None):
    """The processed row (float32 array of bf16 values) of `logits` (bf16 values) under the slot's history -- prompt: bool per token,
    count: int per token -- and parameters; bias: {id: value} or None.  A row that does not process is returned unchanged."""
    l = np.ascontiguousarray(logits, dtype=np.float32)
    if not processes(repetition, presence, frequency, bias):
        return l.copy()
    V = l.size
    cnt = np.minimum(np.asarray(count, dtype=np.int64), COUNT_MAX)
    seen = np.asarray(prompt, dtype=bool) | (cnt > 0)
    r, p, f = np.float32(repetition), np.float32(presence), np.float32(frequency)
    b = np.zeros(V, dtype=np.float32)
    for k, val in (bias or {}).items():
        b[int(k)] = np.float32(val)
    with np.errstate(all="ignore"):
        v = l.copy()
        pos = v > 0
        v = np.where(seen, np.where(pos, v / r, v * r), v).astype(np.float32)
        fc = (f * cnt.astype(np.float32)).astype(np.float32)
        v = (v - fc).astype(np.float32)
        v = np.where(cnt > 0, v - p, v).astype(np.float32)
        v = (v + b).astype(np.float32)
    return bf16_round(v)


class History:
    """A slot's history kept on the host by the tests, by the header's rule: prompt tokens are marked when the slot consumes them,
    a produced token is counted when the slot feeds it back (at the start of the decode step that consumes it)."""

    def __init__(self, vocab):
        self.prompt = np.zeros(vocab, dtype=bool)
        self.count = np.zeros(vocab, dtype=np.int64)

    def consume_prompt(self, tokens):
        self.prompt[np.asarray(list(tokens), dtype=np.int64)] = True

    def feed(self, token):
        self.count[int(token)] += 1

    def copy(self):
        h = History(self.prompt.size)
        h.prompt, h.count = self.prompt.copy(), self.count.copy()
        return h
