"""The stop definition of include/tinyllm_engine.h ("Stop conditions") in plain Python: bytes.find over the accumulated text, no
automaton.  Shared by the CPU and GPU stop tests."""

NONE, ID, STRING, LENGTH = 0, 1, 2, 3


def stop_oracle(tokens, vocab_bytes, ids=(), strings=(), max_new_tokens=0):
    """Examine ``tokens`` (the tokens a slot commits from arming on) in order.  ``vocab_bytes[t]`` is token t's byte string (may be
    empty).  Returns (reason, index, generated, text_bytes, cut_bytes) at the first stop, or with reason NONE after the last token
    (cut_bytes == text_bytes then)."""
    ids = [int(i) for i in ids]
    strings = [bytes(s) for s in strings]
    text = b""
    generated = 0
    for t in tokens:
        generated += 1
        if t in ids:
            return ID, ids.index(t), generated, len(text), len(text)
        before = len(text)
        text += bytes(vocab_bytes[t])
        # the first byte of this token at which some stop string ends; there, the longest such string
        for j in range(before, len(text)):
            ending = [k for k, s in enumerate(strings) if j + 1 >= len(s) and text.find(s, j + 1 - len(s), j + 1) == j + 1 - len(s)]
            if ending:
                k = max(ending, key=lambda i: len(strings[i]))
                return STRING, k, generated, len(text), j + 1 - len(strings[k])
        if max_new_tokens > 0 and generated == max_new_tokens:
            return LENGTH, 0, generated, len(text), len(text)
    return NONE, 0, generated, len(text), len(text)
