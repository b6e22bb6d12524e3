"""CPU tier: the host loop of batched speculative decoding (tiny_llm_hip.engine.batch_speculative_generate_ids) against scripted engines,
and the C declaration / ctypes mirror of tl_engine_verify_batch.

The scripted engines are duck-typed stand-ins for DecodeEngine (the pattern of the _ScriptedModel tests in tests/test_host_logic_cpu.py):
the "model" is a deterministic function of the tokens a slot holds, the draft agrees with the target at a seeded share of the
positions.  Each keeps, per slot, the tokens in its cache, so the loop's bookkeeping is checked where it matters: at every verify_batch
call the draft must hold exactly what the target holds plus the tokens it proposed from."""

import ctypes
import pathlib
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT / "tiny-llm_amd", ROOT / "tiny-llm_amd" / "extensions_hip"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

VOCAB, EOS = 13, 0


def _mix(tokens, salt):
    return zlib.crc32(np.asarray(list(tokens)[-3:] + [len(tokens), salt], np.int64).tobytes())


def target_next(tokens, salt):
    return _mix(tokens, salt) % VOCAB


class ScriptedEngine:
    """begin / prefill / decode / read_tokens / set_token / rewind / verify_batch / release / max_batch over per-slot token lists."""

    def __init__(self, salt, max_batch, agree=1.0, draft=None):
        self.salt, self.max_batch, self.agree, self.draft = salt, max_batch, agree, draft
        self.ctx, self.pending, self.produced = {}, {}, {}
        self.begun = self.released = self.calls = 0
        self.verify_calls = []

    def next(self, tokens):
        want = target_next(tokens, self.salt)
        if self.agree >= 1.0 or (_mix(tokens, self.salt + 99) % 1000) < self.agree * 1000:
            return want
        return (want + 1 + _mix(tokens, 7) % (VOCAB - 1)) % VOCAB  # any other id

    def begin(self, slot):
        self.calls += 1
        assert 0 <= slot < self.max_batch and slot not in self.ctx, f"begin of slot {slot}"
        self.ctx[slot], self.produced[slot] = [], []
        self.begun += 1

    def release(self, slot):
        self.calls += 1
        assert slot in self.ctx, f"slot {slot} released twice (or never begun)"
        del self.ctx[slot]
        self.pending.pop(slot, None)
        self.released += 1

    def prefill(self, slot, tokens, *, chunk=None, want_logits=True):
        self.calls += 1
        self.ctx[slot].extend(tokens)
        if want_logits:
            self.pending[slot] = self.next(self.ctx[slot])
            self.produced[slot].append(self.pending[slot])

    def set_token(self, slot, token):
        self.calls += 1
        assert slot in self.ctx
        self.pending[slot] = int(token)

    def decode(self, steps, batch=None):
        self.calls += 1
        assert 1 <= batch <= self.max_batch and steps >= 1
        for slot in sorted(self.ctx):
            if slot >= batch:
                continue
            for _ in range(steps):
                self.ctx[slot].append(self.pending[slot])
                self.pending[slot] = self.next(self.ctx[slot])
                self.produced[slot].append(self.pending[slot])

    def read_tokens(self, slot, count):
        self.calls += 1
        assert len(self.produced[slot]) >= count
        return list(self.produced[slot][-count:])

    def rewind(self, slot, n):
        self.calls += 1
        assert 0 < n <= len(self.ctx[slot]), f"rewind of {n} tokens"
        del self.ctx[slot][-n:]

    def verify_batch(self, chunks, commit=False):
        self.calls += 1
        assert commit, "the loop lets the engine rewind and set the next input"
        chunks = [(s, list(t)) for s, t in chunks]
        assert len({s for s, _ in chunks}) == len(chunks)
        self.verify_calls.append(chunks)
        out = []
        for slot, toks in chunks:
            assert slot in self.ctx, f"slot {slot} is verified after it finished"
            if self.draft is not None and slot in self.draft.ctx:  # the draft consumed the pending token and all proposals but the last
                assert self.draft.ctx[slot] == self.ctx[slot] + toks[:-1], f"slot {slot}: the draft's cache is out of step"
            g = []
            for t in toks:
                self.ctx[slot].append(t)
                g.append(self.next(self.ctx[slot]))
            a = next((j for j in range(len(toks) - 1) if g[j] != toks[j + 1]), len(toks) - 1)
            if len(toks) - 1 - a:
                del self.ctx[slot][-(len(toks) - 1 - a):]
            self.pending[slot] = g[a]
            out.append(g[:a + 1])
        return out


def target_only(prompt, limit, salt, eos):
    tokens, out = list(prompt), []
    while len(out) < limit:
        tok = target_next(tokens, salt)
        if tok == eos:
            break
        out.append(tok)
        tokens.append(tok)
    return out


@pytest.mark.parametrize("k", [1, 2, 4, 7])
@pytest.mark.parametrize("seed", range(6))
def test_output_equals_target_only_decoding(seed, k):
    from tiny_llm_hip.engine import batch_speculative_generate_ids

    rng = np.random.default_rng(1000 * k + seed)
    n_prompts = int(rng.integers(1, 6))
    prompts = [[int(t) for t in rng.integers(1, VOCAB, size=int(rng.integers(1, 9)))] for _ in range(n_prompts)]
    limit = int(rng.integers(1, 30))
    agree = float(rng.choice([0.0, 0.3, 0.7, 0.95, 1.0]))
    max_batch = int(rng.integers(1, 4))  # fewer slots than prompts now and then: several waves
    salt = 17 + seed
    draft = ScriptedEngine(salt, max_batch + 1, agree=agree)
    target = ScriptedEngine(salt, max_batch, draft=draft)
    stats = {}
    got = batch_speculative_generate_ids(target, draft, prompts, limit, proposal_length=k, eos_token_id=EOS, stats=stats)
    want = [target_only(p, limit, salt, EOS) for p in prompts]
    assert got == want
    for call in target.verify_calls:
        assert all(1 <= len(toks) <= k + 1 for _, toks in call) and sum(len(toks) for _, toks in call) <= 64
        assert len(call) <= min(max_batch, 64 // (k + 1))
    for eng in (target, draft):
        assert eng.begun == eng.released == n_prompts and not eng.ctx, "every slot is released exactly once"
    assert stats["rounds"] == len(target.verify_calls) and stats["target_calls"] == n_prompts + stats["rounds"]
    assert stats["accepted"] <= stats["proposed"]
    if agree == 1.0 and stats["proposed"]:
        assert stats["accepted"] >= stats["proposed"] - n_prompts * k, "an agreeing draft is rejected only where a sequence ends"


def test_full_agreement_needs_few_rounds_and_per_prompt_limits_hold():
    from tiny_llm_hip.engine import batch_speculative_generate_ids

    draft, stats = ScriptedEngine(5, 4), {}
    target = ScriptedEngine(5, 4, draft=draft)
    prompts = [[1, 2, 3], [4, 5], [6]]
    got = batch_speculative_generate_ids(target, draft, prompts, [12, 0, 5], proposal_length=3, eos_token_id=None, stats=stats)
    assert got == [target_only(p, n, 5, None) for p, n in zip(prompts, (12, 0, 5))] and [len(g) for g in got] == [12, 0, 5]
    assert stats["rounds"] <= 3 and stats["accepted"] == stats["proposed"]
    assert target.begun == target.released == 2, "a prompt that may emit nothing takes no slot"


class _Untouchable:
    max_batch = 4

    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was used before the arguments were checked")


@pytest.mark.parametrize("kwargs,message", [
    (dict(prompts=[[1], []], max_new_tokens=4), "at least one token"),
    (dict(prompts=[[1]], max_new_tokens=-1), "non-negative"),
    (dict(prompts=[[1], [2]], max_new_tokens=[3]), "one per prompt"),
    (dict(prompts=[[1]], max_new_tokens=4, proposal_length=8), "proposal_length"),
    (dict(prompts=[[1]], max_new_tokens=4, proposal_length=True), "proposal_length"),
    (dict(prompts=[[1]], max_new_tokens=4, proposal_length=-1), "proposal_length"),
])
def test_argument_validation_happens_before_any_engine_call(kwargs, message):
    from tiny_llm_hip.engine import batch_speculative_generate_ids

    with pytest.raises(ValueError, match=message):
        batch_speculative_generate_ids(_Untouchable(), _Untouchable(), **kwargs)


def test_engine_errors_release_every_slot():
    from tiny_llm_hip.engine import batch_speculative_generate_ids

    draft = ScriptedEngine(5, 4)
    target = ScriptedEngine(5, 4, draft=draft)

    def boom(chunks, commit=False):
        raise RuntimeError("engine: KV page pool exhausted")

    target.verify_batch = boom
    with pytest.raises(RuntimeError, match="pool exhausted"):
        batch_speculative_generate_ids(target, draft, [[1, 2], [3]], 8, proposal_length=2)
    assert target.begun == target.released == 2 and draft.begun == draft.released == 2


@pytest.mark.parametrize("flags,message", [
    (["--sampler-temp", "0.8"], "does not combine with --sampler-temp"),
    (["--repetition-penalty", "1.2"], "does not combine with --repetition-penalty"),
    (["--regex", "a+"], "does not combine with --regex"),
    (["--stop", "END"], "does not combine with --stop"),
    (["--stop-id", "3"], "does not combine with --stop"),
    (["--lora", "some/dir"], "does not combine with --lora"),
    (["--sampler-temp", "0.8", "--lora", "some/dir"], "--sampler-top-k, --lora"),
    (["--proposal-length", "8"], "--proposal-length must be between 1 and 7"),
    (["--proposal-length", "0"], "--proposal-length must be between 1 and 7"),
])
def test_batch_cli_refuses_what_a_draft_model_does_not_combine_with(flags, message, capsys):
    """batch_main.py --draft-model: check_draft_flags' own message, before any checkpoint is read."""
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    import batch_main

    with pytest.raises(SystemExit):
        batch_main.main(["--model", "no/such/dir", "--draft-model", "no/such/draft"] + flags)
    assert message in capsys.readouterr().err


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_ctypes_mirrors_the_record(tmp_path):
    """gcc compiles a probe against the header (the pattern of tests/test_abi_layout_cpu.py): tl_verify_result has the ctypes size and
    offsets, and tl_engine_verify_batch the declared signature."""
    import tiny_llm_ext_hip as ext

    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    flat = re.sub(r"\s+", " ", header)
    assert ("int tl_engine_verify_batch(tl_engine *e, int n_seqs, const int *slots, const int32_t *tokens, const int *lens, int commit, "
            "tl_verify_result *out);") in flat
    assert "typedef struct tl_verify_result { int32_t count; int32_t ids[8]; } tl_verify_result;" in flat
    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", '#include "tinyllm_engine.h"',
        "int (*probe)(tl_engine *, int, const int *, const int32_t *, const int *, int, tl_verify_result *) = tl_engine_verify_batch;",
        "int main(void) {",
        '    printf("%zu %zu %zu %zu\\n", sizeof(tl_verify_result), offsetof(tl_verify_result, count), offsetof(tl_verify_result, ids),',
        "           sizeof(((tl_verify_result *)0)->ids));",
        "    return 0;", "}"]))
    obj = tmp_path / "probe.o"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(obj)], check=True)
    probe = tmp_path / "sizes.c"
    probe.write_text(src.read_text().replace("= tl_engine_verify_batch;", "= 0;"))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(probe), "-o", str(exe)], check=True)
    size, off_count, off_ids, ids_bytes = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    cls = ext.TlVerifyResult
    assert [n for n, *_ in cls._fields_] == ["count", "ids"]
    assert (ctypes.sizeof(cls), cls.count.offset, cls.ids.offset, cls.ids.size) == (size, off_count, off_ids, ids_bytes) == (36, 0, 4, 32)
    fn = ext.lib().tl_engine_verify_batch
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 7 and fn.argtypes[-1] == ctypes.POINTER(cls)
    for name in ("tl_verify_attention_rows", "tl_verify_accept_rows"):
        assert re.search(r"\bint %s\(" % name, header) and hasattr(ext.lib(), name)
