"""CPU tier of prompt-lookup speculative decoding (csrc/lookup.h, include/tinyllm_engine.h "Prompt lookup"):
1. the proposal rule (tests/lookup_oracle.py) on constructed rows;
2. the host half of the history's accounting (csrc/slot_settings.h) against a model of the device, under AddressSanitizer and UBSan;
3. the binding's argument checks and its agreement with the header;
4. the policy of lookup_generate_ids against a stand-in engine."""
import ctypes
import pathlib
import subprocess
from types import SimpleNamespace

import pytest

import lookup_oracle as L

ROOT = pathlib.Path(__file__).resolve().parents[1]


# -- 1. the rule ----------------------------------------------------------------------------------------------------------------------
def test_longest_match_wins():
    #    0  1  2  3  4  5  6  7  8  9
    T = [7, 1, 2, 3, 9, 2, 3, 8, 2, 3]
    assert L.choose(T, 0, 9, 3, 1, 3) == (6, 2, 3)  # (2 3) matches at 3 and at 6 with raw 2; K = 3: both have 3 ids to give, ...
    assert L.propose(T, 0, 9, 3, 1, 3) == [8, 2, 3]  # ... 6 is the more recent, and its continuation runs into the end
    assert L.choose(T, 0, 9, 3, 1, 4) == (3, 2, 4) and L.propose(T, 0, 9, 3, 1, 4) == [9, 2, 3, 8]  # K = 4: only 3 has four to give
    T = [1, 2, 3, 4, 0, 9, 3, 5, 0, 1, 2, 3]
    assert L.choose(T, 0, 11, 3, 1, 2) == (2, 3, 2) and L.propose(T, 0, 11, 3, 1, 2) == [4, 0]  # raw 3 at 2 beats raw 1 at 6
    assert L.choose(T, 0, 11, 1, 1, 2) == (6, 1, 2)  # N = 1: every candidate has raw 1, the most recent wins


def test_ties_in_raw_are_decided_by_avail_and_then_by_recency():
    a, b, c = 5, 6, 7
    T = [a, b, c, a, b, c, a, b, c]
    # candidates 2 and 5 (T[i] == c).  raw: at 2 min(N, 3) = 3, at 5 three as well.  avail(2) = min(K, 6), avail(5) = min(K, 3)
    assert L.choose(T, 0, 8, 3, 1, 3) == (5, 3, 3)  # K = 3: avail ties, the more recent wins
    assert L.choose(T, 0, 8, 3, 1, 4) == (2, 3, 4)  # K = 4: position 2 has more continuation ids
    assert L.propose(T, 0, 8, 3, 1, 4) == [a, b, c, a]
    assert L.choose(T, 0, 8, 16, 1, 3) == (5, 6, 3)  # N = 16: raw(5) = 6 (it reaches back to the start), raw(2) = 3
    assert L.choose(T, 0, 8, 16, 1, 7) == (5, 6, 3)  # raw decides before avail does


def test_start_and_end_bound_what_is_read():
    T = [1, 2, 3, 1, 2, 9, 1, 2, 3, 3, 3]
    assert L.propose(T, 0, 7, 2, 1, 3) == [9, 1, 2]  # (1 2) at 4 beats (1 2) at 1 by recency; T[8 ..] lies behind the end
    assert L.propose(T, 3, 7, 2, 1, 3) == [9, 1, 2]
    assert L.propose(T, 5, 7, 2, 1, 4) == []  # the earlier 2s lie before the start
    assert L.choose(T, 4, 7, 2, 1, 4) == (4, 1, 3)  # a match that reaches exactly to the start: raw is capped at i - s0 + 1 = 1
    assert L.choose(T, 3, 7, 2, 2, 4) == (4, 2, 3) and L.choose(T, 4, 7, 2, 2, 4) is None  # min_ngram == N
    assert L.propose(T, 7, 7) == [] and L.propose(T, 8, 7) == []  # one id, no id
    assert L.propose([4, 4], 0, 1, 3, 1, 7) == [4]  # the continuation is the last id itself
    assert L.propose_ids([3, 1, 2, 3, 1], 3, 1, 4) == [2, 3, 1] and L.propose_ids([3, 1, 2, 3, 1], 3, 1, 4, start=2) == []


def test_the_oracle_refuses_parameters_out_of_range():
    for bad in ((0, 1, 4), (17, 1, 4), (3, 0, 4), (3, 4, 4), (3, 1, 0), (3, 1, 8)):
        with pytest.raises(ValueError):
            L.propose([1, 2, 1], 0, 2, *bad)


# -- 2. the accounting ----------------------------------------------------------------------------------------------------------------
def test_the_history_accounting_under_sanitizers(tmp_path):
    """tests/lookup_history_check.cpp: arming, recording, decode calls that outrun the ring, set_token, rewind, fork, move and release
    through csrc/slot_settings.h against a model of ring, history row and truth, as its own process"""
    exe = tmp_path / "lookup_history_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    str(ROOT / "tiny-llm_amd" / "csrc"), str(ROOT / "tests" / "lookup_history_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert done.stdout.strip().splitlines()[-1].startswith("ok checks="), done.stdout[-500:]
    seen = [line for line in done.stdout.splitlines() if line.startswith("refusal: ")]
    assert len(seen) == 3 and "engine_set_lookup: this engine holds no history rows" in seen[0] and "engine_beam" in seen[2]


# -- 3. the binding -------------------------------------------------------------------------------------------------------------------
def test_python_arguments():
    import tiny_llm_ext_hip as ext
    import torch
    from tiny_llm_hip.engine import DecodeEngine, lookup_generate_ids

    assert ext.lookup_params(3, 1, 4) == (3, 1, 4) and ext.lookup_params(16, 16, 7) == (16, 16, 7)
    for bad, text in (((0, 1, 4), "max_ngram must be 1"), ((17, 1, 4), "max_ngram must be 1"), ((3, 0, 4), "min_ngram must be 1"),
                      ((3, 4, 4), "min_ngram must be 1"), ((3, 1, 0), "num_proposals must be 1"), ((3, 1, 8), "num_proposals must be 1"),
                      ((3.0, 1, 4), "max_ngram must be an int"), ((3, True, 4), "min_ngram must be an int")):
        with pytest.raises(ValueError, match=text):
            ext.lookup_params(*bad)
    with pytest.raises(ValueError, match="int32 tensor on the GPU"):
        ext.lookup_rows(torch.zeros((2, 8), dtype=torch.int32), 0, 7)
    with pytest.raises(ValueError, match="int32 tensor on the GPU"):
        ext.lookup_rows([[1, 2, 1]], 0, 2)

    eng = SimpleNamespace(_h=None)  # the checks stand ahead of the library call
    for slots, kw, text in (([], {}, "between 1 and 64 slots"), (list(range(65)), {}, "between 1 and 64 slots"),
                            ([0, 1], {"max_lens": [2]}, "one value in 1 .. 8 per slot"), ([0], {"max_lens": [9]}, "one value in 1 .. 8 per slot"),
                            ([0], {"max_lens": [0]}, "one value in 1 .. 8 per slot"), (list(range(9)), {}, "need max_lens"),
                            (list(range(9)), {"max_lens": [8] * 9}, "at most 64 tokens"), ([0], {"max_ngram": 17}, "max_ngram must be 1"),
                            ([0], {"num_proposals": 8}, "num_proposals must be 1")):
        with pytest.raises(ValueError, match=text.replace("..", r"\.\.")):
            DecodeEngine.lookup_propose(eng, slots, **kw)
    for kw, text in (({"proposal_length": 0}, "proposal_length"), ({"proposal_length": 8}, "proposal_length"), ({"max_ngram": 0}, "max_ngram"),
                     ({"min_ngram": 4}, "min_ngram"), ({"max_new_tokens": -1}, "max_new_tokens")):
        args = {"max_new_tokens": 4, **kw}
        with pytest.raises(ValueError, match=text):
            lookup_generate_ids(SimpleNamespace(max_batch=4), [[1, 2]], **args)
    with pytest.raises(ValueError, match="at least one token"):
        lookup_generate_ids(SimpleNamespace(max_batch=4), [[]], 4)


def test_header_and_ctypes_agree(tmp_path):
    import tiny_llm_ext_hip as ext

    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        '#include "tinyllm_engine.h"',
        "int (*set_lookup)(tl_engine *, int, int) = tl_engine_set_lookup;",
        "int (*propose)(tl_engine *, int, const int *, const int *, int, int, int, int32_t *, int *) = tl_engine_lookup_propose;",
        "int (*state)(const tl_engine *, int, int *, int *, int *) = tl_engine_lookup_state;",
        "int (*rows)(const int32_t *, int, int, const int32_t *, const int32_t *, int, int, int, int32_t *, int32_t *, int32_t *, void *) = tl_lookup_rows;",
        "int ngram[TL_LOOKUP_MAX_NGRAM == 16 ? 1 : -1], proposals[TL_LOOKUP_MAX_PROPOSALS == 7 ? 1 : -1];"]))
    obj = tmp_path / "probe.o"  # compiled only: a pointer of another type is an error (-Werror), the symbols live in the library
    subprocess.run(["gcc", "-std=c11", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert (ext.TL_LOOKUP_MAX_NGRAM, ext.TL_LOOKUP_MAX_PROPOSALS) == (L.MAX_NGRAM, L.MAX_PROPOSALS) == (16, 7)
    vp, i, pi, p32 = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32)
    assert ext._SIGNATURES["tl_engine_set_lookup"] == (i, [vp, i, i])
    assert ext._SIGNATURES["tl_engine_lookup_propose"] == (i, [vp, i, pi, pi, i, i, i, p32, pi])
    assert ext._SIGNATURES["tl_engine_lookup_state"] == (i, [vp, i, pi, pi, pi])
    assert ext._SIGNATURES["tl_lookup_rows"] == (i, [vp, i, i, vp, vp, i, i, i, vp, vp, vp, vp])
    for name in ("tl_engine_set_lookup", "tl_engine_lookup_propose", "tl_engine_lookup_state", "tl_lookup_rows"):
        fn = getattr(ext._lib, name)
        assert fn.restype is i and list(fn.argtypes) == ext._SIGNATURES[name][1]


# -- 4. the loop ----------------------------------------------------------------------------------------------------------------------
class StandIn:
    """An engine whose model is a function of the sequence, with the calls lookup_generate_ids makes and the engine's own rules about
    them: armed before the prefill, one chunk per live slot, chunks that start with the pending token, a step over live slots only."""

    def __init__(self, next_id, max_batch=4):
        self.next_id, self.max_batch = next_id, max_batch
        self.seq, self.pending, self.armed, self.produced = {}, {}, set(), {}
        self.calls = []

    def begin(self, s):
        assert s not in self.seq and 0 <= s < self.max_batch
        self.seq[s], self.produced[s] = [], []

    def release(self, s):
        del self.seq[s]
        self.pending.pop(s, None)
        self.armed.discard(s)

    def set_lookup(self, s, on=True):
        assert self.seq[s] == [], "armed before the prefill, so that the prompt is matched"
        self.armed.add(s)

    def _produce(self, s):
        self.pending[s] = self.next_id(self.seq[s])
        self.produced[s].append(self.pending[s])

    def prefill(self, s, prompt):
        self.seq[s] += list(prompt)
        self._produce(s)

    def read_tokens(self, s, n):
        return self.produced[s][-n:]

    def lookup_propose(self, slots, max_lens, max_ngram, min_ngram, num_proposals):
        assert list(slots) == sorted(self.seq) and all(s in self.armed for s in slots), "one call over every live slot"
        assert len(max_lens) == len(slots) and all(1 <= m <= 8 for m in max_lens) and sum(max_lens) <= 64
        self.calls.append("propose")
        return [[self.pending[s]] + L.propose_ids(self.seq[s] + [self.pending[s]], max_ngram, min_ngram, num_proposals)[:m - 1]
                for s, m in zip(slots, max_lens)]

    def verify_batch(self, chunks, commit=False):
        assert commit and [s for s, _ in chunks] == sorted(self.seq), "one committed pass over every live slot"
        assert any(len(c) > 1 for _, c in chunks), "a round without a proposal is a decode step"
        self.calls.append("verify")
        out = []
        for s, chunk in chunks:
            assert chunk[0] == self.pending[s] and 1 <= len(chunk) <= 8
            ids = []
            for j, t in enumerate(chunk):  # (commit: the slot keeps the pending token and the accepted proposals)
                self.seq[s].append(t)
                ids.append(self.next_id(self.seq[s]))
                if j + 1 == len(chunk) or chunk[j + 1] != ids[-1]:
                    break
            self.pending[s] = ids[-1]
            out.append(ids)
        return out

    def decode(self, steps, batch):
        assert steps == 1 and batch == max(self.seq) + 1
        self.calls.append("step")
        for s in sorted(self.seq):
            self.seq[s].append(self.pending[s])
            self._produce(s)


def greedy(next_id, prompt, n, eos=None):
    seq, out = list(prompt), []
    while len(out) < n:
        t = next_id(seq)
        if t == eos:
            break
        out.append(t)
        seq.append(t)
    return out


def periodic(seq):  # the sequence repeats with period 5: every lookup hits
    return seq[-5] if len(seq) >= 5 else 100 + len(seq)


def scrambled(seq):  # ids that hardly ever repeat
    return (sum((i + 1) * t for i, t in enumerate(seq)) * 2654435761 + len(seq)) % 1000003


def mixed(seq):  # repeats for a while, then leaves the loop
    return periodic(seq) if len(seq) % 17 else scrambled(seq)


@pytest.mark.parametrize("model", [periodic, scrambled, mixed], ids=["periodic", "scrambled", "mixed"])
@pytest.mark.parametrize("k", [1, 4, 7])
def test_the_loop_returns_the_greedy_continuation(model, k):
    from tiny_llm_hip.engine import lookup_generate_ids

    prompts = [[1, 2, 3, 4, 5, 1, 2], [9, 8, 7], [5] * 6, [1, 2, 3, 4, 5, 6], [2, 4, 2, 4, 2]]
    limits = [20, 1, 0, 33, 7]
    eng, stats = StandIn(model, max_batch=3), {}
    got = lookup_generate_ids(eng, prompts, limits, proposal_length=k, max_ngram=3, min_ngram=1, stats=stats)
    assert got == [greedy(model, p, n) for p, n in zip(prompts, limits)]
    assert eng.seq == {}, "every slot is released"
    assert stats["rounds"] == eng.calls.count("verify") and stats["steps"] == eng.calls.count("step")
    assert eng.calls.count("propose") == stats["rounds"] + stats["steps"], "one propose call per round"
    assert 0 <= stats["accepted"] <= stats["proposed"]
    if model is periodic:
        # (a period that holds an id twice, as 2 4 2 4 2 does, can mislead a 3-gram: not every proposal is accepted)
        assert stats["accepted"] * 2 > stats["proposed"] > 0 and stats["rounds"] + stats["steps"] < sum(limits) / 1.5
    if model is scrambled:
        assert stats["rounds"] == 0 and stats["proposed"] == 0, "nothing repeats: decode steps only"


def test_the_loop_stops_before_the_eos():
    from tiny_llm_hip.engine import lookup_generate_ids

    def model(seq):  # period 5, and the EOS (77) once the sequence holds 23 ids
        return 77 if len(seq) == 23 else periodic(seq)

    prompt = [1, 2, 3, 4, 5, 1, 2]
    want = greedy(model, prompt, 40, eos=77)
    assert len(want) == 16
    for k in (1, 4, 7):
        eng = StandIn(model)
        assert lookup_generate_ids(eng, [prompt, prompt[:6]], 40, proposal_length=k, eos_token_id=77) == [want, greedy(model, prompt[:6], 40, eos=77)]
        assert eng.seq == {}
    # an EOS among the proposals: nothing is proposed behind it, and an accepted EOS ends the sequence without being emitted
    prompt = [1, 2, 77, 3, 4, 1, 2]
    eng, stats = StandIn(periodic), {}
    assert lookup_generate_ids(eng, [prompt], 40, proposal_length=7, eos_token_id=77, stats=stats) == [greedy(periodic, prompt, 40, eos=77)]
    assert stats["proposed"] <= 7


def test_the_cli_refuses_parameters_out_of_range(capsys):
    import lookup_main

    for flags in (["--proposal-length", "0"], ["--proposal-length", "8"], ["--max-ngram", "17"], ["--max-ngram", "0"], ["--min-ngram", "0"],
                  ["--max-ngram", "2", "--min-ngram", "3"]):
        with pytest.raises(SystemExit):
            lookup_main.main(["no-such-checkpoint"] + flags)
    args = lookup_main.build_parser().parse_args(["dir", "a prompt", "another"])
    assert (args.model, args.prompts, args.proposal_length, args.max_ngram, args.min_ngram) == ("dir", ["a prompt", "another"], 4, 3, 1)
    capsys.readouterr()
