"""CPU tier of batched speculative sampling (include/tinyllm_engine.h "tl_engine_verify_batch_sampled"; csrc/verify_sample.h):
1. the point rule (tests/verify_sample_oracle.py), written from its definition, is the two-row rule of tests/spec_sample_oracle.py for a
   draft row peaked at the proposal under draft temperature 0 -- and how many of the shared rows the oracle flags ambiguous;
2. the property the feature rests on: whatever is proposed, the emitted id is distributed as the target's own samples;
3. the binding's agreement with the header;
4. the policy of lookup_generate_ids(sampling=) against a stand-in engine whose sampled verification is the oracle's;
5. the lookup_main parser."""
import ctypes
import pathlib
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import lookup_oracle as L
import sampling_oracle as S
import spec_sample_oracle as SS
import verify_sample_oracle as VS

ROOT = pathlib.Path(__file__).resolve().parents[1]

# rows the oracle flags ambiguous among VS.point_cases(V), measured on the CPU for exactly this construction
AMBIGUOUS = {1024: 1, 8200: 0, 151936: 0, 151941: 0}
ROWS = {1024: 216, 8200: 114, 151936: 114, 151941: 114}


# -- 1. the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SS.VOCABS)
def test_point_rule_is_the_two_row_rule_with_a_one_hot_draft(V):
    rows = ambiguous = accepted = rejected = 0
    for target, params, props in VS.point_cases(V):
        for x, seed, position in props:
            draft, dparams = VS.two_row_twin(target, x, params)
            want = SS.Pair(target, draft, params, dparams).verify(x, seed, position)
            got = VS.point_verify(target, x, params, seed, position)
            assert got == want, (V, params, x, seed, position, got, want)
            if x >= V:
                wp, _, _ = SS.weights(target, *params)  # the residual is p whole
                assert got[:2] == (0, SS.inverse_cdf(wp, SS.uniform(seed, position, SS.RESIDUAL_TAG))[0])
            rows += 1
            ambiguous += bool(got[2])
            accepted += got[0]
            rejected += 1 - got[0]
    print(f"V={V}: rows={rows} ambiguous={ambiguous} accepted={accepted} rejected={rejected}")
    assert rows == ROWS[V] and accepted >= 10 and rejected >= rows // 3  # both branches: the outside third always rejects
    assert ambiguous == AMBIGUOUS[V] and ambiguous <= 0.05 * rows  # (the GPU tier may skip ambiguous rows only below 5 %)


def test_bonus_and_one_hot_rows():
    target = SS.rows(1024, np.random.default_rng(3))["rand"]
    assert VS.point_verify(target, -1, (0.8, 20, 0.9), 4, 9)[:2] == (0, S.sample(target, 0.8, 20, 0.9, 4, 9)[0])
    g = int(np.argmax(target))
    assert VS.point_verify(target, g, (0.0, 0, 1.0), 1, 1) == (1, -1, False) and VS.point_verify(target, g + 1, (0.0, 0, 1.0), 1, 1) == (0, g, False)
    nan = np.full(1024, np.nan)
    assert VS.point_verify(nan, 0, (0.7, 0, 1.0), 1, 1) == (1, -1, False) and VS.point_verify(nan, 5, (0.7, 0, 1.0), 1, 1) == (0, 0, False)


def test_compose():
    tokens = [10, 11, 12, 13, 20, 30, 31]
    row0, lens = [0, 4, 5], [4, 1, 2]
    assert VS.compose(row0, lens, tokens, [1, 1, 1, 0, 0, 1, 0], [-1, -1, -1, 7, 8, -1, 9]) == [[11, 12, 13, 7], [8], [31, 9]]
    # proposals that "accept" behind the first rejection are ignored
    assert VS.compose(row0, lens, tokens, [1, 0, 1, 0, 0, 0, 0], [-1, 5, -1, 7, 8, 6, 9]) == [[11, 5], [8], [6]]
    assert VS.compose(row0, lens, tokens, [0, 1, 1, 0, 0, 0, 0], [4, -1, -1, 7, 8, 6, 9]) == [[4], [8], [6]]


# -- 2. the distribution --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", VS.DIST_MODES)
def test_the_emitted_id_is_distributed_as_the_target(mode):
    target = VS.distribution_target()
    wp, _, _ = SS.weights(target, *SS.DIST_PARAMS)
    p = wp / wp.sum()
    kept = int((p > 0).sum())
    assert kept == SS.DIST_PARAMS[1] == 16
    proposals = VS.distribution_proposals(target, mode)
    emitted, accepted = [], 0
    for seed, x in enumerate(proposals):
        accept, alt, _ = VS.point_verify(target, x, SS.DIST_PARAMS, seed, 5)
        emitted.append(x if accept else alt)
        accepted += accept
    g = SS.g_statistic(emitted, p)
    print(f"{mode}: G={g:.1f} accepted={accepted} of {len(proposals)}")
    assert g < 3 * kept, (mode, g)
    assert (accepted == 0) if mode == "outside" else (0 < accepted < len(proposals))


# -- 3. the binding -------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree(tmp_path):
    import tiny_llm_ext_hip as ext

    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        '#include "tinyllm_engine.h"',
        "int (*batch)(tl_engine *, int, const int *, const int32_t *, const int *, const void *, float, int, float, int, tl_verify_result *) ="
        " tl_engine_verify_batch_sampled;",
        "int (*propose)(tl_engine *, int, const int *, const int *, int, int, int, int32_t *, int *) = tl_engine_lookup_propose_sampled;",
        "int (*copy)(tl_engine *, int, int, void *) = tl_engine_copy_verify_logits;",
        "int (*rows)(const void *, const void *, int, int, const int *, const int *, const int *, const int32_t *, const float *, const int32_t *,"
        " const float *, const uint64_t *, float, int, float, int32_t *, int32_t *, tl_verify_result *, void *) = tl_verify_sample_rows;"]))
    obj = tmp_path / "probe.o"  # compiled only: a pointer of another type is an error (-Werror), the symbols live in the library
    subprocess.run(["gcc", "-std=c11", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(obj)], check=True)
    vp, i, f, pi, p32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32)
    res = ctypes.POINTER(ext.TlVerifyResult)
    assert ext._SIGNATURES["tl_engine_verify_batch_sampled"] == (i, [vp, i, pi, p32, pi, vp, f, i, f, i, res])
    assert ext._SIGNATURES["tl_engine_lookup_propose_sampled"] == ext._SIGNATURES["tl_engine_lookup_propose"] == (i, [vp, i, pi, pi, i, i, i, p32, pi])
    assert ext._SIGNATURES["tl_engine_copy_verify_logits"] == (i, [vp, i, i, vp])
    assert ext._SIGNATURES["tl_verify_sample_rows"] == (i, [vp, vp, i, i, pi, pi, pi, vp, vp, vp, vp, vp, f, i, f, vp, vp, vp, vp])
    for name in ("tl_engine_verify_batch_sampled", "tl_engine_lookup_propose_sampled", "tl_engine_copy_verify_logits", "tl_verify_sample_rows"):
        fn = getattr(ext._lib, name)
        assert fn.restype is i and list(fn.argtypes) == ext._SIGNATURES[name][1]


def test_python_arguments():
    import torch
    from tiny_llm_hip.engine import DecodeEngine

    eng = SimpleNamespace(_h=None, vocab_size=64)  # the checks stand ahead of the library call
    for chunks, kw, text in (([], {}, "at least one chunk"), ([(0, [])], {}, "between 1 and 8 tokens"), ([(0, [1] * 9)], {}, "between 1 and 8 tokens"),
                             ([(s, [1] * 8) for s in range(9)], {}, "at most 64 tokens"),
                             ([(0, [1, 2])], {"draft_rows": torch.zeros((2, 64))}, "draft_rows must be a contiguous bf16"),
                             ([(0, [1, 2])], {"draft_sampling": (-1.0, None, None)}, "temperature")):
        with pytest.raises(ValueError, match=text):
            DecodeEngine.verify_batch_sampled(eng, chunks, **kw)


# -- 4. the loop ----------------------------------------------------------------------------------------------------------------------
V_TOY = 128


class SampledStandIn:
    """An engine whose model is a function of the sequence -- a logits row -- with the calls lookup_generate_ids(sampling=) makes and the
    engine's own rules about them: sampling set before the slot is armed, armed before the prefill, one chunk per live slot, chunks that
    start with the pending token.  The sampler is tests/sampling_oracle.py's, the sampled verification tests/verify_sample_oracle.py's;
    the token drawn behind a sequence of n ids is drawn at position n."""

    def __init__(self, row, max_batch=4):
        self.row, self.max_batch = row, max_batch
        self.seq, self.pending, self.armed, self.produced, self.smp = {}, {}, set(), {}, {}
        self.calls, self.final = [], {}

    def begin(self, s):
        assert s not in self.seq and 0 <= s < self.max_batch
        self.seq[s], self.produced[s] = [], []

    def release(self, s):
        self.final.setdefault(s, []).append((list(self.seq[s]), self.pending.get(s)))
        del self.seq[s]
        self.pending.pop(s, None)
        self.armed.discard(s)
        self.smp.pop(s, None)

    def set_sampling(self, s, temperature=0.0, top_k=None, top_p=None, seed=0):
        assert self.seq[s] == [] and s not in self.armed, "sampling is set after begin, before set_lookup and the prefill"
        self.smp[s] = ((temperature, top_k or 0, 1.0 if top_p is None else top_p), seed)

    def set_lookup(self, s, on=True):
        assert self.seq[s] == [] and s in self.smp
        self.armed.add(s)

    def _draw(self, s):
        params, seed = self.smp[s]
        return S.sample(self.row(self.seq[s]), *params, seed, len(self.seq[s]))[0]

    def _produce(self, s):
        self.pending[s] = self._draw(s)
        self.produced[s].append(self.pending[s])

    def prefill(self, s, prompt):
        self.seq[s] += list(prompt)
        self._produce(s)

    def read_tokens(self, s, n):
        return self.produced[s][-n:]

    def lookup_propose(self, slots, max_lens, max_ngram, min_ngram, num_proposals, sampled=False):
        assert sampled, "the sampled loop asks for the sampled entry point"
        assert list(slots) == sorted(self.seq) and all(s in self.armed for s in slots), "one call over every live slot"
        assert len(max_lens) == len(slots) and all(1 <= m <= 8 for m in max_lens) and sum(max_lens) <= 64
        self.calls.append("propose")
        return [[self.pending[s]] + L.propose_ids(self.seq[s] + [self.pending[s]], max_ngram, min_ngram, num_proposals)[:m - 1]
                for s, m in zip(slots, max_lens)]

    def verify_batch(self, chunks, commit=False):
        raise AssertionError("the sampled loop never calls the greedy verification")

    def verify_batch_sampled(self, chunks, commit=False, draft_rows=None, draft_sampling=(0.0, None, None)):
        assert commit and draft_rows is None and [s for s, _ in chunks] == sorted(self.seq), "one committed point pass over every live slot"
        assert any(len(c) > 1 for _, c in chunks), "a round without a proposal is a decode step"
        self.calls.append("verify")
        out = []
        for s, chunk in chunks:
            assert chunk[0] == self.pending[s] and 1 <= len(chunk) <= 8
            params, seed = self.smp[s]
            ids = []
            for j, t in enumerate(chunk):  # (commit: the slot keeps the pending token and the accepted proposals)
                self.seq[s].append(t)
                x = chunk[j + 1] if j + 1 < len(chunk) else -1
                accept, alt, _ = VS.point_verify(self.row(self.seq[s]), x, params, seed, len(self.seq[s]))
                ids.append(x if accept else alt)
                if not accept:
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


def periodic_id(seq):  # the sequence repeats with period 5: every lookup hits
    return seq[-5] if len(seq) >= 5 else 100 + len(seq)


def make_row(peak, height):
    """A model: the row behind `seq` is noise that depends on the sequence's tail, with `height` added at peak(seq)."""
    def row(seq):
        rng = np.random.default_rng([len(seq)] + list(seq[-3:]))
        r = rng.standard_normal(V_TOY).astype(np.float32)
        r[peak(seq) % V_TOY] += height
        return SS.bf16(r)
    return row


def greedy(row, prompt, n, eos=None):
    seq, out = list(prompt), []
    while len(out) < n:
        t = int(np.argmax(row(seq)))
        if t == eos:
            break
        out.append(t)
        seq.append(t)
    return out


PROMPTS = [[1, 2, 3, 4, 5, 1, 2], [9, 8, 7], [5] * 6, [1, 2, 3, 4, 5, 6], [2, 4, 2, 4, 2]]
LIMITS = [20, 1, 0, 33, 7]


@pytest.mark.parametrize("k", [1, 4, 7])
def test_top_k_one_returns_the_greedy_continuation(k):
    from tiny_llm_hip.engine import lookup_generate_ids

    row = make_row(periodic_id, 6.0)
    eng, stats = SampledStandIn(row, max_batch=3), {}
    got = lookup_generate_ids(eng, PROMPTS, LIMITS, proposal_length=k, stats=stats, sampling={"temperature": 0.9, "top_k": 1}, base_seed=11)
    assert got == [greedy(row, p, n) for p, n in zip(PROMPTS, LIMITS)]
    assert eng.seq == {}, "every slot is released"
    assert stats["rounds"] == eng.calls.count("verify") > 0 and stats["steps"] == eng.calls.count("step")
    assert eng.calls.count("propose") == stats["rounds"] + stats["steps"], "one propose call per round"
    assert 0 < stats["accepted"] <= stats["proposed"]


def test_sampled_loop_emits_every_position_once():
    from tiny_llm_hip.engine import lookup_generate_ids

    row = make_row(periodic_id, 3.0)  # a peak the sampler follows most of the time: proposals are accepted and rejected
    params = {"temperature": 0.8, "top_k": 8, "top_p": 0.95}
    runs = []
    for _ in range(2):
        eng, stats = SampledStandIn(row, max_batch=3), {}
        got = lookup_generate_ids(eng, PROMPTS, LIMITS, proposal_length=4, stats=stats, sampling=params, base_seed=5)
        runs.append(got)
        assert [len(g) for g in got] == LIMITS and eng.seq == {}
        assert 0 < stats["accepted"] < stats["proposed"] and stats["rounds"] == eng.calls.count("verify")
        at = {0: 0, 1: 0, 2: 0}
        for idx, (prompt, out) in enumerate(zip(PROMPTS, got)):
            if LIMITS[idx] == 0:
                continue
            s = idx % 3
            seq, pending = eng.final[s][at[s]]
            at[s] += 1
            # what the slot held when it was released is the prompt and the ids emitted, position by position; the last id the
            # sequence may emit is its pending token, which costs no pass
            assert (seq + [pending])[:len(prompt) + len(out)] == prompt + out and len(seq) >= len(prompt) + len(out) - 1
        # every request draws from base_seed + its index unless it names a seed
        assert eng.calls.count("propose") == stats["rounds"] + stats["steps"]
    assert runs[0] == runs[1], "the same settings give the same ids"
    eng = SampledStandIn(row, max_batch=3)
    per_prompt = [dict(params, seed=5 + i) for i in range(len(PROMPTS))]
    assert lookup_generate_ids(eng, PROMPTS, LIMITS, proposal_length=4, sampling=per_prompt, base_seed=99) == runs[0]


def test_sampled_loop_without_proposals_is_the_plain_sampler():
    from tiny_llm_hip.engine import lookup_generate_ids

    row = make_row(lambda seq: (sum((i + 1) * t for i, t in enumerate(seq)) * 2654435761 + len(seq)) % 1000003, 2.0)
    params = (0.8, 8, 0.95)
    eng, stats = SampledStandIn(row), {}
    prompt = [1, 2, 3, 4, 5, 1, 2]
    got = lookup_generate_ids(eng, [prompt], 12, proposal_length=4, max_ngram=16, min_ngram=16, stats=stats,
                              sampling={"temperature": params[0], "top_k": params[1], "top_p": params[2], "seed": 3})
    seq, want = list(prompt), []
    for _ in range(12):
        want.append(S.sample(row(seq), *params, 3, len(seq))[0])
        seq.append(want[-1])
    assert got == [want] and stats["rounds"] == 0 and stats["proposed"] == 0 and stats["steps"] == 11


def test_sampled_loop_stops_before_the_eos():
    from tiny_llm_hip.engine import lookup_generate_ids

    def peak(seq):  # period 5, and the EOS (77) once the sequence holds 23 ids
        return 77 if len(seq) == 23 else periodic_id(seq)

    row = make_row(peak, 6.0)
    prompt = [1, 2, 3, 4, 5, 1, 2]
    want = greedy(row, prompt, 40, eos=77)
    assert len(want) == 16
    for k in (1, 4, 7):
        eng = SampledStandIn(row)
        got = lookup_generate_ids(eng, [prompt, prompt[:6]], 40, proposal_length=k, eos_token_id=77, sampling={"temperature": 0.5, "top_k": 1})
        assert got == [want, greedy(row, prompt[:6], 40, eos=77)] and eng.seq == {}
    # an EOS among the proposals: nothing is proposed behind it, and an accepted EOS ends the sequence without being emitted
    prompt = [1, 2, 77, 3, 4, 1, 2]
    row = make_row(periodic_id, 6.0)
    eng, stats = SampledStandIn(row), {}
    got = lookup_generate_ids(eng, [prompt], 40, proposal_length=7, eos_token_id=77, stats=stats, sampling={"temperature": 0.5, "top_k": 1})
    assert got == [greedy(row, prompt, 40, eos=77)] and stats["proposed"] <= 7


def test_sampling_takes_the_sampler_keys_only():
    from tiny_llm_hip.engine import lookup_generate_ids

    eng = SimpleNamespace(max_batch=4)
    for bad in ("min_p", "repetition_penalty", "mirostat_tau", "logit_bias", "lora"):
        with pytest.raises(ValueError, match=bad):
            lookup_generate_ids(eng, [[1, 2]], 4, sampling={"temperature": 0.8, bad: 0.5})
    with pytest.raises(ValueError, match="typical_p"):
        lookup_generate_ids(eng, [[1, 2], [3]], 4, sampling=[{"temperature": 0.8}, {"typical_p": 0.5}])
    with pytest.raises(ValueError, match="one dict per prompt"):
        lookup_generate_ids(eng, [[1, 2], [3]], 4, sampling=[{"temperature": 0.8}])
    with pytest.raises(ValueError):
        lookup_generate_ids(eng, [[1, 2]], 4, sampling={"temperature": -1.0})


# -- 5. the command line --------------------------------------------------------------------------------------------------------------
def test_the_cli_has_the_sampler_flags(capsys):
    import lookup_main

    args = lookup_main.build_parser().parse_args(["dir", "a prompt"])
    assert (args.sampler_temp, args.sampler_top_k, args.sampler_top_p, args.sampler_seed) == (0.0, None, None, 0)
    args = lookup_main.build_parser().parse_args(["dir", "--sampler-temp", "0.8", "--sampler-top-k", "40", "--sampler-top-p", "0.9", "--sampler-seed", "7"])
    assert (args.sampler_temp, args.sampler_top_k, args.sampler_top_p, args.sampler_seed) == (0.8, 40, 0.9, 7)
    with pytest.raises(SystemExit):
        lookup_main.main(["no-such-checkpoint", "--sampler-temp", "-1"])
    capsys.readouterr()
