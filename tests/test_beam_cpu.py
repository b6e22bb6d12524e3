"""CPU tier: beam search without a device (include/tinyllm_engine.h "Beam search").

* The search policy (tiny_llm_hip/beam.py: beam_search) against a third party: a tiny float32 ``Qwen3ForCausalLM`` on the CPU feeds
  it, the float64 oracle (tests/beam_oracle.py) selects, and ``transformers``' own ``generate(num_beams=B, num_return_sequences=B,
  ...)`` on the same model must return the same sequences, with scores within 1e-5.  Every step first asserts, on the oracle's
  scores, that the candidates it ranks -- the K kept and the first one dropped -- lie more than 1e-4 apart, so that a near-tie cannot
  hide behind the comparison.
* Bad arguments to tl_beam_rows, tl_engine_beam_select and tl_engine_beam_reorder are TL_ERR_INVALID through the built library.
* tests/beam_reorder_model_check.cpp, built with AddressSanitizer and UBSan for page sizes 1 .. 4 and run as its own process: random
  genealogies on SlotTable::beam_reorder, the code the engine runs."""

import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest
import torch

import beam_oracle as BO

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "beam_reorder_model_check.cpp"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tiny-llm_amd" / "csrc"),
         "-I", str(ROOT / "tests")]
TL_ERR_INVALID = -1
PROMPT = [5, 17, 42, 8, 99]
NEW = 12
GAP = 1e-4


@pytest.fixture(scope="module")
def tiny_model():
    """vocab 100, 2 layers; the head is drawn wide enough (sigma 0.5) for a peaked distribution.  The EOS ids are tokens the greedy
    continuation meets at its fifth and eighth step, so that hypotheses end on them before the length limit."""
    import transformers

    torch.manual_seed(0)
    cfg = transformers.Qwen3Config(vocab_size=100, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=1, head_dim=16, max_position_embeddings=64, tie_word_embeddings=False)
    model = transformers.Qwen3ForCausalLM(cfg).float().eval()
    with torch.no_grad():
        model.lm_head.weight.normal_(0.0, 0.5)
        model.model.embed_tokens.weight.normal_(0.0, 1.0)
        greedy = model.generate(torch.tensor([PROMPT]), do_sample=False, max_new_tokens=NEW, eos_token_id=None, pad_token_id=0)[0, len(PROMPT):].tolist()
    assert greedy[4] != greedy[7]
    return model, {1: [greedy[4]], 2: [greedy[4], greedy[7]]}


def policy_run(model, num_beams, length_penalty, early_stopping, eos):
    """beam_search over the CPU model with the oracle's selection; the smallest gap between adjacent ranked candidates of any step."""
    from tiny_llm_hip.beam import beam_search

    beams, gaps = [[list(PROMPT)]], []

    def select(scores, n_cand):
        with torch.no_grad():
            rows = model(torch.tensor(beams[0])).logits[:, -1].double().numpy()
        ranked = BO.beam_select(rows, scores, n_cand + 1)
        assert all(c[0] >= 0 for c in ranked)
        gaps.extend(a[2] - b[2] for a, b in zip(ranked, ranked[1:]))
        return ranked[:n_cand]

    def advance(parents, tokens):
        beams[0] = [beams[0][p] + [t] for p, t in zip(parents, tokens)]

    out = beam_search(select, advance, num_beams=num_beams, max_new_tokens=NEW, eos_ids=eos, length_penalty=length_penalty,
                      early_stopping=early_stopping)
    return out, min(gaps)


def generate_run(model, num_beams, length_penalty, early_stopping, eos):
    """transformers' answer: (generated ids padded with eos[0], scores).  One beam is generate's greedy search, which reports no
    sequence score: it is the sum of the chosen tokens' log-probabilities, up to the first EOS, over length ** length_penalty."""
    with torch.no_grad():
        o = model.generate(torch.tensor([PROMPT]), num_beams=num_beams, num_return_sequences=num_beams, do_sample=False,
                           length_penalty=length_penalty, early_stopping=early_stopping, eos_token_id=list(eos), pad_token_id=eos[0],
                           max_new_tokens=NEW, return_dict_in_generate=True, output_scores=True)
    seqs = o.sequences[:, len(PROMPT):].tolist()
    if num_beams > 1:
        return seqs, o.sequences_scores.tolist()
    n = next((i + 1 for i, t in enumerate(seqs[0]) if t in eos), len(seqs[0]))
    logprobs = [torch.log_softmax(o.scores[i][0].double(), -1)[seqs[0][i]].item() for i in range(n)]
    return seqs, [sum(logprobs) / n ** length_penalty]


@pytest.mark.parametrize("n_eos", [1, 2])
@pytest.mark.parametrize("early_stopping", [True, False, "never"])
@pytest.mark.parametrize("length_penalty", [0.6, 1.0, 2.0])
@pytest.mark.parametrize("num_beams", [1, 2, 4, 8])
def test_policy_matches_transformers_generate(built_libs, tiny_model, num_beams, length_penalty, early_stopping, n_eos):
    model, eos_sets = tiny_model
    eos = eos_sets[n_eos]
    mine, gap = policy_run(model, num_beams, length_penalty, early_stopping, eos)
    assert gap > GAP, gap  # (about the reference's own scores: no ranking decision of this case is a near-tie)
    seqs, scores = generate_run(model, num_beams, length_penalty, early_stopping, eos)
    assert len(mine) == len(seqs) == num_beams
    for (ids, score), theirs, their_score in zip(mine, seqs, scores):
        assert theirs[:len(ids)] == ids and all(t == eos[0] for t in theirs[len(ids):]), (ids, theirs)
        assert abs(score - their_score) < 1e-5, (score, their_score)
    assert all(a[1] >= b[1] for a, b in zip(mine, mine[1:]))  # best first


def test_some_hypothesis_ends_on_eos_before_the_length_limit(built_libs, tiny_model):
    model, eos_sets = tiny_model
    for n_eos in (1, 2):
        mine, _ = policy_run(model, 4, 1.0, False, eos_sets[n_eos])
        assert any(ids[-1] in eos_sets[n_eos] and len(ids) < NEW for ids, _ in mine), mine
        assert all(not set(ids[:-1]) & set(eos_sets[n_eos]) for ids, _ in mine)  # an EOS id ends a hypothesis, nothing follows it


def test_policy_arguments(built_libs):
    from tiny_llm_hip.beam import beam_candidates, beam_search

    assert [beam_candidates(b, e) for b, e in ((1, 0), (4, 1), (8, 2), (8, 3), (2, 15))] == [2, 8, 24, 32, 32]
    for beams, n_eos in ((0, 1), (9, 1), (True, 1), (8, 4), (3, 10)):
        with pytest.raises(ValueError):
            beam_candidates(beams, n_eos)
    with pytest.raises(ValueError):
        beam_search(None, None, num_beams=2, max_new_tokens=4, early_stopping="sometimes")
    with pytest.raises(ValueError):
        beam_search(None, None, num_beams=2, max_new_tokens=0)


def test_cli_beam_flags_exclude_what_beam_slots_cannot_do(capsys):
    import main as cli

    ap = cli.build_parser()
    ok = ap.parse_args(["--model", "m", "--num-beams", "4", "--length-penalty", "0.6", "--early-stopping", "--stop-id", "7"])
    cli.check_beam_flags(ap, ok)  # (no error)
    for extra, word in ((["--sampler-temp", "0.7"], "sampler"), (["--sampler-seed", "1"], "sampler"), (["--repetition-penalty", "1.1"], "penalty"),
                        (["--regex", "a+"], "--regex"), (["--json", "object"], "--json"), (["--draft-model", "d"], "--draft-model"),
                        (["--mirostat-tau", "3"], "sampler"), (["--stop", "x"], "--stop"), (["--logprobs", "2"], "--logprobs")):
        with pytest.raises(SystemExit):
            cli.check_beam_flags(ap, ap.parse_args(["--model", "m", "--num-beams", "2", *extra]))
        message = capsys.readouterr().err
        assert "--num-beams cannot be combined with" in message and word in message, message
    for argv in (["--num-beams", "0"], ["--num-beams", "9"], ["--length-penalty", "2"], ["--early-stopping"],
                 ["--num-beams", "8", "--stop-id", "1", "--stop-id", "2", "--stop-id", "3"]):
        with pytest.raises(SystemExit):
            cli.check_beam_flags(ap, ap.parse_args(["--model", "m", *argv]))


def test_oracle_orders_and_pads():
    rows = np.array([[0.0, 1.0, 1.0, np.nan], [2.0, -np.inf, 0.5, 0.5]])
    got = BO.beam_select(rows, [0.0, 0.0], 8)
    assert [c[:2] for c in got] == [(1, 0), (0, 1), (0, 2), (0, 0), (1, 2), (1, 3), (1, 1), (-1, -1)]
    assert got[6][2] == float("-inf") and got[7] == BO.EMPTY
    assert BO.beam_select(rows, [float("-inf"), 0.0], 2)[0][0] == 1 and BO.beam_select(rows[:1] * np.nan, [0.0], 2) == [BO.EMPTY] * 2
    assert BO.beam_select(np.array([[1.0, np.inf]]), [0.0], 1) == [BO.EMPTY]
    assert BO.reorder([[1], [2], None], 2, [1, 1, 0], [7, 8, 9]) == [[2, 7], [2, 8], [1, 9]]
    assert BO.reorder([[1], [2], [3]], 3, [2, 0], [7, 8]) == [[3, 7], [1, 8], None]
    assert BO.reorder_pages_needed([5, 8], [0, 0, 0, 1, 1], 4) == 2


def test_the_symbols_are_declared_exported_and_bound(built_libs):
    import tiny_llm_ext_hip as ext

    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    for name in ("tl_beam_rows", "tl_engine_beam_select", "tl_engine_beam_reorder"):
        assert re.search(r"\b%s\(" % name, header), name
        assert getattr(ext.lib(), name).argtypes is not None and name in ext._SIGNATURES, name
    assert ctypes.sizeof(ext.TlBeamCandidate) == 16 and [n for n, _ in ext.TlBeamCandidate._fields_] == ["parent", "token", "score", "logprob"]
    assert (ext.TL_MAX_BEAMS, ext.TL_MAX_BEAM_CANDIDATES) == (8, 32)
    assert re.search(r"#define TL_MAX_BEAMS 8\b", header) and re.search(r"#define TL_MAX_BEAM_CANDIDATES 32\b", header)


def test_beam_candidate_matches_the_c_layout(tmp_path, built_libs):
    import tiny_llm_ext_hip as ext
    from test_abi_layout_cpu import c_fields

    fields = c_fields((ROOT / "include" / "tinyllm_engine.h").read_text(), "tl_beam_candidate")
    assert fields == ["parent", "token", "score", "logprob"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tinyllm_engine.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(tl_beam_candidate));']
    lines += [f'    printf("{f} %zu\\n", offsetof(tl_beam_candidate, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    want = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    assert ctypes.sizeof(ext.TlBeamCandidate) == want.pop("size")
    for name, offset in want.items():
        assert getattr(ext.TlBeamCandidate, name).offset == offset, name


def test_bad_arguments_are_invalid(built_libs):
    """Every refusal below is decided on the host before anything is launched: no device is touched."""
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    # logits, rows, vocab, scores, n_cand, out (the addresses are never read)
    good = (4096, 4, 1000, 8192, 8, 12288)
    bad = [(None,) + good[1:], good[:3] + (None,) + good[4:], good[:5] + (None,), good[:1] + (0,) + good[2:], good[:1] + (9,) + good[2:],
           good[:2] + (0,) + good[3:], good[:2] + (524289,) + good[3:], good[:4] + (0,) + good[5:], good[:4] + (33,) + good[5:]]
    for args in bad:
        assert lib.tl_beam_rows(*args, None) == TL_ERR_INVALID, args
    assert b"beam_rows" in lib.tl_last_error()
    scores = (ctypes.c_float * 8)(*[0.0] * 8)
    out = (ext.TlBeamCandidate * 32)()
    out[0].parent = 77
    assert lib.tl_engine_beam_select(None, 0, 1, scores, 2, out) == TL_ERR_INVALID
    assert out[0].parent == 77  # nothing changed
    parents = (ctypes.c_int * 8)(*[0] * 8)
    tokens = (ctypes.c_int32 * 8)(*[1] * 8)
    assert lib.tl_engine_beam_reorder(None, 0, 1, 2, parents, tokens) == TL_ERR_INVALID
    assert b"engine_beam_reorder" in lib.tl_last_error()


@pytest.fixture(scope="module")
def model_checks(tmp_path_factory):
    out = {}
    for page_size in (1, 2, 3, 4):
        exe = tmp_path_factory.mktemp("beam") / f"beam_reorder_model_check_p{page_size}"
        subprocess.run([*FLAGS, f"-DBEAM_P={page_size}", str(DRIVER), "-o", str(exe)], check=True)
        out[page_size] = exe
    return out


@pytest.mark.parametrize("page_size", [1, 2, 3, 4])
def test_random_genealogies_keep_the_page_invariants(model_checks, page_size):
    lines = []
    for seed in ("12345", "7"):
        done = subprocess.run([str(model_checks[page_size]), "20000", seed], capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        line = done.stdout.strip()
        assert line.startswith(f"ok ops=20000 page_size={page_size} "), line
        counts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)\b", line)}
        # the walk exercises what it claims to: reorders of every shape, on slots in the wrong state, and the other operations between
        for key in ("reorders", "reorder_wrong_state", "fanouts", "shrinks", "permutations", "forks", "moves", "releases", "rewinds", "parks",
                    "step_refusals"):
            assert counts[key] >= 100, (key, line)
        if page_size > 1:  # (one-token pages have no partial tail: nothing to copy, nothing to refuse for)
            assert counts["copies"] >= 100 and counts["reorder_refusals"] >= 100, line
        lines.append(line)
    assert lines[0] != lines[1]  # the seed is read
