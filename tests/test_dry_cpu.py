"""CPU tier: DRY and the n-gram ban (include/tinyllm_engine.h "DRY and the n-gram ban") without a device -- the numpy restatement
(tests/dry_oracle.py) against transformers' NoRepeatNGramLogitsProcessor and against a literal transcription of text-generation-webui's
DRY loop, the setter's refusals (the record of csrc/slot_settings.h driven by tests/dry_settings_check.cpp under AddressSanitizer and
UBSan, and the Python layer's), the C ABI and the command line."""

import ctypes
import pathlib
import subprocess

import numpy as np
import pytest

import dry_oracle as D

ROOT = pathlib.Path(__file__).resolve().parents[1]


# -- 1. the n-gram ban is Hugging Face's ------------------------------------------------------------------------------------------
def _sequences(rng, vocab, lengths):
    """random and periodic sequences of the given lengths"""
    for n in lengths:
        yield rng.integers(0, vocab, n).tolist()
        period = int(rng.integers(1, 9))
        yield (rng.integers(0, vocab, period).tolist() * (n // period + 1))[:n]


@pytest.mark.parametrize("n", [2, 3, 5])
def test_ngram_ban_equals_transformers(n):
    import torch
    from transformers import NoRepeatNGramLogitsProcessor

    V = 50
    proc = NoRepeatNGramLogitsProcessor(n)
    rng = np.random.default_rng(n)
    checked = banned_total = 0
    for seq in _sequences(rng, V, range(1, 201)):
        scores = proc(torch.tensor([seq]), torch.zeros((1, V)))[0]
        want = set(torch.nonzero(torch.isinf(scores)).flatten().tolist())
        got = D.banned(seq, 0, n)
        assert got == want, (n, len(seq), sorted(got), sorted(want))
        row = D.apply(D.bits(np.zeros(V, np.float32)), seq, ngram=n)
        assert set(np.flatnonzero(row == D.NEG_INF).tolist()) == want and (np.delete(row, sorted(want)) == 0).all()
        checked += 1
        banned_total += len(want)
    assert checked == 400 and banned_total > 150  # (a periodic sequence alone bans one token per call: the comparison is not empty)


# -- 2. DRY is text-generation-webui's loop ---------------------------------------------------------------------------------------
def webui_match_lengths(input_ids, _range, sequence_breakers):
    """modules/sampler_hijack.py DRYLogitsProcessor.__call__ of text-generation-webui for one row, in plain Python: token -> match
    length (no cap on the length)."""
    row = list(input_ids)
    if _range > 0:
        row = row[-_range:]
    last_token = row[-1]
    if last_token in sequence_breakers:
        return {}
    match_indices = [k for k in range(len(row) - 1) if row[k] == last_token]
    match_lengths = {}
    for i in match_indices:
        next_token = row[i + 1]
        if next_token in sequence_breakers:
            continue
        match_length = 1
        while True:
            j = i - match_length
            if j < 0:
                break
            previous_token = row[-(match_length + 1)]
            if row[j] != previous_token:
                break
            if previous_token in sequence_breakers:
                break
            match_length += 1
        if next_token in match_lengths:
            match_lengths[next_token] = max(match_length, match_lengths[next_token])
        else:
            match_lengths[next_token] = match_length
    return match_lengths


def test_dry_equals_the_webui_loop():
    rng = np.random.default_rng(12)
    V = 12
    cases = long_matches = entries = 0
    for n in range(1, 301):
        for _ in range(2):
            seq = rng.integers(0, V, n).tolist()
            if rng.random() < 0.3:  # a stretch of the sequence again at its end: long matches
                k = int(rng.integers(1, n + 1))
                at = int(rng.integers(0, n - k + 1))
                seq = (seq + seq[at:at + k])[-n:]
            breakers = set(rng.choice(V, int(rng.integers(0, 4)), replace=False).tolist())
            range_ = int(rng.choice([0, 0, 1, 5, 40, 1000]))
            allowed = int(rng.integers(1, 5))
            ref = webui_match_lengths(seq, range_, breakers)
            if ref and max(ref.values()) > D.MAX_MATCH:
                long_matches += 1
                continue
            want = {t: m for t, m in ref.items() if m >= allowed}
            got = D.dry_lengths(seq, 0, 0.8, allowed, range_, breakers)
            assert got == want, (seq, breakers, range_, allowed, got, want)
            cases += 1
            entries += len(want)
    assert cases > 550 and entries > 300, (cases, entries, long_matches)


def test_dry_match_is_capped_at_64():
    seq = [7] * 200
    assert webui_match_lengths(seq, 0, set()) == {7: 199}
    assert D.dry_lengths(seq, 0, 0.8, 2, 0, ()) == {7: 64}
    assert D.dry_lengths(seq, 0, 0.8, 2, 30, ()) == {7: 29} == webui_match_lengths(seq, 30, set())
    assert D.dry_lengths(seq, 150, 0.8, 2, 0, ()) == {7: 49}  # ids before s0 are never matched: i - s0 + 1 at i = e - 1
    assert D.banned(seq, 0, 64) == {7} and D.banned(seq[:63], 0, 64) == set() and D.banned(seq[:64], 0, 64) == {7}


def test_penalty_is_a_chain_of_float32_products():
    p = D.penalty(0.8, 1.75, 10, 2)
    want = np.float32(0.8)
    for _ in range(8):
        want = np.float32(want * np.float32(1.75))
    assert p == want and p.dtype == np.float32 and abs(float(p) - 0.8 * 1.75 ** 8) < 1e-4
    assert D.penalty(0.8, 1.75, 2, 2) == np.float32(0.8)
    assert np.isinf(D.penalty(1.0, 1e30, 4, 2))
    row = D.bits(np.array([1.0, np.nan, np.inf, -np.inf, 2.0], np.float32))
    out = D.apply(row, [9, 0, 9, 1, 9, 2, 9, 3, 9, 4, 9], multiplier=0.5, allowed_length=1)  # every id follows a 9: L = 1 each
    assert out[0] == D.bits(np.array([0.5], np.float32))[0] and out[1] == row[1] and out[2] == row[2] and out[3] == row[3]
    assert out[4] == D.bits(np.array([1.5], np.float32))[0]
    # p overflows: -inf, except a NaN
    out = D.apply(row, [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3], multiplier=1.0, base=1e30, allowed_length=2)
    assert out[4] == D.NEG_INF and (out[:4] == row[:4]).all()


# -- 3. the setter's refusals -----------------------------------------------------------------------------------------------------
REFUSALS = (
    "engine_set_dry: multiplier must be finite and >= 0 (0 = off)", "engine_set_dry: base must be finite and >= 1",
    "engine_set_dry: allowed_length must be >= 1", "engine_set_dry: range must be >= 0 (0 = the whole recorded sequence)",
    "engine_set_dry: no_repeat_ngram must be 0 (off) or 2 .. 64", "engine_set_dry: between 0 and TL_MAX_DRY_BREAKERS (64) breakers",
    "engine_set_dry: breaker id out of range", "engine_set_dry: a breaker id appears twice",
)


def test_the_record_under_sanitizers(tmp_path):
    """tests/dry_settings_check.cpp: the setter, carry, park / unpark and reset of csrc/slot_settings.h against byte arrays that stand
    for the device, as its own process"""
    exe = tmp_path / "dry_settings_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                    str(ROOT / "tiny-llm_amd" / "csrc"), str(ROOT / "tests" / "dry_settings_check.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
    assert done.stdout.strip().splitlines()[-1].startswith("ok checks="), done.stdout[-500:]
    seen = {line[len("refusal: "):] for line in done.stdout.splitlines() if line.startswith("refusal: ")}
    assert seen == set(REFUSALS)


def test_python_arguments():
    from tiny_llm_hip.engine import DRY_OFF, SETTINGS_KEYS, dry_args, dry_breaker_ids, request_settings

    assert dry_args() == DRY_OFF
    assert dry_args(0.8, 1.75, 2, 0, 3, [5, 9], 100) == (0.8, 1.75, 2, 0, 3, (5, 9))
    for bad, text in (((-1.0,), "dry_multiplier must be >= 0"), ((float("nan"),), "dry_multiplier must be a finite number"),
                      ((0.8, 0.5), "dry_base must be >= 1"), ((0.8, 1.75, 0), "dry_allowed_length must be >= 1"),
                      ((0.8, 1.75, 2, -1), "dry_range must be >= 0"), ((0.0, 1.75, 2, 0, 1), "no_repeat_ngram must be 0 (off) or 2 .. 64"),
                      ((0.0, 1.75, 2, 0, 65), "no_repeat_ngram must be 0 (off) or 2 .. 64"), ((0.8, 1.75, 2.5), "dry_allowed_length must be an int"),
                      ((0.8, 1.75, 2, 0, 0, [3, 3]), "a token id appears twice"), ((0.8, 1.75, 2, 0, 0, [100], 100), "inside the vocabulary"),
                      ((0.8, 1.75, 2, 0, 0, list(range(65))), "at most 64")):
        with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)").replace("..", r"\.\.")):
            dry_args(*bad)
    assert {"dry_multiplier", "dry_base", "dry_allowed_length", "dry_range", "dry_breakers", "no_repeat_ngram"} <= SETTINGS_KEYS
    got = request_settings([{"dry_multiplier": 0.8, "dry_breakers": [4]}, {"no_repeat_ngram": 3}, {}], 3, vocab_size=100)
    assert [s.dry for s in got] == [(0.8, 1.75, 2, 0, 0, (4,)), (0.0, 1.75, 2, 0, 3, ()), DRY_OFF]
    with pytest.raises(ValueError):
        request_settings({"no_repeat_ngram": 1}, 1)

    class Tok:  # each string gives the LAST id of its encoding
        def encode(self, s, add_special_tokens=False):
            return [ord(c) for c in s]

    assert dry_breaker_ids(Tok(), ["\n", "ab:", "x:", ""]) == [10, ord(":")]

    calls = []

    class Eng:
        def set_dry(self, slot, *a):
            calls.append((slot, a))

    for s in got:
        s.apply(Eng(), 2)
    assert calls == [(2, (0.8, 1.75, 2, 0, 0, (4,))), (2, (0.0, 1.75, 2, 0, 3, ()))]  # a request with both off makes no call


# -- 4. the C ABI -------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_agree(tmp_path):
    import tiny_llm_ext_hip as ext

    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        "#include <stdio.h>", '#include "tinyllm_engine.h"',
        "int (*set_dry)(tl_engine *, int, float, float, int, int, int, const int32_t *, int) = tl_engine_set_dry;",
        "int (*dry_rows)(int32_t *, int, int, const int32_t *, const int32_t *, const float *, const float *, const int32_t *, const int32_t *,",
        "                const int32_t *, const int32_t *, const int32_t *, uint32_t *, void *, int, void *) = tl_dry_rows;",
        'int main(void) { printf("%d %d\\n", TL_DRY_MAX_MATCH, TL_MAX_DRY_BREAKERS); return 0; }']))
    obj = tmp_path / "probe.o"  # compiled only: a pointer of another type is an error (-Werror), the symbols live in the library
    subprocess.run(["gcc", "-std=c11", "-Werror", "-I", str(ROOT / "include"), "-c", str(src), "-o", str(obj)], check=True)
    assert (ext.TL_DRY_MAX_MATCH, ext.TL_MAX_DRY_BREAKERS) == (D.MAX_MATCH, D.MAX_BREAKERS) == (64, 64)
    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    assert "#define TL_DRY_MAX_MATCH 64" in header and "#define TL_MAX_DRY_BREAKERS 64" in header
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert ext._SIGNATURES["tl_engine_set_dry"] == (i, [vp, i, f, f, i, i, i, ctypes.POINTER(ctypes.c_int32), i])
    assert ext._SIGNATURES["tl_dry_rows"] == (i, [vp, i, i] + [vp] * 11 + [i, vp])
    for name in ("tl_engine_set_dry", "tl_dry_rows"):
        fn = getattr(ext._lib, name)
        assert fn.restype is i and list(fn.argtypes) == ext._SIGNATURES[name][1]


# -- 5. the command line --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--dry-multiplier", "0.8"], ["--no-repeat-ngram", "3"]])
def test_batch_main_refuses_the_flags_with_a_draft_model(flags, capsys):
    import batch_main

    ap = batch_main.build_parser()
    args = ap.parse_args(["--model", "m", "--draft-model", "d", *flags])
    with pytest.raises(SystemExit):
        batch_main.check_draft_flags(ap, args, False)
    err = capsys.readouterr().err
    assert ("--draft-model runs greedy speculative decoding over the raw logits of one model; it does not combine with "
            "--dry-multiplier / --dry-base / --dry-allowed-length / --dry-range / --dry-breaker / --no-repeat-ngram") in err
    # (behind --lora in the list)
    args = ap.parse_args(["--model", "m", "--draft-model", "d", "--lora", "a", *flags])
    with pytest.raises(SystemExit):
        batch_main.check_draft_flags(ap, args, False)
    assert "does not combine with --lora, --dry-multiplier / " in capsys.readouterr().err
    batch_main.check_draft_flags(ap, ap.parse_args(["--model", "m", "--draft-model", "d", "--dry-base", "2.0"]), False)  # off: no clash


def test_main_flags():
    import main

    ap = main.build_parser()
    args = ap.parse_args(["--model", "m", "--dry-multiplier", "0.8", "--dry-base", "2", "--dry-allowed-length", "3", "--dry-range", "512",
                          "--dry-breaker", "\n", "--dry-breaker", ":", "--no-repeat-ngram", "4"])

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return [ord(c) for c in s]

    assert main.dry_settings(args, Tok()) == {"dry_multiplier": 0.8, "dry_base": 2.0, "dry_allowed_length": 3, "dry_range": 512,
                                             "dry_breakers": (10, 58), "no_repeat_ngram": 4}
    assert main.dry_settings(ap.parse_args(["--model", "m"]), Tok()) == {}
    with pytest.raises(SystemExit):
        main.check_beam_flags(ap, ap.parse_args(["--model", "m", "--num-beams", "2", "--no-repeat-ngram", "3"]))
