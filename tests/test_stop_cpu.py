"""CPU tier: stop conditions without a device (include/tinyllm_engine.h "Stop conditions").

* tests/stop_set_check.cpp, a stand-alone program over csrc/stop_set.h -- the automaton builder the library itself runs -- and the slot
  table's stopped state (csrc/slot_table.h): random string sets over a three-letter alphabet against a naive scan at every prefix of
  random texts, the fixed overlap cases, the invalid sets, and stop / resume / fork / move / park / unpark / release on the table with
  the page identity.  Built with AddressSanitizer and UBSan and run as its own process.
* tests/stop_oracle.py on hand-worked cases (it is the reference of the GPU tests).
* StopSet's argument validation, the struct's ctypes mirror, the symbols, and the entry points' refusals that need no device."""

import ctypes
import pathlib
import re
import subprocess

import pytest

from stop_oracle import ID, LENGTH, NONE, STRING, stop_oracle
from test_abi_layout_cpu import c_fields

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "stop_set_check.cpp"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tiny-llm_amd" / "csrc")]
SYMBOLS = ["tl_stop_create", "tl_stop_destroy", "tl_engine_set_stop", "tl_engine_stop_state", "tl_stop_rows"]
TL_ERR_INVALID = -1


def test_the_automaton_agrees_with_a_naive_scan_and_refuses_invalid_sets(tmp_path):
    exe = tmp_path / "stop_set_check"
    subprocess.run([*FLAGS, str(DRIVER), "-o", str(exe)], check=True)
    lines = []
    for seed in ("1", "7"):
        done = subprocess.run([str(exe), "300", seed], capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        line = done.stdout.strip()
        assert line.startswith("ok rounds=300 "), line
        counts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)\b", line)}
        assert counts["checked"] >= 100_000 and counts["matches"] >= 10_000, line  # the texts do hold the strings
        lines.append(line)
    assert lines[0] != lines[1]  # the seed is read


def test_the_stop_set_header_is_host_only():
    text = (ROOT / "tiny-llm_amd" / "csrc" / "stop_set.h").read_text()
    assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text
    assert '#include "' not in text  # nothing of the project's device code either


VOCAB = [b"", b"a", b"b", b"ab", b"abc", b"cab", b"xyz", b"c"]


@pytest.mark.parametrize("tokens, kw, want", [
    # a string spanning three tokens: "a" + "b" + "cab" holds "abc"; it ends at the first byte of the third token
    ([1, 2, 5], dict(strings=[b"abc"]), (STRING, 0, 3, 5, 0)),
    # ends in mid-token with more bytes behind it: cut < text
    ([6, 5], dict(strings=[b"zc"]), (STRING, 0, 2, 6, 2)),
    # two strings end on one byte: the longest wins (the earliest start)
    ([6, 3], dict(strings=[b"b", b"zab"]), (STRING, 1, 2, 5, 2)),
    # ... but an earlier byte wins over a longer string that ends later
    ([3, 7], dict(strings=[b"abc", b"a"]), (STRING, 1, 1, 2, 0)),
    # an id wins over a string its bytes would complete, and its bytes are no text
    ([1, 2], dict(ids=[9, 2], strings=[b"ab"]), (ID, 1, 2, 1, 1)),
    # id and budget on one token: the id; string and budget: the string; the budget alone
    ([1, 2], dict(ids=[2], max_new_tokens=2), (ID, 0, 2, 1, 1)),
    ([1, 2], dict(strings=[b"ab"], max_new_tokens=2), (STRING, 0, 2, 2, 0)),
    ([1, 1, 1], dict(strings=[b"zz"], max_new_tokens=2), (LENGTH, 0, 2, 2, 2)),
    ([4], dict(max_new_tokens=1), (LENGTH, 0, 1, 3, 3)),
    # a token without bytes is a token all the same
    ([0, 0, 1], dict(strings=[b"b"], max_new_tokens=5), (NONE, 0, 3, 1, 1)),
])
def test_the_oracle_on_worked_cases(tokens, kw, want):
    assert stop_oracle(tokens, VOCAB, **kw) == want


def test_stop_args_validation(built_libs):
    from tiny_llm_hip.stop import MAX_STOP_BYTES, request_stops, stop_args

    assert stop_args([3, 1], ["né", b"\x00\xff"], 10) == ([3, 1], ["né".encode(), b"\x00\xff"])
    assert stop_args(range(16), [bytes([65 + i]) * 64 for i in range(16)], 16)[1][15] == b"P" * 64  # 16 ids, 16 strings, 1,024 bytes
    for bad, err in [
        (dict(ids=[], strings=[]), ValueError), (dict(ids=[10], vocab_size=10), ValueError), (dict(ids=[-1]), ValueError),
        (dict(ids=[2, 2]), ValueError), (dict(ids=list(range(17))), ValueError), (dict(ids=[1.5]), TypeError), (dict(ids=[True]), TypeError),
        (dict(strings=[b""]), ValueError), (dict(strings=["a", b"a"]), ValueError), (dict(strings=[bytes([i]) for i in range(17)]), ValueError),
        (dict(strings=[b"x" * (MAX_STOP_BYTES + 1)]), ValueError), (dict(strings=[b"x" * 1000, b"y" * 25]), ValueError),
        (dict(strings="abc"), TypeError), (dict(strings=[7]), TypeError), (dict(ids=5), TypeError),
    ]:
        with pytest.raises(err):
            stop_args(**bad)
    assert request_stops(None, 3) is None
    with pytest.raises(ValueError):
        request_stops(["not a set"], 1)
    with pytest.raises(ValueError):
        request_stops([None, None], 3)


def test_stop_state_matches_the_c_layout(tmp_path, built_libs):
    import tiny_llm_ext_hip as ext

    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    fields = c_fields(header, "tl_stop_state")
    assert fields == ["reason", "index", "generated", "context", "text_bytes", "cut_bytes"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tinyllm_engine.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(tl_stop_state));']
    lines += [f'    printf("{f} %zu\\n", offsetof(tl_stop_state, {f}));' for f in fields]
    lines += ['    printf("limits %d %d %d %d %d %d %d\\n", TL_MAX_STOP_IDS, TL_MAX_STOP_STRINGS, TL_MAX_STOP_BYTES, TL_STOP_NONE, TL_STOP_ID, TL_STOP_STRING,'
              " TL_STOP_LENGTH);", "    return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    from tiny_llm_hip import stop

    assert out.pop().split()[1:] == [str(v) for v in (stop.MAX_STOP_IDS, stop.MAX_STOP_STRINGS, stop.MAX_STOP_BYTES, NONE, ID, STRING, LENGTH)]
    assert stop.REASONS == ext.STOP_REASONS == ("none", "id", "string", "length")
    want = {k: int(v) for k, v in (line.split() for line in out)}
    cls = ext.TlStopState
    assert ctypes.sizeof(cls) == want.pop("size")
    assert [n for n, *_ in cls._fields_] == list(want)
    for name, offset in want.items():
        assert getattr(cls, name).offset == offset, name


def test_the_symbols_are_declared_exported_and_bound(built_libs):
    import tiny_llm_ext_hip as ext

    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        fn = getattr(ext.lib(), name)
        assert fn.argtypes is not None and name in ext._SIGNATURES, name


def test_bad_arguments_are_invalid_before_anything_is_allocated(built_libs):
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    state = ext.TlStopState(7, 7, 7, 7, 7, 7)
    assert lib.tl_engine_set_stop(None, 0, None, 4) == TL_ERR_INVALID
    assert lib.tl_engine_stop_state(None, 0, ctypes.byref(state)) == TL_ERR_INVALID
    assert (state.reason, state.cut_bytes) == (7, 7)  # nothing changed
    i32 = ctypes.c_int32
    handle = ctypes.c_void_p(123)

    def create(ids, strings):
        data = b"".join(strings)
        offsets = [0]
        for s in strings:
            offsets.append(offsets[-1] + len(s))
        return lib.tl_stop_create(None, (i32 * max(len(ids), 1))(*ids), len(ids), ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p) if data else None,
                                  (i32 * len(offsets))(*offsets), len(strings), None, ctypes.byref(handle))

    assert lib.tl_stop_create(None, None, 0, None, None, 0, None, None) == TL_ERR_INVALID
    for ids, strings in [([], []), ([1, 1], []), ([-1], []), (list(range(17)), []), ([], [b"ab"])]:  # (strings without a vocabulary)
        assert create(ids, strings) == TL_ERR_INVALID, (ids, strings)
        assert handle.value is None  # the output is cleared, nothing was made
        handle = ctypes.c_void_p(123)
    lib.tl_stop_destroy(None)  # a null set is nobody's
    # the rows: null arrays and a bad row count, before any launch
    assert lib.tl_stop_rows(None, None, 1, None, 1, 1, 1, None) == TL_ERR_INVALID
    assert lib.tl_stop_rows(None, 1, 0, None, 1, 1, 1, None) == TL_ERR_INVALID
    assert lib.tl_stop_rows(None, 1, 65536, None, 1, 1, 1, None) == TL_ERR_INVALID


def test_cli_flags_are_repeatable_and_off_by_default():
    import batch_main
    import main

    for parser in (main.build_parser(), batch_main.build_parser()):
        args = parser.parse_args(["--model", "m"])
        assert args.stop == [] and args.stop_id == []
        args = parser.parse_args(["--model", "m", "--stop", "a", "--stop-id", "7", "--stop", "\n\n", "--stop-id", "9"])
        assert args.stop == ["a", "\n\n"] and args.stop_id == [7, 9]
        with pytest.raises(SystemExit):
            parser.parse_args(["--model", "m", "--stop-id", "x"])


def test_cut_text(built_libs):
    from tiny_llm_hip.stop import cut_text

    token_bytes = [b"", b"ab", b"c", "é".encode()]
    assert cut_text([1, 2, 0, 3], token_bytes) == "abcé"
    assert cut_text([1, 2, 3], token_bytes, cut_bytes=2) == "ab"
    assert cut_text([1, 2, 3, 1], token_bytes, strings=["bc", b"\xa9a"]) == "a"  # the earliest match of any string
    assert cut_text([1, 2], token_bytes, strings=["zz"]) == "abc"
    assert cut_text([3], token_bytes, cut_bytes=1) == "\ufffd"  # a cut inside a character
