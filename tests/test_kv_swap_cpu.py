"""CPU tier: KV swap without a device (include/tinyllm_engine.h "KV swap").

* tests/kv_swap_model_check.cpp, a stand-alone program that drives csrc/slot_table.h -- the slot protocol the engine itself runs --
  through 20,000 seeded random begin / prefill / decode step / rewind / attach / fork / park / unpark / move / release / evict
  operations on slots in every state, the prefix cache on for the second half.  Its model of the device (block table, page and record
  contents) learns of the table's decisions only through the edits a call reports (tests/slot_model_check.h).  After every operation:
  the page identity, "a page a slot references is never free", "host records in use == sum over parked slots", every take and
  eviction the brute-force victim, every unparked slot reading its own tokens' fingerprints back, and a refused call -- a decode step
  over several slots that the pool cannot serve among them -- changing nothing.  Built with AddressSanitizer and UBSan and run as its
  own process.
* the new struct's ctypes mirror has the C compiler's layout; the new symbols are exported and bound; the entry points refuse a null
  engine and bad host arguments with TL_ERR_INVALID before anything is launched."""

import ctypes
import pathlib
import re
import subprocess

from test_abi_layout_cpu import c_fields

ROOT = pathlib.Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "kv_swap_model_check.cpp"
FLAGS = ["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "tiny-llm_amd" / "csrc")]
SYMBOLS = ["tl_engine_swap_space", "tl_engine_park", "tl_engine_unpark", "tl_engine_slot_parked", "tl_engine_step_pages",
           "tl_engine_swap_stats", "tl_kv_page_record_bytes", "tl_kv_gather_pages", "tl_kv_scatter_pages"]
TL_ERR_INVALID = -1


def test_random_operations_keep_the_page_and_record_invariants(tmp_path):
    exe = tmp_path / "kv_swap_model_check"
    subprocess.run([*FLAGS, str(DRIVER), "-o", str(exe)], check=True)
    lines = []
    for seed in ("12345", "7"):
        done = subprocess.run([str(exe), "20000", seed], capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]
        line = done.stdout.strip()
        assert line.startswith("ok ops=20000 "), line
        counts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)\b", line)}
        # the run exercises what it claims to: every kind of operation, the refusals for want of pages or records, the cache's
        # registrations and evictions
        for key in ("begins", "forks", "parks", "park_refusals", "unparks", "unpark_refusals", "moves", "releases", "evicted", "registered",
                    "rewinds", "rewind_refusals", "attaches", "fork_refusals", "step_refusals"):
            assert counts[key] >= 100, (key, line)
        assert counts["appends"] >= 5000, line
        lines.append(line)
    assert lines[0] != lines[1]  # the seed is read


def test_swap_stats_matches_the_c_layout(tmp_path, built_libs):
    import tiny_llm_ext_hip as ext

    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    fields = c_fields(header, "tl_swap_stats")
    assert fields == ["host_pages", "host_pages_in_use", "parks", "unparks", "pages_out", "pages_in", "record_bytes"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tinyllm_engine.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(tl_swap_stats));']
    lines += [f'    printf("{f} %zu\\n", offsetof(tl_swap_stats, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    want = {k: int(v) for k, v in (line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())}
    cls = ext.TlSwapStats
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
    assert ext.lib().tl_kv_page_record_bytes.restype is ctypes.c_size_t


def test_null_engine_and_bad_arguments_are_invalid(built_libs):
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    need, obtainable = ctypes.c_int(77), ctypes.c_int(78)
    stats = ext.TlSwapStats()
    stats.parks = 5
    assert lib.tl_engine_swap_space(None, 4) == TL_ERR_INVALID
    assert lib.tl_engine_park(None, 0) == TL_ERR_INVALID
    assert lib.tl_engine_unpark(None, 0) == TL_ERR_INVALID
    assert lib.tl_engine_slot_parked(None, 0) < 0
    assert lib.tl_engine_step_pages(None, 1, ctypes.byref(need), ctypes.byref(obtainable)) == TL_ERR_INVALID
    assert (need.value, obtainable.value) == (77, 78)  # nothing changed
    assert lib.tl_engine_swap_stats(None, ctypes.byref(stats)) == TL_ERR_INVALID
    assert stats.parks == 5
    # the record size is host arithmetic: heads * page_size * sum of row_bytes, 0 on bad input
    pools = (ext.TlKvPoolDesc * 4)(*[ext.TlKvPoolDesc(None, rb) for rb in (256, 256, 4, 6)])
    assert lib.tl_kv_page_record_bytes(pools, 4, 2, 16) == 2 * 16 * 522
    assert lib.tl_kv_page_record_bytes(pools, 2, 8, 128) == 8 * 128 * 512
    assert lib.tl_kv_page_record_bytes(None, 4, 2, 16) == 0
    assert lib.tl_kv_page_record_bytes(pools, 0, 2, 16) == 0 and lib.tl_kv_page_record_bytes(pools, 4, 0, 16) == 0
    # gather and scatter check their host arguments before they launch anything (no device is touched here): pools, offsets, n_pools,
    # heads, page_size, page ids, n_pages, tail_rows, staging, record_bytes
    good = (1, 1, 4, 2, 16, 1, 3, 7, 1, 16704)
    bad = [(None,) + good[1:], good[:1] + (None,) + good[2:], good[:2] + (0,) + good[3:], good[:3] + (0,) + good[4:], good[:4] + (0,) + good[5:],
           good[:5] + (None,) + good[6:], good[:6] + (0,) + good[7:], good[:6] + (65536,) + good[7:], good[:7] + (0,) + good[8:],
           good[:7] + (17,) + good[8:], good[:8] + (None,) + good[9:], good[:9] + (0,)]
    for fn in (lib.tl_kv_gather_pages, lib.tl_kv_scatter_pages):
        for args in bad:
            assert fn(*args, None) == TL_ERR_INVALID, args
