"""CPU tier: the prefix cache's part of the C ABI (include/tinyllm_engine.h "Prefix cache"): the two new structs have the C
compiler's layout in their ctypes mirrors, and the entry points refuse a null engine with TL_ERR_INVALID and change nothing.  (What
an engine with the cache disabled returns needs an engine, hence a device: tests/test_zz_prefix_cache_gpu.py, "cache off".)"""

import ctypes
import pathlib
import subprocess

from test_abi_layout_cpu import c_fields

ROOT = pathlib.Path(__file__).resolve().parents[1]
PAIRS = {"tl_prefix_stats": "TlPrefixStats", "tl_kv_pool_desc": "TlKvPoolDesc"}


def test_new_structs_match_the_c_layout(tmp_path, built_libs):
    import tiny_llm_ext_hip as ext

    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "tinyllm_engine.h"', "int main(void) {"]
    for struct in PAIRS:
        lines.append(f'    printf("{struct} size %zu\\n", sizeof({struct}));')
        for f in c_fields(header, struct):
            lines.append(f'    printf("{struct} {f} %zu\\n", offsetof({struct}, {f}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    want: dict[str, dict[str, int]] = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        struct, field, value = line.split()
        want.setdefault(struct, {})[field] = int(value)
    assert c_fields(header, "tl_prefix_stats") == ["lookups", "hits", "tokens_matched", "tail_rows_copied", "pages_registered", "pages_evicted",
                                                   "entries", "pages_retained", "max_retained_pages", "enabled"]
    for struct, cls_name in PAIRS.items():
        cls = getattr(ext, cls_name)
        assert ctypes.sizeof(cls) == want[struct]["size"], (cls_name, ctypes.sizeof(cls), want[struct]["size"])
        names = [n for n, *_ in cls._fields_]
        assert names == [f for f in want[struct] if f != "size"], f"{cls_name}: field names / order differ from {struct}"
        for n in names:
            assert getattr(cls, n).offset == want[struct][n], f"{cls_name}.{n}"


def test_null_engine_and_bad_arguments_are_invalid(built_libs):
    import tiny_llm_ext_hip as ext

    lib = ext.lib()
    TL_ERR_INVALID = -1
    matched = ctypes.c_int(77)
    tokens = (ctypes.c_int32 * 4)(1, 2, 3, 4)
    stats = ext.TlPrefixStats()
    stats.lookups = 5
    assert lib.tl_engine_prefix_cache(None, 1, 0) == TL_ERR_INVALID
    assert lib.tl_engine_prefix_attach(None, 0, tokens, 4, ctypes.byref(matched)) == TL_ERR_INVALID
    assert matched.value == 77  # nothing changed
    assert lib.tl_engine_prefix_extend(None, 0, tokens, 4) == TL_ERR_INVALID
    assert lib.tl_engine_prefix_clear(None) == TL_ERR_INVALID
    assert lib.tl_engine_prefix_stats(None, ctypes.byref(stats)) == TL_ERR_INVALID
    assert stats.lookups == 5
    # the copy routine checks its host arguments before it launches anything (no device is touched here)
    for args in [(None, 1, 2, 16, 0, 1, 4), (1, 0, 2, 16, 0, 1, 4), (1, 1, 0, 16, 0, 1, 4), (1, 1, 2, 16, 1, 1, 4), (1, 1, 2, 16, -1, 1, 4),
                 (1, 1, 2, 16, 0, 1, 0), (1, 1, 2, 16, 0, 1, 17)]:
        assert lib.tl_kv_copy_rows(*args, None) == TL_ERR_INVALID, args
