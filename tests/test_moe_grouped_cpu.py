"""CPU tier: the host side of the grouped-expert route (tl_moe_grouped_workspace_bytes, tl_moe_experts_rows_grouped,
tl_engine_set_moe_grouped): the workspace's stated layout and the refusals, through the library.  No kernel is launched."""

import ctypes

import pytest


@pytest.fixture(scope="module")
def ext(built_libs):
    import tiny_llm_ext_hip as ext

    return ext


@pytest.mark.parametrize("rows,k,D,I,E", [(1, 1, 128, 128, 1), (9, 8, 2048, 768, 128), (65, 4, 1664, 384, 8), (4095, 16, 256, 128, 1024)])
def test_workspace_bytes_are_the_stated_layout(ext, rows, k, D, I, E):
    """act, y (bf16), perm, offsets (int32, each padded to 16 bytes), the tile table of 1 + ceil(rows k / TM) + min(E, rows k) entries."""
    lib = ext.lib()
    TM = lib.tl_moe_grouped_tile_rows()
    assert TM in (32, 64)
    er, pad = rows * k, lambda b: (b + 15) // 16 * 16
    want = er * I * 2 + er * D * 2 + pad(er * 4) + pad((E + 1) * 4) + (1 + (er + TM - 1) // TM + min(E, er)) * 16
    assert lib.tl_moe_grouped_workspace_bytes(rows, k, D, I, E) == want
    assert lib.tl_moe_grouped_workspace_bytes(0, k, D, I, E) == 0 and lib.tl_moe_grouped_workspace_bytes(65536 // k + 1, k, D, I, E) == 0


def weights(ext, E=8, k=2, I=128, **nulls):
    p = {name: 0x1000 for name in ("gate", "up", "down", "gs", "gb", "us", "ub", "ds", "db")}
    p.update(nulls)
    return ext.TlMoeWeights(ext.TlW4(), p["gate"], p["up"], p["down"], p["gs"], p["gb"], p["us"], p["ub"], p["ds"], p["db"], E, k, I, 0)


@pytest.mark.parametrize("change,message", [
    (dict(xn=0), "null argument"), (dict(ws=0), "null argument"), (dict(w=dict(down=0)), "null expert tensor"),
    (dict(rows=32768), "rows x experts_per_token"), (dict(hidden=192), "hidden must be a positive multiple of 128"),
    (dict(w=dict(I=192)), "intermediate_size must be a positive multiple of 128"), (dict(short=16), "workspace is smaller"),
    (dict(w=dict(E=1025)), "num_experts <= 1024"), (dict(xn=0x1008), "rows must be 16-byte aligned"), (dict(w=dict(up=0x1004)), "expert words must be 16-byte aligned")])
def test_grouped_rows_refuses_bad_arguments_before_any_launch(ext, change, message):
    lib = ext.lib()
    a = dict(xn=0x1000, h=0x1000, ids=0x1000, scores=0x1000, out=0x1000, ws=0x1000, rows=4, hidden=256, short=0, w={})
    a.update(change)
    w = weights(ext, **a["w"])
    nbytes = max(lib.tl_moe_grouped_workspace_bytes(4, 2, 256, 128, 8), lib.tl_moe_grouped_workspace_bytes(a["rows"], 2, a["hidden"], 128, 8)) - a["short"]
    rc = lib.tl_moe_experts_rows_grouped(a["xn"], a["h"], a["ids"], a["scores"], ctypes.byref(w), a["rows"], a["hidden"], a["out"], a["ws"], nbytes, None)
    assert rc != 0
    with pytest.raises(RuntimeError, match=message):
        ext.check(rc)


def test_engine_setting_refuses_a_negative_row_count_and_a_null_engine(ext):
    """min_rows is checked before the engine is touched, so the refusal is reachable without a device (on a real engine:
    tests/test_zz_moe_grouped_gpu.py)."""
    lib = ext.lib()
    with pytest.raises(RuntimeError, match="min_rows must be >= 0"):
        ext.check(lib.tl_engine_set_moe_grouped(None, -1))
    for rc in (lib.tl_engine_set_moe_grouped(None, 8), lib.tl_engine_moe_grouped_state(None, None, None)):
        with pytest.raises(RuntimeError, match="null argument"):
            ext.check(rc)
