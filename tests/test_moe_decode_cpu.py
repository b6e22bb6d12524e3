"""CPU tier: the host side of the decode-shaped expert route (tl_moe_decode_workspace_bytes, tl_moe_experts_rows_decode,
tl_engine_set_moe_decode, the planner behind tl_moe_decode_plan / tl_moe_decode_wave), through the library.  No kernel is launched."""

import ctypes

import numpy as np
import pytest

SHAPES = [(16, 16, 256, 128), (8, 4, 1664, 384), (128, 8, 256, 128), (32, 8, 2048, 768)]  # (E, k, hidden, I)


@pytest.fixture(scope="module")
def ext(built_libs):
    import tiny_llm_ext_hip as ext

    return ext


@pytest.mark.parametrize("rows,k,D,I", [(1, 1, 128, 128), (9, 8, 2048, 768), (64, 16, 1664, 384)])
def test_workspace_bytes_are_the_stated_layout(ext, rows, k, D, I):
    """act [rows k, I] and y [rows k, hidden], bf16; 0 for sizes the route does not take."""
    size = ext.lib().tl_moe_decode_workspace_bytes
    assert size(rows, k, D, I) == rows * k * (I + D) * 2
    assert [size(0, k, D, I), size(65, k, D, I), size(rows, 17, D, I), size(rows, k, D + 64, I), size(rows, k, D, I + 64), size(rows, k, 0, I)] == [0] * 6


def weights(ext, E=8, k=2, I=128, **nulls):
    p = {name: 0x1000 for name in ("gate", "up", "down", "gs", "gb", "us", "ub", "ds", "db")}
    p.update(nulls)
    return ext.TlMoeWeights(ext.TlW4(), p["gate"], p["up"], p["down"], p["gs"], p["gb"], p["us"], p["ub"], p["ds"], p["db"], E, k, I, 0)


@pytest.mark.parametrize("change,message", [
    (dict(rows=65), "rows must be 1 .. 64"), (dict(hidden=192), "hidden must be a positive multiple of 128"), (dict(short=1), "workspace is smaller"),
    (dict(w=dict(up=0x1004)), "expert words must be 16-byte aligned"), (dict(w=dict(I=192)), "intermediate_size must be a positive multiple of 128"),
    (dict(w=dict(E=1025)), "num_experts <= 1024"), (dict(w=dict(E=32, k=17)), "experts_per_token"), (dict(ws=0), "null argument")])
def test_decode_rows_refuses_bad_arguments_before_any_launch(ext, change, message):
    lib = ext.lib()
    a = dict(xn=0x1000, h=0x1000, ids=0x1000, scores=0x1000, out=0x1000, ws=0x1000, rows=4, hidden=256, short=0, w={})
    a.update(change)
    w = weights(ext, **a["w"])
    nbytes = lib.tl_moe_decode_workspace_bytes(4, 2, 256, 128) - a["short"] if a["short"] else 1 << 20  # one byte short, or plenty
    rc = lib.tl_moe_experts_rows_decode(a["xn"], a["h"], a["ids"], a["scores"], ctypes.byref(w), a["rows"], a["hidden"], a["out"], a["ws"], nbytes, None)
    assert rc != 0
    with pytest.raises(RuntimeError, match=message):
        ext.check(rc)


def test_engine_setting_refuses_a_negative_row_count_and_a_null_engine(ext):
    lib = ext.lib()
    with pytest.raises(RuntimeError, match="min_rows must be >= 0"):
        ext.check(lib.tl_engine_set_moe_decode(None, -1))
    for rc in (lib.tl_engine_set_moe_decode(None, 8), lib.tl_engine_moe_decode_state(None, None, None)):
        with pytest.raises(RuntimeError, match="null argument"):
            ext.check(rc)


@pytest.mark.parametrize("cus", [256, 8])
@pytest.mark.parametrize("E,k,D,I", SHAPES)
def test_the_plan_covers_every_feature_and_every_group_exactly_once(ext, E, k, D, I, cus):
    """For 1 .. 64 rows: the waves of a stage's grid x, as the kernels ask tl_moe_decode_wave, tile (features x groups) of gate | up
    (I x hidden / 128) and of down (hidden x I / 128) with no gap and no overlap; a workgroup has at most four waves, all with work;
    grid y is min(rows k, E)."""
    lib = ext.lib()
    for rows in range(1, 65):
        plan, at = (ctypes.c_int * 12)(), (ctypes.c_int * 3)()
        ext.check(lib.tl_moe_decode_plan(rows, k, E, D, I, cus, plan))
        for (features, wk, per, grid_x, grid_y, threads), (N, K) in zip((plan[:6], plan[6:]), ((D, I), (I, D))):
            assert grid_y == min(rows * k, E) and threads % 64 == 0 and 64 <= threads <= 256 and threads == 64 * wk * features // 16
            seen = np.zeros((K, N // 128), dtype=np.int32)
            for block in range(grid_x):
                for wave in range(threads // 64):
                    ext.check(lib.tl_moe_decode_wave(features, wk, per, N // 128, block, wave, at))
                    f0, g0, g1 = at
                    assert 0 <= f0 and f0 + 16 <= K and 0 <= g0 < g1 <= N // 128
                    seen[f0:f0 + 16, g0:g1] += 1
            assert (seen == 1).all(), f"rows {rows}, {N} -> {K}: {(seen != 1).sum()} (feature, group) cells not covered exactly once"
