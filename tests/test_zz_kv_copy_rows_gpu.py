"""GPU tier: tl_kv_copy_rows (csrc/kv_copy.h), the one-launch tail copy of a prefix-cache hit, over caller pools.

Pools [4 pages, 2 heads, 16 rows, row_bytes] with row_bytes 256 (bf16 rows of head size 128), 128 (FP8 rows) and 4 (FP8 row scales)
mixed in ONE call: the 16-byte and the 4-byte path side by side.  Rows [0, rows) of every head of the source page must arrive in the
destination page, and every other byte of every pool must still hold its sentinel -- rows beyond `rows` of the destination page
included."""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
PAGES, HEADS, PAGE = 4, 2, 16
ROW_BYTES = (256, 128, 4)


@pytest.fixture(scope="module")
def ext():
    import tiny_llm_ext_hip

    tiny_llm_ext_hip.load_library(".")
    return tiny_llm_ext_hip


@pytest.mark.parametrize("rows", [1, 7, 15, 16])
def test_rows_arrive_and_nothing_else_is_written(ext, rows):
    gen = torch.Generator().manual_seed(rows)
    pools = [torch.randint(0, 256, (PAGES, HEADS, PAGE, rb), dtype=torch.uint8, generator=gen).cuda() for rb in ROW_BYTES]
    before = [p.clone() for p in pools]
    table = (ext.TlKvPoolDesc * len(pools))(*[ext.TlKvPoolDesc(p.data_ptr(), rb) for p, rb in zip(pools, ROW_BYTES)])
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    src, dst = 2, 1
    torch.cuda.synchronize()
    ext.check(ext.lib().tl_kv_copy_rows(table_dev.data_ptr(), len(pools), HEADS, PAGE, src, dst, rows, None))
    torch.cuda.synchronize()
    for got, was in zip(pools, before):
        want = was.clone()
        want[dst, :, :rows] = was[src, :, :rows]
        assert torch.equal(got[dst, :, :rows], was[src, :, :rows]), "copied rows differ"
        assert torch.equal(got, want), "a byte outside rows [0, rows) of the destination page changed"


def test_bad_arguments_launch_nothing(ext):
    pool = torch.zeros((PAGES, HEADS, PAGE, 16), dtype=torch.uint8).cuda()
    table = (ext.TlKvPoolDesc * 1)(ext.TlKvPoolDesc(pool.data_ptr(), 16))
    table_dev = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    lib = ext.lib()
    for args in [(1, HEADS, PAGE, 1, 1, 4), (1, HEADS, PAGE, 0, 1, 0), (1, HEADS, PAGE, 0, 1, PAGE + 1), (0, HEADS, PAGE, 0, 1, 4), (1, HEADS, PAGE, 0, -1, 4)]:
        assert lib.tl_kv_copy_rows(table_dev.data_ptr(), *args, None) == -1, args
    torch.cuda.synchronize()
    assert int(pool.sum()) == 0
