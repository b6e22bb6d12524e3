"""GPU tier: text embeddings -- the pooling kernels over caller rows (tl_pool_rows, csrc/pool.h) against the float64 numpy pooling with
allowances derived per element (tests/embedding_oracle.py), and the engine's tl_engine_embed / tl_engine_embed_packed / embed_ids against
the bf16 oracle and the float64 truth through the project's rule (helpers.check_against_truth), plus the slot lifecycle around them."""

import ctypes

import numpy as np
import pytest
import torch

import embedding_oracle as E
from helpers import QWEN4B_CFG, TINY_CFG, assert_within, check_against_truth, to_mlx_shaped
from oracle import tiny_oracle as O

pytestmark = pytest.mark.gpu

TL_ERR_INVALID = -1
LENS = [1, 2, 63, 64, 65, 257]  # across the 8 row residues of a wave, the 64-row mark and a few hundred rows


def _ext():
    import tiny_llm_ext_hip as ext

    return ext


def _bf16_rows(rng, total, hidden):
    """Random bf16 rows with per-row and per-column magnitudes spread over a few binades, as float32 (exact bf16 values)."""
    x = rng.standard_normal((total, hidden), dtype=np.float32) * np.exp2(rng.integers(-3, 3, size=(total, 1))).astype(np.float32)
    return O.bf16(x + 0.25)  # (an offset: the column means are not all near zero)


def _dev(rows):
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to("cuda", torch.bfloat16)


def _seq_lens(n_seqs):
    """Mixed lengths for one launch: LENS cycled from 63 on (3 sequences: 63, 64, 65; 16: every length, most of them three times)."""
    return [LENS[(i + 2) % len(LENS)] for i in range(n_seqs)] if n_seqs > 1 else [65]


# ---- the kernels over caller rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seqs", [1, 3, 16])
@pytest.mark.parametrize("hidden", [128, 256, 2560])
def test_pool_rows_matches_the_float64_pooling(hidden, n_seqs):
    ext = _ext()
    rng = np.random.default_rng(hidden + n_seqs)
    lens = _seq_lens(n_seqs)
    gaps = [int(g) for g in rng.integers(0, 3, size=n_seqs)]  # unused rows between the sequences
    row0, at = [], 1
    for ln, g in zip(lens, gaps):
        row0.append(at + g)
        at += g + ln
    rows = _bf16_rows(rng, at + 1, hidden)
    dev = _dev(rows)
    for pooling in ("last", "mean"):
        for normalize in (False, True):
            for dim in (1, 32, 100, hidden):
                got = ext.pool_rows(dev, list(zip(row0, lens)), pooling=pooling, normalize=normalize, dim=dim).cpu().numpy()
                assert got.shape == (n_seqs, dim) and got.dtype == np.float32
                for i, (r0, ln) in enumerate(zip(row0, lens)):
                    seq = rows[r0:r0 + ln]
                    want = E.pool(seq, pooling, dim, normalize)
                    what = f"hidden {hidden}, {n_seqs} sequences, sequence {i} (len {ln}), {pooling}, normalize {normalize}, dim {dim}"
                    if pooling == "last" and not normalize:
                        assert np.array_equal(got[i].astype(np.float64), want), what  # exact: the widened bf16 row
                    else:
                        assert_within(got[i], want, E.pool_allowance(seq, pooling, dim, normalize), what)


@pytest.mark.parametrize("ln", LENS)
def test_pool_rows_every_length_alone(ln):
    ext = _ext()
    rng = np.random.default_rng(ln)
    rows = _bf16_rows(rng, ln, 256)
    dev = _dev(rows)
    for pooling in ("last", "mean"):
        for normalize in (False, True):
            got = ext.pool_rows(dev, [(0, ln)], pooling=pooling, normalize=normalize, dim=100).cpu().numpy()[0]
            if pooling == "last" and not normalize:
                assert np.array_equal(got.astype(np.float64), E.pool(rows, pooling, 100, normalize))
            else:
                assert_within(got, E.pool(rows, pooling, 100, normalize), E.pool_allowance(rows, pooling, 100, normalize), f"len {ln} {pooling} {normalize}")


@pytest.mark.parametrize("hidden", [128, 2560])
def test_pool_rows_does_not_depend_on_position_or_neighbours(hidden):
    ext = _ext()
    rng = np.random.default_rng(7)
    seq = _bf16_rows(rng, 257, hidden)
    alone = _dev(seq)
    lens = [5, 64, 257, 1, 63, 2, 65, 9, 257, 3, 17, 64, 1, 2, 33, 8]
    target = 8  # the 257-row sequence in the middle, at an odd first row
    crowd = _bf16_rows(rng, sum(lens) + 3, hidden)
    row0 = list(3 + np.concatenate([[0], np.cumsum(lens)[:-1]]))
    assert row0[target] % 2 == 1
    crowd[row0[target]:row0[target] + 257] = seq
    crowd_dev = _dev(crowd)
    for pooling in ("last", "mean"):
        for normalize in (False, True):
            for dim in (100, hidden):
                a = ext.pool_rows(alone, [(0, 257)], pooling=pooling, normalize=normalize, dim=dim).cpu().numpy()[0]
                b = ext.pool_rows(crowd_dev, list(zip(row0, lens)), pooling=pooling, normalize=normalize, dim=dim).cpu().numpy()[target]
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (pooling, normalize, dim)


@pytest.mark.parametrize("cuts", [(100,), (64, 65), (1, 256)])
def test_pool_rows_mean_in_chunks_through_the_running_sums(cuts):
    """The rows of one sequence fed in 2 and 3 launches: same allowance as one shot (each launch's column sums and the additions into the
    running sum are among the len roundings the bound counts).  A sequence of zero rows shares every launch."""
    ext = _ext()
    hidden, total = 256, 257
    rng = np.random.default_rng(len(cuts))
    rows = _bf16_rows(rng, total + 40, hidden)
    rows[:20] = 0
    dev = _dev(rows)
    seq = rows[40:40 + total]
    edges = [0, *cuts, total]
    for normalize, dim in ((False, hidden), (True, 100)):
        sums = torch.full((2, hidden), float("nan"), dtype=torch.float32, device="cuda")  # prior 0 replaces whatever is there
        for j in range(len(edges) - 1):
            a, b = edges[j], edges[j + 1]
            last = int(b == total)
            out = ext.pool_rows(dev, [(0, 20), (40 + a, b - a)], pooling="mean", normalize=normalize, dim=dim, finish=[last, last],
                                prior=[20 * j, a], sums=sums)
            assert out.shape == (2 * last, dim)
        got = out.cpu().numpy()
        assert not got[0].any(), "the zero sequence stays zero"
        assert_within(got[1], E.pool(seq, "mean", dim, normalize), E.pool_allowance(seq, "mean", dim, normalize), f"chunks {cuts}, normalize {normalize}")


def test_pool_rows_zero_and_nan_rows_and_bad_arguments():
    ext = _ext()
    lib = ext.lib()
    hidden = 128
    rows = np.zeros((12, hidden), dtype=np.float32)
    rows[4:8] = O.bf16(np.random.default_rng(1).standard_normal((4, hidden), dtype=np.float32))
    rows[6, 5] = np.nan
    dev = _dev(rows)
    for pooling in ("last", "mean"):
        for normalize in (False, True):
            got = ext.pool_rows(dev, [(0, 4), (4, 4), (8, 4)], pooling=pooling, normalize=normalize, dim=hidden).cpu().numpy()
            assert not got[0].any() and not got[2].any(), "a vector of norm 0 stays all zeros"
            if pooling == "mean":
                assert np.isnan(got[1, 5]) and (normalize or not np.isnan(np.delete(got[1], 5)).any())
                assert not normalize or np.isnan(got[1]).all(), "NaN propagates through the norm"
            else:
                assert not np.isnan(got[1]).any()  # the last row holds no NaN
    # a last row with a NaN in column 5: every component is NaN once column 5 is inside dim, none while it is outside
    assert np.isnan(ext.pool_rows(dev, [(4, 3)], pooling="last", normalize=True, dim=32).cpu().numpy()[0]).all()
    assert not np.isnan(ext.pool_rows(dev, [(4, 3)], pooling="last", normalize=True, dim=5).cpu().numpy()[0]).any()

    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    out = torch.zeros(hidden, dtype=torch.float32, device="cuda")
    sums = torch.zeros(hidden, dtype=torch.float32, device="cuda")
    good = dict(rows=dev.data_ptr(), hidden=hidden, n=1, row0=ints(0), len=ints(4), finish=ints(1), prior=ints(0), pooling=1, sums=sums.data_ptr(),
                normalize=1, dim=hidden, out=out.data_ptr())
    call = lambda **kw: lib.tl_pool_rows(*{**good, **kw}.values(), None)
    assert call() == 0
    torch.cuda.synchronize()
    before = out.clone()
    for bad in (dict(pooling=2), dict(pooling=-1), dict(dim=0), dict(dim=hidden + 1), dict(n=0), dict(n=17), dict(hidden=127), dict(hidden=0),
                dict(rows=None), dict(row0=None), dict(len=None), dict(finish=None), dict(sums=None), dict(prior=None), dict(out=None),
                dict(len=ints(0)), dict(row0=ints(-1)), dict(prior=ints(-1))):
        assert call(**bad) == TL_ERR_INVALID, bad
    torch.cuda.synchronize()
    assert torch.equal(out, before)


# ---- the engine -------------------------------------------------------------------------------------------------------------------------------
PROMPT_LENS = [5, 64, 200]
OTHERS = [7, 33, 90]  # the three prompts a packed pass puts beside the one under test


@pytest.fixture(scope="module")
def tiny():
    """The TINY checkpoint on the device and, per KV format and prompt, the final-norm rows of the bf16 oracle and of the float64 truth
    (computed once; the tests only read them)."""
    weights = O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05)
    rng = np.random.default_rng(17)
    prompts = {n: [int(t) for t in rng.integers(1, TINY_CFG["vocab_size"], size=n)] for n in PROMPT_LENS}
    others = [[int(t) for t in rng.integers(1, TINY_CFG["vocab_size"], size=n)] for n in OTHERS]
    truth = {n: E.final_rows(O.TruthQwen3, TINY_CFG, weights, p) for n, p in prompts.items()}
    oracle = {fmt: {n: E.final_rows(O.OracleQwen3, TINY_CFG, weights, p, kv_format=fmt) for n, p in prompts.items()} for fmt in ("bf16", "fp8")}
    return dict(model=to_mlx_shaped(TINY_CFG, weights), weights=weights, prompts=prompts, others=others, truth=truth, oracle=oracle)


def _engine(model, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    args = dict(page_size=16, num_pages=96, max_batch=4, max_prefill_rows=512)
    args.update(kw)
    return DecodeEngine(model, **args)


def _three_ways(eng, prompt, others, pooling, **kw):
    """The prompt's vector alone in slot 0 in one chunk, chunked at 64, and packed into slot 2 beside three other prompts."""
    alone = eng.embed(prompt, slot=0, pooling=pooling, **kw)
    chunked = eng.embed(prompt, slot=0, pooling=pooling, chunk=64, **kw)
    slots = [0, 1, 3]
    for s in (0, 1, 2, 3):
        eng.begin(s)
    try:
        chunks = [(slots[0], others[0], True), (slots[1], others[1], True), (2, prompt, True), (slots[2], others[2], True)]
        packed = eng.embed_packed(chunks, pooling=pooling, **kw)[2]
    finally:
        for s in (0, 1, 2, 3):
            eng.release(s)
    return dict(alone=alone, chunked=chunked, packed=packed)


@pytest.mark.parametrize("n", PROMPT_LENS)
@pytest.mark.parametrize("kv_format", ["bf16", "fp8"])
def test_engine_embeddings_sit_inside_the_truth_band(tiny, kv_format, n):
    eng = _engine(tiny["model"], kv_format=kv_format)
    try:
        prompt = tiny["prompts"][n]
        for pooling in ("last", "mean"):
            want = E.pool(tiny["oracle"][kv_format][n], pooling, normalize=False)
            exact = E.pool(tiny["truth"][n], pooling, normalize=False)
            raw = _three_ways(eng, prompt, tiny["others"], pooling, normalize=False)
            for way, got in raw.items():
                assert got.dtype == np.float32 and got.shape == (TINY_CFG["hidden_size"],)
                rec = check_against_truth(got[None], want[None], exact[None], what=f"embed {pooling}, {n} tokens, {kv_format} pages, {way}")
                print(f"{pooling} {n} {kv_format} {way}: hip {rec['max_abs_hip_vs_truth']:.3e} oracle {rec['max_abs_oracle_vs_truth']:.3e} "
                      f"rms {rec['rms_hip_vs_truth']:.3e} / {rec['rms_oracle_vs_truth']:.3e}")
            # the finish: the normalised / truncated output is the numpy finish of the engine's own un-normalised vector
            for dim in (1, 32, 100, TINY_CFG["hidden_size"]):
                got = eng.embed(prompt, pooling=pooling, normalize=True, dim=dim)
                want_n = E.finish(raw["alone"], dim, True)
                assert_within(got, want_n, np.abs(want_n) * dim * 2.0 ** -24, f"finish {pooling} dim {dim}")
                cut = eng.embed(prompt, pooling=pooling, normalize=False, dim=dim)
                assert np.array_equal(cut, raw["alone"][:dim])
        assert eng.stats()["pages_in_use"] == 0
    finally:
        eng.close()


def _state(eng, slot, produced):
    """What an embed call must leave alone: the pending token, every produced id (and that there are exactly `produced` of them), the
    logits buffer."""
    ext = _ext()
    more = (ctypes.c_int32 * (produced + 1))()
    assert ext.lib().tl_engine_read_tokens(eng._h, slot, produced + 1, more) == TL_ERR_INVALID, "more ids are readable than were produced"
    return dict(pending=eng.read_pending(slot + 1)[slot], ids=eng.read_tokens(slot, produced), logits=eng.logits(1).clone())


def test_embed_leaves_the_decode_state_alone_and_the_slot_usable(tiny):
    ext = _ext()
    eng = _engine(tiny["model"])
    ref = O.OracleQwen3(TINY_CFG, tiny["weights"])
    truth = O.TruthQwen3(TINY_CFG, tiny["weights"])
    try:
        prompt, more = tiny["prompts"][64][:20], tiny["prompts"][64][20:31]
        # a decoding sequence in slot 0 while slot 1 embeds
        eng.begin(0)
        eng.prefill(0, tiny["prompts"][5])
        eng.decode(2, batch=1)
        before, ctx, pages = _state(eng, 0, 3), eng.context_len(0), eng.stats()["pages_in_use"]
        for pooling in ("mean", "last"):
            vec = eng.embed(tiny["prompts"][200], slot=1, pooling=pooling)
            assert abs(float(np.linalg.norm(vec.astype(np.float64))) - 1.0) < 1e-5
        after = _state(eng, 0, 3)
        assert after["pending"] == before["pending"] and after["ids"] == before["ids"] and torch.equal(after["logits"], before["logits"])
        assert eng.context_len(0) == ctx and eng.stats()["pages_in_use"] == pages
        # ... and the embedded slot itself: a finishing chunk into slot 0, which holds a pending token and three produced ids
        out = (ctypes.c_float * 256)()
        tail = tiny["prompts"][64][:9]
        ext.check(ext.lib().tl_engine_embed(eng._h, 0, (ctypes.c_int32 * 9)(*tail), 9, 1, ext.POOL_LAST, 1, 256, out))
        assert abs(float(np.linalg.norm(np.array(out[:], dtype=np.float64))) - 1.0) < 1e-5
        after = _state(eng, 0, 3)
        assert after["pending"] == before["pending"] and after["ids"] == before["ids"] and torch.equal(after["logits"], before["logits"])
        assert eng.context_len(0) == ctx + 9  # the context is what the call extends, like a prefill without logits
        eng.release(0)
        # finish = 0 only appends K/V: the slot then prefills and decodes like any other
        eng.begin(0)
        arr = (ctypes.c_int32 * len(prompt))(*prompt)
        ext.check(ext.lib().tl_engine_embed(eng._h, 0, arr, len(prompt), 0, ext.POOL_LAST, 1, 256, None))
        assert eng.context_len(0) == len(prompt)
        eng.prefill(0, more)
        got = [eng.logits(1)[0].float().cpu().numpy()]
        want, exact = [ref.forward(prompt + more)[0, -1]], [truth.forward(prompt + more)[0, -1]]
        for _ in range(2):
            tok = int(np.argmax(want[-1]))
            want.append(ref.forward([tok])[0, -1])
            exact.append(truth.forward([tok])[0, -1])
            eng.set_token(0, tok)
            eng.decode(1, batch=1)
            got.append(eng.logits(1)[0].float().cpu().numpy())
        check_against_truth(np.stack(got), np.stack(want), np.stack(exact), what="prefill + decode after an embed chunk without finish")
        eng.release(0)
        assert eng.stats()["pages_in_use"] == 0
    finally:
        eng.close()


def test_mean_state_and_invalid_arguments(tiny):
    ext = _ext()
    lib = ext.lib()
    eng = _engine(tiny["model"], prefix_cache=True, swap_pages=32)
    try:
        prompt, long = tiny["prompts"][64], tiny["prompts"][200]
        arr = (ctypes.c_int32 * 64)(*prompt)
        out = (ctypes.c_float * 256)()
        embed = lambda slot, n, finish, pooling, dim=256, tokens=arr, o=out: lib.tl_engine_embed(eng._h, slot, tokens, n, finish, pooling, 1, dim, o)
        MEAN, LAST = ext.POOL_MEAN, ext.POOL_LAST

        def refused(call, slot):
            ctx, pages = eng.context_len(slot), eng.stats()["pages_in_use"]
            assert call() == TL_ERR_INVALID
            assert eng.context_len(slot) == ctx and eng.stats()["pages_in_use"] == pages

        # seed the prefix cache with the first 64 tokens of the long prompt, then embed its first 80
        eng.begin(0)
        eng.prefill(0, long[:64], want_logits=False)
        eng.release(0)
        # MEAN after prefix_attach
        eng.begin(0)
        matched = eng.prefix_attach(0, long[:80])
        assert 48 <= matched <= 64
        refused(lambda: embed(0, 4, 1, MEAN, tokens=(ctypes.c_int32 * 4)(*long[matched:matched + 4])), 0)
        # LAST after the same hit embeds from the remaining tokens, inside the truth band (row 79 of the long prompt's rows: causal)
        rest = long[matched:80]
        ext.check(lib.tl_engine_embed(eng._h, 0, (ctypes.c_int32 * len(rest))(*rest), len(rest), 1, LAST, 0, 256, out))
        got = np.array(out[:], dtype=np.float32)
        check_against_truth(got[None], tiny["oracle"]["bf16"][200][79][None], tiny["truth"][200][79][None], what="embed last after a prefix-cache hit")
        eng.release(0)
        eng.set_prefix_cache(False)

        # MEAN chunks continue each other; a fork, a rewind, a prefill, a decode step, a move, park / unpark break the chain
        eng.begin(0)
        assert embed(0, 16, 0, MEAN) == 0
        assert embed(0, 16, 0, MEAN, tokens=(ctypes.c_int32 * 16)(*prompt[16:32])) == 0
        eng.fork(0, 1)
        refused(lambda: embed(1, 8, 1, MEAN), 1)
        assert embed(0, 8, 0, MEAN, tokens=(ctypes.c_int32 * 8)(*prompt[32:40])) == 0  # the source of the fork goes on
        eng.rewind(0, 8)
        refused(lambda: embed(0, 8, 1, MEAN), 0)
        eng.release(1)
        eng.move(0, 1)
        refused(lambda: embed(1, 8, 1, MEAN), 1)
        eng.release(1)
        eng.begin(0)
        eng.prefill(0, prompt[:9])
        refused(lambda: embed(0, 8, 1, MEAN), 0)
        eng.release(0)
        eng.begin(0)
        assert embed(0, 16, 0, MEAN) == 0
        eng.set_token(0, 5)
        eng.decode(1, batch=1)
        refused(lambda: embed(0, 8, 1, MEAN), 0)
        eng.release(0)
        eng.begin(0)
        assert embed(0, 16, 0, MEAN) == 0
        eng.park(0)
        refused(lambda: embed(0, 8, 1, MEAN), 0)  # parked
        refused(lambda: embed(0, 8, 1, LAST), 0)
        eng.unpark(0)
        refused(lambda: embed(0, 8, 1, MEAN), 0)
        assert embed(0, 8, 1, LAST) == 0  # LAST has no such rule
        eng.release(0)

        # invalid arguments: TL_ERR_INVALID, nothing changed
        eng.begin(0)
        eng.begin(1)
        bad_ids = (ctypes.c_int32 * 4)(1, 2, TINY_CFG["vocab_size"], 3)
        neg_ids = (ctypes.c_int32 * 4)(1, -2, 3, 4)
        for call in (lambda: embed(0, 8, 1, 2), lambda: embed(0, 8, 1, -1), lambda: embed(0, 8, 1, LAST, dim=0), lambda: embed(0, 8, 1, LAST, dim=257),
                     lambda: embed(0, 8, 1, LAST, tokens=None), lambda: embed(0, 8, 1, LAST, o=None), lambda: embed(0, 0, 1, LAST),
                     lambda: embed(0, 4, 1, LAST, tokens=bad_ids), lambda: embed(0, 4, 1, MEAN, tokens=neg_ids), lambda: embed(0, 513, 1, LAST),
                     lambda: embed(3, 8, 1, LAST), lambda: embed(-1, 8, 1, LAST), lambda: embed(4, 8, 1, LAST)):
            refused(call, 0)
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        toks = (ctypes.c_int32 * 8)(*prompt[:8])
        packed = lambda n=2, slots=ints(0, 1), tokens=toks, lens=ints(4, 4), finish=ints(1, 1), pooling=LAST, dim=256, o=out: \
            lib.tl_engine_embed_packed(eng._h, n, slots, tokens, lens, finish, pooling, 1, dim, o)
        bad8 = (ctypes.c_int32 * 8)(*prompt[:7], TINY_CFG["vocab_size"])
        for call in (lambda: packed(slots=ints(1, 1)), lambda: packed(slots=ints(0, 3)), lambda: packed(pooling=7), lambda: packed(dim=0),
                     lambda: packed(dim=300), lambda: packed(tokens=None), lambda: packed(slots=None), lambda: packed(lens=None),
                     lambda: packed(finish=None), lambda: packed(o=None), lambda: packed(n=0), lambda: packed(n=17), lambda: packed(lens=ints(4, 0)),
                     lambda: packed(tokens=bad8), lambda: packed(lens=ints(4, 600))):
            refused(call, 0)
            assert eng.context_len(1) == 0
        assert packed(finish=ints(0, 0), o=None) == 0  # nothing finishes: no output needed, only enqueued
        assert eng.context_len(0) == 4 and eng.context_len(1) == 4
        eng.park(1)
        refused(lambda: packed(), 0)
        eng.unpark(1)
        eng.release(0)
        eng.release(1)
        assert eng.stats()["pages_in_use"] == 0
    finally:
        eng.close()


def test_embed_ids_on_the_engine_and_the_page_accounting(tiny):
    from tiny_llm_hip.embedding import embed_ids

    eng = _engine(tiny["model"], max_prefill_rows=128, num_pages=40, prefix_cache=True)
    try:
        prompts = [tiny["prompts"][5], tiny["prompts"][200], tiny["others"][1], tiny["prompts"][64], tiny["others"][0], tiny["others"][2]]
        before = eng.stats()
        for pooling in ("mean", "last", "last"):  # (the second "last" run finds the first one's pages in the prefix cache)
            got = embed_ids(eng, prompts, pooling=pooling, normalize=False)
            assert got.shape == (6, 256) and got.dtype == np.float32
            for row, n in ((0, 5), (1, 200), (3, 64)):
                check_against_truth(got[row][None], E.pool(tiny["oracle"]["bf16"][n], pooling, normalize=False)[None],
                                    E.pool(tiny["truth"][n], pooling, normalize=False)[None], what=f"embed_ids {pooling}, {n} tokens")
            after = eng.stats()
            assert after["pages_in_use"] == before["pages_in_use"] == 0
            assert after["pages_in_use"] + after["pages_free"] + eng.prefix_stats()["pages_retained"] == 40
        assert eng.prefix_stats()["hits"] > 0
        eng.prefix_clear()
        assert eng.stats()["pages_free"] == before["pages_free"]
        unit = embed_ids(eng, prompts[:2], dim=32)
        assert np.allclose(np.linalg.norm(unit.astype(np.float64), axis=1), 1.0, atol=1e-5)
        with pytest.raises(RuntimeError, match="can never fit"):
            embed_ids(eng, [list(range(1, 700))])
        assert eng.stats()["pages_in_use"] == 0
    finally:
        eng.close()


def test_an_engine_that_never_embeds_allocates_nothing(tiny):
    a, b = _engine(tiny["model"]), _engine(tiny["model"])
    try:
        hidden, base = TINY_CFG["hidden_size"], a.stats()["workspace_bytes"]
        assert b.stats()["workspace_bytes"] == base
        b.embed(tiny["prompts"][5], pooling="last")
        assert b.stats()["workspace_bytes"] == base + 16 * hidden * 4  # the vectors of one call [16, hidden] fp32
        b.embed(tiny["prompts"][5], pooling="mean")
        assert b.stats()["workspace_bytes"] == base + 16 * hidden * 4 + 4 * hidden * 4  # + the running sums [max_batch, hidden] fp32
        b.embed(tiny["prompts"][64], pooling="mean")
        assert b.stats()["workspace_bytes"] == base + 20 * hidden * 4
        assert a.stats()["workspace_bytes"] == base
    finally:
        a.close()
        b.close()


# ---- one real-shape case ---------------------------------------------------------------------------------------------------------------------
def test_qwen3_4b_shaped_embedding():
    """hidden 2560 / 32 + 8 heads / intermediate 9728 with 1 layer and a 2,048-token vocabulary (the numpy oracles take seconds per layer
    at this width, and the float64 truth dequantises the whole embedding table): a 300-token prompt, last and mean, dim 2560 and 1024."""
    cfg = dict(QWEN4B_CFG, num_hidden_layers=1, vocab_size=2048)
    weights = O.make_fast_w4_weights(cfg, seed=7)
    prompt = [int(t) for t in np.random.default_rng(1).integers(1, cfg["vocab_size"], size=300)]
    rows_o = E.final_rows(O.OracleQwen3, cfg, weights, prompt)
    rows_t = E.final_rows(O.TruthQwen3, cfg, weights, prompt)
    eng = _engine(to_mlx_shaped(cfg, weights), page_size=128, num_pages=8, max_batch=2, max_prefill_rows=512)
    try:
        for pooling in ("last", "mean"):
            raw = eng.embed(prompt, slot=1, pooling=pooling, normalize=False)
            check_against_truth(raw[None], E.pool(rows_o, pooling, normalize=False)[None], E.pool(rows_t, pooling, normalize=False)[None],
                                what=f"Qwen3-4B-shaped embed {pooling}, 300 tokens")
            for dim in (2560, 1024):
                got = eng.embed(prompt, slot=1, pooling=pooling, normalize=True, dim=dim)
                want = E.finish(raw, dim, True)
                assert_within(got, want, np.abs(want) * dim * 2.0 ** -24, f"finish {pooling} dim {dim}")
                assert abs(float(np.linalg.norm(got.astype(np.float64))) - 1.0) < 1e-5
    finally:
        eng.close()
