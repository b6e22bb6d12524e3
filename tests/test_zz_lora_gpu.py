"""GPU tier: LoRA adapters -- the shrink / expand kernels over caller rows (tl_lora_rows, csrc/lora.h) against float64 numpy with a
per-element allowance (tests/lora_oracle.py), their independence of position and neighbours, and the engine with per-slot adapters
against the float64 truth over merged weights through the project's rule (helpers.check_against_truth): single and mixed batches,
eager and captured steps, chunked and packed prefill, verify / score / embed, FP8 pages, the untouched base program, the slot
lifecycle and the prefix cache's bypass."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import embedding_oracle as E
import lora_oracle as L
from helpers import TINY_CFG, TRUTH_FACTOR, assert_within, bf16_ulp, check_against_truth, log_softmax, to_mlx_shaped
from oracle import tiny_oracle as O

pytestmark = pytest.mark.gpu

TL_ERR_INVALID, TL_ERR_UNSUPPORTED = -1, -2
# hidden 2,560, intermediate 9,728, 32 / 8 heads: the column counts of Qwen3-4B (2,560, 4,096 and 9,728 all run), two layers, a small vocabulary
WIDE_CFG = dict(TINY_CFG, hidden_size=2560, intermediate_size=9728, num_attention_heads=32, num_key_value_heads=8)
PROMPT21 = [5, 17, 900, 33, 2, 77, 410, 3, 999, 64, 128, 256, 512, 31, 7, 1000, 15, 808, 42, 600, 11]


def _ext():
    import tiny_llm_ext_hip as ext

    return ext


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda", torch.bfloat16)


# ---- 1 / 2: the kernels over caller rows ---------------------------------------------------------------------------------------------
def _fused(rng, n_in, out_cols, rank, seg_mode, seg_ends, mask, scale):
    """One adapter in the fused layout, bf16 values as float32: A [rank * present, in], B [out, rank] (rows of a missing segment zero)."""
    present = bin(mask).count("1")
    a = O.bf16(rng.standard_normal((rank * present, n_in), dtype=np.float32) * 0.05)
    b = O.bf16(rng.standard_normal((out_cols, rank), dtype=np.float32) * 0.05)
    seg = L.segment_of(out_cols, seg_mode, seg_ends)
    for s in range(3):
        if not (mask >> s) & 1:
            b[seg == s] = 0.0
    return a, b, scale, mask


def _rows_case(seed, rows, n_in, out_cols, ranks, mode, seg_mode="plain", seg_ends=(0, 0), masks=None, norm=False, tiles=None, ids=None):
    ext = _ext()
    rng = np.random.default_rng(seed)
    n_seg = {"plain": 1, "blocks": 3, "interleaved": 2}[seg_mode]
    masks = masks or [(1 << n_seg) - 1] * len(ranks)
    adapters = [_fused(rng, n_in, out_cols, r, seg_mode, seg_ends, m, s) for r, m, s in zip(ranks, masks, (1.0, -0.5, 2.0, 0.75))]
    x = O.bf16(rng.standard_normal((rows, n_in), dtype=np.float32) * np.exp2(rng.integers(-2, 2, size=(rows, 1))).astype(np.float32))
    base = O.bf16(rng.standard_normal((rows, out_cols), dtype=np.float32))
    if ids is None:  # adapters mixed per row, -1 included
        ids = [(i % (len(ranks) + 1)) - 1 for i in range(rows)] if rows > 1 else [0]
    w = O.bf16(1.0 + 0.25 * rng.standard_normal(n_in, dtype=np.float32)) if norm else None
    want, allowed = L.lora_rows_reference(x, ids, adapters, base, mode=mode, seg_mode=seg_mode, seg_ends=seg_ends, norm_weight=w)
    got = ext.lora_rows(_dev(x), ids, [(_dev(a), _dev(b), s, m) for a, b, s, m in adapters], out_cols=out_cols, mode=mode, base=_dev(base),
                        seg_mode=seg_mode, seg_ends=seg_ends, tiles=tiles, norm_weight=_dev(w) if norm else None)
    got = got.float().cpu().numpy()
    assert_within(got, want, allowed, f"lora_rows {mode} rows {rows} in {n_in} out {out_cols} ranks {ranks} {seg_mode} norm {norm}")
    return got, ids, base


@pytest.mark.parametrize("rows", [1, 2, 5, 16, 17, 64, 65, 130])
def test_lora_rows_every_row_count_mixed_adapters_two_ranks(rows):
    for norm in (False, True):
        got, ids, base = _rows_case(rows, rows, 256, 256, [16, 8], "add", norm=norm)
        for i, a in enumerate(ids):  # a row without an adapter keeps the base bit for bit
            if a < 0:
                assert np.array_equal(got[i], base[i]), i
        _rows_case(100 + rows, rows, 256, 256, [8, 24], "residual_pre", norm=norm)


@pytest.mark.parametrize("n_in,out_cols,seg_mode,seg_ends,mode", [
    (2560, 6144, "blocks", (4096, 5120), "add"),           # qkv of Qwen3-4B
    (4096, 2560, "plain", (0, 0), "residual_pre"),         # wo
    (2560, 2 * 9728, "interleaved", (0, 0), "swiglu"),     # gate|up
    (9728, 2560, "plain", (0, 0), "residual_pre"),         # w_down
    (256, 256, "interleaved", (0, 0), "swiglu"),
])
@pytest.mark.parametrize("ranks", [[8, 64], [16, 24]])
def test_lora_rows_real_shapes_every_epilogue(n_in, out_cols, seg_mode, seg_ends, mode, ranks):
    for norm in (False, True):
        _rows_case(n_in + ranks[0], 19, n_in, out_cols, ranks, mode, seg_mode, seg_ends, norm=norm)


def test_lora_rows_missing_targets_are_skipped():
    # q, v only and up only: the missing segment's columns keep the base (its B rows are zero AND unread), its A rows do not exist
    got, ids, base = _rows_case(7, 20, 256, 768, [16, 8], "add", "blocks", (256, 512), masks=[0b101, 0b010])
    for i, a in enumerate(ids):
        if a == 0:
            assert np.array_equal(got[i, 256:512], base[i, 256:512]) and not np.array_equal(got[i, :256], base[i, :256])
        if a == 1:
            assert np.array_equal(got[i, :256], base[i, :256]) and np.array_equal(got[i, 512:], base[i, 512:])
    _rows_case(8, 20, 256, 512, [16, 8], "swiglu", "interleaved", masks=[0b10, 0b01])


def test_lora_rows_tile_lists_that_split_at_15_16_and_17():
    for cut in (15, 16, 17):
        # two sequences [0, cut) under adapter 0 and [cut, 40) under adapter 1, a third [40, 45) without, a fourth that looks its rows up
        tiles, ids = [], [0] * cut + [1] * (40 - cut) + [-1] * 5 + [1, -1, 0, 0, 1]
        for r0, r1, ad in ((0, cut, 0), (cut, 40, 1), (40, 45, -1), (45, 50, -2)):
            tiles += [(r, min(16, r1 - r), ad) for r in range(r0, r1, 16)]
        a, _, _ = _rows_case(cut, 50, 512, 256, [16, 8], "add", tiles=tiles, ids=ids)
        b, _, _ = _rows_case(cut, 50, 512, 256, [16, 8], "add", ids=ids)  # the same rows in blocks of 16 that look every row up
        assert np.array_equal(a, b)  # a row's result does not depend on its tile


@pytest.mark.parametrize("mode,seg_mode,norm", [("add", "blocks", True), ("residual_pre", "plain", False), ("swiglu", "interleaved", True)])
def test_a_rows_result_depends_on_the_row_alone(mode, seg_mode, norm):
    ext = _ext()
    rng = np.random.default_rng(11)
    n_in, out_cols, ends = 2560, 768, (256, 512)
    adapters = [_fused(rng, n_in, out_cols, r, seg_mode, ends, (1 << {"plain": 1, "blocks": 3, "interleaved": 2}[seg_mode]) - 1, s)
                for r, s in ((16, 1.0), (64, 0.5), (8, -1.0))]
    zero = (adapters[0][0], np.zeros_like(adapters[0][1]), 1.0, adapters[0][3])  # an adapter whose B is all zeros
    dev = [(_dev(a), _dev(b), s, m) for a, b, s, m in adapters + [zero]]
    x = O.bf16(rng.standard_normal((64, n_in), dtype=np.float32))
    base = O.bf16(rng.standard_normal((64, out_cols), dtype=np.float32))
    w = _dev(O.bf16(1.0 + 0.25 * rng.standard_normal(n_in, dtype=np.float32))) if norm else None
    run = lambda xs, bs, ids: ext.lora_rows(_dev(xs), ids, dev, out_cols=out_cols, mode=mode, base=_dev(bs), seg_mode=seg_mode, seg_ends=ends,
                                            norm_weight=w).view(torch.int16).cpu().numpy()
    crowd_ids = [(i * 7) % 4 - 1 if i != 37 else 0 for i in range(64)]
    crowd_ids = [a if a < 3 else 1 for a in crowd_ids]
    crowd = run(x, base, crowd_ids)
    alone = run(x[37:38], base[37:38], [0])
    assert np.array_equal(crowd[37], alone[0])  # bitwise: alone and inside a 64-row launch of other adapters
    crowd_ids[37] = 2
    assert not np.array_equal(run(x, base, crowd_ids)[37], alone[0])
    none = run(x[:5], base[:5], [-1] * 5)
    assert np.array_equal(run(x[:5], base[:5], [3] * 5), none)  # a zero-B adapter row equals a row without an adapter, bitwise
    if mode != "swiglu":
        assert np.array_equal(none, _dev(base[:5]).view(torch.int16).cpu().numpy())


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name):
    cfg = TINY_CFG if name == "tiny" else WIDE_CFG
    weights = O.make_qwen3_weights(cfg, seed=3, sigma=0.05) if name == "tiny" else O.make_fast_w4_weights(cfg, seed=3, sigma=0.05)
    return cfg, weights, to_mlx_shaped(cfg, weights)


@functools.lru_cache(maxsize=None)
def _adapter(name, rank, targets=L.TARGETS, seed=0):
    return L.make_adapter(_model(name)[0], rank, targets=targets, seed=seed, sigma=0.05, scale=1.0)


ADAPTERS = {"X": ("tiny", 16, L.TARGETS, 0), "Y": ("tiny", 8, ("q", "v"), 1), None: None}


def _named(key):
    return None if key is None else _adapter(*ADAPTERS[key])


_DENSE: dict = {}


@functools.lru_cache(maxsize=None)
def _reference(name, adapter_key, prompt, steps, kv_format="bf16"):
    """(oracle rows, truth rows, greedy ids fed) of prompt + `steps` teacher-forced decode steps; adapter_key: None or _adapter's arguments."""
    cfg, weights, _ = _model(name)
    adapter = _adapter(*adapter_key) if adapter_key else None
    ref, truth = L.LoraOracleQwen3(cfg, weights, adapter, kv_format=kv_format), L.LoraTruthQwen3(cfg, weights, adapter)
    truth._dense = _DENSE.setdefault(name, {})  # (the float64 base weights are expanded once per model; the merged ones are the truth's own)
    want, exact, fed = [ref.forward(list(prompt))[0, -1]], [truth.forward(list(prompt))[0, -1]], []
    for _ in range(steps):
        fed.append(int(np.argmax(want[-1])))
        want.append(ref.forward([fed[-1]])[0, -1])
        exact.append(truth.forward([fed[-1]])[0, -1])
    return np.stack(want), np.stack(exact), fed


def _engine(name="tiny", **kw):
    from tiny_llm_hip.engine import DecodeEngine

    args = dict(page_size=128, num_pages=24, max_batch=1, max_prefill_rows=160)
    args.update(kw)
    return DecodeEngine(_model(name)[2], **args)


def _run(eng, prompt, fed, adapter_id, chunk=None, use_graph=True):
    """Logits [1 + len(fed), vocab] of slot 0: prefill (in chunks), then teacher-forced decode steps."""
    eng.begin(0)
    try:
        if adapter_id is not None:
            eng.set_lora(0, adapter_id)
        eng.prefill(0, list(prompt), chunk=chunk)
        got = [eng.logits(1)[0].float().cpu().numpy()]
        for token in fed:
            eng.set_token(0, token)
            eng.decode(1, batch=1, use_graph=use_graph)
            got.append(eng.logits(1)[0].float().cpu().numpy())
        return np.stack(got)
    finally:
        eng.release(0)


def _check_moved(got, name, adapter_key, prompt, steps, what):
    """The test that fails without the feature: the engine's logits moved with the adapter, at least half as far as the truth did."""
    want, exact, fed = _reference(name, adapter_key, prompt, steps)
    cfg, weights, _ = _model(name)
    truth0 = O.TruthQwen3(cfg, weights)  # the base model's truth over the same teacher-forced ids
    truth0._dense = _DENSE.setdefault(name, {})
    base_rows = [truth0.forward(list(prompt))[0, -1]]
    for token in fed:
        base_rows.append(truth0.forward([token])[0, -1])
    base_rows = np.stack(base_rows)
    moved_truth = float(np.abs(exact - base_rows).max())
    moved_got = float(np.abs(got - base_rows).max())
    print(f"{what}: the adapter moves the truth by {moved_truth:.4g}, the engine by {moved_got:.4g}")
    assert moved_got >= 0.5 * moved_truth, f"{what}: the engine's logits are {moved_got:.4g} from the base truth, the adapter's truth {moved_truth:.4g}"


@pytest.mark.parametrize("key", [("tiny", 16, L.TARGETS, 0), ("tiny", 16, ("q", "v"), 0), ("tiny", 64, L.TARGETS, 2)], ids=["r16-all", "r16-qv", "r64-all"])
def test_engine_with_an_adapter_against_the_truth(key):
    prompt, steps = tuple(PROMPT21), 6
    want, exact, fed = _reference("tiny", key, prompt, steps)
    eng = _engine()
    try:
        adapter = eng.load_lora(L.to_lora_adapter(_adapter(*key)))
        got = _run(eng, prompt, fed, adapter)
        check_against_truth(got, want, exact, what=f"engine with adapter {key[1:3]}, 21 + 6", factor=TRUTH_FACTOR)
        _check_moved(got, "tiny", key, prompt, steps, f"adapter {key[1:3]}")
        stats = eng.lora_stats()
        assert stats["resident"] == 1 and stats["adapter_steps"] == steps and stats["adapter_prefill_rows"] == len(prompt)
        assert stats["bytes"] >= L.to_lora_adapter(_adapter(*key)).nbytes()
        assert "LoRA" not in eng.replay_route()  # no adapter slot is live any more
    finally:
        eng.close()


PROMPT135 = tuple(int(t) for t in np.random.default_rng(5).integers(0, TINY_CFG["vocab_size"], size=135))


@pytest.mark.parametrize("chunk", [1, 15, 16, 17, 130])
def test_engine_prefill_in_chunks_with_an_adapter(chunk):
    key = ("tiny", 16, L.TARGETS, 0)
    want, exact, fed = _reference("tiny", key, PROMPT135, 2)
    eng = _engine()
    try:
        adapter = eng.load_lora(L.to_lora_adapter(_adapter(*key)))
        got = _run(eng, PROMPT135, fed, adapter, chunk=chunk)  # (130 + 5: the first chunk crosses the 128-token page)
        check_against_truth(got, want, exact, what=f"adapter prefill in chunks of {chunk}", factor=TRUTH_FACTOR)
        _check_moved(got, "tiny", key, PROMPT135, 2, f"chunks of {chunk}")
    finally:
        eng.close()


def test_engine_real_widths():
    key = ("wide", 16, L.TARGETS, 0)
    prompt, steps = tuple(PROMPT21), 6
    want, exact, fed = _reference("wide", key, prompt, steps)
    eng = _engine("wide", num_pages=4)
    try:
        adapter = eng.load_lora(L.to_lora_adapter(_adapter(*key)))
        got = _run(eng, prompt, fed, adapter)
        check_against_truth(got, want, exact, what="engine with a rank-16 adapter at Qwen3-4B widths", factor=TRUTH_FACTOR)
        _check_moved(got, "wide", key, prompt, steps, "Qwen3-4B widths")
    finally:
        eng.close()


CYCLE = ["X", None, "Y", "X", None]


def _mixed_prompt(i):
    return tuple(int(t) for t in np.random.default_rng(100 + i).integers(0, TINY_CFG["vocab_size"], size=3 + (i * 5) % 11))


@pytest.mark.parametrize("batch", [1, 4, 5, 17])
def test_mixed_batches_eager_and_captured(batch):
    steps = 3
    keys = [CYCLE[i % len(CYCLE)] for i in range(batch)]
    refs = [_reference("tiny", ADAPTERS[k], _mixed_prompt(i), steps) for i, k in enumerate(keys)]
    eng = _engine(max_batch=batch, num_pages=batch + 2)
    try:
        ids = {"X": eng.load_lora(L.to_lora_adapter(_named("X"))), "Y": eng.load_lora(L.to_lora_adapter(_named("Y"))), None: None}
        runs = {}
        for use_graph in (0, 1):
            for s in range(batch):
                eng.begin(s)
                if keys[s] is not None:
                    eng.set_lora(s, ids[keys[s]])
                eng.prefill(s, list(_mixed_prompt(s)))
            assert "LoRA" in eng.replay_route() or not eng.replay_route().startswith("aql")  # an adapter plan never rides the AQL route
            rows = []
            for k in range(steps):
                for s in range(batch):
                    eng.set_token(s, refs[s][2][k])
                eng.decode(1, batch=batch, use_graph=bool(use_graph))
                rows.append(eng.logits(batch).view(torch.int16).cpu().numpy())
            runs[use_graph] = np.stack(rows)  # [steps, batch, vocab] bits
            assert [eng.slot_lora(s) for s in range(batch)] == [-1 if k is None else ids[k] for k in keys]
            for s in range(batch):
                eng.release(s)
        assert eng.stats()["graph_replays"] >= steps and np.array_equal(runs[0], runs[1])  # the eager and the captured step: bitwise equal
        got = torch.from_numpy(runs[1]).view(torch.bfloat16).float().numpy()
        for s in range(batch):  # every slot against its OWN truth: the base truth for "none"
            want, exact, _ = refs[s]
            check_against_truth(got[:, s], want[1:], exact[1:], what=f"mixed batch of {batch}, slot {s} ({keys[s]})", factor=TRUTH_FACTOR)
    finally:
        eng.close()


def test_packed_prefill_three_sequences_three_adapters():
    lens, keys = (17, 1, 130), ("X", None, "Y")
    prompts = [tuple(int(t) for t in np.random.default_rng(200 + i).integers(0, TINY_CFG["vocab_size"], size=n)) for i, n in enumerate(lens)]
    eng = _engine(max_batch=3)
    try:
        ids = {"X": eng.load_lora(L.to_lora_adapter(_named("X"))), "Y": eng.load_lora(L.to_lora_adapter(_named("Y")))}
        for s in range(3):
            eng.begin(s)
            if keys[s]:
                eng.set_lora(s, ids[keys[s]])
        eng.prefill_packed([(s, list(prompts[s]), True) for s in range(3)])
        got = eng.logits(3).float().cpu().numpy()
        for s in range(3):
            want, exact, _ = _reference("tiny", ADAPTERS[keys[s]], prompts[s], 0)
            check_against_truth(got[s][None], want, exact, what=f"packed prefill, sequence {s} ({lens[s]} tokens, {keys[s]})", factor=TRUTH_FACTOR)
        assert eng.lora_stats()["adapter_prefill_rows"] == 17 + 130
    finally:
        eng.close()


def test_verify_score_and_embed_on_an_adapter_slot():
    key = ("tiny", 16, L.TARGETS, 0)
    cfg, weights, _ = _model("tiny")
    adapter = _adapter(*key)
    prompt, more = list(PROMPT21[:13]), list(PROMPT21[13:])
    eng = _engine(max_batch=8)
    try:
        aid = eng.load_lora(L.to_lora_adapter(adapter))
        # verify: 8 rows behind a 13-token prompt
        ref, truth = L.LoraOracleQwen3(cfg, weights, adapter), L.LoraTruthQwen3(cfg, weights, adapter)
        ref.forward(prompt), truth.forward(prompt)
        want, exact = ref.forward(more, None)[0], truth.forward(more, None)[0]
        eng.begin(0)
        eng.set_lora(0, aid)
        eng.prefill(0, prompt)
        out = eng.verify(0, more)
        got = eng.logits(8).float().cpu().numpy()
        check_against_truth(got, want, exact, what="verify on an adapter slot", factor=TRUTH_FACTOR)
        assert out == [int(np.argmax(r)) for r in got]
        eng.release(0)
        # score: the log-probability of every next token; the logits are bf16 on both sides, so a log-probability may lie as far from
        # the truth's as the logits rule lets two logits lie (the token's and, through the log-sum, the row's largest)
        tokens = list(PROMPT21)
        all_want = L.LoraOracleQwen3(cfg, weights, adapter).forward(tokens, None)[0]
        all_exact = L.LoraTruthQwen3(cfg, weights, adapter).forward(tokens, None)[0]
        lp_want, lp_exact = log_softmax(all_want), log_softmax(all_exact)
        nxt = np.array(tokens[1:])
        pick = lambda lp: lp[np.arange(len(nxt)), nxt].astype(np.float64)
        eng.begin(0)
        eng.set_lora(0, aid)
        arr, lp = (ctypes.c_int32 * len(tokens))(*tokens), (ctypes.c_float * len(tokens))()
        assert _ext().lib().tl_engine_score(eng._h, 0, arr, len(tokens), -1, lp, None) == 0
        eng.release(0)
        got_lp = np.array(list(lp)[:-1], dtype=np.float64)
        bound = 2 * (TRUTH_FACTOR * float(np.abs(all_want - all_exact).max()) + float(bf16_ulp(np.abs(all_exact).max())))
        assert float(np.abs(got_lp - pick(lp_exact)).max()) <= bound, (float(np.abs(got_lp - pick(lp_exact)).max()), bound)
        base_lp = pick(log_softmax(O.TruthQwen3(cfg, weights).forward(tokens, None)[0]))
        assert np.abs(got_lp - base_lp).max() >= 0.5 * np.abs(pick(lp_exact) - base_lp).max()
        # embed: the last token's final-norm row, not normalised
        from tiny_llm_hip.embedding import embed_ids

        rows_want = E.final_rows(L.LoraOracleQwen3, cfg, weights, tokens, adapter=adapter)
        rows_exact = E.final_rows(L.LoraTruthQwen3, cfg, weights, tokens, adapter=adapter)
        vec = embed_ids(eng, [tokens, tokens], pooling="last", normalize=False, lora=[aid, None])
        check_against_truth(vec[0][None], rows_want[-1][None], rows_exact[-1][None], what="embed on an adapter slot", factor=TRUTH_FACTOR)
        base_rows = E.final_rows(O.TruthQwen3, cfg, weights, tokens)
        check_against_truth(vec[1][None], E.final_rows(O.OracleQwen3, cfg, weights, tokens)[-1][None], base_rows[-1][None], what="embed beside it, base")
        assert np.abs(vec[0] - base_rows[-1]).max() >= 0.5 * np.abs(rows_exact[-1] - base_rows[-1]).max()
    finally:
        eng.close()


def test_fp8_pages_with_an_adapter():
    key = ("tiny", 16, L.TARGETS, 0)
    prompt, steps = tuple(PROMPT21), 3
    want, _, fed = _reference("tiny", key, prompt, steps, "fp8")
    _, exact, _ = _reference("tiny", key, prompt, 0)
    cfg, weights, _ = _model("tiny")
    truth = L.LoraTruthQwen3(cfg, weights, _adapter(*key))
    rows = [truth.forward(list(prompt))[0, -1]] + [truth.forward([t])[0, -1] for t in fed]
    eng = _engine(kv_format="fp8")
    try:
        got = _run(eng, prompt, fed, eng.load_lora(L.to_lora_adapter(_adapter(*key))))
        check_against_truth(got, want, np.stack(rows), what="FP8 pages with an adapter", factor=TRUTH_FACTOR)
    finally:
        eng.close()


def test_the_base_program_is_untouched_by_resident_adapters():
    prompt, fed = list(PROMPT21), _reference("tiny", None, tuple(PROMPT21), 4)[2]
    outs, profiles, routes = [], [], []
    for load in (False, True):
        eng = _engine(max_batch=4)
        try:
            if load:
                eng.load_lora(L.to_lora_adapter(_named("X")))
                eng.load_lora(L.to_lora_adapter(_named("Y")))
            else:
                assert eng.lora_stats() == {"resident": 0, "bytes": 0, "adapter_steps": 0, "adapter_prefill_rows": 0}
            eng.begin(0)
            eng.prefill(0, prompt)
            rows = [eng.logits(1).view(torch.int16).cpu().numpy()]
            for t in fed:
                eng.set_token(0, t)
                eng.decode(1, batch=1)
                rows.append(eng.logits(1).view(torch.int16).cpu().numpy())
            routes.append(eng.replay_route())
            prof = eng.profile_step(1)
            profiles.append({k: v["launches"] for k, v in prof["kinds"].items()})
            outs.append(np.stack(rows))
            assert eng.lora_stats()["adapter_steps"] == 0
            eng.release(0)
        finally:
            eng.close()
    assert np.array_equal(outs[0], outs[1])  # bit-identical logits
    assert routes[0] == routes[1] and profiles[0] == profiles[1]
    import os

    if os.environ.get("TL_AQL", "1") != "0":
        assert routes[1].startswith("aql"), routes[1]


def test_lifecycle():
    ext = _ext()
    lib = ext.lib()
    eng = _engine(max_batch=4, swap_pages=4)
    try:
        X, Y = L.to_lora_adapter(_named("X")), L.to_lora_adapter(_named("Y"))
        x = eng.load_lora(X)
        y = eng.load_lora(Y)
        assert (x, y) == (0, 1)
        with pytest.raises(RuntimeError, match="holds no sequence"):
            eng.set_lora(0, x)  # not a live slot
        eng.begin(0)
        assert eng.slot_lora(0) == -1
        with pytest.raises(RuntimeError, match="resident"):
            eng.set_lora(0, 5)
        eng.set_lora(0, x)
        eng.prefill(0, PROMPT21[:9])
        with pytest.raises(RuntimeError, match="already holds tokens"):
            eng.set_lora(0, y)  # refused after the first prefill
        with pytest.raises(RuntimeError, match="carries the adapter"):
            eng.unload_lora(x)  # in use
        eng.fork(0, 1)
        eng.move(0, 2)
        assert [eng.slot_lora(s) for s in range(4)] == [-1, x, x, -1]  # fork copies, move moves
        # park / unpark keep it, and the unparked twin produces the ids of the twin that never parked
        eng.park(1)
        assert eng.slot_lora(1) == x and eng.is_parked(1)
        eng.decode(2, batch=3)  # (slot 2 alone: slot 0 is free, slot 1 parked)
        straight = eng.read_tokens(2, 2)
        eng.release(2)
        eng.unpark(1)
        eng.decode(2, batch=3)
        assert eng.read_tokens(1, 2) == straight and eng.slot_lora(1) == x and eng.lora_stats()["adapter_steps"] == 4
        eng.release(1)
        assert [eng.slot_lora(s) for s in range(4)] == [-1] * 4  # release resets
        eng.begin(1)
        assert eng.slot_lora(1) == -1  # and so does begin
        eng.release(1)
        eng.unload_lora(x)  # works after release
        with pytest.raises(RuntimeError, match="no such adapter"):
            eng.unload_lora(x)
        assert eng.load_lora(Y) == x  # an unloaded id is reused
        ids = [eng.load_lora(Y) for _ in range(30)]
        assert sorted(ids + [x, y]) == list(range(32))
        with pytest.raises(RuntimeError, match="32 adapters"):
            eng.load_lora(Y)  # the 33rd
        assert eng.lora_stats()["resident"] == 32
        # the C interface's refusals: a bad rank, a null A with a non-null B
        hidden = TINY_CFG["hidden_size"]
        buf = torch.zeros(16 * hidden * 4, dtype=torch.bfloat16, device="cuda")
        layers = (ext.TlLoraLayer * TINY_CFG["num_hidden_layers"])()
        layers[0].a_dev[0], layers[0].b_dev[0] = buf.data_ptr(), buf.data_ptr()
        out = ctypes.c_int(-1)
        eng.unload_lora(ids[0])
        for rank in (0, 4, 12, 72):
            assert lib.tl_engine_lora_load(eng._h, layers, rank, 1.0, ctypes.byref(out)) == TL_ERR_INVALID
        assert lib.tl_engine_lora_load(eng._h, layers, 8, float("nan"), ctypes.byref(out)) == TL_ERR_INVALID
        layers[1].b_dev[3] = buf.data_ptr()
        assert lib.tl_engine_lora_load(eng._h, layers, 8, 1.0, ctypes.byref(out)) == TL_ERR_INVALID
        layers[1].b_dev[3] = None
        assert lib.tl_engine_lora_load(eng._h, layers, 8, 1.0, ctypes.byref(out)) == 0 and out.value == ids[0]
    finally:
        eng.close()


def test_mlp_targets_on_a_moe_layer_are_refused(tmp_path):
    from checkpoint_fixture import MOE_CFG_OVERRIDES, make_moe_weights, write_checkpoint
    from tiny_llm_hip import load
    from tiny_llm_hip.engine import DecodeEngine

    cfg = dict(TINY_CFG, **MOE_CFG_OVERRIDES)  # layer 0 dense, layers 1 and 2 sparse
    words = [f"w{i}" for i in range(cfg["vocab_size"] - 2)]
    model, _ = load(str(write_checkpoint(tmp_path / "ckpt", cfg, make_moe_weights(cfg, seed=21), vocab_words=words)))
    eng = DecodeEngine(model, page_size=16, num_pages=8, max_batch=1, max_prefill_rows=16)
    try:
        ext = _ext()
        buf = torch.zeros(8 * 4096, dtype=torch.bfloat16, device="cuda")
        out = ctypes.c_int(-1)
        for layer, target, status in ((1, 4, TL_ERR_UNSUPPORTED), (2, 6, TL_ERR_UNSUPPORTED), (0, 4, 0), (1, 0, 0), (2, 3, 0)):
            layers = (ext.TlLoraLayer * cfg["num_hidden_layers"])()
            layers[layer].a_dev[target], layers[layer].b_dev[target] = buf.data_ptr(), buf.data_ptr()
            assert ext.lib().tl_engine_lora_load(eng._h, layers, 8, 1.0, ctypes.byref(out)) == status, (layer, target)
        # attention targets on the sparse layers run: a zero adapter leaves the ids of the base model
        base = eng.generate([5, 17, 200, 33], 4)
        assert eng.generate([5, 17, 200, 33], 4, lora=out.value) == base and eng.lora_stats()["adapter_steps"] == 3
    finally:
        eng.close()


def test_prefix_cache_is_bypassed_by_adapter_slots():
    key = ("tiny", 16, L.TARGETS, 0)
    prompt = tuple(int(t) for t in np.random.default_rng(9).integers(0, TINY_CFG["vocab_size"], size=40))
    for adapter_first in (True, False):
        eng = _engine(page_size=16, num_pages=32, prefix_cache=True)
        try:
            aid = eng.load_lora(L.to_lora_adapter(_adapter(*key)))
            order = [aid, None] if adapter_first else [None, aid]
            for turn, lora in enumerate(order):
                before = eng.prefix_stats()
                ids = eng.generate(list(prompt), 3, lora=lora)
                after = eng.prefix_stats()
                matched = after["tokens_matched"] - before["tokens_matched"]
                if lora is not None:
                    # the adapter request attaches nothing -- also over a prompt the base request has cached -- and retains nothing
                    assert matched == 0 and after["pages_registered"] == before["pages_registered"] and after["pages_retained"] == before["pages_retained"]
                elif adapter_first:
                    assert matched == 0  # the base request finds nothing of the adapter request's pages
                assert len(ids) == 3
            # the base request's logits meet the base truth whichever came first
            want, exact, fed = _reference("tiny", None, prompt, 0)
            eng.begin(0)
            got_matched = eng.prefix_attach(0, list(prompt))
            # the base request of this engine did publish its full pages: 40 prompt + 2 fed answer tokens = two pages of 16
            assert got_matched == (len(prompt) + 2) // 16 * 16
            eng.prefill(0, list(prompt)[got_matched:])
            got = eng.logits(1).float().cpu().numpy()
            check_against_truth(got, want, exact, what=f"base request beside an adapter request (adapter first: {adapter_first})", factor=TRUTH_FACTOR)
            eng.release(0)
        finally:
            eng.close()
