"""CPU tier: text embeddings without a GPU -- the identity-head route to the oracles' final-norm rows (tests/embedding_oracle.py) against a
third-party implementation, the properties of the numpy pooling oracle, the batch scheduler ``tiny_llm_hip.embedding.embed_ids`` against a
recording fake engine, and the Python argument validation."""

import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import embedding_oracle as E
from helpers import TINY_CFG
from oracle import tiny_oracle as O


# ---- the identity head ---------------------------------------------------------------------------------------------------------------
def test_identity_head_rows_of_the_truth_agree_with_transformers_last_hidden_state():
    transformers = pytest.importorskip("transformers")
    import torch

    import test_truth_vs_transformers_cpu as T

    cfg, seed = dict(TINY_CFG), 3
    w = O.make_qwen3_weights(cfg, seed=seed, sigma=0.05)
    hf_cfg = transformers.Qwen3Config(**T.hf_common(cfg))
    hf_cfg._attn_implementation = "eager"
    model = transformers.Qwen3ForCausalLM(hf_cfg).double().eval()
    tensors = T.attention_and_norm_tensors(w)
    for i, lw in enumerate(w["layers"]):
        for name, key in (("mlp.gate_proj", "gate"), ("mlp.up_proj", "up"), ("mlp.down_proj", "down")):
            tensors[f"model.layers.{i}.{name}.weight"] = T.dense64(lw[key])
    T.load_exactly(model, tensors)
    prompt = [int(t) for t in np.random.default_rng(seed).integers(1, cfg["vocab_size"], size=29)]
    with torch.no_grad():
        want = model.model(torch.tensor([prompt])).last_hidden_state[0].numpy()
    got = E.final_rows(O.TruthQwen3, cfg, w, prompt)
    assert got.shape == want.shape == (29, cfg["hidden_size"])
    worst = float(np.abs(got - want).max())
    print(f"max |truth identity-head rows - transformers last_hidden_state| = {worst:.3e}")
    assert worst < 5e-6, worst  # the tolerance of test_float64_truth_agrees_with_transformers_qwen3


def test_identity_head_rows_of_the_bf16_oracle_are_exact_bf16_values():
    cfg = dict(TINY_CFG)
    w = O.make_qwen3_weights(cfg, seed=3, sigma=0.05)
    prompt = [int(t) for t in np.random.default_rng(5).integers(1, cfg["vocab_size"], size=37)]
    rows = E.final_rows(O.OracleQwen3, cfg, w, prompt)
    assert rows.shape == (37, cfg["hidden_size"])
    assert np.array_equal(O.bf16(rows.astype(np.float32)).astype(np.float64), rows)
    truth = E.final_rows(O.TruthQwen3, cfg, w, prompt)
    for pooling, bound in (("last", 1e-2), ("mean", 1e-2)):  # (measured 1.4e-3 / 7e-4: one bf16 pipeline error on components of ~0.06)
        d = float(np.abs(E.pool(rows, pooling) - E.pool(truth, pooling)).max())
        print(f"{pooling}: max |normalised oracle - truth| = {d:.2e}")
        assert 0 < d < bound


# ---- the pooling oracle -----------------------------------------------------------------------------------------------------------------
def test_pooling_oracle_properties():
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((11, 256))
    for pooling in ("last", "mean"):
        full = E.pool(rows, pooling)
        assert abs(np.linalg.norm(full) - 1.0) < 1e-12
        raw = E.pool(rows, pooling, normalize=False)
        assert np.allclose(raw, rows[-1] if pooling == "last" else rows.mean(0), rtol=0, atol=1e-15)
        cut = E.pool(rows, pooling, dim=100)
        assert cut.shape == (100,) and abs(np.linalg.norm(cut) - 1.0) < 1e-12  # a truncated vector is renormalised
        assert np.allclose(cut, raw[:100] / np.linalg.norm(raw[:100]), rtol=0, atol=1e-15)
        assert np.array_equal(E.pool(rows, pooling, dim=100, normalize=False), raw[:100])
    assert np.array_equal(E.pool(np.zeros((3, 128)), "mean"), np.zeros(128))  # a zero vector maps to zeros
    assert np.array_equal(E.finish(np.zeros(8), 4), np.zeros(4))
    assert np.isnan(E.pool(np.array([[1.0, np.nan]]), "last")).all()
    # the allowance: nothing for an un-normalised last row, positive otherwise
    assert not E.pool_allowance(rows, "last", None, False).any()
    assert (E.pool_allowance(rows, "mean", 32, False) > 0).all() and (E.pool_allowance(rows, "last", 32, True) >= 0).all()


# ---- embed_ids against a recording fake engine -------------------------------------------------------------------------------------------
class FakeEngine:
    """The engine surface embed_ids uses, on the host: a page pool, slots, and 'vectors' that name the prompt they came from
    (component 0 = the sum of the tokens the slot was fed or attached, component 1 = how many)."""

    def __init__(self, *, max_batch=4, max_prefill_rows=32, page_size=8, num_pages=64, prefix_cache=False, cached_prefix=0, fail_pass=None):
        self.args = SimpleNamespace(hidden_size=8)
        self.max_batch, self.max_prefill_rows, self.page_size, self.num_pages = max_batch, max_prefill_rows, page_size, num_pages
        self.prefix_cache_enabled, self.cached_prefix, self.fail_pass = prefix_cache, cached_prefix, fail_pass
        self.live, self.calls, self.passes = {}, [], []

    def _pages(self, tokens):
        return -(-tokens // self.page_size)

    def pages_in_use(self):
        return sum(self._pages(len(t)) for t in self.live.values())

    def step_pages(self, batch):
        return 0, self.num_pages - self.pages_in_use()

    def begin(self, slot):
        assert slot not in self.live and 0 <= slot < self.max_batch
        self.live[slot] = []
        self.calls.append(("begin", slot))

    def release(self, slot):
        assert slot in self.live
        del self.live[slot]
        self.calls.append(("release", slot))

    def prefix_attach(self, slot, tokens):
        assert self.prefix_cache_enabled and self.live[slot] == []
        m = min(self.cached_prefix, len(tokens) - 1)
        self.live[slot] = list(tokens[:m])
        self.calls.append(("attach", slot, m))
        return m

    def embed_packed(self, chunks, *, pooling, normalize, dim):
        if self.fail_pass is not None and len(self.passes) == self.fail_pass:
            raise RuntimeError("the pass failed")
        assert 1 <= len(chunks) <= 16 and len({c[0] for c in chunks}) == len(chunks)
        assert sum(len(c[1]) for c in chunks) <= self.max_prefill_rows and all(len(c[1]) >= 1 for c in chunks)
        self.passes.append([(slot, list(toks), bool(ends)) for slot, toks, ends in chunks])
        out = []
        for slot, toks, ends in chunks:
            self.live[slot] += list(toks)
            if ends:
                v = np.zeros(dim, dtype=np.float32)
                v[0], v[1] = sum(self.live[slot]), len(self.live[slot])
                out.append(v)
        assert self.pages_in_use() <= self.num_pages
        return np.stack(out) if out else np.zeros((0, dim), dtype=np.float32)


def _prompts(lengths, seed=0):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(1, 500, size=n)] for n in lengths]


def _check_vectors(out, prompts):
    assert out.dtype == np.float32 and out.shape[0] == len(prompts)
    for row, p in zip(out, prompts):
        assert (row[0], row[1]) == (sum(p), len(p))


def test_embed_ids_keeps_input_order_and_respects_the_pass_limits():
    from tiny_llm_hip.embedding import embed_ids

    lengths = [5, 31, 1, 17, 40, 3, 3, 3, 3, 3, 3, 64, 2, 9, 33, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 1, 1, 1, 1, 1, 1]
    prompts = _prompts(lengths)
    eng = FakeEngine(max_batch=20, max_prefill_rows=32, page_size=8, num_pages=64)
    out = embed_ids(eng, prompts, pooling="mean", normalize=False, dim=4)
    assert out.shape == (len(prompts), 4)
    _check_vectors(out, prompts)
    assert all(len(p) <= 16 and sum(len(c[1]) for c in p) <= 32 for p in eng.passes)
    assert max(len(p) for p in eng.passes) > 4  # several sequences do share a pass
    assert not eng.live and not any(c[0] == "attach" for c in eng.calls)
    # 17 one-token prompts on 20 slots: never more than 16 in a pass
    eng = FakeEngine(max_batch=20, max_prefill_rows=64)
    out = embed_ids(eng, _prompts([1] * 17), dim=2)
    assert [len(p) for p in eng.passes] == [16, 1]


def test_embed_ids_splits_a_long_prompt_and_its_remainder_leads_the_next_pass():
    from tiny_llm_hip.embedding import embed_ids

    prompts = _prompts([10, 70, 4])
    eng = FakeEngine(max_batch=4, max_prefill_rows=32, page_size=8, num_pages=64)
    out = embed_ids(eng, prompts, dim=3)
    _check_vectors(out, prompts)
    p = eng.passes
    assert [(len(c[1]), c[2]) for c in p[0]] == [(10, True), (22, False)]
    split_slot = p[0][1][0]
    assert [(c[0], len(c[1]), c[2]) for c in p[1]] == [(split_slot, 32, False)]
    assert (p[2][0][0], len(p[2][0][1]), p[2][0][2]) == (split_slot, 16, True)  # the remainder comes first ...
    assert [(len(c[1]), c[2]) for c in p[2][1:]] == [(4, True)]  # ... and the next prompt fills the room behind it
    assert p[0][1][1] + p[1][0][1] + p[2][0][1] == prompts[1]


def test_embed_ids_admits_only_what_the_pages_allow_and_refuses_what_can_never_fit():
    from tiny_llm_hip.embedding import embed_ids

    # 6 pages of 8 tokens: two 20-token prompts (3 pages each) fit together, the third waits for the next pass
    prompts = _prompts([20, 20, 20])
    eng = FakeEngine(max_batch=4, max_prefill_rows=64, page_size=8, num_pages=6)
    out = embed_ids(eng, prompts, dim=2)
    _check_vectors(out, prompts)
    assert [len(p) for p in eng.passes] == [2, 1]
    # a split prompt keeps its pages promised: nothing else is admitted into pages it will need
    eng = FakeEngine(max_batch=4, max_prefill_rows=16, page_size=8, num_pages=6)
    out = embed_ids(eng, _prompts([40, 8]), dim=2)
    assert [[len(c[1]) for c in p] for p in eng.passes] == [[16], [16], [8, 8]]
    eng = FakeEngine(max_batch=4, max_prefill_rows=64, page_size=8, num_pages=6)
    with pytest.raises(RuntimeError, match="can never fit"):
        embed_ids(eng, _prompts([8, 49]), dim=2)
    assert not eng.live  # what was begun has been released
    # longer than a sequence can be (max_pages_per_seq * page_size): refused before anything is begun
    eng = FakeEngine(max_batch=4, max_prefill_rows=64, page_size=8, num_pages=64)
    eng.max_pages_per_seq = 4
    with pytest.raises(RuntimeError, match="can never fit"):
        embed_ids(eng, _prompts([8, 33]), dim=2)
    assert not eng.calls
    _check_vectors(embed_ids(eng, _prompts([8, 32]), dim=2), _prompts([8, 32]))


def test_embed_ids_releases_every_slot_on_error():
    from tiny_llm_hip.embedding import embed_ids

    eng = FakeEngine(max_batch=4, max_prefill_rows=32, fail_pass=1)
    with pytest.raises(RuntimeError, match="the pass failed"):
        embed_ids(eng, _prompts([10, 70, 4]), dim=2)
    assert not eng.live
    begun = [c[1] for c in eng.calls if c[0] == "begin"]
    assert sorted(begun) == sorted(c[1] for c in eng.calls if c[0] == "release")


def test_embed_ids_attaches_cached_prefixes_for_last_and_never_for_mean():
    from tiny_llm_hip.embedding import embed_ids

    prompts = _prompts([12, 30, 5])
    eng = FakeEngine(max_batch=4, max_prefill_rows=64, prefix_cache=True, cached_prefix=8)
    out = embed_ids(eng, prompts, pooling="last", dim=2)
    _check_vectors(out, prompts)
    assert [c[2] for c in eng.calls if c[0] == "attach"] == [8, 8, 4]
    assert [len(c[1]) for c in eng.passes[0]] == [4, 22, 1]  # only the remaining tokens run
    eng = FakeEngine(max_batch=4, max_prefill_rows=64, prefix_cache=True, cached_prefix=8)
    _check_vectors(embed_ids(eng, prompts, pooling="mean", dim=2), prompts)
    assert not any(c[0] == "attach" for c in eng.calls)
    eng = FakeEngine(max_batch=4, max_prefill_rows=64, prefix_cache=False, cached_prefix=8)
    embed_ids(eng, prompts, pooling="last", dim=2)
    assert not any(c[0] == "attach" for c in eng.calls)


# ---- Python argument validation ------------------------------------------------------------------------------------------------------------
def test_python_argument_validation(monkeypatch):
    import torch

    import tiny_llm_ext_hip as ext
    import tiny_llm_hip.engine as EN
    from tiny_llm_hip.embedding import embed_ids, format_query, text_ids

    assert ext.pooling_args("last", True, None, 256) == (ext.POOL_LAST, 1, 256)
    assert ext.pooling_args("mean", False, 32, 256) == (ext.POOL_MEAN, 0, 32)
    for bad in (dict(pooling="cls"), dict(pooling=1), dict(dim=0), dict(dim=257), dict(dim=2.0), dict(dim=True), dict(normalize="yes")):
        with pytest.raises(ValueError):
            ext.pooling_args(**{**dict(pooling="last", normalize=True, dim=None, hidden=256), **bad})
    with pytest.raises(ValueError):
        ext.pool_rows(torch.zeros(4, 128, dtype=torch.bfloat16), [(0, 4)])  # host tensor: the extension is GPU-only

    class Lib:
        def __init__(self):
            self.calls = []

        def tl_engine_begin(self, h, slot):
            self.calls.append(("begin", slot))
            return 0

        def tl_engine_release(self, h, slot):
            self.calls.append(("release", slot))
            return 0

        def tl_engine_embed(self, h, slot, arr, n, finish, pooling, normalize, dim, out):
            self.calls.append(("embed", slot, [arr[i] for i in range(n)], finish, pooling, normalize, dim))
            if finish:
                for i in range(dim):
                    out[i] = float(i)
            return 0

    lib = Lib()
    monkeypatch.setattr(EN, "_lib", lib)
    eng = EN.DecodeEngine.__new__(EN.DecodeEngine)
    eng._h, eng.max_prefill_rows, eng.args = None, 8, SimpleNamespace(hidden_size=16)
    got = eng.embed(list(range(1, 11)), slot=1, pooling="mean", normalize=False, dim=4, chunk=4)
    assert got.dtype == np.float32 and got.tolist() == [0.0, 1.0, 2.0, 3.0]
    assert lib.calls == [("begin", 1), ("embed", 1, [1, 2, 3, 4], 0, 1, 0, 4), ("embed", 1, [5, 6, 7, 8], 0, 1, 0, 4),
                         ("embed", 1, [9, 10], 1, 1, 0, 4), ("release", 1)]
    for kwargs in (dict(chunk=0), dict(chunk=9), dict(pooling="cls"), dict(dim=17), dict(dim=0)):
        with pytest.raises(ValueError):
            eng.embed([1, 2, 3], **kwargs)
    with pytest.raises(ValueError):
        eng.embed([])
    with pytest.raises(ValueError):
        eng.embed_packed([])
    with pytest.raises(ValueError):
        eng.embed_packed([(0, [1], True)] * 17)
    assert [c[0] for c in lib.calls].count("begin") == 1  # nothing was begun by the refused calls
    eng._h = None

    fake = FakeEngine()
    with pytest.raises(ValueError):
        embed_ids(fake, [[1, 2], []])
    with pytest.raises(ValueError):
        embed_ids(fake, [[1]], pooling="max")
    with pytest.raises(ValueError):
        embed_ids(fake, [[1]], dim=9)
    assert not fake.calls
    assert embed_ids(fake, [], dim=2).shape == (0, 2)

    assert format_query("Find it", "what is x") == "Instruct: Find it\nQuery:what is x"
    tok = SimpleNamespace(encode=lambda s: [ord(c) for c in s], convert_tokens_to_ids=lambda t: 151643 if t == "<|endoftext|>" else None)
    assert text_ids(tok, "ab") == [97, 98, 151643]
    assert text_ids(tok, "q", task="T", eos_id=7) == [ord(c) for c in "Instruct: T\nQuery:q"] + [7]
    with pytest.raises(ValueError):
        text_ids(SimpleNamespace(encode=lambda s: [1], convert_tokens_to_ids=lambda t: None), "a")


def test_cli_similarity_matrix_and_arguments():
    import embed_main

    m = embed_main.cosine_matrix(np.array([[3.0, 4.0], [6.0, 8.0], [-4.0, 3.0], [0.0, 0.0]]))
    assert np.allclose(m[:3, :3], [[1, 1, 0], [1, 1, 0], [0, 0, 1]], atol=1e-12) and not m[3].any() and not m[:, 3].any()
    with pytest.raises(SystemExit):
        embed_main.main(["--model", "m", "--texts-file", "f", "--pooling", "cls"])
    with pytest.raises(SystemExit):
        embed_main.main(["--model", "m", "--texts-file", "f", "--batch-size", "17"])
