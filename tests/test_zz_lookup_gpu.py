"""GPU tier of prompt-lookup speculative decoding (csrc/lookup.h, include/tinyllm_engine.h "Prompt lookup"): everything here is integer
data, so every comparison with tests/lookup_oracle.py is exact.

1. tl_lookup_rows over constructed rows: every row length at which the launch takes another path (one id, fewer ids than the tail, one
   wave, one workgroup pass and one id more, several passes), small and large alphabets, starts above 0, stale ids behind the end, ties.
2. The engine: the history an armed slot keeps -- uploaded chunks, decode steps fetched from the ring, set_token, rewind, verify_batch,
   fork, move, park, calls that outrun the ring -- is held against the ids the host itself read, through tl_engine_lookup_propose.
3. lookup_generate_ids on TINY_CFG with the checkpoint of tests/test_zz_verify_batch_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import lookup_oracle as L
from helpers import TINY_CFG, to_mlx_shaped
from oracle import tiny_oracle as O
from test_zz_verify_batch_gpu import assert_near_greedy, oracle_band, prompt_ids

pytestmark = pytest.mark.gpu
DEV = "cuda"
V = TINY_CFG["vocab_size"]


@pytest.fixture(scope="module")
def ext():
    import tiny_llm_ext_hip as ext

    return ext


# ---- 1. the kernel over caller rows -----------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 3, 64, 65, 1024, 1025, 2049, 5000)
ALPHABETS = (2, 5, 1000)
CAP = 5008
PARAMS = ((1, 1, 1), (3, 1, 4), (3, 3, 4), (16, 1, 7), (16, 16, 7), (3, 1, 7), (16, 2, 1))  # (max_ngram, min_ngram, num_proposals)


def constructed_rows():
    """(rows [n, CAP], start, end, names): random rows of every length and alphabet -- the row is full of ids of the same alphabet behind
    its end too, which must not matter -- and the hand-made ones."""
    rng = np.random.default_rng(20260)
    rows, start, end, names = [], [], [], []

    def add(name, ids, s0, e):
        row = np.asarray(ids, dtype=np.int32)
        assert row.shape == (CAP,) and e < CAP
        rows.append(row), start.append(s0), end.append(e), names.append(name)

    for n in LENGTHS:
        for a in ALPHABETS:
            add(f"len {n}, alphabet {a}", rng.integers(0, a, size=CAP), 0, n - 1)
    # start > 0, the same ids before the start as behind it: a match must not be found, or extended, below the start
    for n in (3, 65, 1025):
        unit = rng.integers(0, 5, size=n)
        add(f"start {n}, the row repeats below it", np.resize(unit, CAP), n, 2 * n - 1)
        add(f"start {n + 1} inside the repeat", np.resize(unit, CAP), n + 1, 2 * n + 3)
    filler = 900 + np.arange(CAP) % 90  # ids that occur nowhere else
    row = filler.copy()
    row[10:13] = (1, 2, 3)
    row[40:43] = (1, 2, 3)
    add("a match that reaches exactly to the start", row, 10, 42)
    add("... and one id further", row, 9, 42)
    add("... and with its first id before the start", row, 11, 42)
    row = filler.copy()
    row[5:8] = (1, 2, 3)
    row[20:22] = (1, 2)
    row[22:30] = (3, 7, 7, 1, 2, 3, 4, 5)  # behind the end: the id that would match, and a longer repeat
    add("stale matching ids behind the end", row, 0, 21)
    row = filler.copy()
    row[:9] = (5, 6, 7, 5, 6, 7, 5, 6, 7)
    add("a b c a b c a b c", row, 0, 8)
    row = filler.copy()
    row[100:104] = (4, 4, 4, 4)
    add("a continuation that runs into the end", row, 100, 103)
    row[98:100] = (1, 4)
    add("... two ids", row, 98, 100)
    add("end below start", filler, 7, 6)
    for n in (300, 2500):  # matches of 16 ids and more
        add(f"period 20, {n} ids", np.resize(rng.integers(0, 1000, size=20), CAP), 0, n - 1)
        add(f"period 20, {n} ids, start 13", np.resize(rng.integers(0, 4, size=20), CAP), 13, n - 1)
    add("a start below zero counts as zero", np.resize(rng.integers(0, 3, size=50), CAP), -3, 49)
    return np.stack(rows), np.asarray(start, dtype=np.int32), np.asarray(end, dtype=np.int32), names


@pytest.fixture(scope="module")
def rows_case():
    rows, start, end, names = constructed_rows()
    return rows, start, end, names, torch.from_numpy(rows).to(DEV)


@pytest.mark.parametrize("params", PARAMS, ids=[f"N{n}_min{m}_K{k}" for n, m, k in PARAMS])
def test_rows_equal_the_oracle(ext, rows_case, params):
    rows, start, end, names, dev_rows = rows_case
    n, m, k = params
    proposals, counts, match = ext.lookup_rows(dev_rows, start, end, n, m, k, want_match=True)
    proposals, counts, match = proposals.cpu().numpy(), counts.cpu().numpy(), match.cpu().numpy()
    hits = 0
    for r, name in enumerate(names):
        T, s0, e = rows[r].tolist(), max(int(start[r]), 0), int(end[r])
        want = L.propose(T, s0, e, n, m, k)
        c = L.choose(T, s0, e, n, m, k)
        what = f"{name} (N {n}, min {m}, K {k})"
        assert int(counts[r]) == len(want), what
        assert proposals[r].tolist() == want + [-1] * (8 - len(want)), what
        assert match[r].tolist() == ([c[0], c[1]] if c else [-1, 0]), what
        hits += bool(want)
    assert hits >= (len(names) // 3 if m <= 3 else 4), "the cases hardly ever match"


def test_the_hand_made_rows_say_what_they_were_made_for(rows_case):
    """(the oracle alone, so that a case that lost its point is noticed)"""
    rows, start, end, names, _ = rows_case
    at = {name: (rows[r].tolist(), max(int(start[r]), 0), int(end[r])) for r, name in enumerate(names)}
    assert L.choose(*at["a match that reaches exactly to the start"], 16, 1, 4) == (12, 3, 4)
    assert L.choose(*at["... and one id further"], 16, 1, 4) == (12, 3, 4)
    assert L.choose(*at["... and with its first id before the start"], 16, 1, 4) == (12, 2, 4)
    assert L.choose(*at["stale matching ids behind the end"], 3, 1, 4) == (6, 2, 4)
    assert L.propose(*at["a b c a b c a b c"], 3, 1, 3) == [5, 6, 7] and L.choose(*at["a b c a b c a b c"], 3, 1, 4) == (2, 3, 4)
    assert L.propose(*at["a continuation that runs into the end"], 3, 1, 4) == [4]
    assert L.choose(*at["a continuation that runs into the end"], 3, 1, 4) == (102, 3, 1)
    assert L.propose(*at["end below start"]) == []


def test_rows_refuse_bad_input(ext):
    lib = ext.lib()
    seq = torch.zeros((2, 16), dtype=torch.int32, device=DEV)
    se = torch.zeros(2, dtype=torch.int32, device=DEV)
    out, cnt = torch.zeros((2, 8), dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)

    def call(rows=2, cap=16, n=3, m=1, k=4, seq_p=seq.data_ptr(), out_p=out.data_ptr()):
        return lib.tl_lookup_rows(seq_p, rows, cap, se.data_ptr(), se.data_ptr(), n, m, k, out_p, cnt.data_ptr(), None, None)

    assert call() == 0
    for kw in ({"rows": 0}, {"rows": 65536}, {"cap": 0}, {"cap": (1 << 24) + 1}, {"n": 0}, {"n": 17}, {"m": 0}, {"m": 4}, {"k": 0}, {"k": 8},
               {"seq_p": None}, {"out_p": None}):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="inside the sequence capacity"):
        ext.lookup_rows(seq, 0, 16)
    with pytest.raises(ValueError, match="one value per row"):
        ext.lookup_rows(seq, [0, 0, 0], 3)


# ---- 2. the engine ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ckpt():
    w = O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05)
    return w, to_mlx_shaped(TINY_CFG, w)


def make_engine(model, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    args = dict(page_size=16, num_pages=64, max_batch=3, max_prefill_rows=64)
    args.update(kw)
    return DecodeEngine(model, **args)


class Track:
    """What the host itself knows of a slot: the ids whose K/V the slot holds, the pending token, and where its history starts."""

    def __init__(self, eng, slot, arm=True):
        self.eng, self.slot, self.seq, self.pending, self.s0 = eng, slot, [], None, 0
        eng.begin(slot)
        if arm:
            eng.set_lookup(slot)

    def prefill(self, ids, **kw):
        self.eng.prefill(self.slot, ids, **kw)
        self.seq += list(ids)
        if kw.get("want_logits", True):
            self.pending = self.eng.read_tokens(self.slot, 1)[0]

    def stepped(self, n):  # after eng.decode(n) over this slot
        got = self.eng.read_tokens(self.slot, n)
        self.seq += [self.pending] + got[:-1]
        self.pending = got[-1]

    def decode(self, n):
        self.eng.decode(n, batch=self.slot + 1)
        self.stepped(n)

    def set_token(self, t):
        self.eng.set_token(self.slot, t)
        self.pending = t

    def rewind(self, n):
        self.eng.rewind(self.slot, n)
        del self.seq[len(self.seq) - n:]
        self.s0 = min(self.s0, len(self.seq))

    @classmethod
    def adopt(cls, other, slot):  # the slot a fork or a move gave other's sequence to
        t = cls.__new__(cls)
        t.eng, t.slot, t.seq, t.pending, t.s0 = other.eng, slot, list(other.seq), other.pending, other.s0
        return t

    def want(self, n=3, m=1, k=4):
        assert self.eng.context_len(self.slot) == len(self.seq)
        return [self.pending] + L.propose(self.seq + [self.pending], self.s0, len(self.seq), n, m, k)


def check(tracks, what, params=((3, 1, 4), (1, 1, 7), (16, 2, 2))):
    eng = tracks[0].eng
    for n, m, k in params:
        got = eng.lookup_propose([t.slot for t in tracks], None, n, m, k)
        assert got == [t.want(n, m, k) for t in tracks], f"{what} (N {n}, min {m}, K {k})"
    for t in tracks:
        armed, s0, rec = eng.lookup_state(t.slot)
        assert armed and s0 == t.s0 and rec >= len(t.seq), what


def repetitive(n, seed, period=7):
    """a prompt that repeats itself with a few ids changed: lookups find long and short matches"""
    rng = np.random.default_rng(seed)
    ids = np.resize(rng.integers(1, V, size=period), n)
    ids[rng.integers(0, n, size=max(1, n // 9))] = rng.integers(1, V, size=max(1, n // 9))
    return [int(t) for t in ids]


def test_chunks_and_decode_steps(ckpt):
    eng = make_engine(ckpt[1])
    try:
        base = eng.stats()["workspace_bytes"]
        a = Track(eng, 0, arm=False)
        assert eng.stats()["workspace_bytes"] == base and eng.lookup_state(0) == (False, 0, 0)
        eng.set_lookup(0)
        grown = eng.stats()["workspace_bytes"]
        assert grown >= base + 3 * 64 * 16 * 4, "the first arming allocates the history rows and counts them"
        p = repetitive(40, 1)
        a.prefill(p[:23], want_logits=False)  # two chunks; the first crosses a page
        a.prefill(p[23:])
        check([a], "a prompt prefilled in two chunks")
        a.decode(5)
        assert eng.lookup_state(0)[2] == 40, "decode steps record nothing"
        check([a], "two chunks, then decode(5)")
        assert eng.lookup_state(0)[2] == 45, "the propose launch fetched the steps' ids from the ring"
        b = Track(eng, 1)
        assert eng.stats()["workspace_bytes"] == grown, "the block is allocated once"
        b.prefill(repetitive(19, 2, period=3))
        a.eng.decode(1, batch=2)
        a.stepped(1), b.stepped(1)
        a.eng.decode(7, batch=2)
        a.stepped(7), b.stepped(7)
        check([a, b], "decode(1) and decode(7) over two slots")
        check([b, a], "... named in the other order")
        b.rewind(2)
        b.set_token(b.seq[3])
        a.rewind(2)
        a.set_token(int(p[5]))
        check([a, b], "rewind 2 and set_token")
        a.decode(3)
        check([a], "... and three steps that feed the set token first")
        a.set_token(int(p[6]))
        a.rewind(4)  # (the other order: the token set before the rewind is the one the next step feeds)
        a.decode(2)
        check([a], "set_token, rewind 4, two steps")
        # max_lens clip the proposals; a slot with room for the pending token alone gets no proposal
        got = eng.lookup_propose([0, 1], [2, 1], 3, 1, 4)
        assert got == [a.want(3, 1, 1)[:2], [b.pending]]
    finally:
        eng.close()


def test_verify_batch_then_steps(ckpt):
    """verify_batch(commit=True) leaves a pending token the ring never saw; the steps behind it must not shift the history"""
    eng = make_engine(ckpt[1])
    try:
        a, b = Track(eng, 0), Track(eng, 1)
        a.prefill(repetitive(33, 3)), b.prefill(repetitive(11, 4, period=2))
        eng.decode(2, batch=2)
        a.stepped(2), b.stepped(2)
        for rnd in range(3):
            fed = eng.lookup_propose([0, 1], None, 3, 1, 4)
            assert fed == [a.want(), b.want()]
            fed[0] = fed[0] + [7] * (rnd + 1)  # proposals the engine will mostly reject: the rejected suffix is rewound
            res = eng.verify_batch([(0, fed[0]), (1, fed[1])], commit=True)
            for t, chunk, r in zip((a, b), fed, res):
                t.seq += chunk[:len(r)]
                t.pending = r[-1]
            check([a, b], f"verify_batch + commit, round {rnd}")
            eng.decode(1 + rnd, batch=2)
            a.stepped(1 + rnd), b.stepped(1 + rnd)
            check([a, b], f"... and {1 + rnd} decode steps")
        chunk = a.want()
        out = eng.verify(0, chunk)  # tl_engine_verify: the caller rewinds and sets the token
        a.seq += chunk
        a.rewind(len(chunk) - 1)
        a.set_token(out[0])
        a.decode(2)
        check([a], "verify, rewind, set_token, two steps")
    finally:
        eng.close()


def test_armed_at_a_context_above_zero(ckpt):
    eng = make_engine(ckpt[1])
    try:
        a = Track(eng, 0, arm=False)
        p = repetitive(30, 5, period=4)
        a.prefill(p)
        a.decode(6)
        eng.set_lookup(0)
        a.s0 = len(a.seq)
        assert eng.lookup_state(0) == (True, 36, 37), "s0 is the context length at arming; the pending token is stored"
        assert eng.lookup_propose([0]) == [[a.pending]], "ids before the arming are unknown"
        a.decode(9)
        check([a], "armed at context 36, nine steps")
        a.prefill(p[:12])
        check([a], "... and another chunk")
        eng.set_lookup(0)
        assert eng.lookup_state(0)[1] == 36, "arming an armed slot changes nothing"
        a.rewind(len(a.seq) - 30)
        assert eng.lookup_state(0)[1] == 30, "a rewind below s0 lowers s0"
        a.decode(4)
        check([a], "rewound below s0, four steps")
        eng.set_lookup(0, False)
        assert eng.lookup_state(0) == (False, 0, 0)
    finally:
        eng.close()


def test_fork_move_park_release(ckpt):
    eng = make_engine(ckpt[1], max_batch=4, swap_pages=16)
    try:
        a = Track(eng, 0)
        a.prefill(repetitive(21, 6, period=5))
        a.decode(4)  # (behind when forked: the fork fetches first)
        eng.fork(0, 2)
        c = Track.adopt(a, 2)
        check([a, c], "a fork copies the history")
        eng.decode(5, batch=3)
        a.stepped(5), c.stepped(5)
        check([a, c], "... and both go on")
        c.rewind(3)
        eng.decode(2, batch=3)
        a.stepped(2), c.stepped(2)
        check([c, a], "the fork rewound, two steps")
        eng.move(2, 3)
        c.slot = 3
        assert eng.lookup_state(2) == (False, 0, 0), "a move leaves the source unarmed"
        eng.decode(3, batch=4)
        a.stepped(3), c.stepped(3)
        check([a, c], "a move carries the history")
        before = eng.lookup_state(3)
        eng.park(3)
        assert eng.lookup_state(3) == before
        eng.decode(2, batch=4)
        a.stepped(2)
        eng.unpark(3)
        check([a, c], "park and unpark keep the history")
        eng.decode(2, batch=4)
        a.stepped(2), c.stepped(2)
        check([a, c], "... and two steps")
        eng.release(3)
        assert eng.lookup_state(3) == (False, 0, 0), "release switches it off"
        eng.begin(3)
        assert eng.lookup_state(3) == (False, 0, 0), "begin leaves it off"
        with pytest.raises(RuntimeError, match="not armed"):
            eng.lookup_propose([3])
        with pytest.raises(RuntimeError, match="prompt lookup"):
            eng.beam_reorder(0, 1, [0], [5])
        check([a], "a refused beam reorder leaves the slot as it was")
    finally:
        eng.close()


def test_prefix_attach_and_score_chunks(ckpt):
    eng = make_engine(ckpt[1], prefix_cache=True)
    try:
        p = repetitive(50, 7, period=6)
        a = Track(eng, 0, arm=False)
        a.prefill(p)
        eng.release(0)
        b = Track(eng, 1)
        matched = eng.prefix_attach(1, p)
        assert matched >= 32, "the cached pages of the first request are attached"
        b.seq = p[:matched]
        b.prefill(p[matched:])
        b.decode(3)
        check([b], "ids of attached pages are recorded like a prefill's")
    finally:
        eng.close()


def test_more_steps_than_the_ring_holds(ckpt):
    eng = make_engine(ckpt[1], page_size=128, num_pages=72, max_batch=1)
    try:
        a = Track(eng, 0)
        a.prefill(repetitive(10, 8, period=3))
        a.decode(3000)
        assert eng.lookup_state(0) == (True, 0, 10)
        a.decode(1500)  # 4,500 unrecorded ids would outrun the ring: the call fetches the first 3,000 ahead of itself
        assert eng.lookup_state(0) == (True, 0, 3010)
        check([a], "3,000 and 1,500 steps", params=((3, 1, 4), (16, 1, 7)))
        eng.decode(4096, batch=1)  # a call that outruns the ring alone: the history starts over behind it
        a.seq = [0] * (len(a.seq) + 4096)  # (ids before s0 are never read)
        a.pending, a.s0 = eng.read_tokens(0, 1)[0], len(a.seq)
        assert eng.lookup_state(0) == (True, a.s0, a.s0)
        assert eng.lookup_propose([0]) == [[a.pending]]
        a.decode(40)
        check([a], "forty steps behind the restart", params=((3, 1, 4), (16, 1, 7)))
    finally:
        eng.close()


def raw_propose(eng, slots, max_lens=None, n=3, m=1, k=4):
    """The C entry point without the binding's own argument checks."""
    import tiny_llm_ext_hip as ext

    c = len(slots)
    tokens, lens = (ctypes.c_int32 * 64)(*([-5] * 64)), (ctypes.c_int * max(c, 1))(*([-5] * max(c, 1)))
    rc = ext.lib().tl_engine_lookup_propose(eng._h, c, (ctypes.c_int * max(c, 1))(*slots), (ctypes.c_int * c)(*max_lens) if max_lens else None, n, m, k,
                                            tokens, lens)
    return rc, list(tokens), list(lens)


def test_every_refusal_leaves_the_slots_as_they_were(ckpt):
    import lora_oracle

    eng = make_engine(ckpt[1], max_batch=12, num_pages=96, swap_pages=8)
    try:
        adapter = eng.load_lora(lora_oracle.to_lora_adapter(lora_oracle.make_adapter(TINY_CFG, 8, seed=0)))
        for s in range(10):
            eng.begin(s)
            if s != 7:
                eng.set_lookup(s)
            if s == 6:
                eng.set_lora(s, adapter)
            eng.prefill(s, repetitive(9 + s, 40 + s, period=3))
        eng.decode(3, batch=10)
        eng.set_sampling(2, 0.8, None, None, 1)
        eng.set_penalties(3, 1.3)
        eng.park(4)
        eng.set_stop(5, None, 1)
        eng.decode(1, batch=10)  # slot 5 stops at its budget

        def state():
            return ([eng.context_len(s) for s in range(10)], eng.read_pending(10), [eng.lookup_state(s) for s in range(10)], eng.stats()["pages_in_use"],
                    eng.stats()["workspace_bytes"])

        before = state()
        bad = {"a sampling slot": ([0, 2], None), "a processing slot": ([0, 3], None), "a parked slot": ([0, 4], None), "a stopped slot": ([0, 5], None),
               "an adapter slot": ([0, 6], None), "an unarmed slot": ([0, 7], None), "a slot named twice": ([0, 1, 0], None),
               "a free slot": ([0, 11], None), "a slot out of range": ([0, 12], None), "no slot": ([], None), "max_len 0": ([0], [0]),
               "max_len 9": ([0], [9])}
        for what, (slots, lens) in bad.items():
            rc, tokens, out_lens = raw_propose(eng, slots, lens)
            assert rc != 0, what
            assert set(tokens) == {-5} and set(out_lens) == {-5}, f"{what}: the outputs were written"
            assert state() == before, what
        # 9 slots x 8 rows: the chunks could exceed one verification pass
        for s in (2, 3, 6):
            eng.release(s)
        for s in (2, 3, 6, 10, 11):
            eng.begin(s)
            eng.set_lookup(s)
            eng.prefill(s, repetitive(5, s))
        nine = [0, 1, 2, 3, 6, 8, 9, 10, 11]
        before = state()
        rc, tokens, _ = raw_propose(eng, nine, None)
        assert rc != 0 and set(tokens) == {-5} and state() == before, "nine slots of 8 rows exceed 64"
        rc, tokens, _ = raw_propose(eng, nine, [8] * 8 + [1])
        assert rc != 0 and set(tokens) == {-5}, "a sum of max_lens of 65"
        for kw in ({"n": 0}, {"n": 17}, {"m": 0}, {"m": 4}, {"k": 0}, {"k": 8}):
            rc, tokens, _ = raw_propose(eng, [0], None, **kw)
            assert rc != 0 and set(tokens) == {-5} and state() == before, kw
        rc, tokens, lens = raw_propose(eng, nine, [8] * 7 + [4, 4])
        assert rc == 0 and sum(lens[:9]) <= 64 and all(1 <= n <= 8 for n in lens[:9]), "64 rows go through"
    finally:
        eng.close()


def test_a_step_with_an_armed_slot_issues_the_same_launches(ckpt):
    """tl_engine_profile_step and tl_engine_check_step, the entry points of tests/test_zz_engine_step_launches_gpu.py"""
    eng = make_engine(ckpt[1])
    try:
        seen = []
        for arm in (False, True):
            for s in range(2):
                eng.begin(s)
                if arm:
                    eng.set_lookup(s)
                eng.prefill(s, repetitive(20 + s, 9))
            eng.decode(2, batch=2)
            prof = eng.profile_step(2)
            chk = eng.check_step(2)
            seen.append(([prof["kinds"][k]["launches"] for k in eng.PROFILE_KINDS], prof["n_splits"], chk["launches"], chk["n_splits"],
                         chk["written_once_plan"], eng.replay_route()))
            if arm:
                assert eng.lookup_state(0) == (True, 0, 20), "the steps recorded nothing"
            for s in range(2):
                eng.release(s)
        assert seen[0] == seen[1]
        assert sum(seen[0][0]) > 0 and seen[0][2] > 0
    finally:
        eng.close()


# ---- 3. the loop ----------------------------------------------------------------------------------------------------------------------
LOOP_PROMPTS = ((11, 411), (19, 422), (33, 433), (24, 7))


@pytest.fixture(scope="module")
def band(ckpt):
    return oracle_band(TINY_CFG, ckpt[0], [prompt_ids(n, seed=n) for n in (5, 37, 150)])


def test_lookup_generate_ids(ckpt, band):
    """64 new ids for each of four prompts with K = 4, N = 3, min_ngram = 1.  The bf16 oracle's own greedy continuations of these prompts
    repeat heavily (a simulation of the loop over them accepts 34 to 40 of 40 to 50 proposals on each), and have top-two margins down to
    0.000: no equality with batch_generate_ids is asserted.  Every emitted id is the oracle's best logit, or within the oracle band of it,
    in the oracle's row for the engine's own prefix."""
    from tiny_llm_hip.engine import lookup_generate_ids

    w, model = ckpt
    eng = make_engine(model, num_pages=96)
    try:
        for n, seed in LOOP_PROMPTS:
            prompt, stats = prompt_ids(n, seed=seed), {}
            ids = lookup_generate_ids(eng, [prompt], 64, proposal_length=4, max_ngram=3, min_ngram=1, stats=stats)[0]
            print(f"prompt ({n}, {seed}): {stats}")
            assert len(ids) == 64
            assert stats["accepted"] >= 1 and stats["rounds"] + stats["steps"] < 64, f"prompt ({n}, {seed}): {stats}"
            assert 0 <= stats["accepted"] <= stats["proposed"] <= 4 * stats["rounds"]
            rows = O.OracleQwen3(TINY_CFG, w).forward(prompt + ids, logits_to_keep=None)[0]
            for j, tok in enumerate(ids):
                assert_near_greedy(rows[len(prompt) + j - 1], tok, band, f"prompt ({n}, {seed}), id {j}")
        # the four together, in one wave of three slots and one of one: the same rules
        prompts, stats = [prompt_ids(n, seed=seed) for n, seed in LOOP_PROMPTS], {}
        outs = lookup_generate_ids(eng, prompts, 64, stats=stats)
        assert [len(o) for o in outs] == [64] * 4 and stats["accepted"] >= 4 and stats["rounds"] + stats["steps"] < 2 * 64
        for (n, seed), prompt, ids in zip(LOOP_PROMPTS, prompts, outs):
            rows = O.OracleQwen3(TINY_CFG, w).forward(prompt + ids, logits_to_keep=None)[0]
            for j, tok in enumerate(ids):
                assert_near_greedy(rows[len(prompt) + j - 1], tok, band, f"batched, prompt ({n}, {seed}), id {j}")
        assert eng.stats()["pages_in_use"] == 0
    finally:
        eng.close()


def test_the_cli_gives_the_answers_of_batch_main(ckpt, tmp_path, capsys):
    """lookup_main.py on a written checkpoint against batch_main.py: the prompts of tests/test_zz_verify_batch_gpu.py's draft-model test,
    at which the oracle keeps its two best logits at least 0.3 apart at every position either run generates, so both runs emit the
    oracle's ids and the answers are equal."""
    from checkpoint_fixture import write_checkpoint
    import batch_main
    import lookup_main

    w, _ = ckpt
    words = [f"w{i}" for i in range(V - 2)]
    path = str(write_checkpoint(tmp_path / "ckpt", TINY_CFG, w, vocab_words=words))
    prompts = tmp_path / "prompts.txt"
    prompts.write_text("w194 w491 w354\nw607 w985\nw433 w670 w506 w353\n")
    common = ["--prefill-step", "16", "--max-seq-len", "12", "--raw-prompts", "--prompts-file", str(prompts)]
    plain = dict(batch_main.main(["--model", path, "--batch-size", "2"] + common))
    spec = dict(lookup_main.main([path, "--proposal-length", "3", "--max-ngram", "2"] + common))
    assert sorted(spec) == sorted(plain) == [0, 1, 2]
    assert spec == plain
    assert '"rounds"' in capsys.readouterr().out
