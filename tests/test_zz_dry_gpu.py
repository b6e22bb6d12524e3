"""GPU tier: DRY and the n-gram ban on the device (tl_engine_set_dry, tl_dry_rows, csrc/dry.h) against the numpy restatement of their
definition (tests/dry_oracle.py).  Every processed row is checked bit for bit against the oracle applied to the engine's OWN raw row
(and, where the slot also has penalties or a bias, to tests/logit_processing_oracle.py's row of it) and the ids recorded so far; a
greedy id must be the first maximum of that row, a sampled one tests/sampling_oracle.py's unless it flags the draw ambiguous."""

import numpy as np
import pytest
import torch

import dry_oracle as D
import logit_processing_oracle as P
import sampling_oracle as S
from helpers import TINY_CFG, to_mlx_shaped
from oracle import tiny_oracle as O

pytestmark = pytest.mark.gpu

V = TINY_CFG["vocab_size"]
OFF = dict(multiplier=0.0, base=1.75, allowed_length=2, range_=0, ngram=0, breakers=())
# The prompt is an 8-token pattern repeated 6 times.  Seed picked on the CPU with OracleQwen3 (seed-3 weights) running this file's loop
# under DRY (0.8, 1.75, 2) + n-gram 3: of seeds 0 .. 11 the control changes the greedy choice at 7 .. 12 of 32 steps; seed 4 gives 12,
# with no tie in any processed row (smallest margin 0.047).
PROMPT_SEED = 4


def pattern_prompt(seed=PROMPT_SEED, repeats=6):
    return np.random.default_rng(seed).integers(0, V, 8).tolist() * repeats


def u16(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def tiny():
    return to_mlx_shaped(TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=3, sigma=0.05))


def make_engine(model, n, **kw):
    from tiny_llm_hip.engine import DecodeEngine

    return DecodeEngine(model, page_size=16, num_pages=16 * n + 32, max_batch=n, max_prefill_rows=64, **kw)


# -- 1. the two launches, bit for bit ---------------------------------------------------------------------------------------------
def kernel_rows():
    """(sequence, start, parameters) per row"""
    rng = np.random.default_rng(1)
    period7 = (rng.integers(0, 4104, 7).tolist() * 15)[:100]
    distinct = rng.permutation(4104)[:300].tolist()
    both = dict(OFF, multiplier=0.8, ngram=3)
    rows = [
        (period7, 0, both),                                                       # a period-7 pattern repeated to 100 tokens
        ([77] * 6000, 0, dict(OFF, multiplier=0.5, base=1.1, ngram=64)),          # more candidates than threads, every match at the cap
        (distinct, 0, both),                                                      # no candidate
        ([5], 0, both),                                                           # a length-1 sequence
        (period7[:99] + [period7[1]], 0, dict(both, breakers=(period7[1],))),     # a breaker as the last token: no DRY, the ban stays
        (period7, 0, dict(OFF, multiplier=0.8, breakers=(period7[(99 - 3) % 7],))),  # a breaker three tokens back: B limits
        (period7, 0, dict(OFF, multiplier=0.8, breakers=(period7[(99 + 1) % 7], 4000))),  # a breaker as a continuation
        (period7, 0, dict(OFF, multiplier=0.8, allowed_length=1, range_=12)),     # range cutting a match
        (period7, 90, dict(both, ngram=5)),                                       # start > 0 cutting a match
        (period7, 0, dict(OFF, ngram=4)),                                         # n-gram only
        (period7, 0, dict(OFF, multiplier=0.8, base=1e30, allowed_length=3)),     # DRY only; p overflows
        # both, where one token is banned and penalised, and others only penalised: ... a b c X a b c Y b c Z c
        ([9, 1, 2, 3, 50, 1, 2, 3, 51, 2, 3, 52, 3, 53, 8, 1, 2, 3], 0, dict(OFF, multiplier=1.5, allowed_length=1, ngram=4)),
    ]
    return rows


def test_dry_rows_bit_for_bit():
    import tiny_llm_ext_hip as ext

    vocab, cap = 4104, 8192  # not a multiple of the apply chunk: one chunk plus a tail
    rows = kernel_rows()
    assert len(rows) == 12
    rng = np.random.default_rng(2)
    seqs = np.full((len(rows), cap), -7, np.int32)
    lg = D.bits((rng.standard_normal((len(rows), vocab)) * 3.0).astype(np.float32))
    for r, (seq, start, prm) in enumerate(rows):
        seqs[r, :len(seq)] = seq
        seqs[r, :start] = rng.integers(0, vocab, start)  # ids before start are never matched, whatever they are
        hit = sorted(set(D.banned(seq, start, prm["ngram"])) | set(D.dry_lengths(seq, start, prm["multiplier"], prm["allowed_length"], prm["range_"], prm["breakers"])))
        for k, t in enumerate(hit):  # a NaN, a +inf and a -inf at banned and at penalised positions, by row: most rows have one
            if (r + k) % 4 == 1:
                lg[r, t] = 0x7FC1
            elif (r + k) % 4 == 2:
                lg[r, t] = 0x7F80
            elif (r + k) % 4 == 3:
                lg[r, t] = 0xFF80
    want = np.stack([D.apply(lg[r], [int(t) for t in seqs[r, :len(seq)]], start, **prm) for r, (seq, start, prm) in enumerate(rows)])
    # what the rows are there to show (all from the oracle: the device must agree bit for bit below)
    changed = [(want[r] != lg[r]).sum() for r in range(len(rows))]
    assert changed[2] == 0 and changed[3] == 0 and changed[6] == 0 and all(changed[r] > 0 for r in (0, 1, 4, 8, 9, 10, 11)), changed
    t5, t52, t53 = rows[5][0][93], 52, 53
    assert lg[5][t5] == want[5][t5] == 0x7FC1, "a NaN with a DRY entry keeps its bits"
    assert lg[9][rows[9][0][93]] == 0x7FC1 and want[9][rows[9][0][93]] == D.NEG_INF, "a banned NaN becomes -inf"
    assert lg[10][rows[10][0][93]] == 0x7F80 and want[10][rows[10][0][93]] == D.NEG_INF, "+inf under a penalty that overflows"
    assert lg[11][t52] == want[11][t52] == 0x7FC1 and lg[11][t53] == want[11][t53] == 0x7F80
    assert want[1][77] == D.NEG_INF and D.dry_lengths(rows[1][0], 0, 0.5, 2, 0, ()) == {77: 64}
    assert D.dry_lengths(rows[5][0], 0, 0.8, 2, 0, rows[5][2]["breakers"]) == {rows[5][0][99 - 7 + 1]: 3}
    assert D.dry_lengths(rows[6][0], 0, 0.8, 2, 0, rows[6][2]["breakers"]) == {}
    assert max(D.dry_lengths(rows[7][0], 0, 0.8, 1, 12, ()).values()) == 5
    assert D.banned(rows[8][0], 90, 5) == set() and D.banned(rows[8][0], 0, 5) != set() and max(D.dry_lengths(rows[8][0], 90, 0.8, 2, 0, ()).values()) == 3
    assert D.banned(rows[11][0], 0, 4) == {50, 51} and D.dry_lengths(rows[11][0], 0, 1.5, 1, 0, ()) == {50: 3, 51: 3, 52: 2, 53: 1}
    assert not np.isfinite(D.penalty(0.8, 1e30, 64, 3))

    table = torch.zeros((len(rows), vocab), dtype=torch.int32, device="cuda")
    got = ext.dry_rows(torch.from_numpy(lg.view(np.int16)).cuda().view(torch.bfloat16), torch.from_numpy(seqs).cuda(),
                       [r[1] for r in rows], [len(r[0]) - 1 for r in rows], [r[2]["multiplier"] for r in rows], [r[2]["base"] for r in rows],
                       [r[2]["allowed_length"] for r in rows], [r[2]["range_"] for r in rows], [r[2]["ngram"] for r in rows],
                       [r[2]["breakers"] for r in rows], table=table)
    got = u16(got)
    for r in range(len(rows)):
        bad = np.flatnonzero(got[r] != want[r])
        assert bad.size == 0, f"row {r}: {bad.size} elements differ, first at {bad[:4]}: got {got[r][bad[:4]]}, want {want[r][bad[:4]]}, logit {lg[r][bad[:4]]}"
    assert int(table.ne(0).sum()) == 0, "the table is all zeros after the call"


# -- the engine, step by step -----------------------------------------------------------------------------------------------------
class Sim:
    """An engine and, beside it, what the header says each slot holds: its settings, the ids recorded since it was armed (``seq``, with
    ``start`` = s0) and -- for the penalties -- its history."""

    def __init__(self, model, n, **kw):
        self.eng = make_engine(model, n, **kw)
        self.n = n
        self.cfg, self.seq, self.start, self.hist, self.out, self.pending = {}, {}, {}, {}, {}, {}
        self.changed = {}
        self.draws = self.ambiguous = 0

    def close(self):
        self.eng.close()

    def arm(self, slot, dry=None, pen=(1.0, 0.0, 0.0), bias=None, smp=None, known=()):
        """the slot's settings, set on the engine; ``known``: the ids the slot already holds (they stay unknown to the device)"""
        eng = self.eng
        self.cfg[slot] = dict(dry=dry, pen=pen, bias=dict(bias or {}), smp=smp)
        self.seq[slot], self.start[slot], self.hist[slot] = list(known), len(known), P.History(V)
        self.out.setdefault(slot, [])
        self.changed[slot] = 0
        if pen != (1.0, 0.0, 0.0):
            eng.set_penalties(slot, *pen)
        if bias:
            eng.set_logit_bias(slot, bias)
        if dry:
            eng.set_dry(slot, dry["multiplier"], dry["base"], dry["allowed_length"], dry["range_"], dry["ngram"], dry["breakers"])
        if smp:
            eng.set_sampling(slot, smp[0], None, None, smp[1])

    def expected_row(self, slot, raw_bits):
        c = self.cfg[slot]
        row = raw_bits
        if P.processes(*c["pen"], c["bias"]):
            row = P.bits(P.process(P.from_bits(raw_bits), self.hist[slot].prompt, self.hist[slot].count, *c["pen"], c["bias"]))
        if c["dry"]:
            row = D.apply(row, self.seq[slot], self.start[slot], **c["dry"])
        return row

    def check(self, slot, got_id, raw_bits, proc_bits, position):
        want = self.expected_row(slot, raw_bits)
        bad = np.flatnonzero(proc_bits != want)
        assert bad.size == 0, (f"slot {slot} at position {position}: {bad.size} elements of the processed row differ, first at {bad[:4]}: got "
                               f"{proc_bits[bad[:4]]}, want {want[bad[:4]]}, raw {raw_bits[bad[:4]]}")
        row = D.from_bits(want)
        smp = self.cfg[slot]["smp"]
        if smp:
            want_id, amb = S.sample(row, smp[0], 0, 1.0, smp[1], position)
            self.draws += 1
            self.ambiguous += bool(amb)
            assert got_id == want_id or amb, (slot, position, got_id, want_id)
        else:
            assert got_id == int(np.argmax(row)), f"slot {slot} at position {position}: the id is the first maximum of the processed row"
        self.changed[slot] += int(np.argmax(D.from_bits(raw_bits))) != int(np.argmax(row))

    def prefill(self, slot, tokens, attach=0, check=True):
        """feeds ``tokens`` (the first ``attach`` of them through prefix_attach) and checks the first token"""
        eng = self.eng
        if attach:
            assert eng.prefix_attach(slot, tokens) == attach
        eng.prefill(slot, tokens[attach:])
        self.seq[slot] += list(tokens)
        if P.processes(*self.cfg[slot]["pen"], self.cfg[slot]["bias"]):
            self.hist[slot].consume_prompt(tokens)
        got = eng.read_tokens(slot, 1)[0]
        if check:
            self.check(slot, got, u16(eng.logits(1))[0], u16(eng.processed_logits(1))[0], eng.context_len(slot))
        self.pending[slot] = got
        self.out[slot] = [got]

    def step(self, slots=None, check=True):
        """one decode step over every slot; ``slots``: the slots that run (default: every armed one)"""
        eng, n = self.eng, self.n
        slots = sorted(self.cfg) if slots is None else slots
        ctx = {i: eng.context_len(i) for i in slots}
        for i in slots:  # the step feeds the pending token: it joins the sequence (and is counted) before the row is processed
            self.seq[i].append(self.pending[i])
            if P.processes(*self.cfg[i]["pen"], self.cfg[i]["bias"]):
                self.hist[i].feed(self.pending[i])
        eng.decode(1, batch=n)
        got = eng.read_pending(n)
        raw = u16(eng.logits(n))
        if check:
            proc = u16(eng.processed_logits(n))
            for i in slots:
                self.check(i, got[i], raw[i], proc[i], ctx[i] + 1)
        for i in slots:
            self.pending[i] = got[i]
            self.out[i].append(got[i])
        return raw


DRY_3 = dict(OFF, multiplier=0.8, ngram=3)


def test_engine_single_slot(tiny):
    prompt = pattern_prompt()
    sim = Sim(tiny, 1)
    try:
        assert sim.eng.replay_route() == "aql"
        sim.eng.begin(0)
        sim.arm(0, DRY_3)
        sim.prefill(0, prompt)
        for _ in range(32):
            sim.step()
        route = sim.eng.replay_route()
        assert route.startswith("hipgraph: a slot has DRY or the n-gram ban on"), route
        ids = sim.out[0]
        assert sim.eng.read_tokens(0, 33) == ids
        # condition, not a measurement: the control decides
        assert sim.changed[0] >= 3, f"DRY / the n-gram ban changed the greedy choice at {sim.changed[0]} of 33 rows"
        sim.eng.release(0)
        # the same request in multi-step calls: the sequence is kept on the device
        sim.eng.begin(0)
        sim.eng.set_dry(0, 0.8, 1.75, 2, 0, 3)
        sim.eng.prefill(0, prompt)
        for _ in range(4):
            sim.eng.decode(8, batch=1)
        assert sim.eng.read_tokens(0, 33) == ids
        sim.eng.release(0)
        # ... and through generate()
        assert sim.eng.generate(prompt, 33, dry_multiplier=0.8, no_repeat_ngram=3) == ids
        assert sim.eng.generate(prompt, 33) != ids
    finally:
        sim.close()


def test_mixed_batch(tiny):
    prompts = [pattern_prompt(4), pattern_prompt(6), pattern_prompt(9)]
    sim = Sim(tiny, 3)
    plain = make_engine(tiny, 3)
    try:
        rng = np.random.default_rng(5)
        bias = {int(t): float(np.float32(v)) for t, v in zip(rng.choice(V, 2, replace=False), (1.5, -2.0))}
        settings = [dict(dry=dict(OFF, multiplier=0.8), smp=(0.8, 123)), dict(dry=dict(OFF, ngram=3), pen=(1.3, 0.0, 0.0), bias=bias), dict()]
        for i in range(3):
            sim.eng.begin(i)
            sim.arm(i, **settings[i])
            sim.prefill(i, prompts[i], check=i < 2)
            plain.begin(i)
            plain.prefill(i, prompts[i])
        plain_ids = [plain.read_tokens(2, 1)[0]]
        assert sim.out[2] == plain_ids
        for _ in range(16):
            raw = sim.step(check=False)
            proc = u16(sim.eng.processed_logits(3))
            for i in (0, 1):
                sim.check(i, sim.out[i][-1], raw[i], proc[i], sim.eng.context_len(i))
            assert np.array_equal(proc[2], raw[2]), "the plain slot's row is copied"
            plain.decode(1, batch=3)
            plain_ids.append(plain.read_pending(3)[2])
            assert np.array_equal(u16(plain.logits(3))[2], raw[2]), "the plain slot's raw row does not depend on the other slots' settings"
        assert sim.out[2] == plain_ids
        assert sim.draws == 17 and sim.ambiguous <= 0.1 * sim.draws, (sim.draws, sim.ambiguous)
        assert plain.replay_route() == "aql" and sim.eng.replay_route().startswith("hipgraph")
    finally:
        sim.close()
        plain.close()


# -- 4. life ------------------------------------------------------------------------------------------------------------------------
def test_fork_move_park(tiny):
    prompt = pattern_prompt()
    sim = Sim(tiny, 4, swap_pages=16)
    try:
        sim.eng.begin(0)
        sim.arm(0, DRY_3)
        sim.prefill(0, prompt)
        for _ in range(6):
            sim.step()
        # fork mid-generation: parent and child go on with equal ids
        sim.eng.fork(0, 1)
        for k in ("cfg", "start", "pending"):
            getattr(sim, k)[1] = getattr(sim, k)[0]
        sim.seq[1], sim.out[1], sim.hist[1], sim.changed[1] = list(sim.seq[0]), list(sim.out[0]), P.History(V), 0
        for _ in range(6):
            sim.step()
        assert sim.out[0] == sim.out[1]
        # move the child: parameters, s0 and the sequence row travel; the source is off
        sim.eng.move(1, 3)
        for k in ("cfg", "start", "pending", "seq", "out", "hist", "changed"):
            getattr(sim, k)[3] = getattr(sim, k).pop(1)
        for _ in range(4):
            sim.step()
        assert sim.out[0] == sim.out[3]
        # park the parent while the moved child steps; unparked, it continues where it stood
        sim.eng.park(0)
        for _ in range(3):
            sim.step(slots=[3])
        sim.eng.unpark(0)
        sim.eng.park(3)
        for _ in range(3):
            sim.step(slots=[0])
        sim.eng.unpark(3)
        assert sim.out[0] == sim.out[3]
        for _ in range(2):
            sim.step()
        assert sim.out[0] == sim.out[3] and len(sim.out[0]) == 22
        # ... equal to the unforked run (steps of the same four rows: a step's arithmetic follows its row count)
        for slot in (0, 3):
            sim.eng.release(slot)
        sim.eng.begin(0)
        sim.eng.set_dry(0, 0.8, 1.75, 2, 0, 3)
        sim.eng.prefill(0, prompt)
        for _ in range(21):
            sim.eng.decode(1, batch=4)
        assert sim.eng.read_tokens(0, 22) == sim.out[0]
    finally:
        sim.close()


def test_arming_at_context_20(tiny):
    prompt = pattern_prompt()
    sim = Sim(tiny, 1)
    try:
        sim.eng.begin(0)
        sim.eng.prefill(0, prompt[:20])
        sim.arm(0, dict(OFF, multiplier=0.8, allowed_length=1, ngram=2), known=prompt[:20])  # the first 20 ids are never matched
        assert sim.start[0] == 20
        sim.prefill(0, prompt[20:])
        for _ in range(8):
            sim.step()
        # changing parameters keeps s0 and the sequence; off and on again starts at the current context length
        sim.eng.set_dry(0, 0.5, 2.0, 1, 0, 0)
        sim.cfg[0]["dry"] = dict(OFF, multiplier=0.5, base=2.0, allowed_length=1)
        for _ in range(3):
            sim.step()
        sim.eng.set_dry(0)
        sim.eng.set_dry(0, 0.5, 2.0, 1, 0, 2)
        sim.cfg[0]["dry"] = dict(OFF, multiplier=0.5, base=2.0, allowed_length=1, ngram=2)
        sim.start[0] = sim.eng.context_len(0)
        for _ in range(6):
            sim.step()
    finally:
        sim.close()


def test_prefix_attach_then_prefill(tiny):
    prompt = pattern_prompt()
    sim = Sim(tiny, 2, prefix_cache=True)
    try:
        sim.eng.begin(1)
        sim.eng.prefill(1, prompt)
        sim.eng.release(1)  # its full pages stay cached
        dry = dict(OFF, multiplier=0.8)
        sim.eng.begin(0)
        sim.arm(0, dry)
        matched = sim.eng.prefix_attach(0, prompt)
        assert 0 < matched < len(prompt)
        sim.eng.release(0)
        # the rows below tell whether the matched ids were recorded: the repeat reaches back into them (L = 40; less or none without them)
        assert D.dry_lengths(prompt, 0, 0.8) == {prompt[0]: 40} and D.dry_lengths(prompt, matched, 0.8).get(prompt[0], 0) < 40
        sim.eng.begin(0)
        sim.arm(0, dry)
        sim.prefill(0, prompt, attach=matched)  # the first token is chosen from the DRY row
        for _ in range(6):
            sim.step()
    finally:
        sim.close()


def test_refusals_leave_the_slot_as_it_was(tiny):
    prompt = pattern_prompt()
    eng = make_engine(tiny, 2)
    try:
        eng.begin(0)
        eng.set_dry(0, no_repeat_ngram=3)
        eng.prefill(0, prompt)
        first = eng.read_tokens(0, 1)
        for call, text in ((lambda: eng.rewind(0, 1), "engine_rewind: the slot processes its logits"),
                           (lambda: eng.set_token(0, 5), "engine_set_token: the slot processes its logits"),
                           (lambda: eng.verify(0, [first[0], 1, 2]), "engine_verify: the slot processes its logits"),
                           (lambda: eng.verify_batch([(0, [first[0], 1, 2])]), "engine_verify_batch: a slot processes its logits"),
                           (lambda: eng.beam_select(0, 1, [0.0], 2), "engine_beam: the slot processes its logits")):
            with pytest.raises(RuntimeError, match=text):
                call()
            assert eng.context_len(0) == len(prompt) and eng.read_tokens(0, 1) == first
        with pytest.raises((RuntimeError, ValueError)):
            eng.set_dry(0, no_repeat_ngram=1)
        eng.decode(4, batch=1)
        ids = eng.read_tokens(0, 5)
        eng.release(0)
        assert eng.generate(prompt, 5, no_repeat_ngram=3) == ids
    finally:
        eng.close()


# -- 5. with a stop set -----------------------------------------------------------------------------------------------------------
def test_stop_inside_a_block(tiny):
    prompts = [pattern_prompt(4), pattern_prompt(6)]
    eng = make_engine(tiny, 2)
    try:
        def start(stop_id=None):
            eng.begin(0)
            eng.set_dry(0, 0.8, 1.75, 2, 0, 3)
            if stop_id is not None:
                eng.set_stop(0, eng.make_stop_set(ids=[stop_id]), 0)
            eng.prefill(0, prompts[0])
            eng.begin(1)
            eng.prefill(1, prompts[1])

        start()  # one step at a time, no stop: the reference ids
        for _ in range(16):
            eng.decode(1, batch=2)
        want = [eng.read_tokens(i, 17) for i in range(2)]
        for i in range(2):
            eng.release(i)
        # the stop id: the last id of the armed slot's answer that is new to it where it stands, inside the block of 16 steps
        new = [k for k in range(1, 15) if want[0][k] not in want[0][:k]]
        assert new
        at = new[-1]
        start(want[0][at])
        eng.decode(16, batch=2)
        state = eng.stop_state(0)
        assert state.stopped and state.generated == at + 1
        assert eng.read_tokens(0, at + 1) == want[0][:at + 1], "the armed slot's ids up to the stop equal the one-step run"
        assert eng.read_tokens(1, 17) == want[1], "the other slot is unaffected"
    finally:
        eng.close()


# -- 6. nothing is allocated before the first arming call -----------------------------------------------------------------------------
def test_nothing_allocated_before_arming(tiny):
    eng = make_engine(tiny, 2)
    try:
        eng.begin(0)
        before = eng.stats()["workspace_bytes"]
        eng.set_dry(0)  # off: no block
        eng.prefill(0, pattern_prompt()[:8])
        eng.decode(2, batch=1)
        assert eng.stats()["workspace_bytes"] == before
        eng.set_dry(1 - 1, no_repeat_ngram=2)
        cap = eng.max_pages_per_seq * eng.page_size
        assert eng.stats()["workspace_bytes"] - before >= 2 * (cap * 4 + V * 4) + 2 * V * 2
        after = eng.stats()["workspace_bytes"]
        eng.begin(1)
        eng.set_dry(1, 0.8)
        assert eng.stats()["workspace_bytes"] == after
    finally:
        eng.close()
