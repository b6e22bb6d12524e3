"""Beam search over the decode engine: the search policy, and the loop that drives it through ``DecodeEngine.beam_select`` /
``beam_reorder`` (include/tinyllm_engine.h "Beam search").

The policy is ``beam_search``: a pure function over two callbacks, so it runs without a GPU (tests/test_beam_cpu.py feeds it from a
CPU model).  Its specification is ``transformers`` 5.x ``GenerationMixin._beam_search`` as called by ``generate(num_beams=B,
num_return_sequences=B, do_sample=False, length_penalty=..., early_stopping=..., eos_token_id=[...], max_new_tokens=...)`` for one
prompt, which it restates step for step:

* every step asks for the best ``K = max(2, 1 + n_eos) * B`` (parent, token) pairs by cumulative log-probability (``select``).  The
  first step has one beam with score 0; ``transformers`` starts B copies with scores 0, -1e9, ..., whose best K are the first copy's.
* a candidate *hits* when its token is an EOS id or it is the ``max_new_tokens``-th token.  The next running beams are the best B
  candidates that did not hit.  (K is large enough for B of them: at most ``n_eos * B`` candidates are EOS.)
* only candidates ranked inside the first B may finish a hypothesis: those that hit are scored ``sum_logprobs / generated_len **
  length_penalty``, the EOS or last token counted in ``generated_len``, and merged into the finished list, which keeps the best B.
* after the step, with ``g`` tokens generated: the best running score divided by ``L ** length_penalty`` -- ``L = max_new_tokens`` for
  ``early_stopping="never"`` with a positive length penalty, else ``L = g`` -- is compared with the worst finished score (-1e9 while
  fewer than B are finished).  Once it is not greater, no improvement counts as possible, for good.
* the search goes on while improvement is possible, and the finished list is not full with ``early_stopping=True``, and some candidate
  of the step did not hit.  So ``early_stopping=True`` stops at B finished hypotheses, ``False`` applies the heuristic with the current
  length, ``"never"`` with the greatest one.
* ``generate`` does not run ``_beam_search`` for ``num_beams=1``: it decodes greedily and stops at the first EOS id.  One beam
  therefore searches as with ``early_stopping=True``: its first finished hypothesis ends it.
* the result is the finished list, best first.  (The search always ends with B entries: it cannot stop on the heuristic or on
  ``early_stopping`` before B are finished, and at the length limit the first B candidates all finish.)

Where this text and ``transformers`` differ, ``transformers`` is right: tests/test_beam_cpu.py compares the two.

Out of scope: beam slots that sample, penalise, run a grammar or stop sets (the engine refuses them), diverse / grouped beams, beam
groups inside ``batch_generate_ids`` / ``serve_requests``, and a reorder that runs without the host.
"""

from __future__ import annotations

from typing import Callable, Sequence

MAX_BEAMS = 8        # TL_MAX_BEAMS
MAX_CANDIDATES = 32  # TL_MAX_BEAM_CANDIDATES
_NEVER = -1.0e9      # transformers' score of "no hypothesis"

Candidate = tuple[int, int, float, float]  # (parent, token, score, logprob)


def beam_candidates(num_beams: int, n_eos: int) -> int:
    """How many candidates a step selects: ``max(2, 1 + n_eos) * num_beams``; ValueError beyond the device's 8 beams / 32 candidates."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= MAX_BEAMS:
        raise ValueError(f"num_beams must be an int in [1, {MAX_BEAMS}], got {num_beams!r}")
    if (1 + n_eos) * num_beams > MAX_CANDIDATES:
        raise ValueError(f"(1 + {n_eos} EOS ids) * {num_beams} beams exceeds the {MAX_CANDIDATES} candidates a step can select")
    return max(2, 1 + n_eos) * num_beams


def beam_search(select: Callable[[list[float], int], Sequence[Candidate]], advance: Callable[[list[int], list[int]], None], *,
                num_beams: int, max_new_tokens: int, eos_ids: Sequence[int] = (), length_penalty: float = 1.0,
                early_stopping: bool | str = False) -> list[tuple[list[int], float]]:
    """The hypotheses of one prompt, best first, as (generated ids, score).

    ``select(scores, n_cand)``: the best ``n_cand`` continuations of the running beams, whose cumulative log-probabilities are
    ``scores`` (beam i is row i), as (parent, token, score, logprob) best first; entries with parent < 0 are ignored.
    ``advance(parents, tokens)``: the running beams become ``[beam parents[i] + tokens[i]]`` and the model takes one step, so that the
    next ``select`` sees their rows.  It is not called after the last step."""
    if early_stopping not in (True, False, "never"):
        raise ValueError('early_stopping is True, False or "never"')
    if isinstance(max_new_tokens, bool) or not isinstance(max_new_tokens, int) or max_new_tokens < 1:
        raise ValueError("max_new_tokens must be a positive int")
    eos = {int(t) for t in eos_ids}
    if num_beams == 1:
        early_stopping = True  # (generate's greedy search: the first EOS ends it)
    B, K = num_beams, beam_candidates(num_beams, len(eos))
    length_penalty = float(length_penalty)
    running: list[tuple[list[int], float]] = [([], 0.0)]
    finished: list[tuple[list[int], float]] = []
    improvable = True
    for step in range(max_new_tokens):
        generated = step + 1
        cands = [c for c in select([s for _, s in running], K) if c[0] >= 0]
        hits = [generated >= max_new_tokens or c[1] in eos for c in cands]
        full = len(finished) == B
        # the hypotheses that finish: ranked inside the first B, merged behind the ones already there (the order of equal scores)
        if improvable and not (full and early_stopping is True):
            finished += [(running[c[0]][0] + [c[1]], c[2] / generated ** length_penalty) for c, hit in zip(cands[:B], hits) if hit]
            finished = sorted(finished, key=lambda h: -h[1])[:B]
        nxt = [c for c, hit in zip(cands, hits) if not hit][:B]
        full = len(finished) == B
        if nxt:
            longest = max_new_tokens if early_stopping == "never" and length_penalty > 0.0 else generated
            worst = min(s for _, s in finished) if full else _NEVER
            improvable = improvable and nxt[0][2] / longest ** length_penalty > worst
        if not nxt or not improvable or (full and early_stopping is True):
            break
        running = [(running[p][0] + [t], s) for p, t, s, _ in nxt]
        advance([c[0] for c in nxt], [c[1] for c in nxt])
    return finished


def beam_search_ids(engine, prompt_ids: Sequence[int], num_beams: int, max_new_tokens: int, eos_ids: Sequence[int] = (),
                    length_penalty: float = 1.0, early_stopping: bool | str = False, slot0: int = 0) -> list[tuple[list[int], float]]:
    """Beam search of one prompt on ``engine`` in slots [slot0, slot0 + num_beams), which must be free: prefill into ``slot0``, select
    over its one row, reorder 1 -> B, then ``decode(1)`` / select / reorder per step, then release.  Returns the hypotheses best first
    as (generated ids, score), the policy and scores of ``beam_search``.  The decode steps run over slots [0, slot0 + num_beams): other
    requests living in lower slots advance with the group."""
    beam_candidates(num_beams, len(set(eos_ids)))  # (the arguments are checked before a slot is taken)
    if slot0 < 0 or slot0 + num_beams > engine.max_batch:
        raise ValueError(f"beam_search_ids: slots [{slot0}, {slot0 + num_beams}) are not inside the engine's {engine.max_batch}")
    prompt = [int(t) for t in prompt_ids]
    width = [0]  # slots of the group that hold a beam; 0: the prompt's row is row 0 of a prefill

    def select(scores, n_cand):
        return engine.beam_select(slot0 if width[0] else 0, len(scores), scores, n_cand)

    def advance(parents, tokens):
        engine.beam_reorder(slot0, max(width[0], 1), parents, tokens)
        width[0] = len(parents)
        engine.decode(1, batch=slot0 + width[0])

    engine.begin(slot0)
    try:
        engine.prefill(slot0, prompt)
        return beam_search(select, advance, num_beams=num_beams, max_new_tokens=max_new_tokens, eos_ids=eos_ids,
                           length_penalty=length_penalty, early_stopping=early_stopping)
    finally:
        for slot in range(slot0, slot0 + max(width[0], 1)):
            engine.release(slot)
