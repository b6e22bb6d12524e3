"""CPU tier: the numpy restatement of the decode engine's truncation (tests/truncation_oracle.py) against transformers' warpers and the
properties of Mirostat v2, the argument validation of the Python layer, and the cap on what the oracle leaves undecided -- asserted here
for exactly the rows the GPU test uses.  No kernel is launched here."""

import math
from pathlib import Path

import numpy as np
import pytest

import truncation_oracle as R

ROOT = Path(__file__).resolve().parent.parent


def _hf_kept(warper, x, T):
    import torch

    scores = torch.from_numpy((np.asarray(x, dtype=np.float64) / T)[None])
    return (warper(None, scores)[0] > -math.inf).numpy()


def test_bf16_bits_round_to_nearest_even():
    import torch

    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 50, np.float32([0.0, -0.0, 1.00390625, 1.01171875, np.inf, -np.inf])])
    want = torch.from_numpy(v).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(v), want)
    assert np.array_equal(R.bf16_values(want), torch.from_numpy(v).bfloat16().float().numpy())


def test_min_p_equals_transformers():
    transformers = pytest.importorskip("transformers")
    bits = R.make_rows(1024)
    vals = R.bf16_values(bits)
    for i in range(R.N_ROWS):
        for T in R.TEMPERATURES:
            for mp in R.MIN_PS:
                k, _, und = R.kept(vals[i], T, mp)
                assert not und.any()
                assert np.array_equal(k, _hf_kept(transformers.MinPLogitsWarper(min_p=mp), vals[i], T)), (i, T, mp)


def test_typical_contains_transformers_and_extras_tie_with_the_boundary():
    transformers = pytest.importorskip("transformers")
    bits = R.make_rows(1024)
    vals = R.bf16_values(bits)
    decided = 0
    for i in range(R.N_ROWS):
        for T in R.TEMPERATURES:
            for tp in R.TYPICAL_PS:
                k, _, und = R.kept(vals[i], T, 0.0, tp)
                if und.any():
                    continue  # a boundary decision within rounding: float32 in the warper may fall on either side
                decided += 1
                hf = _hf_kept(transformers.TypicalLogitsWarper(mass=tp), vals[i], T)
                assert not (hf & ~k).any(), (i, T, tp)
                _, d_star, d = R.typical_set(vals[i], T, tp)
                extra = k & ~hf
                assert np.allclose(d[extra], d_star, rtol=1e-12, atol=0), (i, T, tp)
    assert decided >= 100


def test_mirostat_properties():
    vals = R.bf16_values(R.make_rows(1024))
    for i in range(R.N_ROWS):
        for T in R.TEMPERATURES:
            for mu in (-5.0, 0.0, 0.5, 2.0, 8.0, 30.0):
                k, _, _ = R.kept(vals[i], T, mu=mu)
                assert k.any() and k[int(np.argmax(vals[i]))]
    # every surprise equals tau: a row of 2^tau equal logits, all kept -- mu stays at 2 tau
    tau, eta = 4.0, 0.3
    row = np.zeros(16)
    assert R.kept(row, 1.0, mu=2 * tau)[0].all()
    assert R.mirostat_update(row, 5, 1.0, tau, eta, 2 * tau) == pytest.approx(2 * tau, abs=1e-12)
    # mu moves against the sign of s - tau
    x = vals[0].astype(np.float64)
    k, _, _ = R.kept(x, 1.0, mu=12.0)
    f = np.where(k, x, -np.inf)
    order = np.argsort(-f)
    likely, rare = int(order[0]), int(order[int(k.sum()) - 1])
    s = lambda t: (12.0 - R.mirostat_update(f, t, 1.0, 0.0, 1.0, 12.0))  # eta 1, tau 0: mu - mu' = s
    assert s(likely) < s(rare)
    for t in (likely, rare):
        for tau in (0.5 * s(t), 2.0 * s(t) + 0.1):
            moved = R.mirostat_update(f, t, 1.0, tau, 0.2, 12.0) - 12.0
            assert moved * (s(t) - tau) < 0


@pytest.mark.parametrize("V", R.VOCABS)
def test_undecided_cap_on_the_gpu_tests_rows(V):
    """Undecided tokens are at most 0.5 % of a row, for every row and parameter set tests/test_zz_truncation_gpu.py feeds the kernel."""
    vals = R.bf16_values(R.make_rows(V))
    worst = {c: 0.0 for c in R.COMBOS}
    for c in R.COMBOS:
        for i in range(R.N_ROWS):
            k, dr, und = R.kept(vals[i], *R.row_params(i, c))
            assert (k.astype(int) + dr + und == 1).all()
            worst[c] = max(worst[c], und.mean())
    print(V, {c: f"{100 * w:.3f} %" for c, w in worst.items()})
    assert max(worst.values()) <= 0.005, worst


def test_undecided_cap_over_the_generator_grid():
    """... and over the whole grid of the generator at V = 1,024: T x typical_p x min_p."""
    vals = R.bf16_values(R.make_rows(1024))
    for i in range(R.N_ROWS):
        for T in R.TEMPERATURES:
            for tp in R.TYPICAL_PS:
                for mp in (0.0,) + R.MIN_PS:
                    assert R.kept(vals[i], T, mp, tp)[2].mean() <= 0.005, (i, T, tp, mp)


def test_truncation_args_and_request_truncation():
    from tiny_llm_hip.engine import request_settings, truncation_args

    assert truncation_args() == (0.0, 1.0, 0.0, 0.0)
    assert truncation_args(0.05, 0.9) == (0.05, 0.9, 0.0, 0.0)
    assert truncation_args(mirostat_tau=5) == (0.0, 1.0, 5.0, 0.1)
    assert truncation_args(typical_p=None, mirostat_tau=5, mirostat_eta=1) == (0.0, 1.0, 5.0, 1.0)
    for bad in (dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=math.nan), dict(min_p=True), dict(typical_p=0.0), dict(typical_p=1.2),
                dict(typical_p="0.9"), dict(mirostat_tau=-1.0), dict(mirostat_tau=math.inf), dict(mirostat_tau=5, mirostat_eta=0.0),
                dict(mirostat_tau=5, mirostat_eta=1.5)):
        with pytest.raises(ValueError):
            truncation_args(**bad)
    # Mirostat excludes every other truncation
    for bad in (dict(min_p=0.05), dict(typical_p=0.9), dict(top_k=40), dict(top_p=0.9)):
        with pytest.raises(ValueError, match="excludes"):
            truncation_args(mirostat_tau=5.0, **bad)
    def request_truncation(sampling, n):
        return [s.truncation for s in request_settings(sampling, n, vocab_size=100)]

    assert request_truncation(None, 3) == [(0.0, 1.0, 0.0, 0.0)] * 3  # neutral: RequestSettings.apply makes no call
    d = {"temperature": 0.8, "min_p": 0.05, "typical_p": 0.9, "top_k": 40}
    assert request_truncation(d, 2) == [(0.05, 0.9, 0.0, 0.0)] * 2
    assert request_truncation([{"temperature": 1.0, "mirostat_tau": 5.0}, {}], 2) == [(0.0, 1.0, 5.0, 0.1), (0.0, 1.0, 0.0, 0.0)]
    with pytest.raises(ValueError, match="excludes"):
        request_truncation({"temperature": 1.0, "mirostat_tau": 5.0, "top_p": 0.9}, 1)
    # the other fields of the same record
    assert request_settings(d, 1, vocab_size=100)[0].sampling[:3] == (0.8, 40, 1.0)
    assert request_settings(d, 1, vocab_size=100)[0].penalties == (1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        request_settings({"minp": 0.1}, 1)


def test_cli_flags_refuse_mirostat_with_another_truncation():
    import subprocess
    import sys

    for script, extra in (("main.py", ["--sampler-top-p", "0.9"]), ("batch_main.py", ["--sampler-min-p", "0.05"])):
        r = subprocess.run([sys.executable, str(ROOT / script), "--model", "no-such-checkpoint", "--mirostat-tau", "5", "--sampler-temp", "0.8"] + extra, capture_output=True, text=True, cwd=ROOT)
        assert r.returncode != 0 and "excludes" in (r.stderr + r.stdout), (script, r.stderr[-400:])


def test_header_and_sources_declare_the_interface():
    header = (ROOT / "include" / "tinyllm_engine.h").read_text()
    for needle in ("tl_engine_set_truncation", "tl_engine_set_mirostat", "tl_engine_mirostat_mu", "tl_engine_copy_filtered_logits", "tl_truncate_rows",
                   "tl_mirostat_update_rows", "closed under ties"):
        assert needle in header, needle
    engine = (ROOT / "tiny-llm_amd" / "csrc" / "engine.hip").read_text()
    route = (ROOT / "tiny-llm_amd" / "csrc" / "replay_route.h").read_text()  # the plan key's bits, which engine.hip takes from there
    assert '#include "truncate.h"' in engine and '#include "replay_route.h"' in engine and "1L << 57" in route
