"""load_weights(..., quantize=True) on UNQUANTISED checkpoints (bf16 tensors under the Hugging Face names, no `quantization` key):
every linear and the embedding table come back as quantize_affine of the written weights, bit for bit -- through the torch quantiser on
the CPU, through the HIP kernel on the device, where the engine must also compute what it computes from the pre-quantised checkpoint."""
import json
from functools import reduce

import numpy as np
import pytest
import torch
from safetensors.torch import load_file, save_file

from checkpoint_fixture import MOE_CFG_OVERRIDES, _bf16, _u32, make_moe_weights, write_checkpoint
from helpers import TINY_CFG
from oracle import tiny_oracle as O
from tiny_llm_hip import loader


def write_unquantised(path, cfg, w):
    """The fixture's checkpoint with every W4 triple replaced by its dequantised bf16 matrix (stacked experts split into transformers'
    mlp.experts.{e}); a pre-quantised twin beside it; and {layer prefix: quantize_affine(matrix)}, what both must load as."""
    ckpt = write_checkpoint(path, cfg, w)
    stored, raw, twin, want = load_file(ckpt / "model.safetensors"), {}, {}, {}
    for name, t in stored.items():
        base = name[: -len(".weight")]
        if name.endswith((".scales", ".biases")):
            continue
        if base + ".scales" not in stored:
            raw[name] = twin[name] = t
            continue
        dense = O.dequantize_weights(t.view(torch.int32).numpy().view(np.uint32), stored[base + ".scales"].float().numpy(), stored[base + ".biases"].float().numpy())
        want[base] = [x.reshape(*dense.shape[:-1], -1) for x in O.quantize_affine(dense.reshape(-1, dense.shape[-1]))]
        twin[name], twin[base + ".scales"], twin[base + ".biases"] = _u32(want[base][0]), _bf16(want[base][1]), _bf16(want[base][2])
        if dense.ndim == 3:
            raw.update({f"{base.replace('.switch_mlp.', f'.experts.{e}.')}.weight": _bf16(m) for e, m in enumerate(dense)})
        else:
            raw[name] = _bf16(dense)
    save_file(twin, str(write_checkpoint(path.with_name(path.name + "_w4"), cfg, w) / "model.safetensors"))
    save_file(raw, str(ckpt / "model.safetensors"))
    config = json.loads((ckpt / "config.json").read_text())
    (ckpt / "config.json").write_text(json.dumps({k: v for k, v in config.items() if k != "quantization"}))
    return ckpt, want


def check_tree(model, want):
    assert len(want) >= 15
    for prefix, (packed, scales, biases) in want.items():
        layer = reduce(lambda o, p: o[int(p)] if p.isdigit() else getattr(o, p), prefix.split("."), model)
        assert layer.weight.dtype == torch.int32 and layer.scales.dtype == torch.bfloat16 and (layer.group_size, layer.bits) == (128, 4)
        np.testing.assert_array_equal(layer.weight.cpu().numpy().view(np.uint32), packed, err_msg=prefix)
        np.testing.assert_array_equal(layer.scales.float().cpu().numpy(), scales, err_msg=prefix)
        np.testing.assert_array_equal(layer.biases.float().cpu().numpy(), biases, err_msg=prefix)


@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_an_unquantised_checkpoint_loads_as_quantize_affine_of_its_weights(tmp_path, kind):
    cfg = dict(TINY_CFG, tie_word_embeddings=False) if kind == "dense" else dict(TINY_CFG, **MOE_CFG_OVERRIDES)
    w = O.make_qwen3_weights(cfg, seed=4, sigma=0.05) if kind == "dense" else make_moe_weights(cfg, seed=4)
    ckpt, want = write_unquantised(tmp_path / kind, cfg, w)
    model = loader.load_weights(ckpt, device="cpu", quantize=True)
    check_tree(model, want)
    assert model.model.norm.weight.dtype == torch.bfloat16 and hasattr(model, "lm_head") == (kind == "dense")
    with pytest.raises(ValueError, match="not quantized"):
        loader.load_weights(ckpt, device="cpu")


@pytest.mark.gpu
def test_on_the_device_the_kernel_quantises_and_the_engine_computes_the_same_logits(tmp_path):
    from tiny_llm_hip.engine import DecodeEngine

    ckpt, want = write_unquantised(tmp_path / "dense", TINY_CFG, O.make_qwen3_weights(TINY_CFG, seed=4, sigma=0.05))
    models = [loader.load_weights(ckpt, device="cuda", quantize=True), loader.load_weights(ckpt.with_name("dense_w4"), device="cuda")]
    check_tree(models[0], want)
    logits = []
    for model in models:
        engine = DecodeEngine(model, page_size=16, num_pages=16, max_batch=1, max_prefill_rows=16)
        engine.begin(0)
        engine.prefill(0, [5, 17, 900, 33, 2])
        logits.append(engine.logits(1)[0].clone())
        engine.release(0)
        engine.close()
    assert torch.equal(logits[0], logits[1])
