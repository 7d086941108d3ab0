"""HiFi-GAN generator golden fixture, produced by running the REFERENCE's own hifi_gan/models.Generator
(/root/reference/hifi_gan/models.py:75-125) on CPU in fp32 and in float64, as _decoder_golden.py does for the
decoder.  Writes hifigan_golden.npz beside this file.

Per case only the mel, the fp32 output, the float64 output, the reference's ordered state_dict key names and the
recipe seed are stored: the weights are weights_recipe.apply_recipe(model, seed) on the weight-normed parameters
(weight_g / weight_v / bias), which any module with the reference's parameter names reproduces.

A case must not be flattened by the final tanh (errors would hide in the saturation): std > 0.05 and no sample
with |wav| > 0.999.  The first recipe seed from 1 upward that passes both is taken and recorded.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference/hifi_gan")

CASES = {
    "v1_small": dict(resblock="1", upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4],
                     upsample_initial_channel=128, resblock_kernel_sizes=[3, 7, 11],
                     resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]]),
    "v3_small": dict(resblock="2", upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8],
                     upsample_initial_channel=64, resblock_kernel_sizes=[3, 5, 7],
                     resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]]),
}


def run_case(cfg, seed, mel):
    import copy

    import torch
    from env import AttrDict  # the reference's hifi_gan/env.py
    from models import Generator  # the reference's hifi_gan/models.py
    from weights_recipe import apply_recipe

    model = Generator(AttrDict(cfg))
    apply_recipe(model, seed)
    model.eval()
    keys = list(model.state_dict().keys())
    with torch.no_grad():
        y32 = model(mel)
        y64 = copy.deepcopy(model).double()(mel.double())
        folded = copy.deepcopy(model)
        folded.remove_weight_norm()
        y_folded = folded(mel)
    return model, keys, y32, y64, y_folded


def main():
    sys.path.insert(0, str(REF))
    sys.path.insert(0, str(HERE))
    import torch

    torch.set_num_threads(8)
    mel = torch.randn(2, 80, 24, generator=torch.Generator().manual_seed(5)) * 1.5 - 5.5
    out: dict[str, np.ndarray] = {}
    for name, cfg in CASES.items():
        for seed in range(1, 33):
            model, keys, y32, y64, y_folded = run_case(cfg, seed, mel)
            std, sat = float(y64.std()), float((y64.abs() > 0.999).double().mean())
            if std > 0.05 and sat == 0.0:
                break
            print(f"{name}: seed {seed} rejected (std {std:.3f}, saturated share {sat:.4f})")
        else:
            raise SystemExit(f"{name}: no recipe seed in 1..32 gives an unsaturated output")
        assert std > 0.05 and sat == 0.0
        nparams = sum(p.numel() for p in model.parameters())
        err = float((y32.double() - y64).abs().max())
        print(f"{name}: seed {seed}, {nparams} parameters, out {tuple(y32.shape)}, std {std:.3f}, "
              f"fp32 vs float64 {err:.2e}, remove_weight_norm changes the output by "
              f"{float((y_folded - y32).abs().max()):.1e}")
        out[name + "/mel"] = mel.numpy()
        out[name + "/out_f32"] = y32.numpy()
        out[name + "/out_f64"] = y64.numpy()
        out[name + "/keys"] = np.array(keys)
        out[name + "/seed"] = np.array(seed, np.int64)
    np.savez_compressed(HERE / "hifigan_golden.npz", **out)
    print("wrote hifigan_golden.npz")


if __name__ == "__main__":
    main()
