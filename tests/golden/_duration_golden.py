"""duration_path_golden.npz: the dense alignments of tests/test_duration_path_cpu.py's cases, produced by running
the REFERENCE's own builder (matcha/utils/model.py:77-114, build_alignment_path; bound as generate_path in
matcha_tts.py) on CPU in fp32 under the mask x_mask * y_mask of matcha_tts.py:271-274.

    python tests/golden/_duration_golden.py <reference checkout>

Only this script reads the reference; the tests read the fixture (inputs + int8 paths, data only)."""
from __future__ import annotations

import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))


def main(ref_root: str) -> None:
    from test_duration_path_cpu import attn_mask, cases

    spec = importlib.util.spec_from_file_location("ref_utils_model", Path(ref_root) / "matcha" / "utils" / "model.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, d, xl, yl, Ty in cases():
        path = ref.build_alignment_path(torch.from_numpy(d), attn_mask(xl, yl, d.shape[1], Ty)).numpy()
        assert np.isin(path, (0.0, 1.0)).all(), name
        out[name + "_d"], out[name + "_xl"], out[name + "_yl"] = d, xl, yl
        out[name + "_path"] = path.astype(np.int8)
    np.savez_compressed(HERE / "duration_path_golden.npz", **out)
    print(f"wrote {len(out) // 4} cases, {(HERE / 'duration_path_golden.npz').stat().st_size} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
