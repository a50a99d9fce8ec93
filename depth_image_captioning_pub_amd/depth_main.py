"""CLI with the reference's argument convention (depth_main.py:14-35):
    python -m depth_image_captioning_pub_amd.depth_main {soft,hard} cnn {coco,original,synthetic} [--scst-epochs N]
(the reference script itself does not run as shipped - quirk Q5 - so this keeps its intent: 3 repetitions of
train_Cdepth_{soft,hard}(i, useData)).  `mlp` is a no-op in the reference (depth_main.py:27-28,34-35) and here.
--scst-epochs N (not in the reference): N further epochs of self-critical training behind the cross-entropy epochs
(CaptionTrainer.scst_step, soft attention only; default: config.scst_epochs = 0)."""
from __future__ import annotations

import sys

import numpy as np
import torch

from .Captioning_models.Depth_caption_model.depth_train import train_Cdepth_hard, train_Cdepth_soft


EXP_TIME = 3                                   # depth_main.py:16: every experiment is repeated three times


def torch_seed(seed=123):                      # depth_main.py:7-12
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    np.random.seed(seed)


def take_scst_epochs(args):
    """(args without `--scst-epochs N` / `--scst-epochs=N`, N or None when the option is absent); ValueError on a bad value."""
    rest, n, i = [], None, 0
    while i < len(args):
        a = str(args[i])
        if a == "--scst-epochs" or a.startswith("--scst-epochs="):
            if "=" in a:
                value = a.split("=", 1)[1]
            else:
                i += 1
                if i >= len(args):
                    raise ValueError("--scst-epochs needs a value")
                value = str(args[i])
            try:
                n = int(value)
            except ValueError:
                raise ValueError(f"--scst-epochs needs a non-negative integer, got {value!r}") from None
            if n < 0:
                raise ValueError(f"--scst-epochs needs a non-negative integer, got {value!r}")
        else:
            rest.append(args[i])
        i += 1
    return rest, n


def main(argv=None):
    torch_seed()
    exp_time = EXP_TIME
    datas = ["coco", "original", "synthetic"]
    try:
        args, scst_epochs = take_scst_epochs(list(sys.argv if argv is None else argv))
    except ValueError as e:
        print(e)
        return 1
    if len(args) < 4:
        print("input {soft/hard} {cnn/mlp} {coco/original/synthetic}")
        return 1
    kind, enc, use_data = args[1], args[2], args[3]
    if enc == "mlp":
        return 0
    if use_data not in datas:
        print("input {soft/hard} {cnn/mlp} {coco/original/synthetic}")
        return 1
    fn = {"soft": train_Cdepth_soft, "hard": train_Cdepth_hard}.get(kind)
    if fn is None:
        print("input {soft/hard} {cnn/mlp} {coco/original/synthetic}")
        return 1
    for i in range(exp_time):
        fn(i, use_data, scst_epochs=scst_epochs)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
