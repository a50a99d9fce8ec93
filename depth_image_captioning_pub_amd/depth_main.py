"""CLI with the reference's argument convention (depth_main.py:14-35):
    python -m depth_image_captioning_pub_amd.depth_main {soft,hard} cnn {coco,original,synthetic} [--scst-epochs N]
                                                         [--ss-start N --ss-every K --ss-inc P --ss-max P]
                                                         [--clip-grad-norm X] [--label-smoothing E]
(the reference script itself does not run as shipped - quirk Q5 - so this keeps its intent: 3 repetitions of
train_Cdepth_{soft,hard}(i, useData)).  `mlp` is a no-op in the reference (depth_main.py:27-28,34-35) and here.
--scst-epochs N (not in the reference): N further epochs of self-critical training behind the cross-entropy epochs
(CaptionTrainer.scst_step, soft attention only; default: config.scst_epochs = 0).
--ss-start N --ss-every K --ss-inc P --ss-max P (not in the reference): scheduled sampling in the cross-entropy epochs - from
epoch N on the decoder is fed its own tokens with a probability that rises by P every K epochs up to the maximum
(Captioning_models/scheduled.py; defaults 5, 0.05, 0.25).  The default --ss-start -1 means off.
--clip-grad-norm X (not in the reference): every optimiser update clips the gradient to the global L2 norm X, a finite number
above 0, on the device (the trainers' max_grad_norm; default: config.clip_grad_norm = None, no clipping).
--label-smoothing E (not in the reference): the cross-entropy epochs minimise F.cross_entropy's label-smoothed loss with E in
[0, 1] (the trainers' label_smoothing; default: config.label_smoothing = 0, the plain loss) and print the plain
negative log-likelihood beside it; validation loss and the self-critical epochs stay unsmoothed."""
from __future__ import annotations

import math
import sys

import numpy as np
import torch

from .Captioning_models.Depth_caption_model import depth_train
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


SS_OPTIONS = {"--ss-start": ("start", int, -1), "--ss-every": ("increase_every", int, 5), "--ss-inc": ("increase_prob", float, 0.05),
              "--ss-max": ("max_prob", float, 0.25)}


def take_scheduled_sampling(args):
    """(args without the --ss-* options, the scheduled_sampling dict of the training loops or None when --ss-start is absent or
    negative); ValueError on a bad value.  Both `--ss-start N` and `--ss-start=N` are read."""
    rest, got, i = [], {}, 0
    while i < len(args):
        a = str(args[i])
        name = a.split("=", 1)[0]
        if name in SS_OPTIONS:
            key, kind, _ = SS_OPTIONS[name]
            if "=" in a:
                value = a.split("=", 1)[1]
            else:
                i += 1
                if i >= len(args):
                    raise ValueError(f"{name} needs a value")
                value = str(args[i])
            try:
                got[key] = kind(value)
            except ValueError:
                raise ValueError(f"{name} needs {'an integer' if kind is int else 'a number'}, got {value!r}") from None
        else:
            rest.append(args[i])
        i += 1
    ss = {key: got.get(key, default) for key, _, default in SS_OPTIONS.values()}
    if ss["start"] < 0:
        return rest, None
    if ss["increase_every"] < 1:
        raise ValueError(f"--ss-every needs a positive integer, got {ss['increase_every']!r}")
    if not (0.0 <= ss["increase_prob"] <= 1.0 and 0.0 <= ss["max_prob"] <= 1.0):
        raise ValueError("--ss-inc and --ss-max need probabilities in [0, 1]")
    return rest, ss


def take_clip_grad_norm(args):
    """(args without `--clip-grad-norm X` / `--clip-grad-norm=X`, X as a float or None when the option is absent); ValueError on a
    value that is missing, not a number, not above 0 or not finite."""
    rest, x, i = [], None, 0
    while i < len(args):
        a = str(args[i])
        if a == "--clip-grad-norm" or a.startswith("--clip-grad-norm="):
            if "=" in a:
                value = a.split("=", 1)[1]
            else:
                i += 1
                if i >= len(args):
                    raise ValueError("--clip-grad-norm needs a value")
                value = str(args[i])
            try:
                x = float(value)
            except ValueError:
                raise ValueError(f"--clip-grad-norm needs a number, got {value!r}") from None
            if not (x > 0.0 and math.isfinite(x)):
                raise ValueError(f"--clip-grad-norm needs a finite number above 0, got {value!r}")
        else:
            rest.append(args[i])
        i += 1
    return rest, x


def take_label_smoothing(args):
    """(args without `--label-smoothing E` / `--label-smoothing=E`, E as a float or None when the option is absent); ValueError on a
    value that is missing, not a number or outside [0, 1]."""
    rest, x, i = [], None, 0
    while i < len(args):
        a = str(args[i])
        if a == "--label-smoothing" or a.startswith("--label-smoothing="):
            if "=" in a:
                value = a.split("=", 1)[1]
            else:
                i += 1
                if i >= len(args):
                    raise ValueError("--label-smoothing needs a value")
                value = str(args[i])
            try:
                x = float(value)
            except ValueError:
                raise ValueError(f"--label-smoothing needs a number, got {value!r}") from None
            if not 0.0 <= x <= 1.0:
                raise ValueError(f"--label-smoothing needs a number in [0, 1], got {value!r}")
        else:
            rest.append(args[i])
        i += 1
    return rest, x


def run_config(train_module, scheduled, clip_grad_norm=None, *, label_smoothing=None):
    """The config argument of a run: None (the training loop builds its own) without a schedule, without clipping and without
    label smoothing, else the loop's ConfigTrain with them set (the training entry points keep their signatures; all three travel
    in the config, as scst_epochs can)."""
    if scheduled is None and clip_grad_norm is None and label_smoothing is None:
        return None
    config = train_module.ConfigTrain()
    config.scheduled_sampling = scheduled
    config.clip_grad_norm = clip_grad_norm
    if label_smoothing is not None:
        config.label_smoothing = label_smoothing
    return config


def main(argv=None):
    torch_seed()
    exp_time = EXP_TIME
    datas = ["coco", "original", "synthetic"]
    try:
        args, scst_epochs = take_scst_epochs(list(sys.argv if argv is None else argv))
        args, scheduled = take_scheduled_sampling(args)
        args, clip = take_clip_grad_norm(args)
        args, smoothing = take_label_smoothing(args)
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
        fn(i, use_data, config=run_config(depth_train, scheduled, clip, label_smoothing=smoothing), scst_epochs=scst_epochs)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
