#!/usr/bin/env python3
"""Generate the NIC / Show-and-Tell golden vectors by IMPORTING THE REFERENCE'S NIC_RNNDecoder (build machine only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nic.py <root of a checkout of the reference>
      (or DIC_REFERENCE_ROOT=<root>)
Writes tests/golden/nic_*.npz and nic_state_dict_keys.json; nothing of the reference is committed, only these outputs.  Inputs and
weights are regenerated procedurally (synthetic.nic_weights / nic_map / captions_ragged) from the seeds in tests/nic_common.py.

Captioning_models/Base_caption_model/nic.py imports torchvision, Captioning_models.util and Captioning_models.evaluate_metrix at
module level; none of them is needed by NIC_RNNDecoder and none is importable here, so this script registers empty stand-in modules
of its own under those names before the import.  NIC_CNNEncoder cannot be constructed without torchvision; its trainable part is one
nn.Linear(2048, 300), which this script applies itself (torch.nn.Linear) to the pooled [B,2048] input.  Dropout is made an explicit
input with the FixedDropout idea of make_golden.py; here the multiplier is applied to the packed rows."""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DIC_REFERENCE_ROOT")
if not REFERENCE or not os.path.isdir(os.path.join(REFERENCE, "Captioning_models")):
    raise SystemExit("usage: make_golden_nic.py <root of a checkout of Kyo-suke-S/Depth_image_captioning_pub>")
sys.path.insert(0, ROOT)
sys.path.insert(0, REFERENCE)
sys.dont_write_bytecode = True


def _stand_in(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


tv = _stand_in("torchvision")
tv.models = _stand_in("torchvision.models")
tv.transforms = _stand_in("torchvision.transforms")
tv.datasets = _stand_in("torchvision.datasets")
_stand_in("tqdm", tqdm=lambda it, **kw: it) if "tqdm" not in sys.modules else None
import Captioning_models  # noqa: E402  (reference package)
_stand_in("Captioning_models.util")
_stand_in("Captioning_models.evaluate_metrix", load_textfiles=None, score=None)
_stand_in("Captioning_models.config", ConfigTrain=object, ConfigEval=object)

from Captioning_models.Base_caption_model.nic import NIC_RNNDecoder  # noqa: E402  (reference)

from depth_image_captioning_pub_amd import synthetic as syn  # noqa: E402
from tests import nic_common as nc  # noqa: E402
from tests.helpers import SUB  # noqa: E402

BIG = 1 << 14      # tensors above this many elements are stored as a strided subsample + sum + L2 norm (tests.helpers.check_packed)


def pack(t, name, out):
    a = t.detach().cpu().contiguous().numpy()
    if a.size <= BIG:
        out[name] = a
        return
    flat = a.reshape(-1)
    out[name + "__sub"] = flat[::SUB].copy()
    out[name + "__sum"] = np.float64(flat.astype(np.float64).sum())
    out[name + "__l2"] = np.float64(np.sqrt((flat.astype(np.float64) ** 2).sum()))
    out[name + "__shape"] = np.asarray(a.shape, np.int64)


class FixedDropoutPacked(nn.Module):
    """Stands in for decoder.dropout: h * mult on the packed rows (nn.Dropout's train-mode arithmetic, mask as an input)."""

    def __init__(self, mult_packed):
        super().__init__()
        self.mult = mult_packed

    def forward(self, h):
        return h * self.mult


def _modules(name):
    w, hw, fmap, caps, lens, drop = nc.case_inputs(name)
    dec = NIC_RNNDecoder(300, 128, w["linear.weight"].shape[0], 2, 0.5)
    dec.load_state_dict(w, strict=True)
    lin = nn.Linear(2048, 300)
    lin.load_state_dict({k[len('linear.'):]: v for k, v in hw.items()}, strict=True)
    return dec, lin, fmap, caps, lens, drop


def case_teacher_forced(name):
    out = {}
    dec, lin, fmap, caps, lens, drop = _modules(name)
    train = drop is not None
    dec.train(train)
    if train:
        dec.dropout = FixedDropoutPacked(pack_padded_sequence(drop, lens, batch_first=True).data)
    packed_ref = pack_padded_sequence(caps, lens, batch_first=True)
    logits = dec(lin(fmap.mean(1)), caps, lens)
    loss = F.cross_entropy(logits, packed_ref.data)
    out["batch_sizes"] = packed_ref.batch_sizes.numpy().astype(np.int64)
    pack(logits, "logits", out)
    out["loss"] = np.float32(loss.item())
    out["argmax"] = logits.argmax(1).numpy().astype(np.int64)
    if train:
        named = list(dec.named_parameters()) + [("encoder.linear." + k, p) for k, p in lin.named_parameters()]
        opt = torch.optim.AdamW([p for _, p in named], lr=1e-3)          # nic.py:243-245
        opt.zero_grad()
        loss.backward()
        for k, p in named:
            pack(p.grad, "grad." + k, out)
        opt.step()
        for k, p in named:
            pack(p, "adamw1." + k, out)
    np.savez_compressed(os.path.join(HERE, f"nic_{name}.npz"), **out)
    print(name, "loss", out["loss"], "N", int(logits.shape[0]))


def case_adamw3():
    """Three optimiser steps on the ragged batch, dropout off (weight seed 73)."""
    out = {}
    w, hw = syn.nic_weights(50, seed=73)
    fmap = syn.nic_map(5, 1, 74)
    caps, lens = syn.captions_ragged([9, 7, 7, 4, 3], 50, seed=73)
    dec = NIC_RNNDecoder(300, 128, 50, 2, 0.5)
    dec.load_state_dict(w, strict=True)
    lin = nn.Linear(2048, 300)
    lin.load_state_dict({k[len('linear.'):]: v for k, v in hw.items()}, strict=True)
    dec.eval()
    named = list(dec.named_parameters()) + [("encoder.linear." + k, p) for k, p in lin.named_parameters()]
    opt = torch.optim.AdamW([p for _, p in named], lr=1e-3)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        logits = dec(lin(fmap.mean(1)), caps, lens)
        loss = F.cross_entropy(logits, pack_padded_sequence(caps, lens, batch_first=True).data)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out["losses"] = np.asarray(losses, np.float32)
    for k, p in named:
        pack(p, "adamw3." + k, out)
    np.savez_compressed(os.path.join(HERE, "nic_adamw3.npz"), **out)
    print("adamw3", losses)


def case_batch_sample():
    out = {}
    w, hw, fmap = nc.greedy_inputs("golden")
    dec = NIC_RNNDecoder(300, 128, w["linear.weight"].shape[0], 2, 0.5)
    dec.load_state_dict(w, strict=True)
    dec.eval()
    feats = F.linear(fmap.mean(1), hw["linear.weight"], hw["linear.bias"])
    ids = dec.batch_sample(feats, max_length=30)
    out["ids"] = np.asarray(ids, np.int64)
    assert dec.sample(feats[:1], max_length=30) == ids[0]
    _, gap64, _ = nc.greedy_run("golden", True)          # the whole evaluation in fp64, head included
    out["min_gap_fp64"] = np.float64(gap64.min())
    np.savez_compressed(os.path.join(HERE, "nic_batch_sample.npz"), **out)
    print("batch_sample", ids[0][:10], "distinct", len({t for row in ids for t in row}), "gap", float(gap64.min()))


def case_state_dict_keys():
    mod = NIC_RNNDecoder(300, 128, 50, 2, 0.5)
    out = {"NIC_RNNDecoder": {"state_dict": {k: list(v.shape) for k, v in mod.state_dict().items()},
                              "parameters": [k for k, _ in mod.named_parameters()]}}
    with open(os.path.join(HERE, "nic_state_dict_keys.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("state_dict_keys ok")


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(8)
    for name in ("ragged_train", "ragged_eval", "equal_train"):
        case_teacher_forced(name)
    case_adamw3()
    case_batch_sample()
    case_state_dict_keys()
