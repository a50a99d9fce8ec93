"""CPU: global-norm gradient clipping - the fp64 restatement the GPU tests use against torch's own clip_grad_norm_ + AdamW, the two
entry points in the prototype table, their host-side refusals (taken before the first HIP call), the --clip-grad-norm option and the
configuration default."""
import ctypes
import math

import pytest
import torch

from depth_image_captioning_pub_amd import _lib
from tests import clip_common as cc

_I, _LL, _F, _P = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p


@pytest.mark.parametrize("max_norm", [0.1, 1e6], ids=["clipping", "inactive"])
def test_restatement_matches_torch_clip_and_adamw(max_norm):
    """Three steps, the second on an outlier batch: clip_common against torch.nn.utils.clip_grad_norm_ followed by torch.optim.AdamW
    on fp64 CPU tensors.  Both sides are fp64 evaluations of the same formulas in slightly different operation orders: 1e-12."""
    gen = torch.Generator().manual_seed(5)
    shapes = {"a": (7, 5), "b": (33,), "c": (2, 3, 4)}
    init = {k: torch.randn(s, generator=gen, dtype=torch.float64) for k, s in shapes.items()}
    grads = [{k: torch.randn(s, generator=gen, dtype=torch.float64) * scale for k, s in shapes.items()} for scale in (0.05, 40.0, 0.05)]
    ref = {k: torch.nn.Parameter(v.clone()) for k, v in init.items()}
    opt = torch.optim.AdamW(list(ref.values()), lr=cc.ADAMW["lr"], betas=(cc.ADAMW["beta1"], cc.ADAMW["beta2"]), eps=cc.ADAMW["eps"],
                            weight_decay=cc.ADAMW["weight_decay"])
    p = {k: v.clone() for k, v in init.items()}
    m = {k: torch.zeros_like(v) for k, v in init.items()}
    v2 = {k: torch.zeros_like(v) for k, v in init.items()}
    coefs = []
    for step, g in enumerate(grads, 1):
        for k in ref:
            ref[k].grad = g[k].clone()
        total_ref = float(torch.nn.utils.clip_grad_norm_(list(ref.values()), max_norm))
        opt.step()
        total, coef = cc.clipped_adamw_step(p, g, m, v2, step, max_norm)
        coefs.append(coef)
        assert abs(total - total_ref) <= 1e-12 * total_ref
        for k in ref:
            assert torch.allclose(ref[k].grad, g[k] * coef, rtol=1e-12, atol=0.0), (step, k)        # (the scaling itself)
            assert torch.allclose(p[k], ref[k].detach(), rtol=1e-12, atol=1e-15), (step, k)
            state = opt.state[ref[k]]
            assert torch.allclose(m[k], state["exp_avg"], rtol=1e-12, atol=1e-18), (step, k)
            assert torch.allclose(v2[k], state["exp_avg_sq"], rtol=1e-12, atol=1e-24), (step, k)
    if max_norm < 1.0:
        assert all(c < 1.0 for c in coefs) and coefs[1] < 0.01 * coefs[0]      # every step clipped, the outlier hardest
    else:
        assert coefs == [1.0, 1.0, 1.0]


def test_prototypes_of_the_two_entry_points_read_by_hand():
    table = _lib.prototypes()
    assert table["dic_grad_norm"] == (_I, [_P, _LL, _P, _I, _F, _P, _P, _P, _P])
    assert table["dic_adamw_step_clipped"] == (_I, [_P, _P, _P, _P, _LL, _I, _F, _F, _F, _F, _F, _P, _P, _P])
    # the binding's constants are the header's macros; the scratch is one fp64 partial per workgroup and span, not a query
    import re
    from depth_image_captioning_pub_amd import native
    macro = {k: int(v) for k, v in re.findall(r"#define\s+DIC_GRAD_NORM_(\w+)\s+(\d+)", open(_lib.HEADER).read())}
    assert macro == {"BLOCKS": 1024, "MAX_SPANS": 8, "SCRATCH_BYTES": 1024 * 8 * 8}
    assert native.GRAD_NORM_SCRATCH_BYTES == macro["SCRATCH_BYTES"] and native.GRAD_NORM_MAX_SPANS == macro["MAX_SPANS"]
    assert native.GRAD_NORM_PASS == macro["BLOCKS"] * 256 * 4
    assert not any("grad_norm" in n and n.endswith("_workspace_bytes") for n in table)


def _last_error(lib) -> str:
    return lib.dic_last_error().decode()


def test_host_side_refusals_name_the_offending_value():
    """Every refusal comes before the first HIP call and before the null-pointer check, so the device pointers can be NULL and no GPU
    is needed (as for dic_nic_beam, tests/test_abi_cpu.py)."""
    lib = _lib.load()

    def ends(*values):
        return (ctypes.c_longlong * len(values))(*values)

    def refused(*args):
        assert lib.dic_grad_norm(*args) != 0
        return _last_error(lib)

    assert "n=0" in refused(None, 0, None, 1, 1.0, None, None, None, None)
    assert "n=-3" in refused(None, -3, None, 1, 1.0, None, None, None, None)
    msg = refused(None, 10, None, 1, float("nan"), None, None, None, None)
    assert "max_norm=" in msg and "nan" in msg.lower()
    assert "n_spans=0" in refused(None, 10, None, 0, 1.0, None, None, None, None)
    assert "n_spans=9" in refused(None, 10, ends(1, 2, 3, 4, 5, 6, 7, 8, 10), 9, 1.0, None, None, None, None)
    assert "n_spans=2" in refused(None, 10, None, 2, 1.0, None, None, None, None)                       # NULL ends mean ONE span
    msg = refused(None, 10, ends(5, 5, 10), 3, 1.0, None, None, None, None)
    assert "span_ends[1]=5" in msg and "ascend" in msg
    assert "span_ends[0]=0" in refused(None, 10, ends(0, 10), 2, 1.0, None, None, None, None)           # an empty first span
    msg = refused(None, 10, ends(3, 7), 2, 1.0, None, None, None, None)
    assert "7" in msg and "n=10" in msg
    assert "null pointer" in refused(None, 10, ends(3, 10), 2, 1.0, None, None, None, None)             # everything else in order
    assert "null pointer" in refused(None, 10, None, 1, 0.0, None, None, None, None)                    # (max_norm <= 0 is allowed)
    assert lib.dic_adamw_step_clipped(None, None, None, None, 10, 1, 1e-3, 0.9, 0.999, 1e-8, 0.01, None, None, None) != 0
    assert "grad_scale" in _last_error(lib)
    scale = ctypes.c_float(1.0)                       # a grad_scale, and nothing else: dic_adamw_step's own refusal
    assert lib.dic_adamw_step_clipped(None, None, None, None, 10, 1, 1e-3, 0.9, 0.999, 1e-8, 0.01, None, ctypes.byref(scale), None) != 0
    assert "adamw" in _last_error(lib)


def test_clip_grad_norm_option_of_the_mains():
    from depth_image_captioning_pub_amd import base_main, depth_main
    take = depth_main.take_clip_grad_norm
    assert base_main.take_clip_grad_norm is take
    base = ["depth_main", "soft", "cnn", "synthetic"]
    assert take(base) == (base, None)
    assert take(base + ["--clip-grad-norm", "5"]) == (base, 5.0)
    assert take(base[:2] + ["--clip-grad-norm=0.25"] + base[2:]) == (base, 0.25)
    assert take(["base_main", "nic", "--clip-grad-norm", "1e-3"]) == (["base_main", "nic"], 1e-3)
    for bad in (["--clip-grad-norm"], ["--clip-grad-norm", "0"], ["--clip-grad-norm", "-1"], ["--clip-grad-norm=nan"],
                ["--clip-grad-norm", "inf"], ["--clip-grad-norm", "abc"], ["--clip-grad-norm="]):
        with pytest.raises(ValueError, match="--clip-grad-norm"):
            take(base + bad)
        assert depth_main.main(base + bad) == 1 and base_main.main(["base_main", "soft", "synthetic"] + bad) == 1
    # the value travels in the run's config, next to the schedule; without either the loops build their own config
    from depth_image_captioning_pub_amd.Captioning_models.Depth_caption_model import depth_train
    assert depth_main.run_config(depth_train, None, None) is None
    cfg = depth_main.run_config(depth_train, None, 2.5)
    assert cfg.clip_grad_norm == 2.5 and cfg.scheduled_sampling is None
    cfg = depth_main.run_config(depth_train, dict(start=0), None)
    assert cfg.clip_grad_norm is None and cfg.scheduled_sampling == dict(start=0)


def test_configuration_default_is_no_clipping():
    from depth_image_captioning_pub_amd.Captioning_models.config import ConfigTrain
    assert ConfigTrain().clip_grad_norm is None


def test_clipped_optimizer_refuses_bad_norms():
    """scst.ClippedOptimizer is how the module-level steps are clipped (they run backward() and step() inside one function and keep
    their parameter lists)."""
    from depth_image_captioning_pub_amd.Captioning_models import scst
    p = torch.nn.Parameter(torch.ones(4, dtype=torch.float64))
    opt = scst.ClippedOptimizer(torch.optim.SGD([p], lr=1.0), 1e-3)
    assert opt.param_groups[0]["params"][0] is p
    p.grad = torch.full_like(p, 3.0)
    opt.step()
    assert abs(float((1.0 - p.detach()).norm()) - 1e-3) <= 1e-3 * 1e-5
    opt.zero_grad()
    assert p.grad is None
    for bad in (0, -1.0, math.nan, math.inf):
        with pytest.raises(_lib.DicError, match="max_grad_norm"):
            scst.ClippedOptimizer(opt, bad)
