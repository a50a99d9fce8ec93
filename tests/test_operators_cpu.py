"""CPU: the references of tests/operators_common.py against published known answers and against torch's own fp64 operators,
so that the GPU parity tests (tests/test_operators_gpu.py) compare the kernels with something that is itself pinned."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import operators_common as oc


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("counter,key,expected", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, expected):
    """The three Philox4x32-10 vectors of Random123's kat_vectors (zeros, all ones, digits of pi)."""
    got = oc.philox4x32_10(np.array(_words(counter), dtype=np.uint64), np.array(_words(key), dtype=np.uint64))
    assert [int(v) for v in got] == _words(expected)


def test_philox_is_vectorised_over_counters():
    ctr = np.array([_words("00000000 00000000 00000000 00000000"), _words("243f6a88 85a308d3 13198a2e 03707344")], dtype=np.uint64)
    one_by_one = [oc.philox4x32_10(c, np.array([7, 9], dtype=np.uint64)) for c in ctr]
    assert np.array_equal(oc.philox4x32_10(ctr, np.array([7, 9], dtype=np.uint64)), np.stack(one_by_one))


def test_dropout_mask_ref_layout_and_threshold():
    """Element 4q + j is lane j of block q; the counter is q + offset carried into its high word; p = 0 keeps everything."""
    seed, n = oc.DROPOUT_SEED, 23
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    for offset in (0, 1, 2 ** 32 - 2):
        m = oc.dropout_mask_ref(n, 0.5, seed, offset)
        assert m.dtype == np.float32 and m.shape == (n,) and set(np.unique(m).tolist()) <= {0.0, 2.0}
        for i in (0, 3, 4, 9, 22):
            c = (i // 4) + offset
            bits = int(oc.philox4x32_10(np.array([c & 0xFFFFFFFF, c >> 32, 0, 0], dtype=np.uint64), key)[i % 4])
            assert (m[i] != 0) == ((bits >> 8) * 2.0 ** -24 >= 0.5), (offset, i)
    assert np.array_equal(oc.dropout_mask_ref(9, 0.0, seed, 0), np.ones(9, dtype=np.float32))
    m9 = oc.dropout_mask_ref(4099, 0.9, seed, 0)
    assert set(np.unique(m9).tolist()) == {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.9)))}
    assert abs(float((m9 != 0).mean()) - 0.1) < 0.02
    assert np.array_equal(oc.dropout_mask_ref(16, 0.5, seed, 1)[:12], oc.dropout_mask_ref(16, 0.5, seed, 0)[4:])


def test_dropout_reference_draws_on_the_threshold():
    """The two blocks operators_common names hold a draw of exactly 0.5 and of exactly 0; the reference keeps both elements."""
    key = np.array([oc.DROPOUT_SEED & 0xFFFFFFFF, oc.DROPOUT_SEED >> 32], dtype=np.uint64)
    for (block, lane), p, bits in ((oc.DRAW_EQUALS_HALF, 0.5, 1 << 23), (oc.DRAW_EQUALS_ZERO, 0.0, 0)):
        got = oc.philox4x32_10(np.array([block, 0, 0, 0], dtype=np.uint64), key)
        assert int(got[lane]) >> 8 == bits
        mask = oc.dropout_mask_ref(8, p, oc.DROPOUT_SEED, block)
        assert mask[lane] == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    assert oc.dropout_mask_ref(8, 0.9, oc.DROPOUT_SEED, oc.DRAW_EQUALS_HALF[0])[oc.DRAW_EQUALS_HALF[1]] == 0.0


def test_resize_size_and_center_crop_origin():
    """torchvision's rules: the long edge is truncated, the crop origin rounds halves to even."""
    assert oc.resize_size(60, 64, 384) == (384, 409)
    assert oc.center_crop_origin(409, 384) == 12          # 12.5 -> 12 (a round-half-away rule gives 13)
    assert oc.center_crop_origin(384 + 195, 384) == 98    # 97.5 -> 98: halves that round UP to the even neighbour
    assert oc.resize_size(100, 150, 384) == (384, 576) and oc.center_crop_origin(576, 384) == 96
    assert oc.resize_size(301, 200, 384) == (577, 384) and oc.center_crop_origin(577, 384) == 96      # 96.5 -> 96
    assert oc.resize_size(200, 301, 384) == (384, 577)
    assert oc.resize_size(224, 224, 384) == (384, 384) and oc.center_crop_origin(384, 384) == 0


@pytest.mark.parametrize("H,W,s", [(224, 224, 384), (384, 384, 224), (24, 24, 14), (14, 14, 24), (60, 64, 384), (301, 200, 384)])
def test_resize_crop_ref_equals_interpolate_fp64(H, W, s):
    """The explicit gather against F.interpolate in fp64 followed by the crop window, enlarging and shrinking."""
    x = torch.rand(2, H, W, generator=torch.Generator().manual_seed(H + W), dtype=torch.float64)
    RH, RW = oc.resize_size(H, W, s)
    cy, cx = oc.center_crop_origin(RH, s), oc.center_crop_origin(RW, s)
    ref = F.interpolate(x[None], size=(RH, RW), mode="bilinear", align_corners=False)[0][:, cy:cy + s, cx:cx + s]
    got = oc.resize_crop_ref(x, s, s, 2.0, -1.0)
    assert got.shape == (2, s, s)
    assert float((got - (ref * 2.0 - 1.0)).abs().max()) <= 1e-12


@pytest.mark.parametrize("H,W", [(1, 1), (1, 5), (5, 1), (5, 7)])
def test_upsample2x_ref_equals_interpolate_fp64(H, W):
    x = torch.randn(2, H, W, 4, generator=torch.Generator().manual_seed(H * 10 + W), dtype=torch.float64)
    ref = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    assert float((oc.upsample2x_ref(x) - ref).abs().max()) <= 1e-13


def test_depth_standardize_ref():
    d = torch.tensor([[float("nan"), 2.0, -1.0, float("nan")], [0.5, 0.5, 3.0, float("nan")]])
    ref = oc.depth_standardize_ref(d)
    assert torch.equal(ref, torch.tensor([[0.5, 1.0, 0.0, 0.5], [0.0, 0.0, 1.0, 0.0]], dtype=torch.float64))


@pytest.mark.parametrize("with_alphas", [False, True])
def test_caption_loss_ref_equals_autograd_fp64(with_alphas):
    g = torch.Generator().manual_seed(5)
    n, V, B, T, lam = 11, 13, 3, 4, 0.7
    logits = torch.randn(n, V, generator=g, dtype=torch.float64, requires_grad=True)
    targets = torch.randint(0, V, (n,), generator=g)
    alphas = torch.softmax(torch.randn(B, T, oc.L_CELLS, generator=g, dtype=torch.float64), -1).requires_grad_(True) if with_alphas else None
    ce = F.cross_entropy(logits, targets)
    reg = lam * ((1.0 - alphas.sum(dim=1)) ** 2).mean() if with_alphas else None        # depth_train.py:214-216
    (ce * 0.25).backward(retain_graph=True)
    if with_alphas:
        (reg * 0.5).backward()
    loss, dlogits, dalphas, lse = oc.caption_loss_ref(logits.detach(), targets, alphas.detach() if with_alphas else None, lam, 0.25, 0.5)
    assert abs(float(loss) - float((ce + (reg if with_alphas else 0.0)).detach())) <= 1e-13
    assert float((dlogits - logits.grad).abs().max()) <= 1e-15
    assert float((lse - torch.logsumexp(logits.detach(), 1)).abs().max()) == 0.0
    if with_alphas:
        assert float((dalphas - alphas.grad).abs().max()) <= 1e-15
    else:
        assert dalphas is None


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_adamw_ref_equals_torch_optim_fp64(weight_decay):
    g = torch.Generator().manual_seed(6)
    p0 = torch.randn(257, generator=g, dtype=torch.float64)
    grads = [torch.randn(257, generator=g, dtype=torch.float64) * 0.01 for _ in range(3)]
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step, gr in enumerate(grads, start=1):
        q.grad = gr.clone()
        opt.step()
        p, m, v = oc.adamw_ref(p, gr, m, v, step, 1e-3, 0.9, 0.999, 1e-8, weight_decay)
        st = opt.state[q]
        assert float((p - q.detach()).abs().max()) <= 1e-14
        assert float((m - st["exp_avg"]).abs().max()) <= 1e-16 and float((v - st["exp_avg_sq"]).abs().max()) <= 1e-18


def test_norm_refs_equal_torch_fp64():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 35, 24, generator=g, dtype=torch.float64) * 2 + 1
    ga, be = torch.randn(24, generator=g, dtype=torch.float64), torch.randn(24, generator=g, dtype=torch.float64)
    res = torch.randn(2, 35, 24, generator=g, dtype=torch.float64)
    ref = torch.relu(F.group_norm(x.permute(0, 2, 1), 4, ga, be, 1e-5).permute(0, 2, 1) + res)
    assert float((oc.group_norm_ref(x, 4, ga, be, 1e-5, res, True) - ref).abs().max()) <= 1e-13
    rows = x.reshape(70, 24)
    assert float((oc.layer_norm_ref(rows, ga, be, 1e-6) - F.layer_norm(rows, (24,), ga, be, 1e-6)).abs().max()) <= 1e-13
    w = torch.randn(5, 27, generator=g, dtype=torch.float64)
    std, mean = torch.std_mean(w, dim=1, keepdim=True, unbiased=False)                  # timm StdConv2dSame.get_weight
    assert float((oc.weight_standardize_ref(w, 1e-8) - (w - mean) / (std + 1e-8)).abs().max()) <= 1e-13
    assert torch.equal(oc.weight_standardize_ref(torch.full((1, 9), 0.25), 1e-8), torch.zeros(1, 9, dtype=torch.float64))
    v = torch.linspace(-10, 10, 101, dtype=torch.float64)
    assert float((oc.gelu_ref(v) - F.gelu(v)).abs().max()) <= 1e-15


def test_bound_has_a_floor_and_follows_the_fp32_error():
    ref = torch.tensor([1.0, -8.0], dtype=torch.float64)
    assert oc.bound(ref.float(), ref) == 4.0 * oc.FP32_ULP
    assert math.isclose(oc.bound(torch.tensor([1.0, -8.0 + 8e-5]), ref), 4.0 * 1e-5, rel_tol=1e-2)
    assert oc.scaled_err(torch.zeros(3), torch.zeros(3, dtype=torch.float64)) == 0.0
