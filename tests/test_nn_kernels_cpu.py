"""CPU: the restatements of tests/nn_kernels_common.py against torch's own operators in fp64, the properties the GPU file relies on
(no near-tie and no near-kink value in the reference inputs, the fma element, the plane formats), the mutants against the bounds of
their cases, and the argument refusals of the dic_debug_* entry points of the BatchNorm / pooling kernels (taken on the host before
the first HIP call: no GPU).

Mutants: each is the fp64 reference wrong in one term; `ratio` = its deviation in units of the named case's bound
(operators_common.bound; selections: shortfall in units of the replay rule's 4 ulps), as this file prints them:

  mutant                                  case                               ratio
  unbiased variance in the normalisation  finalize (33, 40), invstd          5.0e+02
  biased variance in the running stats    finalize (33, 40), running_var     2.4e+02
  momentum swapped                        finalize (1, 32, 5), running_mean  3.5e+06
  last partial row dropped                finalize (33, 40), mean            5.9e+04
  second slice dropped                    finalize (1025, 64), mean          5.2e+05
  count taken as mtiles * 64              finalize (33, 40), mean            7.0e+03
  ReLU before the residual add            apply 5 x 32, fp32 residual        7.8e+05
  residual BatchNorm shift dropped        apply 5 x 32, raw residual         1.1e+06
  padding counted as 0 with relu off      pool (2, 9, 11, 4, 3, 2, 1), y     6.7e+05
  window origin off by one at p = 1       pool (2, 9, 11, 4, 3, 2, 1), y     1.7e+06
  index transposed (kw * k + kh)          pool (2, 9, 11, 4, 3, 2, 1), idx   2.8e+06
  average divisor taken as k^2            adaptive (20, 20, 7)               1.5e+06
  window end floored                      adaptive (20, 20, 7)               1.7e+06
  dx without the k2 term                  bn_backward 63 x 64, dx            1.2e+05
  k3 without invstd                       bn_backward 63 x 64, dx            1.3e+05
  dgamma without the mean                 bn_backward 63 x 64, dgamma        6.3e+06
  last row chunk dropped                  bn_backward 63 x 64, dbeta         2.8e+05
  pooled gradient to every tied maximum   pool backward (1, 10, 7, 3)        1.6e+06
  mask taken as >= 0                      pool backward (1, 10, 7, 3)        2.4e+05

The finalize is compared per kind of channel (plain / constant / mean 1e3), so the figures of its mutants are those of the plain
channels; pooled over all channels the constant channel's invstd of 316 would have hidden the first one at the larger cases.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from depth_image_captioning_pub_amd import _lib
from tests import nn_kernels_common as nk
from tests import operators_common as oc

F64, F32 = torch.float64, torch.float32


def _close(a, b, tol=1e-12):
    assert oc.scaled_err(a, b) <= tol, oc.scaled_err(a, b)


# ---- restatements against torch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,C", [(5, 32), (2105, 40), (70, 64)])
def test_batchnorm_train_restatement_is_torch_batch_norm(count, C):
    g = nk.gen(count)
    y = torch.randn(count, C, generator=g, dtype=F64) * 1.7 + 0.4
    gamma, beta = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64)
    rm, rv = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    r = nk.bn_train_ref(nk.make_partials(y, F64), count, gamma, beta, rm, rv)
    trm, trv = rm.clone(), rv.clone()
    want = F.batch_norm(y.t().reshape(1, C, count), trm, trv, gamma, beta, True, nk.MOMENTUM, nk.EPS)[0].t()
    _close(y * r["scale"] + r["shift"], want)
    _close(r["running_mean"], trm)
    _close(r["running_var"], trv)
    _close(r["mean"], y.mean(0))
    _close(r["invstd"], 1.0 / torch.sqrt(y.var(0, unbiased=False) + nk.EPS))


def test_batchnorm_eval_restatement_is_torch_batch_norm():
    g = nk.gen(3)
    C = 40
    y = torch.randn(9, C, generator=g, dtype=F64)
    gamma, beta = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64)
    rm, rv = torch.randn(C, generator=g, dtype=F64), torch.rand(C, generator=g, dtype=F64) + 0.5
    r = nk.bn_eval_ref(gamma, beta, rm, rv)
    _close(y * r["scale"] + r["shift"], F.batch_norm(y, rm, rv, gamma, beta, False, nk.MOMENTUM, nk.EPS))


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", nk.POOL_CASES[:3] + [(2, 12, 9, 8, 2, 2, 0), (1, 7, 7, 4, 3, 1, 1)], ids=str)
@pytest.mark.parametrize("relu", [0, 1])
def test_maxpool_restatement_is_torch_max_pool2d_with_indices(case, relu):
    B, H, W, Cc, k, s, p = case
    if Cc > 32:
        Cc = 32
    d = nk.select_inputs((B, H, W, Cc), seed=1)
    y, idx, v = nk.bn_relu_maxpool_ref(d["x"], d["scale"], d["shift"], relu, k, s, p)
    ty, ti = F.max_pool2d(_nchw(v), k, s, p, return_indices=True)
    assert torch.equal(_nchw(y), ty)
    PH, PW = y.shape[1:3]
    h = torch.arange(PH).view(1, PH, 1, 1) * s - p + idx.long() // k
    w = torch.arange(PW).view(1, 1, PW, 1) * s - p + idx.long() % k
    assert torch.equal(_nchw(h * W + w), ti)          # exact ties included: torch keeps the first maximum in scan order too
    sel, ok = nk.gather_selected(v, idx, k, s, p)
    assert bool(ok.all()) and torch.equal(sel, y)


@pytest.mark.parametrize("H,W,O", nk.ADAPTIVE_CASES)
def test_adaptive_avgpool_restatement_is_torch(H, W, O):
    x = torch.randn(2, H, W, 8, generator=nk.gen(H * W + O), dtype=F64)
    _close(nk.adaptive_avgpool_ref(x, O), F.adaptive_avg_pool2d(_nchw(x), O).permute(0, 2, 3, 1))
    dy = torch.randn(2, O, O, 8, generator=nk.gen(5), dtype=F64)
    xt = _nchw(x).clone().requires_grad_(True)
    F.adaptive_avg_pool2d(xt, O).backward(_nchw(dy))
    _close(nk.adaptive_avgpool_bwd_ref(dy, H, W), xt.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("rows,C", [(1, 64), (63, 64), (300, 128)])
def test_batchnorm_backward_closed_form_is_autograd_of_the_forward(rows, C):
    g = nk.gen(rows)
    x = (torch.randn(rows, C, generator=g, dtype=F64) * 1.5 + 0.3).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(rows, C, generator=g, dtype=F64)
    if rows == 1:      # (torch refuses a one-value batch: the same expression written out)
        y = (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + nk.EPS) * gamma + beta
    else:
        y = F.batch_norm(x.t().reshape(1, C, rows), None, None, gamma, beta, True, nk.MOMENTUM, nk.EPS)[0].t()
    y.backward(dy)
    xd = x.detach()
    r = nk.bn_backward_ref(dy, xd, gamma.detach(), xd.mean(0), 1.0 / torch.sqrt(xd.var(0, unbiased=False) + nk.EPS))
    _close(r["dx"], x.grad, 1e-10)
    _close(r["dgamma"], gamma.grad, 1e-10)
    _close(r["dbeta"], beta.grad, 1e-10)


@pytest.mark.parametrize("B,H,W,k", nk.POOL_BWD_CASES[:1] + nk.POOL_BWD_CASES[2:] + [(2, 13, 11, 3)])
def test_pool_backward_restatement_is_autograd(B, H, W, k):
    """continuous random inputs: no ties, so autograd's selection is the restatement's"""
    g = nk.gen(B * H + k)
    x = torch.randn(B, H, W, 8, generator=g, dtype=F64).requires_grad_(True)
    scale, shift = torch.rand(8, generator=g, dtype=F64) + 0.5, torch.randn(8, generator=g, dtype=F64) * 0.3
    _, idx, _ = nk.bn_relu_maxpool_ref(x.detach(), scale, shift, 1, k, k, 0)
    dpool = torch.randn(B, H // k, W // k, 8, generator=g, dtype=F64)
    v = (x * scale + shift).requires_grad_(True)
    v.retain_grad()
    F.max_pool2d(_nchw(torch.relu(v)), k, k).backward(_nchw(dpool))
    _close(nk.maxpool_relu_bwd_ref(dpool, idx, x.detach(), scale, shift, k), v.grad)


# ---- properties of the inputs and formats --------------------------------------------------------------------------------------
def test_fma_element_passes_fused_and_exact_but_not_in_two_roundings():
    x, s, t = np.float32(nk.FMA_X), np.float32(nk.FMA_S), np.float32(nk.FMA_T)
    assert float(x) == nk.FMA_X and float(s) == nk.FMA_S and float(t) == nk.FMA_T          # fp32 numbers
    assert np.float32(x * s) + t == 0.0
    assert float(x) * float(s) + float(t) == nk.FMA_V > 0.0                               # exact in fp64: what an fma rounds


def test_plane_formats():
    x = (torch.randn(5000, generator=nk.gen(0)) * torch.exp(torch.rand(5000, generator=nk.gen(1)) * 30 - 20)).numpy()
    hi, mid, lo = nk.split3_bf16(x)
    assert np.array_equal((nk.bf16_to_f32(hi) + nk.bf16_to_f32(mid)) + nk.bf16_to_f32(lo), x)
    assert np.array_equal(nk.bf16_rne_bits(x), torch.from_numpy(x).bfloat16().view(torch.int16).numpy().view(np.uint16))
    for rows, K in ((1, 32), (5, 96), (64, 2048)):
        off = nk.paired_offsets(rows, K)
        assert len(np.unique(off)) == rows * K and off.max() < nk.plane_elems(rows, K)
        assert nk.pad_row_of(np.zeros(nk.plane_elems(rows, K), np.uint16), rows, K).size == (K if rows % 2 else 0)
    assert off[3, 70] == ((1 * 64 + 2) * 64 + 32 + 6)


@pytest.mark.parametrize("case", nk.POOL_CASES, ids=str)
@pytest.mark.parametrize("relu", [0, 1])
def test_pool_inputs_have_no_near_tie_and_no_near_kink_value(case, relu):
    B, H, W, Cc, k, s, p = case
    d = nk.select_inputs((B, H, W, Cc), seed=0, fma_at=nk.pool_fma_at(case))
    _, _, v = nk.bn_relu_maxpool_ref(d["x"], d["scale"], d["shift"], relu, k, s, p)
    gaps = nk.window_gaps(v, k, s, p)
    tol = nk.ARGMAX_ULPS * oc.FP32_ULP * float(v.abs().max())
    near = (gaps > 0) & (gaps <= 16.0 * tol)         # exact ties (gap 0) or maxima clear by 16 x the replay rule, nothing between ...
    if relu and nk.pool_fma_at(case) is not None:           # ... but the constructed fma element, 2^-24 above its window's zeros
        assert bool((gaps[..., nk.pool_fma_at(case)[-1]][near[..., nk.pool_fma_at(case)[-1]]] == nk.FMA_V).all())
        near[..., nk.pool_fma_at(case)[-1]] = False
    assert not bool(near.any())
    raw = (d["x"].double() * d["scale"].double() + d["shift"].double()).abs()
    if nk.pool_fma_at(case) is not None:
        assert float(raw[nk.pool_fma_at(case)]) == nk.FMA_V
        raw[nk.pool_fma_at(case)] = 1.0
    assert float(raw.min()) >= nk.KINK_MARGIN


@pytest.mark.parametrize("B,H,W,k", nk.POOL_BWD_CASES)
def test_backward_inputs_stay_off_the_kink(B, H, W, k):
    d = nk.select_inputs((B, H, W, 64), seed=0, fma_at=(0, 1, 1, 2), zero_at=(0, 0, 0, 5))
    raw = d["x"].double() * d["scale"].double() + d["shift"].double()
    assert float(raw[0, 1, 1, 2]) == nk.FMA_V and float(raw[0, 0, 0, 5]) == 0.0
    raw[0, 1, 1, 2] = raw[0, 0, 0, 5] = 1.0
    assert float(raw.abs().min()) >= nk.KINK_MARGIN
    # the zero element is its window's selection (every other value of the channel is negative), so `>= 0` would pass a gradient there
    _, idx, _ = nk.bn_relu_maxpool_ref(d["x"], d["scale"], d["shift"], 1, k, k, 0)
    assert int(idx[0, 0, 0, 5]) == 0 and int(idx[0, 1 // k, 1 // k, 2]) == (1 % k) * k + 1 % k


# ---- mutants -------------------------------------------------------------------------------------------------------------------
def _report(name, case, ratio):
    print(f"[nn_kernels-mutant] {name} @ {case}: {ratio:.1e} bounds")
    assert ratio > 1.0, (name, case, ratio)


def _finalize_ratio(case, mutant, key, group="plain"):
    d = nk.finalize_inputs(*case)
    args = (d["partial"], d["count"], d["gamma"], d["beta"], d["rm"], d["rv"])
    ref, t32, mut = nk.bn_train_ref(*args), nk.bn_train_ref(*args, dtype=F32), nk.bn_train_ref(*args, mutant=mutant)
    ch = nk.channel_groups(case[1])[group]
    return nk.mutant_ratio(mut[key][ch], ref[key][ch], t32[key][ch])


def test_finalize_mutants_exceed_their_bounds():
    _report("unbiased variance in the normalisation", "finalize (33, 40) invstd", _finalize_ratio(nk.FINALIZE_CASES[1], "unbiased_norm", "invstd"))
    _report("biased variance in the running statistics", "finalize (33, 40) running_var", _finalize_ratio(nk.FINALIZE_CASES[1], "biased_running", "running_var"))
    _report("momentum swapped", "finalize (1, 32, 5) running_mean", _finalize_ratio(nk.FINALIZE_CASES[0], "momentum_swapped", "running_mean"))
    _report("last partial row dropped", "finalize (33, 40) mean", _finalize_ratio(nk.FINALIZE_CASES[1], "drop_last_row", "mean"))
    _report("second slice dropped", "finalize (1025, 64) mean", _finalize_ratio(nk.FINALIZE_CASES[5], "drop_second_slice", "mean"))
    _report("count taken as mtiles * 64", "finalize (33, 40) mean", _finalize_ratio(nk.FINALIZE_CASES[1], "count_mtiles64", "mean"))


def test_apply_mutants_exceed_their_bounds():
    d = nk.apply_inputs(5, 32)
    a = (d["x"], d["scale"], d["shift"], 1, d["res"])
    _report("ReLU before the residual add", "apply 5 x 32, fp32 residual",
            nk.mutant_ratio(nk.bn_apply_ref(*a, mutant="relu_before_add"), nk.bn_apply_ref(*a), nk.bn_apply_ref(*a, dtype=F32)))
    a = a + (d["res_scale"], d["res_shift"])
    _report("residual BatchNorm shift dropped", "apply 5 x 32, raw residual",
            nk.mutant_ratio(nk.bn_apply_ref(*a, mutant="res_shift_dropped"), nk.bn_apply_ref(*a), nk.bn_apply_ref(*a, dtype=F32)))


def test_pool_mutants_exceed_their_bounds():
    case = nk.POOL_CASES[0]
    B, H, W, Cc, k, s, p = case
    d = nk.select_inputs((B, H, W, Cc), seed=0, fma_at=nk.pool_fma_at(case))
    a = (d["x"], d["scale"], d["shift"])
    y, idx, v = nk.bn_relu_maxpool_ref(*a, 0, k, s, p)
    y32 = nk.bn_relu_maxpool_ref(*a, 0, k, s, p, dtype=F32)[0]
    _report("padding counted as 0 with relu off", f"pool {case} y", nk.mutant_ratio(nk.bn_relu_maxpool_ref(*a, 0, k, s, p, mutant="pad_zero")[0], y, y32))
    _report("window origin off by one at p = 1", f"pool {case} y", nk.mutant_ratio(nk.bn_relu_maxpool_ref(*a, 0, k, s, p, mutant="origin_plus_one")[0], y, y32))
    frac, worst, ok = nk.argmax_replay(nk.bn_relu_maxpool_ref(*a, 0, k, s, p, mutant="idx_transposed")[1], idx, y, v, k, s, p)
    assert frac > nk.ARGMAX_EXCUSED
    _report("index transposed (kw * k + kh)", f"pool {case} idx", worst)
    assert nk.argmax_replay(idx, idx, y, v, k, s, p) == (0.0, 0.0, True)


def test_adaptive_mutants_exceed_their_bounds():
    H, W, O = nk.ADAPTIVE_CASES[4]
    x = torch.randn(2, H, W, 8, generator=nk.gen(7))
    ref, t32 = nk.adaptive_avgpool_ref(x, O), nk.adaptive_avgpool_ref(x, O, dtype=F32)
    _report("average divisor taken as k^2", "adaptive (20, 20, 7)", nk.mutant_ratio(nk.adaptive_avgpool_ref(x, O, mutant="divisor_k2"), ref, t32))
    _report("window end floored", "adaptive (20, 20, 7)", nk.mutant_ratio(nk.adaptive_avgpool_ref(x, O, mutant="floor_end"), ref, t32))


def test_backward_mutants_exceed_their_bounds():
    d = nk.select_inputs((63, 64), seed=0)
    g = torch.randn(63, 64, generator=nk.gen(11))
    a = (g, d["x"], d["gamma"], d["mean"], d["invstd"])
    ref, t32 = nk.bn_backward_ref(*a), nk.bn_backward_ref(*a, dtype=F32)
    for name, mutant, key in (("dx without the k2 term", "no_k2", "dx"), ("k3 without invstd", "k3_no_invstd", "dx"),
                              ("dgamma without the mean", "dgamma_no_mean", "dgamma"), ("last row chunk dropped", "drop_last_chunk", "dbeta")):
        _report(name, f"bn_backward 63 x 64 {key}", nk.mutant_ratio(nk.bn_backward_ref(*a, mutant=mutant)[key], ref[key], t32[key]))
    B, H, W, k = nk.POOL_BWD_CASES[2]
    d = nk.select_inputs((B, H, W, 64), seed=0, fma_at=(0, 1, 1, 2), zero_at=(0, 0, 0, 5))
    _, idx, _ = nk.bn_relu_maxpool_ref(d["x"], d["scale"], d["shift"], 1, k, k, 0)
    dpool = torch.randn(B, H // k, W // k, 64, generator=nk.gen(12))
    a = (dpool, idx, d["x"], d["scale"], d["shift"], k)
    ref, t32 = nk.maxpool_relu_bwd_ref(*a), nk.maxpool_relu_bwd_ref(*a, dtype=F32)
    _report("pooled gradient sent to every tied maximum", f"pool backward {nk.POOL_BWD_CASES[2]}", nk.mutant_ratio(nk.maxpool_relu_bwd_ref(*a, mutant="all_ties"), ref, t32))
    _report("mask taken as >= 0", f"pool backward {nk.POOL_BWD_CASES[2]}", nk.mutant_ratio(nk.maxpool_relu_bwd_ref(*a, mutant="mask_ge"), ref, t32))


def test_column_sum_bound_stays_within_factor_16_and_the_running_sum_is_an_order_not_a_term():
    """The two-level running sum (the order nn_kernels.h describes) against torch's pairwise sum, both fp32 on the same operands: the
    figures that set colsum_rows' bound.  A dropped row is far outside either."""
    worst = 0.0
    for rows in nk.COLSUM_ROWS:
        for C_ in nk.COLSUM_C:
            for ld, offset in nk.colsum_layouts(C_):
                _, X = nk.colsum_input(rows, C_, ld, offset)
                ref = nk.colsum_ref(X, C_)
                b, t32 = nk.colsum_bound(X, C_, ref)
                e32, e2 = oc.scaled_err(t32, ref), oc.scaled_err(nk.colsum_two_level_fp32(X, C_), ref)
                print(f"[nn_kernels-colsum] rows={rows} C={C_} ld={ld} offset={offset}: torch fp32 {e32:.2e}  two-level running sum {e2:.2e}  bound {b:.2e}")
                assert oc.bound(t32, ref) <= b <= max(nk.COLSUM_FACTOR_CAP * e32, 4.0 * oc.FP32_ULP)
                worst = max(worst, b / max(e32, oc.FP32_ULP))
                if rows > 1:
                    assert oc.scaled_err(nk.colsum_ref(X[:-1], C_), ref) > 100.0 * b
    print(f"[nn_kernels-colsum] largest bound / torch fp32 error: {worst:.1f}")


# ---- argument refusals (host side, before any HIP call) -------------------------------------------------------------------------
def _refused(lib, rc, *words):
    assert rc < 0, rc
    msg = lib.dic_last_error().decode()
    assert all(w in msg for w in words), (words, msg)


def test_debug_entry_points_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    bn = (p, p, p, p)
    none4 = (None, None, None, None)
    pl3 = (C.c_void_p * 3)(p, p, p)
    pl2 = (C.c_void_p * 3)(p, p, None)
    bad = (C.c_void_p * 3)(p, None, p)
    _refused(lib, lib.dic_debug_bn_finalize(None, 1, 5, 32, p, p, p, p, *bn, None, 0, None, None), "dic_debug_bn_finalize", "NULL")
    _refused(lib, lib.dic_debug_bn_finalize(p, 1, 5, 32, p, p, p, p, p, p, None, p, None, 0, None, None), "BatchNorm buffer")
    _refused(lib, lib.dic_debug_bn_finalize(p, 0, 5, 32, p, p, p, p, *bn, None, 0, None, None), "mtiles=0")
    _refused(lib, lib.dic_debug_bn_finalize(p, 1, 5, 32, p, p, p, None, *bn, None, 0, None, None), "go together")
    _refused(lib, lib.dic_debug_bn_finalize(p, 1025, 65000, 64, p, p, p, p, *bn, p, 100, None, None), "red holds 100 doubles")
    _refused(lib, lib.dic_debug_bn_finalize_eval(32, p, None, p, p, *bn, None), "NULL")
    _refused(lib, lib.dic_debug_bn_apply(p, None, None, p, None, 4, 30, *bn, 1, *none4, None, None), "C=30 % 4")
    _refused(lib, lib.dic_debug_bn_apply(p, None, None, p, pl3, 4, 48, *bn, 1, *none4, None, None), "C=48 % 32")
    _refused(lib, lib.dic_debug_bn_apply(p, None, None, None, None, 4, 32, *bn, 1, *none4, None, None), "no output")
    _refused(lib, lib.dic_debug_bn_apply(None, None, None, p, None, 4, 32, *bn, 1, *none4, None, None), "x is NULL")
    _refused(lib, lib.dic_debug_bn_apply(p, None, None, p, bad, 4, 32, *bn, 1, *none4, None, None), "planes[0] / planes[1]")
    _refused(lib, lib.dic_debug_bn_apply(p, p, pl3, p, pl3, 4, 32, *bn, 1, *none4, None, None), "not both")
    _refused(lib, lib.dic_debug_bn_apply(p, None, pl3, p, pl2, 4, 32, *bn, 1, *none4, None, None), "f16x2")
    _refused(lib, lib.dic_debug_bn_apply(p, None, None, p, pl3, 4, 32, *bn, 1, p, p, p, p, None, None), "residual_bn needs")
    _refused(lib, lib.dic_debug_bn_apply(p, p, None, p, pl3, 4, 32, *bn, 1, p, None, p, p, None, None), "(residual)")
    _refused(lib, lib.dic_debug_bn_apply(p, p, None, p, None, 4, 32, *bn, 1, p, p, p, p, None, None), "needs plane output")
    _refused(lib, lib.dic_debug_bn_relu_maxpool(p, 1, 4, 4, 6, *none4, 1, 3, 2, 1, p, None, None, None, None, None), "C=6 % 4")
    _refused(lib, lib.dic_debug_bn_relu_maxpool(p, 1, 4, 4, 8, *none4, 1, 3, 2, 1, p, None, pl3, None, None, None), "C=8 % 32")
    _refused(lib, lib.dic_debug_bn_relu_maxpool(p, 1, 4, 4, 8, *none4, 1, 3, 2, 1, None, None, None, None, None, None), "no output")
    _refused(lib, lib.dic_debug_bn_relu_maxpool(p, 1, 4, 4, 8, *none4, 1, 3, 2, 2, p, None, None, None, None, None), "p=2")
    _refused(lib, lib.dic_debug_bn_relu_maxpool(p, 1, 2, 4, 8, *none4, 1, 3, 2, 0, p, None, None, None, None, None), "does not fit")
    _refused(lib, lib.dic_debug_bn_relu_maxpool(p, 1, 4, 4, 8, p, None, p, p, 1, 3, 2, 1, p, None, None, None, None, None), "BatchNorm buffer")
    _refused(lib, lib.dic_debug_adaptive_avgpool(p, 1, 7, 7, 6, *none4, 0, 14, p, None), "C=6 % 4")
    _refused(lib, lib.dic_debug_adaptive_avgpool(p, 1, 7, 7, 8, *none4, 0, 14, None, None), "NULL")
    _refused(lib, lib.dic_debug_adaptive_avgpool_bwd(p, 1, 7, 7, 6, 14, p, None), "C=6 % 4")
    _refused(lib, lib.dic_debug_adaptive_avgpool_bwd(None, 1, 7, 7, 8, 14, p, None), "NULL")
    _refused(lib, lib.dic_debug_maxpool_relu_bwd(p, p, p, 1, 4, 4, 6, 2, *bn, p, None), "C=6 % 4")
    _refused(lib, lib.dic_debug_maxpool_relu_bwd(p, None, p, 1, 4, 4, 8, 2, *bn, p, None), "NULL")
    _refused(lib, lib.dic_debug_maxpool_relu_bwd(p, p, p, 1, 4, 4, 8, 2, *none4, p, None), "BatchNorm buffer")
    _refused(lib, lib.dic_debug_relu_mask_bwd(p, p, 4, 6, *bn, None), "C=6 % 4")
    _refused(lib, lib.dic_debug_relu_mask_bwd(None, p, 4, 8, *bn, None), "NULL")
    assert lib.dic_debug_bn_backward_ws_floats(96) < 0 and lib.dic_debug_bn_backward_ws_floats(0) < 0
    ws = lib.dic_debug_bn_backward_ws_floats(64)
    assert ws > 0
    _refused(lib, lib.dic_debug_bn_backward(p, p, 4, 96, p, *bn, p, p, p, 1 << 30, None, None, None, None), "C=96 % 64")
    _refused(lib, lib.dic_debug_bn_backward(p, p, 4, 64, p, *bn, p, p, p, ws - 1, None, None, None, None), f"ws holds {ws - 1} floats")
    _refused(lib, lib.dic_debug_bn_backward(p, p, 4, 64, None, *bn, p, p, p, ws, None, None, None, None), "NULL")
    _refused(lib, lib.dic_debug_bn_backward(p, p, 4, 64, p, *bn, p, p, p, ws, pl2, None, p, None), "f16x2 planes need")
    _refused(lib, lib.dic_debug_bn_pool_backward(p, p, p, 1, 4, 4, 96, 2, p, *bn, p, p, p, 1 << 30, p, None, None, None, None), "C=96 % 64")
    _refused(lib, lib.dic_debug_bn_pool_backward(p, p, p, 1, 4, 4, 192, 2, p, *bn, p, p, p, 1 << 30, p, None, None, None, None), "dividing 256")
    _refused(lib, lib.dic_debug_bn_pool_backward(p, p, p, 1, 4, 4, 64, 2, p, *bn, p, p, p, ws - 1, p, None, None, None, None), "ws holds")
    _refused(lib, lib.dic_debug_bn_pool_backward(p, p, p, 1, 4, 4, 64, 2, p, *bn, p, p, p, ws, None, None, None, None, None), "NULL")
    _refused(lib, lib.dic_debug_bn_pool_backward(p, p, p, 1, 4, 4, 64, 2, p, *bn, p, p, p, ws, p, pl2, p, None, None), "f16x2 planes need")
    _refused(lib, lib.dic_debug_bn_pool_backward(p, p, p, 1, 4, 4, 64, 5, p, *bn, p, p, p, ws, p, None, None, None, None), "does not fit")
    _refused(lib, lib.dic_debug_colsum_rows(p, 2, 4, 3, p, p, 768, None), "ld=2")
    _refused(lib, lib.dic_debug_colsum_rows(p, 3, 4, 3, p, p, 767, None), "ws holds 767 floats")
    _refused(lib, lib.dic_debug_colsum_rows(p, 3, 4, 3, None, p, 768, None), "NULL")
    _refused(lib, lib.dic_debug_f16_scale_reset(p, 65, None), "n=65")
    _refused(lib, lib.dic_debug_f16_scale_reset(None, 1, None), "NULL")
    _refused(lib, lib.dic_debug_f16_scale_from_absmax(p, 6, p, p, None), "n=6 % 4")
    _refused(lib, lib.dic_debug_f16_scale_from_absmax(p, 8, None, p, None), "NULL")
    _refused(lib, lib.dic_debug_f16_scale_finish(p, None, None), "NULL")
