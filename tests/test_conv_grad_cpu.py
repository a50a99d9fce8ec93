"""CPU: what tests/test_conv_grad_gpu.py relies on, checked without a device - the fp64 restatements of tests/conv_grad_common.py
against torch's own fp64 autograd, the plane helpers against nn_kernels_common's, the launch plan every case is meant to reach
(dic_debug_bf3_plan makes no HIP call), every mutant against its case's bound, and the refusals of the new dic_debug_* entry points
(they return before the first launch, so they need the library but no GPU).  Prints the table of e32, e_fmt and the bound per case."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import conv_grad_common as cg
from tests import nn_kernels_common as nk
from tests import operators_common as oc

F64 = torch.float64
EXACT = 1e-12
MUTANT_MARGIN = 20.0          # every mutant lies at least this many bounds from the reference


def _plan(lib, query):
    name = C.create_string_buffer(512)
    out = (C.c_int * 6)()
    rc = lib.dic_debug_bf3_plan(*query, name, len(name), out)
    assert rc == 0, (query, rc, lib.dic_last_error())
    return name.value.decode(), out[0], out[2], out[3]


def _assert_plan(lib, query, want, cid):
    name, grid, fix, fix_n = _plan(lib, query)
    assert name.startswith(want[0]) and (grid, fix, fix_n) == tuple(want[1:]), (cid, name, grid, fix, fix_n, want)


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in cg.WCASES])
def test_wgrad_restatement_plan_bounds_and_mutants(lib, cid):
    c, inp = cg.WCASE[cid], cg.wgrad_inputs(cid)
    OH, OW, M, K = cg.w_geom(c)
    for fmt in (0, 1):
        _assert_plan(lib, cg.wgrad_plan_query(c, fmt), cg.wgrad_expected_plan(c, fmt), cid)
    for gscale in (1.0,) + c.scales:
        ref, b, s_dy = cg.wgrad_bounds(cid, gscale)
        if gscale == 1.0:
            assert oc.scaled_err(cg.wgrad_autograd(c, inp["x"], inp["dy"], F64), ref) <= EXACT
        assert nk.is_pow2(s_dy) and 2.0 ** 13 <= float(inp["dy"].abs().max()) * gscale * s_dy < 2.0 ** 14
        print(f"[conv_grad-table] wgrad {cid} g={gscale:g} M={M} K={K} CO={c.CO} {c.reach}: e32 {b[0].e32:.2e}  e_fmt {b[1].e_fmt:.2e}  "
              f"bound bf16x3 {b[0].bound:.2e}  f16x2 {b[1].bound:.2e}")
        assert b[1].e_fmt <= 4.0 * 2.0 ** -22, "the f16x2 format itself must stay at its 2^-22 representation error"
        if gscale != 1.0:
            continue
        x, dy = inp["x"], inp["dy"]
        for m in cg.WGRAD_MUTANTS:
            if m == "kh_kw_transposed" and not (c.k > 1 and c.H != c.W):
                continue
            if m == "last_slab_dropped" and M <= 32:
                continue
            if m == "k_slice_dropped" and M < 64:
                continue
            ratio = oc.scaled_err(cg.wgrad_ref(c, x, dy, mutant=m), ref) / b[1].bound
            print(f"[conv_grad-mutant] wgrad {cid} {m}: {ratio:.1e} bounds")
            assert ratio >= MUTANT_MARGIN, (cid, m, ratio)


def test_wgrad_cases_cover_both_sides_of_every_term_of_the_route_choice():
    by = {c.id: c for c in cg.WCASES}
    t22 = lambda c: cg.ceil_div(c.CO, 128) * cg.ceil_div(cg.w_geom(c)[3], 128)
    slabs = lambda c: cg.ceil_div(cg.w_geom(c)[2], 32)
    assert (t22(by["G4"]), t22(by["G5"])) == (31, 32) and (by["G4"].reach, by["G5"].reach) == ("tile", "persist")
    assert cg.w_geom(by["G6"])[3] % 128 == 32 and by["G6"].reach == "tile" and t22(by["G6"]) == 36
    assert (slabs(by["G7"]), slabs(by["G8"])) == (63, 64) and (by["G7"].reach, by["G8"].reach) == ("tile", "persist")
    assert (t22(by["G15"]), t22(by["G9"]), t22(by["G10"])) == (128, 255, 256)
    assert (by["G15"].reach, by["G9"].reach, by["G10"].reach) == ("persist", "plain", "tile")
    Ms = [cg.w_geom(c)[2] for c in cg.WCASES]
    assert any(m < 32 for m in Ms) and any(m % 2 and m % 32 for m in Ms)
    assert any(c.stride == 2 and c.pad == 1 for c in cg.WCASES) and any(c.k == 3 and c.H != c.W for c in cg.WCASES)
    assert any(c.C == c.CO == 32 for c in cg.WCASES)
    # the encoder's geometries at the smallest batch the persistent route takes: one image less is the tile route
    for big, small in (("G11", "G12"), ("G13", "G14")):
        assert by[big]._replace(id="", B=0, reach="", scales=(), why="") == by[small]._replace(id="", B=0, reach="", scales=(), why="")
        assert by[big].B == by[small].B + 1 and cg.wgrad_persist_shape(by[big]) and not cg.wgrad_persist_shape(by[small])
    assert (by["G12"].splitk, by["G14"].splitk) == (5, 3)


# ---- data gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in cg.DCASES])
def test_dgrad_restatement_plan_bounds_and_mutants(lib, cid):
    c, inp = cg.DCASE[cid], cg.dgrad_inputs(cid)
    for fmt in (0, 1):
        _assert_plan(lib, cg.dgrad_plan_query(c, fmt), cg.dgrad_expected_plan(c, fmt), cid)
    ref, b, s_dy, s_w = cg.dgrad_bounds(cid)
    assert oc.scaled_err(cg.dgrad_autograd(c, inp["dy"], inp["w"], F64), ref) <= EXACT
    print(f"[conv_grad-table] dgrad {cid} {c.reach}: e32 {b[0].e32:.2e}  e_fmt {b[1].e_fmt:.2e}  bound bf16x3 {b[0].bound:.2e}  f16x2 {b[1].bound:.2e}")
    assert b[1].e_fmt <= 4.0 * 2.0 ** -22
    for m in cg.DGRAD_MUTANTS:
        if c.k == 1 or (m == "pad_not_converted" and c.k - 1 - c.pad == c.pad) or (m == "kh_kw_transposed" and c.H == c.W):
            continue
        ratio = oc.scaled_err(cg.dgrad_ref(c, inp["dy"], inp["w"], mutant=m), ref) / b[1].bound
        print(f"[conv_grad-mutant] dgrad {cid} {m}: {ratio:.1e} bounds")
        assert ratio >= MUTANT_MARGIN, (cid, m, ratio)


def test_dgrad_cases_cover_what_the_issue_lists():
    by = cg.DCASE
    assert by["D1"].k == 1 and (by["D2"].k, by["D2"].pad) == (3, 0) and (by["D3"].k, by["D3"].pad) == (3, 1)
    assert cg.d_geom(by["D4"])[:2] == (3, 5) and by["D2"].H != by["D2"].W
    assert {c.reach for c in cg.DCASES} == {"tile", "tail", "persist"}
    for m in cg.DGRAD_MUTANTS:              # every mutant applies to some case
        assert any(c.k > 1 and not (m == "pad_not_converted" and c.k - 1 - c.pad == c.pad) and not (m == "kh_kw_transposed" and c.H == c.W)
                   for c in cg.DCASES), m


# ---- plane helpers ------------------------------------------------------------------------------------------------------------------
def test_plane_helpers_equal_nn_kernels_commons_bit_for_bit():
    x = torch.randn(37, 64, generator=cg.gen(1)) * torch.exp(torch.randn(37, 64, generator=cg.gen(2)) * 3.0)
    for s in (4.0, 2.0 ** -3, 2.0 ** 9):
        x = x.clamp(-16000.0 / s, 16000.0 / s)
        h1, h2 = cg.split_f16x2(x, s)
        n1, n2 = nk.split2_f16(x.numpy(), s)
        assert np.array_equal(nk.f16_bits(h1.numpy().astype(np.float16)), nk.f16_bits(n1))
        assert np.array_equal(nk.f16_bits(h2.numpy().astype(np.float16)), nk.f16_bits(n2))
        p = cg.planes_of(x, 1, s)
        assert np.array_equal(p[0], nk.f16_bits(n1)) and np.array_equal(p[1], nk.f16_bits(n2))
    hi, mid, lo = cg.planes_of(x, 0)
    assert np.array_equal((nk.bf16_to_f32(hi) + nk.bf16_to_f32(mid)) + nk.bf16_to_f32(lo), x.numpy())
    flat = cg.paired(hi, 37, 64)
    assert flat.size == nk.plane_elems(37, 64) and np.array_equal(nk.from_paired(flat, 37, 64), hi)
    assert not nk.pad_row_of(flat, 37, 64).any()
    for v, s in ((1.0, 2.0 ** 13), (1.999, 2.0 ** 13), (2.0, 2.0 ** 12), (1.0e-6, 2.0 ** 33), (3.0e4, 2.0 ** -1)):
        assert cg.f16_scale_of(v) == s


def test_prepare_restatement_is_the_four_one_line_definitions():
    w2, w3 = cg.prepare_inputs()
    r = cg.prepare_ref(w2, w3)
    assert {k: tuple(v.shape) for k, v in r.items()} == cg.PREP_SHAPES
    for o, i, kh, kw in ((0, 0, 0, 0), (511, 127, 2, 1), (17, 99, 1, 2), (300, 5, 0, 2)):
        assert r["w2"][o, (kh * 3 + kw) * 128 + i] == w2[o, i, kh, kw]
        assert r["w2f"][i, ((2 - kh) * 3 + (2 - kw)) * 512 + o] == w2[o, i, kh, kw]
    assert torch.equal(r["w3"], w3) and torch.equal(r["w3f"], w3.t())
    # the flipped sets are the data gradient's operand: flip_weights of the OHWI weights
    c2 = cg.DCase("", 1, 24, 24, 128, 512, 3, 0, "", "")
    assert torch.equal(r["w2f"], cg.flip_weights(c2, r["w2"]))


# ---- layer 1 ------------------------------------------------------------------------------------------------------------------------
def _l1_autograd(inp):
    """torch's fp64 autograd of conv -> BatchNorm (the given statistics ARE the batch statistics) -> the replayed ReLU / max-pool selection"""
    depth = inp["depth"].double()[:, None]
    w = inp["w"].double().view(128, 1, 7, 7).clone().requires_grad_(True)
    b = inp["b"].double().clone().requires_grad_(True)
    gamma = inp["gamma"].double().clone().requires_grad_(True)
    beta = torch.zeros(128, dtype=F64, requires_grad=True)
    x1 = torch.nn.functional.conv2d(depth, w, b, stride=3).permute(0, 2, 3, 1)
    mu, var = x1.mean(dim=(0, 1, 2)), x1.var(dim=(0, 1, 2), unbiased=False)
    y = (x1 - mu) / torch.sqrt(var + nk.EPS) * gamma + beta
    sel = cg.gather_idx(y, inp["idx"]) * cg.relu_mask(inp).double()
    gw, gb, gg, gbeta = torch.autograd.grad(sel, (w, b, gamma, beta), inp["dpool"].double())
    return dict(dW=gw.reshape(128, 49), db=gb, dgamma=gg, dbeta=gbeta)


@pytest.mark.parametrize("cid", [c.id for c in cg.L1CASES if c.packed])
def test_layer1_dense_chain_bounds_and_mutants(cid):
    c, inp = cg.L1CASE[cid], cg.l1_inputs(cid)
    ref, b = cg.l1_bounds(cid)
    auto = _l1_autograd(inp)
    # the buffer's mean / invstd are the batch statistics rounded to fp32: autograd of the exact ones agrees to that rounding, and the
    # conv bias gradient in front of a train-mode BatchNorm is zero up to fp64 rounding
    for k in ("dW", "dgamma", "dbeta"):
        assert oc.scaled_err(auto[k], ref[k]) <= 3e-6, (cid, k)
    assert float(auto["db"].abs().max()) <= 1e-9 * float(inp["dpool"].abs().sum()) and not ref["db"].any()
    print(f"[conv_grad-table] layer1 {cid} {c.B}x{c.H}x{c.W}: " + "  ".join(f"{k} e32 {b[k].e32:.2e} bound {b[k].bound:.2e}" for k in b))
    OH, OW, PH, PW = cg.l1_geom(c)
    for m in cg.L1_MUTANTS:
        if m == "dropped_rows_not_in_G" and OH % 3 == 0 and OW % 3 == 0:
            continue
        ratio = oc.scaled_err(cg.l1_dense(inp, mutant=m)["dW"], ref["dW"]) / b["dW"].bound
        print(f"[conv_grad-mutant] layer1 {cid} {m}: {ratio:.1e} bounds")
        assert ratio >= MUTANT_MARGIN, (cid, m, ratio)


@pytest.mark.parametrize("cid", [c.id for c in cg.L1CASES if c.packed])
def test_layer1_exact_statistics_make_the_chain_torchs_autograd(cid):
    """with mean / invstd kept in fp64 the dense chain IS autograd of the forward, to fp64 rounding - on every case"""
    inp = dict(cg.l1_inputs(cid))
    x1 = cg.conv1_ref(inp["depth"], inp["w"], inp["b"])
    inp["mean"] = x1.mean(dim=(0, 1, 2))
    inp["invstd"] = 1.0 / torch.sqrt(x1.var(dim=(0, 1, 2), unbiased=False) + nk.EPS)
    ref, auto = cg.l1_dense(inp), _l1_autograd(inp)
    for k in ("dW", "dgamma", "dbeta"):
        assert oc.scaled_err(auto[k], ref[k]) <= EXACT, (cid, k)


def test_layer1_cases_cover_what_the_issue_lists():
    by = cg.L1CASE
    assert [by[i].W for i in ("P1", "P2", "P3", "P4", "P5", "P10")] == [256, 257, 512, 513, 640, 641] and not by["P10"].packed
    assert all(13 <= by[i].H <= 25 for i in ("P1", "P2", "P3", "P4", "P5", "P10"))
    geo = {c.id: cg.l1_geom(c) for c in cg.L1CASES}
    assert {g[1] % 4 for g in geo.values()} == {0, 1, 2, 3}
    assert geo["P6"][:2] == (3, 3) and any(g[0] % 3 for g in geo.values()) and any(g[1] % 3 for g in geo.values())
    assert any(c.H > c.W for c in cg.L1CASES) and any(c.W > c.H for c in cg.L1CASES)
    rows = [c.B * geo[c.id][0] for c in cg.L1CASES]
    assert min(rows) < 512 < max(rows)
    inp = cg.l1_inputs("P6")
    assert float(inp["b"].abs().min()) > 0 and float((inp["b"] - inp["mean"]).abs().min()) > 0
    m = cg.relu_mask(inp).float().mean()
    assert 0.2 < m < 0.8, "both ReLU decisions must occur"


@pytest.mark.parametrize("cid", [c.id for c in cg.L1CASES])
def test_conv1_restatement_equals_autograd(cid):
    inp = cg.l1_inputs(cid)
    ref, b = cg.conv1_bounds(cid)
    y, gw, gb = cg.conv1_autograd(inp, F64)
    assert oc.scaled_err(y, ref["y"]) <= EXACT and oc.scaled_err(gw, ref["dW"]) <= EXACT and oc.scaled_err(gb, ref["db"]) <= EXACT
    print(f"[conv_grad-table] conv1 {cid}: " + "  ".join(f"{k} e32 {b[k].e32:.2e} bound {b[k].bound:.2e}" for k in b))


# ---- refusals: every one before the first launch (no device here) ------------------------------------------------------------------
def _refused(lib, rc, text):
    msg = lib.dic_last_error().decode()
    assert rc < 0 and text in msg, (rc, msg, text)


def test_new_entry_points_refuse_bad_arguments_before_any_launch(lib):
    one = torch.zeros(16)                                       # a host pointer that is never dereferenced
    P = C.c_void_p(one.data_ptr())
    tri = (C.c_void_p * 3)(P, P, P)
    two = (C.c_void_p * 3)(P, P, None)
    hole = (C.c_void_p * 3)(P, None, P)
    sizes = (C.c_size_t * 3)()
    geo = (2, 7, 10, 64, 96, 3, 1, 1)
    assert lib.dic_debug_conv_wgrad_sizes(*geo, 4, C.byref(sizes, 0), C.byref(sizes, 8), C.byref(sizes, 16)) == 0
    dyT, pT, ws = sizes[0], sizes[1], sizes[2]
    assert (dyT, pT, ws) == (96 * 160, 576 * 160, 2 * 9 * 4 * 4096)
    wg = lambda **k: lib.dic_debug_conv_wgrad(*[k.get(n, d) for n, d in (
        ("x", P), ("B", 2), ("H", 7), ("W", 10), ("C", 64), ("CO", 96), ("k", 3), ("stride", 1), ("pad", 1), ("dy", P), ("dw", P), ("splitk", 4),
        ("dyT", tri), ("dyT_elems", dyT), ("pT", tri), ("pT_elems", pT), ("ws", P), ("ws_floats", ws), ("fmt", 0), ("slot", None), ("stream", None))])
    who = "dic_debug_conv_wgrad"
    _refused(lib, wg(x=None), who + ": x / dy")
    _refused(lib, wg(dw=None), who + ": x / dy")
    _refused(lib, wg(C=48), "C=48 and CO=96 % 32")
    _refused(lib, wg(CO=100), "CO=100 % 32")
    _refused(lib, wg(splitk=0), "splitk=0")
    _refused(lib, wg(splitk=17), "splitk=17")
    _refused(lib, wg(stride=0), "stride=0")
    _refused(lib, wg(pad=3), "pad=3")
    _refused(lib, wg(H=1, pad=0), "does not fit")
    _refused(lib, wg(dyT=hole), "dyT: a plane pointer is NULL")
    _refused(lib, wg(pT=two), "pT: a plane pointer is NULL")
    _refused(lib, wg(fmt=1, dyT=two, pT=two), "scale slot")
    _refused(lib, wg(fmt=2), "fmt=2")
    _refused(lib, wg(dyT_elems=dyT - 1), f"dyT planes hold {dyT - 1} elements, {dyT} needed")
    _refused(lib, wg(pT_elems=pT - 1), f"pT planes hold {pT - 1} elements, {pT} needed")
    _refused(lib, wg(ws_floats=ws - 1), f"ws holds {ws - 1} floats, {ws} needed")
    _refused(lib, lib.dic_debug_conv_wgrad_sizes(*geo, 4, None, C.byref(sizes, 8), C.byref(sizes, 16)), "output pointer")
    # the persistent shapes need room for their K slices whatever splitk says
    assert lib.dic_debug_conv_wgrad_sizes(5, 24, 24, 128, 512, 3, 1, 0, 1, C.byref(sizes, 0), C.byref(sizes, 8), C.byref(sizes, 16)) == 0
    assert sizes[2] == 4 * 256 * 4096

    dg = lambda **k: lib.dic_debug_conv_dgrad_s1(*[k.get(n, d) for n, d in (
        ("dy", tri), ("B", 2), ("H", 9), ("W", 12), ("C", 32), ("CO", 64), ("k", 3), ("pad", 0), ("wf", tri), ("dx", P), ("tail", P), ("slabs", 1024),
        ("fmt", 0), ("a0", None), ("a1", None), ("stream", None))])
    who = "dic_debug_conv_dgrad_s1"
    _refused(lib, dg(dy=None), "dy_planes: a plane pointer is NULL")
    _refused(lib, dg(wf=two), "wflip_planes: a plane pointer is NULL")
    _refused(lib, dg(dx=None), who + ": dx is NULL")
    _refused(lib, dg(C=40), "C=40 and CO=64 % 32")
    _refused(lib, dg(CO=72), "CO=72 % 32")
    _refused(lib, dg(k=7, pad=3, H=20, W=20), "at most 32 taps")
    _refused(lib, dg(tail=None), "go together")
    _refused(lib, dg(slabs=2048), "go together")
    _refused(lib, dg(a0=P), "belong to the f16x2 format")
    _refused(lib, dg(fmt=3), "fmt=3")

    n2, n3 = 512 * 1152, 2048 * 512
    pw = lambda **k: lib.dic_debug_depth_prepare_weights(*[k.get(n, d) for n, d in (
        ("w2", P), ("w3", P), ("a", tri), ("b", tri), ("c", tri), ("d", tri), ("n2", n2), ("n3", n3), ("slots", None), ("stream", None))])
    _refused(lib, pw(w3=None), "w2 / w3 is NULL")
    for key, what in (("a", "w2_pl"), ("b", "w2f_pl"), ("c", "w3_pl"), ("d", "w3f_pl")):
        _refused(lib, pw(**{key: two}), what + ": a plane pointer is NULL")
        _refused(lib, pw(**{key: hole, "slots": P}), what + ": a plane pointer is NULL")
    _refused(lib, pw(n2=n2 - 1), "planes hold")
    _refused(lib, pw(n3=n3 - 1), "planes hold")

    wf = lambda **k: lib.dic_debug_conv_wgrad_f32(*[k.get(n, d) for n, d in (
        ("x", P), ("B", 1), ("H", 19), ("W", 641), ("C", 1), ("nchw", 1), ("CO", 128), ("k", 7), ("stride", 3), ("pad", 0), ("dy", P), ("dw", P), ("splitk", 8),
        ("ws", P), ("ws_floats", 8 * 128 * 49), ("stream", None))])
    _refused(lib, wf(dy=None), "x / dy / dw_ohwi is NULL")
    _refused(lib, wf(ws=None), "ws holds 0 floats")
    _refused(lib, wf(ws_floats=8 * 128 * 49 - 1), f"{8 * 128 * 49} needed")
    _refused(lib, wf(splitk=0), "splitk=0")
    _refused(lib, wf(nchw=2), "in_nchw=2")
    _refused(lib, wf(H=5), "does not fit")

    need = lib.dic_debug_depth_layer1_sparse_ws_floats(2, 25, 256)
    assert need == 2 * 2 * 28 * 128 + 256 * 4096 + 2 * 4096 + 8 + 6272 + 768 * 6272
    assert lib.dic_debug_depth_layer1_sparse_ws_floats(0, 25, 256) < 0 and lib.dic_debug_depth_layer1_sparse_ws_floats(1, 6, 256) < 0
    bn_need, cs_need = lib.dic_debug_bn_backward_ws_floats(128), 64 * 6272
    names = ("depth", "B", "H", "W", "dpool", "idx", "xsel", "w", "b", "gamma", "scale", "shift", "mean", "invstd", "dgamma", "dbeta", "dW", "db",
             "bn_ws", "bn_n", "ws", "ws_n", "cs", "cs_n", "stream")
    dflt = dict.fromkeys(names, P)
    dflt.update(B=2, H=25, W=256, bn_n=bn_need, ws_n=need, cs_n=cs_need, stream=None)
    l1 = lambda **k: lib.dic_debug_depth_layer1_bwd_sparse(*[k.get(n, dflt[n]) for n in names])
    who = "dic_debug_depth_layer1_bwd_sparse"
    for n in names:
        if dflt[n] is P:
            rc = l1(**{n: None})
            assert rc < 0 and who in lib.dic_last_error().decode() and "NULL" in lib.dic_last_error().decode(), n
    _refused(lib, l1(B=0), "B=0")
    _refused(lib, l1(bn_n=bn_need - 1), f"bn_ws holds {bn_need - 1} floats")
    _refused(lib, l1(ws_n=need - 1), f"ws holds {need - 1} floats, {need} needed")
    _refused(lib, l1(cs_n=cs_need - 1), f"cs_ws holds {cs_need - 1} floats")
    assert l1(W=641) == 1 and l1(H=13, W=12) == 1 and l1(H=12, W=13) == 1          # not this route's shape: nothing launched

    rows = C.c_int(0)
    f1 = lambda **k: lib.dic_debug_conv1_fwd_checked(*[k.get(n, d) for n, d in (
        ("x", P), ("B", 2), ("H", 25), ("W", 256), ("w", P), ("bias", P), ("y", P), ("partial", P), ("n", 14 * 256), ("rows", C.byref(rows)), ("stream", None))])
    _refused(lib, f1(x=None), "x / w / bias / y is NULL")
    _refused(lib, f1(bias=None), "x / w / bias / y is NULL")
    _refused(lib, f1(H=6), "H=6")
    _refused(lib, f1(n=14 * 256 - 1), f"partial holds {14 * 256 - 1} floats, {14 * 256} needed")
    assert f1(W=641) == 1
    g1 = lambda **k: lib.dic_debug_conv1_wgrad_checked(*[k.get(n, d) for n, d in (
        ("x", P), ("B", 2), ("H", 25), ("W", 256), ("dy", P), ("dw", P), ("dbias", None), ("ws", P), ("ws_n", 14 * 6400), ("cs", P), ("cs_n", cs_need),
        ("stream", None))])
    _refused(lib, g1(dw=None), "x / dy / dw / ws / cs_ws is NULL")
    _refused(lib, g1(cs=None), "x / dy / dw / ws / cs_ws is NULL")
    _refused(lib, g1(ws_n=14 * 6400 - 1), f"ws holds {14 * 6400 - 1} floats, {14 * 6400} needed")
    _refused(lib, g1(cs_n=cs_need - 1), "cs_ws holds")
    _refused(lib, g1(W=3), "W=3")
    assert g1(W=641) == 1
