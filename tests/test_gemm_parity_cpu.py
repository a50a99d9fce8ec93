"""CPU: what tests/test_gemm_parity_gpu.py rests on, without a device - the fp64 references of tests/gemm_common.py against a second
route, the inputs' scale, the emulated summation order of the kernel against half of every bound, the restated tail and split-K rules
against the case tables, the tables' own arithmetic (keys, tile counts, workspace sizes, operand buffers), and the sensitivity of
every bound to ten fp64 mutants."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_common as gc
from tests import linear_common as lc
from tests import operators_common as oc


# ---- 1. references against a second route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["G2", "G3b", "G6c", "G6h", "G10"])
def test_gemm_reference_reads_the_views_as_the_abi_states_them(cid):
    """The reference (F.linear on the strided views) against an element-wise restatement of include/dic.h: element (i, k) of an operand
    is p[i*ld + k], of a K-major one p[k*ld + i], p starting `off` floats into the buffer - and every other float of the buffer is NaN."""
    c, inp = gc.CASE[cid], gc.inputs(cid)
    dense = []
    for buf, R, colk, ld, off in ((inp["a_buf"], c.M, c.a, c.lda, c.a_off), (inp["b_buf"], c.N, c.b, c.ldb, c.b_off)):
        i, k = torch.meshgrid(torch.arange(R), torch.arange(c.K), indexing="ij")
        idx = off + (k * ld + i if colk else i * ld + k)
        dense.append(buf[idx].double())
        assert bool(torch.isfinite(dense[-1]).all())
        rest = torch.ones_like(buf, dtype=torch.bool)
        rest[idx.reshape(-1)] = False
        assert int(rest.sum()) == buf.numel() - R * c.K and bool(torch.isnan(buf[rest]).all())
    z = torch.einsum("mk,nk->mn", dense[0], dense[1])
    assert oc.scaled_err(gc.reference(cid, 0), z) <= 1e-14
    for act, fn in ((0, lambda t: t), (1, F.relu), (2, torch.sigmoid), (3, F.gelu)):
        want = fn(z + inp["bias"].double()) + inp["c_old"].double()
        assert oc.scaled_err(gc.reference(cid, 1, act, 1), want) <= 1e-14, (cid, act)
    want32 = F.gelu(F.linear(dense[0].float(), dense[1].float(), inp["bias"])) + inp["c_old"]
    assert torch.equal(gc.torch_fp32(cid, 1, 3, 1), want32)


@pytest.mark.parametrize("cid", ["V1", "V3", "V4a", "V4b", "V5", "V6", "V7a", "V8a"])
def test_conv_reference_agrees_with_the_explicit_unfold(cid):
    """F.conv2d on NCHW, permuted to NHWC, against the gathered-patch matrix times the OHWI weights; x_dev is the stated storage order."""
    c, inp = gc.CASE[cid], gc.inputs(cid)
    _, _, M, K = gc.conv_dims(c)
    z = gc.patches(c, inp["x"]) @ inp["w"].double().reshape(c.CO, K).t()
    assert z.shape == (M, c.CO)
    assert oc.scaled_err(gc.reference(cid, 0), z) <= 1e-14
    assert oc.scaled_err(gc.reference(cid, 1), z + inp["bias"].double()) <= 1e-14
    assert inp["x_dev"].shape == ((c.B, c.C, c.H, c.W) if c.nchw else (c.B, c.H, c.W, c.C)) and inp["x_dev"].is_contiguous()
    assert torch.equal(inp["x_dev"].permute(0, 2, 3, 1) if c.nchw else inp["x_dev"], inp["x"])
    ref = gc.reference(cid, 1)
    for tile in c.tiles:
        part = gc.tile_partials(ref, tile)
        assert part.shape == (gc.ceil_div(M, tile), 2, c.CO)
        assert torch.allclose(part[:, 0].sum(0), ref.sum(0), rtol=1e-12, atol=1e-12) and torch.allclose(part[:, 1].sum(0), (ref * ref).sum(0), rtol=1e-12)
        assert torch.allclose(part[-1, 0], ref[(part.shape[0] - 1) * tile:].sum(0), rtol=1e-12, atol=1e-12)


# ---- 2. the inputs' scale -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", gc.GEMM_IDS + gc.CONV_IDS)
def test_preactivations_straddle_one(cid):
    """Pre-activations reach beyond +-1 with and without the bias, so that ReLU and GELU outputs keep the scale of their arguments.  G4b
    has one element: it lies above 1 with and without the bias (seed chosen so)."""
    z = gc.reference(cid, 0)
    for pre in (z, z + gc.inputs(cid)["bias"].double()):
        if z.numel() == 1:
            assert float(pre.min()) > 1.0, (cid, float(pre.min()))
        else:
            assert float(pre.min()) < -1.0 and float(pre.max()) > 1.0, (cid, float(pre.min()), float(pre.max()))


# ---- 3. the kernel's summation order stays within every bound ----------------------------------------------------------------------------
def _combos(c):
    return lc.combos(c) if c in gc.GEMM_CASES else [(b, 0, 0) for b in (1, 0)]


@pytest.mark.parametrize("cid", gc.GEMM_IDS + gc.CONV_IDS)
def test_chain_emulation_stays_within_half_the_bound(cid):
    """One fp32 chain of K terms per element (per split-K slice, slices added in order), then the epilogue in fp32, stays within half of
    operators_common.bound(torch fp32, ref) for every combination of every case - V2 and V3, whose K their routes pin at 800 and 1056,
    within three quarters (gemm_common.HALF_EXCEPTIONS) - and no bound exceeds the bar of tests/test_gemm_gpu.py.  The bound is 4 x the
    error of torch's BLAS, which sums up to about a hundred terms as a plain chain and, depending on the build, blocks longer sums from
    K of 200 or of 400 on; the cases are short enough that the assertion holds under both.
    The partial sums have no documented order to emulate; as ONE fp32 chain over the tile's 64 or 128 rows - longer than any chain of a
    kernel that sums per lane and then across lanes, so an upper estimate - they stay within their bounds."""
    c = gc.CASE[cid]
    K = c.K if c in gc.GEMM_CASES else gc.conv_dims(c)[3]
    chain = min(K, gc.eff_splitk(K, getattr(c, "splitk", 1))[1] * gc.BK)          # terms of the longest chain
    worst, largest = (0.0,), 0.0
    for bias, act, acc in _combos(c):
        ref = gc.reference(cid, bias, act, acc)
        b = gc.bound(cid, bias, act, acc, ref)
        e32 = oc.scaled_err(gc.torch_fp32(cid, bias, act, acc), ref)
        e = oc.scaled_err(gc.emulated(cid, bias, act, acc), ref)
        largest = max(largest, b)
        worst = max(worst, (e / b, e, e32, b, bias, lc.ACT_NAMES[act], acc))
        assert 4.0 * oc.FP32_ULP <= b <= gc.BAR, (cid, bias, act, acc, b)
        assert e <= gc.HALF_EXCEPTIONS.get(cid, gc.HALF) * b, (cid, bias, act, acc, e, b, chain)
    ratio, e, e32, b, bias, act, acc = worst
    print(f"[gemm-chain] {cid}: chain {chain}  emulation {e:.2e} = {e / e32 if e32 else math.inf:.2f} x torch fp32 {e32:.2e}, {ratio:.2f} of the bound {b:.2e} at bias {bias} act {act} "
          f"accumulate {acc}; largest bound {largest:.2e}")
    if c in gc.CONV_CASES:
        for bias in (1, 0):
            y = gc.emulated(cid, bias).numpy()
            for tile in c.tiles:
                ref, bs, _ = gc.partial_bounds(cid, bias, tile)
                got = torch.from_numpy(gc.chain_partials(y, tile))
                for k in (0, 1):
                    e = oc.scaled_err(got[:, k], ref[:, k])
                    print(f"[gemm-chain] {cid} bias {bias} tile {tile} partial {k}: emulation {e:.2e}, {e / bs[k]:.2f} of the bound {bs[k]:.2e}")
                    assert e <= bs[k] <= gc.BAR, (cid, bias, tile, k, e, bs[k])


def test_largest_bound_over_all_cases():
    """The largest bound the rule yields over every combination of every case, printed, within the 2e-5 bar of tests/test_gemm_gpu.py."""
    largest = (0.0,)
    for c in gc.GEMM_CASES + gc.CONV_CASES:
        for bias, act, acc in _combos(c):
            largest = max(largest, (gc.bound(c.id, bias, act, acc), c.id, bias, lc.ACT_NAMES[act], acc))
        if c in gc.CONV_CASES:
            for bias in (1, 0):
                for tile in c.tiles:
                    largest = max(largest, (max(gc.partial_bounds(c.id, bias, tile)[1].values()), c.id, bias, f"partials, tile {tile}", 0))
    print(f"[gemm-bounds] largest bound over all cases: {largest[0]:.3e} at {largest[1:]}")
    assert 4.0 * oc.FP32_ULP <= largest[0] <= gc.BAR
    assert set(gc.HALF_EXCEPTIONS) == {"V2", "V3"} and max(gc.HALF_EXCEPTIONS.values()) < 1.0


# ---- 4. the launcher's documented rules against the tables ------------------------------------------------------------------------------
def test_tail_rule():
    assert gc.tail_plan(784, 18, True, 64, True) == (16, 9)              # 64x14x14, 64 -> 256, 3x3: the documented example
    assert gc.tail_plan(40, 2, True, 64, True) == (0, 1)                 # two K tiles: one slice
    assert gc.tail_plan(406, 9, True, 64, True) == (0, 1)                # r = 150 > 128
    assert gc.tail_plan(256, 9, True, 64, True) == (0, 1)                # r = 0
    assert gc.tail_plan(258, 72, True, 64, True) == (2, 16)              # the cap
    assert gc.tail_plan(7 * 256 + 2, 9, True, 64, True) == (0, 1)        # deep grids
    for dma, tile, ws in ((False, 64, True), (True, 128, True), (True, 64, False)):
        assert gc.tail_plan(258, 9, dma, tile, ws) == (0, 1)


@pytest.mark.parametrize("cid", gc.CONV_IDS)
def test_conv_table_is_self_consistent(cid):
    c = gc.CASE[cid]
    OH, OW, M, K = gc.conv_dims(c)
    assert OH > 0 and OW > 0
    im2col = not c.nchw and c.C % 32 == 0
    assert c.kind == (gc.IM2COL if im2col else gc.GATHER)
    assert c.dma == int(im2col and c.KH * c.KW <= 32 and K % 4 == 0)
    for tile, tail_ws in gc.conv_runs(c):
        T, nk = gc.ceil_div(M, tile) * gc.ceil_div(c.CO, tile), gc.ceil_div(K, gc.BK)
        plan = gc.tail_plan(T, nk, c.dma, tile, tail_ws)
        assert plan == (c.tail if (c.tail and tail_ws) else (0, 1)), (cid, tile, tail_ws, T, nk, plan)
        assert plan[0] * plan[1] <= 256                       # slabs of the tail workspace
    assert (M * c.CO * K) < 4e8                                # a few hundred million MACs at the most
    if c.kind == gc.GATHER:                                   # the table's condition, as the `why` states it
        table = K <= 256 and c.C * c.H * c.W < 2 ** 20
        assert table == (cid in ("V7a", "V7b", "V9a")), (cid, K, c.C * c.H * c.W)
        assert cid not in ("V8a", "V8b") or 256 < K <= 264 + 8          # just above the table's 256
    if cid == "V9a":
        assert 2 ** 20 - 5000 < c.C * c.H * c.W < 2 ** 20
    if cid == "V9b":
        assert c.C * c.H * c.W == 2 ** 20
    if cid == "V10a":
        assert M % 64 == 52 and gc.ceil_div(M, 64) == 40
    if cid == "V10b":
        assert gc.ceil_div(M, 64) * 2 == 258 and M % 64 == 40


def test_the_issue_shapes_of_v10_do_not_split():
    """Why V10 differs from the shapes first proposed: by the rule neither of them reaches the fix-up."""
    assert gc.tail_plan(gc.ceil_div(13 * 196, 64) * 1, 2, True, 64, True) == (0, 1)
    assert gc.tail_plan(gc.ceil_div(66 * 196, 64) * 2, 9, True, 64, True) == (0, 1)


@pytest.mark.parametrize("cid", gc.GEMM_IDS)
def test_gemm_table_is_self_consistent(cid):
    c = gc.CASE[cid]
    tile = gc.gemm_tile(c)
    assert c.key == gc.route_key(gc.gemm_dma_expected(c), tile, gc.COLK if c.a else gc.ROWK, gc.COLK if c.b else gc.ROWK), cid
    assert c.lda >= (c.M if c.a else c.K) and c.ldb >= (c.N if c.b else c.K) and c.ldc >= c.N
    assert c.splitk > 1 or c.K <= 640                          # the long K only under split-K
    slices, per = gc.eff_splitk(c.K, c.splitk)
    nk = gc.ceil_div(c.K, gc.BK)
    assert (slices - 1) * per < nk <= slices * per and slices <= min(max(c.splitk, 1), nk)
    assert gc.ws_floats(c) >= (slices * c.M * c.N if slices > 1 else 0)
    inp = gc.inputs(cid)
    assert inp["a_buf"].numel() == c.a_off + ((c.K if c.a else c.M) + gc.PAD_ROWS) * c.lda
    assert inp["x"].shape == (c.M, c.K) and inp["w"].shape == (c.N, c.K)
    assert bool(torch.isfinite(inp["x"]).all()) and bool(torch.isfinite(inp["w"]).all())
    assert int(torch.isnan(inp["a_buf"]).sum()) == inp["a_buf"].numel() - c.M * c.K
    assert int(torch.isnan(inp["b_buf"]).sum()) == inp["b_buf"].numel() - c.N * c.K


def test_key_arithmetic_and_split_rule():
    assert gc.route_key(1, 64, gc.ROWK, gc.ROWK) == 1000 and gc.route_key(1, 128, gc.IM2COL, gc.ROWK) == 1120
    assert gc.route_key(0, 128, gc.COLK, gc.COLK) == 111 and gc.route_key(0, 64, gc.GATHER, gc.ROWK) == 30
    assert gc.eff_splitk(2304, 12) == (12, 6) and gc.eff_splitk(2304, 7) == (7, 11) and gc.eff_splitk(2304, 5) == (5, 15)
    assert gc.eff_splitk(100, 9) == (4, 1) and gc.eff_splitk(1280, 8) == (8, 5) and gc.eff_splitk(100, 1) == (1, 4)
    assert gc.eff_splitk(160, 4) == (3, 2)                    # five K tiles in four: two per slice, so three slices
    combos = lc.combos(gc.CASE["G1"])
    assert len(combos) == 16 and (0, 0, 1) in combos
    assert sorted({c.key for c in gc.GEMM_CASES}) == [0, 1, 10, 11, 100, 111, 1000, 1100]
    assert torch.tensor(gc.SENTINEL).float().double().item() == gc.SENTINEL


# ---- 5. the bounds tell the mutants -----------------------------------------------------------------------------------------------------
def test_every_mutant_is_due_somewhere():
    assert set().union(*(gc.mutants_due(c) for c in gc.CASES)) == set(gc.MUTANT_NAMES)
    assert "tap (KH-1, KW-1) dropped" in gc.mutants_due(gc.CASE["V2"]) and "kh and kw swapped" in gc.mutants_due(gc.CASE["V4a"])


@pytest.mark.parametrize("cid", gc.GEMM_IDS + gc.CONV_IDS)
def test_bounds_tell_the_mutants(cid):
    """Each fp64 mutant of the reference - one wrong term - lies beyond ten times the bound wherever it changes anything, and every
    mutant that is due in this case changes something."""
    c = gc.CASE[cid]
    nearest = {}

    def see(name, d, b, where):
        assert name in gc.MUTANT_NAMES, name
        if d == 0.0:
            return
        nearest[name] = min(nearest.get(name, (math.inf,)), (d / b,) + where)
        assert d >= 10.0 * b, (cid, name, where, d, b)

    for bias, act, acc in _combos(c):
        ref = gc.reference(cid, bias, act, acc)
        b = gc.bound(cid, bias, act, acc, ref)
        for name, m in gc.mutants(cid, bias, act, acc).items():
            see(name, oc.scaled_err(m, ref), b, (bias, lc.ACT_NAMES[act], acc))
    if c in gc.CONV_CASES:
        for bias in (1, 0):
            for tile in c.tiles:
                ref, bs, _ = gc.partial_bounds(cid, bias, tile)
                for name, m in gc.partial_mutants(cid, bias, tile).items():
                    k = 1 if name == "sum of squares before the bias" else None
                    for kind in ((k,) if k is not None else (0, 1)):
                        see(name, oc.scaled_err(m[:, kind], ref[:, kind]), bs[kind], (bias, f"tile {tile} partial {kind}", 0))
    assert set(nearest) == gc.mutants_due(c), (cid, sorted(nearest), sorted(gc.mutants_due(c)))
    for name, (ratio, bias, act, acc) in sorted(nearest.items()):
        print(f"[gemm-mutants] {cid} {name}: smallest distance / bound {ratio:.3g} at bias {bias} {act} accumulate {acc}")
