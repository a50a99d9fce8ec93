"""The guarded arena and the allocation interception of tests/buffer_contract_common.py, tested on host tensors, and every workspace
size query of include/dic.h at the shapes of tests/test_buffer_contract_gpu.py (the queries are host functions: no GPU)."""
import ctypes as C

import pytest
import torch

import buffer_contract_common as bc
from depth_image_captioning_pub_amd import _lib


def _arena():
    return bc.GuardedArena("cpu")


# ---- 1. the arena ---------------------------------------------------------------------------------------------------------------------
def test_a_clean_use_passes():
    arena = _arena()
    t = arena.empty((3, 5), torch.float32, 0xFF, "clean")
    assert bool(torch.isnan(t).all())                                   # 0xFF bytes are NaN as fp32 ...
    assert bool(torch.isnan(arena.empty((2,), torch.float64, 0xFF)).all())          # ... and as fp64
    t.copy_(torch.arange(15.0).view(3, 5))
    arena.buffers[0].payload[-1] = 7                                    # the payload's last byte is the caller's
    arena.buffers[0].payload[0] = 7
    arena.check()
    assert arena.violations() == []


def test_layout_is_exact():
    arena = _arena()
    t = arena.empty((77,), torch.uint8, 0x00, "odd")
    g = arena.buffers[0]
    assert g.nbytes == 77 and g.payload.numel() == 77
    assert g.front.numel() == bc.FRONT_GUARD == (1 << 20) + 256 and g.back.numel() == bc.BACK_GUARD == 1 << 20
    assert g.back.data_ptr() == t.data_ptr() + 77                       # no rounding behind the payload
    assert g.front.data_ptr() + bc.FRONT_GUARD == t.data_ptr()
    assert t.data_ptr() % 256 == 0 and t.data_ptr() % 512 != 0
    assert bool((g.front == bc.GUARD_BYTE).all()) and bool((g.back == bc.GUARD_BYTE).all()) and bc.GUARD_BYTE == 0xA5


@pytest.mark.parametrize("side, at, offset", [
    ("back", 0, 40),                           # one byte past the payload (10 floats = 40 bytes)
    ("front", bc.FRONT_GUARD - 1, -1),         # one byte before the payload
    ("back", bc.BACK_GUARD - 1, 40 + bc.BACK_GUARD - 1),        # the far end of either guard
    ("front", 0, -bc.FRONT_GUARD),
])
def test_a_stray_byte_is_reported_with_its_buffer_and_offset(side, at, offset):
    arena = _arena()
    arena.empty((4,), torch.int32, 0x00, "bystander")
    arena.empty((10,), torch.float32, 0x00, "victim")
    getattr(arena.buffers[1], side)[at] = 0
    found = arena.violations()
    assert len(found) == 1
    assert found[0].startswith("victim (output, 40 bytes)") and f"{side} guard" in found[0] and "in 1 bytes" in found[0]
    assert f"offsets {offset} .. {offset} " in found[0]
    with pytest.raises(AssertionError, match="victim"):
        arena.check()


def test_first_and_last_offending_offsets():
    arena = _arena()
    arena.empty((3,), torch.uint8, 0x00, "row")
    arena.buffers[0].back[0:100:9] = 1                                  # offsets 3, 12, .. 3 + 99
    (line,) = arena.violations()
    assert "in 12 bytes" in line and "offsets 3 .. 102 " in line


def test_a_guard_byte_written_with_the_guard_value_is_invisible_by_construction():
    """What the harness cannot see, stated: a stray store of the byte 0xA5 itself.  The fills (0x00 / 0xFF) and every value a kernel
    computes from them differ from 0xA5A5A5A5 (fp32 -2.87e-16) except by accident."""
    arena = _arena()
    arena.empty((3,), torch.uint8, 0x00)
    arena.buffers[0].back[0] = bc.GUARD_BYTE
    arena.check()


# ---- 2. the interception --------------------------------------------------------------------------------------------------------------
def test_intercepted_allocations_are_exact():
    arena = _arena()
    real = torch.empty
    with bc.intercept_allocations(arena, 0xFF, workspace_fill=0x00) as made:
        a = torch.empty((3, 7), dtype=torch.float32)
        b = torch.empty(5, 2, dtype=torch.int64, device="cpu")
        ws = torch.empty(1000, dtype=torch.uint8, device=torch.device("cpu"))
        z = torch.zeros((4,), dtype=torch.float32)
        f = torch.full((2, 2), 3, dtype=torch.int32)
        like = torch.empty_like(a)
        n0 = a.new_zeros((3,))
        n1 = a.new_full((2,), 1.5)
        n2 = a.new_empty((2, 2))
        elsewhere = torch.empty((2,), dtype=torch.float32, device="meta")
    assert torch.empty is real
    assert len(made) == 9 and elsewhere.device.type == "meta"
    for t, shape, dtype in ((a, (3, 7), torch.float32), (b, (5, 2), torch.int64), (ws, (1000,), torch.uint8), (z, (4,), torch.float32),
                            (f, (2, 2), torch.int32), (like, (3, 7), torch.float32), (n0, (3,), torch.float32),
                            (n1, (2,), torch.float32), (n2, (2, 2), torch.float32)):
        g = arena.record_of(t)
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
        assert g.nbytes == t.numel() * t.element_size()
        assert t.data_ptr() % 256 == 0 and t.data_ptr() % 512 != 0
    assert bool(torch.isnan(a).all()) and bool((b == -1).all()) and bool(torch.isnan(like).all()) and bool(torch.isnan(n2).all())
    assert bool((ws == 0).all()) and [g.role for g in made].count("workspace") == 1 and arena.workspaces()[0].tensor is ws
    assert bool((z == 0).all()) and bool((f == 3).all()) and bool((n0 == 0).all()) and bool((n1 == 1.5).all())       # their own fill
    arena.check()


def test_the_workspace_is_the_uint8_request_of_the_queried_size():
    arena = _arena()
    with bc.intercept_allocations(arena, 0x00, workspace_fill=0xFF, workspace_bytes=512) as made:
        other = torch.empty(300, dtype=torch.uint8)
        ws = torch.empty(512, dtype=torch.uint8)
    assert [g.role for g in made] == ["output", "workspace"] and bool((other == 0).all()) and bool((ws == 0xFF).all())
    with bc.intercept_allocations(arena, 0x00, workspace_fill=0xFF, short_workspace=True) as made:
        ws = torch.empty(512, dtype=torch.uint8)
    assert ws.numel() == 511 and made[0].nbytes == 511 and made[0].back.data_ptr() == ws.data_ptr() + 511


def test_torch_is_restored_after_an_exception():
    before = {n: getattr(torch, n) for n in ("empty", "zeros", "full", "empty_like", "zeros_like", "full_like")}
    before_t = {n: torch.Tensor.__dict__.get(n) for n in ("new_empty", "new_zeros", "new_full")}
    with pytest.raises(RuntimeError, match="boom"):
        with bc.intercept_allocations(_arena(), 0x00):
            assert torch.empty is not before["empty"]
            raise RuntimeError("boom")
    assert all(getattr(torch, n) is f for n, f in before.items())
    assert all(torch.Tensor.__dict__.get(n) is f for n, f in before_t.items())
    assert torch.empty((2,)).new_zeros((1,)).shape == (1,)


# ---- 3. the size queries ----------------------------------------------------------------------------------------------------------------
V = 300
BLOCKS = (C.c_int * 4)(1, 1, 1, 1)
DEC = (3, 5)          # teacher-forced decoder: B 3, decode lengths (5, 3, 1): Tmax 5, n_packed 9
NIC = (3, 6)          # NIC: B 3, lengths (6, 4, 2): Tmax 6, n_packed 12
# name[/variant]: (the (B, T) of tests/test_buffer_contract_gpu.py, the query's arguments as a function of (B, T), made by Carver - then a
# multiple of 256).  n_packed grows by one row with B and by one step with T, as a batch with one more caption or a longer first one.
QUERIES = {
    "dic_decoder_workspace_bytes": (DEC, lambda B, T: (B, T, V, 9 + (B - 3) + (T - 5)), True),
    "dic_decoder_workspace_bytes/v77": (DEC, lambda B, T: (B, T, 77, 9 + (B - 3) + (T - 5)), True),
    "dic_decoder_greedy_workspace_bytes": ((2, 6), lambda B, T: (B, T, V), True),
    "dic_decoder_beam_workspace_bytes": ((2, 6), lambda B, T: (B, 3, T, V), True),
    "dic_decoder_sample_workspace_bytes": ((2, 6), lambda B, T: (B, 2, T, V), True),
    "dic_decoder_sample_workspace_bytes/v10300": ((2, 6), lambda B, T: (B, 2, T, 10300), True),
    "dic_decoder_score_workspace_bytes": ((2, 6), lambda B, T: (B, 2, T, V), True),
    "dic_decoder_beam_constrained_sizes": ((2, 6), lambda B, T: (B, 3, T, V), True),
    "dic_decoder_sample_constrained_sizes": ((2, 6), lambda B, T: (B, 2, T, V), True),
    "dic_decoder_beam_diverse_sizes": ((2, 6), lambda B, T: (B, 4, 2, T, V), True),
    "dic_decoder_beam_ensemble_sizes": ((2, 6), lambda B, T: (2, B, 3, T, V), True),
    "dic_decoder_states_workspace_bytes": ((2, 5), lambda B, T: (B, 2, T, V), True),
    "dic_decoder_states_hard_sizes": ((2, 5), lambda B, T: (B, 2, T, V), True),
    "dic_token_logprobs_workspace_bytes": ((130, 1), lambda M, T: (M * T, V), True),
    "dic_token_logprobs_workspace_bytes/v1000": ((130, 1), lambda M, T: (M * T, 1000), True),
    "dic_token_logprobs_bwd_workspace_bytes": ((130, 1), lambda M, T: (M * T, V), True),
    "dic_token_logprobs_bwd_workspace_bytes/v1000": ((130, 1), lambda M, T: (M * T, 1000), True),
    "dic_token_mean_logit_sizes": ((130, 1), lambda M, T: (M * T, V), True),
    "dic_token_mean_logit_sizes/v1000": ((130, 1), lambda M, T: (M * T, 1000), True),
    "dic_nic_workspace_bytes": (NIC, lambda B, T: (B, T, V, 12 + (B - 3) + (T - 6)), True),
    "dic_nic_greedy_workspace_bytes": ((2, 6), lambda B, T: (B, T, V), True),
    "dic_nic_beam_workspace_bytes": ((2, 6), lambda B, T: (B, 3, T, V), True),
    "dic_nic_score_sizes": ((2, 6), lambda B, T: (B, 2, T, V), True),
    "dic_nic_states_sizes": ((2, 5), lambda B, T: (B, 2, T, V), True),
    "dic_nic_sample_sizes": ((2, 6), lambda B, T: (B, 2, T, V), True),
    "dic_attention_workspace_bytes": ((3, 1), lambda B, T: (B,), True),
    "dic_attention_bwd_workspace_bytes": ((3, 1), lambda B, T: (B,), True),
    # (T: a size step of the image, 32 pixels - one cell of the final map)
    "dic_depth_encoder_workspace_bytes/b2-224": ((2, 0), lambda B, T: (B, 224 + 32 * T, 224 + 32 * T), True),
    "dic_depth_encoder_workspace_bytes/b3-100": ((3, 0), lambda B, T: (B, 100 + 32 * T, 100 + 32 * T), True),
    "dic_resnet_workspace_bytes/fp32-64": ((2, 0), lambda B, T: (B, 64 + 32 * T, 64 + 32 * T, BLOCKS, 0), True),
    "dic_resnet_workspace_bytes/bf16x3-64": ((2, 0), lambda B, T: (B, 64 + 32 * T, 64 + 32 * T, BLOCKS, 1), True),
    "dic_resnet_workspace_bytes/f16x2-64": ((2, 0), lambda B, T: (B, 64 + 32 * T, 64 + 32 * T, BLOCKS, 2), True),
    "dic_resnet_workspace_bytes/f16x2-224": ((1, 0), lambda B, T: (B, 224 + 32 * T, 224 + 32 * T, BLOCKS, 2), True),
    "dic_groupnorm_workspace_bytes": ((3, 0), lambda B, T: (B, 32), True),
    "dic_vit_attention_workspace_bytes": ((3, 37), lambda B, T: (B, T, 12), True),
}


def _query(lib, name, args):
    fn = getattr(lib, name.split("/")[0])
    if fn.restype is C.c_size_t:
        return int(fn(*args))
    out = C.c_size_t(0)
    assert fn(*args, C.byref(out)) == 0, name
    return int(out.value)


def test_the_table_names_every_size_query_of_the_header():
    declared = {n for n in _lib.prototypes() if (n.endswith("_workspace_bytes") or n.endswith("_sizes")) and "debug" not in n}
    assert declared == {n.split("/")[0] for n in QUERIES}


@pytest.mark.parametrize("name", sorted(QUERIES))
def test_size_query(name):
    lib = _lib.load()
    (B, T), args, carved = QUERIES[name]
    need = _query(lib, name, args(B, T))
    print(f"{name}{tuple(a for a in args(B, T) if isinstance(a, int))}: {need} bytes")
    assert need > 0
    if carved:
        assert need % 256 == 0
    assert _query(lib, name, args(B + 1, T)) >= need
    assert _query(lib, name, args(B, T + 1)) >= need
