"""The launch plan of the split-operand contractions (plan_bf3, csrc/bf3_plan.cpp: a function of the launch's parameters and a
Bf3Policy value, csrc/bf3_plan.h) on the CPU: kernel, grid, workgroup size, fix-up, BatchNorm partial-sum rows and profile key for every
convolution of the product's hot path.  The plan makes no HIP call, so dic_debug_bf3_plan runs without a GPU; it answers for the
process-wide policy, which the tests set through the switch codes and restore.  tests/golden/bf3_plan.json was recorded from the
launches of the library before the plan was separated from them (each launch reported instead of made), and
tests/golden/bf3_plan_switches.json from the library before the policy became a value, so both pin the policy as it was."""
import ctypes
import json
import os

from depth_image_captioning_pub_amd import build, synthetic

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "bf3_plan.json")
PLANES, BN1X1, BN3X3, WGRAD, STEM = range(5)                  # routes of dic_debug_bf3_plan
RES, COPY, RES_BN, BIAS, NO_STATS = 1, 2, 4, 8, 16            # its flags
TAIL_SLABS = 1024                                             # kResnetTailSlabs: the ResNet and depth-encoder workspaces


def resnet_cases(fmt, B):
    """(route, fmt, B, H, W, C, CO, k, stride, pad, flags, splitk, tail_slabs) of every route each ResNet-152 convolution can take."""
    out = [(STEM, fmt, B, 224, 224, 3, 64, 7, 2, 3, 0, 1, 0)]
    h = hin = 56
    for key, _bn, co, ci, k, s, p in synthetic.resnet152_spec()[1:]:
        if key.endswith("conv1.weight"):
            hin = h
            ih = h
        elif key.endswith("conv2.weight"):
            ih = h
            h = (h + 2 * p - k) // s + 1
        elif key.endswith("conv3.weight"):
            ih = h
        else:                                                 # downsample: the block input
            ih = hin
        out.append((PLANES, fmt, B, ih, ih, ci, co, k, s, p, 0, 1, TAIL_SLABS))
        if k == 1 and s == 1:
            for flags in (0, RES | COPY) + ((RES | RES_BN,) if fmt else ()):
                out.append((BN1X1, fmt, B, ih, ih, ci, co, 1, 1, 0, flags, 1, TAIL_SLABS))
        if k == 3 and s == 1:
            out.append((BN3X3, fmt, B, ih, ih, ci, co, 3, 1, 1, 0, 1, TAIL_SLABS))
    return out


def depth_encoder_cases(fmt, B=64):
    """conv2 (3x3, 24x24 -> 22x22, 128 -> 512) and conv3 (1x1, 7x7, 512 -> 2048) of the depth encoder: forward, data gradient
    (the stride-1 full correlation with the flipped kernel), weight gradient with the encoder's K split."""
    out = []
    for H, C, CO, k, splitk in ((24, 128, 512, 3, 5), (7, 512, 2048, 1, 3)):
        oh = H - k + 1
        out.append((PLANES, fmt, B, H, H, C, CO, k, 1, 0, BIAS, 1, TAIL_SLABS))
        out.append((PLANES, fmt, B, oh, oh, CO, C, k, 1, k - 1, NO_STATS, 1, TAIL_SLABS))
        out.append((WGRAD, fmt, B, H, H, C, CO, k, 1, 0, 0, splitk, 0))
    return out


# switch settings: (dic_conv_persistent_grid, dic_debug_force_staged_gemm code); 224 / 20 are the library's defaults, 11 / 21 force the
# 64x64 / 128x64 workgroup tile (no persistent kernel: the tile kernels, their tail K split and its BatchNorm-fused fix-up)
SETTINGS = {"224": (224, 20), "49": (49, 20), "tile11": (224, 11), "tile21": (224, 21)}


def all_cases():
    """{setting: sorted cases}"""
    default = set()
    for fmt, batches in ((1, (32, 64, 256)), (0, (64,))):
        for B in batches:
            default.update(resnet_cases(fmt, B))
    for fmt in (0, 1):
        default.update(depth_encoder_cases(fmt))
    b64 = set(resnet_cases(1, 64)) | set(resnet_cases(0, 64)) | set(depth_encoder_cases(1)) | set(depth_encoder_cases(0))
    return {"224": sorted(default), "49": sorted(set(resnet_cases(1, 64)) | set(depth_encoder_cases(1))),
            "tile11": sorted(b64), "tile21": sorted(b64)}


def query(lib, case):
    name = ctypes.create_string_buffer(512)
    out = (ctypes.c_int * 6)()
    rc = lib.dic_debug_bf3_plan(*case, name, len(name), out)
    assert rc in (0, 1), (case, rc, lib.dic_last_error())
    if rc == 1:
        return "not eligible"
    return [name.value.decode()] + list(out)        # kernel, grid, workgroup size, fix-up, its workgroups / quadrants, rows, key


def test_plan_matches_the_recorded_launches():
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    with open(GOLDEN) as f:
        golden = json.load(f)
    seen = 0
    try:
        for setting, cases in all_cases().items():
            grid, code = SETTINGS[setting]
            assert lib.dic_conv_persistent_grid(grid) == 0 and lib.dic_debug_force_staged_gemm(code) == 0
            want = golden[setting]
            for case in cases:
                key = " ".join(map(str, case))
                assert key in want, f"case {key} missing from {GOLDEN}"
                assert query(lib, case) == want[key], key
                seen += 1
    finally:
        assert lib.dic_conv_persistent_grid(224) == 0 and lib.dic_debug_force_staged_gemm(20) == 0
    assert seen == sum(len(v) for v in golden.values())


# The product's other plan-visible switches, each one code away from the default: {code: the code that restores the default}.
# tests/golden/bf3_plan_switches.json holds, per code, the cases of switch_cases() whose plan differs from the default setting's
# ("224" of bf3_plan.json), recorded from the library as it stood before the policy became a value.
SWITCHES = {70: 79, 73: 79, 75: 78, 90: 91, 81: 80, 94: 95, 96: 97, 112: 113, 115: 114, 118: 119, 120: 121, 24: 20}
GOLDEN_SWITCHES = os.path.join(os.path.dirname(__file__), "golden", "bf3_plan_switches.json")


def switch_cases():
    return sorted(set(resnet_cases(1, 64)) | set(resnet_cases(0, 64)) | set(depth_encoder_cases(1)) | set(depth_encoder_cases(0)))


def test_plan_under_each_switch():
    """Every case either has the plan recorded for the switch, which differs from the default's, or keeps the default plan."""
    lib = ctypes.CDLL(build.build())
    lib.dic_last_error.restype = ctypes.c_char_p
    with open(GOLDEN) as f:
        default = json.load(f)["224"]
    with open(GOLDEN_SWITCHES) as f:
        golden = json.load(f)
    cases = switch_cases()
    keys = {" ".join(map(str, case)) for case in cases}
    assert len(cases) == 126 and sorted(golden) == sorted(map(str, SWITCHES))
    assert lib.dic_conv_persistent_grid(224) == 0 and lib.dic_debug_force_staged_gemm(20) == 0
    for code, restore in SWITCHES.items():
        want = golden[str(code)]
        assert want, f"switch {code}: no recorded plan differs from the default's"
        assert set(want) <= keys, f"switch {code}: recorded cases outside switch_cases()"
        try:
            assert lib.dic_debug_force_staged_gemm(code) == 0
            for case in cases:
                key = " ".join(map(str, case))
                if key in want:
                    assert want[key] != default[key], (code, key)
                assert query(lib, case) == want.get(key, default[key]), (code, key)
        finally:
            assert lib.dic_debug_force_staged_gemm(restore) == 0
        for case in cases[::9]:                     # the restoring code brings the default back
            key = " ".join(map(str, case))
            assert query(lib, case) == default[key], (code, restore, key)
