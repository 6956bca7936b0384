"""keep_set_option / keep_get_option, name by name: defaults (include/keep_hip.h), round trips, the bool clamp, every rejected value with
its error text and the value it leaves behind, the write-only and read-only names, and the two options with side effects (the comp_*
shorthands rewrite the per-block plan; cls_tail invalidates a bias calibration made under the other setting).

Characterisation: the expected defaults and strings are what the engine answered before the setter and the getter were put on one table.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from keep_amd import KEEPModel, _lib
from keep_amd.config import small_shape
from keep_amd.synth import synth_state_dict, synth_tiles

pytestmark = pytest.mark.gpu

# name -> (default, a valid value other than the default, [(rejected value, keep_last_error)])
RANGED = {
    "strict_blocks": (0, 3, [(-1, "strict_blocks < 0")]),
    "comp_full_blocks": (1, 2, [(-1, "comp_full_blocks < 0")]),
    "comp_mlp_blocks": (8, 5, [(-1, "comp_mlp_blocks < 0")]),
    "comp_qkv_from": (1 << 20, 3, [(-1, "comp_qkv_from < 0")]),
    "comp_min_tiles": (32, 48, [(23, "comp_min_tiles must be >= 24 (the compensated product needs the 256x256 kernel)")]),
    "max_tiles": (256, 8, [(0, "max_tiles < 1")]),
    "max_prompts": (64, 16, [(0, "max_prompts < 1")]),
    "grid_plan": (1, 2, [(-1, "grid_plan must be 0, 1 or 2"), (3, "grid_plan must be 0, 1 or 2")]),
    "streams": (2, 4, [(0, "streams must be 1..4"), (5, "streams must be 1..4")]),
    "gemm_persistent": (1, 0, [(-1, "gemm_persistent must be 0..1024"), (1025, "gemm_persistent must be 0..1024")]),
    "gemm_splitk_tiles": (64, 256, [(-1, "gemm_splitk_tiles must be 0..256"), (257, "gemm_splitk_tiles must be 0..256")]),
    "sgemv_m": (16, 8, [(-1, "sgemv_m must be 0..16"), (17, "sgemv_m must be 0..16")]),
    "gemm_skinny_m": (320, 1024, [(-1, "gemm_skinny_m must be 0..1024"), (1025, "gemm_skinny_m must be 0..1024")]),
    "ln_impl": (2, 0, [(-1, "ln_impl must be 0, 1 or 2"), (3, "ln_impl must be 0, 1 or 2")]),
    # the options whose domain is a set
    "precision": (_lib.PREC_COMP, _lib.PREC_FP16, [(3, "precision 3"), (-1, "precision -1")]),
    "proj_impl": (2128, 0, [(1, "proj_impl must be 0 or 2128"), (128, "proj_impl must be 0 or 2128")]),
    "attn_waves": (16, 4, [(12, "attn_waves must be 4, 8 or 16 (16: persistent double-buffered kernel for the image tower)"),
                           (0, "attn_waves must be 4, 8 or 16 (16: persistent double-buffered kernel for the image tower)")]),
    "gemm_impl": (0, 128, [(64, "gemm_impl 64 (0, 128, 256)"), (-1, "gemm_impl -1 (0, 128, 256)")]),
}
BOOLS = {"graphs": 1, "comp_qkv": 0, "cls_tail": 1, "patch_split": 1, "bias_correction": 1, "skinny_wide": 1}      # name -> default
# can be set (ranges checked) but read back as -1
WRITE_ONLY = {
    "fused_screening": (2, [(-1, "fused_screening must be 0..2"), (3, "fused_screening must be 0..2")]),
    "lane_min_tiles": (8, [(5, "lane_min_tiles must be >= 6")]),
}
READ_ONLY = {"plan_custom": 0, "bias_ready": 0}


@pytest.fixture()
def handle():
    lib = _lib.load()
    h = C.c_void_p(0)
    assert lib.keep_create(0, C.byref(h)) == _lib.KEEP_OK
    yield h
    lib.keep_destroy(h)


def _set(h, name, value):
    return _lib.load().keep_set_option(h, name.encode(), float(value))


def _get(h, name):
    return _lib.load().keep_get_option(h, name.encode())


def _err(h):
    return _lib.load().keep_last_error(h).decode()


def test_defaults(handle):
    for name, (default, _, _) in RANGED.items():
        assert _get(handle, name) == default, name
    for name, default in {**BOOLS, **READ_ONLY}.items():
        assert _get(handle, name) == default, name
    for name in WRITE_ONLY:
        assert _get(handle, name) == -1, name
    assert _get(handle, "label_margin") == float(np.float32(2.5e-4))
    assert _get(handle, "nope") == -1


@pytest.mark.parametrize("name", sorted(RANGED))
def test_ranged_option(handle, name):
    default, valid, rejected = RANGED[name]
    assert _set(handle, name, valid) == _lib.KEEP_OK and _get(handle, name) == valid
    for bad, msg in rejected:
        assert _set(handle, name, bad) == _lib.KEEP_EINVAL, (name, bad)
        assert _err(handle) == msg
        assert _get(handle, name) == valid, (name, bad)            # a rejected value changes nothing
    assert _set(handle, name, default) == _lib.KEEP_OK and _get(handle, name) == default
    for v in {"precision": (_lib.PREC_STRICT,), "attn_waves": (8,), "gemm_impl": (256,)}.get(name, ()):      # every member of a set
        assert _set(handle, name, v) == _lib.KEEP_OK and _get(handle, name) == v


@pytest.mark.parametrize("name", sorted(BOOLS))
def test_bool_option_clamps(handle, name):
    for v, want in ((7, 1), (0, 0), (-3, 1), (1, 1)):
        assert _set(handle, name, v) == _lib.KEEP_OK and _get(handle, name) == want, (name, v)


@pytest.mark.parametrize("name", sorted(WRITE_ONLY))
def test_write_only_option(handle, name):
    valid, rejected = WRITE_ONLY[name]
    assert _set(handle, name, valid) == _lib.KEEP_OK and _get(handle, name) == -1
    for bad, msg in rejected:
        assert _set(handle, name, bad) == _lib.KEEP_EINVAL and _err(handle) == msg and _get(handle, name) == -1


def test_label_margin_is_a_float_in_0_2(handle):
    for v in (1e-3, 0.0, 2.0):
        assert _set(handle, "label_margin", v) == _lib.KEEP_OK and _get(handle, "label_margin") == float(np.float32(v))
    for bad in (-0.1, 2.5):
        assert _set(handle, "label_margin", bad) == _lib.KEEP_EINVAL
        assert _err(handle) == "label_margin must be in [0, 2]" and _get(handle, "label_margin") == 2.0


def test_unknown_and_read_only_names(handle):
    assert _set(handle, "nope", 0) == _lib.KEEP_EINVAL and _err(handle) == "unknown option nope"
    for name in READ_ONLY:
        assert _set(handle, name, 1) == _lib.KEEP_EINVAL and _err(handle) == f"unknown option {name}"
        assert _get(handle, name) == 0
    for name in ("gemm_ablate", "gemm_dbg"):                       # diagnostics builds only
        assert _set(handle, name, 1) == _lib.KEEP_EINVAL and _err(handle) == f"unknown option {name}" and _get(handle, name) == -1


def test_prefix_shorthand_rewrites_the_plan(handle):
    lib = _lib.load()

    def block(i):
        a, m = C.c_int32(-1), C.c_int32(-1)
        assert lib.keep_get_block_precision(handle, i, C.byref(a), C.byref(m)) == _lib.KEEP_OK
        return a.value, m.value

    assert block(0) == (_lib.ATTN_SPLIT_COMPQKV, _lib.MLP_COMP) and block(3) == (_lib.ATTN_PLAIN, _lib.MLP_CLS)      # the plan a handle starts with
    assert lib.keep_set_block_precision(handle, 3, _lib.ATTN_SPLIT, _lib.MLP_SPLIT) == _lib.KEEP_OK
    assert _get(handle, "plan_custom") == 1 and block(3) == (_lib.ATTN_SPLIT, _lib.MLP_SPLIT)
    assert _set(handle, "comp_mlp_blocks", 2) == _lib.KEEP_OK
    assert _get(handle, "plan_custom") == 0
    assert [block(i) for i in range(4)] == [(_lib.ATTN_SPLIT, _lib.MLP_COMP), (_lib.ATTN_PLAIN, _lib.MLP_COMP),
                                            (_lib.ATTN_PLAIN, _lib.MLP_PLAIN), (_lib.ATTN_PLAIN, _lib.MLP_PLAIN)]
    assert lib.keep_set_block_precision(handle, 3, -1, _lib.MLP_CLS) == _lib.KEEP_OK and _get(handle, "plan_custom") == 1
    assert _set(handle, "comp_mlp_blocks", -1) == _lib.KEEP_EINVAL and _get(handle, "plan_custom") == 1     # rejected: the plan stays
    assert _set(handle, "comp_qkv", 1) == _lib.KEEP_OK and _get(handle, "plan_custom") == 0
    assert block(0) == (_lib.ATTN_SPLIT_COMPQKV, _lib.MLP_COMP) and block(3) == (_lib.ATTN_PLAIN, _lib.MLP_PLAIN)


def test_cls_tail_invalidates_a_bias_calibration():
    m = KEEPModel(small_shape(2, 2), towers=("image",))
    m.auto_calibrate = False
    m.load_state_dict(synth_state_dict(small_shape(2, 2), seed=5, text=False), strict=True)
    m.to("cuda:0").eval()
    assert m.get_option("bias_ready") == 0
    m.calibrate_bias(tiles=synth_tiles(8, seed=3))
    assert m.get_option("bias_ready") == 1
    m.set_option("cls_tail", 1)                                    # the setting it was calibrated under: still valid
    assert m.get_option("bias_ready") == 1
    m.set_option("cls_tail", 0)
    assert m.get_option("bias_ready") == 0 and m.get_option("cls_tail") == 0
