"""timm dynamic_img_size (quick_start/keep_inference.py:32-40) without a GPU: the Python-side tile-size rule of the opt-in, the constructor /
from_pretrained / HF plumbing of the flag, and the ctypes signatures of the new C-ABI entry points."""
import ctypes as C

import pytest

import keep_amd.hf                                          # noqa: F401
from keep_amd import KEEPModel, _lib, build
from keep_amd.config import small_shape
from keep_amd.synth import write_synthetic_release
from transformers import AutoModel


def test_default_is_224_only():
    m = KEEPModel(small_shape(1, 1))
    assert m.dynamic_img_size is False
    m._check_hw(224, 224, "x")
    for H, W in ((256, 256), (16, 16), (224, 448), (223, 224)):
        with pytest.raises(ValueError, match="224x224"):
            m._check_hw(H, W, "x")


def test_opt_in_accepts_multiples_of_16():
    m = KEEPModel(small_shape(1, 1), dynamic_img_size=True)
    assert m.dynamic_img_size is True
    for H, W in ((16, 16), (224, 224), (256, 256), (512, 512), (112, 448), (1024, 256)):
        m._check_hw(H, W, "x")
    for H, W in ((0, 224), (224, 0), (8, 16), (250, 256), (256, 17), (-16, 32)):
        with pytest.raises(ValueError, match="multiples of 16"):
            m._check_hw(H, W, "x")


def test_flag_reaches_from_pretrained_and_automodel(tmp_path_factory):
    release = write_synthetic_release(str(tmp_path_factory.mktemp("KEEP_release")), small_shape(1, 1), seed=4)
    assert KEEPModel.from_pretrained(release, dynamic_img_size=True).dynamic_img_size is True
    assert KEEPModel.from_pretrained(release).dynamic_img_size is False
    assert AutoModel.from_pretrained(release, dynamic_img_size=True).dynamic_img_size is True
    assert AutoModel.from_pretrained(release).dynamic_img_size is False


def test_signatures_of_the_new_exports():
    S = _lib.SIGNATURES
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    # keep_encode_image_hw(h, pixels, pix_dtype, B, H, W, out, stream)
    assert S["keep_encode_image_hw"] == (i32, [vp, vp, i32, i64, i64, i64, vp, vp])
    # keep_vit_pos_embed(h, gh, gw, out, stream)
    assert S["keep_vit_pos_embed"] == (i32, [vp, i32, i32, vp, vp])
    # keep_op_attention_long(h, qkv, B, T, heads, split, q_rows, out, stream)
    assert S["keep_op_attention_long"] == (i32, [vp, vp, i64, i64, i32, i32, i32, vp, vp])
    # keep_encode_image keeps its six arguments
    assert S["keep_encode_image"] == (i32, [vp, vp, i32, i64, vp, vp])


def test_new_exports_refuse_a_null_handle():
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.keep_encode_image_hw(None, None, 0, 1, 224, 224, None, None) == _lib.KEEP_EINVAL
    assert lib.keep_vit_pos_embed(None, 14, 14, None, None) == _lib.KEEP_EINVAL
    assert lib.keep_op_attention_long(None, None, 1, 600, 1, 0, 0, None, None) == _lib.KEEP_EINVAL
