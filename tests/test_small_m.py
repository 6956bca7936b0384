"""The single-operator entry points behind tests/test_small_m_gpu.py, without a GPU: their ctypes signatures and the argument checks that
come before anything touches the device (a null handle, with arguments that are otherwise valid and with ones that are not)."""
import ctypes as C

from keep_amd import _lib, build


def test_signatures_of_the_small_m_exports():
    S = _lib.SIGNATURES
    vp, i64, i32, f32 = C.c_void_p, C.c_int64, C.c_int, C.c_float
    # keep_op_linear_ln(h, a, w, bias, ls, resid, ln_gamma, ln_beta, ln_eps, M, N, K, epi, split, out, ln_out, ln_hi, did_ln, stream)
    assert S["keep_op_linear_ln"] == (i32, [vp, vp, vp, vp, vp, vp, vp, vp, f32, i64, i64, i64, i32, i32, vp, vp, vp, C.POINTER(i32), vp])
    # keep_op_attention_cls(h, qkv, B, T, heads, split, q_rows, out, cls_out, stream)
    assert S["keep_op_attention_cls"] == (i32, [vp, vp, i64, i64, i32, i32, i32, vp, vp, vp])
    # the operators they extend keep their arguments
    assert S["keep_op_linear"] == (i32, [vp, vp, vp, vp, vp, vp, i64, i64, i64, i32, i32, vp, vp])
    assert S["keep_op_attention"] == (i32, [vp, vp, vp, i64, i64, i32, i32, vp, vp])


def test_small_m_exports_refuse_a_null_handle():
    """No handle: KEEP_EINVAL, whatever else is passed (nothing is dereferenced, no device call is made: this runs where there is no GPU)."""
    build.build(verbose=False)
    lib = _lib.load()
    did = C.c_int(7)
    for M, epi, split in ((1, 2, 0), (64, 4, 1), (0, 2, 0), (-3, 4, 0), (1, 0, 0), (1, 3, 1), (1, 2, 5)):
        assert lib.keep_op_linear_ln(None, None, None, None, None, None, None, None, 1e-6, M, 1024, 1024, epi, split, None, None, None,
                                     C.byref(did), None) == _lib.KEEP_EINVAL
    assert did.value == 7                                    # a refused call writes nothing
    for B, T, heads, split, q_rows in ((1, 197, 16, 0, 1), (2, 64, 12, 1, 0), (1, 197, 16, 0, -1), (0, 197, 16, 0, 0), (1, 0, 1, 0, 0)):
        assert lib.keep_op_attention_cls(None, None, B, T, heads, split, q_rows, None, None, None) == _lib.KEEP_EINVAL
