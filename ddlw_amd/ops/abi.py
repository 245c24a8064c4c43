"""The C ABI of ``libddlw_kernels.so``: one signature per ``DDLW_EXPORT``.

``runtime._try_load`` applies this table to the ``CDLL`` once, so call sites
pass tensors, ints and floats as they are and ctypes converts (and range-
checks) each one against the declared C type. ``tests/test_abi.py`` parses
the ``DDLW_EXPORT`` declarations out of ``hip/*.hip`` and fails if they and
this table disagree. This is the only module under ``ddlw_amd/`` that
constructs ctypes values.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_char_p, c_float, c_int, c_long, c_ulonglong


class Ptr(ctypes.c_void_p):
    """``void*`` parameter: a tensor (its ``data_ptr()``), ``None`` (null) or
    a raw integer address (a HIP stream, a pointer with an offset applied)."""

    @classmethod
    def from_param(cls, v):
        if v is None or isinstance(v, int):
            return ctypes.c_void_p(v)
        return ctypes.c_void_p(v.data_ptr())


def long_array(values):
    """Host array for a ``const long*`` parameter."""
    return (c_long * len(values))(*values)


def int_array(values):
    """Host array for a ``const int*`` parameter."""
    return (c_int * len(values))(*values)


_P, _I, _L, _F = Ptr, c_int, c_long, c_float

# name -> (restype, argtypes). Every launching export ends in ``void* stream``.
SIGNATURES = {
    # core.hip
    "ddlw_last_error": (c_char_p, []),
    "ddlw_device_sync": (_I, []),
    # bn.hip
    "ddlw_bn_nparts": (_I, [_L, _I]),
    "ddlw_bn_stats": (_I, [_P, _P, _P, _L, _I, _P]),
    "ddlw_bn_parts_fold": (_I, [_P, _P, _P, _P, _L, _I, _I, _P]),
    "ddlw_bn_finalize": (_I, [_P] * 6 + [_L, _I, _I, _F, _F, _P]),
    "ddlw_bn_apply": (_I, [_P] * 8 + [_L, _I, _I, _P]),
    "ddlw_bn_bwd_reduce": (_I, [_P] * 7 + [_L, _I, _I, _P]),
    "ddlw_bn_grad_finalize": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "ddlw_bn_bwd_dx": (_I, [_P] * 10 + [_L, _I, _I, _P]),
    # pool.hip
    "ddlw_maxpool3x3s2_fwd": (_I, [_P, _P, _P] + [_I] * 6 + [_P]),
    "ddlw_maxpool3x3s2_bwd": (_I, [_P, _P, _P] + [_I] * 6 + [_P]),
    "ddlw_gap_fwd": (_I, [_P, _P, _I, _I, _I, _P]),
    "ddlw_gap_bwd": (_I, [_P, _P, _I, _I, _I, _P]),
    # head.hip
    "ddlw_softmax_ce": (_I, [_P, _P, _P, _P, _I, _I, _F, _P]),
    "ddlw_dropout_fwd": (_I, [_P, _P, _P, _L, _F, c_ulonglong, _P]),
    "ddlw_dropout_bwd": (_I, [_P, _P, _P, _L, _F, _P]),
    "ddlw_argmax_rows": (_I, [_P, _P, _L, _I, _P]),
    "ddlw_accuracy": (_I, [_P, _P, _P, _L, _I, _P]),
    "ddlw_ce_metrics_nblocks": (_I, [_I, _I, _P]),
    "ddlw_ce_metrics": (_I, [_P] * 6 + [_I, _I, _F, _I, _P]),
    "ddlw_normalize_u8": (_I, [_P, _P, _L, _P]),
    # optim.hip
    "ddlw_fused_sgd": (_I, [_P, _I, _L, _F, _F, _F, _I, _P]),
    "ddlw_fused_adam": (_I, [_P, _I, _L, _F, _F, _F, _F, _F, _F, _F, _P]),
    "ddlw_fused_adadelta": (_I, [_P, _I, _L, _F, _F, _F, _F, _P]),
    # depthwise.hip
    "ddlw_depthwise_fwd": (_I, [_P, _P, _P] + [_I] * 10 + [_P]),
    "ddlw_depthwise_fwd_ep": (_I, [_P] * 5 + [_I] * 9 + [_P]),
    "ddlw_depthwise_dgrad": (_I, [_P, _P, _P] + [_I] * 10 + [_P]),
    "ddlw_depthwise_wgrad_nparts": (_I, [_L, _I]),
    "ddlw_depthwise_wgrad": (_I, [_P, _P, _P, _P] + [_I] * 10 + [_P]),
    # pointwise.hip
    "ddlw_pw_conv_fwd": (_I, [_P] * 6 + [_I, _L, _I, _I, _P]),
    "ddlw_pw_conv_nparts": (_I, [_L, _I, _P]),
    "ddlw_pw_conv_fwd_stats": (_I, [_P] * 5 + [_L, _I, _I, _P]),
    # conv_gemm.hip
    "ddlw_conv_fwd_nparts": (_L, [_I] * 8),
    "ddlw_conv_fwd_igemm": (_I, [_P] * 14 + [_I] * 15 + [_P]),
    "ddlw_conv_dgrad_s2m": (_I, [_P] * 4 + [_I] * 9
                            + [POINTER(c_long), POINTER(c_long), POINTER(c_int), _P]),
    # conv_wgrad.hip
    "ddlw_conv_wgrad": (_I, [_P] * 5 + [_I] * 12 + [_P]),
    "ddlw_conv_wgrad3x3": (_I, [_P] * 5 + [_I] * 10 + [_P]),
    # conv_stem.hip
    "ddlw_stem_repack": (_I, [_P, _P, _I, _I, _I, _P]),
    "ddlw_conv_stem": (_I, [_P] * 4 + [_I] * 8 + [_P, _P, _I, _P]),
    "ddlw_stem_wgrad": (_I, [_P] * 5 + [_I] * 7 + [_P]),
    "ddlw_stem3_u8_fwd_ep": (_I, [_P] * 5 + [_I] * 6 + [_P]),
    "ddlw_stem3_u8_nparts": (_I, [_L, _P]),
    "ddlw_stem3_u8_fwd_stats": (_I, [_P] * 5 + [_I] * 6 + [_P]),
    "ddlw_stem3_u8_wgrad_nparts": (_I, [_L, _P]),
    "ddlw_stem3_u8_wgrad": (_I, [_P] * 4 + [_I] * 6 + [_P]),
}


def apply(cdll, on_missing) -> None:
    """Declare restype/argtypes for every export on ``cdll``. A name the
    library does not export goes to ``on_missing(name)``, which must raise."""
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            on_missing(name)
            raise
        fn.restype = restype
        fn.argtypes = argtypes
