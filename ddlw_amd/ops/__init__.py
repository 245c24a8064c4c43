"""``ddlw_amd.ops`` — hand-written CDNA4 (gfx950) HIP kernels.

The implicit GPU-kernel inventory of the reference rebuilt
as native HIP, built by ``ddlw_amd/ops/build.py`` (raw hipcc — no hipify, no
CUDA path, no Triton) and bound via ctypes: ``abi.py`` holds the signature
table, ``binding.py`` / ``conv_gemm.py`` the tensor-level wrappers.

On a GPU box the HIP extension is REQUIRED: ops raise if the library is
missing (no silent eager fallback; override only via DDLW_DISABLE_HIP_OPS=1).
On CPU the same layers fall back to stock PyTorch, which doubles as the
numerics oracle for the parity tests.
"""
from .runtime import lib, has_lib, require_lib, KernelLibError
from .layers import (
    BatchNormAct2d,
    MaxPool3x3s2,
    GlobalAvgPool2d,
    softmax_cross_entropy,
    softmax_ce_metrics,
    normalize_u8_bf16,
)
from .optim import FusedSGD, FusedAdam, FusedAdadelta
from .conv import Conv2d
from .precision import apply_bf16_policy, prepare_batch

__all__ = [
    "lib",
    "has_lib",
    "require_lib",
    "KernelLibError",
    "BatchNormAct2d",
    "MaxPool3x3s2",
    "GlobalAvgPool2d",
    "softmax_cross_entropy",
    "softmax_ce_metrics",
    "normalize_u8_bf16",
    "FusedSGD",
    "FusedAdam",
    "FusedAdadelta",
    "Conv2d",
    "apply_bf16_policy",
    "prepare_batch",
]
