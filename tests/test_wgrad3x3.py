"""Tap-fused 3x3 stride-1 weight gradient (``k_conv_wgrad3x3``): parity with
the fp32 reference and with the per-tap kernel, exact counts across image
borders and slice starts, zero padding, determinism, the routing gate and
the host-side slice function."""
import pytest
import torch

from ddlw_amd.ops import conv_gemm
from ddlw_amd.ops.conv_gemm import wgrad3x3_slices

gpu = pytest.mark.gpu

# (N, H, W, C, K): Wo below / at / off the padded widths, H != W, a row
# longer than one 32-m group, two tiles on each side; the last one runs the
# 32-wide instantiation (one row per 32-m group) that the 28x28 layers use
PARITY_SHAPES = [
    (3, 7, 7, 64, 64),
    (3, 14, 14, 128, 64),
    (2, 15, 15, 64, 128),
    (2, 6, 10, 64, 64),
    (2, 36, 36, 64, 64),
    (2, 28, 28, 64, 128),
]
PRIME_SPLIT = 7


def _cuda():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _ref(x, dy, K, C):
    return torch.nn.grad.conv2d_weight(x.float(), (K, C, 3, 3), dy.float(),
                                       stride=1, padding=1)


def _nerr(dw, ref):
    return ((dw.float() - ref).abs().max() / (ref.abs().max() + 1e-6)).item()


def _starts(rows, split):
    return [a for a, _ in wgrad3x3_slices(rows, split)]


# ---------------------------------------------------------------- slices (CPU)

def test_slice_function_partitions_rows():
    grid = [(rows, split) for rows in range(1, 41) for split in range(1, 46)]
    grid.append((256 * 56, 256))
    for rows, split in grid:
        sl = wgrad3x3_slices(rows, split)
        assert 1 <= len(sl) <= rows
        assert len(sl) == min(split, rows)
        assert sl[0][0] == 0 and sl[-1][1] == rows
        for (a0, a1), (b0, _) in zip(sl, sl[1:]):
            assert a1 == b0                      # contiguous, each row once
        sizes = [b - a for a, b in sl]
        assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
    # the workload's 56x56 layer: one image per slice
    assert wgrad3x3_slices(256 * 56, 256)[3] == (3 * 56, 4 * 56)


def test_prime_split_slice_starts():
    """With every parity shape the prime split starts a slice in the middle
    of an image (the halo row above is staged). A start on the border between
    two images (no halo row: the gap row) needs N*H and the split to agree:
    of the parity shapes only (2, 6, 10) has one, at row 6; the exact-count
    test places the others (row 7 of 14) with its own splits."""
    on_border = []
    for shape in PARITY_SHAPES:
        N, H = shape[0], shape[1]
        later = _starts(N * H, PRIME_SPLIT)[1:]
        assert len(later) == PRIME_SPLIT - 1
        assert any(s % H != 0 for s in later)
        if any(s % H == 0 for s in later):
            on_border.append(shape)
    assert on_border == [(2, 6, 10, 64, 64)]
    assert 6 in _starts(2 * 6, PRIME_SPLIT)[1:]


# ---------------------------------------------------------------- parity (GPU)

@gpu
@pytest.mark.parametrize("split", [None, 1, PRIME_SPLIT])
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_parity(shape, split):
    N, H, W, C, K = shape
    torch.manual_seed(3)
    x = _cl(torch.randn(N, C, H, W, device=_cuda()).to(torch.bfloat16))
    dy = _cl(torch.randn(N, K, H, W, device=_cuda()).to(torch.bfloat16))
    ref = _ref(x, dy, K, C)
    dw = conv_gemm.conv_wgrad3x3_kernel(dy, x, (K, C, 3, 3), 1, 1, split=split)
    old = conv_gemm.conv_wgrad_pertap_kernel(dy, x, (K, C, 3, 3), 1, 1)
    e_new, e_old = _nerr(dw, ref), _nerr(old, ref)
    print(f"wgrad3x3 {shape} split={split}: err {e_new:.3e} per-tap {e_old:.3e}")
    assert e_new <= 5e-2
    assert e_new <= 2 * e_old + 1e-3


# ---------------------------------------------------------- exact counts (GPU)

def _exact_case(x, dy, split):
    K, C = dy.shape[1], x.shape[1]
    dw = conv_gemm.conv_wgrad3x3_kernel(dy, x, (K, C, 3, 3), 1, 1, split=split)
    return dw.float(), _ref(x, dy, K, C)


@gpu
@pytest.mark.parametrize("split", [1, 2, 5, 14])
def test_exact_counts(split):
    """All-ones operands: every product is 1 and every partial sum an
    integer below 256, so the result is exact. A row leaking across the
    image border or a missing halo row at a slice start changes a count."""
    N, H, W, C, K = 2, 7, 7, 64, 64
    assert 7 in _starts(N * H, 2)     # slice start at ho = 0 of image 1
    assert 3 in _starts(N * H, 5)     # slice start at ho = 3
    assert {3, 7} <= set(_starts(N * H, 14))
    dev = _cuda()
    dy = _cl(torch.ones(N, K, H, W, device=dev, dtype=torch.bfloat16))
    ones = torch.ones(N, C, H, W, device=dev, dtype=torch.bfloat16)

    dw, ref = _exact_case(_cl(ones), dy, split)
    want = torch.empty(3, 3)
    for r in range(3):
        for s in range(3):
            want[r, s] = 2 * (7 - (r != 1)) * (7 - (s != 1))
    assert set(want.flatten().tolist()) == {72.0, 84.0, 98.0}
    assert torch.equal(dw, want.to(dev).expand(K, C, 3, 3))
    assert torch.equal(dw, ref)

    last0 = torch.zeros_like(ones)
    last0[0, :, H - 1, :] = 1          # only the last row of image 0
    dw, ref = _exact_case(_cl(last0), dy, split)
    assert torch.equal(dw, ref)
    assert dw[:, :, 0, :].abs().max().item() == 0   # nothing below row H-1

    first1 = torch.zeros_like(ones)
    first1[1, :, 0, :] = 1             # only the first row of image 1
    dw, ref = _exact_case(_cl(first1), dy, split)
    assert torch.equal(dw, ref)
    assert dw[:, :, 2, :].abs().max().item() == 0   # nothing above row 0


# --------------------------------------------------------------- padding (GPU)

@gpu
@pytest.mark.parametrize("shape", [(2, 7, 7, 64, 64), (2, 6, 10, 64, 64)])
def test_padding_is_zero_next_to_large_values(shape):
    """Columns 0 and W-1 hold +-3e38 (finite in bf16). A tap left of column
    0 or right of column W-1 that read a neighbouring row as data would put
    an edge value where the reference has none. dy is small so that the
    fp32 sums stay finite."""
    N, H, W, C, K = shape
    torch.manual_seed(5)
    dev = _cuda()
    x = torch.randn(N, C, H, W, device=dev)
    big = torch.tensor(3e38, dtype=torch.bfloat16).float().item()
    sign = torch.where(torch.rand(N, C, H, 2, device=dev) < 0.5, -1.0, 1.0)
    x[..., 0] = big * sign[..., 0]
    x[..., W - 1] = big * sign[..., 1]
    x = _cl(x.to(torch.bfloat16))
    assert torch.isfinite(x.float()).all()
    dy = _cl((1e-3 * torch.randn(N, K, H, W, device=dev)).to(torch.bfloat16))
    ref = _ref(x, dy, K, C)
    assert torch.isfinite(ref).all()
    for split in (None, 1, 5):
        dw = conv_gemm.conv_wgrad3x3_kernel(dy, x, (K, C, 3, 3), 1, 1,
                                            split=split).float()
        assert torch.isfinite(dw).all()
        assert _nerr(dw, ref) <= 5e-2


# ----------------------------------------------------------- determinism (GPU)

@gpu
def test_two_calls_bit_equal_and_lever(monkeypatch):
    """28x28 is routed to the tap-fused kernel by default, so the lever is
    what moves this input to k_conv_wgrad."""
    N, H, W, C, K = 2, 28, 28, 128, 64
    wshape = (K, C, 3, 3)
    torch.manual_seed(7)
    x = _cl(torch.randn(N, C, H, W, device=_cuda()).to(torch.bfloat16))
    dy = _cl(torch.randn(N, K, H, W, device=_cuda()).to(torch.bfloat16))
    a = conv_gemm.conv_wgrad3x3_kernel(dy, x, wshape, 1, 1)
    b = conv_gemm.conv_wgrad3x3_kernel(dy, x, wshape, 1, 1)
    assert torch.equal(a, b)
    pertap = conv_gemm.conv_wgrad_pertap_kernel(dy, x, wshape, 1, 1)

    names = _record_launches(monkeypatch)
    monkeypatch.delenv("DDLW_WGRAD_TAPS", raising=False)
    on = conv_gemm.conv_wgrad_kernel(dy, x, wshape, 1, 1)
    assert names == ["conv_wgrad3x3"]
    assert torch.equal(on, a)

    del names[:]
    monkeypatch.setenv("DDLW_WGRAD_TAPS", "0")
    off = conv_gemm.conv_wgrad_kernel(dy, x, wshape, 1, 1)
    assert names == ["conv_wgrad"]
    assert torch.equal(off, pertap)


@gpu
def test_lever_forces_the_widths_that_are_off_by_default(monkeypatch):
    """14x14 stays on the per-tap kernel by default; DDLW_WGRAD_TAPS=1 puts
    it on the tap-fused kernel (A/B through the model)."""
    wshape = (64, 64, 3, 3)
    torch.manual_seed(8)
    x = _cl(torch.randn(2, 64, 14, 14, device=_cuda()).to(torch.bfloat16))
    dy = _cl(torch.randn(2, 64, 14, 14, device=_cuda()).to(torch.bfloat16))
    names = _record_launches(monkeypatch)
    monkeypatch.delenv("DDLW_WGRAD_TAPS", raising=False)
    conv_gemm.conv_wgrad_kernel(dy, x, wshape, 1, 1)
    monkeypatch.setenv("DDLW_WGRAD_TAPS", "1")
    forced = conv_gemm.conv_wgrad_kernel(dy, x, wshape, 1, 1)
    assert names == ["conv_wgrad", "conv_wgrad3x3"]
    assert torch.equal(forced, conv_gemm.conv_wgrad3x3_kernel(dy, x, wshape, 1, 1))


# ------------------------------------------------------------------ gate (GPU)

def _record_launches(monkeypatch):
    names = []
    real = conv_gemm.launch

    def recording(name, *a):
        names.append(name)
        return real(name, *a)

    monkeypatch.setattr(conv_gemm, "launch", recording)
    return names


# (H, C, K, R, stride, pad): stride 2, 1x1, a channel count below the tile,
# all at 28x28, a width whose supported shapes are routed by default (and
# forced with the lever below), so a gate that let one through would send it
# to the export, which refuses it
UNSUPPORTED = [
    (28, 64, 64, 3, 2, 1),
    (28, 64, 64, 1, 1, 0),
    (28, 32, 64, 3, 1, 1),
]


@gpu
@pytest.mark.parametrize("lever", [None, "1"])
@pytest.mark.parametrize("case", UNSUPPORTED)
def test_gate_keeps_other_shapes_on_the_per_tap_kernel(monkeypatch, case, lever):
    H, C, K, R, st, pad = case
    monkeypatch.delenv("DDLW_WGRAD_TAPS", raising=False)
    if lever is not None:
        monkeypatch.setenv("DDLW_WGRAD_TAPS", lever)
    Ho = (H + 2 * pad - R) // st + 1
    torch.manual_seed(9)
    x = _cl(torch.randn(2, C, H, H, device=_cuda()).to(torch.bfloat16))
    dy = _cl(torch.randn(2, K, Ho, Ho, device=_cuda()).to(torch.bfloat16))
    names = _record_launches(monkeypatch)
    dw = conv_gemm.conv_wgrad_kernel(dy, x, (K, C, R, R), st, pad)
    assert names == ["conv_wgrad"]
    ref = torch.nn.grad.conv2d_weight(x.float(), (K, C, R, R), dy.float(),
                                      stride=st, padding=pad)
    assert _nerr(dw, ref) <= 5e-2


@gpu
def test_gate_routes_supported_shape(monkeypatch):
    monkeypatch.delenv("DDLW_WGRAD_TAPS", raising=False)
    torch.manual_seed(9)
    x = _cl(torch.randn(2, 64, 28, 28, device=_cuda()).to(torch.bfloat16))
    dy = _cl(torch.randn(2, 64, 28, 28, device=_cuda()).to(torch.bfloat16))
    names = _record_launches(monkeypatch)
    conv_gemm.conv_wgrad_kernel(dy, x, (64, 64, 3, 3), 1, 1)
    assert names == ["conv_wgrad3x3"]


@gpu
@pytest.mark.parametrize("case,text", list(zip(UNSUPPORTED, [
    "stride must be 1", "R and S must be 3", "multiples of 64"])))
def test_export_refuses_unsupported(case, text):
    from ddlw_amd.ops.runtime import KernelLibError

    H, C, K, R, st, pad = case
    Ho = (H + 2 * pad - R) // st + 1
    x = _cl(torch.zeros(2, C, H, H, device=_cuda(), dtype=torch.bfloat16))
    dy = _cl(torch.zeros(2, K, Ho, Ho, device=_cuda(), dtype=torch.bfloat16))
    with pytest.raises(KernelLibError, match=text):
        conv_gemm.conv_wgrad3x3_kernel(dy, x, (K, C, R, R), st, pad)
