"""Trainable MobileNetV2 stem from uint8: the stem forward with BN statistics
from its epilogue (``k_stem3_u8<true>``), the weight gradient from the bytes
(``k_stem3_u8_wgrad``), the stage Function ``_StemU8BnActFn``
(``ops/mbconv.py``), its gate, the opt-in mark and the model wiring.

Bounds. Sums of exact bf16 values (or of exact bf16 x bf16 products) in fp32
over M terms in any order are within ``(M - 1) * 2^-24 * sum|terms|`` of the
exact sum; the tests use ``M * 2^-24`` for plain sums and, as for the squares
in ``tests/test_pw_train.py``, ``M * 2^-23`` where the terms are products
summed by FMA chains in several stages. Comparisons of two bf16 pipelines use
the project's ``err(new) <= 2 * err(yardstick) + 1e-3`` in relative L2.

``(4, 128, 128)`` is M = 16384 output pixels: 128 forward partial rows, and 64
weight-gradient blocks that each loop over four 64-pixel groups.
"""
import copy
import functools
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from ddlw_amd.models import build_resnet50
from ddlw_amd.models.mobilenet_v2 import MobileNetV2, build_model
from ddlw_amd.ops import abi, mbconv
from ddlw_amd.ops.precision import apply_bf16_policy

ENV_SWITCHES = ("DDLW_DISABLE_HIP_OPS", "DDLW_EVAL_FOLD", "DDLW_CONV", "DDLW_STEM_U8",
                "DDLW_STEM_U8_TRAIN", "DDLW_PW_TRAIN")
NEW_FUNCTIONS = ("stem3_u8_fwd_stats", "stem3_u8_wgrad")
COUNTED = NEW_FUNCTIONS + ("stem3_u8_fwd_ep", "normalize_u8")

SHAPES = [(1, 2, 2), (2, 7, 9), (3, 16, 16), (2, 15, 17), (2, 33, 18), (2, 5, 130),
          (1, 64, 64), (4, 128, 128)]
_ids = lambda s: "n%d_h%d_w%d" % s  # noqa: E731


def _dev():
    return torch.device("cuda:0")


def _clear_env(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _nchw(u8_nhwc):
    """The model's input contract: N x C x H x W over NHWC memory."""
    return u8_nhwc.permute(0, 3, 1, 2)


def _out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def _rel_l2(y, ref):
    y, ref = y.detach().double().cpu(), ref.detach().double().cpu()
    return ((y - ref).norm() / (ref.norm() + 1e-30)).item()


def _assert_two_pipelines(new, parent, ref, what):
    e_n, e_p = _rel_l2(new, ref), _rel_l2(parent, ref)
    print(f"{what}: err_new {e_n:.4e}  err_parent {e_p:.4e}")
    assert torch.isfinite(new.float()).all(), what
    assert e_n <= 2 * e_p + 1e-3, (what, e_n, e_p)


def _count_calls(monkeypatch, names=COUNTED):
    from ddlw_amd.ops import binding

    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(binding, n)

        def counted(*a, _real=real, _n=n, **k):
            calls[_n] += 1
            return _real(*a, **k)

        monkeypatch.setattr(binding, n, counted)
    return calls


@functools.lru_cache(maxsize=None)
def _case(shape):
    """CPU inputs of one shape (never modified): the uint8 batch N x H x W x 3,
    a bf16 weight, a bf16 output gradient N x Ho x Wo x 32."""
    N, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(1000 * N + 37 * H + W)
    u8 = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
    w = torch.randn(32, 3, 3, 3, generator=g).to(torch.bfloat16)
    Ho, Wo = _out_hw(H, W)
    dy = torch.randn(N, Ho, Wo, 32, generator=g).to(torch.bfloat16)
    return u8, w, dy


def _xn_dev(u8_nhwc_dev):
    """``normalize_u8_bf16`` of a uint8 N x H x W x 3 device batch as bf16
    N x 3 x H x W (channels_last). Its kernel takes multiples of 16 bytes and
    it computes other sizes in bf16 torch arithmetic, which rounds differently;
    the value the stem kernels are specified to is the kernel's,
    bf16(float(u8) * (1/127.5f) - 1), so the bytes go through it zero-padded
    to a multiple of 16 (``tests/test_stem_u8.py`` holds the forward kernel to
    the same value bit for bit)."""
    from ddlw_amd.ops.layers import normalize_u8_bf16

    flat = u8_nhwc_dev.reshape(-1)
    padded = torch.zeros(-(-flat.numel() // 16) * 16, dtype=torch.uint8, device=flat.device)
    padded[: flat.numel()] = flat
    xn = normalize_u8_bf16(padded)[: flat.numel()].view(u8_nhwc_dev.shape)
    return _nchw(xn)


def _wgrad_ref(xn64, dy64_nchw):
    return torch.nn.grad.conv2d_weight(xn64, (32, 3, 3, 3), dy64_nchw, stride=2, padding=1)


# --------------------------------------------------------------------------- #
# 1-3. forward with statistics
# --------------------------------------------------------------------------- #


def _raw_fwd_stats(x, wp, y, ps, pq, nparts):
    from ddlw_amd.ops.runtime import launch

    n, c, h, w = x.shape
    launch("stem3_u8_fwd_stats", x, wp, y, ps, pq, nparts, n, h, w, c, wp.shape[0])


def _stat_errors(mean, rstd, rm, rv, ref):
    mean64, vare64, rm64, rv64 = ref
    std = vare64.sqrt()
    return {
        "mean": ((mean.double() - mean64).abs() / std).max().item(),
        "rstd": ((1.0 / rstd.double() - std).abs() / std).max().item(),
        "running_mean": ((rm.double() - rm64).abs() / std).max().item(),
        "running_var": ((rv.double() - rv64).abs() / vare64).max().item(),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_fwd_stats(shape):
    """y is the plain kernel's, bit for bit; the partials are the fp32 sums of
    the bf16 y and finalize as well as ``bn_stats`` of y does; and the kernel
    writes nothing but y and its ``nparts`` partial rows."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import query

    N, H, W = shape
    Ho, Wo = _out_hw(H, W)
    M = N * Ho * Wo
    dev = _dev()
    u8, w, _ = _case(shape)
    x, w = _nchw(u8.to(dev)), w.to(dev)

    nparts_q = int(query("stem3_u8_nparts", M, None))
    assert nparts_q == -(-M // 128)
    y, ps, pq, nparts = binding.stem3_u8_fwd_stats(x, w)
    assert nparts == nparts_q and ps.shape == pq.shape == (nparts, 32)
    assert ps.dtype == pq.dtype == torch.float32
    assert y.shape == (N, 32, Ho, Wo) and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    plain = binding.stem3_u8_fwd_ep(x, w)
    assert torch.equal(y, plain)
    assert torch.isfinite(ps).all() and torch.isfinite(pq).all()

    # statistics: fp32 summation bounds against the fp64 sums of the bf16 y
    y64 = y.permute(0, 2, 3, 1).reshape(M, 32).double()
    e_s = (ps.double().sum(0) - y64.sum(0)).abs()
    e_q = (pq.double().sum(0) - (y64 * y64).sum(0)).abs()
    b_s = M * 2.0 ** -24 * y64.abs().sum(0)
    b_q = M * 2.0 ** -23 * (y64 * y64).sum(0)
    print(f"fwd_stats {shape}: sum err/bound {(e_s / b_s.clamp_min(1e-300)).max().item():.3e}  "
          f"sumsq err/bound {(e_q / b_q.clamp_min(1e-300)).max().item():.3e}")
    assert (e_s <= b_s).all() and (e_q <= b_q).all()

    g = torch.Generator(device="cpu").manual_seed(M)
    rm0 = torch.empty(32).uniform_(-0.3, 0.3, generator=g).to(dev)
    rv0 = torch.empty(32).uniform_(0.5, 1.5, generator=g).to(dev)
    eps, mom = 1e-5, 0.1
    rm_f, rv_f, rm_s, rv_s = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    mean_f, rstd_f = binding.bn_finalize_parts(ps, pq, nparts, M, 32, eps, mom, rm_f, rv_f)
    mean_s, rstd_s = binding.bn_stats(y, eps, mom, rm_s, rv_s)
    mean64 = y64.mean(0)
    var64 = ((y64 - mean64) ** 2).mean(0)
    ref = (mean64, var64 + eps, (1 - mom) * rm0.double() + mom * mean64,
           (1 - mom) * rv0.double() + mom * var64 * M / max(M - 1, 1))
    e_f = _stat_errors(mean_f, rstd_f, rm_f, rv_f, ref)
    e_y = _stat_errors(mean_s, rstd_s, rm_s, rv_s, ref)
    slack = M * 2.0 ** -24
    for name in e_f:
        print(f"fwd_stats {shape} {name}: err_fused {e_f[name]:.3e}  "
              f"err_standalone {e_y[name]:.3e}  slack {slack:.3e}")
    for name in e_f:
        assert e_f[name] <= 2 * e_y[name] + slack, (name, e_f[name], e_y[name])

    # canaries: y and the partials inside larger buffers
    PAD = 2
    wp = binding.stem3_pack_weight(w)
    ybuf = torch.full((M + 2 * PAD, 32), -77.0, dtype=torch.bfloat16, device=dev)
    pbuf = torch.full((2, nparts + 2 * PAD, 32), -1234.0, dtype=torch.float32, device=dev)
    y_before, p_before = ybuf.clone(), pbuf.clone()
    _raw_fwd_stats(x, wp, ybuf[PAD:PAD + M], pbuf[0, PAD:], pbuf[1, PAD:], nparts)
    assert torch.equal(ybuf[PAD:PAD + M].view(N, Ho, Wo, 32), y.permute(0, 2, 3, 1))
    assert torch.equal(ybuf[:PAD], y_before[:PAD])
    assert torch.equal(ybuf[PAD + M:], y_before[PAD + M:])
    assert torch.equal(pbuf[0, PAD:PAD + nparts], ps) and torch.equal(pbuf[1, PAD:PAD + nparts], pq)
    assert torch.equal(pbuf[:, :PAD], p_before[:, :PAD])
    assert torch.equal(pbuf[:, PAD + nparts:], p_before[:, PAD + nparts:])

    # determinism
    y2, ps2, pq2, _ = binding.stem3_u8_fwd_stats(x, w)
    assert torch.equal(y2, y) and torch.equal(ps2, ps) and torch.equal(pq2, pq)


# --------------------------------------------------------------------------- #
# 4-7. weight gradient
# --------------------------------------------------------------------------- #


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_wgrad_parity(shape):
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import query

    N, H, W = shape
    Ho, Wo = _out_hw(H, W)
    M = N * Ho * Wo
    dev = _dev()
    u8, w, dy = _case(shape)
    x = _nchw(u8.to(dev))
    dy_d = _nchw(dy.to(dev))
    assert dy_d.is_contiguous(memory_format=torch.channels_last)
    assert int(query("stem3_u8_wgrad_nparts", M, None)) == max(1, min(-(-M // 256), 256))

    dw = binding.stem3_u8_wgrad(x, dy_d, (32, 3, 3, 3))
    assert dw.shape == (32, 3, 3, 3) and dw.dtype == torch.float32 and dw.is_contiguous()
    assert torch.equal(dw, binding.stem3_u8_wgrad(x, dy_d, (32, 3, 3, 3)))  # determinism

    xn_d = _xn_dev(u8.to(dev))
    assert xn_d.is_contiguous(memory_format=torch.channels_last)
    xn64 = xn_d.cpu().double().contiguous()
    dy64 = _nchw(dy.double()).contiguous()
    ref = _wgrad_ref(xn64, dy64)
    bound = M * 2.0 ** -23 * _wgrad_ref(xn64.abs(), dy64.abs())
    err = (dw.cpu().double() - ref).abs()
    print(f"wgrad {shape}: max err/bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all()

    lib = torch.ops.aten.convolution_backward(
        dy_d, xn_d, w.to(dev), None, [2, 2], [1, 1], [1, 1], False, [0, 0], 1,
        [False, True, False])[1]
    e_k, e_l = _rel_l2(dw, ref), _rel_l2(lib, ref)
    print(f"wgrad {shape}: rel-L2 kernel {e_k:.3e}  library bf16 {e_l:.3e}")
    assert e_k <= 2 * e_l + 1e-3, (e_k, e_l)


# output pixels (n, ho, wo) of shape (2, 7, 9) -> Ho x Wo = 4 x 5: a corner, a
# top-edge pixel, a right-edge pixel (W = 9 is odd: column 2wo+1 = 9 is outside),
# an interior pixel, and the very last pixel M - 1 (bottom-right corner, H odd)
SINGLE_PIXELS = {"corner": (0, 0, 0), "top_edge": (0, 0, 2), "right_edge": (1, 1, 4),
                 "interior": (0, 2, 2), "last": (1, 3, 4)}


@pytest.mark.gpu
@pytest.mark.parametrize("where", list(SINGLE_PIXELS))
def test_wgrad_single_pixel_is_exact(where):
    """dy zero except at one output pixel: every dW element is one exact
    product (or exactly 0 where the tap lies outside the image)."""
    from ddlw_amd.ops import binding

    shape = (2, 7, 9)
    N, H, W = shape
    Ho, Wo = _out_hw(H, W)
    n, ho, wo = SINGLE_PIXELS[where]
    if where == "last":
        assert (n * Ho + ho) * Wo + wo == N * Ho * Wo - 1
    u8, _, dy_full = _case(shape)
    dy = torch.zeros_like(dy_full)
    dy[n, ho, wo] = dy_full[n, ho, wo]
    assert dy[n, ho, wo].float().abs().min().item() > 0
    dev = _dev()
    xn = _xn_dev(u8.to(dev)).cpu().float()      # exact: bf16 values
    expect = torch.zeros(32, 3, 3, 3)
    outside = 0
    for r in range(3):
        for s in range(3):
            hh, ww = 2 * ho - 1 + r, 2 * wo - 1 + s
            if 0 <= hh < H and 0 <= ww < W:
                # fp32 product of two bf16 values: exact
                expect[:, :, r, s] = dy[n, ho, wo].float().view(32, 1) * xn[n, :, hh, ww].view(1, 3)
            else:
                outside += 1
    assert outside == {"corner": 5, "top_edge": 3, "right_edge": 3, "interior": 0,
                       "last": 5}[where]
    dw = binding.stem3_u8_wgrad(_nchw(u8.to(dev)), _nchw(dy.to(dev)), (32, 3, 3, 3))
    assert torch.equal(dw.cpu(), expect), (dw.cpu() - expect).abs().max()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 6])
def test_wgrad_padding_is_zero_in_normalized_space(size):
    """x all byte 0 (normalized: exactly -1), dy all ones: dW[k][c][r][s] is
    minus the number of output pixels whose tap (r, s) is inside the image.
    Padding in byte space would count every output pixel."""
    from ddlw_amd.ops import binding

    dev = _dev()
    Ho, Wo = _out_hw(size, size)
    counts = torch.zeros(3, 3)
    for r in range(3):
        for s in range(3):
            counts[r, s] = sum(1 for ho in range(Ho) for wo in range(Wo)
                               if 0 <= 2 * ho - 1 + r < size and 0 <= 2 * wo - 1 + s < size)
    assert counts.min().item() < Ho * Wo == counts[1, 1].item()
    u8 = torch.zeros(1, size, size, 3, dtype=torch.uint8, device=dev)
    dy = torch.ones(1, Ho, Wo, 32, dtype=torch.bfloat16, device=dev)
    dw = binding.stem3_u8_wgrad(_nchw(u8), _nchw(dy), (32, 3, 3, 3))
    assert torch.equal(dw.cpu(), (-counts).expand(32, 3, 3, 3)), dw.cpu()[0, 0]


# --------------------------------------------------------------------------- #
# 8. rejections
# --------------------------------------------------------------------------- #


@pytest.mark.gpu
def test_bad_arguments_are_refused():
    """The library refuses with its ``who: why`` text and status 2, which it
    returns before any launch."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import KernelLibError, launch

    dev = _dev()

    def u8(c):
        return _nchw(torch.zeros(1, 4, 4, c, dtype=torch.uint8, device=dev))

    def dyt(k):
        return _nchw(torch.zeros(1, 2, 2, k, dtype=torch.bfloat16, device=dev))

    def wt(k, c):
        return torch.zeros(k, c, 3, 3, dtype=torch.bfloat16, device=dev)

    for args in ((u8(4), wt(32, 4)), (u8(3), wt(24, 3))):
        with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_fwd_stats: ") as e:
            binding.stem3_u8_fwd_stats(*args)
        assert "C=3, K=32" in str(e.value)
    for args in ((u8(4), dyt(32), (32, 4, 3, 3)), (u8(3), dyt(24), (24, 3, 3, 3))):
        with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_wgrad: ") as e:
            binding.stem3_u8_wgrad(*args)
        assert "C=3, K=32" in str(e.value)

    x, wp = u8(3), binding.stem3_pack_weight(wt(32, 3))
    y = torch.zeros(4, 32, dtype=torch.bfloat16, device=dev)
    parts = torch.zeros(2, 1, 32, device=dev)
    part = torch.zeros(1, 32, 27, device=dev)
    dw = torch.zeros(32, 3, 3, 3, device=dev)
    # a bf16 [1,32,2,2] channels_last view that starts 2 bytes into its buffer
    buf = torch.zeros(4 * 32 + 8, dtype=torch.bfloat16, device=dev)
    dy_off = _nchw(buf[1:1 + 4 * 32].view(1, 2, 2, 32))
    assert dy_off.is_contiguous(memory_format=torch.channels_last) and dy_off.data_ptr() % 16 == 2
    with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_wgrad: dy must be 16-byte"):
        binding.stem3_u8_wgrad(x, dy_off, (32, 3, 3, 3))
    for ps, pq in ((None, parts[1]), (parts[0], None)):
        with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_fwd_stats: psum and psq"):
            launch("stem3_u8_fwd_stats", x, wp, y, ps, pq, 1, 1, 4, 4, 3, 32)
    with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_wgrad: part and dw"):
        launch("stem3_u8_wgrad", x, dyt(32), None, dw, 1, 1, 4, 4, 3, 32)
    for bad in (0, 2):
        with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_fwd_stats: nparts"):
            launch("stem3_u8_fwd_stats", x, wp, y, parts[0], parts[1], bad, 1, 4, 4, 3, 32)
        with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_wgrad: nparts"):
            launch("stem3_u8_wgrad", x, dyt(32), part, dw, bad, 1, 4, 4, 3, 32)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# 9. stage Function
# --------------------------------------------------------------------------- #


def _stage_setup():
    """fp32 stem conv + BN (CPU), gamma in [0.5, 1.5], beta in [-0.2, 0.2]. With
    such an affine the pre-activation is ~N(0, 1) per channel and nothing of a
    uniformly random image would reach 6, so the image is mostly low contrast
    (bytes 126..130) with one full-range row: the batch statistics are
    dominated by the quiet part and the full-range row's outputs lie many batch
    standard deviations out, on both sides."""
    g = torch.Generator(device="cpu").manual_seed(77)
    N, H, W = 2, 33, 16                         # 16 | N*H*W*3: k_normalize_u8 takes it
    u8 = torch.randint(126, 131, (N, H, W, 3), dtype=torch.uint8, generator=g)
    u8[:, :1] = torch.randint(0, 256, (N, 1, W, 3), dtype=torch.uint8, generator=g)
    net = MobileNetV2()
    conv, bn = net.features[0], net.features[1]
    with torch.no_grad():
        conv.weight.copy_(torch.randn(32, 3, 3, 3, generator=g).to(torch.bfloat16).float())
        bn.weight.copy_(torch.empty(32).uniform_(0.5, 1.5, generator=g))
        bn.bias.copy_(torch.empty(32).uniform_(-0.2, 0.2, generator=g))
        bn.running_mean.copy_(torch.empty(32).uniform_(-0.3, 0.3, generator=g))
        bn.running_var.copy_(torch.empty(32).uniform_(0.5, 1.5, generator=g))
    Ho, Wo = _out_hw(H, W)
    gout = torch.randn(N, 32, Ho, Wo, generator=g).to(torch.bfloat16).float()
    return net.train(), u8, gout


def _stage_preact(net, u8):
    conv, bn = net.features[0], net.features[1]
    with torch.no_grad():
        x = _nchw(u8).float() / 127.5 - 1
        return F.batch_norm(F.conv2d(x, conv.weight, stride=2, padding=1), None, None,
                            bn.weight, bn.bias, True, 0.0, bn.eps)


def _assert_all_regions(pre, what):
    """The fp32 ReLU6 pre-activation has elements below 0, inside and above 6
    (at least 0.2% of them in the thinnest region, so a handful stays on each
    side under bf16 rounding)."""
    n = pre.numel()
    for name, cnt in (("<0", (pre < 0).sum()), ("(0,6)", ((pre > 0) & (pre < 6)).sum()),
                      (">6", (pre > 6).sum())):
        share = cnt.item() / n
        print(f"{what} region {name}: {share:.4f}")
        assert share >= 0.002, (what, name, share)


def test_stage_seed_covers_relu6_regions():
    net, u8, _ = _stage_setup()
    _assert_all_regions(_stage_preact(net, u8), "stem stage")


def _stage_run(net, x, gout, fused):
    conv, bn = net.features[0], net.features[1]
    if fused:
        assert mbconv.stem_u8_train_fusable(net, x)
        y = mbconv.stem_u8_train_forward(net, x)
    else:
        y = bn(conv(mbconv.normalize_u8_input(x, conv.weight)))
    (y.float() * gout.float()).sum().backward()
    torch.cuda.synchronize()
    return {"y": y.detach(), "dW": conv.weight.grad, "dgamma": bn.weight.grad,
            "dbeta": bn.bias.grad, "running_mean": bn.running_mean.detach().clone(),
            "running_var": bn.running_var.detach().clone(),
            "num_batches_tracked": int(bn.num_batches_tracked)}


@pytest.mark.gpu
def test_stage_function_vs_parent_path(monkeypatch):
    """normalize + stem conv + BatchNormAct2d(relu6), one step, three ways:
    fp32 stock ops, bf16 unmarked (the parent path) and bf16 on the stage
    Function."""
    _clear_env(monkeypatch)
    net, u8, gout = _stage_setup()
    _assert_all_regions(_stage_preact(net, u8), "stem stage")
    dev = _dev()
    x, gout = _nchw(u8.to(dev)), gout.to(dev).contiguous(memory_format=torch.channels_last)
    net32 = net.to(dev)
    netb = copy.deepcopy(net32).to(memory_format=torch.channels_last)
    netb.features[0].to(torch.bfloat16)
    netn = copy.deepcopy(netb)
    netn.enable_u8_train_stem()

    monkeypatch.setenv("DDLW_DISABLE_HIP_OPS", "1")
    ref = _stage_run(net32, x, gout, fused=False)
    monkeypatch.delenv("DDLW_DISABLE_HIP_OPS")

    calls = _count_calls(monkeypatch)
    assert not mbconv.stem_u8_train_fusable(netb, x)
    parent = _stage_run(netb, x, gout.to(torch.bfloat16), fused=False)
    assert calls["normalize_u8"] == 1 and not any(calls[n] for n in NEW_FUNCTIONS), calls
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    new = _stage_run(netn, x, gout.to(torch.bfloat16), fused=True)
    assert calls["stem3_u8_fwd_stats"] == 1 and calls["stem3_u8_wgrad"] == 1, calls
    assert calls["normalize_u8"] == 1, calls

    for name in ("y", "dW", "dgamma", "dbeta", "running_mean", "running_var"):
        assert new[name].shape == ref[name].shape, name
        _assert_two_pipelines(new[name], parent[name], ref[name], f"stem stage {name}")
    assert new["dW"].dtype == torch.bfloat16
    assert new["num_batches_tracked"] == parent["num_batches_tracked"] == 1
    assert new["y"].max().item() == 6.0 and new["y"].min().item() == 0.0


# --------------------------------------------------------------------------- #
# 10-11. model and facade
# --------------------------------------------------------------------------- #


def _randomize_bn(module, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for mod in module.modules():
            if isinstance(getattr(mod, "running_mean", None), torch.Tensor):
                for t, lo, hi in ((mod.running_mean, -0.3, 0.3), (mod.running_var, 0.5, 1.5),
                                  (mod.weight, 0.5, 1.5), (mod.bias, -0.2, 0.2)):
                    t.copy_(torch.empty_like(t, device="cpu").uniform_(lo, hi, generator=g))


def _to_bf16_convs(m):
    m = copy.deepcopy(m).to(memory_format=torch.channels_last)
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
            mod.to(torch.bfloat16)
    return m


def _u8_batch(seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 256, (8, 64, 64, 3), dtype=torch.uint8, generator=g)


def _fp32_model(**kw):
    torch.manual_seed(31)
    model = build_model(64, 64, 3, 5, dropout=0.0, **kw)
    _randomize_bn(model, seed=9)
    return model


def _bf16_model(dev, marked, **kw):
    m = _to_bf16_convs(_fp32_model(**kw).to(dev))
    if marked:
        m.base.base.enable_u8_train_stem()
    return m


def _step(m, u8, labels):
    from ddlw_amd.ops.layers import softmax_cross_entropy

    logits = m(u8)
    softmax_cross_entropy(logits, labels).backward()
    torch.cuda.synchronize()
    return logits.detach()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1])
def test_marked_model_trains_its_stem_from_uint8(k, monkeypatch):
    _clear_env(monkeypatch)
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    dev = _dev()
    u8 = _nchw(_u8_batch().to(dev))
    labels = torch.randint(0, 5, (8,), device=dev)
    m = _bf16_model(dev, True, fine_tune_at=k).train()
    calls = _count_calls(monkeypatch)
    _step(m, u8, labels)
    assert calls == {"stem3_u8_fwd_stats": 1, "stem3_u8_wgrad": 1 - k, "stem3_u8_fwd_ep": 0,
                     "normalize_u8": 0}, calls
    trainable = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert any(n.startswith("base.base.features.1.") for n, _ in trainable)
    for n, p in trainable:
        assert p.grad is not None and torch.isfinite(p.grad.float()).all(), (k, n)
    stem_w = m.base.base.features[0].weight
    if k == 0:
        assert stem_w.grad.dtype == torch.bfloat16
        assert stem_w.grad.float().abs().max().item() > 0
    else:
        assert not stem_w.requires_grad and stem_w.grad is None
    assert int(m.base.base.features[1].num_batches_tracked) == 1


@pytest.mark.gpu
def test_marked_model_evaluates_on_the_fused_frozen_stem(monkeypatch):
    _clear_env(monkeypatch)
    dev = _dev()
    u8 = _nchw(_u8_batch().to(dev))
    marked = _bf16_model(dev, True, fine_tune_at=0).eval()
    plain = _bf16_model(dev, False, fine_tune_at=0).eval()
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        logits = marked(u8)
        assert calls["stem3_u8_fwd_ep"] == 1 and calls["normalize_u8"] == 0, calls
        assert not any(calls[n] for n in NEW_FUNCTIONS), calls
        ref = plain(u8)
        assert calls["stem3_u8_fwd_ep"] == 1 and calls["normalize_u8"] == 1, calls
    # another kernel sequence (fused stem vs normalize + conv + bn_apply)
    rel = ((logits.float() - ref.float()).abs().max() / ref.float().abs().max()).item()
    print(f"marked eval from uint8, logits: rel {rel:.4e}")
    assert rel <= 5e-2, rel


@pytest.mark.gpu
def test_switch_off_and_unmarked_stay_on_the_parent_path(monkeypatch):
    _clear_env(monkeypatch)
    dev = _dev()
    u8 = _nchw(_u8_batch().to(dev))
    labels = torch.randint(0, 5, (8,), device=dev)
    calls = _count_calls(monkeypatch)
    plain = _bf16_model(dev, False, fine_tune_at=0).train()
    logits_plain = _step(plain, u8, labels)
    assert calls == {"stem3_u8_fwd_stats": 0, "stem3_u8_wgrad": 0, "stem3_u8_fwd_ep": 0,
                     "normalize_u8": 1}, calls
    # the switch does not matter to an unmarked model
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    _step(_bf16_model(dev, False, fine_tune_at=0).train(), u8, labels)
    assert calls["normalize_u8"] == 2 and not any(calls[n] for n in NEW_FUNCTIONS), calls
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "0")
    for n in calls:
        calls[n] = 0
    off = _bf16_model(dev, True, fine_tune_at=0).train()
    logits_off = _step(off, u8, labels)
    assert calls == {"stem3_u8_fwd_stats": 0, "stem3_u8_wgrad": 0, "stem3_u8_fwd_ep": 0,
                     "normalize_u8": 1}, calls
    assert torch.equal(logits_off, logits_plain)


@pytest.mark.gpu
def test_marked_gradients_against_fp32(monkeypatch):
    """One step at fine_tune_at=0, marked vs unmarked bf16 against the fp32
    model (CPU, stock ops) on the same weights and bytes."""
    _clear_env(monkeypatch)
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    dev = _dev()
    u8_cpu = _nchw(_u8_batch())
    labels_cpu = torch.randint(0, 5, (8,), generator=torch.Generator().manual_seed(3))
    ref = _fp32_model(fine_tune_at=0).train()
    F.cross_entropy(ref(u8_cpu), labels_cpu).backward()
    u8, labels = _nchw(_u8_batch().to(dev)), labels_cpu.to(dev)
    marked = _bf16_model(dev, True, fine_tune_at=0).train()
    plain = _bf16_model(dev, False, fine_tune_at=0).train()
    calls = _count_calls(monkeypatch)
    _step(marked, u8, labels)
    assert calls["stem3_u8_wgrad"] == 1 and calls["normalize_u8"] == 0, calls
    _step(plain, u8, labels)
    assert calls["stem3_u8_wgrad"] == 1 and calls["normalize_u8"] == 1, calls
    grads = lambda m: dict(m.named_parameters())  # noqa: E731
    for name in ("classifier.weight", "classifier.bias", "base.base.features.0.weight",
                 "base.base.features.1.weight", "base.base.features.1.bias"):
        _assert_two_pipelines(grads(marked)[name].grad, grads(plain)[name].grad,
                              grads(ref)[name].grad, f"model grad {name}")


@pytest.mark.gpu
def test_facade_takes_the_new_route(monkeypatch):
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    dev = _dev()
    torch.manual_seed(6)
    model = Model(build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=0), dev,
                  precision="bf16").compile("adam")
    stem = model.module.base.base.features[0]
    assert stem.u8_train
    before = stem.weight.detach().clone()
    u8 = _u8_batch().to(dev)                     # N x H x W x C, as the loader yields it
    labels = torch.randint(0, 5, (8,), device=dev)
    calls = _count_calls(monkeypatch)
    logs = model.train_step(u8, labels)
    assert calls == {"stem3_u8_fwd_stats": 1, "stem3_u8_wgrad": 1, "stem3_u8_fwd_ep": 0,
                     "normalize_u8": 0}, calls
    assert logs["loss"] == logs["loss"] and abs(logs["loss"]) < float("inf"), logs
    assert not torch.equal(stem.weight.detach(), before)
    # validation during fit: the fused frozen stem
    model.eval_step(u8, labels)
    assert calls["stem3_u8_fwd_ep"] == 1 and calls["normalize_u8"] == 0, calls


def _fresh_stem_reference(m, u8, train):
    """What the stem of ``m`` has to give on ``u8`` from its LIVE tensors,
    with nothing cached: the bindings called directly on a weight packed now
    and (eval) a BN fold computed now."""
    from ddlw_amd.ops import binding

    conv, bn = m.base.base.features[0], m.base.base.features[1]
    with torch.no_grad():
        wp = binding.stem3_pack_weight(conv.weight)
        if train:
            return binding.stem3_u8_fwd_stats(u8, conv.weight, wp=wp)[0]
        scale = bn.weight.float() * (bn.running_var.float() + bn.eps).rsqrt()
        bias = bn.bias.float() - bn.running_mean.float() * scale
        return binding.stem3_u8_fwd_ep(u8, conv.weight, scale.contiguous(),
                                       bias.contiguous(), 2, wp=wp)


def _capture(monkeypatch, name):
    """Record what ``binding.<name>`` returns (first element of a tuple)."""
    from ddlw_amd.ops import binding

    real = getattr(binding, name)
    seen = []

    def wrapped(*a, **k):
        out = real(*a, **k)
        seen.append((out[0] if isinstance(out, tuple) else out).detach().clone())
        return out

    monkeypatch.setattr(binding, name, wrapped)
    return seen


@pytest.mark.gpu
def test_second_step_sees_the_updated_stem_weight(monkeypatch):
    """Two FusedAdam steps through the facade: the optimizer kernel writes the
    bf16 stem weight through a raw pointer (no ``_version`` bump), and the
    second training forward must convolve with THAT weight."""
    from ddlw_amd.ops import binding
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    dev = _dev()
    torch.manual_seed(6)
    model = Model(build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=0), dev,
                  precision="bf16").compile("adam", learning_rate=1e-2)
    m = model.module
    stem = m.base.base.features[0]
    u8 = _u8_batch().to(dev)
    x = _nchw(u8)
    labels = torch.randint(0, 5, (8,), device=dev)
    w0 = stem.weight.detach().clone()
    wp0 = binding.stem3_pack_weight(w0)
    seen = _capture(monkeypatch, "stem3_u8_fwd_stats")
    model.train_step(u8, labels)
    assert len(seen) == 1
    assert torch.equal(seen[0], binding.stem3_u8_fwd_stats(x, w0, wp=wp0)[0])
    w1 = stem.weight.detach().clone()
    assert not torch.equal(w1, w0)
    expect = _fresh_stem_reference(m, x, train=True)
    stale = binding.stem3_u8_fwd_stats(x, w0, wp=wp0)[0]
    assert not torch.equal(expect, stale)
    del seen[:]
    model.train_step(u8, labels)
    assert len(seen) == 1
    assert torch.equal(seen[0], expect)
    assert not torch.equal(stem.weight.detach(), w1)


@pytest.mark.gpu
def test_validation_between_steps_sees_the_live_stem(monkeypatch):
    """train step -> eval -> train step -> eval on a marked trainable stem:
    each eval's fused stem equals the kernel on the weight, BN affine and
    running statistics as they are then; the second differs from the first."""
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    dev = _dev()
    u8 = _u8_batch().to(dev)
    x = _nchw(u8)
    labels = torch.randint(0, 5, (8,), device=dev)
    for switch in ("1", "0"):                   # whichever way the stem trains
        monkeypatch.setenv("DDLW_STEM_U8_TRAIN", switch)
        torch.manual_seed(6)
        model = Model(build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=0), dev,
                      precision="bf16").compile("adam", learning_rate=1e-2)
        m = model.module
        seen = _capture(monkeypatch, "stem3_u8_fwd_ep")
        outs = []
        for _ in range(2):
            model.train_step(u8, labels)
            del seen[:]
            model.eval_step(u8, labels)
            assert len(seen) == 1, switch
            m.eval()
            expect = _fresh_stem_reference(m, x, train=False)
            assert torch.equal(seen[0], expect), switch
            outs.append(seen[0])
        assert not torch.equal(outs[0], outs[1]), switch
        monkeypatch.undo()
        _clear_env(monkeypatch)


# --------------------------------------------------------------------------- #
# 12-15. CPU: the gate, the mark and the policy, CPU numerics, ABI rows
# --------------------------------------------------------------------------- #


class _FakeCudaU8:
    """Stands in for a CUDA uint8 channels_last batch so the gate's other
    conditions can be checked without a GPU."""
    is_cuda = True
    dtype = torch.uint8

    def __init__(self, channels_last=True):
        self._cl = channels_last

    def dim(self):
        return 4

    def is_contiguous(self, memory_format=torch.contiguous_format):
        return self._cl == (memory_format == torch.channels_last)


def _cpu_u8(channels=3, seed=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return _nchw(torch.randint(0, 256, (2, 64, 64, channels), dtype=torch.uint8,
                               generator=g))


def _marked_bf16_net(channels=3, mark=True):
    net = MobileNetV2(channels).train()
    for mod in net.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.to(torch.bfloat16)
    net.enable_u8_train_stem(mark)
    return net


def test_train_gate(monkeypatch):
    _clear_env(monkeypatch)
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    fake = _FakeCudaU8()
    net = _marked_bf16_net()
    assert mbconv.stem_u8_train_fusable(net, fake)
    assert not mbconv.stem_u8_train_fusable(_marked_bf16_net(mark=False), fake)  # unmarked
    net.enable_u8_train_stem(False)
    assert not mbconv.stem_u8_train_fusable(net, fake)
    net.enable_u8_train_stem()
    with torch.no_grad():
        assert not mbconv.stem_u8_train_fusable(net, fake)
    net.features[1].eval()
    assert not mbconv.stem_u8_train_fusable(net, fake)  # BN on running statistics
    net.features[1].train()
    net.features[0].eval()                              # a frozen conv under a live BN
    assert mbconv.stem_u8_train_fusable(net, fake)
    stem_params = [net.features[0].weight, net.features[1].weight, net.features[1].bias]
    for p in stem_params:
        p.requires_grad = False
    assert not mbconv.stem_u8_train_fusable(net, fake)  # nothing wants a gradient
    for p in stem_params:
        p.requires_grad = True
        assert mbconv.stem_u8_train_fusable(net, fake)
        p.requires_grad = False
    for p in stem_params:
        p.requires_grad = True
    assert not mbconv.stem_u8_train_fusable(net, _FakeCudaU8(channels_last=False))
    assert not mbconv.stem_u8_train_fusable(net, _cpu_u8())  # a real CPU batch
    assert not mbconv.stem_u8_train_fusable(_marked_bf16_net(channels=1), fake)
    fp32 = MobileNetV2().train()
    fp32.enable_u8_train_stem()
    assert not mbconv.stem_u8_train_fusable(fp32, fake)  # fp32 weights
    bn = net.features[1]
    bn.running_mean = bn.running_mean.to(torch.bfloat16)
    assert not mbconv.stem_u8_train_fusable(net, fake)
    bn.running_mean = bn.running_mean.float()
    assert mbconv.stem_u8_train_fusable(net, fake)
    for name, value in (("DDLW_DISABLE_HIP_OPS", "1"), ("DDLW_CONV", "stock"),
                        ("DDLW_STEM_U8_TRAIN", "0")):
        monkeypatch.setenv(name, value)
        assert not mbconv.stem_u8_train_fusable(net, fake), name
        monkeypatch.setenv(name, "1" if name == "DDLW_STEM_U8_TRAIN" else "0")
        assert mbconv.stem_u8_train_fusable(net, fake), name
    # the frozen stem's switches do not govern the training stem
    monkeypatch.setenv("DDLW_STEM_U8", "0")
    monkeypatch.setenv("DDLW_EVAL_FOLD", "0")
    assert mbconv.stem_u8_train_fusable(net, fake)


def test_mark_and_policy(tmp_path):
    from ddlw_amd.core.model_io import load_model, save_model

    plain = build_model()
    assert plain.base.base.features[0].u8_train is False
    keys = list(plain.state_dict())
    model = apply_bf16_policy(build_model())
    stem = model.base.base.features[0]
    assert stem.u8_train is True and "u8_train" in vars(stem)
    assert [m for m in model.modules() if getattr(m, "u8_train", False)] == [stem]
    params = [id(p) for p in model.parameters()]
    dtypes = [p.dtype for p in model.parameters()]
    again = apply_bf16_policy(model)
    assert again is model and stem.u8_train is True
    assert [id(p) for p in model.parameters()] == params
    assert [p.dtype for p in model.parameters()] == dtypes
    assert copy.deepcopy(model).base.base.features[0].u8_train is True
    assert list(model.state_dict()) == keys
    assert not [k for k in keys if "u8" in k]
    save_model(model, tmp_path / "m")
    loaded = load_model(str(tmp_path / "m"))
    assert loaded.base.base.features[0].u8_train is False
    assert list(loaded.state_dict()) == keys
    model.base.base.enable_u8_train_stem(False)
    assert stem.u8_train is False
    # a model without the method passes through the policy unchanged
    resnet = build_resnet50()
    assert not [m for m in resnet.modules() if hasattr(m, "enable_u8_train_stem")]
    apply_bf16_policy(resnet)
    assert not [m for m in resnet.modules() if "u8_train" in vars(m)]


@pytest.mark.parametrize("k", [0, 1, 13])
def test_cpu_marked_model_equals_normalized(k, monkeypatch):
    _clear_env(monkeypatch)
    monkeypatch.setenv("DDLW_STEM_U8_TRAIN", "1")
    torch.manual_seed(4)
    net = build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=k).train()
    net.base.base.enable_u8_train_stem()
    _randomize_bn(net, seed=3)
    u8 = _cpu_u8()
    twin = copy.deepcopy(net)                    # the step updates BN buffers
    y = net(u8)
    ref = twin(u8.float() / 127.5 - 1)
    assert y.dtype == torch.float32 and torch.isfinite(y).all()
    assert torch.equal(y, ref)


def test_abi_rows_for_the_new_exports():
    P, I, L = abi.Ptr, abi.c_int, abi.c_long
    # x, wp, y, psum, psq, nparts, N, H, W, C, K, stream
    assert abi.SIGNATURES["ddlw_stem3_u8_fwd_stats"] == (I, [P] * 5 + [I] * 6 + [P])
    # x, dy, part, dw, nparts, N, H, W, C, K, stream
    assert abi.SIGNATURES["ddlw_stem3_u8_wgrad"] == (I, [P] * 4 + [I] * 6 + [P])
    for name in ("ddlw_stem3_u8_nparts", "ddlw_stem3_u8_wgrad_nparts"):
        assert abi.SIGNATURES[name] == (I, [L, P])   # M, stream
    src = (Path(abi.__file__).resolve().parent / "hip" / "conv_stem.hip").read_text()
    for name in ("ddlw_stem3_u8_nparts", "ddlw_stem3_u8_fwd_stats",
                 "ddlw_stem3_u8_wgrad_nparts", "ddlw_stem3_u8_wgrad"):
        m = re.search(r"DDLW_EXPORT\s+int\s+" + name + r"\s*\(([^)]*)\)", src)
        assert m and re.search(r"void\s*\*\s*stream\s*$", m.group(1)), name
