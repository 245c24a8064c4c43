"""GPU tests for the native dgrad weight layouts (``hip/weights.hip``,
``DDLW_DGRAD_WPACK``): the packed bytes equal the torch expressions they
replace, bad channel counts are refused, and the dgrads and a whole
bottleneck block compute the same bits with the levers on and off."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _cuda():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rand(*shape, scale=1.0):
    return _cl((torch.randn(*shape, device=_cuda()) * scale).to(torch.bfloat16))


def _image(t):
    """Flat memory image of a channels_last 4-D tensor."""
    assert t.is_contiguous(memory_format=torch.channels_last)
    return t.permute(0, 2, 3, 1).reshape(-1)


# tiles smaller than the 64x64 LDS tile, and not multiples of it
@pytest.mark.parametrize("shape", [(8, 16, 1, 1), (16, 8, 3, 3),
                                   (64, 24, 3, 3), (136, 72, 1, 1)])
def test_wpack_bytes_equal_torch(monkeypatch, shape):
    from ddlw_amd.ops import conv_gemm

    monkeypatch.delenv("DDLW_DGRAD_WPACK", raising=False)
    torch.manual_seed(3)
    w = _rand(*shape)
    ref = conv_gemm.dgrad_weight_torch(w)
    got = conv_gemm.dgrad_weight(w)
    assert got.data_ptr() != ref.data_ptr()
    assert got.shape == ref.shape and got.dtype == ref.dtype
    assert torch.equal(_image(got), _image(ref))
    monkeypatch.setenv("DDLW_DGRAD_WPACK", "0")  # the lever is read per call
    assert torch.equal(_image(conv_gemm.dgrad_weight(w)), _image(ref))


@pytest.mark.parametrize("kc", [(64, 8), (128, 72)])
def test_wpack_s2_bytes_equal_torch(monkeypatch, kc):
    from ddlw_amd.ops import conv_gemm

    monkeypatch.delenv("DDLW_DGRAD_WPACK", raising=False)
    torch.manual_seed(4)
    w = _rand(kc[0], kc[1], 3, 3)
    ref = conv_gemm.dgrad_s2_wcat_torch(w)
    got = conv_gemm.dgrad_s2_wcat(w)
    assert got.shape == ref.shape == (9 * kc[0] * kc[1],)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("kc", [(12, 16), (16, 12), (64, 4)])
def test_wpack_refuses_channels_not_multiple_of_8(monkeypatch, kc):
    from ddlw_amd.ops import conv_gemm
    from ddlw_amd.ops.runtime import KernelLibError

    monkeypatch.delenv("DDLW_DGRAD_WPACK", raising=False)
    with pytest.raises(KernelLibError, match="multiples of 8"):
        conv_gemm.dgrad_weight(_rand(kc[0], kc[1], 1, 1))
    with pytest.raises(KernelLibError, match="multiples of 8"):
        conv_gemm.dgrad_s2_wcat(_rand(kc[0], kc[1], 3, 3))
    torch.cuda.synchronize()


# (R, pad, stride) of a 1x1, a 3x3 stride-1 and a 3x3 stride-2 conv
@pytest.mark.parametrize("conv", [(1, 0, 1), (3, 1, 1), (3, 1, 2)])
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("C", [64, 128])
def test_dgrad_same_bits_with_and_without_wpack(monkeypatch, C, K, conv):
    from ddlw_amd.ops import conv_gemm

    r, pad, stride = conv
    torch.manual_seed(5)
    w = _rand(K, C, r, r, scale=0.1)
    dy = _rand(2, K, 8 // stride, 8 // stride)
    dx = {}
    for lever in ("0", "1"):
        monkeypatch.setenv("DDLW_DGRAD_WPACK", lever)
        dx[lever] = conv_gemm.conv_dgrad_kernel(dy, w, (2, C, 8, 8), pad, stride)
    assert dx["1"].shape == (2, C, 8, 8)
    assert torch.equal(dx["1"], dx["0"])


def test_bottleneck_same_bits_with_both_levers(monkeypatch):
    """One Bottleneck forward + backward at N = 16, 56x56, 64 -> 256 (conv
    epilogue partial counts above 512, so the folded finalize runs): output,
    every gradient and every running statistic bit-equal with
    DDLW_BN_FOLDED and DDLW_DGRAD_WPACK both off and both on."""
    from ddlw_amd.models.resnet import Bottleneck, Downsample
    from ddlw_amd.ops import binding

    monkeypatch.setenv("DDLW_CONV", "hip")
    torch.manual_seed(6)
    ds = Downsample(64, 256, 1)
    blk = Bottleneck(64, 64, stride=1, downsample=ds)
    for bn in (blk.bn1, blk.bn2, blk.bn3, ds.bn):
        torch.nn.init.uniform_(bn.weight, 0.5, 1.5)
        torch.nn.init.uniform_(bn.bias, -0.2, 0.2)
    blk = blk.to(_cuda()).to(memory_format=torch.channels_last)
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(torch.bfloat16)
    blk.train()
    x = _rand(16, 64, 56, 56)

    folded_calls = []
    real = binding._folded_args

    def spy(p0, nparts, C):
        out = real(p0, nparts, C)
        folded_calls.append(out is not None)
        return out

    monkeypatch.setattr(binding, "_folded_args", spy)
    res = {}
    for lever in ("0", "1"):
        monkeypatch.setenv("DDLW_BN_FOLDED", lever)
        monkeypatch.setenv("DDLW_DGRAD_WPACK", lever)
        folded_calls.clear()
        b = copy.deepcopy(blk)
        xa = x.clone().requires_grad_(True)
        out = b(xa)
        out.float().square().mean().backward()
        assert any(folded_calls) == (lever == "1"), \
            "the block's partial counts must reach the folded finalize"
        res[lever] = dict(
            {"out": out.detach(), "dx": xa.grad},
            **{"grad." + n: p.grad for n, p in b.named_parameters()},
            **{"buf." + n: t for n, t in b.named_buffers()})
    assert res["1"].keys() == res["0"].keys()
    assert any(n.endswith("running_var") for n in res["0"])
    for n, t in res["0"].items():
        assert torch.equal(res["1"][n], t), n
