"""MobileNetV2 takes uint8 images: the fused normalize + stem conv + BN +
ReLU6 kernel (``k_stem3_u8`` in ``ops/hip/conv_stem.hip``), its gate
(``mbconv.stem_u8_fusable``) and the model wiring.

Kernel parity bound, ``max|y - ref| <= 1e-2 * max|ref|`` against fp32 stock
ops (the convention of ``tests/test_mbconv_eval.py``): the kernel rounds the
normalized input to bf16 (2^-9 relative per operand, 27 products that mostly
cancel) and its output once (2^-9 of up to ~12); on these shapes a CPU model
of exactly that rounding reaches 0.19-0.44 of the bound, and the kernel on an
MI355X measured 0.26-0.47 of it.
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from ddlw_amd.models.mobilenet_v2 import MobileNetV2, build_model
from ddlw_amd.ops import abi, mbconv

TOL = 1e-2
ENV_SWITCHES = ("DDLW_DISABLE_HIP_OPS", "DDLW_EVAL_FOLD", "DDLW_CONV", "DDLW_STEM_U8")


def _dev():
    return torch.device("cuda:0")


def _clear_env(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _act(v, act):
    return {0: lambda t: t, 1: F.relu, 2: F.relu6}[act](v)


def _nchw(u8_nhwc):
    """The model's input contract: N x C x H x W over NHWC memory."""
    return u8_nhwc.permute(0, 3, 1, 2)


# --------------------------------------------------------------------------- #
# 1. kernel parity
# --------------------------------------------------------------------------- #

# (N, H, W): one output pixel with five of nine taps padding; odd H and W
# (bottom / right padding); even; odd; mixed; 390 output pixels (three 128-row
# tiles, the last a tail, and a 390-byte row pitch); 1024 output pixels
STEM_SHAPES = [(1, 2, 2), (2, 7, 9), (3, 16, 16), (2, 15, 17), (2, 33, 18),
               (2, 5, 130), (1, 64, 64)]
# (name, scale/bias?, act)
STEM_EPILOGUES = [("plain", False, 0), ("affine", True, 0), ("relu", True, 1),
                  ("relu6", True, 2)]


@functools.lru_cache(maxsize=None)
def _stem_case(shape):
    """CPU inputs and the fp32 reference convolution of one shape, computed
    once and shared by its four epilogues (never modified)."""
    N, H, W = shape
    g = torch.Generator(device="cpu").manual_seed(1000 * N + 37 * H + W)
    u8 = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
    w = torch.randn(32, 3, 3, 3, generator=g).to(torch.bfloat16)
    # 27 taps of U(-1,1) x N(0,1) ~ N(0, 3^2): scale ~1, bias ~3 puts the
    # pre-activation at ~N(3, 3^2): ~16% < 0, ~68% in (0, 6), ~16% > 6
    scale = torch.empty(32).uniform_(0.9, 1.1, generator=g)
    bias = torch.empty(32).uniform_(2.8, 3.2, generator=g)
    conv = F.conv2d(_nchw(u8).float() / 127.5 - 1, w.float(), stride=2, padding=1)
    return u8, w, scale, bias, conv


def _check(y, ref, what):
    assert torch.isfinite(y).all(), what
    err = (y.float() - ref).abs().max().item()
    bound = TOL * ref.abs().max().item()
    print(f"{what}: max|y-ref| {err:.4e}  bound {bound:.4e}")
    assert err <= bound, (what, err, bound)


def _assert_regions(pre, what):
    """Each region of the fp32 pre-activation holds >= 5% of the elements."""
    n = pre.numel()
    for name, cnt in (("<0", (pre < 0).sum()), ("(0,6)", ((pre > 0) & (pre < 6)).sum()),
                      (">6", (pre > 6).sum())):
        share = cnt.item() / n
        print(f"{what} region {name}: {share:.3f}")
        assert share >= 0.05, (what, name, share)


@pytest.mark.gpu
@pytest.mark.parametrize("ep", STEM_EPILOGUES, ids=[e[0] for e in STEM_EPILOGUES])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "n%d_h%d_w%d" % s)
def test_stem3_u8_parity(shape, ep):
    from ddlw_amd.ops import binding

    N, H, W = shape
    name, affine, act = ep
    u8, w, scale, bias, conv = _stem_case(shape)
    pre = conv
    if affine:
        pre = conv * scale.view(1, 32, 1, 1) + bias.view(1, 32, 1, 1)
    dev = _dev()
    y = binding.stem3_u8_fwd_ep(
        _nchw(u8.to(dev)), w.to(dev), scale.to(dev) if affine else None,
        bias.to(dev) if affine else None, act)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert y.shape == (N, 32, Ho, Wo) and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    what = f"stem {shape} {name}"
    y = y.cpu()
    _check(y, _act(pre, act), what)
    if act == 2 and pre.numel() >= 1000:
        _assert_regions(pre, what)
        assert y.max().item() == 6.0 and y.min().item() == 0.0


@pytest.mark.gpu
def test_stem3_u8_normalize_is_the_kernels_value():
    """A centre-tap identity weight (channel k copies input channel k) makes
    output channels 0..2 the normalized input at the even pixels: bit-equal
    to ``normalize_u8_bf16`` for every byte value, and channels 3.. zero."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.layers import normalize_u8_bf16

    dev = _dev()
    h = torch.arange(16).view(16, 1, 1)
    wcol = torch.arange(16).view(1, 16, 1)
    c = torch.arange(3).view(1, 1, 3)
    even = ((h * 16 + wcol + 85 * c) % 256).to(torch.uint8)  # the sampled pixels
    u8 = even.repeat_interleave(2, 0).repeat_interleave(2, 1).unsqueeze(0).to(dev)
    x = _nchw(u8)
    assert x.shape == (1, 3, 32, 32)
    assert all(len(torch.unique(x[:, k, ::2, ::2])) == 256 for k in range(3))
    w = torch.zeros(32, 3, 3, 3, dtype=torch.bfloat16, device=dev)
    for k in range(3):
        w[k, k, 1, 1] = 1.0
    y = binding.stem3_u8_fwd_ep(x, w)
    xn = normalize_u8_bf16(x)
    assert torch.equal(y[:, :3], xn[:, :, ::2, ::2])
    assert torch.count_nonzero(y[:, 3:]).item() == 0


# --------------------------------------------------------------------------- #
# 2. padding is zero in normalized space
# --------------------------------------------------------------------------- #


@pytest.mark.gpu
@pytest.mark.parametrize("size", [5, 6])
def test_stem3_u8_padding_is_exact(size):
    """w = 1, image all 255 (normalized: exactly 1): every output is 3 x the
    number of in-image taps — 27 interior, 18 edge, 12 corner. Padding done
    in byte space (byte 0 = -1) gives smaller numbers at the border."""
    from ddlw_amd.ops import binding

    dev = _dev()
    taps = F.conv2d(torch.ones(1, 1, size, size), torch.ones(1, 1, 3, 3),
                    stride=2, padding=1)
    expect = (3 * taps).expand(1, 32, -1, -1)
    assert set(expect.unique().tolist()) == {12.0, 18.0, 27.0}
    w = torch.ones(32, 3, 3, 3, dtype=torch.bfloat16, device=dev)
    for byte, sign in ((255, 1.0), (0, -1.0)):
        u8 = torch.full((1, size, size, 3), byte, dtype=torch.uint8, device=dev)
        y = binding.stem3_u8_fwd_ep(_nchw(u8), w)
        assert torch.equal(y.float().cpu(), sign * expect), (byte, y.float().cpu()[0, 0])


# --------------------------------------------------------------------------- #
# 3. neighbouring images do not leak; calls are deterministic
# --------------------------------------------------------------------------- #


@pytest.mark.gpu
def test_stem3_u8_neighbours_do_not_leak():
    from ddlw_amd.ops import binding

    dev = _dev()
    _, w, scale, bias, _ = _stem_case((2, 7, 9))
    w, scale, bias = w.to(dev), scale.to(dev), bias.to(dev)
    g = torch.Generator(device="cpu").manual_seed(11)
    mid = torch.randint(0, 256, (2, 7, 9, 3), dtype=torch.uint8, generator=g).to(dev)
    outs = []
    for fill in (255, 0):
        buf = torch.full((6, 7, 9, 3), fill, dtype=torch.uint8, device=dev)
        buf[2:4] = mid
        x = _nchw(buf)[2:4]
        assert x.data_ptr() == buf[2].data_ptr()
        outs.append(binding.stem3_u8_fwd_ep(x, w, scale, bias, 2))
    alone = binding.stem3_u8_fwd_ep(_nchw(mid.clone()), w, scale, bias, 2)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], alone)


# --------------------------------------------------------------------------- #
# 4. rejections
# --------------------------------------------------------------------------- #


@pytest.mark.gpu
def test_stem3_u8_rejects_bad_arguments():
    """The library refuses with its ``who: why`` text and status 2, which it
    returns before any launch."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import KernelLibError

    dev = _dev()

    def u8(c):
        return _nchw(torch.zeros(1, 4, 4, c, dtype=torch.uint8, device=dev))

    def wt(k, c):
        return torch.zeros(k, c, 3, 3, dtype=torch.bfloat16, device=dev)

    ones = torch.ones(32, device=dev)
    for args, why in (((u8(4), wt(32, 4)), "C=3, K=32"),
                      ((u8(3), wt(24, 3)), "C=3, K=32"),
                      ((u8(3), wt(32, 3), ones, None), "scale and bias come together")):
        with pytest.raises(KernelLibError, match=r"status 2\): stem3_u8_fwd_ep: ") as e:
            binding.stem3_u8_fwd_ep(*args)
        assert why in str(e.value)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- #
# 5. whole model
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


COUNTED = ("stem3_u8_fwd_ep", "normalize_u8", "bn_apply", "pw_conv_fwd",
           "depthwise_fwd_ep")


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


def _u8_batch(dev, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    u8 = torch.randint(0, 256, (8, 64, 64, 3), dtype=torch.uint8, generator=g)
    return _nchw(u8.to(dev))


def _frozen_model(dev, **kw):
    torch.manual_seed(31)
    model = build_model(64, 64, 3, 5, dropout=0.0, **kw)
    _randomize_bn(model, seed=9)
    return _to_bf16_convs(model.to(dev))


@pytest.mark.gpu
def test_frozen_model_from_uint8(monkeypatch):
    from ddlw_amd.ops.layers import normalize_u8_bf16, softmax_cross_entropy

    _clear_env(monkeypatch)
    dev = _dev()
    m = _frozen_model(dev).train()
    assert not m.base.base.training
    u8 = _u8_batch(dev)
    labels = torch.randint(0, 5, (8,), device=dev)

    calls = _count_calls(monkeypatch)
    logits = m(u8)
    assert calls == {"stem3_u8_fwd_ep": 1, "normalize_u8": 0, "bn_apply": 0,
                     "pw_conv_fwd": 34, "depthwise_fwd_ep": 17}, calls
    loss = softmax_cross_entropy(logits, labels)
    loss.backward()
    grad = m.classifier.weight.grad
    assert grad is not None and torch.isfinite(grad.float()).all()
    assert grad.float().abs().max().item() > 0

    with torch.no_grad():
        ref = m(normalize_u8_bf16(u8))
    rel = ((logits.float() - ref.float()).abs().max() / ref.float().abs().max()).item()
    print(f"frozen model from uint8, logits: rel {rel:.4e}")
    assert rel <= 5e-2, rel


@pytest.mark.gpu
def test_frozen_model_stem_switched_off(monkeypatch):
    from ddlw_amd.ops.layers import normalize_u8_bf16

    _clear_env(monkeypatch)
    dev = _dev()
    m = _frozen_model(dev).eval()
    u8 = _u8_batch(dev)
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        monkeypatch.setenv("DDLW_STEM_U8", "0")
        logits = m(u8)
        assert calls["stem3_u8_fwd_ep"] == 0 and calls["normalize_u8"] == 1, calls
        assert calls["bn_apply"] == 1, calls
        assert calls["pw_conv_fwd"] == 34 and calls["depthwise_fwd_ep"] == 17, calls
        assert torch.equal(logits, m(normalize_u8_bf16(u8)))
        monkeypatch.delenv("DDLW_STEM_U8")
        for name, value in (("DDLW_EVAL_FOLD", "0"), ("DDLW_CONV", "stock"),
                            ("DDLW_DISABLE_HIP_OPS", "1")):
            monkeypatch.setenv(name, value)
            for k in calls:
                calls[k] = 0
            logits = m(u8)
            assert calls["stem3_u8_fwd_ep"] == 0, (name, calls)
            assert torch.equal(logits, m(normalize_u8_bf16(u8))), name
            monkeypatch.delenv(name)


@pytest.mark.gpu
def test_fine_tune_splits_from_uint8(monkeypatch):
    from ddlw_amd.ops.layers import softmax_cross_entropy

    _clear_env(monkeypatch)
    dev = _dev()
    u8 = _u8_batch(dev)
    labels = torch.randint(0, 5, (8,), device=dev)
    calls = _count_calls(monkeypatch)

    m = _frozen_model(dev, fine_tune_at=13).train()
    softmax_cross_entropy(m(u8), labels).backward()
    assert calls["stem3_u8_fwd_ep"] == 1 and calls["normalize_u8"] == 0, calls
    for name, p in m.base.base.features.named_parameters():
        idx = int(name.split(".")[0])
        assert (p.grad is not None) == (idx >= 13), name
        if p.grad is not None:
            assert torch.isfinite(p.grad.float()).all(), name

    for k in (1, 0):
        for n in calls:
            calls[n] = 0
        m = _frozen_model(dev, fine_tune_at=k).train()
        softmax_cross_entropy(m(u8), labels).backward()
        assert calls["stem3_u8_fwd_ep"] == 0 and calls["normalize_u8"] == 1, (k, calls)
        trainable = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
        assert any(n.startswith("base.base.features.1.") for n, _ in trainable)
        for n, p in trainable:
            assert p.grad is not None and torch.isfinite(p.grad.float()).all(), (k, n)


# --------------------------------------------------------------------------- #
# CPU: equality with the normalized batch, the gate, keys, ABI
# --------------------------------------------------------------------------- #


def _cpu_u8(channels=3, seed=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return _nchw(torch.randint(0, 256, (2, 64, 64, channels), dtype=torch.uint8,
                               generator=g))


@pytest.mark.parametrize("case", ["base_eval", "head_eval", "head_train", "ft13_eval",
                                  "ft13_train", "one_channel"])
def test_cpu_uint8_equals_normalized(case, monkeypatch):
    _clear_env(monkeypatch)
    torch.manual_seed(4)
    if case == "base_eval":
        net = MobileNetV2().eval()
    elif case == "one_channel":
        net = MobileNetV2(channels=1).eval()
    else:
        kw = {"fine_tune_at": 13} if case.startswith("ft13") else {}
        net = build_model(64, 64, 3, 5, dropout=0.0, **kw).train(case.endswith("train"))
    _randomize_bn(net, seed=3)
    u8 = _cpu_u8(1 if case == "one_channel" else 3)
    with torch.set_grad_enabled(net.training):
        y = net(u8)
        ref = net(u8.float() / 127.5 - 1)
    assert y.dtype == torch.float32 and torch.isfinite(y).all()
    assert torch.equal(y, ref)


def test_train_model_steps_accept_uint8(monkeypatch):
    from ddlw_amd.train import Model

    _clear_env(monkeypatch)
    torch.manual_seed(6)
    model = Model(build_model(64, 64, 3, 5, dropout=0.0)).compile("adam")
    u8 = _cpu_u8()
    labels = torch.tensor([1, 3])
    for logs in (model.train_step(u8, labels), model.eval_step(u8, labels)):
        assert logs["loss"] == logs["loss"] and abs(logs["loss"]) < float("inf"), logs


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


def _bf16_net(channels=3):
    net = MobileNetV2(channels).eval()
    for mod in net.modules():
        if isinstance(mod, torch.nn.Conv2d):
            mod.to(torch.bfloat16)
    return net


def test_stem_u8_gate(monkeypatch):
    _clear_env(monkeypatch)
    net = _bf16_net()
    fake = _FakeCudaU8()
    assert not mbconv.stem_u8_fusable(net, fake)  # grad enabled
    with torch.no_grad():
        assert mbconv.stem_u8_fusable(net, fake)
        net.train()
        assert not mbconv.stem_u8_fusable(net, fake)
        net.eval()
        net.features[1].train()
        assert not mbconv.stem_u8_fusable(net, fake)
        net.eval()
        for name, value in (("DDLW_DISABLE_HIP_OPS", "1"), ("DDLW_EVAL_FOLD", "0"),
                            ("DDLW_CONV", "stock"), ("DDLW_STEM_U8", "0")):
            monkeypatch.setenv(name, value)
            assert not mbconv.stem_u8_fusable(net, fake), name
            monkeypatch.delenv(name)
        monkeypatch.setenv("DDLW_STEM_U8", "1")
        assert mbconv.stem_u8_fusable(net, fake)
        monkeypatch.delenv("DDLW_STEM_U8")
        assert not mbconv.stem_u8_fusable(net, _FakeCudaU8(channels_last=False))
        assert not mbconv.stem_u8_fusable(net, _cpu_u8())  # a real CPU batch
        assert not mbconv.stem_u8_fusable(_bf16_net(channels=1), fake)
        assert not mbconv.stem_u8_fusable(MobileNetV2().eval(), fake)  # fp32 weights
        bn = net.features[1]
        bn.running_mean = bn.running_mean.to(torch.bfloat16)
        assert not mbconv.stem_u8_fusable(net, fake)
        bn.running_mean = bn.running_mean.float()
        assert mbconv.stem_u8_fusable(net, fake)


def test_state_dict_keys_unchanged_by_stem_switch(monkeypatch):
    _clear_env(monkeypatch)
    keys = list(build_model().state_dict())
    for value in ("0", "1"):
        monkeypatch.setenv("DDLW_STEM_U8", value)
        assert keys == list(build_model().state_dict())
    assert "base.base.features.0.weight" in keys and len(build_model().base.base.features) == 23
    assert not [k for k in keys if "stem3" in k or "u8" in k]
    # running the uint8 entry adds nothing to the state either
    model = build_model(64, 64, 3, 5).eval()
    with torch.no_grad():
        model(_cpu_u8())
    assert list(model.state_dict()) == keys


def test_abi_row_for_the_stem_export():
    restype, argtypes = abi.SIGNATURES["ddlw_stem3_u8_fwd_ep"]
    # x, wp, y, scale, bias, act, N, H, W, C, K, stream
    assert restype is abi.c_int and len(argtypes) == 12
    assert argtypes[:5] == [abi.Ptr] * 5 and argtypes[-1] is abi.Ptr
    assert argtypes[5:11] == [abi.c_int] * 6
