"""Trainable MobileNetV2 pointwise (1x1) convs on the MFMA kernels: the
forward with BN statistics from its epilogue (``k_pw_conv_stats``), dgrad on
the same GEMM, wgrad on the split-K kernel, the stage Function
(``ops/mbconv.py``), the layer Function (``ops/conv.py``) and the model
wiring.

Tolerances: the GEMM parity tests use the file-level rule of
``test_mbconv_eval.py`` (one bf16 output rounding, 2^-8, against
``1e-2 * max|ref|``); comparisons of two bf16 pipelines use the project's
``err(new) <= 2 * err(yardstick) + 1e-3`` in relative L2 against fp32.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from ddlw_amd.models import build_resnet50
from ddlw_amd.models.mobilenet_v2 import InvertedResidual, MobileNetV2, build_model
from ddlw_amd.ops import mbconv
from ddlw_amd.ops.conv import Conv2d
from ddlw_amd.ops.layers import BatchNormAct2d

TOL = 1e-2
ENV_SWITCHES = ("DDLW_DISABLE_HIP_OPS", "DDLW_EVAL_FOLD", "DDLW_CONV", "DDLW_PW_TRAIN")
NEW_FUNCTIONS = ("pw_conv_fwd_stats", "pw_conv_train_fwd", "pw_conv_dgrad",
                 "pw_conv_wgrad")


def _dev():
    return torch.device("cuda:0")


def _clear_env(monkeypatch):
    for k in ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _bf16_randn(*shape, g):
    return torch.randn(*shape, generator=g).to(torch.bfloat16)


def _check(y, ref, what):
    assert torch.isfinite(y).all(), what
    err = (y.float() - ref).abs().max().item()
    bound = TOL * ref.abs().max().item()
    print(f"{what}: max|y-ref| {err:.4e}  bound {bound:.4e}")
    assert err <= bound, (what, err, bound)


def _rel_l2(y, ref):
    return ((y.float() - ref.float()).norm() / (ref.float().norm() + 1e-30)).item()


def _assert_two_pipelines(new, parent, ref, what):
    e_n, e_p = _rel_l2(new, ref), _rel_l2(parent, ref)
    print(f"{what}: err_new {e_n:.4e}  err_parent {e_p:.4e}")
    assert torch.isfinite(new.float()).all(), what
    assert e_n <= 2 * e_p + 1e-3, (what, e_n, e_p)


def _assert_regions(pre, what):
    """Each region of the fp32 ReLU6 pre-activation holds >= 5% of the
    elements."""
    n = pre.numel()
    for name, cnt in (("<0", (pre < 0).sum()), ("(0,6)", ((pre > 0) & (pre < 6)).sum()),
                      (">6", (pre > 6).sum())):
        share = cnt.item() / n
        print(f"{what} region {name}: {share:.3f}")
        assert share >= 0.05, (what, name, share)


def _count_calls(monkeypatch, names):
    from ddlw_amd.ops import binding

    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(binding, n)

        def counted(*a, _real=real, _n=n, **k):
            calls[_n] += 1
            return _real(*a, **k)

        monkeypatch.setattr(binding, n, counted)
    return calls


def _to_bf16_convs(m):
    m = copy.deepcopy(m).to(memory_format=torch.channels_last)
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
            mod.to(torch.bfloat16)
    return m


# --------------------------------------------------------------------------- #
# 1. forward with statistics
# --------------------------------------------------------------------------- #

# (C, K, M): every channels-per-wave instantiation, M tails, one row, two N
# tiles plus a K tail, and the tail conv's ten N tiles
STATS_SHAPES = [(24, 136, 130), (16, 96, 147), (40, 376, 162), (64, 192, 162),
                (32, 64, 1), (320, 1280, 130)]


def _stat_errors(mean, rstd, rm, rv, ref):
    """Errors in units of the channel's std (variances: of its variance),
    worst channel. ``ref`` = fp64 (mean, var + eps, running_mean, running_var)."""
    mean64, vare64, rm64, rv64 = ref
    std = vare64.sqrt()
    return {
        "mean": ((mean.double() - mean64).abs() / std).max().item(),
        "rstd": ((1.0 / rstd.double() - std).abs() / std).max().item(),
        "running_mean": ((rm.double() - rm64).abs() / std).max().item(),
        "running_var": ((rv.double() - rv64).abs() / vare64).max().item(),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("shape", STATS_SHAPES, ids=lambda s: "c%d_k%d_m%d" % s)
def test_pw_conv_fwd_stats(shape):
    """y is bit-equal to the plain kernel's (same MFMA chain per accumulator,
    same single rounding); the statistics from the epilogue partials are those
    of the bf16 y: against fp64, err_fused <= 2 * err_standalone + M * 2^-24
    (two fp32 sums in different orders; M * 2^-24 is the recursive-sum
    bound)."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import query

    C, K, M = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(C * 7 + K + M)
    x = _bf16_randn(M, C, g=g).to(dev)
    w = _bf16_randn(K, C, g=g).to(dev)
    rm0 = torch.empty(K).uniform_(-0.3, 0.3, generator=g).to(dev)
    rv0 = torch.empty(K).uniform_(0.5, 1.5, generator=g).to(dev)
    eps, mom = 1e-5, 0.1

    nparts_q = int(query("pw_conv_nparts", M, K, None))
    assert nparts_q == -(-M // 128)
    PAD = 2
    buf = torch.full((2, nparts_q + 2 * PAD, K), -1234.0, dtype=torch.float32, device=dev)
    before = buf.clone()
    parts = (buf[0, PAD:PAD + nparts_q], buf[1, PAD:PAD + nparts_q])
    y, ps, pq, nparts = binding.pw_conv_fwd_stats(x, w.view(K, C, 1, 1), parts=parts)
    assert nparts == nparts_q
    assert ps.data_ptr() == parts[0].data_ptr() and pq.data_ptr() == parts[1].data_ptr()
    assert y.shape == (M, K) and y.dtype == torch.bfloat16
    assert torch.equal(y, binding.pw_conv_fwd(x, w))
    assert torch.equal(buf[:, :PAD], before[:, :PAD])
    assert torch.equal(buf[:, PAD + nparts:], before[:, PAD + nparts:])
    assert torch.isfinite(ps).all() and torch.isfinite(pq).all()

    rm_f, rv_f, rm_s, rv_s = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    mean_f, rstd_f = binding.bn_finalize_parts(ps, pq, nparts, M, K, eps, mom, rm_f, rv_f)
    mean_s, rstd_s = binding.bn_stats(y, eps, mom, rm_s, rv_s)

    y64 = y.double()
    mean64 = y64.mean(0)
    var64 = ((y64 - mean64) ** 2).mean(0)
    ref = (mean64, var64 + eps, (1 - mom) * rm0.double() + mom * mean64,
           (1 - mom) * rv0.double() + mom * var64 * M / max(M - 1, 1))
    e_f = _stat_errors(mean_f, rstd_f, rm_f, rv_f, ref)
    e_s = _stat_errors(mean_s, rstd_s, rm_s, rv_s, ref)
    slack = M * 2.0 ** -24
    for name in e_f:
        print(f"stats {shape} {name}: err_fused {e_f[name]:.3e}  "
              f"err_standalone {e_s[name]:.3e}  slack {slack:.3e}")
    for name in e_f:
        assert e_f[name] <= 2 * e_s[name] + slack, (name, e_f[name], e_s[name])


@pytest.mark.gpu
def test_pw_conv_fwd_stats_nhwc_and_own_buffers():
    """4-D channels_last entry, partial buffers allocated by the binding."""
    from ddlw_amd.ops import binding

    g = torch.Generator(device="cpu").manual_seed(4)
    x = _bf16_randn(3, 24, 7, 7, g=g).to(_dev()).contiguous(memory_format=torch.channels_last)
    w = _bf16_randn(136, 24, 1, 1, g=g).to(_dev())
    y, ps, pq, nparts = binding.pw_conv_fwd_stats(x, w)
    assert y.shape == (3, 136, 7, 7) and y.is_contiguous(memory_format=torch.channels_last)
    assert nparts == 2 and ps.shape == pq.shape == (2, 136)
    y2 = y.permute(0, 2, 3, 1).reshape(-1, 136).float()
    # 147 exact bf16 values summed in fp32: 147 * 2^-24 relative to sum|y|
    assert (ps.sum(0) - y2.sum(0)).abs().max() <= 147 * 2.0 ** -24 * y2.abs().sum(0).max()
    assert (pq.sum(0) - (y2 * y2).sum(0)).abs().max() <= 147 * 2.0 ** -23 * (y2 * y2).sum(0).max()


# --------------------------------------------------------------------------- #
# 2. dgrad
# --------------------------------------------------------------------------- #

# (C, K, M): a tail on the reduction axis (K=40), a narrow output, five N
# tiles, one row
DGRAD_SHAPES = [(24, 40, 147), (144, 24, 130), (960, 160, 162), (16, 96, 1)]


def _dgrad_inputs(C, K, M, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = _dev()
    dy = _bf16_randn(M, K, g=g).to(dev)
    w = _bf16_randn(K, C, g=g).to(dev)
    acc = _bf16_randn(M, C, g=g).to(dev)
    return dy, w, acc


@pytest.mark.gpu
@pytest.mark.parametrize("with_acc", [False, True], ids=["plain", "acc"])
@pytest.mark.parametrize("shape", DGRAD_SHAPES, ids=lambda s: "c%d_k%d_m%d" % s)
def test_pw_conv_dgrad_parity(shape, with_acc):
    from ddlw_amd.ops import binding

    C, K, M = shape
    dy, w, acc = _dgrad_inputs(C, K, M, seed=C * 5 + K + M)
    ref = dy.float() @ w.float()
    if with_acc:
        ref = ref + acc.float()
    dx = binding.pw_conv_dgrad(dy, w.view(K, C, 1, 1), (M, C),
                               acc=acc if with_acc else None)
    assert dx.shape == (M, C) and dx.dtype == torch.bfloat16
    _check(dx, ref, f"pw dgrad {shape} acc={with_acc}")


@pytest.mark.gpu
def test_pw_conv_dgrad_tails_do_not_leak():
    """dy, w^T and acc are row slices out of NaN-filled buffers and dx sits
    inside a sentinel buffer: K=40 leaves an 8-channel tail in the 32-deep
    reduction step, C=24 an output-channel tail, M=147 a row tail."""
    from ddlw_amd.ops import binding

    C, K, M, PAD = 24, 40, 147, 40
    dy, w, acc = _dgrad_inputs(C, K, M, seed=6)
    dev = _dev()

    def embed(t, pad):
        buf = torch.full((t.shape[0] + 2 * pad, t.shape[1]), float("nan"),
                         dtype=torch.bfloat16, device=dev)
        buf[pad:pad + t.shape[0]] = t
        return buf[pad:pad + t.shape[0]]

    dys, wts, accs = embed(dy, PAD), embed(w.t().contiguous(), 8), embed(acc, PAD)
    dxbuf = torch.full((M + 2 * PAD, C), -1234.0, dtype=torch.bfloat16, device=dev)
    before = dxbuf.clone()
    dx = binding.pw_conv_dgrad(dys, w.view(K, C, 1, 1), (M, C), acc=accs,
                               out=dxbuf[PAD:PAD + M], w_t=wts)
    assert dx.data_ptr() == dxbuf[PAD].data_ptr()
    _check(dx, dy.float() @ w.float() + acc.float(), "pw dgrad tails")
    assert torch.equal(dxbuf[:PAD], before[:PAD])
    assert torch.equal(dxbuf[PAD + M:], before[PAD + M:])


# --------------------------------------------------------------------------- #
# 3. wgrad at pointwise shapes
# --------------------------------------------------------------------------- #

# (N, H=W, C, K): K and C below the 64-wide tile, both tile mixes, one row
WGRAD_SHAPES = [(3, 7, 16, 96), (2, 9, 96, 24), (2, 9, 24, 144), (2, 9, 160, 960),
                (1, 1, 32, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "n%d_hw%d_c%d_k%d" % s)
def test_conv_wgrad_at_pointwise_shapes(shape):
    """relL2(hip) <= 2 * relL2(library) + 1e-3 against the fp32 product."""
    from ddlw_amd.ops.conv_gemm import conv_wgrad_kernel

    N, HW, C, K = shape
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(N + HW * 3 + C + K)
    x = _bf16_randn(N, C, HW, HW, g=g).to(dev).contiguous(memory_format=torch.channels_last)
    dy = _bf16_randn(N, K, HW, HW, g=g).to(dev).contiguous(memory_format=torch.channels_last)
    x2 = x.permute(0, 2, 3, 1).reshape(-1, C)
    dy2 = dy.permute(0, 2, 3, 1).reshape(-1, K)
    ref = dy2.float().T @ x2.float()
    dw = conv_wgrad_kernel(dy, x, (K, C, 1, 1), 1, 0)
    assert dw.shape == (K, C, 1, 1) and dw.dtype == torch.bfloat16
    w0 = torch.zeros(K, C, 1, 1, dtype=torch.bfloat16, device=dev)
    _, lib, _ = torch.ops.aten.convolution_backward(
        dy, x, w0, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
        [False, True, False])
    _assert_two_pipelines(dw.reshape(K, C), lib.reshape(K, C), ref, f"wgrad {shape}")


# --------------------------------------------------------------------------- #
# 4. stage Function
# --------------------------------------------------------------------------- #

STAGE_CASES = [(24, 144, "none"), (24, 144, "relu6"), (144, 24, "none"),
               (144, 24, "relu6")]


def _stage_setup(C, K, act):
    """fp32 conv + BN (CPU) with the BN affine of ``_pw_inputs`` in
    test_mbconv_eval.py: the normalized conv output is ~N(0,1), gamma ~3 and
    beta ~3 put the pre-activation at ~N(3, 3^2): ~16% < 0, ~68% in (0,6),
    ~16% > 6."""
    g = torch.Generator(device="cpu").manual_seed(C * 3 + K + len(act))
    conv = Conv2d(C, K, 1, bias=False)
    conv.pw_train = True
    bn = BatchNormAct2d(K, act=act)
    with torch.no_grad():
        conv.weight.copy_(_bf16_randn(K, C, 1, 1, g=g).float() / C ** 0.5)
        conv.weight.copy_(conv.weight.to(torch.bfloat16).float())
        bn.weight.copy_(torch.empty(K).uniform_(0.9, 1.1, generator=g) * 3.0)
        bn.bias.copy_(torch.empty(K).uniform_(2.8, 3.2, generator=g))
        bn.running_mean.copy_(torch.empty(K).uniform_(-0.3, 0.3, generator=g))
        bn.running_var.copy_(torch.empty(K).uniform_(0.5, 1.5, generator=g))
    x = _bf16_randn(2, C, 9, 9, g=g).float()
    gout = _bf16_randn(2, K, 9, 9, g=g).float()
    return conv.train(), bn.train(), x, gout


def _stage_preact(conv, bn, x):
    """fp32 pre-activation of the stage in training mode (no buffer update)."""
    with torch.no_grad():
        return F.batch_norm(F.conv2d(x, conv.weight), None, None, bn.weight, bn.bias,
                            True, 0.0, bn.eps)


@pytest.mark.parametrize("case", STAGE_CASES, ids=lambda c: "c%d_k%d_%s" % c)
def test_stage_seeds_cover_relu6_regions(case):
    """CPU, fp32 reference alone: the seeds of the stage test put >= 5% of the
    pre-activation into each ReLU6 region."""
    conv, bn, x, _ = _stage_setup(*case)
    _assert_regions(_stage_preact(conv, bn, x), f"stage {case}")


def _stage_run(conv, bn, x, gout, fused):
    x = x.detach().clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = mbconv.pw_conv_bn_train(conv, bn, x) if fused else bn(conv(x))
    (y.float() * gout.float()).sum().backward()
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": x.grad, "dW": conv.weight.grad,
            "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
            "running_mean": bn.running_mean.detach().clone(),
            "running_var": bn.running_var.detach().clone(),
            "num_batches_tracked": int(bn.num_batches_tracked)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", STAGE_CASES, ids=lambda c: "c%d_k%d_%s" % c)
def test_stage_function_vs_parent_path(case, monkeypatch):
    """conv1x1 + BatchNormAct2d, one step, three ways: fp32 stock ops, bf16
    with DDLW_PW_TRAIN=0 (the parent path) and bf16 on the stage Function."""
    _clear_env(monkeypatch)
    C, K, act = case
    conv, bn, x, gout = _stage_setup(C, K, act)
    _assert_regions(_stage_preact(conv, bn, x), f"stage {case}")
    dev = _dev()
    conv32, bn32 = conv.to(dev), bn.to(dev)
    x, gout = x.to(dev), gout.to(dev)
    convb, bnb = copy.deepcopy(conv32).to(torch.bfloat16), copy.deepcopy(bn32)
    convn, bnn = copy.deepcopy(convb), copy.deepcopy(bn32)
    convb.to(memory_format=torch.channels_last), convn.to(memory_format=torch.channels_last)

    monkeypatch.setenv("DDLW_DISABLE_HIP_OPS", "1")
    ref = _stage_run(conv32, bn32, x, gout, fused=False)
    monkeypatch.delenv("DDLW_DISABLE_HIP_OPS")

    calls = _count_calls(monkeypatch, NEW_FUNCTIONS)
    monkeypatch.setenv("DDLW_PW_TRAIN", "0")
    parent = _stage_run(convb, bnb, x.to(torch.bfloat16), gout.to(torch.bfloat16), fused=False)
    assert not any(calls.values()), calls
    monkeypatch.delenv("DDLW_PW_TRAIN")
    new = _stage_run(convn, bnn, x.to(torch.bfloat16), gout.to(torch.bfloat16), fused=True)
    assert calls["pw_conv_fwd_stats"] == 1 and calls["pw_conv_dgrad"] == 1, calls

    for name in ("y", "dx", "dW", "dgamma", "dbeta", "running_mean", "running_var"):
        assert new[name].shape == ref[name].shape, name
        _assert_two_pipelines(new[name], parent[name], ref[name], f"stage {case} {name}")
    assert new["num_batches_tracked"] == parent["num_batches_tracked"] == 1
    if act == "relu6":
        assert new["y"].max().item() == 6.0 and new["y"].min().item() == 0.0


# --------------------------------------------------------------------------- #
# 5. block routing
# --------------------------------------------------------------------------- #

BLOCK_COUNTED = NEW_FUNCTIONS + ("pw_conv_fwd", "bn_stats")


def _block_step(blk, x, requires_grad=True):
    x = x.detach().clone().requires_grad_(requires_grad)
    y = blk(x)
    # a weighted sum: the plain sum of a batch-normalized output has no gradient
    g = torch.Generator(device="cpu").manual_seed(7)
    gout = _bf16_randn(*y.shape, g=g).to(y.device)
    (y.float() * gout.float()).sum().backward()
    torch.cuda.synchronize()
    return y.detach(), x.grad


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(24, 24, 1, 6), (16, 24, 2, 6)],
                         ids=lambda c: "%dto%d_s%d_t%d" % c)
def test_training_block_routing(cfg, monkeypatch):
    _clear_env(monkeypatch)
    in_ch, out_ch, stride, t = cfg
    dev = _dev()
    torch.manual_seed(41)
    blk = _to_bf16_convs(InvertedResidual(in_ch, out_ch, stride, t).to(dev)).train()
    g = torch.Generator(device="cpu").manual_seed(in_ch + out_ch)
    x = _bf16_randn(2, in_ch, 9, 9, g=g).to(dev).contiguous(memory_format=torch.channels_last)

    calls = _count_calls(monkeypatch, BLOCK_COUNTED)
    y, dx = _block_step(blk, x)
    assert calls == {"pw_conv_fwd_stats": 2, "pw_conv_train_fwd": 0,
                     "pw_conv_dgrad": 2, "pw_conv_wgrad": 2, "pw_conv_fwd": 0,
                     "bn_stats": 1}, calls
    assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all()
    for p in blk.parameters():
        assert p.grad is not None and torch.isfinite(p.grad.float()).all()
        assert p.grad.float().abs().max().item() > 0

    # the first trainable block's input comes out of the no_grad prefix
    for k in calls:
        calls[k] = 0
    _block_step(blk, x, requires_grad=False)
    assert calls["pw_conv_dgrad"] == 1 and calls["pw_conv_wgrad"] == 2, calls

    for name, value in (("DDLW_PW_TRAIN", "0"), ("DDLW_CONV", "stock"),
                        ("DDLW_DISABLE_HIP_OPS", "1")):
        for k in calls:
            calls[k] = 0
        monkeypatch.setenv(name, value)
        assert not mbconv.inverted_residual_train_fusable(blk, x), name
        if name == "DDLW_DISABLE_HIP_OPS":
            # stock BatchNorm does not take bf16 activations with fp32
            # buffers: off the gate, step the block's marked expand conv
            _block_step(blk.conv[0], x)
        else:
            y_off, _ = _block_step(blk, x)
        if name == "DDLW_PW_TRAIN":
            inner = blk.conv(x)
            assert torch.equal(y_off, x + inner if blk.use_res else inner)
        monkeypatch.delenv(name)
        assert not any(calls[n] for n in NEW_FUNCTIONS), (name, calls)


# --------------------------------------------------------------------------- #
# 6. model
# --------------------------------------------------------------------------- #


@pytest.mark.gpu
def test_fine_tune_model_on_pointwise_training_kernels(monkeypatch):
    from ddlw_amd.ops.layers import softmax_cross_entropy

    _clear_env(monkeypatch)
    dev = _dev()
    torch.manual_seed(42)
    model = build_model(64, 64, 3, 5, dropout=0.0, fine_tune_at=13)
    m = _to_bf16_convs(model.to(dev)).train()
    g = torch.Generator(device="cpu").manual_seed(43)
    x = _bf16_randn(8, 3, 64, 64, g=g).to(dev).contiguous(memory_format=torch.channels_last)
    labels = torch.randint(0, 5, (8,), generator=g).to(dev)
    calls = _count_calls(monkeypatch, BLOCK_COUNTED)
    loss = softmax_cross_entropy(m(x), labels)
    assert calls["pw_conv_fwd_stats"] == 7 * 2, calls   # seven blocks x two stages
    assert calls["bn_stats"] == 7 + 1, calls            # depthwise BNs + the tail BN
    assert calls["pw_conv_train_fwd"] == 1, calls       # the tail conv, _PointwiseFn
    assert calls["pw_conv_fwd"] == 10 * 2 - 1, calls    # the frozen prefix only
    loss.backward()
    torch.cuda.synchronize()
    # features[13]'s expand conv gets its input from the no_grad prefix
    assert calls["pw_conv_dgrad"] == 7 * 2 + 1 - 1, calls
    assert calls["pw_conv_wgrad"] == 7 * 2 + 1, calls
    for name, p in m.base.base.features.named_parameters():
        idx = int(name.split(".")[0])
        if idx < 13:
            assert p.grad is None, name
        else:
            assert p.grad is not None, name
            assert torch.isfinite(p.grad.float()).all(), name
            assert p.grad.float().abs().max().item() > 0, name


# --------------------------------------------------------------------------- #
# 7. CPU: the gate, the opt-in mark, unchanged keys
# --------------------------------------------------------------------------- #


class _FakeCudaBf16:
    """Stands in for a CUDA bf16 activation so the gate's other conditions
    can be checked without a GPU."""
    is_cuda = True
    dtype = torch.bfloat16


def test_train_gate(monkeypatch):
    _clear_env(monkeypatch)
    blk = InvertedResidual(16, 24, 2, 6).train()
    fake = _FakeCudaBf16()
    assert mbconv.inverted_residual_train_fusable(blk, fake)
    assert not mbconv.inverted_residual_train_fusable(blk, torch.randn(1, 16, 4, 4))
    assert not mbconv.inverted_residual_train_fusable(
        blk, torch.randn(1, 16, 4, 4).to(torch.bfloat16))
    blk.eval()
    assert not mbconv.inverted_residual_train_fusable(blk, fake)
    blk.train()
    for name, value in (("DDLW_PW_TRAIN", "0"), ("DDLW_CONV", "stock"),
                        ("DDLW_DISABLE_HIP_OPS", "1")):
        monkeypatch.setenv(name, value)
        assert not mbconv.inverted_residual_train_fusable(blk, fake), name
        monkeypatch.delenv(name)
    assert mbconv.inverted_residual_train_fusable(blk, fake)
    blk.conv[1].running_mean = blk.conv[1].running_mean.to(torch.bfloat16)
    assert not mbconv.inverted_residual_train_fusable(blk, fake)


def test_cpu_training_block_is_the_module_composition(monkeypatch):
    _clear_env(monkeypatch)
    torch.manual_seed(5)
    x = torch.randn(2, 24, 9, 9)
    blk = InvertedResidual(24, 24, 1, 6).train()
    ref = copy.deepcopy(blk)
    assert torch.equal(blk(x), x + ref.conv(x))


def test_opt_in_mark():
    """Every 1x1 conv of MobileNetV2 (1 project conv of the t=1 block, 16 x 2
    of the expanded blocks, the tail: 34) carries the mark and is a shape the
    kernels take; nothing else does; ResNet-50 does not opt in."""
    convs = [m for m in MobileNetV2().modules() if isinstance(m, Conv2d)]
    pointwise = [m for m in convs if m.kernel_size == (1, 1)]
    assert len(pointwise) == 1 + 16 * 2 + 1
    assert all(m.pw_train and m.pw_trainable() for m in pointwise)
    assert not any(m.pw_train or m.pw_trainable() for m in convs if m.kernel_size != (1, 1))
    marked_copy = [m for m in copy.deepcopy(MobileNetV2()).modules()
                   if isinstance(m, Conv2d) and m.pw_train]
    assert len(marked_copy) == len(pointwise)
    res_convs = [m for m in build_resnet50(num_classes=10).modules()
                 if isinstance(m, torch.nn.Conv2d)]
    assert len(res_convs) > 50
    assert not any(getattr(m, "pw_train", False) for m in res_convs)
    assert not any(m.pw_trainable() for m in res_convs if isinstance(m, Conv2d))


def test_measured_routing_rows(monkeypatch):
    """The table's losers (docs/KERNELS.md) go to the library at their measured
    row count, their neighbours and every small shape stay on our kernels;
    DDLW_CONV=hip forces our kernels."""
    from ddlw_amd.ops.binding import pw_train_route

    _clear_env(monkeypatch)
    losers = [("wgrad", 32, 16, 802816), ("wgrad", 24, 144, 200704),
              ("wgrad", 144, 24, 200704), ("fwd", 96, 24, 200704),
              ("fwd", 960, 160, 3136), ("fwd", 960, 320, 3136),
              ("dgrad", 160, 960, 3136), ("dgrad", 320, 1280, 3136)]
    for row in losers:
        assert not pw_train_route(*row), row
    winners = [("fwd", 32, 16, 802816), ("dgrad", 32, 16, 802816),
               ("wgrad", 16, 96, 802816), ("wgrad", 96, 24, 200704),
               ("dgrad", 96, 24, 200704), ("fwd", 24, 144, 200704),
               ("fwd", 576, 160, 3136), ("dgrad", 576, 160, 3136),
               ("dgrad", 960, 160, 3136), ("dgrad", 960, 320, 3136),
               ("wgrad", 960, 320, 3136), ("fwd", 320, 1280, 3136),
               ("wgrad", 320, 1280, 3136), ("fwd", 160, 960, 3136)]
    for row in winners:
        assert pw_train_route(*row), row
    for direction in ("fwd", "dgrad", "wgrad"):
        for c, k, m in ((960, 160, 32), (160, 960, 32), (24, 144, 162), (144, 24, 162),
                        (96, 24, 50), (320, 1280, 32), (32, 16, 128)):
            assert pw_train_route(direction, c, k, m), (direction, c, k, m)
        assert not pw_train_route(direction, 3, 32, 1000)
    with pytest.raises(ValueError):
        pw_train_route("bwd", 32, 16, 128)
    monkeypatch.setenv("DDLW_CONV", "hip")
    assert all(pw_train_route(*row) for row in losers)
    assert not pw_train_route("fwd", 3, 32, 1000)


def test_state_dict_keys_unchanged_by_switch(monkeypatch):
    _clear_env(monkeypatch)
    keys = list(build_model().state_dict())
    monkeypatch.setenv("DDLW_PW_TRAIN", "0")
    assert keys == list(build_model().state_dict())
    assert len(keys) == 314
    assert not [k for k in keys if "pw_train" in k]
    feats = build_model().base.base.features
    assert len(feats) == 23 and isinstance(feats[20], Conv2d)
