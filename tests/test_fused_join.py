"""GPU tests for the residual join without ``dres`` (masked accumulate in
the conv epilogue, ``DDLW_FUSED_JOIN``) and for bn3's (dbeta, dgamma)
partials coming from the next block's conv1 dgrad (``DDLW_FUSED_BN3``).

Kernel shapes: N=3, H=W=7, so M=147 = one full 128-row tile plus a 19-row
tail; channel counts pick the epilogue (T = R*S*C/64 K-steps: T<=4 is the
LDS-bounce epilogue, above it the direct one; bnb always bounces)."""
import copy
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu

N, HW = 3, 7


def _cuda():
    return torch.device("cuda:0")


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rand(*shape, scale=1.0):
    return _cl((torch.randn(*shape, device=_cuda()) * scale).to(torch.bfloat16))


def _rand_mask(n, c, h, w):
    return torch.randint(0, 256, (n * h * w * (c // 8),), dtype=torch.uint8,
                         device=_cuda())


def _bits(mask, n, c, h, w):
    """Byte mask (byte = NHWC index >> 3, bit = channel & 7) -> bool NCHW."""
    sh = torch.arange(8, device=mask.device, dtype=torch.uint8)
    b = ((mask[:, None] >> sh) & 1).bool().reshape(n, h, w, c)
    return b.permute(0, 3, 1, 2)


# (dy channels, dx channels, R, pad)
DGRAD_CASES = [
    (64, 72, 1, 0),    # T=1: LDS bounce, one LDS buffer, N-tile tail (72 = 64 + 8)
    (320, 64, 1, 0),   # T=5: direct epilogue
    (64, 128, 3, 1),   # T=9: direct epilogue, 3x3
]


def _dgrad_inputs(kdy, cdx, r, seed):
    torch.manual_seed(seed)
    w = _rand(kdy, cdx, r, r, scale=0.1)
    dy = _rand(N, kdy, HW, HW)
    a = _rand(N, cdx, HW, HW)
    m = _rand_mask(N, cdx, HW, HW)
    return w, dy, a, m


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_masked_acc_is_exact(case):
    """acc + acc_mask == acc pre-masked on the host, bit for bit."""
    from ddlw_amd.ops import conv_gemm

    kdy, cdx, r, pad = case
    w, dy, a, m = _dgrad_inputs(kdy, cdx, r, 21)
    shape = (N, cdx, HW, HW)
    got = conv_gemm.conv_dgrad_kernel(dy, w, shape, pad, 1, acc=a, acc_mask=m)
    a0 = _cl(torch.where(_bits(m, *shape), a, torch.zeros_like(a)))
    ref = conv_gemm.conv_dgrad_kernel(dy, w, shape, pad, 1, acc=a0)
    assert torch.equal(got, ref)
    # the mask did something: the unmasked sum differs
    full = conv_gemm.conv_dgrad_kernel(dy, w, shape, pad, 1, acc=a)
    assert not torch.equal(got, full)


def test_masked_acc_bad_arguments():
    """acc_mask without acc, or together with the eval fold, is refused by
    the launcher (no kernel runs)."""
    from ddlw_amd.ops import conv_gemm
    from ddlw_amd.ops.runtime import KernelLibError

    torch.manual_seed(22)
    x = _rand(N, 64, HW, HW)
    w = _rand(64, 64, 1, 1, scale=0.1)
    a = _rand(N, 64, HW, HW)
    m = _rand_mask(N, 64, HW, HW)
    with pytest.raises(KernelLibError, match="acc_mask"):
        conv_gemm.conv_fwd_kernel(x, w, 1, 0, acc_mask=m)
    scale = torch.ones(64, device=_cuda())
    bias = torch.zeros(64, device=_cuda())
    with pytest.raises(KernelLibError, match="acc_mask"):
        conv_gemm.conv_fwd_kernel(x, w, 1, 0, acc=a, acc_mask=m,
                                  ep=(scale, bias, True))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", [c for c in DGRAD_CASES if c[2] == 1])
def test_masked_acc_with_bnb(case):
    """acc + acc_mask + bnb: dx as without bnb, (dbeta, dgamma) as the
    standalone reduce over that dx (bound of
    test_conv_dgrad_fused_bnb_parity)."""
    from ddlw_amd.ops import binding, conv_gemm

    kdy, cdx, r, pad = case
    w, dy, a, m = _dgrad_inputs(kdy, cdx, r, 23)
    shape = (N, cdx, HW, HW)
    x_bn = _rand(*shape)
    mean = torch.randn(cdx, device=_cuda())
    rstd = torch.rand(cdx, device=_cuda()) + 0.5
    m2 = _rand_mask(*shape)
    dx, parts, np_ = conv_gemm.conv_dgrad_kernel(
        dy, w, shape, pad, 1, acc=a, acc_mask=m, bnb=(x_bn, m2, mean, rstd))
    a0 = _cl(torch.where(_bits(m, *shape), a, torch.zeros_like(a)))
    ref = conv_gemm.conv_dgrad_kernel(dy, w, shape, pad, 1, acc=a0)
    assert torch.equal(dx, ref)
    db_f, dg_f = binding.bn_grad_finalize_parts(parts[0], parts[1], np_, cdx)
    db_u, dg_u = binding.bn_bwd_reduce(ref, m2, x_bn, mean, rstd, True)
    sb = db_u.abs().max() + 1e-3
    sg = dg_u.abs().max() + 1e-3
    eb = ((db_f - db_u).abs().max() / sb).item()
    eg = ((dg_f - dg_u).abs().max() / sg).item()
    print(f"bnb {case}: dbeta {eb:.3e} dgamma {eg:.3e}")
    assert eb < 1e-3 and eg < 1e-3


# --------------------------------------------------------------------------- #
# block level
# --------------------------------------------------------------------------- #


def _make_block(in_ch, mid, seed, stride=1, downsample=False):
    from ddlw_amd.models.resnet import Bottleneck, Downsample

    torch.manual_seed(seed)
    ds = Downsample(in_ch, mid * 4, stride) if downsample else None
    blk = Bottleneck(in_ch, mid, stride=stride, downsample=ds)
    bns = [blk.bn1, blk.bn2, blk.bn3] + ([ds.bn] if ds else [])
    for bn in bns:
        torch.nn.init.uniform_(bn.weight, 0.5, 1.5)
        torch.nn.init.uniform_(bn.bias, -0.2, 0.2)
    blk = blk.to(_cuda()).to(memory_format=torch.channels_last)
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            m.to(torch.bfloat16)
    return blk.train()


def _block_input():
    torch.manual_seed(31)
    return _rand(4, 256, 8, 8)


def _grads(mods):
    return {f"{i}.{n}": p.grad.clone() for i, m in enumerate(mods)
            for n, p in m.named_parameters()}


@pytest.mark.parametrize("downsample", [False, True])
def test_fused_join_block_bit_exact(monkeypatch, downsample):
    """DDLW_FUSED_JOIN=1 vs 0: output, input gradient and every parameter
    gradient bit-equal (identity block and stride-2 downsample block)."""
    monkeypatch.setenv("DDLW_CONV", "hip")
    monkeypatch.setenv("DDLW_FUSED_BN3", "0")
    blk = _make_block(256, 64, 32, stride=2 if downsample else 1,
                      downsample=downsample)
    x = _block_input()
    res = {}
    for join in ("1", "0"):
        monkeypatch.setenv("DDLW_FUSED_JOIN", join)
        b = copy.deepcopy(blk)
        xa = x.clone().requires_grad_(True)
        out = b(xa)
        out.float().square().mean().backward()
        res[join] = (out.detach(), xa.grad, _grads([b]))
    assert torch.equal(res["1"][0], res["0"][0])
    assert torch.equal(res["1"][1], res["0"][1])
    for n, g in res["0"][2].items():
        assert torch.equal(res["1"][2][n], g), n


def _make_chain():
    """identity -> identity -> stride-2 downsample, as at a stage boundary."""
    return [_make_block(256, 64, 41), _make_block(256, 64, 42),
            _make_block(256, 128, 43, stride=2, downsample=True)]


_chain_cache = {}


def _run_chain(monkeypatch, bn3, mode="plain"):
    """One forward + backward of a fresh copy of the chain. ``mode``:
    ``plain``; ``hook`` (both inter-block tensors get a gradient-doubling
    hook); ``hook1`` (only the first one); ``fork`` (both inter-block
    tensors also feed ``.float().sum()``). Returns (out, dx, grads, the
    channel counts of every standalone bn_bwd_reduce call). Cached: every
    run is deterministic, and the references are shared between tests."""
    key = (bn3, mode)
    if key in _chain_cache:
        return _chain_cache[key]
    from ddlw_amd.ops import binding

    monkeypatch.setenv("DDLW_CONV", "hip")
    monkeypatch.setenv("DDLW_FUSED_BN3", bn3)
    if "chain" not in _chain_cache:
        _chain_cache["chain"] = _make_chain()
    mods = copy.deepcopy(_chain_cache["chain"])
    calls = []
    real = binding.bn_bwd_reduce

    def counting(dy, mask, x, mean, rstd, relu):
        calls.append(x.shape[1])
        return real(dy, mask, x, mean, rstd, relu)

    monkeypatch.setattr(binding, "bn_bwd_reduce", counting)
    xa = _block_input().requires_grad_(True)
    h1 = mods[0](xa)
    h2 = mods[1](h1)
    out = mods[2](h2)
    loss = out.float().square().mean()
    if mode in ("hook", "hook1"):
        h1.register_hook(lambda g: g * 2)
        if mode == "hook":
            h2.register_hook(lambda g: g * 2)
    elif mode == "fork":
        loss = loss + 1e-3 * (h1.float().sum() + h2.float().sum())
    loss.backward()
    monkeypatch.setattr(binding, "bn_bwd_reduce", real)
    r = (out.detach(), xa.grad, _grads(mods), sorted(calls))
    _chain_cache[key] = r
    return r


# standalone reduces of the chain in hip mode with nothing fused across
# blocks: bn3 of the two identity blocks (256 channels), and in the
# downsample block bn3 and bn_d (512) and bn1 (128: its conv2 dgrad is
# stride 2, which has no bnb epilogue)
_REDUCES_UNFUSED = [128, 256, 256, 512, 512]
_FUSED_BN3 = ("0.bn3.", "1.bn3.")


def _close(a, b, tol, what):
    s = b.float().abs().max() + 1e-6
    err = ((a.float() - b.float()).abs().max() / s).item()
    assert err < tol, (what, err)


def _assert_chain_close(got, ref):
    assert torch.equal(got[0], ref[0])  # forward is untouched
    _close(got[1], ref[1], 2e-2, "dx")
    for n, g in ref[2].items():
        tol = 1e-3 if n.startswith(_FUSED_BN3) else 2e-2
        _close(got[2][n], g, tol, n)


def _assert_chain_equal(got, ref):
    assert torch.equal(got[0], ref[0])
    assert torch.equal(got[1], ref[1])
    for n, g in ref[2].items():
        assert torch.equal(got[2][n], g), n


def test_fused_bn3_chain(monkeypatch):
    """DDLW_FUSED_BN3=1 vs 0 on three blocks: the first two blocks, and only
    they, skip their bn3 reduce."""
    fused = _run_chain(monkeypatch, "1")
    ref = _run_chain(monkeypatch, "0")
    assert ref[3] == _REDUCES_UNFUSED
    assert fused[3] == [128, 512, 512]
    _assert_chain_close(fused, ref)


def test_fused_bn3_fallback_hook(monkeypatch):
    """A hook that rewrites the gradient between two blocks: the block
    behind it must not use the partials. With a hook on BOTH inter-block
    tensors nothing is fused, so every gradient is bit-equal to the
    DDLW_FUSED_BN3=0 run with the same hooks. (With one hook the other link
    still fuses, and its summation order differs from the unfused run's, so
    that case is held to the bounds of test_fused_bn3_chain and to the
    count of reduces instead.)"""
    got = _run_chain(monkeypatch, "1", "hook")
    ref = _run_chain(monkeypatch, "0", "hook")
    assert got[3] == _REDUCES_UNFUSED
    _assert_chain_equal(got, ref)
    got1 = _run_chain(monkeypatch, "1", "hook1")
    ref1 = _run_chain(monkeypatch, "0", "hook1")
    assert got1[3] == [128, 256, 512, 512]  # block 0 fell back, block 1 fused
    _assert_chain_close(got1, ref1)


def test_fused_bn3_fallback_second_consumer(monkeypatch):
    """Inter-block tensors that also feed another op: the gradient a block
    receives is a sum, not the dgrad's buffer — bit-equal to the unfused
    run."""
    got = _run_chain(monkeypatch, "1", "fork")
    ref = _run_chain(monkeypatch, "0", "fork")
    assert got[3] == _REDUCES_UNFUSED
    _assert_chain_equal(got, ref)


def test_fused_bn3_retain_graph(monkeypatch):
    """backward(retain_graph=True) twice: no error; the links are consumed
    by the first pass, so the second one is the unfused computation, bit for
    bit, and the first is within the fused bounds of it."""
    monkeypatch.setenv("DDLW_CONV", "hip")
    monkeypatch.setenv("DDLW_FUSED_BN3", "1")
    ref = _run_chain(monkeypatch, "0")
    monkeypatch.setenv("DDLW_FUSED_BN3", "1")
    if "chain" not in _chain_cache:
        _chain_cache["chain"] = _make_chain()
    mods = copy.deepcopy(_chain_cache["chain"])
    xa = _block_input().requires_grad_(True)
    out = xa
    for m in mods:
        out = m(out)
    loss = out.float().square().mean()
    passes = []
    for _ in range(2):
        loss.backward(retain_graph=True)
        passes.append((out.detach(), xa.grad.clone(), _grads(mods)))
        xa.grad = None
        for m in mods:
            m.zero_grad(set_to_none=True)
    _assert_chain_close(passes[0], ref)
    _assert_chain_equal(passes[1], ref)


def test_bn3_link_lifetime(monkeypatch):
    """No link outlives its graph, and none keeps memory after it: once the
    tensors and the model are gone, the allocator is back where it was."""
    monkeypatch.setenv("DDLW_CONV", "hip")
    monkeypatch.setenv("DDLW_FUSED_BN3", "1")

    def run(keep):
        mods = _make_chain()
        xa = _block_input().requires_grad_(True)
        h1 = mods[0](xa)
        h2 = mods[1](h1)
        out = mods[2](h2)
        links = [t._ddlw_bn3_link for t in (h1, h2, out)]
        # reachable from the graph and the tensor only, never from a module
        for m in mods:
            for sub in m.modules():
                assert not any(v is l for v in vars(sub).values()
                               for l in links)
        out.float().square().mean().backward()
        # consumed: no tensor reference left behind while the graph lives
        for l in links:
            assert all(getattr(l, s) is None for s in l.FIELDS)
        keep.extend(weakref.ref(l) for l in links)

    run([])  # warm-up: lazily created global buffers (zero page) exist now
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    refs = []
    run(refs)
    gc.collect()
    torch.cuda.synchronize()
    assert all(r() is None for r in refs)
    assert torch.cuda.memory_allocated() == base
