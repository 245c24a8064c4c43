"""The split-reduction pointwise conv kernel (``hip/pointwise_deep.hip``)
against the fp64 product of the bf16 inputs with the epilogue in fp64.

Bound, elementwise, derived and not tuned:
  |y - ref| <= 2^-8 |pre| + (depth + 8) 2^-23 (|scale| (|x| |w|^T) + |bias| + |res|)
``pre`` is the fp64 pre-activation. The first term is the one rounding to
bf16 (8 significant bits: at most 2^-8 relative, 2^-9 on average); the second
is the fp32 recursive-sum bound over the reduction and the epilogue's few
operations, doubled, which also covers that the rounding is taken of the fp32
value and not of ``pre``. ReLU and ReLU6 are 1-Lipschitz, so the bound passes
through them. (A plain fp32 product on the CPU reaches 0.6-0.98 of it.)
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (C, K, M): 18 steps split 5/5/4/4 with an M tail; a 32-deep step with an
# 8-channel tail, one row; two waves with no step at all; two N tiles with a
# K tail and more than one row tile at either mr; the deepest loop on exactly
# one 16-row fragment
SHAPES = [(576, 160, 33), (520, 40, 1), (64, 96, 35), (960, 328, 70), (1280, 320, 16)]
CASES = ([(s, 2) for s in SHAPES] + [(s, None) for s in SHAPES] + [(SHAPES[0], 1)])


def _inputs(C, K, M, seed=0):
    """CPU bf16 x [M,C], w [K,C], res [M,K] and fp32 scale, bias [K]. The
    product is ~N(0, C); scale ~3/sqrt(C) and bias ~3 put the pre-activation
    at ~N(3, 3.2^2): ~17% below 0, ~65% in (0,6), ~17% above 6."""
    g = torch.Generator(device="cpu").manual_seed(C * 7 + K + M + seed)
    x = torch.randn(M, C, generator=g).to(torch.bfloat16)
    w = torch.randn(K, C, generator=g).to(torch.bfloat16)
    res = torch.randn(M, K, generator=g).to(torch.bfloat16)
    scale = torch.empty(K).uniform_(0.9, 1.1, generator=g) * 3.0 / C ** 0.5
    bias = torch.empty(K).uniform_(2.8, 3.2, generator=g)
    return x, w, res, scale, bias


def _assert_bound(y, x, w, res, scale, bias, act, what, regions=False):
    """y (device) against the fp64 reference of the CPU operands; ``None``
    operands are absent (scale 1, bias 0, no residual)."""
    M, C = x.shape
    K = w.shape[0]
    sc = torch.ones(K, dtype=torch.float64) if scale is None else scale.double()
    bi = torch.zeros(K, dtype=torch.float64) if bias is None else bias.double()
    rs = torch.zeros(M, K, dtype=torch.float64) if res is None else res.double()
    pre = (x.double() @ w.double().t()) * sc + bi + rs
    ref = pre if not act else pre.clamp(min=0.0, max=6.0 if act == 2 else None)
    bound = (2.0 ** -8 * pre.abs() + (C + 8) * 2.0 ** -23
             * (sc.abs() * (x.double().abs() @ w.double().abs().t()) + bi.abs() + rs.abs()))
    if regions:
        for name, cnt in (("<0", (pre < 0).sum()), ("(0,6)", ((pre > 0) & (pre < 6)).sum()),
                          (">6", (pre > 6).sum())):
            assert cnt.item() / pre.numel() >= 0.05, (what, name, cnt.item())
    assert y.shape == (M, K) and y.dtype == torch.bfloat16
    y = y.cpu().double()
    assert torch.isfinite(y).all(), what
    worst = ((y - ref).abs() / bound.clamp(min=1e-300)).max().item()
    print(f"{what}: max |y-ref| / bound = {worst:.3f}")
    assert ((y - ref).abs() <= bound).all(), (what, worst)


@pytest.mark.parametrize("mr", [1, 2])
@pytest.mark.parametrize("shape,act", CASES,
                         ids=["c%d_k%d_m%d_%s" % (*s, a) for s, a in CASES])
def test_forward(shape, act, mr):
    """act 2 / 1: scale, bias, residual and the activation; None: plain."""
    from ddlw_amd.ops import binding

    x, w, res, scale, bias = _inputs(*shape)
    if act is None:
        res = scale = bias = None
    dev = torch.device("cuda:0")
    y = binding.pw_conv_deep_fwd(
        x.to(dev), w.to(dev), None if scale is None else scale.to(dev),
        None if bias is None else bias.to(dev), act or 0,
        None if res is None else res.to(dev), mr=mr)
    _assert_bound(y, x, w, res, scale, bias, act or 0, f"deep fwd {shape} act={act} mr={mr}",
                  regions=act == 2)


@pytest.mark.parametrize("mr", [1, 2])
@pytest.mark.parametrize("shape", [(520, 40, 33), (64, 96, 35)], ids=lambda s: "c%d_k%d_m%d" % s)
def test_tails_do_not_leak(shape, mr):
    """x, w, res and y are row slices out of the middle of larger buffers: NaN
    around the inputs must not reach the result, the sentinels around y must
    survive."""
    from ddlw_amd.ops import binding

    C, K, M = shape
    PAD = 40
    x, w, res, scale, bias = _inputs(C, K, M, seed=1)
    dev = torch.device("cuda:0")

    def embed(t, pad):
        buf = torch.full((t.shape[0] + 2 * pad, t.shape[1]), float("nan"),
                         dtype=torch.bfloat16, device=dev)
        buf[pad:pad + t.shape[0]] = t.to(dev)
        return buf[pad:pad + t.shape[0]]

    ybuf = torch.full((M + 2 * PAD, K), -1234.0, dtype=torch.bfloat16, device=dev)
    before = ybuf.clone()
    y = binding.pw_conv_deep_fwd(embed(x, PAD), embed(w, 8), scale.to(dev), bias.to(dev),
                                 0, embed(res, PAD), out=ybuf[PAD:PAD + M], mr=mr)
    assert y.data_ptr() == ybuf[PAD].data_ptr()
    _assert_bound(y, x, w, res, scale, bias, 0, f"deep tails {shape} mr={mr}")
    assert torch.equal(ybuf[:PAD], before[:PAD])
    assert torch.equal(ybuf[PAD + M:], before[PAD + M:])


@pytest.mark.parametrize("mr", [1, 2])
def test_deterministic(mr):
    from ddlw_amd.ops import binding

    dev = torch.device("cuda:0")
    x, w, res, scale, bias = (t.to(dev) for t in _inputs(960, 160, 162))
    a = binding.pw_conv_deep_fwd(x, w, scale, bias, 2, res, mr=mr)
    b = binding.pw_conv_deep_fwd(x, w, scale, bias, 2, res, mr=mr)
    assert torch.equal(a, b)


@pytest.mark.parametrize("mr", [1, 2])
@pytest.mark.parametrize("shape", [(576, 160, 33), (960, 328, 70), (64, 96, 1)],
                         ids=lambda s: "c%d_k%d_m%d" % s)
def test_statistics(shape, mr):
    """The partial sums are fp32 sums of exact bf16 values: M * 2^-24 relative
    to sum|y| (2^-23 for the squares, each rounded once more)."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import query

    C, K, M = shape
    dev = torch.device("cuda:0")
    x, w = (t.to(dev) for t in _inputs(C, K, M, seed=2)[:2])
    nparts_q = int(query("pw_conv_deep_nparts", M, mr, None))
    assert nparts_q == -(-M // (16 * mr))
    PAD = 2
    buf = torch.full((2, nparts_q + 2 * PAD, K), -1234.0, dtype=torch.float32, device=dev)
    before = buf.clone()
    parts = (buf[0, PAD:PAD + nparts_q], buf[1, PAD:PAD + nparts_q])
    y, ps, pq, nparts = binding.pw_conv_deep_fwd_stats(x, w.view(K, C, 1, 1), parts=parts, mr=mr)
    assert nparts == nparts_q
    assert ps.data_ptr() == parts[0].data_ptr() and pq.data_ptr() == parts[1].data_ptr()
    assert torch.equal(y, binding.pw_conv_deep_fwd(x, w, mr=mr))
    assert torch.equal(buf[:, :PAD], before[:, :PAD])
    assert torch.equal(buf[:, PAD + nparts:], before[:, PAD + nparts:])
    y64 = y.double()
    err_s = (ps.double().sum(0) - y64.sum(0)).abs()
    err_q = (pq.double().sum(0) - (y64 * y64).sum(0)).abs()
    assert (err_s <= M * 2.0 ** -24 * y64.abs().sum(0)).all(), err_s.max().item()
    assert (err_q <= M * 2.0 ** -23 * (y64 * y64).sum(0)).all(), err_q.max().item()


def test_routing(monkeypatch):
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import launch

    C, K, M = 960, 160, 3136
    dev = torch.device("cuda:0")
    x, w, res, scale, bias = (t.to(dev) for t in _inputs(C, K, M))

    monkeypatch.setenv("DDLW_PW_DEEP", "1")
    mr = binding.pw_deep_route(C, K, M)
    assert mr in (1, 2)
    assert torch.equal(binding.pw_conv_fwd(x, w, scale, bias, 2, res),
                       binding.pw_conv_deep_fwd(x, w, scale, bias, 2, res, mr=mr))
    # dgrad of the 160 -> 960 conv with weight w^T [960,160,1,1]: x stands in
    # for dy [M, 960], the GEMM's weights are (w^T)^T = w, its depth is 960
    weight = w.t().contiguous().view(C, K, 1, 1)
    dx = binding.pw_conv_dgrad(x, weight, (M, K), acc=res)
    assert torch.equal(dx, binding.pw_conv_deep_fwd(x, w, res=res, mr=mr))
    assert binding.pw_deep_route(320, 1280, M) is None

    monkeypatch.setenv("DDLW_PW_DEEP", "0")
    assert binding.pw_deep_route(C, K, M) is None
    assert binding.pw_deep_route(320, 1280, M) is None
    plain = torch.empty(M, K, dtype=torch.bfloat16, device=dev)
    launch("pw_conv_fwd", x, w, plain, res, scale, bias, 2, M, C, K)
    assert torch.equal(binding.pw_conv_fwd(x, w, scale, bias, 2, res), plain)

    monkeypatch.delenv("DDLW_PW_DEEP")
    assert binding.pw_deep_route(320, 1280, M) is None
