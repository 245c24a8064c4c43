"""The fused tail kernel (``hip/pointwise_gap.hip``): 1x1 conv + folded BN +
activation + global average pool, against fp64 and against the two kernels it
replaces.

Reference: ``pre`` = fp64 product of the bf16 operands with the epilogue in
fp64, ``ref = act(pre)``, ``P = mean_r ref``. Bound, elementwise, derived and
not tuned, with ``b_r`` the per-pixel bound of ``test_pw_deep.py`` at depth C:
  |p - P| <= 2^-8 |P| + (1 + 2^-8) mean_r b_r + (HW + 8) 2^-23 mean_r(|ref_r| + b_r)
The first term is the final rounding to bf16, the second the per-pixel error
of y carried through it, the third the fp32 recursive sum and the multiply.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (C, K, HW, N): the layer (pixel-tile tail, N odd against imgs); a channel
# vector tail inside a 32-step, K below one workgroup tile, exactly one pixel
# tile; the KS = 5 boundary, a K tail in a second workgroup, one pixel past a
# tile; two pixel tiles with a tail; the smallest supported shape
SHAPES = [(320, 1280, 49, 3), (136, 40, 64, 2), (160, 136, 65, 4), (320, 264, 100, 5),
          (8, 8, 1, 1)]
IDS = ["c%d_k%d_hw%d_n%d" % s for s in SHAPES]


def _inputs(C, K, HW, N, seed=0):
    """CPU bf16 x [N,HW,C], w [K,C], fp32 scale, bias [K], as ``_inputs`` of
    ``test_pw_deep.py``: pre-activation ~N(3, 3.2^2)."""
    g = torch.Generator(device="cpu").manual_seed(C * 7 + K + N * HW + seed)
    x = torch.randn(N, HW, C, generator=g).to(torch.bfloat16)
    w = torch.randn(K, C, generator=g).to(torch.bfloat16)
    scale = torch.empty(K).uniform_(0.9, 1.1, generator=g) * 3.0 / C ** 0.5
    bias = torch.empty(K).uniform_(2.8, 3.2, generator=g)
    return x, w, scale, bias


def _nchw(x):
    """[N,HW,C] rows as the channels_last [N,C,HW,1] tensor over the same memory."""
    return x.view(x.shape[0], x.shape[1], 1, x.shape[2]).permute(0, 3, 1, 2)


def _assert_bound(p, x, w, scale, bias, act, what, regions=False):
    N, HW, C = x.shape
    K = w.shape[0]
    sc = torch.ones(K, dtype=torch.float64) if scale is None else scale.double()
    bi = torch.zeros(K, dtype=torch.float64) if bias is None else bias.double()
    pre = (x.double() @ w.double().t()) * sc + bi
    ref = pre if not act else pre.clamp(min=0.0, max=6.0 if act == 2 else None)
    b = (2.0 ** -8 * pre.abs() + (C + 8) * 2.0 ** -23
         * (sc.abs() * (x.double().abs() @ w.double().abs().t()) + bi.abs()))
    P = ref.mean(1)
    bound = (2.0 ** -8 * P.abs() + (1 + 2.0 ** -8) * b.mean(1)
             + (HW + 8) * 2.0 ** -23 * (ref.abs() + b).mean(1))
    if regions:
        for name, cnt in (("<0", (pre < 0).sum()), ("(0,6)", ((pre > 0) & (pre < 6)).sum()),
                          (">6", (pre > 6).sum())):
            assert cnt.item() / pre.numel() >= 0.05, (what, name, cnt.item())
    assert p.shape == (N, K) and p.dtype == torch.bfloat16
    p = p.cpu().double()
    assert torch.isfinite(p).all(), what
    worst = ((p - P).abs() / bound.clamp(min=1e-300)).max().item()
    print(f"{what}: max |p-P| / bound = {worst:.3f}")
    assert ((p - P).abs() <= bound).all(), (what, worst)


@pytest.mark.parametrize("imgs", [1, 2])
@pytest.mark.parametrize("act", [2, None])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_fp64_and_the_pair(shape, act, imgs):
    """Within the bound of fp64, bit-equal to ``gap_fwd(pw_conv_fwd(...))``
    and to a second call."""
    from ddlw_amd.ops import binding

    x, w, scale, bias = _inputs(*shape)
    if act is None:
        scale = bias = None
    dev = torch.device("cuda:0")
    xd, wd = _nchw(x.to(dev)), w.to(dev)
    sd, bd = (None, None) if scale is None else (scale.to(dev), bias.to(dev))
    p = binding.pw_conv_gap_fwd(xd, wd, sd, bd, act or 0, imgs=imgs)
    _assert_bound(p, x, w, scale, bias, act or 0, f"pw_gap {shape} act={act} imgs={imgs}",
                  regions=act == 2 and shape != SHAPES[-1])  # 8 values: no statistics
    assert torch.equal(p, binding.gap_fwd(binding.pw_conv_fwd(xd, wd, sd, bd, act or 0)))
    assert torch.equal(p, binding.pw_conv_gap_fwd(xd, wd, sd, bd, act or 0, imgs=imgs))
    assert torch.equal(p, binding.pw_conv_gap_fwd(xd, wd, sd, bd, act or 0))


@pytest.mark.parametrize("shape", [(136, 40, 64, 2), (160, 136, 65, 4)], ids=IDS[1:3])
def test_tails_do_not_leak(shape):
    """x, w and out are row slices out of the middle of larger buffers: NaN
    around the inputs must not reach the result, the sentinels around out
    must survive."""
    from ddlw_amd.ops import binding

    C, K, HW, N = shape
    x, w, scale, bias = _inputs(*shape, seed=1)
    dev = torch.device("cuda:0")

    def embed(t, pad):
        buf = torch.full((t.shape[0] + 2 * pad, *t.shape[1:]), float("nan"),
                         dtype=torch.bfloat16, device=dev)
        buf[pad:pad + t.shape[0]] = t.to(dev)
        return buf[pad:pad + t.shape[0]]

    PAD = 3
    pbuf = torch.full((N + 2 * PAD, K), -1234.0, dtype=torch.bfloat16, device=dev)
    before = pbuf.clone()
    p = binding.pw_conv_gap_fwd(_nchw(embed(x, 1)), embed(w, 8), scale.to(dev), bias.to(dev),
                                2, out=pbuf[PAD:PAD + N], imgs=3)
    assert p.data_ptr() == pbuf[PAD].data_ptr()
    _assert_bound(p, x, w, scale, bias, 2, f"pw_gap tails {shape}")
    assert torch.equal(pbuf[:PAD], before[:PAD])
    assert torch.equal(pbuf[PAD + N:], before[PAD + N:])


def _count(monkeypatch):
    from ddlw_amd.ops import binding

    calls = []
    real = binding.pw_conv_gap_fwd
    monkeypatch.setattr(binding, "pw_conv_gap_fwd",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def _model(**kw):
    from ddlw_amd.models import build_model
    from ddlw_amd.ops import apply_bf16_policy

    torch.manual_seed(31)
    return apply_bf16_policy(build_model(32, 32, 3, 5, dropout=0.0, **kw).to("cuda:0"))


@pytest.mark.parametrize("size", [32, 96])
def test_through_the_model(monkeypatch, size):
    """A frozen ``build_model`` reaches the kernel under ``DDLW_TAIL_GAP=1``,
    once per forward, and its logits are those of ``=0``."""
    from ddlw_amd.ops import binding

    g = torch.Generator(device="cpu").manual_seed(size)
    u8 = torch.randint(0, 256, (3, size, size, 3), dtype=torch.uint8, generator=g)
    u8 = u8.to("cuda:0").permute(0, 3, 1, 2)
    m = _model().eval()
    calls = _count(monkeypatch)
    logits = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DDLW_TAIL_GAP", mode)
        assert binding.pw_gap_route(320, 1280, (size // 32) ** 2, 3) is (mode == "1")
        assert not binding.pw_gap_route(328, 1280, 49, 3)
        with torch.no_grad():
            logits[mode] = m(u8)
        assert len(calls) == int(mode)
    assert torch.isfinite(logits["1"]).all()
    assert torch.equal(logits["0"], logits["1"])


def test_trainable_tail_stays_on_the_module_path(monkeypatch):
    monkeypatch.setenv("DDLW_TAIL_GAP", "1")
    m = _model(fine_tune_at=20).train()
    calls = _count(monkeypatch)
    u8 = torch.randint(0, 256, (3, 32, 32, 3), dtype=torch.uint8).to("cuda:0")
    assert m(u8.permute(0, 3, 1, 2)).shape == (3, 5)
    assert not calls
