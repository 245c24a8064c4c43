"""GPU tests for the prefetched bounce epilogue of the conv dgrad
(the ``PF`` instantiations of ``k_conv_fwd_igemm``, lever
``DDLW_EPI_PREFETCH``): the side reads (acc, acc_mask, bnb x, bnb mask) run
ahead of their use, and the T > 4 early add comes from a coalesced fp32
bounce. Neither changes a bit of dx or of the (dbeta, dgamma) partials.

Shapes: N=2, H=W=9, so M=162 = one full 128-row tile plus a 34-row tail
(there one store-loop iteration is partly live, the later ones and the whole
second wave row are dead: every prefetch predicate is exercised). 1x1
convs; T = dy channels / 64 K-steps picks the tile: T=1 one LDS buffer,
T>1 two, T>4 the early (fp32) add. dx channels pick BN and the N-tile tail
(136 = 128 + 8, 72 = 64 + 8: the second N tile has one live 8-channel chunk).

The early add without ``acc_mask`` is not routed to the new path (its
partials came out one bit off, docs/KERNELS.md): for the two 512-channel
cases without a mask both levers run the in-order kernel, and the tests hold
that route to the same assertions.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, HW = 2, 9

# (dy channels, dx channels)
CASES = [
    (64, 136),   # T=1, one buffer, BN=128, N-tile tail of 8
    (64, 72),    # T=1, one buffer, BN=64, tail
    (128, 128),  # T=2, two buffers
    (256, 64),   # T=4, two buffers
    (512, 136),  # T=8, early add, tail
    (512, 64),   # T=8, early add
]


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


_cache = {}


def _run(monkeypatch, case, masked):
    """Both levers on one case, plus the references computed by the
    in-order code (lever 0): the dgrad with a host-pre-masked acc and no
    bnb, and the standalone reduce over it. Cached: shared by the tests."""
    key = (case, masked)
    if key in _cache:
        return _cache[key]
    from ddlw_amd.ops import binding, conv_gemm

    kdy, cdx = case
    shape = (N, cdx, HW, HW)
    torch.manual_seed(100 + kdy + cdx + int(masked))
    w = _rand(kdy, cdx, 1, 1, scale=0.1)
    dy = _rand(N, kdy, HW, HW)
    a = _rand(*shape)
    m = _rand_mask(*shape) if masked else None
    x_bn = _rand(*shape)
    mean = torch.randn(cdx, device=_cuda())
    rstd = torch.rand(cdx, device=_cuda()) + 0.5
    m2 = _rand_mask(*shape)
    out = {}
    for lever in ("0", "1"):
        monkeypatch.setenv("DDLW_EPI_PREFETCH", lever)
        out[lever] = conv_gemm.conv_dgrad_kernel(
            dy, w, shape, 0, 1, acc=a, acc_mask=m,
            bnb=(x_bn, m2, mean, rstd))
    monkeypatch.setenv("DDLW_EPI_PREFETCH", "0")
    a0 = a if m is None else _cl(
        torch.where(_bits(m, *shape), a, torch.zeros_like(a)))
    ref = conv_gemm.conv_dgrad_kernel(dy, w, shape, 0, 1, acc=a0)
    red = binding.bn_bwd_reduce(ref, m2, x_bn, mean, rstd, True)
    torch.cuda.synchronize()
    monkeypatch.delenv("DDLW_EPI_PREFETCH")
    _cache[key] = (out, ref, red)
    return _cache[key]


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}to{c[1]}")
def test_prefetch_lever_bit_equal(monkeypatch, case, masked):
    """DDLW_EPI_PREFETCH=0 and =1: dx, both partial buffers and nparts."""
    out, _, _ = _run(monkeypatch, case, masked)
    dx0, parts0, np0 = out["0"]
    dx1, parts1, np1 = out["1"]
    assert np0 == np1
    assert torch.equal(dx0, dx1)
    assert torch.equal(parts0, parts1)


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}to{c[1]}")
def test_prefetch_against_unfused(monkeypatch, case, masked):
    """New path: dx is the dgrad with a host-pre-masked acc, bit for bit;
    (dbeta, dgamma) from the partials match the standalone reduce over that
    dx (bound of test_masked_acc_with_bnb)."""
    from ddlw_amd.ops import binding

    out, ref, (db_u, dg_u) = _run(monkeypatch, case, masked)
    dx, parts, np_ = out["1"]
    assert torch.equal(dx, ref)
    db_f, dg_f = binding.bn_grad_finalize_parts(parts[0], parts[1], np_,
                                                case[1])
    sb = db_u.abs().max() + 1e-3
    sg = dg_u.abs().max() + 1e-3
    eb = ((db_f - db_u).abs().max() / sb).item()
    eg = ((dg_f - dg_u).abs().max() / sg).item()
    print(f"bnb {case} masked={masked}: dbeta {eb:.3e} dgamma {eg:.3e}")
    assert eb < 1e-3 and eg < 1e-3


def test_lever_values(monkeypatch):
    """``epi_prefetch_enabled`` mirrors what the launcher reads per call."""
    from ddlw_amd.ops import conv_gemm

    monkeypatch.delenv("DDLW_EPI_PREFETCH", raising=False)
    assert conv_gemm.epi_prefetch_enabled()
    for val, on in (("0", False), ("1", True)):
        monkeypatch.setenv("DDLW_EPI_PREFETCH", val)
        assert conv_gemm.epi_prefetch_enabled() is on
