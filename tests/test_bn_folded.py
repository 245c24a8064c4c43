"""GPU tests for the fold + finalize of a large BatchNorm partial set in one
launch (``hip/bn_folded.hip``, ``DDLW_BN_FOLDED=1``): bit-equal to
``k_bn_parts_fold`` followed by the finalize kernel, on one stream, twice in a
row and on a second stream, and the ticket counters are zero afterwards.

Sizes: C = 8 (a partial 32-channel block), 64 (two blocks), 96 (not a
multiple of 32), 256 (many blocks); nparts = 513 and 520 (just above the
512-row threshold), 4099 (not a multiple of 8 * G), 12544 (the flagship's
largest count). With G from ``binding._fold_groups`` one channel group has up
to 512 blocks, more than one XCD holds at once."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CS = (8, 64, 96, 256)
NPARTS = (513, 520, 4099, 12544)
ROWS, EPS, MOMENTUM = 802816, 1e-5, 0.1

_base = {}


def _cuda():
    return torch.device("cuda:0")


def _parts(nparts, C):
    """A pair of contiguous fp32 [nparts, C] partial arrays, cut from one
    random block that every case shares."""
    if "p" not in _base:
        g = torch.Generator(device="cpu").manual_seed(7)
        _base["p"] = torch.randn(2, max(NPARTS), max(CS), generator=g).to(_cuda())
    p = _base["p"][:, :nparts, :C].contiguous()
    return p[0], p[1]


def _running(C):
    g = torch.Generator(device="cpu").manual_seed(11)
    rm = torch.randn(C, generator=g).to(_cuda())
    rv = (torch.rand(C, generator=g) + 0.5).to(_cuda())
    return rm, rv


def _two_kernel_stats(ps, pq, nparts, C):
    """k_bn_parts_fold + k_bn_finalize through the old exports."""
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import launch

    G = binding._fold_groups(C)
    stage = torch.empty(2, G, C, dtype=torch.float32, device=_cuda())
    mean = torch.empty(C, dtype=torch.float32, device=_cuda())
    rstd = torch.empty_like(mean)
    rm, rv = _running(C)
    launch("bn_parts_fold", ps, pq, stage[0], stage[1], nparts, C, G)
    launch("bn_finalize", stage[0], stage[1], mean, rstd, rm, rv, ROWS, C, G,
           EPS, MOMENTUM)
    return mean, rstd, rm, rv


def _two_kernel_grad(pb, pg, nparts, C):
    from ddlw_amd.ops import binding
    from ddlw_amd.ops.runtime import launch

    G = binding._fold_groups(C)
    stage = torch.empty(2, G, C, dtype=torch.float32, device=_cuda())
    dbeta = torch.empty(C, dtype=torch.float32, device=_cuda())
    dgamma = torch.empty_like(dbeta)
    launch("bn_parts_fold", pb, pg, stage[0], stage[1], nparts, C, G)
    launch("bn_grad_finalize", stage[0], stage[1], dbeta, dgamma, C, G)
    return dbeta, dgamma


def _folded_stats(ps, pq, nparts, C):
    from ddlw_amd.ops import binding

    rm, rv = _running(C)
    mean, rstd = binding.bn_finalize_parts(ps, pq, nparts, ROWS, C, EPS,
                                           MOMENTUM, rm, rv)
    return mean, rstd, rm, rv


def _folded_grad(pb, pg, nparts, C):
    from ddlw_amd.ops import binding

    return binding.bn_grad_finalize_parts(pb, pg, nparts, C)


def _assert_equal(got, ref, what):
    for i, (g, r) in enumerate(zip(got, ref)):
        assert torch.equal(g, r), f"{what}: output {i} differs"


def _assert_tickets_zero():
    from ddlw_amd.ops import runtime

    torch.cuda.synchronize()
    assert runtime._tickets, "no ticket buffer was created"
    for key, t in runtime._tickets.items():
        assert int(t.abs().sum()) == 0, f"ticket buffer {key} is not zero"


@pytest.mark.parametrize("nparts", NPARTS)
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("variant", ["stats", "grad"])
def test_folded_equals_fold_plus_finalize(monkeypatch, variant, C, nparts):
    monkeypatch.setenv("DDLW_BN_FOLDED", "1")
    p0, p1 = _parts(nparts, C)
    two, folded = ((_two_kernel_stats, _folded_stats) if variant == "stats"
                   else (_two_kernel_grad, _folded_grad))
    ref = two(p0, p1, nparts, C)
    # twice in a row on one stream: the second call finds the counters the
    # first one left
    _assert_equal(folded(p0, p1, nparts, C), ref, "first call")
    _assert_equal(folded(p0, p1, nparts, C), ref, "second call")
    side = torch.cuda.Stream(_cuda())
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = folded(p0, p1, nparts, C)
    torch.cuda.current_stream().wait_stream(side)
    _assert_equal(got, ref, "second stream")
    _assert_tickets_zero()


def _sentinel_tickets():
    """Every ticket buffer (at least the current stream's) set to 7: a folded
    launch would move it."""
    from ddlw_amd.ops import runtime

    runtime.ticket_buffer(_cuda())
    for t in runtime._tickets.values():
        t.fill_(7)
    torch.cuda.synchronize()


def _tickets_untouched_then_zeroed():
    from ddlw_amd.ops import runtime

    torch.cuda.synchronize()
    ok = all(bool((t == 7).all()) for t in runtime._tickets.values())
    for t in runtime._tickets.values():
        t.zero_()
    torch.cuda.synchronize()
    return ok


@pytest.mark.parametrize("C", CS)
def test_512_parts_take_the_plain_finalize(monkeypatch, C):
    """nparts = 512 is below the threshold: the finalize kernels read the
    partials directly and no ticket is drawn."""
    from ddlw_amd.ops.runtime import launch

    monkeypatch.setenv("DDLW_BN_FOLDED", "1")
    p0, p1 = _parts(512, C)
    mean = torch.empty(C, dtype=torch.float32, device=_cuda())
    rstd = torch.empty_like(mean)
    rm, rv = _running(C)
    launch("bn_finalize", p0, p1, mean, rstd, rm, rv, ROWS, C, 512, EPS, MOMENTUM)
    dbeta, dgamma = torch.empty_like(mean), torch.empty_like(mean)
    launch("bn_grad_finalize", p0, p1, dbeta, dgamma, C, 512)
    _sentinel_tickets()
    try:
        got_s = _folded_stats(p0, p1, 512, C)
        got_g = _folded_grad(p0, p1, 512, C)
    finally:
        untouched = _tickets_untouched_then_zeroed()
    assert untouched
    _assert_equal(got_s, (mean, rstd, rm, rv), "stats")
    _assert_equal(got_g, (dbeta, dgamma), "grad")


@pytest.mark.parametrize("lever", ["0", None])
def test_lever_off_restores_two_launches(monkeypatch, lever):
    """DDLW_BN_FOLDED=0 or unset, read per call: fold + finalize, no ticket
    drawn."""
    if lever is None:
        monkeypatch.delenv("DDLW_BN_FOLDED", raising=False)
    else:
        monkeypatch.setenv("DDLW_BN_FOLDED", lever)
    C, nparts = 96, 4099
    p0, p1 = _parts(nparts, C)
    _sentinel_tickets()
    try:
        got_s = _folded_stats(p0, p1, nparts, C)
        got_g = _folded_grad(p0, p1, nparts, C)
    finally:
        untouched = _tickets_untouched_then_zeroed()
    assert untouched
    _assert_equal(got_s, _two_kernel_stats(p0, p1, nparts, C), "stats")
    _assert_equal(got_g, _two_kernel_grad(p0, p1, nparts, C), "grad")


def test_small_ticket_buffer_is_refused():
    """A ticket buffer with fewer than ceil(C/32) counters: refused by the
    launcher, no kernel runs."""
    from ddlw_amd.ops.runtime import KernelLibError, launch

    C, nparts, G = 96, 520, 8
    p0, p1 = _parts(nparts, C)
    stage = torch.empty(2, G, C, dtype=torch.float32, device=_cuda())
    ticket = torch.zeros(2, dtype=torch.int32, device=_cuda())
    out = torch.empty(2, C, dtype=torch.float32, device=_cuda())
    with pytest.raises(KernelLibError, match="ticket"):
        launch("bn_grad_finalize_folded", p0, p1, stage, ticket, 2, out[0],
               out[1], C, nparts, G)
    torch.cuda.synchronize()
    assert int(ticket.sum()) == 0
