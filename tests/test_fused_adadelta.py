"""``k_fused_adadelta`` / ``FusedAdadelta`` on the GPU against
``torch.optim.Adadelta``. Tolerances are those of
``test_fused_adam_matches_torch_adam`` (atol 1e-5, rtol 1e-4): the library is
built ``-ffast-math``, so sqrt and the division are a few ulp off IEEE."""
import pytest
import torch

ATOL, RTOL = 1e-5, 1e-4


def _dev():
    return torch.device("cuda:0")


def _run_pair(sizes, steps, seed, **kw):
    """Same start, same grads: FusedAdadelta on one copy, stock on the other."""
    from ddlw_amd.ops import FusedAdadelta

    g = torch.Generator(device="cpu").manual_seed(seed)
    p1 = [torch.randn(n, generator=g).to(_dev()).requires_grad_(True) for n in sizes]
    p2 = [p.detach().clone().requires_grad_(True) for p in p1]
    o1 = FusedAdadelta(p1, **kw)
    o2 = torch.optim.Adadelta(p2, **kw)
    for _ in range(steps):
        for a, b in zip(p1, p2):
            gr = torch.randn(a.numel(), generator=g).to(_dev())
            a.grad, b.grad = gr.clone(), gr.clone()
        o1.step()
        o2.step()
    torch.cuda.synchronize()
    return p1, p2, o1, o2


def _assert_close(p1, p2, o1, o2):
    worst = max((a - b).abs().max().item() for a, b in zip(p1, p2))
    print(f"max |fused - torch| over {len(p1)} tensors = {worst:.3e}")
    for a, b in zip(p1, p2):
        assert torch.allclose(a, b, atol=ATOL, rtol=RTOL), a.numel()
        for k in ("square_avg", "acc_delta"):
            assert torch.allclose(o1.state[a][k], o2.state[b][k], atol=ATOL, rtol=RTOL), k


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(lr=1.0), dict(lr=0.05, weight_decay=1e-4)],
                         ids=["lr1", "lr0.05_wd"])
def test_fused_adadelta_matches_torch_adadelta(kw):
    """1, 7, 257 and 1000 elements in one group: tails, more than one block,
    several chunks in one launch."""
    _assert_close(*_run_pair([1, 7, 257, 1000], steps=4, seed=29, **kw))


@pytest.mark.gpu
def test_fused_adadelta_many_chunks_and_grid_stride():
    """70 chunks (> the 64 rows of grid.y, so blocks walk on to a second
    chunk) and one tensor of 140,000 elements (> 512 blocks x 256 threads, so
    threads take a second element)."""
    _assert_close(*_run_pair([3] * 70 + [140_000], steps=2, seed=30, lr=1.0,
                             weight_decay=1e-4))


@pytest.mark.gpu
def test_fused_adadelta_bf16_master():
    from ddlw_amd.ops import FusedAdadelta

    torch.manual_seed(31)
    base = torch.randn(512, device=_dev())
    p_bf = base.to(torch.bfloat16).requires_grad_(True)
    p_ref = base.to(torch.bfloat16).float().requires_grad_(True)
    o1 = FusedAdadelta([p_bf], lr=1.0)
    o2 = torch.optim.Adadelta([p_ref], lr=1.0)
    for _ in range(4):
        g = torch.randn(512, device=_dev())
        p_bf.grad = g.to(torch.bfloat16)
        p_ref.grad = g.to(torch.bfloat16).float()
        o1.step()
        o2.step()
    st = o1.state[p_bf]
    assert set(st) == {"master", "square_avg", "acc_delta"}
    assert all(v.dtype == torch.float32 for v in st.values())
    assert torch.allclose(st["master"], p_ref, atol=ATOL, rtol=RTOL)
    # the shadow is the master rounded once, written in the same pass
    assert torch.equal(p_bf.detach(), st["master"].to(torch.bfloat16))


@pytest.mark.gpu
def test_fused_adadelta_small_updates_survive_bf16():
    """Why the kernel exists. 4096 weights ~N(0, 0.05^2), grads ~N(0, 0.01^2),
    lr 1e-3, 20 steps: the per-step update (~5e-7) is far below one bf16 ulp
    of a 0.05 weight (~2e-4), and stock Adadelta on bf16 parameters leaves
    96.8 % of them where they started. The fp32 master moves all of them and
    tracks fp32 Adadelta."""
    from ddlw_amd.ops import FusedAdadelta

    torch.manual_seed(37)
    start = (torch.randn(4096, device=_dev()) * 0.05).to(torch.bfloat16)
    p_bf = start.clone().requires_grad_(True)
    p_ref = start.float().requires_grad_(True)
    o1 = FusedAdadelta([p_bf], lr=1e-3)
    o2 = torch.optim.Adadelta([p_ref], lr=1e-3)
    for _ in range(20):
        g = (torch.randn(4096, device=_dev()) * 0.01).to(torch.bfloat16)
        p_bf.grad = g
        p_ref.grad = g.float()
        o1.step()
        o2.step()
    master = o1.state[p_bf]["master"]
    assert torch.allclose(master, p_ref, atol=ATOL, rtol=RTOL)
    # the movement itself, not only the endpoint, matches: |dw| is ~1e-5,
    # the size of atol, so compare the displacement relative to itself
    moved, moved_ref = master - start.float(), p_ref.detach() - start.float()
    rel = ((moved - moved_ref).abs().max() / moved_ref.abs().max()).item()
    print(f"mean |dw| {moved.abs().mean().item():.3e}, displacement rel err {rel:.3e}")
    unchanged = (master == start.float()).float().mean().item()
    print(f"master elements unchanged: {unchanged:.4%}")
    assert unchanged < 0.01, unchanged
    assert torch.equal(p_bf.detach(), master.to(torch.bfloat16))


@pytest.mark.gpu
def test_fused_adadelta_is_deterministic():
    from ddlw_amd.ops import FusedAdadelta

    outs = []
    for _ in range(2):
        g = torch.Generator(device="cpu").manual_seed(53)
        ps = [torch.randn(n, generator=g).to(_dev()).requires_grad_(True)
              for n in (5, 300, 1000)]
        ps.append(torch.randn(257, generator=g).to(_dev()).to(torch.bfloat16)
                  .requires_grad_(True))
        opt = FusedAdadelta(ps, lr=0.5, weight_decay=1e-4)
        for _ in range(3):
            for p in ps:
                p.grad = torch.randn(p.numel(), generator=g).to(_dev()).to(p.dtype)
            opt.step()
        outs.append([p.detach().clone() for p in ps]
                    + [opt.state[p][k].clone() for p in ps
                       for k in ("square_avg", "acc_delta")])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_fused_adadelta_load_state_dict_on_gpu():
    """fp32 state of a bf16 parameter survives a state_dict round trip and the
    rebuilt descriptor points at the loaded buffers."""
    from ddlw_amd.ops import FusedAdadelta

    torch.manual_seed(59)
    p = torch.randn(300, device=_dev()).to(torch.bfloat16).requires_grad_(True)
    o = FusedAdadelta([p], lr=0.5)
    grads = [torch.randn(300, device=_dev()).to(torch.bfloat16) for _ in range(3)]
    for g in grads[:2]:
        p.grad = g.clone()
        o.step()
    q = p.detach().clone().requires_grad_(True)
    fresh = FusedAdadelta([q], lr=0.5)
    fresh.load_state_dict(o.state_dict())
    assert all(v.dtype == torch.float32 for v in fresh.state[q].values())
    p.grad, q.grad = grads[2].clone(), grads[2].clone()
    o.step()
    fresh.step()
    assert torch.equal(p, q)
    assert torch.equal(o.state[p]["master"], fresh.state[q]["master"])
