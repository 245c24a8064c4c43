"""``fine_tune_bn="frozen"``: the fine-tuned suffix trains its conv weights
under BatchNorms that stay frozen (eval mode, no-grad gamma / beta, untouched
buffers). CPU only: the option needs no GPU."""
import torch

from ddlw_amd.core.model_io import load_model, save_model
from ddlw_amd.models import build_model
from ddlw_amd.ops.layers import BatchNormAct2d


def _bns(model, lo=0):
    return [m for f in model.base.base.features[lo:] for m in f.modules()
            if isinstance(m, BatchNormAct2d)]


def _flags(model):
    return {n: p.requires_grad for n, p in model.named_parameters()}


def test_frozen_mode_trains_only_the_suffix_convs(tmp_path):
    torch.manual_seed(0)
    m = build_model(32, 32, 3, 5, fine_tune_at=13, fine_tune_bn="frozen").train()
    feats = m.base.base.features
    assert _bns(m) and not any(bn.training for bn in _bns(m))
    assert not any(p.requires_grad for bn in _bns(m, 13) for p in (bn.weight, bn.bias))
    convs = [p for f in feats[13:] for n, p in f.named_parameters() if p.dim() == 4]
    assert convs and all(p.requires_grad for p in convs)
    assert not any(p.requires_grad for p in feats[:13].parameters())

    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.1)
    loss = torch.nn.functional.cross_entropy(m(torch.randn(4, 3, 32, 32)),
                                             torch.tensor([0, 1, 2, 3]))
    loss.backward()
    opt.step()
    after = m.state_dict()
    for k, v in before.items():
        if "running_" in k or "num_batches_tracked" in k:
            assert torch.equal(v, after[k]), k
    assert not torch.equal(before["base.base.features.13.conv.0.weight"],
                           after["base.base.features.13.conv.0.weight"])

    save_model(m, tmp_path / "m")
    back = load_model(str(tmp_path / "m"))
    assert back.base.fine_tune_bn == "frozen" and back.base.fine_tune_at == 13
    assert _flags(back) == _flags(m)


def test_default_is_unchanged_and_batch_restores():
    default = build_model(32, 32, 3, 5, fine_tune_at=13)
    assert "fine_tune_bn" not in default._ddlw_builder_spec[1]
    m = build_model(32, 32, 3, 5, fine_tune_at=13, fine_tune_bn="frozen")
    assert m._ddlw_builder_spec[1]["fine_tune_bn"] == "frozen"
    m.set_fine_tune_at(13)                       # None keeps the mode
    assert m.base.fine_tune_bn == "frozen"
    m.set_fine_tune_at(13, "batch")
    assert m._ddlw_builder_spec == default._ddlw_builder_spec
    assert _flags(m) == _flags(default)
    m.train(), default.train()
    assert [bn.training for bn in _bns(m)] == [bn.training for bn in _bns(default)]
    assert any(bn.training for bn in _bns(m, 13))
