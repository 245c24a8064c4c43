"""The bf16 policy, ``Model(precision=...)``, ``FusedAdadelta``'s CPU fallback
and the loader's ``output="uint8"`` — everything that needs no GPU."""
import copy

import pyarrow as pa
import pytest
import torch

from ddlw_amd.core.model_io import load_model, save_model
from ddlw_amd.data.loader import make_converter
from ddlw_amd.data.synthetic import make_synthetic_dataset
from ddlw_amd.models import build_model
from ddlw_amd.ops import FusedAdadelta, apply_bf16_policy, prepare_batch
from ddlw_amd.ops.layers import BatchNormAct2d
from ddlw_amd.train import Model


def _dtypes(m):
    out = {k: v.dtype for k, v in m.named_parameters()}
    out.update({k: v.dtype for k, v in m.named_buffers()})
    return out


def test_apply_bf16_policy_casts_convs_keeps_bn(tmp_path):
    torch.manual_seed(3)
    m = build_model(32, 32, 3, 5, fine_tune_at=17)
    params_before = {k: p for k, p in m.named_parameters()}
    grad_before = {k: p.requires_grad for k, p in m.named_parameters()}
    assert any(grad_before.values()) and not all(grad_before.values())
    keys_before = list(m.state_dict().keys())

    out = apply_bf16_policy(m)
    assert out is m
    n_conv = n_bn = 0
    for mod in m.modules():
        if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
            n_conv += 1
            for p in mod.parameters(recurse=False):
                assert p.dtype == torch.bfloat16
        elif isinstance(mod, (torch.nn.BatchNorm2d, BatchNormAct2d)):
            n_bn += 1
            for t in list(mod.parameters(recurse=False)) + list(mod.buffers(recurse=False)):
                if t.is_floating_point():
                    assert t.dtype == torch.float32
    assert n_conv > 50 and n_bn > 50, (n_conv, n_bn)
    # the same Parameter objects, the same trainable split, the same keys
    for k, p in m.named_parameters():
        assert p is params_before[k], k
        assert p.requires_grad == grad_before[k], k
    assert list(m.state_dict().keys()) == keys_before

    # idempotent
    dt = _dtypes(m)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    apply_bf16_policy(m)
    assert _dtypes(m) == dt
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k

    # a saved bf16-policy model loads as fp32 with the bf16 values widened
    save_model(m, tmp_path / "model")
    back = load_model(str(tmp_path / "model"))
    for k, v in back.state_dict().items():
        if v.is_floating_point():
            assert v.dtype == torch.float32, k
            assert torch.equal(v, sd[k].float()), k
    assert {k: p.requires_grad for k, p in back.named_parameters()} == grad_before


def test_accepts_uint8_adds_no_state():
    from ddlw_amd.models.mobilenet_v2 import FrozenBase, MobileNetV2, TransferModel

    for cls in (MobileNetV2, FrozenBase, TransferModel):
        assert cls.__dict__["accepts_uint8"] is True
    m = build_model(32, 32, 3, 5)
    assert not any("accepts_uint8" in k for k in m.state_dict())
    assert "accepts_uint8" not in m.__dict__


def test_prepare_batch_layouts_cpu():
    m = build_model(32, 32, 3, 5)
    u8 = torch.randint(0, 256, (4, 32, 32, 3), dtype=torch.uint8)
    a = prepare_batch(m, u8)
    assert a.dtype == torch.uint8 and a.shape == (4, 3, 32, 32)
    assert a.data_ptr() == u8.data_ptr()
    b = prepare_batch(m, u8.permute(0, 3, 1, 2))
    assert b.shape == (4, 3, 32, 32) and torch.equal(a, b)
    with pytest.raises(ValueError, match="layout"):
        prepare_batch(m, torch.zeros(4, 1, 32, 3, dtype=torch.uint8))
    # a module without the attribute gets the normalized bf16 batch
    plain = torch.nn.Identity()
    c = prepare_batch(plain, u8)
    assert c.dtype == torch.bfloat16 and c.shape == (4, 3, 32, 32)
    ref = (u8.permute(0, 3, 1, 2).to(torch.bfloat16) / 127.5) - 1.0
    assert torch.equal(c, ref)
    # float: bf16 channels_last for images, a plain cast for any other rank
    f = prepare_batch(m, torch.randn(2, 3, 8, 8))
    assert f.dtype == torch.bfloat16
    assert f.is_contiguous(memory_format=torch.channels_last)
    assert prepare_batch(m, torch.randn(2, 7)).dtype == torch.bfloat16


def test_model_precision_on_cpu():
    m = build_model(32, 32, 3, 5)
    before = _dtypes(m)
    with pytest.raises(ValueError, match="CUDA"):
        Model(copy.deepcopy(m), precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        Model(m, precision="fp16")
    auto = Model(m, torch.device("cpu"), precision="auto")
    assert auto.precision == "fp32"
    assert _dtypes(m) == before
    assert Model(m).precision == "fp32"
    assert _dtypes(m) == before


def test_fused_adadelta_cpu_matches_torch():
    torch.manual_seed(41)
    shapes = [(7,), (33, 5), (4, 3, 3, 3)]
    p1 = [torch.randn(s, requires_grad=True) for s in shapes]
    p2 = [p.detach().clone().requires_grad_(True) for p in p1]
    o1 = FusedAdadelta(p1, weight_decay=1e-4)
    o2 = torch.optim.Adadelta(p2, weight_decay=1e-4)
    assert o1.defaults == dict(lr=1.0, rho=0.9, eps=1e-6, weight_decay=1e-4)
    for _ in range(5):
        for a, b in zip(p1, p2):
            g = torch.randn_like(a)
            a.grad, b.grad = g.clone(), g.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        assert torch.allclose(a, b, atol=1e-5, rtol=1e-4)
        for k in ("square_avg", "acc_delta"):
            assert torch.allclose(o1.state[a][k], o2.state[b][k], atol=1e-5, rtol=1e-4)


def test_fused_adadelta_state_dict_keeps_fp32_for_bf16_param():
    torch.manual_seed(43)
    base = torch.randn(64).to(torch.bfloat16)
    p = base.clone().requires_grad_(True)
    o = FusedAdadelta([p], lr=0.5)
    for _ in range(2):
        p.grad = torch.randn(64).to(torch.bfloat16)
        o.step()
    st = o.state[p]
    assert set(st) == {"master", "square_avg", "acc_delta"}
    assert all(v.dtype == torch.float32 for v in st.values())
    assert torch.equal(p.detach(), st["master"].to(torch.bfloat16))

    q = p.detach().clone().requires_grad_(True)
    fresh = FusedAdadelta([q], lr=0.5)
    fresh._desc[0] = ("stale",)
    fresh.load_state_dict(o.state_dict())
    assert fresh._desc == {}
    for k, v in fresh.state[q].items():
        assert v.dtype == torch.float32, k
        assert torch.equal(v, st[k]), k
    # both continue identically
    g = torch.randn(64).to(torch.bfloat16)
    p.grad, q.grad = g.clone(), g.clone()
    o.step()
    fresh.step()
    assert torch.equal(p, q)
    assert torch.equal(o.state[p]["master"], fresh.state[q]["master"])


def test_loader_output_uint8(ddlw_home):
    # images at their native size: no resampler runs on either path, so the
    # two loaders differ by the normalization alone
    contents, labels = make_synthetic_dataset(12, 24, 20, jpeg=True, num_classes=3)
    table = pa.table({"content": pa.array(contents, pa.binary()), "label_idx": labels})
    conv = make_converter(table, row_group_rows=4)
    kw = dict(batch_size=5, num_epochs=1, img_height=24, img_width=20)
    try:
        with conv.make_torch_dataset(output="uint8", **kw) as ds_u8, \
                conv.make_torch_dataset(output="float", **kw) as ds_f, \
                conv.make_torch_dataset(**kw) as ds_default:
            n = 0
            for (xu, yu), (xf, yf), (xd, _) in zip(ds_u8, ds_f, ds_default):
                assert xu.dtype == torch.uint8 and xu.shape[1:] == (24, 20, 3)
                assert xf.dtype == torch.float32 and xf.shape[1:] == (3, 24, 20)
                assert torch.equal(xu.permute(0, 3, 1, 2).float() / 127.5 - 1.0, xf)
                assert torch.equal(xf, xd)
                assert torch.equal(yu, yf)
                n += len(xu)
            assert n == 12
        with pytest.raises(ValueError, match="transform"):
            conv.make_torch_dataset(output="uint8", transform=lambda c: c, **kw)
        with pytest.raises(ValueError, match="output"):
            conv.make_torch_dataset(output="int8", **kw)
    finally:
        conv.delete()


def test_loader_uint8_transform_is_picklable():
    import functools
    import pickle

    from ddlw_amd.data.loader import _uint8_transform

    contents, _ = make_synthetic_dataset(1, 16, 16, jpeg=True)
    fn = pickle.loads(pickle.dumps(
        functools.partial(_uint8_transform, img_height=16, img_width=16)))
    out = fn(contents[0])
    assert out.dtype == torch.uint8 and out.shape == (16, 16, 3)
