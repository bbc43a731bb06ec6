"""``models.SFNONet`` on CPU tensors: the amd backend (the ops' ATen kernels) against the torch backend in fp64, export,
the ONNX runner, engines and their files.  The hand kernels under it: tests/test_sfno_net_gpu.py."""
import itertools

import pytest
import torch

from helpers import rel_l2
from tensorrt_dft_plugins_amd.engine import Engine
from tensorrt_dft_plugins_amd.engine import cli
from tensorrt_dft_plugins_amd.models import SFNOConfig, SFNONet
from tensorrt_dft_plugins_amd.onnx import exporter as ex
from tensorrt_dft_plugins_amd.onnx import proto as P
from tensorrt_dft_plugins_amd.onnx.runner import OnnxGraph

BF = torch.bfloat16
TOL_BF16 = 2e-2  # the project's bf16 layer bound (tests/test_sfno_bf16.py), per field


def make_net(seed=0, **kw):
    """The small network of this file, with every norm's affine parameters and the biases drawn at random (their
    defaults, ones and zeros, would hide a dropped weight or bias)."""
    cfg = dict(img_size=(17, 32), in_chans=3, out_chans=2, embed_dim=6, depth=2, lmax=8, mmax=8)
    cfg.update(kw)
    torch.manual_seed(seed)
    net = SFNONet(SFNOConfig(**cfg)).eval()
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "norm" in name:
                p.copy_(1.0 + 0.3 * torch.randn_like(p) if name.endswith("weight") else 0.3 * torch.randn_like(p))
    return net


def field_err(out, ref):
    """max over (batch, channel) fields of the rel-L2 against the fp64 reference"""
    o, r = out.detach().cpu().double().flatten(2), ref.flatten(2)
    return float(((o - r).norm(dim=2) / r.norm(dim=2)).max())


@pytest.mark.parametrize("norm,pos_embed,mix", list(itertools.product(["instance", "none"], [True, False],
                                                                      ["auto", "degree"])))
def test_sfno_net_amd_equals_torch_fp64(norm, pos_embed, mix):
    net = make_net(norm=norm, pos_embed=pos_embed, mix=mix)
    assert net.backend == "amd"
    x = torch.randn(2, 3, 17, 32)
    with torch.no_grad():
        ya = net(x)
        ref = net.set_backend("torch")(x.double())
        yt = net(x)
    assert ya.shape == (2, 2, 17, 32) and ya.dtype == torch.float32 and ref.dtype == torch.float64
    err = rel_l2(ya, ref)
    print(f"MEASURED sfno_net cpu norm={norm} pos={pos_embed} mix={mix} amd vs fp64 {err:.3e}")
    assert err < 1e-6 and rel_l2(yt, ref) < 1e-6


def test_sfno_net_pieces_matter():
    """The position embedding, the norms' affine parameters and the residual all reach the output."""
    x = torch.randn(1, 3, 17, 32)
    with torch.no_grad():
        base = make_net()(x)
        assert rel_l2(make_net(pos_embed=False)(x), base) > 1e-4
        assert rel_l2(make_net(norm="none")(x), base) > 1e-3
        net = make_net()
        net.blocks[1].norm1.bias.add_(1.0)
        assert rel_l2(net(x), base) > 1e-3
        net = make_net()
        net.pos.mul_(2.0)  # the cached batch expansion follows the parameter
        assert rel_l2(net(x), base) > 1e-4


def test_sfno_net_set_backend_and_errors():
    net = make_net()
    assert net.set_backend("torch") is net and net.backend == "torch"
    assert all(b.layer.backend == "torch" and b.layer.spectral.backend == "torch" for b in net.blocks)
    net.set_backend("amd")
    assert all(b.layer.backend == "amd" and b.layer.spectral.sht.backend == "amd" for b in net.blocks)
    with pytest.raises(ValueError):
        net.set_backend("cuda")
    with pytest.raises(ValueError):
        SFNONet(SFNOConfig(norm="layer"))
    with pytest.raises(ValueError):
        net(torch.randn(1, 3, 17, 33))
    with pytest.raises(TypeError):
        net(torch.randn(1, 3, 17, 32).double())


def test_sfno_net_bf16_cpu():
    """A bf16 input gives a bf16 network.  Against the fp64 oracle on the same bf16 input and bf16-rounded weights."""
    net = make_net()
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(p.to(BF).float())
        x = torch.randn(2, 3, 17, 32).to(BF)
        out = net(x)
        ref = net.set_backend("torch")(x.double())
    assert out.dtype == BF
    err = field_err(out, ref)
    print(f"MEASURED sfno_net cpu bf16 depth 2 per-field rel-L2 {err:.3e}")
    assert err < TOL_BF16


@pytest.mark.parametrize("mix", ["auto", "degree"])
def test_sfno_net_export_runner_engine(mix, tmp_path):
    net = make_net(mix=mix)
    x = torch.randn(2, 3, 17, 32)
    with torch.no_grad():
        eager = net(x)
    data = ex.export(net, (x,))
    nodes = P.load_model(data).graph.node
    compute = {n.op_type for n in nodes if n.domain == "com.amd.dft"}
    assert {"fno_pointwise", "instance_norm", "legendre"} <= compute
    assert ("sfno_mix" if mix == "degree" else "fno_mix") in compute
    # every compute node is a com.amd.dft op: what is left in the default domain only moves or reshapes data
    stock = {n.op_type for n in nodes if n.domain != "com.amd.dft"}
    print(f"MEASURED sfno_net export mix={mix} com.amd.dft {sorted(compute)} other {sorted(stock)}")
    assert not stock & {"Conv", "InstanceNormalization", "MatMul", "Gemm", "Einsum", "Add", "Mul", "Erf", "Gelu",
                        "ReduceMean", "Div", "Sqrt", "Sub"}
    (y,) = OnnxGraph(data, torch.device("cpu")).run(x)
    assert torch.equal(y, eager)
    eng = Engine.build(net, (x,), device="cpu")
    (ye,) = eng.infer(x)
    assert torch.equal(ye, eager)
    p = str(tmp_path / "sfno.engine")
    eng.save(p)
    (yl,) = Engine.load(p, device="cpu").infer(x)
    assert torch.equal(yl, eager)


def test_sfno_net_dftexec(tmp_path):
    net = make_net()
    x = torch.randn(1, 3, 17, 32)
    onnx_path, eng_path = str(tmp_path / "sfno.onnx"), str(tmp_path / "sfno.engine")
    ex.export(net, (x,), onnx_path)
    assert cli.main(["--onnx", onnx_path, "--saveEngine", eng_path, "--buildOnly", "--device", "cpu"]) == 0
    assert cli.main(["--loadEngine", eng_path, "--device", "cpu", "--iterations", "2", "--warmUp", "1"]) == 0
    with torch.no_grad():
        (y,) = Engine.load(eng_path, device="cpu").infer(x)
        assert torch.equal(y, net(x))
