"""FrozenBatchNorm2d.convert_frozen_batchnorm keeps the device and dtype of the module it converts (CPU half; the CUDA module is
tests/test_layers_gpu.py)."""
import torch
from torch import nn

from __graft_entry__ import load_package

load_package()


def check_conversion(device, dtype):
    """a BatchNorm2d under a Sequential and a bare one, on `device` in `dtype`: after the conversion every buffer and parameter
    sits where the source's did, in its dtype, with its values"""
    from drn_wsod_pytorch_amd.layers import FrozenBatchNorm2d

    def bn(c, seed):
        g = torch.Generator().manual_seed(seed)
        m = nn.BatchNorm2d(c, eps=1e-3)
        with torch.no_grad():
            m.weight.copy_(torch.randn(c, generator=g))
            m.bias.copy_(torch.randn(c, generator=g))
            m.running_mean.copy_(torch.randn(c, generator=g))
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        return m.to(device=device, dtype=dtype)

    dev = torch.empty(0, device=device).device
    for wrap in (True, False):
        src = bn(5, 3)
        want = {k: v.detach().clone() for k, v in src.state_dict().items() if k != "num_batches_tracked"}
        mod = nn.Sequential(nn.Conv2d(3, 5, 1).to(device=device, dtype=dtype), src) if wrap else src
        out = FrozenBatchNorm2d.convert_frozen_batchnorm(mod)
        frozen = out[1] if wrap else out
        assert isinstance(frozen, FrozenBatchNorm2d) and frozen.eps == 1e-3 and frozen.num_features == 5
        tensors = dict(out.named_buffers())
        tensors.update(out.named_parameters())
        assert len(tensors) == (6 if wrap else 4)
        for k, t in tensors.items():
            assert t.device == dev and t.dtype == dtype, (wrap, k, t.device, t.dtype)
        got = dict(frozen.named_buffers())
        assert sorted(got) == sorted(want)
        for k in want:
            assert torch.equal(got[k], want[k]), (wrap, k)
        x = torch.randn(2, 5, 3, 3, generator=torch.Generator().manual_seed(1)).to(device=device, dtype=dtype)
        y = frozen(x)  # (a CPU buffer beside a CUDA input would raise here)
        assert y.device == dev and y.dtype == dtype


def test_convert_frozen_batchnorm_keeps_float64_on_the_cpu():
    check_conversion("cpu", torch.float64)
