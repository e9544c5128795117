"""FrozenBatchNorm2d.convert_frozen_batchnorm on a module that is already on the GPU (CNNBlockBase.freeze after model.to(device)):
the replacement used to be built on the CPU in fp32 and was left there."""
import pytest
import torch

from test_layers_cpu import check_conversion

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_convert_frozen_batchnorm_keeps_the_cuda_device(dtype):
    check_conversion("cuda", dtype)
