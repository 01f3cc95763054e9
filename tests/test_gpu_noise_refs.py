"""esr_fill_noise (the z every fused noise epilogue draws: csrc/common.h philox_normal8) against its independent float64
definition in tests/noise_refs.py.  z enters as 1 + 0.1 z, so 1e-3 absolute keeps the hardware's log / sqrt / sin / cos
approximations under a quarter of an fp16 ulp of the activation; a structural error — counter layout, key words, round
count, which half of a word feeds the radius — is O(1).  Worst |dz| measured on an MI355X: 4.6e-7."""
import pytest
import torch

from tests import noise_refs as NR

pytestmark = pytest.mark.gpu

SEED = (0x2b5f << 40) | 0x9abc_def1          # bits above 2^32: the key's high word


@pytest.mark.parametrize('layer', [0, 91])
def test_fill_noise_matches_the_reference(layer):
    from esrganplus_amd import ops
    assert torch.cuda.is_available()
    shape = (2, 20, 5, 70)                   # C not a multiple of 8, W not a multiple of anything
    z = ops.philox_normal(shape, SEED, layer, torch.device('cuda:0')).cpu().double()
    ref = torch.from_numpy(NR.normal(shape, SEED, layer))
    e = (z - ref).abs().max().item()
    print('esr_fill_noise layer %d: worst |dz| %.2e' % (layer, e))
    assert e <= 1e-3, e
    assert (z - torch.from_numpy(NR.normal(shape, SEED & 0xFFFFFFFF, layer))).abs().max().item() > 1.0
