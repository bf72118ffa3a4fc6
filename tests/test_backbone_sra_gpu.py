"""The MiT backbones with the fused attention core on a real MI355X: the shared run_*(device) bodies of tests/test_backbone_sra.py (what
is checked and why is written there)."""
import pytest
import torch

from tests import test_backbone_sra as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('dwconv', ['hip', 'torch'])
def test_goldens_with_the_fused_attention(dwconv):
    T.run_goldens(dev(), dwconv)


def test_hip_against_torch():
    T.run_hip_vs_torch(dev())


def test_call_counts():
    T.run_call_counts(dev())


def test_fallback_is_the_torch_sequence():
    T.run_fallback(dev())
