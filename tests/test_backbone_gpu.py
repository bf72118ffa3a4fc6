"""The MiT backbones on a real MI355X: the shared run_*(device) bodies of tests/test_backbone.py (the goldens, the gates and why are
written there) with 'torch' (stock PyTorch on the GPU) and 'hip' (cffm_dwconv_gelu_fwd / _bwd of libcffm_hip.so)."""
import pytest
import torch

from tests import test_backbone as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_golden_train_64(kind):
    T.run_golden_train(dev(), kind)


@pytest.mark.parametrize('kind', ['torch', 'hip'])
def test_golden_eval_96x72(kind):
    T.run_golden_eval(dev(), kind)


def test_hip_against_torch():
    T.run_hip_vs_torch(dev())


def test_hip_runs_the_library():
    T.run_hip_is_used(dev())


def test_segmentor_with_mit_b0_eval():
    T.run_segmentor_eval(dev())


def test_segmentor_with_mit_b0_forward_train():
    T.run_segmentor_train(dev())
