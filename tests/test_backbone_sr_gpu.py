"""The MiT backbone with the fused spatial reduction (Attention.sr_impl = 'hip') on a real MI355X: the shared run_*(device) bodies of
tests/test_backbone_sr.py under the goldens and gates of tests/test_backbone.py."""
import pytest
import torch

from tests import test_backbone_sr as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def test_golden_train_64():
    T.run_golden_train(dev())


def test_golden_eval_96x72():
    T.run_golden_eval(dev())


def test_call_counts():
    T.run_call_counts(dev())


def test_fp64_takes_the_torch_lines():
    T.run_other_inputs_take_the_torch_lines(dev())
