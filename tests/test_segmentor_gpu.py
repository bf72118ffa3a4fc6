"""``EncoderDecoder_clips`` on a real MI355X: the shared run_*(device) bodies of tests/test_segmentor.py on the same toy input."""
import pytest
import torch

from tests import test_segmentor as T

pytestmark = pytest.mark.gpu


def dev():
    return torch.device('cuda:0')


def test_simple_test_is_one_prediction_call():
    T.run_feeds_the_metrics(dev())


def test_short_clip_takes_the_short_circuit():
    T.run_simple_test(dev(), t=2)


def test_aug_test_accumulates_in_one_buffer():
    T.run_aug_test(dev())


def test_forward_train_returns_the_head_losses():
    T.run_forward_train(dev())
