"""compress_predictions without a GPU: the restatement the GPU tests use is pinned to the reference's utils/util.py:38-68,
and the drop-in's argument checks raise the reference's AssertionErrors before anything touches the device."""
import numpy as np
import pytest

from oracle.ref_loader import load_reference, reference_available
from tests.fixtures import load_npz


def restated_compress_predictions(query_masks, sims, topk):
  """utils/util.py:38-68 with a stable sort (equal scores by ascending index)."""
  valid = sims[np.asarray(query_masks).reshape(-1).astype(bool)]
  return np.argsort(-valid, axis=1, kind='stable')[:, :topk]


@pytest.mark.skipif(not reference_available(), reason='reference tree not present')
def test_restatement_equals_the_reference_compress_predictions_on_the_golden_matrix():
  g = load_npz('trainer_valid')
  util = load_reference().util
  for topk in (1, 5, 10):
    want = util.compress_predictions(g['query_masks'], g['sims'], topk=topk)
    got = restated_compress_predictions(g['query_masks'], g['sims'], topk)
    assert got.shape == want.shape == (55, topk)
    assert np.array_equal(got, want), topk


def test_drop_in_argument_checks_raise_before_the_device():
  from mmt_amd.metric import compress_predictions
  with pytest.raises(AssertionError, match='Expected query_masks to be a matrix'):
    compress_predictions(np.ones(6, np.float32), np.zeros((6, 3), np.float32))
  with pytest.raises(AssertionError, match='same number of videos'):
    compress_predictions(np.ones((3, 2), np.float32), np.zeros((6, 4), np.float32))
  with pytest.raises(AssertionError, match='same number of queries'):
    compress_predictions(np.ones((3, 2), np.float32), np.zeros((5, 3), np.float32))
