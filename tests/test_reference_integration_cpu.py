"""Reference-side integration (CPU).  Where the reference tree is present (MMT_REFERENCE_ROOT) every check below runs
against it; elsewhere the checks that need only the reference's OUTPUTS run against tests/golden/trainer_valid.npz and
tests/golden/reference_integration.npz (oracle/gen_integration_golden.py), and the trainer-loop identity, which is a
statement about the reference's own code, is skipped.

  * the golden trajectory tests/golden/trainer_epoch.npz IS what the reference's own `Trainer._train_epoch` produces, and
    `trainer_harness.mimic_train_epoch` (what the GPU test drives the MI355X drop-in with) is that method, statement for
    statement: bit-identical losses and weights on the reference model;
  * `BaseTrainer.match_checkpoint_to_model` (base/base_trainer.py:391-406: zero-padding of
    vid_bert.embeddings.position_embeddings.weight, e.g. a 32-position MSRVTT checkpoint into a 102-position model)
    followed by `load_state_dict` works on the drop-in's state dict;
  * the shim of INTEGRATION.md section 1(b) makes `config.init('arch', model.model, ...)` (parse_config.py:138-145,
    train.py:86-91) build the drop-in from a PUBLISHED config's arch arguments, and the trainer's imported
    `sharded_cross_view_inner_product` resolve to ours."""
import collections
import importlib
import json
import warnings

import numpy as np
import pytest
import torch

from oracle.ref_loader import load_reference, reference_available
from tests import trainer_harness as H
from tests.fixtures import load_npz

REFERENCE = reference_available()


@pytest.mark.skipif(not REFERENCE, reason='needs the reference tree (runs the reference\'s own Trainer._train_epoch)')
def test_real_trainer_epoch_reproduces_golden_and_mimic_is_the_same_loop():
  from oracle import gen_trainer_golden as G
  R = load_reference()
  g = load_npz('trainer_epoch')
  with warnings.catch_warnings():
    warnings.simplefilter('ignore')
    model, sd, losses, logs, tr = G.run_real(R)
  assert np.abs(np.asarray(losses) - g['losses']).max() < 1e-6
  assert np.abs(np.asarray([l['loss'] for l in logs]) - g['epoch_loss']).max() < 1e-6
  assert abs(tr.optimizer.param_groups[0]['lr'] - float(g['final_lr'])) < 1e-12
  final = model.state_dict()
  for k in H.PROBE_PARAMS:
    assert np.abs(final[k].reshape(-1)[::37][:4096].numpy() - g['final/' + k]).max() < 1e-6, k
  m2, losses2, logs2, st = G.run_mimic(R)
  assert losses2 == losses
  for (k, a), (_, b) in zip(final.items(), m2.state_dict().items()):
    assert torch.equal(a, b), k
  assert (st.n_samples, st.n_steps) == (tr.n_samples, tr.n_steps)


def test_real_valid_epoch_reproduces_golden_and_mimic_is_the_same_loop():
  """Evaluation half: the reference's own `Trainer._valid_epoch` (+ `_get_embeddings`, trainer/trainer.py:286-483) on the
  validation loader with 3 captions per video and masked captions gives tests/golden/trainer_valid.npz, and
  `trainer_harness.mimic_valid_epoch` (what the GPU test drives the drop-in with) is that method: identical similarity
  matrix, metrics and rank vectors."""
  g = load_npz('trainer_valid')
  want = json.loads(str(g['metrics']))
  if REFERENCE:
    from oracle import gen_trainer_golden as G
    R = load_reference()
    model, _ = G.build_reference_model(R)
    sims, qm, metrics = G.run_real_valid(R, model)
    assert np.abs(sims - g['sims']).max() < 1e-6 and np.array_equal(qm, g['query_masks'])
    for name in ('t2v_metrics', 'v2t_metrics'):
      for k in H.METRIC_KEYS:
        assert abs(float(metrics[name][k]) - want[name][k]) < 1e-4, (name, k)
    sims2, nested2, _ = H.mimic_valid_epoch(model, H.MODS, H.EvalLoader(), torch.device('cpu'),
                                            R.model.sharded_cross_view_inner_product,
                                            [R.metric.t2v_metrics, R.metric.v2t_metrics])
    assert np.array_equal(sims, sims2)
    for name in ('t2v_metrics', 'v2t_metrics'):
      assert np.array_equal(metrics[name]['cols'], nested2[name]['cols'])
  else:
    # the reference's similarity matrix, query masks and metrics as its own _valid_epoch recorded them
    sims, qm, metrics = g['sims'], g['query_masks'], want
  # and the oracle's restatement of model/metric.py (what the GPU tests compare the device-side ranks with) agrees
  from oracle import mmt_oracle as O
  for name, fn in (('t2v_metrics', O.t2v_metrics), ('v2t_metrics', O.v2t_metrics)):
    got = fn(sims, query_masks=qm)
    for k in H.METRIC_KEYS:
      assert abs(got[k] - float(metrics[name][k])) < 1e-4, (name, k)


def _native_cenet(max_pos, txt_bert=None):
  from mmt_amd import synthetic
  from mmt_amd.model import CENet
  args = H.arch_args()
  args['vid_bert_params'] = dict(args['vid_bert_params'], max_position_embeddings=max_pos)
  return CENet(expert_dims=synthetic.compute_dims(H.MODS), tokenizer=None, txt_bert=txt_bert or H.HashTextTower(), **args)


def test_match_checkpoint_to_model_then_load_state_dict():
  gi = load_npz('reference_integration')
  small, big = _native_cenet(32), _native_cenet(102)
  key = 'vid_bert.embeddings.position_embeddings.weight'
  small.load_state_dict(dict(small.state_dict(), **{key: torch.from_numpy(gi['pos_in'])}), strict=True)
  ckpt = {k: v.detach().clone() for k, v in small.state_dict().items()}
  assert ckpt[key].shape[0] == 32 and big.state_dict()[key].shape[0] == 102
  if REFERENCE:
    load_reference()
    BT = importlib.import_module('base.base_trainer').BaseTrainer
    BT.match_checkpoint_to_model(None, ckpt, big.state_dict())      # base/base_trainer.py:391-406
    assert torch.equal(ckpt[key], torch.from_numpy(gi['pos_out']))
  else:
    ckpt[key] = torch.from_numpy(gi['pos_out'])                      # what that method made of the same table
  assert ckpt[key].shape[0] == 102
  big.load_state_dict(ckpt, strict=True)                            # base/base_trainer.py:432
  got = big.state_dict()[key]
  assert torch.equal(got[:32], small.state_dict()[key]) and float(got[32:].abs().max()) == 0.0
  for k, v in small.state_dict().items():
    if k != key:
      assert torch.equal(big.state_dict()[k], v), k


def test_integration_shim_builds_the_drop_in_from_a_published_config(monkeypatch):
  import mmt_amd.loss
  import mmt_amd.model
  gi = load_npz('reference_integration')
  cfg = json.loads(str(gi['config']))                         # experts / arch / loss of the published config
  expert_dims = collections.OrderedDict((k, v) for k, v in json.loads(str(gi['expert_dims'])))
  want = {k: tuple(v) for k, v in json.loads(str(gi['param_shapes'])).items()}
  arch = cfg['arch']
  if REFERENCE:
    from oracle import gen_integration_golden as GI
    R = load_reference()
    T = importlib.import_module('trainer.trainer')
    # INTEGRATION.md section 1(b)
    monkeypatch.setattr(R.model, 'CENet', mmt_amd.model.CENet)
    monkeypatch.setattr(R.model, 'sharded_cross_view_inner_product', mmt_amd.model.sharded_cross_view_inner_product)
    monkeypatch.setattr(R.loss, 'MaxMarginRankingLoss', mmt_amd.loss.MaxMarginRankingLoss)
    monkeypatch.setattr(T, 'sharded_cross_view_inner_product', mmt_amd.model.sharded_cross_view_inner_product)
    full = GI.published_config()
    assert {k: full[k] for k in cfg} == cfg
    assert list(R.util.compute_dims(full).items()) == list(expert_dims.items())
    model_module, loss_module = R.model, R.loss
  else:
    # the modules the shim leaves the reference's names pointing at
    model_module, loss_module = mmt_amd.model, mmt_amd.loss
  # parse_config.py:138-145: getattr(module, cfg[name]['type'])(*args, **cfg[name]['args'], **kwargs)
  model = getattr(model_module, arch['type'])(expert_dims=expert_dims, tokenizer=None, txt_bert=H.HashTextTower(),
                                              **arch['args'])
  assert isinstance(model, mmt_amd.model.CENet) and isinstance(model, torch.nn.Module)
  assert list(model.modalities) == list(expert_dims.keys())
  loss = getattr(loss_module, cfg['loss']['type'])(**cfg['loss']['args'])
  assert isinstance(loss, mmt_amd.loss.MaxMarginRankingLoss)
  # every parameter the reference model has, by name and shape (released checkpoints load)
  if REFERENCE:
    assert {k: tuple(v.shape) for k, v in GI.reference_cenet(arch['args'], expert_dims).state_dict().items()} == want
  got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
  assert got == want
