"""TEST INFRASTRUCTURE -- tests/golden/reference_integration.npz: what tests/test_reference_integration_cpu.py needs from the
REAL reference when the reference tree is not there.

    python -m oracle.gen_integration_golden        # needs the reference tree (MMT_REFERENCE_ROOT)

Records, as data only:
  * `config`: the settings of the published MSRVTT jsfusion config that the integration shim builds the drop-in from
    (its `experts`, `arch` and `loss` sections, configs_pub/eccv20/MSRVTT_jsfusion_trainval.json);
  * `expert_dims`: the reference's `utils.util.compute_dims` of that config (name -> {dim, idx}, in order);
  * `param_shapes`: name -> shape of every entry of the reference CENet's state dict built from that config;
  * `pos_in` / `pos_out`: a seeded 32-row position-embedding table and what the reference's
    `BaseTrainer.match_checkpoint_to_model` turns it into for a 102-position model."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.ref_loader import REFERENCE_ROOT, load_reference  # noqa: E402

POS_KEY = 'vid_bert.embeddings.position_embeddings.weight'
CONFIG_REL = ('configs_pub', 'eccv20', 'MSRVTT_jsfusion_trainval.json')


def published_config():
  return json.load(open(os.path.join(REFERENCE_ROOT, *CONFIG_REL)))


def reference_cenet(arch_args, expert_dims):
  """The reference's CENet from a PRIVATE copy of model/model.py (tests may monkeypatch the public attribute)."""
  import importlib.util

  from tests import trainer_harness as H
  spec = importlib.util.spec_from_file_location('model_model_private', os.path.join(REFERENCE_ROOT, 'model', 'model.py'))
  ref = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(ref)
  ref.TxtBertModel = H.HashTextTower
  return ref.CENet(expert_dims=expert_dims, tokenizer=None, **arch_args)


def padded_position_table(R, rows=32, model_rows=102, hidden=512):
  import importlib
  BT = importlib.import_module('base.base_trainer').BaseTrainer
  pos_in = torch.randn(rows, hidden, generator=torch.Generator().manual_seed(0))
  ckpt = {POS_KEY: pos_in.clone()}
  BT.match_checkpoint_to_model(None, ckpt, {POS_KEY: torch.zeros(model_rows, hidden)})
  return pos_in.numpy(), ckpt[POS_KEY].numpy()


def main():
  R = load_reference()
  cfg = published_config()
  expert_dims = R.util.compute_dims(cfg)
  shapes = {k: list(v.shape) for k, v in reference_cenet(cfg['arch']['args'], expert_dims).state_dict().items()}
  pos_in, pos_out = padded_position_table(R)
  out = dict(config=json.dumps({k: cfg[k] for k in ('experts', 'arch', 'loss')}),
             expert_dims=json.dumps([[k, dict(v)] for k, v in expert_dims.items()]),
             param_shapes=json.dumps(shapes), pos_in=pos_in.astype(np.float32), pos_out=pos_out.astype(np.float32))
  np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'reference_integration.npz'), **out)
  print('reference_integration.npz: %d experts, %d state-dict entries, position table %s -> %s' % (
      len(expert_dims), len(shapes), pos_in.shape, pos_out.shape))


if __name__ == '__main__':
  main()
