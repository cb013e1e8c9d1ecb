"""The host side of item-set pooling (VideoIndex.item_pooling and item_pooling= of the scans; mmt_search_topk_itemsets,
mmt_search_thresholds_itemsets, mmt_search_count_itemsets and their bf16 forms) without a GPU: the header and the ctypes
table, the workspace sizers against the tile rule, the argument gates of the entry points, the set-alignment check of the
sharded layout, the argument errors of the calls, and the definition against the reference's 'avg' similarities on the
gallery axis."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.fixtures import load_npz
from tests.test_index_pooled_cpu import _hollow_index, _hollow_sharded, _params, brute_pooled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ('mmt_topk_itemsets_workspace_keys', 'mmt_count_itemsets_workspace_ints')
F32 = np.float32


def test_signatures_of_the_new_exports_agree_with_the_header():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle = ctypes.CDLL(_lib.LIB_PATH)
  arity = dict(zip(SIZES, (4, 4)))
  for name in SIZES:
    res_name, params = _params(src, name)
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if res_name == 'int' else ctypes.c_int64), name
    assert (res_name == 'int64_t') == (name in SIZES)
    assert len(args) == len(params) == arity[name], name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p) and (a is ctypes.c_int) == (p.startswith('int ')), (name, p)
    assert hasattr(handle, name)
  assert handle.mmt_abi_version() == 6
  assert _lib.lib().mmt_abi_version() == 6                  # and every declared symbol binds


def _fns():
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fns = {}
  for name in SIZES:
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  return fns


def test_workspace_sizes_follow_the_tiles():
  """A tile holds 128 // C whole sets and a chunk is a whole number of tiles: the chunk rule of the unpooled scans (4096
  columns, halved down to 128 while the launch has fewer than 512 blocks) on 128 columns per tile."""
  from mmt_amd import _lib
  fns = _fns()
  keys, ints = fns['mmt_topk_itemsets_workspace_keys'], fns['mmt_count_itemsets_workspace_ints']
  plain_keys, plain_ints = _lib.lib().mmt_topk_workspace_keys, _lib.lib().mmt_count_workspace_ints
  for nq, nt, c, k in ((1, 1, 1, 1), (130, 3650, 4, 10), (3, 5, 128, 128), (9, 513, 8, 10), (65, 129, 2, 1),
                       (1000, 3000, 33, 7), (70, 5000, 1, 3), (4096, 13107, 20, 10), (64, 65536, 4, 10), (7, 100000, 65, 5)):
    tiles = -(-nt // (128 // c))
    blocks, chunk = -(-nq // 64), 4096
    while chunk > 128 and blocks * -(-tiles * 128 // chunk) < 512:
      chunk //= 2
    n_chunks = -(-tiles // (chunk // 128))
    t = k % 32 + 1
    assert keys(nq, nt, c, k) == nq * n_chunks * k, (nq, nt, c, k)
    assert ints(nq, nt, c, t) == nq * t * 2 * n_chunks
    if c == 1:
      assert keys(nq, nt, c, k) == plain_keys(nq, nt, k) and ints(nq, nt, c, t) == plain_ints(nq, nt, t)
  assert keys(130, 3650, 4, 10) == 130 * 115 * 10           # 3 query blocks x 115 chunks of one tile of 32 sets
  for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 129, 1), (1, 1, -1, 1), (1, 1, 1, 0), (1, 2 ** 24, 128, 1),
              (-1, 1, 1, 1)):
    assert keys(*bad) == -1 and ints(*bad) == -1, bad
  assert keys(1, 1, 1, 129) == -1 and ints(1, 1, 1, 33) == -1
  assert keys(1, 2 ** 24 - 1, 128, 1) > 0                   # NT * C = 2^31 - 128: the largest allowed at C = 128


def _maps(capacities, pieces):
  """The item maps ShardedVideoIndex.add builds for pieces of the given sizes: (global -> shard, global -> local)."""
  from mmt_amd.search import place
  fills = [0] * len(capacities)
  shard_of, local_of = [], []
  for n in pieces:
    for s, count in place(capacities, fills, n):
      shard_of += [s] * count
      local_of += range(fills[s], fills[s] + count)
      fills[s] += count
  return torch.tensor(shard_of), torch.tensor(local_of)


def test_sets_must_be_whole_on_one_shard_in_order_at_a_multiple_of_the_set_size():
  from mmt_amd.search import sets_whole
  # per-shard capacity a multiple of C, pieces of whole sets: whole, also where a piece spills (235 + 65)
  shard_of, local_of = _maps([235] * 3, [300, 100, 300])
  assert shard_of[234].item() == 0 and shard_of[235].item() == 1 and shard_of[300].item() == 2     # it did spill
  assert bool(sets_whole(shard_of, local_of, 5)) and bool(sets_whole(shard_of, local_of, 1))
  assert not bool(sets_whole(shard_of[:696], local_of[:696], 3))      # 235 is no multiple of 3: a set straddles the spill
  # the spilling layout of tests/test_index_sharded_gpu.py: a piece of 129 items on a shard of its own splits the set at 428
  shard_of, local_of = _maps([234] * 3, [300, 129, 271])
  assert not bool(sets_whole(shard_of, local_of, 2)) and bool(sets_whole(shard_of, local_of, 1))
  assert bool(sets_whole(shard_of[:300], local_of[:300], 6)) and not bool(sets_whole(shard_of[:300], local_of[:300], 4))
  # whole and on one shard, but starting off a multiple of C there; and whole but out of order
  assert not bool(sets_whole(torch.tensor([0, 1, 1, 0]), torch.tensor([0, 0, 1, 1]), 2))
  assert not bool(sets_whole(torch.tensor([0, 0, 0, 0]), torch.tensor([1, 2, 3, 4]), 2))
  assert not bool(sets_whole(torch.tensor([0, 0, 0, 0]), torch.tensor([1, 0, 2, 3]), 2))
  assert bool(sets_whole(torch.tensor([1, 1, 0, 0]), torch.tensor([0, 1, 0, 1]), 2))
  # one contiguous range per shard (the constructor's layout): whole iff every range is a multiple of C
  shard_of, local_of = _maps([8, 7], [8, 7])
  assert not bool(sets_whole(shard_of, local_of, 3)) and bool(sets_whole(shard_of[:12], local_of[:12], 4))


def test_mean_over_the_gallery_axis_of_the_reference_indep_similarities_is_its_avg_mode():
  """model/model.py:826-831 seen from the video: the mean over a video's captions of the 'indep' similarities, with the
  captions as the stored items, is sims_avg transposed.  Tolerance: the 1e-5 tests/test_oracle_golden.py uses on this file."""
  g = load_npz('sim_loss_metric')
  indep, avg = g['sims_indep'], g['sims_avg']
  b, c = avg.shape[0], indep.shape[0] // avg.shape[0]
  assert indep.shape == (b * c, b) and c == 3
  iw = np.full(b * c, F32(1) / F32(c), F32)
  v2t = brute_pooled(indep, c, iw, 'mean').T                # [video, caption set]: brute_pooled of the transposed matrix, .T
  assert v2t.shape == (b, b) and np.abs(v2t - avg.T).max() < 1e-5


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd.search import MAX_ITEM_SET, ItemPooling, ShardedItemPooling, ShardedVideoIndex, VideoIndex
  assert MAX_ITEM_SET == 128
  index = hollow(6)
  for bad in (0, 129, -1):
    with pytest.raises(ValueError, match=r'set_size must lie in 1\.\.128'):
      index.item_pooling(bad)
  for bad in (2.0, True, None, '3'):
    with pytest.raises(ValueError, match='set_size must be an int'):
      index.item_pooling(bad)
  for bad in ('avg', 'sum', None, 0):
    with pytest.raises(ValueError, match="mode must be 'mean' or 'max'"):
      index.item_pooling(2, mode=bad)
  with pytest.raises(ValueError, match='6 items are no whole number of sets of 4'):
    index.item_pooling(4)
  with pytest.raises(ValueError, match='holds no items'):
    hollow(0).item_pooling(2)
  w = torch.tensor([0.5, 0.5, 0.0, 1.0, -2.0, 0.0])
  for bad in (w.tolist(), w.numpy(), w.double(), w.to(torch.bfloat16), (w * 2).long()):
    with pytest.raises(ValueError, match='item_weights must be a float32 tensor'):
      index.item_pooling(2, bad)
  with pytest.raises(ValueError, match='index device'):
    index.item_pooling(2, w)                                       # host weights for a device index
  index.device = torch.device('cpu')                               # lets the value checks be reached with host tensors
  for bad in (w[:5], w.reshape(2, 3), w.reshape(6, 1), torch.zeros(7), torch.tensor(1.0)):
    with pytest.raises(ValueError, match=r'item_weights of shape \(6,\) or \(3, 2\) expected'):
      index.item_pooling(2, bad)
  for value in (float('nan'), float('inf'), -float('inf')):
    bad = w.clone()
    bad[4] = value
    with pytest.raises(ValueError, match='item_weights must be finite'):
      index.item_pooling(2, bad)
  with pytest.raises(ValueError, match='every set needs an item'):
    index.item_pooling(2, torch.tensor([0.5, 0.5, 0.0, -0.0, -2.0, 0.0]))
  if hollow is _hollow_sharded:
    # the layout check reads the item maps: sets of 2 whole on shard 0, then one split over shards 0 and 1
    index._shard_of, index._local_of = torch.tensor([0, 0, 0, 0, 0, 1, 9]), torch.tensor([0, 1, 2, 3, 4, 0, 9])
    with pytest.raises(ValueError, match='split across shards'):
      index.item_pooling(2, w)
    return
  ip = index.item_pooling(2, w, mode='max')                        # nothing of the build needs the device
  assert isinstance(ip, ItemPooling) and (ip.set_size, ip.num_sets, ip.num_items, ip.mode) == (2, 3, 6, 'max')
  assert ip.device == index.device and ip.weights.dtype == torch.float32 and ip.weights.tolist() == w.tolist()
  assert ip.weights.data_ptr() != w.data_ptr()                     # a copy of its own
  assert index.item_pooling(2, w.reshape(3, 2)).weights.tolist() == w.tolist()
  default = index.item_pooling(3)
  assert default.mode == 'mean' and default.weights.tolist() == [float(np.float32(1) / np.float32(3))] * 6
  assert index.item_pooling(1).weights.tolist() == [1.0] * 6
  # the calls: type, device, age and combinations of item_pooling come before the queries
  q, qw = torch.zeros(4, 2, 8), torch.zeros(4, 2)
  tg = torch.zeros(4, dtype=torch.int64)
  thr = torch.zeros(4)
  calls = [('search', lambda **kw: index.search(q, qw, **kw)), ('ranks', lambda **kw: index.rank_counts(q, qw, tg, **kw)),
           ('ranks', lambda **kw: index.ranks(q, qw, tg, **kw)), ('ranks', lambda **kw: index.target_scores(q, qw, tg, **kw)),
           ('ranks', lambda **kw: index.threshold_counts(q, qw, thr, **kw))]
  pool = index.pooling(2, 2)
  for who, call in calls:
    for foreign in (w, 2, 'mean', pool):
      with pytest.raises(ValueError, match=who + r': item_pooling must come from item_pooling\(\)'):
        call(item_pooling=foreign)
    with pytest.raises(ValueError, match='does not combine with pooling=, exclude= or norm='):
      call(item_pooling=ip, norm=object())
    with pytest.raises(ValueError, match='does not combine with pooling=, exclude= or norm='):
      call(item_pooling=ip, pooling=pool)
    with pytest.raises(ValueError, match='CUDA tensor'):
      call(item_pooling=ip)                                        # the queries themselves are host tensors
  with pytest.raises(ValueError, match='does not combine with pooling=, exclude= or norm='):
    index.search(q, qw, item_pooling=ip, exclude=torch.zeros(4, dtype=torch.int64))
  index.device = torch.device('cuda', 0)
  with pytest.raises(ValueError, match='search: the item pooling is on cpu, the index on cuda:0'):
    index.search(q, qw, item_pooling=ip)
  index.device = torch.device('cpu')
  index.num_items = 8                                              # a further `add`
  with pytest.raises(ValueError, match='search: the item pooling was built for 6 items, the index holds 8'):
    index.search(q, qw, item_pooling=ip)
  index.num_items = 6
  # targets are set numbers: the range is that of the sets; a subset must be one of the sets
  index._queries = lambda embds, weights: (embds, weights)
  with pytest.raises(ValueError, match=r'targets must lie in -1 \.\. 2, got 0 \.\. 3'):
    index.rank_counts(q, qw, torch.tensor([0, 1, 2, 3]), item_pooling=ip)
  with pytest.raises(ValueError, match=r'targets must lie in -1 \.\. 2, got -2 \.\. 0'):
    index.target_scores(q, qw, torch.tensor([0, -1, -2, 0]), item_pooling=ip)
  for bad in (torch.ones(6, dtype=torch.bool), torch.tensor([3]), torch.tensor([-1]), torch.zeros(3, dtype=torch.bool),
              torch.ones(3)):
    with pytest.raises(ValueError, match='subset: '):
      ip.subset(bad)
  # search_groups and range_search take no item pooling; both classes have one surface
  for method in ('search_groups', 'range_search'):
    assert 'item_pooling' not in inspect.signature(getattr(VideoIndex, method)).parameters
    assert 'item_pooling' not in inspect.signature(getattr(ShardedVideoIndex, method)).parameters
  for method in ('item_pooling', 'search', 'rank_counts', 'ranks'):
    assert (inspect.signature(getattr(ShardedVideoIndex, method)).parameters.keys() ==
            inspect.signature(getattr(VideoIndex, method)).parameters.keys())
    if method != 'item_pooling':
      assert inspect.signature(getattr(VideoIndex, method)).parameters['item_pooling'].default is None
  assert list(inspect.signature(VideoIndex.item_pooling).parameters) == ['self', 'set_size', 'item_weights', 'mode']
  assert inspect.signature(VideoIndex.item_pooling).parameters['mode'].default == 'mean'
  for method in ('target_scores', 'threshold_counts'):
    assert inspect.signature(getattr(VideoIndex, method)).parameters['item_pooling'].default is None
  assert ShardedItemPooling is not ItemPooling


def test_the_metric_refuses_what_avg_mode_does_not_combine_with():
  from mmt_amd.metric import retrieval_metrics_indexed
  vid, txt, vw, tw = np.zeros((2, 1, 8), F32), np.zeros((2, 1, 3, 8), F32), np.ones((2, 1), F32), np.ones((2, 3, 1), F32)
  assert inspect.signature(retrieval_metrics_indexed).parameters['caption_mode'].default == 'indep'
  with pytest.raises(ValueError, match="caption_mode must be 'indep' or 'avg'"):
    retrieval_metrics_indexed(vid, txt, vw, tw, caption_mode='max')
  for extra in ({'query_masks': np.ones((2, 3))}, {'text_bank': (txt, tw), 'beta': 20.0}, {'video_bank': (vid, vw), 'beta': 20.0}):
    with pytest.raises(ValueError, match="caption_mode='avg' does not combine with"):
      retrieval_metrics_indexed(vid, txt, vw, tw, caption_mode='avg', **extra)
