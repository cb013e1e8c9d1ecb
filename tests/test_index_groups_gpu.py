"""VideoIndex.search_groups / ShardedVideoIndex.search_groups (mmt_search_topk_groups, its bf16 form and
mmt_search_merge_group_lists): the k best groups of a gallery whose items carry a group id, each with its best item.

  1. lattice inputs, where fp32, bf16 and fp64 agree bit for bit and ties abound: groups, items and score bits equal
     brute_groups on the fp64 scores, for six groupings and k in {1, 10, 128};
  2. random inputs: equal to brute_groups on the device's own score matrix (target_scores over every item);
  3. consistent with search (singletons, one group), subsets, query tiles;  4. sharded equals monolithic;
  5. no buffer that grows with NQ * NV or NQ * num_groups."""
import functools

import numpy as np
import pytest
import torch

from tests.test_index_groups_cpu import best_first, padded_groups
from tests.test_index_ranks_gpu import _dev, _lattice, _random
from tests.test_index_sharded_gpu import _spilling, _whole
from tests.test_search_gpu import _cuda, _ref_sims

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
DTYPES = [torch.float32, torch.bfloat16]
INF = float('inf')

# (nq, nv, M, d): across the query block (64), the tile (128), 128-column chunks and several of them; the last has 256-item
# chunks, two tiles per block, and a last chunk of 8 items
LATTICE = [(1, 1, 1, 8), (63, 127, 7, 8), (65, 129, 2, 8), (130, 8193, 3, 64), (513, 14600, 1, 8)]
RANDOM = [(1, 1), (63, 127), (65, 129), (130, 4097)]   # (nq, nv) with M = 7, d = 16
KS = (1, 10, 128)


def _groupings(nv):
  """name -> int64 [nv]: non-dense singletons; one group; runs of 5 (they straddle tile and chunk borders); strided (every
  group has members in every tile and chunk: the merge must de-duplicate); flood (items 256 .. 555 one group: more than
  k + 64 same-group candidates in one chunk); random labels over nv // 3 ids."""
  every = np.arange(nv, dtype=np.int64)
  flood = 7 * every + 3
  flood[256:556] = 1
  return {'singletons': 7 * every + 3, 'one': np.full(nv, 2 ** 31 - 2, np.int64), 'runs': every // 5, 'strided': every % 37,
          'flood': flood, 'random': np.random.default_rng(nv).integers(0, max(1, nv // 3), nv) * 5}


def _assert_groups(got, want, what=None):
  scores, groups, items = (x.cpu().numpy() for x in got)
  for x, dtype in zip(got, (torch.float32, torch.int64, torch.int64)):
    assert x.dtype == dtype and tuple(x.shape) == want[0].shape and x.device == DEV, what
  wrong = [(items != want[2]).sum(), (groups != want[1]).sum(), (scores.view(np.int32) != want[0].view(np.int32)).sum()]
  print('%s: %d slots, wrong items %d, groups %d, score bits %d' % (what, items.size, *wrong))
  assert np.array_equal(items, want[2]), what
  assert np.array_equal(groups, want[1]), what
  assert np.array_equal(scores.view(np.int32), want[0].view(np.int32)), what


def _same(a, b):
  return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and a[0].shape == b[0].shape and \
      torch.equal(a[0].contiguous().view(torch.int32), b[0].contiguous().view(torch.int32))


# ---- 1. lattice inputs ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _lattice_case(case):
  """The lattice of tests/test_index_ranks_gpu.py at T = 1 and its fp64 scores, which are float32 values bit for bit."""
  q, qw, g, gw = _lattice(*LATTICE[case], 1)[:4]
  ref = _ref_sims(q, qw, g, gw)
  ref32 = ref.astype(np.float32) + np.float32(0)       # the key of the kernels does not tell -0 from +0
  assert np.array_equal(ref, ref32)
  ref32.setflags(write=False)
  return q, qw, g, gw, ref32, best_first(ref32)


@functools.lru_cache(maxsize=None)
def _lattice_expect(case, name):
  """The expectation at k = 128, computed once for both dtypes; a smaller k is its first columns."""
  gids = _groupings(LATTICE[case][1])[name]
  ref, order = _lattice_case(case)[4:]
  return padded_groups(ref, gids, min(128, np.unique(gids).size), order=order)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', range(len(LATTICE)), ids=['x'.join(map(str, s)) for s in LATTICE])
def test_groups_are_exact_on_lattice_inputs(case, dtype):
  from mmt_amd import _lib
  from mmt_amd.search import VideoIndex
  nq, nv, m, d = LATTICE[case]
  q, qw, g, gw, ref, _ = _lattice_case(case)
  if case == len(LATTICE) - 1:
    # 9 query tiles x 58 chunks of 256 items >= 512 blocks: every block walks two tiles and carries its lists across them
    assert _lib.lib().mmt_topk_workspace_keys(nq, nv, 10) == nq * 58 * 10 and nv - 57 * 256 == 8
  if case % 2 and nv > 1:
    index = VideoIndex.empty(nv + 200, m, d, DEV, dtype=dtype)      # two pieces and spare capacity
    index.add(_dev(g[:nv // 3]), _dev(gw[:nv // 3]))
    index.add(_dev(g[nv // 3:]), _dev(gw[nv // 3:]))
    assert index.num_items == nv < index.capacity
  else:
    index = VideoIndex(_dev(g), _dev(gw), dtype=dtype)
  qd, qwd = _dev(q), _dev(qw)
  for name, gids in _groupings(nv).items():
    grp = index.grouping(_dev(gids))
    n_groups = np.unique(gids).size
    assert grp.num_groups == n_groups and grp.num_items == nv and grp.device == DEV and grp.ids.dtype == torch.int32
    for k in KS:
      got = index.search_groups(qd, qwd, grp, k=k)
      assert got[0].shape == (nq, min(k, n_groups))
      _assert_groups(got, tuple(x[:, :k] for x in _lattice_expect(case, name)), (name, k))
  none = index.search_groups(qd[:0], qwd[:0], grp, k=10)            # no queries: empty outputs, no launch
  assert [tuple(x.shape) for x in none] == [(0, min(10, n_groups))] * 3
  assert [x.dtype for x in none] == [torch.float32, torch.int64, torch.int64] and none[0].device == DEV


# ---- 2. random inputs against the device's own scores ----------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_case(nq, nv, dtype):
  """A random index, its queries and its own score matrix: target_scores with every item as a target."""
  from mmt_amd.search import VideoIndex
  q, qw, g, gw = _random(nq, nv, 7, 16, nq + 3 * nv)
  index = VideoIndex(g, gw, dtype=dtype)
  matrix = index.target_scores(q, qw, torch.arange(nv, device=DEV).repeat(nq, 1)).cpu().numpy()
  assert matrix.shape == (nq, nv) and not np.isnan(matrix).any() and not (np.signbit(matrix) & (matrix == 0)).any()
  matrix.setflags(write=False)
  return index, q, qw, matrix, best_first(matrix)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv', RANDOM)
def test_groups_equal_the_definition_on_the_scores_of_the_scan(nq, nv, dtype):
  index, q, qw, matrix, order = _random_case(nq, nv, dtype)
  for name, gids in _groupings(nv).items():
    grp = index.grouping(_cuda(gids))
    want = padded_groups(matrix, gids, min(128, grp.num_groups), order=order)
    for k in KS:
      _assert_groups(index.search_groups(q, qw, grp, k=k), tuple(x[:, :k] for x in want), (name, k))
  assert _same(index.search_groups(q, qw, grp, k=10), index.search_groups(q, qw, grp, k=10))       # bit-reproducible
  if nq % 5 == 0:   # the text layout of `search`: (B, M, C, d) / (B, C, M) are rows b * C + c
    q4 = q.reshape(nq // 5, 5, 7, 16).permute(0, 2, 1, 3).contiguous()
    assert _same(index.search_groups(q4, qw.reshape(nq // 5, 5, 7), grp, k=10), index.search_groups(q, qw, grp, k=10))


# ---- 3. consistency ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('nq,nv', RANDOM)
def test_consistent_with_search(nq, nv, dtype):
  index, q, qw, matrix, order = _random_case(nq, nv, dtype)
  single = index.grouping(_cuda(7 * np.arange(nv, dtype=np.int64) + 3))
  one = index.grouping(_cuda(np.full(nv, 5, np.int64)))
  for k in KS:
    s, i = index.search(q, qw, k=k)
    gs, gg, gi = index.search_groups(q, qw, single, k=k)
    assert torch.equal(gi, i) and torch.equal(gg, 7 * i + 3)        # singletons: `search`, and groups map back to items
    assert torch.equal(gs.view(torch.int32), s.contiguous().view(torch.int32))
    s, i = index.search(q, qw, k=1)
    gs, gg, gi = index.search_groups(q, qw, one, k=k)                # one group: the best item, whatever k
    assert gs.shape == (nq, 1) and torch.equal(gi, i) and bool((gg == 5).all())
    assert torch.equal(gs.view(torch.int32), s.contiguous().view(torch.int32))


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_subsets_on_random_inputs(dtype):
  """130 x 4097, chunks of one tile: a random half; every group's best member for query 0 removed (the representative
  changes, the group stays); whole tiles emptied; a group wholly removed (the (-inf, -1, -1) tail)."""
  nq, nv = RANDOM[-1]
  index, q, qw, matrix, order = _random_case(nq, nv, dtype)
  every = np.arange(nv)
  for name in ('runs', 'strided', 'flood'):
    gids = _groupings(nv)[name]
    grp = index.grouping(_cuda(gids))
    n_groups = grp.num_groups
    best0 = np.ones(nv, bool)
    best0[padded_groups(matrix[:1], gids, n_groups, order=order[:1])[2][0]] = False
    masks = {'random_half': np.random.default_rng(4).random(nv) < 0.5, 'without_best_of_query_0': best0,
             'without_tiles_1_to_4': (every < 128) | (every >= 640), 'without_a_group': gids != gids[300]}
    for mask_name, mask in masks.items():
      sub = index.subset(_cuda(mask))
      want = padded_groups(matrix, gids, min(128, n_groups), mask, order)
      for k in (10, 128):
        got = index.search_groups(q, qw, grp, k=k, subset=sub)
        _assert_groups(got, tuple(x[:, :k] for x in want), (name, mask_name, k))
    if n_groups <= 128:                                            # strided: 37 groups, one of them removed
      assert bool((got[1][:, -1] == -1).all()) and bool((got[2][:, -1] == -1).all()) and bool((got[0][:, -1] == -INF).all())
      assert bool((got[1][:, :-1] >= 0).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_a_subset_that_empties_tiles_and_a_whole_chunk(dtype):
  """513 x 14600, 256-item chunks of two tiles: the mask drops chunk 1 whole, the second tile of chunk 4, the first of
  chunk 6 and a random half of the rest.  Then a stale subset and a stale grouping are refused."""
  from mmt_amd.search import VideoIndex
  case = len(LATTICE) - 1
  nq, nv, m, d = LATTICE[case]
  q, qw, g, gw, ref, order = _lattice_case(case)
  mask = np.random.default_rng(9).random(nv) < 0.5
  every = np.arange(nv)
  mask[(every >= 256) & (every < 512)] = False
  mask[(every >= 4 * 256 + 128) & (every < 5 * 256)] = False
  mask[(every >= 6 * 256) & (every < 6 * 256 + 128)] = False
  index = VideoIndex.empty(nv + 1, m, d, DEV, dtype=dtype)
  index.add(_dev(g), _dev(gw))
  sub = index.subset(_cuda(mask))
  grps = {}
  for name in ('runs', 'strided'):
    gids = _groupings(nv)[name]
    grps[name] = index.grouping(_dev(gids))
    want = padded_groups(ref, gids, min(128, grps[name].num_groups), mask, order)
    for k in (10, 128):
      got = index.search_groups(_dev(q), _dev(qw), grps[name], k=k, subset=sub)
      _assert_groups(got, tuple(x[:, :k] for x in want), (name, k))
  index.add(_dev(g[:1]), _dev(gw[:1]))
  with pytest.raises(ValueError, match='the grouping was built for %d items, the index holds %d' % (nv, nv + 1)):
    index.search_groups(_dev(q), _dev(qw), grps['runs'])
  fresh = index.grouping(_dev(np.arange(nv + 1) // 5))
  with pytest.raises(ValueError, match='the subset was built for %d items, the index holds %d' % (nv, nv + 1)):
    index.search_groups(_dev(q), _dev(qw), fresh, subset=sub)


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_query_tiles_do_not_change_the_result(dtype):
  nq, nv = RANDOM[-1]
  index, q, qw, matrix, order = _random_case(nq, nv, dtype)
  grp = index.grouping(_cuda(_groupings(nv)['runs']))
  whole = index.search_groups(q, qw, grp, k=10)
  parts = [index.search_groups(q[a:b], qw[a:b], grp, k=10) for a, b in ((0, 64), (64, 128), (128, 130))]
  assert _same(tuple(torch.cat([p[j] for p in parts]) for j in range(3)), whole)


# ---- 4. sharded -------------------------------------------------------------------------------------------------------

def _five_with_an_empty_shard(g, gw, dtype):
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex.empty(1000, g.shape[1], g.shape[2], [DEV] * 5, dtype=dtype)
  assert index.add(g, gw) == (0, 700)                         # one chunk that spills three times; the last shard stays empty
  assert index.shard_sizes == [200, 200, 200, 100, 0]
  return index


@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
@pytest.mark.parametrize('build', [_whole(1), _spilling, _five_with_an_empty_shard], ids=['1', '3_spilling', '5_one_empty'])
def test_sharded_equals_monolithic_bit_for_bit(build, dtype):
  from mmt_amd.search import ShardedGrouping, VideoIndex
  nq, nv, m, d = 65, 700, 3, 8
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  for twin in (nv // 2, nv - 1):                              # copies of item 0 on other shards: ties across shards
    g[twin], gw[twin] = g[0], gw[0]
  qw[nq // 2] = 0                                             # every score 0: one tie over all shards
  mono = VideoIndex(g, gw, dtype=dtype)
  shard = build(g, gw, dtype)
  assert shard.num_items == nv
  every = torch.arange(nv, device=DEV)
  masks = {None: None, 'every_other': every % 2 == 1, 'one_item': every == nv // 2}
  if len(shard.shards) > 1:
    masks['without_shard_0'] = shard._shard_of[:nv] != 0     # a shard without an allowed item
  for name, gids in (('strided', every % 37), ('runs', every // 5)):   # strided: every group on every shard
    grp_m, grp_s = mono.grouping(gids), shard.grouping(gids)
    assert isinstance(grp_s, ShardedGrouping) and grp_s.num_groups == grp_m.num_groups and grp_s.device == DEV
    assert torch.equal(grp_s.ids, grp_m.ids) and grp_s.num_items == nv
    for mask_name, mask in masks.items():
      sub_m, sub_s = (None, None) if mask is None else (mono.subset(mask), shard.subset(mask))
      for k in KS:
        want = mono.search_groups(q, qw, grp_m, k=k, subset=sub_m)
        got = shard.search_groups(q, qw, grp_s, k=k, subset=sub_s)
        assert all(x.device == DEV for x in got)
        assert _same(got, want), (name, mask_name, k)
  none = shard.search_groups(q[:0], qw[:0], grp_s, k=10)
  assert [tuple(x.shape) for x in none] == [(0, 10)] * 3
  if shard.num_items < shard.capacity:
    shard.add(g[:1], gw[:1])
    with pytest.raises(ValueError, match='the grouping was built for %d items' % nv):
      shard.search_groups(q, qw, grp_s)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')
@pytest.mark.parametrize('dtype', DTYPES, ids=['fp32', 'bf16'])
def test_two_devices_equal_one(dtype):
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  nq, nv, m, d = 65, 700, 3, 8
  q, qw, g, gw = _random(nq, nv, m, d, nq + nv + m + d)
  g[nv - 1], gw[nv - 1] = g[0], gw[0]
  mono = VideoIndex(g, gw, dtype=dtype)
  index = ShardedVideoIndex.empty(700, m, d, ['cuda:0', 'cuda:1'], dtype=dtype)
  for a, b in ((0, 300), (300, 429), (429, 700)):
    index.add(g[a:b], gw[a:b])
  every = torch.arange(nv, device=DEV)
  mask = every % 2 == 1
  for gids in (every % 37, every // 5):
    grp_m, grp_s = mono.grouping(gids), index.grouping(gids)
    for sub_m, sub_s in ((None, None), (mono.subset(mask), index.subset(mask))):
      got = index.search_groups(q, qw, grp_s, k=10, subset=sub_s)
      assert got[0].device == DEV and _same(got, mono.search_groups(q, qw, grp_m, k=10, subset=sub_m))
  with pytest.raises(ValueError, match='must be on the index device'):
    index.grouping((every % 37).to(torch.device('cuda', 1)))


# ---- 5. memory --------------------------------------------------------------------------------------------------------

def test_search_groups_allocates_no_quadratic_buffer():
  """64 x 262 144, M = 1, d = 8, bf16, runs of 8 (32 768 groups), k = 10.  What the call holds at its peak: the outputs,
  the folded queries and the chunk lists (mmt_topk_workspace_keys), together far below 3 MiB, where the score matrix would
  be 64 MiB and a [NQ, num_groups] array 8 MiB."""
  from mmt_amd import _lib
  from mmt_amd.search import VideoIndex
  nq, nv, m, d, k = 64, 262144, 1, 8, 10
  gen = torch.Generator(device=DEV).manual_seed(8)
  index = VideoIndex(torch.rand(nv, m, d, device=DEV, generator=gen) - 0.5, torch.rand(nv, m, device=DEV, generator=gen) + 0.5,
                     dtype=torch.bfloat16)
  q = torch.rand(nq, m, d, device=DEV, generator=gen) - 0.5
  qw = torch.rand(nq, m, device=DEV, generator=gen) + 0.5
  gids = torch.arange(nv, device=DEV) // 8
  grp = index.grouping(gids)
  assert grp.num_groups == nv // 8
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  scores, groups, items = index.search_groups(q, qw, grp, k=k)
  torch.cuda.synchronize()
  growth = torch.cuda.max_memory_allocated() - base
  lists = 8 * _lib.lib().mmt_topk_workspace_keys(nq, nv, k)
  print('allocator peak growth %.1f KiB, chunk lists %.1f KiB, matrix %.1f KiB' % (growth / 1024, lists / 1024, nq * nv * 4 / 1024))
  assert lists + 20 * nq * k + 32 * nq <= 3 << 20
  assert growth < nq * nv * 4 // 4, growth
  # and the answer is that of `search` over all items, collapsed: the 128 best items hold at least 10 groups here
  s, i = index.search(q, qw, k=128)
  for r in range(0, nq, 7):
    seen, want = set(), []
    for item in i[r].tolist():
      if item // 8 not in seen:
        seen.add(item // 8)
        want.append(item)
    assert len(want) >= k and items[r].tolist() == want[:k] and groups[r].tolist() == [w // 8 for w in want[:k]]
    assert torch.equal(scores[r].view(torch.int32), s[r][[i[r].tolist().index(w) for w in want[:k]]].view(torch.int32))
