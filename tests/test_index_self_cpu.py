"""The host side of the gallery self-join (VideoIndex.neighbours, neighbour_range, duplicate_groups; mmt_search_self_topk,
mmt_search_self_range_count, mmt_search_self_range_fill) without a GPU: the brute-force order the GPU tests hold the
kernels to and the component function, on cases worked by hand, on CPU tensors; the header, the ctypes table and the
library; every gate of every new entry; the argument errors that need no device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.test_index_groups_cpu import _hollow_index, _hollow_sharded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {'mmt_search_self_topk': 20, 'mmt_search_self_range_count': 19, 'mmt_search_self_range_fill': 21}
SIZES = {'mmt_self_topk_workspace_keys': 3, 'mmt_self_range_workspace_ints': 2}
INF = float('inf')


def brute_neighbours(sims, own, k, allowed=None):
  """The self-join's top-k restated on a given matrix, on CPU tensors: sims float32 [R, N], row r the sims of row item r
  to the items 0 .. N - 1; own int64 [R], the item row r must not meet (-1 = none): it goes by NUMBER, whatever it scores;
  allowed bool [N] or None -> (scores float32 [R, k], indices int64 [R, k]): the candidates in `search`'s order -- sim
  descending, -0 tied with +0 and returned as +0, equal sims by ascending item -- cut to k and padded with (-inf, -1)."""
  from mmt_amd.search import search_order
  r, n = sims.shape
  scores, indices = torch.full((r, k), -INF, dtype=torch.float32), torch.full((r, k), -1, dtype=torch.int64)
  every = torch.arange(n)
  for i in range(r):
    ok = every != own[i]
    if allowed is not None:
      ok = ok & allowed
    cand = every[ok]
    best = cand[search_order(sims[i, cand], cand)[:k]]
    scores[i, :best.shape[0]], indices[i, :best.shape[0]] = sims[i, best] + 0.0, best
  return scores, indices


def brute_range(sims, own, thr, allowed=None):
  """The self-join's range restated likewise: thr float32 [R] -> (offsets int64 [R + 1], indices int64, scores float32):
  per row every candidate with sims >= thr (a plain compare: NaN hits nothing, -inf everything) by ascending item, the
  scores as they are."""
  r, n = sims.shape
  every = torch.arange(n)
  hit = (sims >= thr[:, None]) & (every[None, :] != own[:, None])
  if allowed is not None:
    hit = hit & allowed[None, :]
  offsets = torch.zeros(r + 1, dtype=torch.int64)
  offsets[1:] = torch.cumsum(hit.sum(1), 0)
  at = torch.nonzero(hit)   # row-major: rows ascending, items ascending within a row
  return offsets, at[:, 1].contiguous(), sims[hit]


def test_the_brute_force_order_on_cases_worked_by_hand():
  from mmt_amd.search import search_order
  # item 1 and item 3 tie at 0.5: the lower number first; -0 ties with +0: item 2 before item 4; -inf is a score like any
  sims = torch.tensor([[0.25, 0.5, -0.0, 0.5, 0.0, -INF]])
  assert search_order(sims[0], torch.arange(6)).tolist() == [1, 3, 0, 2, 4, 5]
  assert search_order(torch.tensor([1.0, 1.0, 2.0]), torch.tensor([9, 4, 6])).tolist() == [2, 1, 0]   # numbers, not positions
  s, i = brute_neighbours(sims, torch.tensor([1]), 3)
  assert i.tolist() == [[3, 0, 2]] and s.tolist() == [[0.5, 0.25, 0.0]]
  assert not torch.signbit(s[0, 2])                                   # the -0 of item 2 comes back as +0
  s, i = brute_neighbours(sims, torch.tensor([-1]), 8)                # no self pair; more room than candidates
  assert i.tolist() == [[1, 3, 0, 2, 4, 5, -1, -1]] and s[0, 5] == -INF and s[0, 6] == -INF
  # the self pair goes by number: row item 0 scores 1.0 with itself and with its exact copy, item 2; the copy stays
  two = torch.tensor([[1.0, 0.5, 1.0], [0.5, 2.0, 0.5]])
  s, i = brute_neighbours(two, torch.tensor([0, 1]), 2)
  assert i.tolist() == [[2, 1], [0, 2]] and s.tolist() == [[1.0, 0.5], [0.5, 0.5]]
  s, i = brute_neighbours(two, torch.tensor([0, 1]), 2, allowed=torch.tensor([True, True, False]))
  assert i.tolist() == [[1, -1], [0, -1]]
  # the range: >= is plain, NaN hits nothing, -inf everything but the row's own item; rows ascend by item
  thr = torch.tensor([1.0, float('nan')])
  offsets, items, scores = brute_range(two, torch.tensor([0, 1]), thr)
  assert offsets.tolist() == [0, 1, 1] and items.tolist() == [2] and scores.tolist() == [1.0]
  offsets, items, scores = brute_range(two, torch.tensor([0, 1]), torch.tensor([-INF, 0.5]))
  assert offsets.tolist() == [0, 2, 4] and items.tolist() == [1, 2, 0, 2] and scores.tolist() == [0.5, 1.0, 0.5, 0.5]
  offsets, items, _ = brute_range(two, torch.tensor([-1, -1]), torch.tensor([1.0, 1.0]))
  assert offsets.tolist() == [0, 2, 3] and items.tolist() == [0, 2, 1]             # source=: no self pair is removed


def test_connected_components_on_cases_worked_by_hand():
  from mmt_amd.search import connected_components
  none = torch.zeros(0, dtype=torch.int64)
  assert connected_components(4, none, none).tolist() == [0, 1, 2, 3]
  # the chain 0 - 1 - ... - 6 given from its far end, 7 alone, 8 hanging on 3: several rounds of propagation
  src, dst = torch.tensor([6, 5, 4, 3, 2, 1, 8]), torch.tensor([5, 4, 3, 2, 1, 0, 3])
  labels = connected_components(9, src, dst)
  assert labels.dtype == torch.int64 and labels.tolist() == [0, 0, 0, 0, 0, 0, 0, 7, 0]
  assert connected_components(9, dst, src).tolist() == labels.tolist()                      # direction does not matter
  assert connected_components(9, torch.cat([src, src]), torch.cat([dst, dst])).tolist() == labels.tolist()   # nor repeats
  # two components whose minima are not their first-listed members; a self loop; a long chain in a scrambled order
  assert connected_components(6, torch.tensor([5, 4, 2, 2]), torch.tensor([3, 1, 4, 2])).tolist() == [0, 1, 1, 3, 1, 3]
  n = 257
  order = torch.randperm(n - 1, generator=torch.Generator().manual_seed(0))
  assert connected_components(n, order + 1, order).tolist() == [0] * n
  odd = order[order % 2 == 1]                                                               # 2j - 1 ~ 2j: pairs, 0 alone
  want = [0] + [2 * ((g + 1) // 2) - 1 for g in range(1, n)]
  assert connected_components(n, odd, odd + 1).tolist() == want


def _functions():
  from mmt_amd import _lib
  handle = ctypes.CDLL(_lib.LIB_PATH)
  fns = {}
  for name in list(ENTRIES) + list(SIZES):
    fns[name] = getattr(handle, name)
    fns[name].restype, fns[name].argtypes = _lib.SIGNATURES[name]
  return handle, fns


def test_header_bindings_and_library_agree_on_the_new_entries():
  from mmt_amd import _lib
  src = open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read()
  handle, _ = _functions()
  for name, arity in {**ENTRIES, **SIZES}.items():
    kind = 'int' if name in ENTRIES else 'int64_t'
    m = re.search(r'\b%s %s\(([^;]*?)\);' % (kind, name), src)
    assert m, name + ' is not declared in mmt_hip.h'
    params = [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]
    res, args = _lib.SIGNATURES[name]
    assert res is (ctypes.c_int if name in ENTRIES else ctypes.c_int64) and len(args) == len(params) == arity, name
    for p, a in zip(params, args):
      assert (a is ctypes.c_void_p) == ('*' in p), (name, p)
      assert (a is ctypes.c_int) == p.startswith('int '), (name, p)
    assert hasattr(handle, name)
  for name in ENTRIES:   # two stored operands, in the order A side, B side, storage, M, d
    params = re.search(r'\bint %s\(([^;]*?)\);' % name, src).group(1).replace('\n', ' ')
    names = [p.split()[-1].lstrip('*') for p in params.split(',')]
    assert names[:15] == ['a_rows', 'a_weights', 'a_scales', 'NA', 'items', 'self', 'R', 'g', 'gw', 'gscale', 'NV', 'subset',
                          'storage', 'M', 'd'], name
    assert names[-1] == 'stream'
  assert 'search_self.hip' in src and 'MmtSearchScan' not in re.search(r'int mmt_search_self_topk\([^;]*\);', src).group(0)
  assert handle.mmt_abi_version() == 6
  assert os.path.exists(os.path.join(ROOT, 'mmt_amd', 'csrc', 'search_self.hip'))


def test_workspace_sizes():
  _, fns = _functions()
  keys, ints = fns['mmt_self_topk_workspace_keys'], fns['mmt_self_range_workspace_ints']
  assert keys(300, 300, 10) == 300 * 3 * 10 and ints(300, 300) == 300 * 3        # one tile per chunk: three chunks
  assert keys(4096, 262144, 10) == 4096 * 64 * 10 and ints(4096, 262144) == 4096 * 64   # full-size chunks of 4096 columns
  assert keys(1, 1, 128) == 128 and ints(1, 1) == 1
  for bad in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 129), (-1, 5, 1)):
    assert keys(*bad) == -1, bad
  for bad in ((0, 5), (5, 0), (-3, 5)):
    assert ints(*bad) == -1, bad


A_SIDE = ['a_rows', 'a_weights', 'a_scales', 'NA', 'items', 'self', 'R']
B_SIDE = ['g', 'gw', 'gscale', 'NV', 'subset', 'storage', 'M', 'd']
TAILS = {'mmt_search_self_topk': ['k', 'ws', 'scores', 'index', 'stream'],
         'mmt_search_self_range_count': ['thr', 'ws', 'row_counts', 'stream'],
         'mmt_search_self_range_fill': ['thr', 'ws', 'offsets', 'indices', 'scores', 'stream']}


@pytest.mark.parametrize('name', list(ENTRIES))
def test_new_entries_gate_their_arguments_on_the_host(name):
  """Every refusal below returns before any launch: MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2.  The pointers are aligned and
  never dereferenced.  A knock-out of an argument gate is made with g off its boundary as well, so a gate that has gone
  missing shows as -2 (or as a launch)."""
  _, fns = _functions()
  fn, tail = fns[name], TAILS[name]
  buf = (ctypes.c_char * 256)()
  P = ctypes.addressof(buf) + -ctypes.addressof(buf) % 16
  names = A_SIDE + B_SIDE + tail
  assert len(names) == ENTRIES[name]
  for storage, mult in ((0, 4), (1, 8), (2, 16)):
    sc = P if storage == 2 else None
    good = dict(a_rows=P, a_weights=P, a_scales=sc, NA=9, items=P, self=P, R=3, g=P, gw=P, gscale=sc, NV=5, subset=P,
                storage=storage, M=2, d=32, stream=None)
    good.update({n: P for n in tail if n not in ('k', 'stream')})
    if 'k' in tail:
      good['k'] = 10

    def call(**changes):
      return fn(*[dict(good, **changes)[n] for n in names])
    for off in (4, 8):   # everything else in order: only the alignment is refused
      assert call(g=P + off) == -2 and call(a_rows=P + off) == -2 and call(subset=P + off) == -2, storage
    assert call(g=P + 8, items=None, self=None, subset=None) == -2, storage      # the three nullable ones
    assert call(g=P + 8, items=None, R=9) == -2, storage                        # R == NA without a row table
    bad = [dict(a_rows=None), dict(a_weights=None), dict(gw=None), dict(a_scales=None if storage == 2 else P),
           dict(gscale=None if storage == 2 else P), dict(storage=3), dict(storage=-1), dict(NA=0), dict(NA=-1), dict(R=0),
           dict(R=-1), dict(NV=0), dict(NV=-1), dict(M=0), dict(M=17), dict(d=0), dict(d=-16), dict(d=32 + mult // 2),
           dict(items=None, R=10)]
    bad += [{n: None} for n in tail if n not in ('k', 'stream')]
    if 'k' in tail:
      bad += [dict(k=0), dict(k=-1), dict(k=129)]
      assert call(g=P + 8, k=1) == -2 and call(g=P + 8, k=128) == -2, storage
    for changes in bad:
      assert call(**dict(dict(g=P + 8), **changes)) == -1, (storage, changes)
    assert call(g=None) == -1, storage
  # an fp32 width on a bf16 index, a bf16 width on an fp8 index
  assert fn(*[dict(good, storage=1, a_scales=None, gscale=None, d=4, g=P + 8)[n] for n in names]) == -1
  assert fn(*[dict(good, storage=2, d=8, g=P + 8)[n] for n in names]) == -1


@pytest.mark.parametrize('hollow', [_hollow_index, _hollow_sharded], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_are_raised_without_a_device(hollow):
  from mmt_amd import search
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  items = torch.zeros(3, dtype=torch.int64)
  index = hollow(5)
  calls = {'neighbours': lambda **kw: index.neighbours(**kw), 'neighbour_range': lambda **kw: index.neighbour_range(0.5, **kw),
           'duplicate_groups': lambda **kw: index.duplicate_groups(0.5, **kw)}
  for name, call in calls.items():
    for option in ('norm', 'pooling', 'item_pooling', 'grouping', 'after', 'exclude'):
      with pytest.raises(ValueError, match='%s: %s= is out of scope' % (name, option)):
        call(**{option: None})
    with pytest.raises(TypeError, match='unexpected keyword'):
      call(neighbors=3)
    with pytest.raises(ValueError, match=name + ': subset must come from'):
      call(subset=items)
    with pytest.raises(ValueError, match=name + ': the index holds no items'):
      empty = hollow(0)
      getattr(empty, name)(*(() if name == 'neighbours' else (0.5,)))
  for bad in (0, 129, -1, 2.0, True, None, 'all'):
    with pytest.raises(ValueError, match=r'neighbours: k must be an int in 1\.\.128'):
      index.neighbours(k=bad)
  for name in ('neighbours', 'neighbour_range'):
    call = calls[name]
    for bad in ([0, 1], 3, items.to(torch.int32), items.double(), items > 0):
      with pytest.raises(ValueError, match=name + ': items must be an int64 tensor'):
        call(items=bad)
    with pytest.raises(ValueError, match=name + ': items must be on the index device'):
      call(items=items)                                            # host items for a device index
  index.device = torch.device('cpu')                               # lets the later checks be reached with host tensors
  for name in ('neighbours', 'neighbour_range'):
    for bad in (items.reshape(3, 1), torch.tensor(3)):
      with pytest.raises(ValueError, match=name + r': items \[R\] expected'):
        calls[name](items=bad)
    for bad in (torch.tensor([0, 5]), torch.tensor([-1, 2])):
      with pytest.raises(ValueError, match=name + r': items must lie in 0 \.\. 4'):
        calls[name](items=bad)
  # source=: a VideoIndex of the same dtype, num_experts and dim on the same device; never on a sharded index
  other = _hollow_index(7)
  other.device = torch.device('cpu')
  for name in ('neighbours', 'neighbour_range'):
    call = calls[name]
    if hollow is _hollow_sharded:
      with pytest.raises(ValueError, match=name + ': source= is not available on a ShardedVideoIndex'):
        call(source=other)
      continue
    for bad in ('index', items, _hollow_sharded(5)):
      with pytest.raises(ValueError, match=name + ': source must be a VideoIndex'):
        call(source=bad)
    for field, value in (('num_experts', 3), ('dim', 16), ('dtype', torch.bfloat16)):
      wrong = _hollow_index(7)
      wrong.device = torch.device('cpu')
      setattr(wrong, field, value)
      with pytest.raises(ValueError, match=name + r': the source holds \(dtype, num_experts, dim\)'):
        call(source=wrong)
    with pytest.raises(ValueError, match=name + ': the source is on cuda:0, this index on cpu'):
      call(source=_hollow_index(7))
    with pytest.raises(ValueError, match=name + ': the source holds no items'):
      empty = _hollow_index(0)
      empty.device = torch.device('cpu')
      call(source=empty)
    with pytest.raises(ValueError, match=name + r': items must lie in 0 \.\. 6'):
      call(source=other, items=torch.tensor([7]))                  # `items` numbers the source
  # neighbour_range: order, max_hits and threshold in the words of range_search
  with pytest.raises(ValueError, match="neighbour_range: order must be 'index' or 'score'"):
    index.neighbour_range(0.5, order='item')
  for bad in (-1, 2.5, True, None):
    with pytest.raises(ValueError, match='neighbour_range: max_hits must be an int >= 0'):
      index.neighbour_range(0.5, max_hits=bad)
    with pytest.raises(ValueError, match='duplicate_groups: max_hits must be an int >= 0'):
      index.duplicate_groups(0.5, max_hits=bad)
  for bad in ('high', None, True, [0.5]):
    with pytest.raises(ValueError, match='neighbour_range: threshold must be a float or a float32 tensor'):
      index.neighbour_range(bad)
  with pytest.raises(ValueError, match='neighbour_range: threshold must be a float or a float32 tensor, got torch.float64'):
    index.neighbour_range(torch.zeros(5, dtype=torch.float64))
  with pytest.raises(ValueError, match=r'neighbour_range: threshold \[R\] expected'):
    index.neighbour_range(torch.zeros(5, 1))
  with pytest.raises(ValueError, match='neighbour_range: 5 rows but threshold'):
    index.neighbour_range(torch.zeros(4))
  with pytest.raises(ValueError, match='neighbour_range: 3 rows but threshold'):
    index.neighbour_range(torch.zeros(5), items=items)
  for bad in ('high', None, True, torch.zeros(5)):
    with pytest.raises(ValueError, match='duplicate_groups: threshold must be a float'):
      index.duplicate_groups(bad)
  for method in ('neighbours', 'neighbour_range', 'duplicate_groups'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)
  assert list(inspect.signature(VideoIndex.neighbours).parameters) == ['self', 'k', 'items', 'subset', 'source', 'unsupported']
  assert list(inspect.signature(VideoIndex.neighbour_range).parameters) == [
      'self', 'threshold', 'items', 'subset', 'source', 'order', 'max_hits', 'unsupported']
  assert list(inspect.signature(VideoIndex.duplicate_groups).parameters) == ['self', 'threshold', 'subset', 'max_hits', 'unsupported']
  defaults = inspect.signature(VideoIndex.neighbour_range).parameters
  assert inspect.signature(VideoIndex.neighbours).parameters['k'].default == 10
  assert defaults['order'].default == 'index' and defaults['max_hits'].default == search._MAX_HITS == 1 << 27
  assert 'the eleventh question' in search.__doc__.lower()
