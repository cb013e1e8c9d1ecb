"""Cursor paging on the GPU: VideoIndex.search(after=) (mmt_search_topk_after and its bf16 / fp8 / normalised forms) and
search_deep.  Every claim is one of bit identity: a page is the slice right behind its position in the complete ordered
list of the query's candidates, with the score bits `target_scores` gives the pair on the same index (with norm= its
normalised bits).  The reference is that call over all 777 items for the bits and the numpy definition of
tests.test_index_after_cpu for the lists; results are compared with torch.equal on the indices and on the int32 views of
the scores.  Shapes and data are those of the rescore tests."""
import numpy as np
import pytest
import torch

from tests.test_index_after_cpu import complete_list, slice_after
from tests.test_index_rescore_gpu import DEV, DTYPES, FP8, IDS, M, D, NQ, NV, _data, _index, _same, _three_shards_one_empty

pytestmark = pytest.mark.gpu
INF = float('inf')
PAD = 136                  # vacant columns behind a complete list: a page that starts anywhere is one gather
_cache = {}


def _bits(dtype, norm=None):
  """score(q, g) for all 130 x 777 pairs with the scan's own bits, float32 numpy; with a norm the normalised bits."""
  key = ('bits', dtype, None if norm is None else id(norm))
  if key not in _cache:
    _, _, q, qw = _data()
    targets = torch.arange(NV, device=DEV).expand(NQ, NV).contiguous()
    kwargs = {} if norm is None else {'norm': norm, 'dynamic': False}
    _cache[key] = _index(dtype).target_scores(q, qw, targets, **kwargs).cpu().numpy()
  return _cache[key]


def _padded(bits, allowed=None):
  """The complete ordered list of every row of a score matrix (numpy, computed on the host) -> (scores [NQ, NV + PAD],
  items [NQ, NV + PAD]) on the device, (-inf, -1) behind each row's candidates.  allowed: bool [NQ, NV] or None."""
  nq = bits.shape[0]
  s, i = np.full((nq, NV + PAD), -INF, np.float32), np.full((nq, NV + PAD), -1, np.int64)
  for r in range(nq):
    rs, ri = complete_list(bits[r], None if allowed is None else allowed[r])
    s[r, :ri.size], i[r, :ri.size] = rs, ri
  return torch.from_numpy(s).to(DEV), torch.from_numpy(i).to(DEV)


def _complete(dtype):
  if ('list', dtype) not in _cache:
    _cache['list', dtype] = _padded(_bits(dtype))
  return _cache['list', dtype]


def _pages_from(lists, start, k):
  """Rows start[r] .. start[r] + k - 1 of padded complete lists: what a page behind position start[r] - 1 must hold."""
  at = start[:, None] + torch.arange(k, device=DEV)[None]
  return torch.gather(lists[0], 1, at), torch.gather(lists[1], 1, at)


def _cursor_at(lists, start):
  """The cursor that stands right before position start[r] of each row's list: the entry at start[r] - 1, no cursor for 0,
  and -- since a list is padded with vacant slots -- exhausted behind its end."""
  at = (start - 1).clamp(min=0)[:, None]
  s, i = torch.gather(lists[0], 1, at)[:, 0], torch.gather(lists[1], 1, at)[:, 0]
  none = start == 0
  return torch.where(none, torch.full_like(s, INF), s), torch.where(none, torch.full_like(i, -1), i)


def _by_definition(bits, cursor, k, allowed=None):
  """slice_after row by row for any cursor (numpy) -> (scores [nq, k], items [nq, k]) on the device."""
  a_s, a_i = cursor[0].cpu().numpy(), cursor[1].cpu().numpy()
  rows = [slice_after(bits[r], a_s[r], a_i[r], k, None if allowed is None else allowed[r]) for r in range(a_s.shape[0])]
  return (torch.from_numpy(np.stack([r[0] for r in rows])).to(DEV), torch.from_numpy(np.stack([r[1] for r in rows])).to(DEV))


def _mixed_starts(nq):
  """A start per row: no cursor (0), exhausted (NV + 1: the cursor is a vacant slot), behind the last item (NV), before
  the last item, and everything in between -- inside the 60-way tie of rows 100 .. 139 / 500 .. 519 wherever it falls."""
  start = (torch.arange(nq, device=DEV) * 37) % (NV + 1)
  start[::5] = 0
  start[1::13] = NV + 1
  start[2::17] = NV
  if nq > 3:
    start[3] = NV - 1
  return start


@pytest.mark.parametrize('k', [10, 128])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_the_pages_of_a_full_traversal_are_the_complete_list_then_vacant(dtype, k):
  _, _, q, qw = _data()
  index, want = _index(dtype), _complete(dtype)
  assert (want[1][7, :NV] == torch.arange(NV, device=DEV)).all()        # the all-zero query: every item ties, by item number
  pages, cursor = [], None
  for _ in range(-(-NV // k) + 1):
    page = index.search(q, qw, k=k, after=cursor)
    assert page[0].shape == page[1].shape == (NQ, k) and page[0].dtype is torch.float32 and page[1].dtype is torch.int64
    pages.append(page)
    cursor = (page[0][:, -1], page[1][:, -1])
  got = tuple(torch.cat(parts, 1) for parts in zip(*pages))
  assert got[0].shape[1] >= NV + k                                     # the last page of all is vacant throughout
  assert _same((got[0][:, :NV], got[1][:, :NV]), (want[0][:, :NV], want[1][:, :NV]))
  assert (got[1][:, NV:] == -1).all() and torch.isneginf(got[0][:, NV:]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_without_a_cursor_the_page_is_the_search(dtype):
  _, _, q, qw = _data()
  index = _index(dtype)
  none = (torch.full((NQ,), INF, device=DEV), torch.full((NQ,), -1, device=DEV, dtype=torch.int64))
  for nq in (1, 65, 130):
    for k in (1, 10, 128):
      want = index.search(q[:nq], qw[:nq], k=k)
      assert _same(index.search(q[:nq], qw[:nq], k=k, after=None), want), (nq, k)
      assert _same(index.search(q[:nq], qw[:nq], k=k, after=(none[0][:nq], none[1][:nq])), want), (nq, k)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_one_call_mixes_rows_without_a_cursor_exhausted_and_mid_list(dtype):
  _, _, q, qw = _data()
  index, lists = _index(dtype), _complete(dtype)
  for nq in (1, 65, 130):       # a second query tile with one live row, a third with two
    start = _mixed_starts(nq) if nq > 1 else torch.tensor([120], device=DEV)
    cursor = _cursor_at((lists[0][:nq], lists[1][:nq]), start)
    for k in (1, 10, 128):
      got = index.search(q[:nq], qw[:nq], k=k, after=cursor)
      assert _same(got, _pages_from((lists[0][:nq], lists[1][:nq]), start, k)), (nq, k)
  start = _mixed_starts(NQ)
  exhausted = start >= NV
  after = _cursor_at(lists, start)
  assert (after[1][start == NV] >= 0).all() and (after[1][start > NV] == -1).all() and torch.isneginf(after[0][start > NV]).all()
  got = index.search(q, qw, k=10, after=after)
  assert (start == NV).any() and (start > NV).any() and (got[1][exhausted] == -1).all() and torch.isneginf(got[0][exhausted]).all()
  assert (got[1][3] >= 0).sum() == 1                                    # the row that stood before its last item
  whole = torch.full((130,), NV + 1, device=DEV)                            # every row exhausted: no block scores anything
  got = index.search(q, qw, k=10, after=_cursor_at(lists, whole))
  assert (got[1] == -1).all() and torch.isneginf(got[0]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_cursor_need_not_be_the_position_of_a_stored_item(dtype):
  _, _, q, qw = _data()
  index, bits, lists = _index(dtype), _bits(dtype), _complete(dtype)
  s = lists[0][:, :NV]
  # a score strictly between two neighbours of the list, with an arbitrary item number
  j = torch.full((NQ,), 200, device=DEV)
  hi, lo = s[:, 199], s[:, 200]
  mid = ((hi.double() + lo.double()) / 2).float()
  between = (mid < hi) & (mid > lo)
  assert between.sum() > 100                                            # not the all-zero query, whose neighbours tie
  a_s = torch.where(between, mid, hi)
  a_i = torch.where(between, torch.full_like(j, 400), lists[1][:, 199])
  for k in (10, 128):
    got = index.search(q, qw, k=k, after=(a_s, a_i))
    assert _same(got, _pages_from(lists, j, k)), k
    assert _same(got, _by_definition(bits, (a_s, a_i), k)), k
  # a tied score with an arbitrary item number: the copies of item 100 are rows 100 .. 139 and 500 .. 519
  tie = torch.from_numpy(bits[:, 100].copy()).to(DEV)
  for item in (0, 99, 119, 300, 519, 776):
    cursor = (tie, torch.full((NQ,), item, device=DEV))
    got = index.search(q, qw, k=128, after=cursor)
    assert _same(got, _by_definition(bits, cursor, 128)), item
  left = index.search(q, qw, k=128, after=(tie, torch.full((NQ,), 300, device=DEV)))[1]
  assert left[0, :20].tolist() == list(range(500, 520))                 # behind (the tie's score, 300): its members from 500 on
  # scores no item has: above everything, below everything, and the infinities as positions
  for value, start in ((1e30, 0), (INF, 0), (-1e30, NV), (-INF, NV)):
    cursor = (torch.full((NQ,), value, device=DEV), torch.zeros(NQ, device=DEV, dtype=torch.int64))
    assert _same(index.search(q, qw, k=10, after=cursor), _pages_from(lists, torch.full((NQ,), start, device=DEV), 10)), value


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_subset_and_exclusions_combine_with_the_cursor(dtype):
  _, _, q, qw = _data()
  index, bits, lists = _index(dtype), _bits(dtype), _complete(dtype)
  mask = torch.arange(NV, device=DEV) % 3 != 1
  sub = index.subset(mask)
  rows = torch.arange(NQ, device=DEV)
  ex = torch.stack([rows, 100 + rows % 40, torch.full_like(rows, -1)], 1)          # the query's own number, one of the tie
  allowed = mask.cpu().numpy()[None].repeat(NQ, 0)
  allowed[np.arange(NQ)[:, None], ex[:, :2].cpu().numpy()] = False
  want = _padded(bits, allowed)
  # positions of the UNRESTRICTED list: the cursor's item is outside the subset for about a third of the rows
  start = _mixed_starts(NQ)
  cursor = _cursor_at(lists, start)
  assert ((cursor[1] >= 0) & ~mask[cursor[1].clamp(min=0)]).sum() > 10
  for k in (10, 128):
    got = index.search(q, qw, k=k, subset=sub, exclude=ex, after=cursor)
    assert got[0].shape == (NQ, k) and _same(got, _by_definition(bits, cursor, k, allowed)), k
  few = index.subset(torch.tensor([3, 100, 101, 700], device=DEV))                 # fewer allowed items than k: 4 columns
  got = index.search(q, qw, k=10, subset=few, after=cursor)
  assert got[0].shape == (NQ, 4)
  only = np.zeros((NQ, NV), bool)
  only[:, [3, 100, 101, 700]] = True
  assert _same(got, _by_definition(bits, cursor, 4, only))
  # and pages of the restricted list, walked by its own last columns
  pages, after = [], None
  for _ in range(3):
    pages.append(index.search(q, qw, k=128, subset=sub, exclude=ex, after=after))
    after = (pages[-1][0][:, -1], pages[-1][1][:, -1])
  got = tuple(torch.cat(parts, 1) for parts in zip(*pages))
  assert _same(got, (want[0][:, :384], want[1][:, :384]))


def _norms(index):
  """A static norm and a dynamic one over a bank of the first 40 queries: those are hub rows, most others are not."""
  _, _, q, qw = _data()
  return index.hub_norm(q[:40], qw[:40], 20.0), index.hub_norm(q[:40], qw[:40], 20.0, dynamic=True)


@pytest.mark.parametrize('dtype', DTYPES[:2], ids=IDS[:2])
def test_the_normalised_pages_and_the_dynamic_rule(dtype):
  _, _, q, qw = _data()
  index, plain_bits = _index(dtype), _bits(dtype)
  static, dynamic = _norms(index)
  bits = _bits(dtype, static)
  assert not np.array_equal(bits, plain_bits)
  want = _padded(bits)
  start = _mixed_starts(NQ)
  for k in (10, 128):
    assert _same(index.search(q, qw, k=k, norm=static, after=_cursor_at(want, start)), _pages_from(want, start, k)), k
  # the dynamic rule: a query is normalised iff its plain top-1 -- of the WHOLE list, whatever the page -- is a hub
  use = dynamic.hubs[_complete(dtype)[1][:, 0]].cpu().numpy()
  assert use[:40].all() and 0 < use.sum() < NQ
  mixed = _padded(np.where(use[:, None], bits, plain_bits))
  pages, cursor = [], None
  for _ in range(4):
    pages.append(index.search(q, qw, k=10, norm=dynamic, after=cursor))
    cursor = (pages[-1][0][:, -1], pages[-1][1][:, -1])
  got = tuple(torch.cat(parts, 1) for parts in zip(*pages))
  assert _same(got, (mixed[0][:, :40], mixed[1][:, :40]))
  assert _same(pages[0], index.search(q, qw, k=10, norm=dynamic))
  # a cursor deep in the list, where a decision taken behind the cursor would look at another top-1
  assert _same(index.search(q, qw, k=128, norm=dynamic, after=_cursor_at(mixed, start)), _pages_from(mixed, start, 128))
  assert _same(index.search(q, qw, k=10, norm=dynamic, dynamic=False, after=_cursor_at(want, start)), _pages_from(want, start, 10))
  assert _same(index.search_deep(q, qw, 300, page=64, norm=dynamic), (mixed[0][:, :300], mixed[1][:, :300]))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_row_batches_do_not_change_a_page(dtype, monkeypatch):
  from mmt_amd import search
  _, _, q, qw = _data()
  index, lists = _index(dtype), _complete(dtype)
  start = _mixed_starts(NQ)
  cursor = _cursor_at(lists, start)
  ex = torch.arange(NQ, device=DEV)
  with monkeypatch.context() as patch:
    patch.setattr(search, '_BATCH_BYTES', 1)
    assert index._row_batches(NQ, 8 * 10) == [(0, 64), (64, 128), (128, 130)]
    assert _same(index.search(q, qw, k=10, after=cursor), _pages_from(lists, start, 10))
    batched = index.search(q, qw, k=128, exclude=ex, after=cursor)
  assert _same(batched, index.search(q, qw, k=128, exclude=ex, after=cursor))


def _three_shards_interleaved(g, gw, dtype):
  """Pieces of 37 items go to the emptiest shard in turn: every shard's table is increasing and none is contiguous."""
  from mmt_amd.search import ShardedVideoIndex
  index = ShardedVideoIndex.empty(900, M, D, [DEV] * 3, dtype=dtype)
  for lo in range(0, NV, 37):
    index.add(g[lo:lo + 37], gw[lo:lo + 37])
  assert index.shard_sizes == [259, 259, 259] and index.shards[1].ids[:3].tolist() == [37, 38, 39]
  return index


@pytest.mark.parametrize('build', [_three_shards_interleaved, _three_shards_one_empty], ids=['interleaved', 'one_empty'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_sharded_equals_the_single_index_bit_for_bit(dtype, build):
  g, gw, q, qw = _data()
  mono, shards, lists = _index(dtype), build(g, gw, dtype), _complete(dtype)
  start = _mixed_starts(NQ)
  cursor = _cursor_at(lists, start)
  tie = (torch.from_numpy(_bits(dtype)[:, 100].copy()).to(DEV), torch.full((NQ,), 300, device=DEV))
  for nq, k in ((130, 10), (130, 128), (65, 10), (1, 1)):
    for after in (cursor, tie):
      after = (after[0][:nq], after[1][:nq])
      got = shards.search(q[:nq], qw[:nq], k=k, after=after)
      assert got[0].device == DEV and _same(got, mono.search(q[:nq], qw[:nq], k=k, after=after)), (nq, k)
  assert _same(shards.search(q, qw, k=10, after=cursor), _pages_from(lists, start, 10))
  mask = torch.arange(NV, device=DEV) % 3 != 1
  ex = torch.stack([torch.arange(NQ, device=DEV), 100 + torch.arange(NQ, device=DEV) % 40], 1)
  assert _same(shards.search(q, qw, k=128, subset=shards.subset(mask), exclude=ex, after=cursor),
               mono.search(q, qw, k=128, subset=mono.subset(mask), exclude=ex, after=cursor))
  assert _same(shards.search_deep(q, qw, 300, page=64), (lists[0][:, :300], lists[1][:, :300]))
  if dtype != FP8:
    theirs, mine = shards.hub_norm(q[:40], qw[:40], 20.0, dynamic=True), mono.hub_norm(q[:40], qw[:40], 20.0, dynamic=True)
    for dyn in (None, False):
      assert _same(shards.search(q, qw, k=10, norm=theirs, dynamic=dyn, after=cursor),
                   mono.search(q, qw, k=10, norm=mine, dynamic=dyn, after=cursor)), dyn


@pytest.mark.parametrize('page', [7, 64, 128])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_search_deep_is_the_complete_list_cut_at_the_depth(dtype, page):
  _, _, q, qw = _data()
  index, lists = _index(dtype), _complete(dtype)
  for depth in (300, 1000):
    w = min(depth, NV)
    got = index.search_deep(q, qw, depth, page=page)
    assert got[0].shape == got[1].shape == (NQ, w) and _same(got, (lists[0][:, :w], lists[1][:, :w])), depth
  if page == 64:
    assert _same(index.search_deep(q, qw, 40), index.search(q, qw, k=40))            # one page: the search itself
    mask = torch.arange(NV, device=DEV) % 3 != 1
    ex = torch.arange(NQ, device=DEV)
    allowed = mask.cpu().numpy()[None].repeat(NQ, 0)
    allowed[np.arange(NQ), np.arange(NQ)] = False
    want = _padded(_bits(dtype), allowed)
    got = index.search_deep(q, qw, 1000, page=page, subset=index.subset(mask), exclude=ex)
    assert got[0].shape == (NQ, 518) and _same(got, (want[0][:, :518], want[1][:, :518]))   # 518 allowed; a row may end vacant
    assert (got[1][0, -1] == -1) and (got[1][1, -1] >= 0)                            # row 0 lost an allowed item; item 1 was not one


@pytest.mark.parametrize('sharded', [False, True], ids=['VideoIndex', 'ShardedVideoIndex'])
def test_argument_errors_leave_the_index_usable(sharded):
  from mmt_amd.search import ShardedVideoIndex
  g, gw, q, qw = _data()
  index = ShardedVideoIndex(g, gw, [DEV] * 2) if sharded else _index(torch.float32)
  lists = _complete(torch.float32)
  start = _mixed_starts(NQ)
  a_s, a_i = _cursor_at(lists, start)
  want = _pages_from(lists, start, 10)

  def broken(at, score=None, item=None):
    s, i = a_s.clone(), a_i.clone()
    if score is not None:
      s[at] = score
    if item is not None:
      i[at] = item
    return s, i
  for bad, text in (((a_s.double(), a_i), 'after must be None or a pair'), ((a_s, a_i.to(torch.int32)), 'after must be None or a pair'),
                    (a_s, 'after must be None or a pair'), ((a_s.cpu(), a_i.cpu()), 'after must be on the index device'),
                    ((a_s[:, None], a_i[:, None]), 'expected'), ((a_s[:129], a_i[:129]), '130 queries but after holds 129 rows'),
                    (broken(129, item=-1, score=0.5), '-1 in after goes with'), (broken(0, score=float('nan')), 'after must not be NaN'),
                    (broken(64, item=NV), r'items of after must lie in -1 \.\. 776, got -1 \.\. 777'),
                    (broken(64, item=-2), r'items of after must lie in -1 \.\. 776, got -2 \.\. ')):
    with pytest.raises(ValueError, match=text):
      index.search(q, qw, k=10, after=bad)
    assert _same(index.search(q, qw, k=10, after=(a_s, a_i)), want)
  with pytest.raises(ValueError, match=r'exclude must lie in -1 \.\. 776'):        # both value checks in one call
    index.search(q, qw, k=10, exclude=torch.full((NQ,), NV, device=DEV), after=(a_s, a_i))
  pool = index.pooling(2, 65)
  with pytest.raises(ValueError, match='after= does not combine with pooling= or item_pooling='):
    index.search(q, qw, k=10, pooling=pool, after=(a_s[:65], a_i[:65]))
  with pytest.raises(ValueError, match='after= does not combine with pooling= or item_pooling='):
    index.search(q, qw, k=10, item_pooling=object(), after=(a_s, a_i))            # refused before it is looked at
  for bad in (0, True, 2.5):
    with pytest.raises(ValueError, match='depth must be an int >= 1'):
      index.search_deep(q, qw, bad)
  for bad in (0, 129):
    with pytest.raises(ValueError, match='page must be an int in'):
      index.search_deep(q, qw, 300, page=bad)
  s, i = index.search(q[:0], qw[:0], k=10, after=(a_s[:0], a_i[:0]))               # no queries: empty lists
  assert s.shape == i.shape == (0, 10)
  s, i = index.search_deep(q[:0], qw[:0], 300, page=64)
  assert s.shape == i.shape == (0, 300) and s.dtype is torch.float32 and i.dtype is torch.int64
  assert _same(index.search(q, qw, k=10, after=(a_s, a_i)), want)
