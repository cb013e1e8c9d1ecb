"""Per-query attribute filters without a GPU (include/mmt_hip.h: the five `_where` entries): the numpy
restatement `tag_pass` against a plain Python loop over 64-bit ints, the checks of `where()`, and the C ABI -- additive to
the scans: the version and the descriptor stay, every entry keeps the gates of its unfiltered twin for the cells it
takes and refuses norm, sets, a null `tags` and a null `where` before the alignment check.  No call here launches
anything: every call is refused on the host (MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2), and a supported cell is recognised by
the alignment refusal that only an otherwise accepted call reaches."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = (1 << 64) - 1
BITS = (0, 31, 32, 63)     # a 32-bit truncation loses 32 and 63, a sign extension of bit 31 sets 32 .. 63

FP32, BF16, FP8 = 'fp32', 'bf16', 'fp8'
STORAGES = {FP32: (0, 4), BF16: (1, 8), FP8: (2, 16)}            # tag, the multiple d must be
# entry -> (the parts it takes, its own arguments between `where` and the stream: (name, kind) as in test_search_abi_cpu)
ENTRIES = {
    'mmt_search_topk_where': (('subset', 'exclude', 'after'), [('k', 'k'), ('ws', 'p'), ('scores', 'n'), ('index', 'p')]),
    'mmt_search_topk_stream_where': (('subset', 'exclude', 'after'),
                                     [('k', 'k'), ('ws', 'p'), ('scores', 'n'), ('index', 'p')]),
    'mmt_search_count_where': (('subset',), [('thr', 'p'), ('T', 'T'), ('ws', 'p'), ('greater', 'p'), ('equal', 'p')]),
    'mmt_search_range_count_where': (('subset',), [('thr', 'p'), ('ws', 'p'), ('row_counts', 'p')]),
    'mmt_search_range_fill_where': (('subset',), [('thr', 'p'), ('ws', 'p'), ('offsets', 'p'), ('indices', 'p'),
                                                  ('scores', 'p')]),
}
BAD = {'k': (0, -1, 129), 'T': (0, 33)}
GOOD = {'k': 1, 'T': 1}

_buf = (ctypes.c_char * 256)()
P = ctypes.addressof(_buf) + -ctypes.addressof(_buf) % 16        # 16-byte aligned, never dereferenced: every call is refused


def _signed(v):
  return v - (1 << 64) if v >= 1 << 63 else v


def _loop(tags, masks):
  """The definition, one pair at a time, on Python ints in 0 .. 2^64 - 1."""
  out = np.zeros((len(masks), len(tags)), bool)
  for q, (a, n, y) in enumerate(masks):
    for g, t in enumerate(tags):
      out[q, g] = (t & a) == a and (t & n) == 0 and (y == 0 or (t & y) != 0)
  return out


def _words():
  """Every subset of the four bits: 16 words that use bits 0, 31, 32 and 63."""
  return [sum(1 << b for b in some) for n in range(len(BITS) + 1) for some in itertools.combinations(BITS, n)]


def test_tag_pass_is_the_definition_on_64_bit_ints():
  from mmt_amd.search import tag_pass
  tags = _words() + [U64, U64 ^ (1 << 63), 1 << 62]
  masks = [(a, n, y) for a in (0, 1, 1 << 31, 1 << 32, 1 << 63, (1 << 63) | 1) for n in (0, 1 << 31, 1 << 63, 1 << 32)
           for y in (0, 1 << 63, (1 << 32) | (1 << 31), 1)]
  want = _loop(tags, masks)
  assert want.any() and not want.all()
  assert want[0].all()                                                 # three zero masks admit every item
  as_i64 = np.array([_signed(t) for t in tags], np.int64), np.array([[_signed(v) for v in m] for m in masks], np.int64)
  as_u64 = np.array(tags, np.uint64), np.array(masks, np.uint64)
  for t, m in (as_i64, as_u64, (torch.from_numpy(as_i64[0]), torch.from_numpy(as_i64[1]))):
    got = tag_pass(t, m)
    assert got.dtype == bool and got.shape == want.shape and (got == want).all()
  # what a 32-bit truncation or a sign extension would get wrong
  assert not tag_pass(np.array([1 << 31], np.uint64), np.array([[1 << 32, 0, 0]], np.uint64))[0, 0]
  assert not tag_pass(np.array([_signed(1 << 63)], np.int64), np.array([[0, 0, 1 << 32]], np.int64))[0, 0]
  assert tag_pass(np.array([_signed(1 << 63)], np.int64), np.array([[_signed(1 << 63), 1 << 32, 0]], np.int64))[0, 0]
  assert not tag_pass(np.array([-(1 << 31)], np.int64), np.array([[0, 1 << 40, 0]], np.int64))[0, 0]  # a true bit 40 bars
  with pytest.raises(ValueError, match='tag_pass'):
    tag_pass(np.zeros(3, np.int32), np.zeros((1, 3), np.int64))


def _tagging(n=5):
  from mmt_amd.search import IndexTagging
  return IndexTagging(torch.arange(n, dtype=torch.int64))


def test_where_broadcasts_ints_and_takes_rows():
  from mmt_amd.search import TagFilter
  tg = _tagging()
  assert (tg.num_items, tg.device) == (5, torch.device('cpu')) and tg.tags.dtype is torch.int64
  flt = tg.where()
  assert isinstance(flt, TagFilter) and flt.tagging is tg and flt.num_rows is None
  assert flt.masks.dtype is torch.int64 and flt.masks.is_contiguous() and flt.masks.tolist() == [[0, 0, 0]]
  assert flt._rows(4).shape == (4, 3) and flt._rows(4).is_contiguous() and not flt._rows(4).any()
  flt = tg.where(all_of=U64, none_of=1 << 63, any_of=(1 << 32) | 1)
  assert flt.masks.tolist() == [[-1, -(1 << 63), (1 << 32) | 1]]      # bit patterns: bit 63 is an ordinary bit
  rows = torch.tensor([1, -(1 << 63), 1 << 32], dtype=torch.int64)
  flt = tg.where(all_of=rows, any_of=1 << 31)
  assert flt.num_rows == 3 and flt.masks.shape == (3, 3) and flt.masks.is_contiguous()
  assert flt.masks.tolist() == [[1, 0, 1 << 31], [-(1 << 63), 0, 1 << 31], [1 << 32, 0, 1 << 31]]
  assert flt._rows(3) is flt.masks
  flt = tg.where(rows, rows, rows)
  assert flt.num_rows == 3 and (flt.masks == rows[:, None]).all()


def test_where_refusals():
  from mmt_amd.search import VideoIndex, _Index
  tg = _tagging()
  for bad in (1.0, True, None, 'x', [1]):
    with pytest.raises(ValueError, match='all_of must be an int or an int64 tensor'):
      tg.where(all_of=bad)
  for name in ('all_of', 'none_of', 'any_of'):
    for bad in (-1, 1 << 64):
      with pytest.raises(ValueError, match=r'%s must lie in 0 \.\. 2\^64 - 1' % name):
        tg.where(**{name: bad})
    with pytest.raises(ValueError, match='%s must be an int or an int64 tensor, got torch.int32' % name):
      tg.where(**{name: torch.zeros(3, dtype=torch.int32)})
    with pytest.raises(ValueError, match=r'%s \[NQ\] expected' % name):
      tg.where(**{name: torch.zeros(3, 1, dtype=torch.int64)})
    with pytest.raises(ValueError, match='%s must be on the index device' % name):
      tg.where(**{name: torch.zeros(3, dtype=torch.int64, device='meta')})
  with pytest.raises(ValueError, match='none_of holds 4 rows, the masks before it 3'):
    tg.where(torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64))

  # the checks of a call, on an index that holds nothing on a device: type, origin, age, rows, combinations
  index = VideoIndex.__new__(VideoIndex)
  index.num_items, index.device = 5, torch.device('cpu')
  index._where(tg.where(), 'search')
  with pytest.raises(ValueError, match='search: where must come from the where\\(\\) of a tagging, got Tensor'):
    index._where(torch.zeros(1, 3, dtype=torch.int64), 'search')
  with pytest.raises(ValueError, match='the tagging was built for 6 items, the index holds 5'):
    index._where(_tagging(6).where(), 'search')                       # another index's, or this one's before an `add`
  other = _tagging()
  other.device = torch.device('meta')
  with pytest.raises(ValueError, match='the tagging is on meta, the index on cpu'):
    index._where(other.where(), 'ranks')
  for name in ('norm', 'pooling', 'item_pooling'):
    with pytest.raises(ValueError, match='range_search: where= does not combine with %s=' % name):
      index._where(tg.where(), 'range_search', **{name: object()})
  _Index._where_rows(tg.where(), 'search', 7)                          # ints stand for any number of rows
  _Index._where_rows(tg.where(all_of=torch.zeros(7, dtype=torch.int64)), 'search', 7)
  with pytest.raises(ValueError, match='search: 8 query rows but the where= filter holds 7 rows'):
    _Index._where_rows(tg.where(all_of=torch.zeros(7, dtype=torch.int64)), 'search', 8)
  for who in ('search_groups', 'rescore', 'reverse_search'):
    with pytest.raises(ValueError, match='%s: where= is out of scope' % who):
      getattr(index, who)(*([None] * (3 if who != 'reverse_search' else 2)), where=tg.where())
  for who in ('neighbours', 'neighbour_range', 'duplicate_groups', 'query_lse', 'search_softmax'):
    args = {'neighbours': (), 'neighbour_range': (0.5,), 'duplicate_groups': (0.5,), 'query_lse': (None, None, 1.0),
            'search_softmax': (None, None)}[who]
    with pytest.raises(ValueError, match='%s: where= is out of scope' % who):
      getattr(index, who)(*args, where=tg.where())
  with pytest.raises(ValueError, match='tagging: tags must be an int64 tensor, got torch.int32'):
    index.tagging(torch.zeros(5, dtype=torch.int32))
  with pytest.raises(ValueError, match=r'tagging: tags of shape \(5,\) expected'):
    index.tagging(torch.zeros(6, dtype=torch.int64))
  with pytest.raises(ValueError, match='tagging: tags must be on the index device'):
    index.tagging(torch.zeros(5, dtype=torch.int64, device='meta'))
  mine = torch.arange(5, dtype=torch.int64)
  made = index.tagging(mine)
  mine += 1
  assert made.tags.tolist() == [0, 1, 2, 3, 4] and made.num_items == 5   # a copy of its own


def test_where_is_keyword_only_beside_the_pinned_parameter_lists():
  """The parameter lists that earlier tests pin stay what they are; where= is a keyword-only option carried by a wrapper
  (`_where_option`), refused by name where the call takes no filter (`_refuses_where`), and said in the docstrings."""
  import inspect
  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  assert list(inspect.signature(VideoIndex.search).parameters)[-1] == 'after'
  assert list(inspect.signature(VideoIndex.search_deep).parameters)[-1] == 'dynamic'
  assert list(inspect.signature(VideoIndex.search_refined).parameters)[-1] == 'exclude'
  assert list(inspect.signature(VideoIndex.rescore).parameters)[-1] == 'k'
  assert list(inspect.signature(VideoIndex.search_groups).parameters)[-1] == 'subset'
  for method in ('search', 'search_deep', 'search_refined'):
    assert getattr(ShardedVideoIndex, method) is getattr(VideoIndex, method)
    assert 'where' in getattr(VideoIndex, method).__doc__
    assert 'where' in inspect.signature(getattr(VideoIndex, method), follow_wrapped=False).parameters
    assert inspect.signature(getattr(VideoIndex, method), follow_wrapped=False).parameters['where'].kind is inspect.Parameter.KEYWORD_ONLY
  for cls, methods in ((VideoIndex, ('rank_counts', 'ranks', 'threshold_counts', 'range_search', 'reverse_search')),
                       (ShardedVideoIndex, ('rank_counts', 'ranks', 'range_search', 'reverse_search'))):
    for method in methods:                                             # no list of theirs is pinned: an ordinary parameter
      assert inspect.signature(getattr(cls, method)).parameters['where'].default is None
  index = VideoIndex.__new__(VideoIndex)
  index.num_items, index.device = 5, torch.device('cpu')
  flt = _tagging().where()
  host = torch.zeros(2, 1, 4), torch.zeros(2, 1)
  # the filter reaches the checks of the call: a filtered call is refused for what the unfiltered one is refused for ...
  for call in (lambda **kw: index.search(*host, **kw), lambda **kw: index.search_deep(*host, 3, **kw)):
    with pytest.raises(ValueError, match='CUDA tensor'):
      call()
    with pytest.raises(ValueError, match='CUDA tensor'):
      call(where=flt)
    with pytest.raises(ValueError, match='the tagging was built for 6 items'):    # ... and first for its own filter
      call(where=_tagging(6).where())
    with pytest.raises(ValueError, match='where= does not combine with norm='):
      call(where=flt, norm=object())
  with pytest.raises(TypeError):
    index.search(*host, 10, None, None, None, None, None, None, None, flt)   # not positional


def test_a_scan_carries_its_filter():
  from mmt_amd.search import _Scan
  flt = _tagging().where()
  scan = _Scan(where=flt)
  assert scan.where is flt and scan.plain().where is flt and scan.uncursored().where is flt and scan.at(None).where is flt
  assert scan.scored().where is None                                   # a target is scored whether or not it passes
  assert _Scan().where is None


def _descriptor(store, parts, **changes):
  """A descriptor every gate accepts for the cell: NQ = NV = M = 1, d = 16 (a multiple for every storage)."""
  from mmt_amd import _lib
  parts = frozenset(parts)
  f = dict(q=P, q_lo=None if store == FP32 else P, qw=P, g=P, gw=P, gscale=P if store == FP8 else None,
           subset=P if 'subset' in parts else None, exclude=P if 'exclude' in parts else None,
           after=P if 'after' in parts else None, lse=P if 'norm' in parts else None,
           set_weights=P if parts & {'qsets', 'isets'} else None, storage=STORAGES[store][0], NQ=1, NV=1, M=1, d=16,
           E=1 if 'exclude' in parts else 0, beta=1.0 if 'norm' in parts else 0.0,
           sets=1 if 'qsets' in parts else 2 if 'isets' in parts else 0, set_size=1 if parts & {'qsets', 'isets'} else 0, mode=0)
  f.update(changes)
  return _lib.MmtSearchScan(**f)


def _call(entry, desc, tags=P, where=P, **changes):
  from mmt_amd import _lib
  own = [changes.get(name, P if kind in 'pn' else GOOD[kind]) for name, kind in ENTRIES[entry][1]]
  return getattr(_lib.lib(), entry)(None if desc is None else ctypes.byref(desc), tags, where, *own, None)


def _cells(entry):
  taken = ENTRIES[entry][0]
  for storage in STORAGES:
    for n in range(len(taken) + 1):
      for parts in itertools.combinations(taken, n):
        yield storage, frozenset(parts)


def test_header_bindings_and_library_agree_on_the_five_entries():
  from mmt_amd import _lib
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read(), flags=re.S)
  handle = ctypes.CDLL(_lib.LIB_PATH)
  assert len(ENTRIES) == 5
  for entry, (_, own) in ENTRIES.items():
    params = [p.strip() for p in re.search(r'\bint %s\(([^;]*?)\);' % entry, src).group(1).replace('\n', ' ').split(',')]
    assert params[:3] == ['const MmtSearchScan* scan', 'const uint64_t* tags', 'const uint64_t* where'], entry
    assert params[-1] == 'void* stream', entry
    restype, args = _lib.SIGNATURES[entry]
    assert restype is ctypes.c_int and args[0] is ctypes.POINTER(_lib.MmtSearchScan), entry
    assert args[1] is ctypes.c_void_p and args[2] is ctypes.c_void_p and args[-1] is ctypes.c_void_p, entry
    assert [p.split()[-1].lstrip('*') for p in params[3:-1]] == [n for n, _ in own], entry
    for p, a, (_, kind) in zip(params[3:-1], args[3:-1], own):
      assert (a is ctypes.c_void_p) == ('*' in p) == (kind in 'pn'), (entry, p)
      assert (a is ctypes.c_int) == p.startswith('int '), (entry, p)
    # the unfiltered twin's arguments with the two behind the descriptor
    twin = _lib.SIGNATURES[entry[:-len('_where')]]
    assert (restype, args) == (twin[0], twin[1][:1] + [ctypes.c_void_p] * 2 + twin[1][1:]), entry
    assert hasattr(handle, entry)
  # additive: the version and the descriptor are what they were
  assert handle.mmt_abi_version() == 6
  assert ctypes.sizeof(_lib.MmtSearchScan) == 128 and len(_lib.MmtSearchScan._fields_) == 21
  assert 'sizeof(MmtSearchScan) == 128' in src


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_the_gate_table(entry):
  """A supported cell with misaligned query rows returns -2; norm, sets, a part the entry does not take, a null `tags` and
  a null `where` return -1 -- with the rows misaligned as well, so a gate that has gone missing shows as -2, never as a
  launch."""
  taken = ENTRIES[entry][0]
  assert _call(entry, None) == -1
  for tag in (3, -1):
    assert _call(entry, _descriptor(FP32, (), storage=tag, q=P + 8)) == -1
    assert _call(entry, _descriptor(FP32, (), sets=tag, q=P + 8)) == -1
  seen = 0
  for storage, parts in _cells(entry):
    who = (entry, storage, sorted(parts))
    bf16 = storage != FP32
    seen += 1
    for off in (4, 8):
      assert _call(entry, _descriptor(storage, parts, q=P + off)) == -2, who
    for field in ['g'] + (['q_lo'] if bf16 else []) + (['subset'] if 'subset' in parts else []):
      assert _call(entry, _descriptor(storage, parts, **{field: P + 8})) == -2, who + (field,)

    def arg(own=None, tags=P, where=P, **fields):
      return _call(entry, _descriptor(storage, parts, **dict(dict(q=P + 8), **fields)), tags, where, **(own or {}))
    assert arg(tags=None) == -1 and arg(where=None) == -1 and arg(tags=None, where=None) == -1, who
    for more in ('norm', 'qsets', 'isets') + tuple(p for p in ('exclude', 'after') if p not in taken):
      assert _call(entry, _descriptor(storage, parts | {more}, q=P + 8)) == -1, who + (more,)
      assert _call(entry, _descriptor(storage, parts | {more})) == -1, who + (more,)
    assert arg(lse=P) == -1 and arg(beta=1.0) == -1, who                # a norm given by half
    for field in ['q', 'qw', 'g', 'gw'] + (['q_lo'] if bf16 else []) + (['gscale'] if storage == FP8 else []):
      assert arg(**{field: None}) == -1, who + (field,)
    for field, value in (('NQ', 0), ('NV', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 16 + STORAGES[storage][1] // 2),
                         ('NQ', -1), ('NV', -1), ('d', -16)):
      assert arg(**{field: value}) == -1, who + (field, value)
    for name, kind in ENTRIES[entry][1]:
      if kind == 'p':
        assert arg({name: None}) == -1, who + (name,)
      if kind == 'n':
        assert arg({name: None}) == -2, who + (name,)                  # nullable: the call goes on to the alignment gate
      for bad in BAD.get(kind, ()):
        assert arg({name: bad}) == -1, who + (name, bad)
    if not bf16:
      assert arg(q_lo=P) == -1, who
    if storage != FP8:
      assert arg(gscale=P) == -1, who
    for field, value in (('set_weights', P), ('set_size', 1), ('mode', 1)):
      assert arg(**{field: value}) == -1, who + (field,)
    if 'exclude' in parts:                                             # behind the alignment of the rows: subset off instead
      for e in (-1, 33):
        assert _call(entry, _descriptor(storage, parts, E=e, subset=P + 8)) == -1, who + (e,)
      assert _call(entry, _descriptor(storage, parts, exclude=None, subset=P + 8)) == -1, who
  assert seen == 3 * 2 ** len(taken)
