"""The C ABI of the streaming top-k schedule (include/mmt_hip.h: mmt_search_topk_stream and its workspace function; DESIGN
9.21), additive to the nine scans: the version and the descriptor stay, and the entry keeps mmt_search_topk's gates for
the cells it takes -- every storage with subset, exclude and after -- and refuses norm and both kinds of sets.  No call here
launches anything: every call is refused on the host (MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2), and a supported cell is
recognised by the alignment refusal that only an otherwise accepted call reaches."""
import ctypes
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FP32, BF16, FP8 = 'fp32', 'bf16', 'fp8'
STORAGES = {FP32: (0, 4), BF16: (1, 8), FP8: (2, 16)}            # tag, the multiple d must be
TAKEN = ('subset', 'exclude', 'after')
REFUSED = ('norm', 'qsets', 'isets')

_buf = (ctypes.c_char * 256)()
P = ctypes.addressof(_buf) + -ctypes.addressof(_buf) % 16        # 16-byte aligned, never dereferenced: every call is refused


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


def _call(desc, k=1, ws=P, scores=P, index=P):
  from mmt_amd import _lib
  return _lib.lib().mmt_search_topk_stream(None if desc is None else ctypes.byref(desc), k, ws, scores, index, None)


def _cells():
  for storage in STORAGES:
    for n in range(len(TAKEN) + 1):
      for parts in itertools.combinations(TAKEN, n):
        yield storage, frozenset(parts)


def test_header_declares_and_bindings_bind_both_entries():
  from mmt_amd import _lib
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read(), flags=re.S)
  flat = ' '.join(src.split())
  assert 'int64_t mmt_topk_stream_workspace_keys(int NQ, int NV, int k);' in flat
  assert ('int mmt_search_topk_stream(const MmtSearchScan* scan, int k, uint64_t* ws, float* scores, int64_t* index, '
          'void* stream);') in flat
  assert _lib.SIGNATURES['mmt_topk_stream_workspace_keys'] == (ctypes.c_int64, [ctypes.c_int] * 3)
  assert _lib.SIGNATURES['mmt_search_topk_stream'] == _lib.SIGNATURES['mmt_search_topk']   # the same arguments
  handle = _lib.lib()
  assert hasattr(handle, 'mmt_search_topk_stream') and hasattr(handle, 'mmt_topk_stream_workspace_keys')
  # additive: the version and the descriptor are what they were
  assert handle.mmt_abi_version() == 6
  assert ctypes.sizeof(_lib.MmtSearchScan) == 128 and len(_lib.MmtSearchScan._fields_) == 21
  assert 'sizeof(MmtSearchScan) == 128' in src


def test_every_taken_cell_reaches_the_alignment_gate():
  seen = 0
  for storage, parts in _cells():
    assert _call(_descriptor(storage, parts, q=P + 4)) == -2, (storage, sorted(parts))
    assert _call(_descriptor(storage, parts, q=P + 8)) == -2, (storage, sorted(parts))
    seen += 1
  assert seen == 3 * 8


def test_norm_and_sets_are_refused_in_every_cell():
  for storage, parts in _cells():
    for more in REFUSED:
      if more != 'norm' and parts & {'exclude', 'after'}:
        continue   # a descriptor the common gate refuses anyway; below with the parts a set may carry
      for desc in (_descriptor(storage, parts | {more}), _descriptor(storage, parts | {more}, q=P + 8)):
        assert _call(desc) == -1, (storage, sorted(parts), more)
  for storage in STORAGES:   # and whatever else comes with them
    for parts in (('norm', 'qsets'), ('norm', 'isets'), ('exclude', 'qsets'), ('after', 'isets'), ('subset', 'exclude', 'qsets')):
      assert _call(_descriptor(storage, parts, q=P + 8)) == -1, (storage, parts)
    # a norm given by half: lse without beta, beta without lse
    assert _call(_descriptor(storage, (), lse=P, q=P + 8)) == -1
    assert _call(_descriptor(storage, (), beta=1.0, q=P + 8)) == -1


def test_gates_of_every_taken_cell():
  """One thing knocked out of a good call at a time, with the query rows misaligned as well (the exclusion bounds, gated
  behind that check, with the subset words instead): a gate that has gone missing shows as -2, never as a launch."""
  assert _call(None) == -1
  for tag in (3, -1):
    assert _call(_descriptor(FP32, (), storage=tag, q=P + 8)) == -1
    assert _call(_descriptor(FP32, (), sets=tag, q=P + 8)) == -1
  for storage, parts in _cells():
    who = (storage, sorted(parts))
    bf16 = storage != FP32

    def arg(own=None, **fields):
      return _call(_descriptor(storage, parts, **dict(dict(q=P + 8), **fields)), **(own or {}))
    for field in ['q', 'qw', 'g', 'gw'] + (['q_lo'] if bf16 else []) + (['gscale'] if storage == FP8 else []):
      assert arg(**{field: None}) == -1, who + (field,)
    for field, value in (('NQ', 0), ('NV', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 16 + STORAGES[storage][1] // 2),
                         ('NQ', -1), ('NV', -1), ('d', -16)):
      assert arg(**{field: value}) == -1, who + (field, value)
    if storage == FP8:
      assert arg(d=8) == -1, who
    if storage == BF16:
      assert arg(d=4) == -1, who
    for k in (0, -1, 129):
      assert arg({'k': k}) == -1, who + (k,)
    for name in ('ws', 'index'):
      assert arg({name: None}) == -1, who + (name,)
    assert arg({'scores': None}) == -2, who                       # nullable: the call goes on to the alignment gate
    if not bf16:
      assert arg(q_lo=P) == -1, who
    if storage != FP8:
      assert arg(gscale=P) == -1, who
    for field, value in (('set_weights', P), ('set_size', 1), ('mode', 1)):
      assert arg(**{field: value}) == -1, who + (field,)
    if 'exclude' in parts:
      for e in (-1, 33):
        assert _call(_descriptor(storage, parts, E=e, subset=P + 8)) == -1, who + (e,)
      assert _call(_descriptor(storage, parts, exclude=None, subset=P + 8)) == -1, who   # E = 1 without exclude
    else:
      assert _call(_descriptor(storage, parts | {'exclude'}, exclude=None, subset=P + 8)) == -1, who
    for field in ['q', 'g'] + (['q_lo'] if bf16 else []) + (['subset'] if 'subset' in parts else []):
      for off in (4, 8):
        assert _call(_descriptor(storage, parts, **{field: P + off})) == -2, who + (field, off)


def test_workspace_function():
  from mmt_amd import _lib
  keys = _lib.lib().mmt_topk_stream_workspace_keys
  for bad in ((0, 1, 1), (-1, 1, 1), (1, 0, 1), (1, -1, 1), (1, 1, 0), (1, 1, -1), (1, 1, 129)):
    assert keys(*bad) == -1, bad
  sizes = sorted(set([1, 2, 31, 32, 33, 127, 129, 511, 512, 513, 1000, 1024, 1025, 1536, 1537, 4096, 4097, 65536, 262143,
                      262144, 262145, 523264, 523265, 1 << 20, (1 << 21) + 1, 1 << 22, 5000000, (1 << 24) + 3]))
  for nq in (1, 2, 31, 32, 33, 64, 65, 1000, 4096):
    chunks = []
    for nv in sizes:
      per_k = {k: keys(nq, nv, k) for k in (1, 10, 128)}
      assert all(v > 0 and v % (nq * k) == 0 for k, v in per_k.items()), (nq, nv)
      n = {v // (nq * k) for k, v in per_k.items()}
      assert len(n) == 1, (nq, nv)                               # keys / (NQ * k) depends on (NQ, NV) only
      chunks.append(n.pop())
      assert 1 <= chunks[-1] <= -(-nv // 512), (nq, nv)          # a chunk is at least one 512-item sweep
    assert chunks == sorted(chunks), (nq, chunks)                # monotone in NV
  # one chunk up to 512 items, and densely monotone where the count first moves
  dense = [keys(1, nv, 1) for nv in range(1, 2200)]
  assert dense == sorted(dense) and dense[0] == dense[511] == 1 and dense[512] == 2 and dense[1024] == 3


def test_the_schedule_is_a_checked_property_of_both_index_classes():
  """No device: hollow indexes.  The property refuses what it does not know and keeps what it had; a streaming index
  refuses norm, dynamic and the poolings by name before it looks at anything else; the parameter lists of `search` and
  `search_refined` are what they were."""
  import inspect

  import pytest

  from mmt_amd.search import ShardedVideoIndex, VideoIndex
  for cls in (VideoIndex, ShardedVideoIndex):
    index = cls.__new__(cls)
    assert index.schedule is None
    for bad in ('streaming', 'Stream', '', 0, 1, True, b'stream', ['stream'], ('tile',)):
      with pytest.raises(ValueError, match="schedule must be None, 'tile' or 'stream'"):
        index.schedule = bad
      assert index.schedule is None
    for good in ('tile', 'stream', None, 'stream'):
      index.schedule = good
      assert index.schedule == good
    with pytest.raises(ValueError, match='schedule must be'):
      index.schedule = 'fast'
    assert index.schedule == 'stream'
    other = cls.__new__(cls)
    assert other.schedule is None                                  # a setting of one index, not of the class
    for name in ('norm', 'dynamic', 'pooling', 'item_pooling'):
      with pytest.raises(ValueError, match="search: the index's schedule 'stream' does not combine with %s=" % name):
        index.search(None, None, k=3, **{name: False if name == 'dynamic' else object()})
    assert 'schedule' not in inspect.signature(cls.search).parameters
    assert 'schedule' not in inspect.signature(cls.search_refined).parameters
    assert isinstance(inspect.getattr_static(cls, 'schedule'), property)


def test_the_gallery_size_is_bounded_so_that_item_numbers_stay_ints():
  """A sweep's last tile may reach up to 511 numbers past NV: NV above INT_MAX - 512 is refused by both entries."""
  from mmt_amd import _lib
  keys = _lib.lib().mmt_topk_stream_workspace_keys
  top = 2 ** 31 - 1 - 512
  assert keys(1, top, 1) == -(-top // 512 // 8) and keys(1, top + 1, 1) == -1 and keys(1, 2 ** 31 - 1, 1) == -1
  for storage in STORAGES:
    assert _call(_descriptor(storage, (), NV=top, q=P + 8)) == -2
    assert _call(_descriptor(storage, (), NV=top + 1, q=P + 8)) == -1
