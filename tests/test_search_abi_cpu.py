"""The C ABI of the gallery scans: nine entry points over one descriptor, MmtSearchScan (include/mmt_hip.h).

One table drives everything: SYMBOLS lists the 54 per-variant scan entry points the library exported before the
descriptor, each translated to (entry, storage, the parts it required, the parts it took when given).  The supported
(entry, storage, parts) cells are exactly those the table spans; every other cell of the cross product is refused.  No
call here launches anything: every call is refused on the host (MMT_ERR_ARG = -1, MMT_ERR_ALIGN = -2), and a supported
cell is recognised by the alignment refusal that only an otherwise accepted call reaches."""
import ctypes
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float('inf')

FP32, BF16, FP8 = 'fp32', 'bf16', 'fp8'
STORAGES = {FP32: (0, 4), BF16: (1, 8), FP8: (2, 16)}            # tag, the multiple d must be
PARTS = ('subset', 'exclude', 'after', 'norm', 'qsets', 'isets')  # qsets / isets: the two values of the sets tag
ME = ('subset', 'exclude')

# old symbol -> (entry, storage, required parts, parts taken when given)
SYMBOLS = {}
for tag, st in (('', FP32), ('_bf16', BF16), ('_fp8', FP8)):
  SYMBOLS['mmt_search_topk%s' % tag] = ('topk', st, (), ())
  SYMBOLS['mmt_search_topk%s_ex' % tag] = ('topk', st, (), ME)
  SYMBOLS['mmt_search_topk%s_after' % tag] = ('topk', st, ('after',), ME)
  SYMBOLS['mmt_search_rank%s' % tag] = ('rank', st, (), ())
  SYMBOLS['mmt_search_rank%s_ex' % tag] = ('rank', st, (), ('subset',))
  SYMBOLS['mmt_search_thresholds%s' % tag] = ('thresholds', st, (), ())
  SYMBOLS['mmt_search_count%s' % tag] = ('count', st, (), ('subset',))
  SYMBOLS['mmt_search_range_count%s' % tag] = ('range_count', st, (), ('subset',))
  SYMBOLS['mmt_search_range_fill%s' % tag] = ('range_fill', st, (), ('subset',))
  SYMBOLS['mmt_search_rescore%s' % tag] = ('rescore', st, (), ())
for tag, st in (('', FP32), ('_bf16', BF16)):
  SYMBOLS['mmt_search_topk%s_norm' % tag] = ('topk', st, ('norm',), ME)
  SYMBOLS['mmt_search_topk%s_norm_after' % tag] = ('topk', st, ('norm', 'after'), ME)
  SYMBOLS['mmt_search_topk%s_pooled' % tag] = ('topk', st, ('qsets',), ('subset',))
  SYMBOLS['mmt_search_topk%s_itemsets' % tag] = ('topk', st, ('isets',), ('subset',))
  SYMBOLS['mmt_search_topk_groups%s' % tag] = ('topk_groups', st, (), ('subset',))
  SYMBOLS['mmt_search_thresholds%s_norm' % tag] = ('thresholds', st, ('norm',), ())
  SYMBOLS['mmt_search_thresholds%s_pooled' % tag] = ('thresholds', st, ('qsets',), ())
  SYMBOLS['mmt_search_thresholds%s_itemsets' % tag] = ('thresholds', st, ('isets',), ())
  SYMBOLS['mmt_search_count%s_norm' % tag] = ('count', st, ('norm',), ('subset',))
  SYMBOLS['mmt_search_count%s_pooled' % tag] = ('count', st, ('qsets',), ('subset',))
  SYMBOLS['mmt_search_count%s_itemsets' % tag] = ('count', st, ('isets',), ('subset',))
  SYMBOLS['mmt_search_col_lse%s' % tag] = ('col_lse', st, (), ())

# entry -> its own arguments between the descriptor and the stream: (name, kind); kind 'p' a required pointer, 'n' a
# nullable one, 'a' a required pointer that must also be 16-byte aligned, 'k' / 'T' / 'C' / 'beta' a bounded value,
# 'i' any int
ENTRIES = {
    'topk': [('k', 'k'), ('ws', 'p'), ('scores', 'n'), ('index', 'p')],
    'topk_groups': [('k', 'k'), ('group_ids', 'p'), ('ws', 'p'), ('scores', 'p'), ('groups', 'p'), ('items', 'p')],
    'rank': [('targets', 'p'), ('T', 'T'), ('ws', 'p'), ('greater', 'p'), ('equal', 'p')],
    'thresholds': [('targets', 'p'), ('T', 'T'), ('thr', 'p')],
    'count': [('thr', 'p'), ('T', 'T'), ('ws', 'p'), ('greater', 'p'), ('equal', 'p')],
    'range_count': [('thr', 'p'), ('ws', 'p'), ('row_counts', 'p')],
    'range_fill': [('thr', 'p'), ('ws', 'p'), ('offsets', 'p'), ('indices', 'p'), ('scores', 'p')],
    'rescore': [('candidates', 'p'), ('C', 'C'), ('k', 'k'), ('ws', 'p'), ('scores', 'p'), ('index', 'p')],
    'col_lse': [('beta', 'beta'), ('ws', 'a'), ('state', 'p'), ('first', 'i'), ('lse', 'n')],
}
BAD = {'k': (0, -1, 129), 'T': (0, 33), 'C': (0, -1, 1025), 'beta': (0.0, -1.0, INF, float('nan'))}
GOOD = {'k': 1, 'T': 1, 'C': 1, 'beta': 1.0, 'i': 1}


def _supported():
  cells = set()
  for entry, storage, required, optional in SYMBOLS.values():
    for n in range(len(optional) + 1):
      for some in itertools.combinations(optional, n):
        cells.add((entry, storage, frozenset(required + some)))
  return cells


def _all_cells():
  options = PARTS[:4]
  for entry in ENTRIES:
    for storage in STORAGES:
      for n in range(len(options) + 1):
        for some in itertools.combinations(options, n):
          for sets in ((), ('qsets',), ('isets',)):
            yield entry, storage, frozenset(some + sets)


_buf = (ctypes.c_char * 256)()
P = ctypes.addressof(_buf) + -ctypes.addressof(_buf) % 16        # 16-byte aligned, never dereferenced: every call is refused


def _descriptor(store, parts, **changes):
  """A descriptor every gate accepts for the cell: NQ = NV = M = 1, d = 16 (a multiple for every storage)."""
  from mmt_amd import _lib
  f = dict(q=P, q_lo=None if store == FP32 else P, qw=P, g=P, gw=P, gscale=P if store == FP8 else None,
           subset=P if 'subset' in parts else None, exclude=P if 'exclude' in parts else None,
           after=P if 'after' in parts else None, lse=P if 'norm' in parts else None,
           set_weights=P if parts & {'qsets', 'isets'} else None, storage=STORAGES[store][0], NQ=1, NV=1, M=1, d=16,
           E=1 if 'exclude' in parts else 0, beta=1.0 if 'norm' in parts else 0.0,
           sets=1 if 'qsets' in parts else 2 if 'isets' in parts else 0, set_size=1 if parts & {'qsets', 'isets'} else 0, mode=0)
  f.update(changes)
  return _lib.MmtSearchScan(**f)


def _call(entry, desc, **changes):
  from mmt_amd import _lib
  fn = getattr(_lib.lib(), 'mmt_search_' + entry)
  own = [changes.get(name, P if kind in 'pna' else GOOD[kind]) for name, kind in ENTRIES[entry]]
  return fn(None if desc is None else ctypes.byref(desc), *own, None)


def test_the_supported_cells_are_the_parent_symbols():
  assert len(SYMBOLS) == 54
  per_entry = {}
  for entry, _, _, _ in SYMBOLS.values():
    per_entry[entry] = per_entry.get(entry, 0) + 1
  assert per_entry == {'topk': 17, 'topk_groups': 2, 'rank': 6, 'thresholds': 9, 'count': 9, 'range_count': 3,
                       'range_fill': 3, 'rescore': 3, 'col_lse': 2}
  assert set(per_entry) == set(ENTRIES)
  # what the table spans, restated as rules: fp8 without norm or sets; sets without norm, exclusions or cursor, one kind
  takes = {'topk': set(PARTS), 'topk_groups': {'subset'}, 'rank': {'subset'}, 'thresholds': {'norm', 'qsets', 'isets'},
           'count': {'subset', 'norm', 'qsets', 'isets'}, 'range_count': {'subset'}, 'range_fill': {'subset'},
           'rescore': set(), 'col_lse': set()}
  fp8 = {'topk', 'rank', 'thresholds', 'count', 'range_count', 'range_fill', 'rescore'}
  rules = set()
  for entry, storage, parts in _all_cells():
    sets = parts & {'qsets', 'isets'}
    if parts <= takes[entry] and (storage != FP8 or (entry in fp8 and not sets and 'norm' not in parts)) and \
        not (sets and parts & {'norm', 'exclude', 'after'}):
      rules.add((entry, storage, parts))
  assert rules == _supported()


def test_header_struct_and_bindings_agree():
  from mmt_amd import _lib
  src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mmt_hip.h')).read(), flags=re.S)
  body = re.search(r'typedef struct MmtSearchScan \{(.*?)\} MmtSearchScan;', src, flags=re.S).group(1)
  fields = [re.match(r'(.*?)(\w+)$', line.strip()).groups() for line in body.split(';') if line.strip()]
  assert len(fields) == 21
  assert [name for _, name in fields] == [name for name, _ in _lib.MmtSearchScan._fields_]
  for (ctype, name), (_, bound) in zip(fields, _lib.MmtSearchScan._fields_):
    assert ctypes.sizeof(bound) == (8 if '*' in ctype else 4), name
    assert (bound is ctypes.c_float) == (ctype.strip() == 'float'), name
  widths = [ctypes.sizeof(bound) for _, bound in _lib.MmtSearchScan._fields_]
  assert widths == sorted(widths, reverse=True)                  # pointers first: no padding anywhere
  assert ctypes.sizeof(_lib.MmtSearchScan) == sum(widths) == 128
  assert 'sizeof(MmtSearchScan) == 128' in src
  assert (_lib.SEARCH_FP32, _lib.SEARCH_BF16, _lib.SEARCH_FP8) == tuple(
      int(re.search(r'#define MMT_SEARCH_%s (\d+)' % n, src).group(1)) for n in ('FP32', 'BF16', 'FP8'))
  assert (_lib.SEARCH_SETS_NONE, _lib.SEARCH_SETS_QUERY, _lib.SEARCH_SETS_ITEM) == tuple(
      int(re.search(r'#define MMT_SEARCH_SETS_%s (\d+)' % n, src).group(1)) for n in ('NONE', 'QUERY', 'ITEM'))
  handle = ctypes.CDLL(_lib.LIB_PATH)
  for entry, own in ENTRIES.items():
    name = 'mmt_search_' + entry
    params = [p.strip() for p in re.search(r'\bint %s\(([^;]*?)\);' % name, src).group(1).replace('\n', ' ').split(',')]
    restype, args = _lib.SIGNATURES[name]
    assert restype is ctypes.c_int and params[0] == 'const MmtSearchScan* scan' and params[-1] == 'void* stream', name
    assert args[0] is ctypes.POINTER(_lib.MmtSearchScan) and args[-1] is ctypes.c_void_p, name
    assert [p.split()[-1].lstrip('*') for p in params[1:-1]] == [n for n, _ in own], name
    for p, a, (_, kind) in zip(params[1:-1], args[1:-1], own):
      assert (a is ctypes.c_void_p) == ('*' in p) == (kind in 'pna'), (name, p)
      assert (a is ctypes.c_float) == p.startswith('float ') == (kind == 'beta'), (name, p)
      assert (a is ctypes.c_int) == p.startswith('int '), (name, p)
    assert hasattr(handle, name)
  for old in SYMBOLS:                                            # none of the per-variant names is left
    if old not in ['mmt_search_' + e for e in ENTRIES]:
      assert not re.search(r'\b%s\(' % old, src) and old not in _lib.SIGNATURES and not hasattr(handle, old), old
  assert handle.mmt_abi_version() == 6


def test_every_unsupported_cell_is_refused_and_every_supported_one_is_reached():
  supported = _supported()
  seen = 0
  for entry, storage, parts in _all_cells():
    # with the query rows off a 16-byte boundary an accepted call stops at the alignment gate, a refused one before it
    for off in (4, 8):
      rc = _call(entry, _descriptor(storage, parts, q=P + off))
      assert rc == (-2 if (entry, storage, parts) in supported else -1), (entry, storage, sorted(parts), rc)
    if (entry, storage, parts) not in supported:
      assert _call(entry, _descriptor(storage, parts)) == -1, (entry, storage, sorted(parts))
      seen += 1
  assert seen == 9 * 3 * 16 * 3 - len(supported)
  for entry in ENTRIES:
    assert _call(entry, None) == -1                              # a null descriptor
    for field, tag in (('storage', 3), ('storage', -1), ('sets', 3), ('sets', -1)):
      assert _call(entry, _descriptor(FP32, frozenset(), **{field: tag})) == -1, (entry, field, tag)


def test_gates_of_every_supported_cell():
  """One thing knocked out of a good call at a time.  A knock-out that returns MMT_ERR_ARG is made with the query rows
  misaligned as well (the exclusion bounds, gated behind that check, with the subset words instead), so a gate that has
  gone missing shows as -2, never as a launch."""
  for entry in ENTRIES:
    for _, storage, parts in sorted((c for c in _supported() if c[0] == entry), key=lambda c: (c[1], sorted(c[2]))):
      bf16 = storage != FP32
      who = (entry, storage, sorted(parts))

      def arg(own=None, **fields):
        return _call(entry, _descriptor(storage, parts, **dict(dict(q=P + 8), **fields)), **(own or {}))
      required = ['q', 'qw', 'g', 'gw'] + (['q_lo'] if bf16 else []) + (['gscale'] if storage == FP8 else []) + \
          (['set_weights'] if parts & {'qsets', 'isets'} else [])
      for field in required:
        assert arg(**{field: None}) == -1, who + (field,)
      for field, value in (('NQ', 0), ('NV', 0), ('M', 0), ('M', 17), ('d', 0), ('d', 16 + STORAGES[storage][1] // 2),
                           ('NQ', -1), ('NV', -1), ('d', -16)):
        assert arg(**{field: value}) == -1, who + (field, value)
      if storage == FP8:
        assert arg(d=8) == -1, who                                   # a bf16 width, not an fp8 one
      if storage == BF16:
        assert arg(d=4) == -1, who                                   # an fp32 width
      for name, kind in ENTRIES[entry]:
        if kind in 'pa':
          assert arg({name: None}) == -1, who + (name,)
        for bad in BAD.get(kind, ()):
          assert arg({name: bad}) == -1, who + (name, bad)
      # never ignored: a field whose part is absent
      if not bf16:
        assert arg(q_lo=P) == -1, who
      if storage != FP8:
        assert arg(gscale=P) == -1, who
      if not parts & {'qsets', 'isets'}:
        for field, value in (('set_weights', P), ('set_size', 1), ('mode', 1)):
          assert arg(**{field: value}) == -1, who + (field,)
      if 'norm' in parts:
        for beta in BAD['beta']:
          assert arg(beta=beta) == -1, who + (beta,)
        assert arg(lse=None) == -1, who                               # a missing lse
      if 'exclude' in parts:                                          # behind the alignment of the rows: subset off instead
        for e in (-1, 33):
          assert _call(entry, _descriptor(storage, parts, E=e, subset=P + 8)) == -1, who + (e,)
        assert _call(entry, _descriptor(storage, parts, exclude=None, subset=P + 8)) == -1, who   # E = 1 without exclude
      elif entry == 'topk' and not parts & {'qsets', 'isets'}:
        assert _call(entry, _descriptor(storage, parts | {'exclude'}, exclude=None, subset=P + 8)) == -1, who
      if 'qsets' in parts:
        for size, nq in ((0, 1), (-1, 1), (65, 65), (2, 1), (2, 3)):  # out of range; NQ not a whole number of sets
          assert arg(set_size=size, NQ=nq) == -1, who + (size, nq)
      if 'isets' in parts:
        for size, nv in ((0, 1), (-1, 1), (129, 129), (2, 1), (2, 3)):
          assert arg(set_size=size, NV=nv) == -1, who + (size, nv)
      if parts & {'qsets', 'isets'}:
        for mode in (2, -1):
          assert arg(mode=mode) == -1, who + (mode,)
      # alignment: the gates passed, each of the four alone 4 or 8 bytes off
      for field in ['q', 'g'] + (['q_lo'] if bf16 else []) + (['subset'] if 'subset' in parts else []):
        for off in (4, 8):
          assert _call(entry, _descriptor(storage, parts, **{field: P + off})) == -2, who + (field, off)
      for name, kind in ENTRIES[entry]:
        if kind == 'a':
          assert _call(entry, _descriptor(storage, parts), **{name: P + 8}) == -2, who + (name,)
