"""Plain restatements of the token layouts that the front-end kernels write (assemble.hip, video_front.h), for
tests/test_video_front_gpu.py.  Nothing here reads device output or imports the native library; the video half is itself
checked against oracle.mmt_oracle.assemble_video_tokens by tests/test_video_front_ref_cpu.py.

Video tokens of one sample: slot 0 = CLS, then per expert e one AGG slot (1 + e * (T + 1)) followed by its T FEA slots.
Text tokens of one caption: the W words of the padded row."""
import numpy as np

# (B, M, T) of part 1 of the front-end tests and the code path each exists for
PLAN_SHAPES = [
    (1, 1, 1),     # smallest
    (3, 2, 5),     # ordinary
    (5, 7, 30),    # S = 218: one scan pass, M > 4
    (2, 3, 100),   # S = 304: two scan passes; T > 64: lane loops wrap
    (2, 16, 40),   # M = 16, S = 657: three scan passes, the wave-per-expert loop wraps four times
    (70, 2, 3),    # B > 64: the `before` count wraps its lane loop
]
PATTERNS = ['ones', 'zeros', 'holes', 'first_empty', 'last_empty', 'expert_empty']
MAX_POS = 32


def make_ind(B, M, T, pattern, seed=0):
  """features_ind of every expert: list of M float32 (B, T) arrays with values in {0, 1}."""
  rng = np.random.RandomState(1000 + seed)
  if pattern == 'ones':
    return [np.ones((B, T), np.float32) for _ in range(M)]
  if pattern == 'zeros':
    return [np.zeros((B, T), np.float32) for _ in range(M)]
  ind = [(rng.rand(B, T) < 0.6).astype(np.float32) for _ in range(M)]
  if pattern == 'holes':
    if T >= 3:
      for e in range(M):
        ind[e][e % B, :3] = (1, 0, 1)  # a hole in the middle of a sample
  elif pattern == 'first_empty':
    for e in range(M):
      ind[e][0] = 0
  elif pattern == 'last_empty':
    for e in range(M):
      ind[e][B - 1] = 0
  elif pattern == 'expert_empty':
    ind[M // 2][:] = 0
  else:
    raise ValueError(pattern)
  return ind


def make_times(B, M, T, max_pos=MAX_POS, seed=0):
  """features_t of every expert: random fractional times on both sides of [0, max_pos] with the edge values planted."""
  rng = np.random.RandomState(2000 + seed)
  special = [-4.5, 2.7, float(max_pos), max_pos + 0.5, max_pos + 7.0, 1e9, 0.999, -0.25, max_pos - 0.001]
  out = []
  for e in range(M):
    t = rng.uniform(-3.0, max_pos + 5.0, size=(B, T)).astype(np.float32)
    flat = t.reshape(-1)
    k = min(len(special), flat.size)
    rot = special[e % len(special):] + special[:e % len(special)]
    flat[rng.permutation(flat.size)[:k]] = np.asarray(rot[:k], np.float32)
    out.append(t)
  return out


def video_plan_reference(ind, t, type_idx, max_pos, pack):
  """Everything mmt_video_plan writes, from the documented layout.  ind / t: lists of M (B, T) float32 arrays.
  Keeps slot s of sample b if it is CLS, an AGG token, or a FEA token with ind != 0 (pack = 0: every slot, and every
  feature row counts as valid), in (b, s) order."""
  M = len(ind)
  B, T = ind[0].shape
  S = 1 + M * (T + 1)
  slot = np.full(B * S, -1, np.int32)
  rows = dict(row_index=[], type_ids=[], pos_ids=[], mask=[], src_row=[])
  agg_row = np.zeros(B * M, np.int32)
  counts = np.zeros(B, np.int32)
  xsrc = [[] for _ in range(M)]  # feature row b * T + t behind compact row B + i of expert e
  for b in range(B):
    for s in range(S):
      e, j = ((s - 1) // (T + 1), (s - 1) % (T + 1)) if s else (-1, -1)
      if s == 0:
        keep, typ, pos, mask, srow = True, 0, 0, 1.0, -1
      elif j == 0:
        keep, typ, pos, mask, srow = True, type_idx[e], 0, float(ind[e][b].max()), b
      else:
        valid = ind[e][b, j - 1] != 0
        keep = bool(valid) or not pack
        typ, mask = type_idx[e], float(ind[e][b, j - 1])
        pos = int(np.clip(np.float32(t[e][b, j - 1]), np.float32(0), np.float32(max_pos)))
        srow = B + len(xsrc[e])
        if keep:
          xsrc[e].append(b * T + j - 1)
      if not keep:
        continue
      r = len(rows['row_index'])
      slot[b * S + s] = r
      if s and j == 0:
        agg_row[b * M + e] = r
      counts[b] += 1
      for k, v in zip(('row_index', 'type_ids', 'pos_ids', 'mask', 'src_row'), (b * S + s, typ, pos, mask, srow)):
        rows[k].append(v)
  mask = np.asarray(rows['mask'], np.float32)
  return dict(B=B, M=M, T=T, S=S, counts=counts, cu_seqlens=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
              n_rows=int(counts.sum()), slot=slot, agg_row=agg_row,
              row_index=np.asarray(rows['row_index'], np.int32), type_ids=np.asarray(rows['type_ids'], np.int32),
              pos_ids=np.asarray(rows['pos_ids'], np.int32), mask=mask,
              mask_bias=(np.float32(1.0) - mask) * np.float32(-10000.0),
              src_row=np.asarray(rows['src_row'], np.int32),
              src_cnt=np.asarray([B + len(x) for x in xsrc], np.int32),
              xsrc=[np.asarray(x, np.int32) for x in xsrc])


def text_plan_reference(ids, types, pos, mask):
  """Everything mmt_text_plan writes.  (B, W) int64 arrays; types / pos may be None (0 / 0 .. W - 1).  A token is kept
  if its mask is non-zero, and token 0 of every caption always."""
  B, W = ids.shape
  keep = mask != 0
  keep[:, 0] = True
  flat = np.flatnonzero(keep.reshape(-1))
  counts = keep.sum(1).astype(np.int32)
  cu = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
  types = np.zeros_like(ids) if types is None else types
  pos = np.broadcast_to(np.arange(W), (B, W)) if pos is None else pos
  return dict(counts=counts, cu_seqlens=cu, n_rows=int(cu[-1]), row_index=flat.astype(np.int32),
              ids=ids.reshape(-1)[flat].astype(np.int32), types=types.reshape(-1)[flat].astype(np.int32),
              pos=pos.reshape(-1)[flat].astype(np.int32), cls_rows=cu[:-1].copy())
