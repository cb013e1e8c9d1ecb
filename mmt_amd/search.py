"""Text-to-video search over a gallery held on the MI355X: the k best videos per query without the N_query x N_video
similarity matrix.

    index = VideoIndex(vid_embds, vid_weights)          # (NV, M, d), (NV, M) CUDA tensors; folded once
    scores, indices = index.search(text_embds, text_weights, k=10)

The score is the 'indep' similarity of model/model.py:789-837 (the matrix `metric.eval_similarity` builds):
    score(q, g) = sum_m qw[q][m] gw[g][m] <Q_m[q], G_m[g]> / sum_m qw[q][m] gw[g][m]     (0 -> 1e-5)
It is symmetric, so video-to-text search is an index of captions queried with videos.  Each query gets min(k, NV)
(score, index) pairs, best first, equal scores by ascending gallery index.  One launch scores 64-query x 4096-video
blocks on the matrix cores and keeps a running top-k per query; a second merges the chunk lists (mmt_search_topk).
Results are bit-reproducible.  Every scan goes to one of nine C entry points with one descriptor, MmtSearchScan
(include/mmt_hip.h; built per row batch by VideoIndex._describe): the storage, the operands and whatever of subset,
exclusions, cursor, norm and sets the call has (a tenth entry over the same descriptor, mmt_search_col_topk, serves the
ninth question at the end).  Below, `mmt_search_topk [lse, after]` stands for "that entry with those
parts of the descriptor set".

    index = VideoIndex(vid_embds, vid_weights, dtype=torch.bfloat16)    # half the bytes per item (d % 8 == 0)
    index = VideoIndex.empty(capacity, M, d, device, dtype=...)         # preallocated, filled in pieces:
    first, last = index.add(chunk_embds, chunk_weights)                 # items first .. last - 1
    index.num_items, index.capacity, index.dtype, index.nbytes

A bfloat16 index stores bf16(gw (.) G), the fp32 fold rounded once to nearest-even; the weights stay fp32 and the queries
are NOT rounded to 8 bits: score(q, g) = <fold_fp32(Q, qw)[q], dequant(stored[g])> / sum_m qw gw, computed on the bf16
matrix cores with the query split into hi = bf16(qf) and lo = bf16(qf - hi) (mmt_search_topk [bf16]; within 1e-5 of the
fp64 value of that definition).  Against the float32 index a score moves by at most
2^-8 * sum_m qw gw <|Q_m|, |G_m|> / sum_m qw gw, i.e. 2^-8 for unit-norm rows.

    index = VideoIndex(vid_embds, vid_weights, dtype=torch.float8_e4m3fn)   # a quarter of the bytes per item (d % 16 == 0)
    index.folded, index.scales, index.weights     # float8_e4m3fn [capacity, M*d], float32 [capacity], float32 [capacity, M]

A float8_e4m3fn index stores, with f = fold_fp32(G, gw)[g] (the row the float32 index keeps), one power of two per item and
the row divided by it, rounded once: scale[g] = 2^e, the smallest power of two with max_k |f[k]| / 2^e <= 448 (e clamped to
-120 .. 120; an all-zero row has scale 1), and stored[g][k] = e4m3fn_rne(f[k] / scale[g]) -- the division is exact, the cast
is round-to-nearest-even with e4m3's subnormals and never saturates.  The scale depends on the item alone, so the stored
bytes do not depend on how `add` was chunked or which shard holds the item.  nbytes = capacity * (M*d + 4*M + 4).  The
values are taken to be finite and `add` does not check them: a NaN or Inf spoils the scale and the row of its own item,
whose scores then mean nothing, and no other item.  As for bfloat16 only the storage is lossy and the score is defined on
the stored value:
    score(q, g) = fl(fl(acc * scale[g]) / den),   acc = <fold_fp32(Q, qw)[q], dequant(stored[g])>,   den = sum_m qw gw
(0 -> 1e-5), acc computed as on a bfloat16 index -- every e4m3 value is a bf16 value, so the gallery is widened exactly on
its way to the bf16 matrix cores and the query is the same hi / lo pair (mmt_search_topk [fp8]; within 1e-5 of the fp64 value
of that definition); the scale being a power of two, where it is multiplied in cannot change the bits.  Against the float32
index only the gallery rounding differs:
    |score_fp8 - score_fp32| <= (2^-4 * <|qf|, |f|> + 2^-10 * scale[g] * sum_k |qf[k]|) / |den|  + 1e-5
-- e4m3's unit roundoff for normal values, and the subnormal range below 2^-6 * scale[g].  `search` (plain, subset=,
exclude=), `rank_counts`, `ranks`, `target_scores`, `threshold_counts` and `range_search` work on it, on both index classes,
with the same score bits on every path.  That is the coarse stage of a two-stage search: search(k=128) on the
float8_e4m3fn index, then `rescore` of the shortlist on a float32 or bfloat16 index of the same items -- `search_refined`
below is the two in one call.  Not yet: `hub_norm` / norm=, `search_groups`, pooling= and item_pooling= raise ValueError
naming the dtype before anything is scored.

    greater, equal = index.rank_counts(embds, weights, targets)   # int32, shape of targets ([NQ] or [NQ, T], int64)
    ranks = index.ranks(embds, weights, targets)                  # float64: greater + (equal - 1) / 2

The other half of evaluation (R@k, MedR, MeanR: model/metric.py:90-121, 153-243) needs the exact rank of each query's
ground truth wherever it falls: for every target item, how many of the index's items score above it and how many score
equal to it -- the same scan with a counter per (query, target) in place of the top-k list (mmt_search_rank), so again
no N_query x N_video matrix.  The target's own score is taken from the same scoring tile, bit for bit, so it always
counts itself (equal >= 1) and `ranks` is the reference's tie-averaged 0-based rank; a target of -1 means "none" and
gives 0 / 0 and rank +inf.  metric.retrieval_metrics_indexed builds the t2v / v2t metrics on it.

    sub = index.subset(items)            # items: bool [num_items] or int64 ids (any order, duplicates allowed)
    sub.count, sub.num_items, sub.words  # allowed items; the num_items it was built for; packed uint32 bitmap
    scores, indices = index.search(q, qw, k=10, subset=sub, exclude=ex)
    greater, equal = index.rank_counts(q, qw, targets, subset=sub)
    ranks = index.ranks(q, qw, targets, subset=sub)

One stored corpus answers for any subset of its items -- a test cut, the real captions of a padded set -- without a
gathered copy: the subset is packed once into a bitmap (bit i & 31 of word i >> 5 is item i; mmt_search_subset_pack) and
reused across calls; the scan skips every 128-item tile that holds no allowed item and otherwise only declines to select
(or count) the items whose bit is clear (mmt_search_topk [subset, exclude], mmt_search_rank [subset]).  Indices stay the original item
numbers and a returned score has the bits plain `search` gives that item.  `exclude` ([NQ] or [NQ, E <= 32] int64, -1 =
none) bars items per query -- "the k best videos for this caption, not counting its own" -- and a query left with fewer
than k' candidates gets (-inf, -1) in the remaining slots.  subset=None and exclude=None take the unmasked calls.

    thr = index.target_scores(q, qw, targets)                    # float32, NaN for -1: score(q, target), the scan's bits
    greater, equal = index.threshold_counts(q, qw, thr, subset=None)

The two halves of `rank_counts` on their own (mmt_search_thresholds, mmt_search_count): what lets a gallery be cut up.

    index = ShardedVideoIndex(vid_embds, vid_weights, devices=['cuda:0', 'cuda:1', ...], dtype=...)   # or .empty + add
    index.search(...), index.rank_counts(...), index.ranks(...), index.subset(...)    # as VideoIndex, on devices[0]
    index.num_items, index.capacity, index.dtype, index.nbytes, index.devices, index.shard_sizes

One gallery held as one VideoIndex per entry of `devices` (up to 32; a device may repeat), for a corpus beyond one card's
memory or a scan at the rate of several cards.  Item numbers are global insertion order and every result is bit-identical
to that of one VideoIndex over the same items: a score does not depend on where its item is stored, the shards' lists are
merged on the device under the global tie rule (mmt_search_merge_lists), and a target is scored on the shard that holds
it and counted on all of them.

    norm = index.hub_norm(bank_embds, bank_weights, beta=20.0)             # HubNorm: .lse [num_items], .beta, .bank_size
    scores, indices = index.search(q, qw, k=10, norm=norm)                 # also with subset= and exclude=
    ranks = index.ranks(q, qw, targets, norm=norm)                         # rank_counts, target_scores, threshold_counts too
    norm = index.hub_norm(bank_embds, bank_weights, 20.0, dynamic=True)    # + .hubs: the plain top-1 items of the bank

Querybank hubness normalisation (inverted softmax, the static half of QB-Norm: Bogolin et al., CVPR 2022): a video that is
every query's nearest neighbour stops crowding out the right answers once each item is re-scored by how strongly a bank of
queries already pulls on it.  In fp32, with score the plain value above:
    lse[g] = log sum_b exp(fl(beta * score(b, g)))       over the bank, blockwise (mmt_search_col_lse)
    score'(q, g) = fl(fl(beta * score(q, g)) - lse[g])   a rounded multiply, then a rounded subtract
score' is the log of the inverted-softmax probability; with norm= the calls rank by it and return it, and norm=None takes
exactly the plain calls.  The bank streams through a scan of its own in batches of whole 64-row blocks -- no bank x
gallery matrix -- and lse[g] depends on item g, the bank in its row order and beta only: not on num_items, the item's
position, the batching or the shard, so ShardedVideoIndex.hub_norm (one HubNorm per shard, .lse and .hubs in global order
on the primary) gives bit-identical results.  A norm with .hubs applies QB-Norm's dynamic rule: a query is normalised only
if its plain top-1 among its candidates (after subset / exclude) is a hub, else it keeps its plain result; dynamic=False on
the call normalises every query.  Like a subset, a norm is refused after a further `add`.

    res = index.range_search(q, qw, threshold, subset=None, order='index', max_hits=1 << 27)   # RangeResult, a CSR:
    res.offsets, res.indices, res.scores, res.counts     # int64 [NQ + 1], int64 [total], float32 [total], int64 [NQ]

The third question, beside "the k best" and "how many beat this one": WHICH items score at least threshold[q] (a float, or
float32 [NQ]), however many -- near-duplicate joins of a gallery against itself, every caption that matches a video, all
negatives inside a margin, any list deeper than MAX_K.  Query q's hits are positions offsets[q] .. offsets[q + 1] - 1, by
ascending item (order='index') or in `search`'s order (order='score'); a score has the bits `search` gives the pair.  Two
scans with the hit counts summed in between (mmt_search_range_count, mmt_search_range_fill): every hit has a slot of its
own before it is written, so there are no atomics and the result is bit-reproducible; the total is known -- and held
against max_hits -- before anything of its size is allocated.  ShardedVideoIndex.range_search is bit-identical.

    grp = index.grouping(group_ids)      # IndexGrouping, built once like a subset: int64 [num_items], any labelling
    grp.ids, grp.num_groups, grp.num_items, grp.device
    scores, groups, items = index.search_groups(q, qw, grp, k=10, subset=None)      # each [NQ, min(k, num_groups)]

The fourth question: the k best VIDEOS of a gallery that holds clips (windows of a long video, segments, feature crops) or
of a caption index with several captions per video, each video reported once, with its best item -- "grouping search" /
"search groups" / field collapsing of the serving engines.  A group's representative is its member with the largest key
under `search`'s order (score descending, -0 tied with +0, equal scores by ascending item); groups are ranked by their
representatives; slot j holds the j-th best group, its representative's item number and that item's score, with the bits
`search` gives the pair.  With a subset a representative is the group's best allowed member and a group without one does not
appear: the slots left over hold (-inf, -1, -1).  It is not `search` plus a host-side de-duplication -- one video's clips
would push other videos' best clips out of a list before anybody could remove them: the running top-k of the scan keeps the
best k distinct groups, and the chunk and shard merges de-duplicate again (mmt_search_topk_groups,
mmt_search_merge_group_lists).  ShardedVideoIndex.search_groups is bit-identical; a group may have members on several shards.

    pool = index.pooling(set_size, num_sets, row_weights=None, mode='mean')     # QueryPooling, built once like a subset
    pool.set_size, pool.num_sets, pool.num_rows, pool.mode, pool.weights, pool.device
    scores, indices = index.search(q, qw, k=10, pooling=pool, subset=None)      # [num_sets, k']: one row per SET
    greater, equal = index.rank_counts(q, qw, targets, pooling=pool)            # targets [num_sets] or [num_sets, T]
    index.ranks(...), index.target_scores(...), index.threshold_counts(...)     # likewise

The fifth question: the queries are SETS of rows with one answer per set -- the captions of a video (the reference's
merge_caption_similiarities = 'avg', model/model.py:826-831: the mean of the captions' similarities), a query video cut into
clips (max over the clips), a caption and its paraphrases (mean), "any of these captions" (max).  The score is not linear in
the query -- its denominator sum_m qw[q][m] gw[g][m] depends on the pair -- so the rows cannot be averaged before the scan,
and per-row top-k lists cannot be merged exactly (a set's best item need not be in any member's list): the pooling happens
on the score tile, inside the kernel (mmt_search_topk [query sets], mmt_search_thresholds [query sets], mmt_search_count [query sets]).  The
queries are num_sets * set_size rows (either layout of `search`; the text layout (B, M, C, d) / (B, C, M) is sets of C
already), set s is rows s * set_size .. s * set_size + set_size - 1, 1 <= set_size <= MAX_SET = 64.  Every row has a weight
rw[r] (float32, finite; default float32(1 / set_size)); a row with rw[r] == 0 takes no part at all -- a padded caption --
and every set has a row that does.  With s_r = score(r, g), the bits the plain scan gives the pair, and r0 < r1 < ... the
participating rows of the set:
    mode='mean': v = fl(rw[r0] * s_r0), then v = fl(v + fl(rw[ri] * s_ri))    a rounded multiply, then a rounded add:
                                                                               never an fma, never reassociated
    mode='max' : v = s_r0, then v = s_ri where s_ri > v                        a plain compare, the first of equals stays;
                                                                               the weights act as a mask only
v depends on the set's rows, their weights and the item -- not on the launch geometry, the set's place in its block or the
shard that holds the item.  Ranking, ties and k' are `search`'s; a returned score has -0 as +0, `target_scores` returns the
pooled bits as they are, and a target counts itself.  A pooling does not describe the stored items: it stays valid after
`add`.  ShardedVideoIndex has the same surface: every shard sees all the query rows, so results are bit-identical to one
VideoIndex.  Out of scope: pooling= does not combine with exclude= or norm=, and `search_groups` and `range_search` take no
pooling.

    ip = index.item_pooling(set_size, item_weights=None, mode='mean')           # ItemPooling, built once like a subset
    ip.set_size, ip.num_sets, ip.num_items, ip.mode, ip.weights, ip.device
    scores, sets = index.search(q, qw, k=10, item_pooling=ip, subset=ip.subset(allowed_sets))   # [NQ, k']: SET numbers
    index.rank_counts(...), index.ranks(...), index.target_scores(...), index.threshold_counts(...)   # likewise

The sixth question, the fifth along the other axis: the STORED items are sets with one answer per set -- an index of
captions, C per video, queried with a video for "the k videos whose captions match best on average" (video-to-text in the
reference's 'avg' mode), a clip gallery ranked by the mean, not the best, of each video's clips.  `search_groups` collapses
a gallery by its best member; it cannot give a mean and gives no ranks.  The denominator of the score depends on the pair,
so the C items of a set cannot be averaged into one when the index is built, and per-item top-k lists cannot be merged into
set means: the pooling happens on the score tile (mmt_search_topk [item sets], mmt_search_thresholds [item sets],
mmt_search_count [item sets]).  The stored items are num_items / set_size sets, set t is items t * set_size .. t * set_size +
set_size - 1, 1 <= set_size <= MAX_ITEM_SET = 128 (one 128-column tile holds whole sets), num_items % set_size == 0.
Every item has a weight iw[g] (float32, finite; default float32(1 / set_size)); an item with iw[g] == 0 takes no part and
every set has an item that does.  With s_g = score(q, g), the bits the plain scan gives the pair, and g0 < g1 < ... the
participating items of the set in item order, the value v is `pooling`'s: 'mean' a rounded multiply, then a rounded add,
never an fma, never reassociated; 'max' a plain compare, the first of equals stays, the weights a mask.  v depends on the
query row, the set's items and their weights -- not on the launch geometry, the set's place in its tile, the chunking or
the shard.  Indices, targets (-1 .. num_sets - 1), subset= (from ip.subset: an IndexSubset over set numbers) and k' are in
set numbers; ranking and ties are `search`'s; a returned score has -0 as +0, `target_scores` returns the pooled bits as
they are, and a target counts itself; a target set outside the subset is still pooled and does not count itself.  An item
pooling describes the num_items of its moment: after a further `add` it is refused.  item_pooling= does not combine with
pooling=, exclude= or norm=, and `search_groups` and `range_search` do not take it.  ShardedVideoIndex.item_pooling is
accepted when every set is stored whole on one shard, in order, from a local item number that is a multiple of set_size
(`.empty` with a per-shard capacity that is a multiple of set_size, then `add` in pieces of whole sets that fit one shard);
each shard pools its own sets and the lists are merged through local-set -> global-set tables, bit-identical to one
VideoIndex.  metric.retrieval_metrics_indexed(caption_mode='avg') builds the reference's 'avg' evaluation on `pooling`
(text-to-video) and `item_pooling` (video-to-text).

    scores, indices = index.rescore(q, qw, candidates, k=None)        # candidates int64 [NQ, C <= MAX_C = 1024], -1 = none
    scores, indices = fine.search_refined(q, qw, coarse, k=10, shortlist=MAX_K, subset=None, exclude=None)

The seventh question: the k best among THESE items, per query -- the second stage of a two-stage search, whose shortlist
comes from a float8_e4m3fn index of the same items, a `range_search`, another model's list, or several of them
concatenated.  The candidates of a query come in any order, -1 is "none" and an item may be listed more than once: row q
of the result is the min(k, C) best of the distinct candidates S_q under `search`'s order (score descending, -0 tied with
+0, equal scores by ascending item), each item once, then (-inf, -1) -- what search(q, k, subset=subset(S_q)) returns,
padded -- and a score has the bits `search` and `target_scores` give the pair on this index, a -0 as +0; k=None is
min(C, MAX_K).  It is the threshold pass of `rank_counts` for any C with `search`'s order on top: the pairs are scored
on the scans' own tile through a gallery-row indirection and leave it as keys, 0 for none; one block per query then sorts
the keys in LDS and drops a key equal to its predecessor -- a repeated item has the same score bits and the same number,
hence the same key (mmt_search_rescore).  No atomics; the result depends on the candidates of a query as a set, not on
their order, the row batching or the launch geometry.  ShardedVideoIndex.rescore is bit-identical: every shard re-scores
the candidates it holds and the lists are merged on the primary.  `search_refined` is host code: coarse.search(k=shortlist,
subset=, exclude=) on an index TAKEN to hold the same items under the same numbers (same num_items, num_experts, dim and
device is all that can be checked), then `rescore` on this one.  Out of scope: norm=, pooling=, item_pooling= and groupings.

    scores, indices = index.search(q, qw, k=10, after=(page1_scores[:, -1], page1_indices[:, -1]), subset=..., exclude=..., norm=...)
    scores, indices = index.search_deep(q, qw, depth, page=DEEP_PAGE, subset=None, exclude=None, norm=None, dynamic=None)

The eighth question: the k best items that come AFTER a given position in `search`'s order -- "the next ten results", and
through it a sorted list deeper than MAX_K.  `search`'s order (score descending, -0 tied with +0, equal scores by ascending
item) totally orders a query's candidates, so a position is a (score, item) pair -- one key of the scans -- and "everything
strictly after it" is one more compare at selection time, on the score tile the scan computes anyway
(mmt_search_topk [after]; exclude= holds 32 items and range_search needs a threshold nobody knows in advance).  A cursor row
(a_scores[q], a_items[q]) with a_items[q] >= 0 admits the items g with score(q, g) < a_scores[q], or an equal score (-0 as
+0) and g > a_items[q]; it need not be the position of a stored or allowed item.  (+inf, -1) is no cursor, (-inf, -1) is
exhausted -- the vacant slot of an earlier page -- so after=(scores[:, -1], indices[:, -1]) of the page before is always
valid.  Exact and bit-reproducible like the other seven: a score has the bits plain `search` gives the pair, the rows are
slices of the one complete ordered list, on all three storage dtypes and both index classes (a shard gets the cursor
restated in its own item numbers).  Combines with subset=, exclude=, norm= and dynamic= (the dynamic rule's plain top-1 is
taken without the cursor, so every page of a query makes the same choice); not with pooling= or item_pooling=, and
`search_groups` has no cursor.  `search_deep` is host code: ceil(w / page) pages of `search`, w = min(depth, candidates),
each continuing from the last column of the one before, concatenated to [NQ, w].

    index.schedule = 'stream'                                          # a property of the index: None, 'tile' or 'stream'
    scores, indices = index.search(q, qw, k=10, subset=..., exclude=..., after=...)
    coarse.schedule = 'stream'; scores, indices = fine.search_refined(q, qw, coarse, k=10)

Not a further question but a second SCHEDULE of the first: the launches above are tuned for evaluation, thousands of queries
at once; a service answers one caption, or a few, at a time, and then the scan is a matter of reading the gallery once.
On an index whose `schedule` is 'stream', `search` sends its plain top-k pass to mmt_search_topk_stream: a block holds 32 query rows, a gallery row goes
from memory straight into the registers of the lane that multiplies it, a whole slab ahead, and never through LDS; the
queries go through LDS double-buffered, one barrier per slab.  Meant for NQ <= 32; any NQ is taken.  The results are
`search`'s to the bit on all three storage dtypes and both index classes -- the same MFMA sequence per pair, the same
epilogue expression, the same keys and running top-k, a merge by rank that looks at the lists' heads first -- so the
schedule is a matter of speed alone (one query over 262 144 items in 0.44 ms on bf16, 0.28 ms on fp8).  It combines with
subset=, exclude= and after=; norm=, dynamic=, pooling= and item_pooling= are refused by name.  Opt-in: an index starts
with schedule None, None and 'tile' take exactly the calls they always took, and nothing chooses a schedule by NQ.  It
is a setting of the index and not an argument of `search`, whose parameter list stays what it was.

    scores, rows = index.reverse_search(q, qw, k=10)                       # [num_items, k'], k' = min(k, NQ), k <= MAX_RK = 32
    norm = index.csls_norm(bank_embds, bank_weights, k=10, dynamic=False)  # HubNorm: kind='csls', .k, .beta == 2.0, .lse = r
    scores, indices = index.search(q, qw, k=10, norm=norm)                 # every norm= consumer, unchanged

The ninth question runs the other way: per stored ITEM, the k best QUERY rows -- which captions pull on a video (hubness
diagnosis, reciprocal-neighbour checks, mining the captions that wrongly land on it).  The eight above answer per query and
the lse pass of `hub_norm` collapses an item's column to one number; the only other route is the NQ x num_items matrix this
module exists to avoid, or a second index of the queries searched with the items, which doubles the storage and, on a
bfloat16 or float8_e4m3fn index, rounds the other operand, so its scores are not the bits `search` gives the pair.  The
order is `search`'s with the row number in the item's place -- score descending, -0 tied with +0, equal scores by ascending
query row (the text layout numbers its rows b * C + c) -- and a score has the bits `search` returns for the pair on this
index, on all three storage dtypes.  The rows stream through the scan in batches of whole 64-row blocks; every block
leaves its best k rows per item, and a fold keeps a running list per item across blocks and batches
(mmt_search_col_topk, the tenth entry: additive, no option of the descriptor).  Keys of distinct rows are distinct, so
the k best of a union do not depend on the batching, the launch geometry, num_items, the item's position or the shard:
ShardedVideoIndex.reverse_search -- every shard takes all the rows and answers for its own items -- is bit-identical.
It takes no options.  `csls_norm` puts the second standard hubness correction on it, Cross-domain Similarity Local Scaling
(Conneau et al., ICLR 2018; the other bank normaliser of QB-Norm): r[g] = the mean of item g's k' = min(k, NB) best bank
scores, in fp32 as v = s_0, v = fl(v + s_i) in list order, r[g] = fl(v * float32(1 / k')) -- no fma, no division, restated
bit for bit by numpy.  CSLS ranks by 2 score(q, g) - r_q - r[g]; r_q is constant within a query's row, so the ranking is
that of fl(fl(2 * score(q, g)) - r[g]): the norm slot above with beta = 2 and r in place of lse.  Hence no scoring kernel
of its own, and `search`, `rank_counts`, `ranks`, `target_scores`, `threshold_counts`, the dynamic rule, after=, subset=,
exclude=, both index classes and metric.retrieval_metrics_indexed(bank_norm='csls', bank_k=) take it as they take a
`hub_norm`.  Like `hub_norm` it is refused on a float8_e4m3fn index, because norm= is.

    sims = index.pair_scores(candidates)                                   # int64 [R, C <= MAX_DC = 128] -> float32 [R, C, C]
    scores, indices, values = index.diversify(q, qw, candidates, k=10, lam=0.5)
    scores, indices, values = index.search_diverse(q, qw, k=10, lam=0.5, shortlist=MAX_K, subset=None, exclude=None, coarse=None)

The tenth question: the k best items that are not copies of one another.  The nine above rank by relevance alone, and on a
gallery of clips cut from long videos, re-uploads and crops the top of a list is often one thing several times;
`search_groups` removes such copies only where somebody has labelled them.  Max marginal relevance (Carbonell & Goldstein,
SIGIR 1998) repeatedly picks the item most relevant to the query and least similar to the items already picked.  That
needs the one quantity nothing above computes, the similarity of two STORED items to each other, defined on the stored
values like every score here: with f_g the dequantised stored row (float32: the row; bfloat16: widened; float8_e4m3fn:
code * scales[g]),
    sim(g, h) = <f_g, f_h> / sum_m gw[g][m] gw[h][m]      (0 -> 1e-5)
the 'indep' similarity with item g in the query's place, in fp32 on the matrix cores: one block per shortlist gathers its
rows through a row indirection on BOTH operands and computes the C x C Gram in place (mmt_search_pair_scores), where the
torch route -- index_select of the shortlist rows, then torch.bmm -- materialises 7.5 GB of gathered operands for 4 096
shortlists of 128 rows of 3 584.  sim(g, h) has the bits of sim(h, g) and depends on the two stored rows, their weights and
scales only.  `diversify` is rescore(q, qw, candidates, k=None) -- the distinct candidates in `search`'s order with
`search`'s score bits, rel -- followed by the Gram of that list and the selection (mmt_search_mmr), in fp32 with
a = float32(lam) and b = float32(1.0 - lam): slot 0 is the most relevant item with value fl(a * rel); then every unselected
p has pen_p = the largest sim(p, s) over the selected s and
    v_p = fl(fl(a * rel_p) - fl(b * pen_p))        two rounded multiplies and a rounded subtract, never an fma
and the largest v_p is selected, -0 tied with +0, equal values to the item earlier in `search`'s order; numpy restates it
bit for bit.  Slot t returns the item's relevance, its number and v_p, and a row that runs out of candidates ends in
(-inf, -1, -inf).  lam=1 is `rescore` bit for bit; the result depends on a row's candidates as a set.  `search_diverse` is
host code like `search_refined`: (coarse or self).search(k=shortlist, subset=, exclude=), then `diversify` on this index.
ShardedVideoIndex has the three calls, bit-identical: per row batch every shard copies the stored bytes, weights and scales
of the batch's distinct candidates into a staging index on the primary, the candidates are renumbered into it and the same
kernel runs there -- exact, because sim depends on the two stored rows alone.  Out of scope: norm=, pooling=, item_pooling=,
grouping= and after= raise ValueError naming the option.

    scores, indices = index.neighbours(k=10, items=None, subset=None, source=None)          # [R, k] float32 / int64
    result = index.neighbour_range(threshold, items=None, subset=None, source=None, order='index', max_hits=...)  # RangeResult
    labels = index.duplicate_groups(threshold, subset=None, max_hits=...)                   # int64 [num_items]

The eleventh question: the gallery searched against itself.  The ten above start from a query; a clip gallery is full of
re-uploads, crops and windows of one video, `search_groups` removes such copies only where somebody has labelled them, and
`diversify` works around them inside one 128-item shortlist, per query, at query time.  The quantity is `pair_scores`'
sim(g, h), reachable there only for lists of C <= 128 as a C x C matrix; searching with dequantised rows as queries is a
different quantity (on a bfloat16 or float8_e4m3fn index it re-rounds one operand).  The self-join is a streaming scan
with BOTH operands stored rows (search_self.hip): blocks of 64 row items x one gallery chunk score 64 x 128 tiles with the
Gram kernel's own pieces (search_scan.h: one slab stager, one K loop, one MFMA step, and tk_pair_sims, the one
definition of sim) -- fp32 rows on v_mfma_f32_32x32x2_f32, bf16 rows and exactly widened fp8 codes on one
v_mfma_f32_32x32x16_bf16 per fragment -- so every score the three calls return has exactly the bits `pair_scores` gives
the pair on the same index, on
all three storage dtypes, whatever the row batching, the launch geometry, num_items, the position or the shard.  The order
is `search`'s; the self pair (g, g) is left out by item NUMBER, not by score, so an exact copy of g stays in g's list.
`neighbours` keeps a running top-k per row (the selection, workspace and merge of `search`); `neighbour_range` is the two
scans of `range_search` (one range step on the device, one CSR assembly `_csr` and one pair of batch loops on the host),
no atomics, the total known after the first; `duplicate_groups` turns the threshold graph's edges,
taken from `neighbour_range` in row batches, into connected components by minimum-label propagation with pointer jumping
(`connected_components`, torch ops), labels[g] = the smallest item number of g's component -- which `grouping` accepts
unchanged, so `search_groups` de-duplicates without anybody's labels and `diversify` penalises with the same bits.
source= takes another VideoIndex's items as the rows (an upload batch against the gallery before `add`; no self pair).
ShardedVideoIndex has the three calls, bit-identical: per row batch the rows' stored bytes, weights and scales are staged
on the primary and copied to every shard, which joins them against its own items; lists are merged
(mmt_search_merge_lists), CSR rows assembled by the helper that assembles `range_search`'s
(`_range_csr`).  Out of scope: norm=, pooling=,
item_pooling=, grouping=, after= and exclude= raise ValueError naming the option.

    lse = index.query_lse(q, qw, beta=20.0, subset=None)          # QueryLse: .lse [NQ], .top_scores, .top_items, .sums, .bits
    log_p = lse.log_prob(scores)                                  # any [NQ, ...] scores of those queries; .prob = exp
    scores, indices, log_probs = index.search_softmax(q, qw, k=10, beta=20.0, subset=None)

The twelfth question: what a score is worth.  The eleven above are about order; the common first use of a dual-encoder index
is softmax(beta * sims, dim=-1) -- the probability of each item given the query, the confidence of the top hit, a scale on
which the scores of different queries compare -- and its row-wise log-partition is the missing half of the contrastive loss
this project trains with (loss.InfoNceLoss, large_sim.ShardedInfoNceLoss, model/loss.py:68-81).  `hub_norm` has the column
direction; the row direction cannot be composed from the calls above (`search` returns at most 128 scores per row,
`threshold_counts` counts), and an index of the queries searched with the items re-rounds the other operand.  Every result
here depends on the query and the set of candidates only, and a floating-point sum over 262 144 items cannot keep that
rule; an integer sum can.  In fp32 unless stated, s the bits `search` gives the pair on this index (any dtype):
    x(q, g) = fl(beta * s(q, g))                           a rounded multiply
    xmax[q] = max_g x(q, g) = fl(beta * top-1 score)       fl(beta * .) is monotone: search(k=1, subset=)
    e(q, g) = expf(x(q, g) - xmax[q])                      in [0, 1], exactly 1 for the top-1 item
    t(q, g) = (int64) rint(ldexp(e(q, g), F))              F = lse_bits(num_items) = 62 - ceil(log2(max(num_items, 2)))
    T[q]    = sum_g t(q, g)                                int64: t <= 2^F, num_items <= 2^(62 - F), so T <= 2^62
    lse[q]  = float32(float64(xmax[q]) + log(float64(T[q])) - F ln 2)       lse_from_sums, torch float64 ops
    log_prob(q, g) = fl(x(q, g) - lse[q]),  prob = exp(log_prob)            as the norm= slot: multiply, then subtract
T[q] is one exact number whatever the chunking, the row batching, the block geometry, the order of the items or the shard.
Quantising a term costs at most half a unit, so at most num_items * 2^-(F + 1) relative on T (T >= 2^F), at most 2^(2c - 63)
for num_items <= 2^c: 2^-25 at 2^19 items, below half an fp32 ulp.  Two scans: the top-1 is `search`'s, the sum is the
scans' own score tile with the selection replaced by the sum (mmt_search_row_expsum, search_lse.hip: four threads per
row, an int64 register each across a chunk's tiles, one writer per (row, chunk); a tile without an allowed item is skipped
before its K loop).  `search_softmax` is host code: `search`, `query_lse` fed the top-1 already found, `log_prob`.
ShardedVideoIndex.query_lse takes xmax from the merged top-1 and F from the global num_items; every shard sums over its own
items and the int64 partials are added on the primary: bit-identical in .sums and .lse.  metric.info_nce_indexed evaluates
the reference's InfoNceLoss over a whole evaluation set on it (rows: `query_lse`; columns: `hub_norm`; diagonal:
`target_scores`).  Out of scope: exclude=, norm= (a dual softmax), pooling=, item_pooling=, after= and grouping= raise
ValueError naming the option; a single-pass online softmax would save a scan and lose the bit-identity across shards.

    tg  = index.tagging(tags)                                     # IndexTagging: one int64 tag word per stored item
    flt = tg.where(all_of=0, none_of=0, any_of=0)                 # TagFilter: ints (broadcast) or int64 [NQ] per argument
    scores, indices = index.search(q, qw, k=10, where=flt, subset=..., exclude=..., after=...)

Not a further question but a per-query CANDIDATE SET for the ones above.  `subset=` is one bitmap for every row of a call
and `exclude=` bars at most 32 named items per row; a retrieval service has a predicate per query over what the stored
videos ARE -- "English, not flagged, category A or B", "this channel only".  Every stored item carries one 64-bit tag word
t[g] whose bits mean what the caller decides, every query row three 64-bit masks, and item g is a candidate of row q iff
    (t[g] & all_of[q]) == all_of[q]  and  (t[g] & none_of[q]) == 0  and  (any_of[q] == 0 or (t[g] & any_of[q]) != 0)
-- plain 64-bit integer operations on bit patterns: the int64 tensors are bit patterns, bit 63 an ordinary bit, and a row
whose three masks are 0 admits every item (`tag_pass` restates it in numpy).  The predicate is ANDed with subset=,
exclude= and after= and acts at selection and counting only, so every returned score keeps the bits plain `search` gives
the pair, and ShardedVideoIndex stays bit-identical (the predicate depends on the item and the row alone).  where= is
taken by `search` on both schedules, `search_deep`, `rank_counts`, `ranks`, `threshold_counts`, `range_search` and
`search_refined` (the coarse stage, with a filter from the coarse index's tagging), on all three storage dtypes and both
index classes (mmt_search_topk_where and its four kin: the unfiltered entries' arguments with the tags and the masks
behind the descriptor).  The result shapes are exclude='s: width min(k, candidates after subset), slots without a
candidate hold (-inf, -1); a target of the counts is scored whether or not it passes and counts itself only if it does.
On the tile schedule a 128-item tile in which no (live row, allowed item) pair passes is skipped before its K loop -- an
exact test, so a selective predicate shared by a block's rows costs what the same subset costs; the streaming schedule
filters in the selection alone.  Like a grouping, a tagging describes the num_items of its moment and is
refused after a further `add`; the index's own storage and `nbytes` do not change.  where= with norm=, pooling= or
item_pooling=, and on `search_groups`, `rescore`, `reverse_search`, the self-join and `query_lse`, is a ValueError before
anything is scored; where=None takes exactly the calls above.

    es = index.expert_scores(q, qw, candidates)            # ExpertScores: .parts, .mix float32 [NQ, C, M]; .expert_sims
    scores, indices, es = index.search_explained(q, qw, k=10, subset=None, exclude=None, after=None, where=None)
    es = index.pair_expert_scores(items, candidates)       # items int64 [R]: stored rows in the query's place

The thirteenth question: WHICH EXPERT produced a match, and with what share of the gate.  The twelve above return the
mixture as one number; what makes the model multi-modal -- "matched on speech 46 %, OCR 31 %", the reason for a wrong
top-1, what the renormalisation of a missing modality (gw[g][m] = 0) did, whether two "duplicates" agree in the picture
or only in the audio track -- is its decomposition, which is exact and additive: the score is a sum over experts of
terms that share one denominator.  With qf = fold_fp32(Q, qw)[q], f_g the dequantised stored row (float32: the row;
bfloat16: widened; float8_e4m3fn: code * scales[g]) and den = sum_m qw[q][m] gw[g][m] in fp32 in expert order (0 -> 1e-5):
    dot_m  = sum_{j < d} qf[m d + j] * f_g[m d + j]
    part_m = dot_m / den           float8_e4m3fn: fl(fl(dot_m * scales[g]) / den) on the codes, as the scans place the scale
    mix_m  = fl(qw[q][m] * gw[g][m]) / den
sum_m part_m is the score on the stored value -- what `search` returns on this index -- sum_m mix_m is 1 (0 where the
denominator was 0) and expert_sims = part_m / mix_m is <Q_m[q], G_m[g]>, the pair's similarity under expert m alone (the
cosine, for unit-norm experts).  candidates int64 [NQ, C <= MAX_C = 1024] as for `rescore` (-1 = none, any order, repeats);
a none has NaN in all M slots.  Only the listed rows are touched: a gather of NQ * C stored rows at about 2 flops per
byte, so it runs on the vector ALUs -- one wave per pair, 16-byte loads of the stored row, the query's fold in LDS
(mmt_search_expert_parts, search_explain.hip) -- not on the 64 x 128 MFMA tile of `rescore`, which computes 64 rows to keep
one; M one-hot-weight searches would cost M full scans and answer another question (another denominator), and
index_select + dequantise + einsum materialises 7.5 GB for 4 096 x 128 hits and needs a dequantiser.  dot_m is one fp32
fma chain per lane in an order fixed by (d, dtype) and the element index alone, then a fixed butterfly; both quotients are
correctly rounded divisions.  Hence, deduced and not measured: the values of a pair depend on the pair alone, bit for bit
-- not on its place in the list, the other candidates, C, NQ, the row batching, the query layout or the shard
(ShardedVideoIndex: every shard explains the candidates it holds and the primary takes each pair from its owner) -- and
every part is within (d + M + 4) * 2^-24 * <|qf_m|, |f_g,m|> / |den| of the fp64 value of the definition.  The fold is
the fp32 one on every dtype: the entry takes plain arguments, not the descriptor, whose q / q_lo are the bf16 pair on a
bfloat16 or float8_e4m3fn index.  `search_explained` is host code like `search_refined`: `search` with the given options
under the index's schedule, then `expert_scores` of the returned indices; the list is `search`'s to the bit and a vacant
slot has NaN parts.  `pair_expert_scores` explains the hits of `pair_scores`, `neighbours` and `duplicate_groups`: the R
rows of `items` are gathered and dequantised to fp32 (exact), their stored weights serve as qw and the same kernel runs,
so the parts sum to sim(g, h) and, every product commuting and the denominator being symmetric, (g, h) has the bits of
(h, g).  4 096 x 128 pairs on 262 144 items x 7 x 512 take 1.40 ms on a float32 index, 0.79 ms on bfloat16 and 0.78 ms on
float8_e4m3fn.  Out of scope: norm=, dynamic=, pooling= and item_pooling= raise ValueError naming the
option -- the parts explain the plain score -- and there is no per-expert top-k over the whole gallery.

Cell-probed search (`cells`, `search_probed`; `cells_from_centres`, `cells.probes`, `search_cells`): the inverted file,
the cut of a scan PER QUERY that `subset=` (one set for the whole call), `where=` (64 tag bits, a tile skipped only when no
row of a 64-query block wants it) and `rescore` (1 024 candidates, 64 rows computed to keep one) do not give.  The items
are partitioned into cells, `index.cells(cell_ids)`, once: a CSR of item numbers sorted by (cell, item); the stored rows
stay where they are.  `search_probed(q, qw, cells, probes, k)` takes int64 [NQ, P <= MAX_PROBES = 64] cell numbers per row
(-1 = none, a repeat counts once) and row q of the result is the k best items of the union of its cells in `search`'s
order -- equal scores by ascending item number across cells too -- then (-inf, -1): search(subset = those items) for that
row, with the score bits of `search`, `rescore` and `target_scores`, on all three dtypes.  Exact; the approximation of an
inverted file is the choice of cells, and that is the caller's: a k-means of their own and a coarse index, or
`cells_from_centres(centres)`, which assigns every item to its best centre with `neighbours` and whose `probes` are
`search` over the centres.  The (row, probe) pairs are regrouped on the device -- sorted by (cell, row), cut into groups of
at most 64 rows and pieces of at most CELL_PIECE = 2 048 items (`probe_plan` is the numpy restatement) -- and one block per
(group, piece) scans 64 x 128 tiles through two row tables with the K loop, epilogue, running top-k and merge of the other
scans (mmt_search_topk_cells, search_cells.hip).  A result depends on the row's probes as a set alone.  Timings, tile counts
and recall: DESIGN 9.24.  Out of scope: subset=, exclude=, after=, where=, norm=, dynamic=, pooling=, item_pooling= and
grouping= raise ValueError naming the option; no trainer, no product quantisation, no re-ordering of the stored rows.

K-means cells (`train_cells`, `cell_sums`, `cell_centroids`; `CellQuantiser`): the trainer the inverted file lacked.  A
stored item is its folded row f_g = gw_g (.) G_g and its weights gw_g; for a cell with member list L (its slice of
`IndexCells.items`, ascending, n = |L|)
    S[m] = sum_{g in L} f_g[m]      w[m] = sum_{g in L} gw_g[m]      G_c[m] = S[m] / |S[m]|_2      gw_c[m] = w[m] / n
on the stored values dequantised exactly: spherical k-means per expert, weighted by the gate -- a member without a
modality adds nothing to that expert, an expert missing in every member has weight 0 in the centroid and a zero row, and
the centroid of a one-item cell is the item.  `cell_sums` and `cell_centroids` are the update step (search_kmeans.hip:
a cell's list is cut into pieces of SUM_PIECE = 256 positions, a thread owns its columns and adds a piece's rows in
ascending position, one block per cell joins the pieces in ascending order; no atomics, so two calls are bit-identical
and a cell's sums do not depend on the other cells, num_items or the launch -- `cell_sums_ref` restates the order);
the assignment step is `centroids.neighbours(k=1, source=index)` against a VideoIndex of the centroids in the gallery's
dtype.  `train_cells(num_cells, iters)` is the Lloyd loop around them, deterministic, with empty cells re-seeded by the
worst-served items (`reseed_ref`), and returns a `CellQuantiser`: `.assign(index)` gives that index's cells, whose
`probes` and `search_cells` then work as on cells made from centres.  Timings and recall: DESIGN 9.25.  Out of scope:
these fp32 sums on a ShardedVideoIndex (they depend on the order of a cell's list; the exact sums below do not), subset=,
where=, norm=, pooling= and item_pooling=: ValueError naming the call or the option.

Exact cell sums (`sum_scale`, `cell_sums_exact`, `cell_centroids(exact=True)`, `train_cells(exact=True)`, `assign_cells`, on
VideoIndex and ShardedVideoIndex): the update step with an accumulator whose result does not depend on the order of the
additions, the idea of `query_lse`.  THE DEFINITION.  f_g[k] is the dequantised stored value of item g, column k, exactly
as `cell_sums` forms it in fp32 (fp32 as stored, bf16 widened, fp8 code x the item's scale), gw_g[m] its weights, and the
index holds num_items items.
    bits B = lse_bits(num_items)
    exponent E = the least integer with max |f_g[k]| <= 2^E over the stored rows (0 when all are zero; a maximum of
                 exactly 1.0 gives 0, the next float up 1); wexponent the same over |gw_g[m]|
    term(g, k) = (int64) rint(f_g[k] * 2^(B - E))     in fp64, where the scaling is exact; nearest, ties to even
    sums[c][k] = sum_{g in cell c} term(g, k)         int64; wsums likewise with wexponent; counts as `cell_sums`
    S = ldexp(float32(sum), E - B)                    float32(sum): ONE int64 -> fp32 conversion, nearest even
|term| <= 2^B and a cell has at most num_items <= 2^(62 - B) members, so a sum stays within +-2^62; a value beyond 2^E (a
stale or foreign scale) is clamped to +-2^B and never wraps.  Integer addition is associative, so the sums are functions
of a cell's member SET: the same items inserted in another order, or spread over shards, give the same sums and the same
centroids.  |S - sum f| <= n_c 2^(E - B - 1) + ulp32(S) / 2 per column.  The conversion back never goes through fp64, which
would round twice (2^53 + 2^29 + 1).  The centroid is `cell_centroids`' formula on these S and w, by the same device code,
so equal fp32 sums give equal centroid bits on both paths.  `sum_scale_ref`, `cell_sums_exact_ref` and `exact_sums_float`
restate it in numpy.  `sum_scale()` -> SumScale(exponent, wexponent, bits, num_items): one pass over the stored rows
(mmt_search_absmax) and the one host sync of the path, kept until the next `add`.  On a ShardedVideoIndex E and wexponent
are the maxima over the shards and B comes from the global num_items; every shard sums its own part of the cells under
those three numbers on its own device (mmt_search_cell_sums_exact), the int64 tensors are added on the primary, and the
finish runs there (mmt_search_cell_centroids_exact).  Everything is opt-in by name: the fp32 accumulator stays the default
on a VideoIndex, bit for bit, and plain `train_cells`, `cell_sums`, `cell_centroids` and `quantiser.assign` keep raising
ValueError on a ShardedVideoIndex.  With exact=True its `train_cells` is the same Lloyd loop -- the assignment shard by
shard against a copy of the centroids on the shard's device, labels and scores gathered on the primary -- and for any
placement of the same items the sums, centroids, objective, moved, iterations and labels, and `assign_cells` and
`search_cells` on the result, are bit-identical to one VideoIndex; checked, as everything in that class, with all shards
on one device.  Timings: DESIGN 9.26.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import check

MAX_K = 128
DEEP_PAGE = 64  # default page of `search_deep`: the width at which a scan costs least per column
MAX_T = 32  # targets per query and launch of the rank kernels; wider target lists are sliced
MAX_E = 32  # exclusions per query of a masked search
MAX_RK = 32  # query rows per item of `reverse_search` and `csls_norm`: a wave's list of the fold is k + 64 keys of LDS
MAX_C = 1024  # candidates per query of `rescore`: one query's keys are sorted in LDS
MAX_DC = 128  # candidates per query of `pair_scores` and `diversify`: one block computes a list's C x C Gram
_NOT_DIVERSE = ('norm', 'dynamic', 'pooling', 'item_pooling', 'grouping', 'after')  # options `diversify` refuses by name
MAX_SET = 64  # rows per query set of a pooled scan: one 64-row query block holds whole sets
MAX_ITEM_SET = 128  # items per stored set of an item-pooled scan: one 128-column tile holds whole sets
_POOL_MODES = {'mean': 0, 'max': 1}  # the `mode` of the pooled entry points
_BATCH_BYTES = 48 << 20  # folded queries (fp32, or the bf16 hi + lo pair: 4 bytes per element either way) + chunk lists
_MAX_HITS = 1 << 27  # default cap of a range search's total: a guard against a mistyped threshold, not a tuned number
_NOT_SELF = ('norm', 'pooling', 'item_pooling', 'grouping', 'after', 'exclude', 'where')  # options the self-join refuses by name
_NOT_EXPLAINED = ('norm', 'dynamic', 'pooling', 'item_pooling')  # options `search_explained` refuses by name
_NOT_LSE = ('exclude', 'norm', 'pooling', 'item_pooling', 'after', 'grouping', 'where')  # options `query_lse` refuses by name
MAX_PROBES = 64  # cells per query row of `search_probed`: a row's lists in the merge are MAX_PROBES * pieces * k keys
CELL_PIECE = 2048  # items of a cell one block of the probed scan walks (16 tiles); a larger cell is cut into pieces
_NOT_PROBED = ('subset', 'exclude', 'after', 'where', 'norm', 'dynamic', 'pooling', 'item_pooling', 'grouping')  # refused by name
SUM_PIECE = 256  # positions of a cell's list one block of `cell_sums` adds; a longer list is cut into pieces
SUM_SLAB = 1024  # columns of the M * d one block of `cell_sums` takes
MAX_SUM_EXPONENT = 160  # |exponent| of a SumScale: past every finite fp32 magnitude (MMT_SEARCH_SUM_MAX_EXPONENT)
_ABSMAX_BLOCKS = 1024  # blocks of the `sum_scale` pass at most: 256 K threads grid-striding over the 16-byte groups
_NOT_TRAINED = ('subset', 'where', 'norm', 'pooling', 'item_pooling')  # options the k-means calls refuse by name
_GROUP_ROWS = 1 << 16  # rows per `neighbour_range` call of `duplicate_groups`: the CSR of a batch is dropped for its edges
FP8 = torch.float8_e4m3fn
_DTYPES = {torch.float32: 4, torch.bfloat16: 8, FP8: 16}  # storage dtype -> multiple d must have (16-byte folded rows)
_STORAGE = {torch.float32: _lib.SEARCH_FP32, torch.bfloat16: _lib.SEARCH_BF16, FP8: _lib.SEARCH_FP8}  # MmtSearchScan.storage
# sets tag of a scan -> the workspace-size functions of its top-k and its count pass
_WORKSPACES = {_lib.SEARCH_SETS_NONE: ('mmt_topk_workspace_keys', 'mmt_count_workspace_ints'),
               _lib.SEARCH_SETS_QUERY: ('mmt_topk_pooled_workspace_keys', 'mmt_count_pooled_workspace_ints'),
               _lib.SEARCH_SETS_ITEM: ('mmt_topk_itemsets_workspace_keys', 'mmt_count_itemsets_workspace_ints')}


def _cuda_f32(x, name):
  if not torch.is_tensor(x) or not x.is_cuda:
    raise ValueError('%s must be a CUDA tensor' % name)
  return x.to(torch.float32).contiguous()


def _fold(x, w):
  n, m, d = x.shape
  out = torch.empty(n, m * d, device=x.device, dtype=torch.float32)
  check(_lib.lib().mmt_search_fold(ops._p(x), ops._p(w), n, m, d, ops._p(out), ops._stream()), 'mmt_search_fold')
  return out


def _dequantised(stored, dtype, scales):
  """Stored rows as bytes (uint8 [n, row bytes]) of an index of `dtype`, with their scales (float8_e4m3fn) or None -> the
  rows in fp32 [n, M * d]: float32 as it is, bfloat16 widened, float8_e4m3fn code * scale -- a power of two.  All exact."""
  rows = stored.view(dtype).to(torch.float32)
  return rows if scales is None else rows * scales[:, None]


def _limits(exclude, after, nq, nv):
  """The checks of `search` that look at values, together: exclude and after (types, devices and ranks already checked) ->
  (None or int64 [NQ, E]; None or the cursor as (scores float32 [NQ], first int64 [NQ])).  The exclusions are held against
  -1 .. nv - 1; a cursor row is a position (item 0 .. nv - 1, any score but NaN), (+inf, -1) = no cursor or (-inf, -1) =
  exhausted.  `first` is the lowest item number still admitted at the cursor's score, item + 1, and -1 where the row is a
  sentinel (tk_tile_select of search_topk.h; mmt_search_after_keys).  One small reduction each and ONE host sync for both."""
  ex, cursor, facts = None, None, []
  if exclude is not None:
    if exclude.shape[0] != nq:
      raise ValueError('search: %d queries but exclude %s' % (nq, tuple(exclude.shape)))
    ex = exclude.reshape(nq, -1).contiguous()
    if nq:
      facts += list(torch.aminmax(ex))
  if after is not None:
    a_scores, a_items = after
    if a_scores.shape[0] != nq:
      raise ValueError('search: %d queries but after holds %d rows' % (nq, a_scores.shape[0]))
    a_scores, a_items = a_scores.contiguous(), a_items.contiguous()
    if nq:
      facts += [torch.isnan(a_scores).any().long(), ((a_items == -1) & ~torch.isinf(a_scores)).any().long()]
      facts += list(torch.aminmax(a_items))
    cursor = (a_scores, torch.where(a_items >= 0, a_items + 1, a_items))
  if facts:
    facts = [int(v) for v in torch.stack(facts).tolist()]
    if ex is not None and (facts[0] < -1 or facts[1] >= nv):
      raise ValueError('search: exclude must lie in -1 .. %d, got %d .. %d' % (nv - 1, facts[0], facts[1]))
    if cursor is not None:
      nan, loose, lo, hi = facts[-4:]
      if nan:
        raise ValueError('search: the scores of after must not be NaN')
      if lo < -1 or hi >= nv:
        raise ValueError('search: the items of after must lie in -1 .. %d, got %d .. %d' % (nv - 1, lo, hi))
      if loose:
        raise ValueError('search: an item of -1 in after goes with a score of +inf (no cursor) or -inf (exhausted)')
  return ex, cursor


def _width(embds):
  """d of an (NV, M, d) argument, read off its shape alone; None for anything else (the later checks say what)."""
  shape = getattr(embds, 'shape', None)
  return shape[-1] if shape is not None and len(shape) == 3 else None


def _check_dtype(dtype, dim=None):
  """The storage dtype and, where it is known as a plain int already, the width d it allows: no tensor is looked at."""
  if dtype not in _DTYPES:
    raise ValueError('VideoIndex: dtype must be torch.float32, torch.bfloat16 or torch.float8_e4m3fn, got %r' % (dtype,))
  if dtype == FP8 and isinstance(dim, int) and not isinstance(dim, bool) and (dim < 16 or dim % 16):
    raise ValueError('VideoIndex: need d %% 16 == 0 for %s (16-byte folded rows), got d = %d' % (dtype, dim))


class IndexSubset:
  """A set of items of a VideoIndex, packed for the masked scans (VideoIndex.subset): `words` is the uint32 bitmap on the
  device (bit i & 31 of word i >> 5 is item i; 4 words per 128 items, padding bits zero), `mask` the same as bool
  [num_items], `count` the number of allowed items, `num_items` the index size it was built for."""

  def __init__(self, mask, count):
    n = mask.shape[0]
    self.num_items, self.device, self.mask, self.count = n, mask.device, mask, count
    words = torch.empty(4 * -(-n // 128), device=mask.device, dtype=torch.int32)
    with torch.cuda.device(mask.device):
      check(_lib.lib().mmt_search_subset_pack(ops._p(mask.view(torch.uint8)), n, ops._p(words), ops._stream()),
            'mmt_search_subset_pack')
    self.words = words.view(torch.uint32)


class HubNorm:
  """The querybank normaliser of a VideoIndex (VideoIndex.hub_norm): `lse` fp32 [num_items] on the index device,
  lse[g] = log sum_b exp(beta * score(b, g)) over the `bank_size` bank queries; `beta`; `num_items` and `device` it was built
  for; `hubs` bool [num_items] (dynamic=True, else None): the items that are the plain top-1 of at least one bank query.
  `kind` is 'softmax' for that, or 'csls' (VideoIndex.csls_norm): `lse` then holds r[g], the mean of item g's `k` best bank
  scores, and `beta` is 2.0 -- the same slot of every scan, fl(fl(beta * score) - lse[g]); `k` is None for 'softmax'."""

  def __init__(self, lse, beta, bank_size, hubs=None, *, kind='softmax', k=None):
    self.lse, self.beta, self.bank_size, self.hubs = lse, beta, bank_size, hubs
    self.num_items, self.device = lse.shape[0], lse.device
    self.kind, self.k = kind, k


class RangeResult:
  """The hits of a range search (VideoIndex.range_search) as a CSR over the queries, on the index device: query q's hits are
  positions offsets[q] .. offsets[q + 1] - 1 of `indices` (int64 item numbers) and `scores` (float32); `offsets` int64
  [NQ + 1] with offsets[0] = 0, `counts` int64 [NQ] = offsets[1:] - offsets[:-1]."""

  def __init__(self, offsets, indices, scores):
    self.offsets, self.indices, self.scores = offsets, indices, scores
    self.counts = offsets[1:] - offsets[:-1]


class ExpertScores:
  """The per-expert breakdown of scores (`expert_scores`, `search_explained`, `pair_expert_scores`) on the index device:
  `parts` and `mix` float32 [R, C, M], slot m of pair (r, candidates[r, c]) -- part_m, expert m's share of the score (the
  parts of a pair sum to its score), and mix_m, expert m's share of the gate (they sum to 1, or to 0 where the pair's
  denominator was 0); NaN in all M slots of a candidate of -1.  `expert_sims` = parts / mix, the raw similarity
  <Q_m, G_m> of the pair under expert m alone (the cosine, for unit-norm experts): torch's division, NaN where the
  expert has no share of the gate (a missing modality: 0 / 0)."""

  def __init__(self, parts, mix):
    self.parts, self.mix = parts, mix

  @property
  def expert_sims(self):
    return self.parts / self.mix


MAX_GROUP_ID = 2 ** 31 - 2


class IndexGrouping:
  """The groups of a VideoIndex's items (VideoIndex.grouping): `ids` int32 [num_items] on the index device, the group of
  every item; `num_groups` the number of distinct ids; `num_items` and `device` it was built for."""

  def __init__(self, ids, num_groups):
    self.ids, self.num_groups = ids, num_groups
    self.num_items, self.device = ids.shape[0], ids.device


class ShardedGrouping:
  """The groups of a ShardedVideoIndex's items (ShardedVideoIndex.grouping): `parts[s]` is shard s's IndexGrouping in its own
  item order on its own device (None for a shard without items), with the same, global, group ids; `ids` int32 [num_items]
  in global item order on the primary device; `num_groups`, `num_items`, `device`."""

  def __init__(self, parts, ids, num_groups):
    self.parts, self.ids, self.num_groups = parts, ids, num_groups
    self.num_items, self.device = ids.shape[0], ids.device


def _mask_word(name, v):
  """One argument of `where` that is a Python int: 0 .. 2^64 - 1 -> the int64 with that bit pattern."""
  if not 0 <= v < 1 << 64:
    raise ValueError('where: %s must lie in 0 .. 2^64 - 1, got %d' % (name, v))
  return v - (1 << 64) if v >= 1 << 63 else v


def _tag_filter(tagging, all_of, none_of, any_of):
  """The checks of `where` -> TagFilter over `tagging`."""
  given = (('all_of', all_of), ('none_of', none_of), ('any_of', any_of))
  rows = None
  for name, v in given:
    if torch.is_tensor(v):
      if v.dtype != torch.int64:
        raise ValueError('where: %s must be an int or an int64 tensor, got %s' % (name, v.dtype))
      if v.device != tagging.device:
        raise ValueError('where: %s must be on the index device %s, got %s' % (name, tagging.device, v.device))
      if v.dim() != 1:
        raise ValueError('where: %s [NQ] expected, got %s' % (name, tuple(v.shape)))
      if rows is not None and v.shape[0] != rows:
        raise ValueError('where: %s holds %d rows, the masks before it %d' % (name, v.shape[0], rows))
      rows = v.shape[0]
    elif isinstance(v, bool) or not isinstance(v, int):
      raise ValueError('where: %s must be an int or an int64 tensor, got %s' % (name, type(v).__name__))
  words = [v if torch.is_tensor(v) else _mask_word(name, v) for name, v in given]
  masks = torch.empty(1 if rows is None else rows, 3, device=tagging.device, dtype=torch.int64)
  for j, w in enumerate(words):
    masks[:, j] = w
  return TagFilter(masks, tagging, rows)


class TagFilter:
  """The per-query attribute filter of a scan (IndexTagging.where / ShardedTagging.where), passed as where=: `masks` int64
  [NQ, 3] on the index device, contiguous, row q = (all_of, none_of, any_of) as bit patterns; `tagging` the tagging it
  filters; `num_rows` = NQ, the query rows a call must bring -- or None when every argument was a Python int: `masks` is
  then [1, 3] and stands for any number of rows."""

  def __init__(self, masks, tagging, num_rows):
    self.masks, self.tagging, self.num_rows = masks, tagging, num_rows

  def _rows(self, nq):
    """The masks of a call with nq query rows, [nq, 3] contiguous (a broadcast filter is written out)."""
    return self.masks if self.num_rows is not None else self.masks.expand(nq, 3).contiguous()

  def _passes(self, items):
    """Which of items int64 [NQ, T] (-1 = none, which fails) pass their row's masks -> bool [NQ, T], in torch ops on the
    tagging's device: `tag_pass` for the given pairs."""
    t = self.tagging.tags[items.clamp(min=0)]
    a, n, y = (self.masks[:, j:j + 1] for j in range(3))
    return (items >= 0) & ((t & a) == a) & ((t & n) == 0) & ((y == 0) | ((t & y) != 0))


class IndexTagging:
  """The attribute tags of a VideoIndex's items (VideoIndex.tagging): `tags` int64 [num_items] on the index device, one
  64-bit word per item, a bit pattern whose bits mean what the caller decides (one-hot fields, flags, cohort bits);
  `num_items` and `device` it was built for."""

  def __init__(self, tags):
    self.tags = tags
    self.num_items, self.device = tags.shape[0], tags.device

  def where(self, all_of=0, none_of=0, any_of=0):
    """The filter of a call's query rows -> TagFilter for where=.  Each argument is a Python int in 0 .. 2^64 - 1 (the
    same mask for every row) or an int64 tensor [NQ] on the index device (a bit pattern per row; bit 63 is an ordinary
    bit); tensors must agree in NQ.  Item g is a candidate of row q iff (t[g] & all_of[q]) == all_of[q] and
    (t[g] & none_of[q]) == 0 and (any_of[q] == 0 or (t[g] & any_of[q]) != 0).  Nothing here waits for the device."""
    return _tag_filter(self, all_of, none_of, any_of)


class ShardedTagging:
  """The attribute tags of a ShardedVideoIndex's items (ShardedVideoIndex.tagging): `parts[s]` is shard s's IndexTagging in
  its own item order on its own device (None for a shard without items); `tags` int64 [num_items] in global item order on
  the primary device; `num_items`, `device`."""

  def __init__(self, parts, tags):
    self.parts, self.tags = parts, tags
    self.num_items, self.device = tags.shape[0], tags.device

  where = IndexTagging.where


class QueryPooling:
  """How the query rows of a pooled scan form sets (VideoIndex.pooling / ShardedVideoIndex.pooling): `num_sets` sets of
  `set_size` consecutive rows, `num_rows` = num_sets * set_size; `weights` float32 [num_rows] on `device`, the row weights
  (a row with weight 0 takes no part); `mode` 'mean' or 'max'.  It does not depend on the number of stored items."""

  def __init__(self, set_size, num_sets, weights, mode):
    self.set_size, self.num_sets, self.num_rows = set_size, num_sets, set_size * num_sets
    self.weights, self.mode, self.device = weights, mode, weights.device
    self._copies = {weights.device: weights}

  def _on(self, device):
    """The weights on a shard's device, copied once."""
    if device not in self._copies:
      self._copies[device] = self.weights.to(device)
    return self._copies[device]


def _mask_of(items, n, device, what='items'):
  """The checks of a subset of n numbered things -> (the set as a bool mask [n] of its own, the number allowed)."""
  if not torch.is_tensor(items) or items.dtype not in (torch.bool, torch.int64):
    raise ValueError('subset: %s must be a bool or int64 tensor, got %s' % (
        what, items.dtype if torch.is_tensor(items) else type(items).__name__))
  if items.device != device:
    raise ValueError('subset: %s must be on the index device %s, got %s' % (what, device, items.device))
  if items.dtype == torch.bool:
    if tuple(items.shape) != (n,):
      raise ValueError('subset: a bool mask of shape (%d,) expected, got %s' % (n, tuple(items.shape)))
    mask = items.contiguous().clone()
  else:
    ids = items.reshape(-1)
    if ids.numel() == 0:
      raise ValueError('subset: no item allowed')
    lo, hi = (int(v) for v in torch.aminmax(ids))
    if lo < 0 or hi >= n:
      raise ValueError('subset: %s must lie in 0 .. %d, got %d .. %d' % (what, n - 1, lo, hi))
    mask = torch.zeros(n, device=device, dtype=torch.bool).index_fill_(0, ids, True)
  count = int(mask.sum())
  if count == 0:
    raise ValueError('subset: no item allowed')
  return mask, count


class ItemPooling:
  """How the stored items of an item-pooled scan form sets (VideoIndex.item_pooling): `num_sets` sets of `set_size`
  consecutive items, `num_items` = num_sets * set_size, the index size it was built for; `weights` float32 [num_items] on
  `device`, the item weights (an item with weight 0 takes no part); `mode` 'mean' or 'max'."""

  def __init__(self, set_size, num_sets, weights, mode):
    self.set_size, self.num_sets, self.num_items = set_size, num_sets, set_size * num_sets
    self.weights, self.mode, self.device = weights, mode, weights.device

  @property
  def _columns(self):
    """The virtual columns of the scans: 128 per tile of 128 // set_size whole sets."""
    return 128 * -(-self.num_sets // (128 // self.set_size))

  def subset(self, sets):
    """sets: bool [num_sets] (True = allowed) or int64 set numbers (any shape, any order, duplicates allowed), on the
    index device -> the IndexSubset over SET numbers (its num_items is num_sets) that subset= takes next to this
    item_pooling=.  Checked and packed as VideoIndex.subset."""
    return IndexSubset(*_mask_of(sets, self.num_sets, self.device, 'sets'))


class ShardedItemPooling:
  """The item sets of a ShardedVideoIndex (ShardedVideoIndex.item_pooling): `parts[s]` is shard s's ItemPooling in its own
  set numbers on its own device (None for a shard without items); `tables[s]` int64 on the primary, shard s's local set ->
  global set; `weights` float32 [num_items] in global item order on the primary; `set_size`, `num_sets`, `num_items`,
  `mode`, `device`."""

  def __init__(self, set_size, num_sets, weights, mode, parts, tables, set_shard_of, set_local_of):
    self.set_size, self.num_sets, self.num_items = set_size, num_sets, set_size * num_sets
    self.weights, self.mode, self.device = weights, mode, weights.device
    self.parts, self.tables = parts, tables
    self._maps = (set_shard_of, set_local_of)   # global set -> (shard, local set), on the primary
    self._table_cache = {}

  def subset(self, sets):
    """sets: bool [num_sets] or int64 set numbers on the primary device, as ItemPooling.subset -> ShardedSubset over SET
    numbers: the set cut into one IndexSubset per shard, in the shard's own set numbers."""
    return _cut_subset(*_mask_of(sets, self.num_sets, self.device, 'sets'),
                       [(table, part and part.device) for table, part in zip(self.tables, self.parts)])


def _cut_subset(mask, count, tables):
  """A set as a bool mask on the primary and the number allowed -> ShardedSubset: the mask cut into one IndexSubset per
  shard through tables, one (the shard's local -> global table on the primary, the shard's device) per shard -- the table
  None for a shard that holds nothing, which like a shard without an allowed member gets no part."""
  parts = []
  for table, device in tables:
    part = None
    if table is not None:
      local = mask[table]  # gathered on the primary, where the table is
      with torch.cuda.device(device):
        local = local.to(device)
        allowed = int(local.sum())
        if allowed:
          part = IndexSubset(local, allowed)
    parts.append(part)
  return ShardedSubset(parts, mask, count)


def sets_whole(shard_of, local_of, set_size):
  """Whether sets of `set_size` consecutive global items are each stored whole on one shard, in order, starting at a local
  item number that is a multiple of set_size: (global item -> shard, global item -> local item), int64 [num_sets *
  set_size] -> a 0-dim bool tensor on their device (one reduction, no host sync here)."""
  so, lo = shard_of.view(-1, set_size), local_of.view(-1, set_size)
  steps = torch.arange(set_size, device=lo.device, dtype=lo.dtype)
  return ((so == so[:, :1]) & (lo == lo[:, :1] + steps) & (lo[:, :1] % set_size == 0)).all()


def _check_sets(who, member, ints, max_size, count, count_first, mode, weights, device):
  """The checks of `pooling` (member 'a row') and `item_pooling` ('an item'): sets of set_size members with a mode and a
  weight per member -> (num_sets, the weights as float32 [num_sets * set_size] of their own).  ints: the (name, value)
  pairs that must be ints, set_size first; count(): the caller's own limits on the number of sets, which returns it --
  asked before the mode is looked at (count_first) or after it.  One small reduction and one host sync where weights are
  given."""
  for name, v in ints:
    if isinstance(v, bool) or not isinstance(v, int):
      raise ValueError('%s: %s must be an int, got %r' % (who, name, v))
  set_size, noun = ints[0][1], member.split()[1] + '_weights'
  if not 1 <= set_size <= max_size:
    raise ValueError('%s: set_size must lie in 1..%d, got %d' % (who, max_size, set_size))
  if count_first:
    num_sets = count()
  if mode not in _POOL_MODES:
    raise ValueError("%s: mode must be 'mean' or 'max', got %r" % (who, mode))
  if not count_first:
    num_sets = count()
  n = num_sets * set_size
  if weights is None:
    return num_sets, torch.full((n,), 1.0 / set_size, device=device, dtype=torch.float32)
  if not torch.is_tensor(weights) or weights.dtype != torch.float32:
    raise ValueError('%s: %s must be a float32 tensor, got %s' % (
        who, noun, weights.dtype if torch.is_tensor(weights) else type(weights).__name__))
  if weights.device != device:
    raise ValueError('%s: %s must be on the index device %s, got %s' % (who, noun, device, weights.device))
  if tuple(weights.shape) not in ((n,), (num_sets, set_size)):
    raise ValueError('%s: %s of shape (%d,) or (%d, %d) expected, got %s' % (
        who, noun, n, num_sets, set_size, tuple(weights.shape)))
  w = weights.reshape(-1).contiguous().clone()
  if num_sets:
    sets = w.view(num_sets, set_size)
    finite, manned = (bool(v) for v in torch.stack([torch.isfinite(w).all(), (sets != 0).any(1).all()]).tolist())
    if not finite:
      raise ValueError('%s: %s must be finite' % (who, noun))
    if not manned:
      raise ValueError('%s: every set needs %s with a weight other than 0' % (who, member))
  return num_sets, w


def _check_item_sets(who, set_size, num_items, item_weights, mode, device):
  """The checks of `item_pooling` on either index class -> (num_sets, the weights as float32 [num_items] of their own)."""
  def count():
    if num_items == 0:
      raise ValueError('%s: the index holds no items' % who)
    if num_items % set_size:
      raise ValueError('%s: %d items are no whole number of sets of %d' % (who, num_items, set_size))
    return num_items // set_size
  return _check_sets(who, 'an item', (('set_size', set_size),), MAX_ITEM_SET, count, False, mode, item_weights, device)


def _count_groups(ids):
  """The number of distinct values of a non-empty id tensor: one torch.unique, whose size is the one wait for the device."""
  return int(torch.unique(ids).numel())


def _csr_rows(offsets):
  """offsets int64 [NQ + 1] -> the row of every CSR position, int64 [offsets[-1]]."""
  counts = offsets[1:] - offsets[:-1]
  return torch.repeat_interleave(torch.arange(counts.shape[0], device=offsets.device), counts)


def _range_result(offsets, indices, scores, order):
  """A CSR whose rows ascend by item -> RangeResult in the given order.  order='score' is `search`'s order (tk_key of the
  kernels): descending score with -0 tied to +0, equal scores by ascending item -- two stable torch sorts, by score over
  everything (which keeps (row, item) order among equal scores), then by row."""
  if order == 'score' and indices.numel():
    by_score = torch.argsort(scores + 0.0, descending=True, stable=True)  # -0.0 + 0.0 = +0.0
    perm = by_score[torch.argsort(_csr_rows(offsets)[by_score], stable=True)]
    indices, scores = indices[perm], scores[perm]
  return RangeResult(offsets, indices, scores)


def search_order(scores, items):
  """The order of `search` (tk_key of the kernels) over one list: scores float32 [n] and item numbers int64 [n] (distinct)
  -> the positions int64 [n], best first: score descending with -0 tied to +0, equal scores by ascending item number.
  Two stable torch sorts, on CPU or device tensors; a NaN has no place in a list and is not expected here."""
  by_item = torch.argsort(items, stable=True)
  return by_item[torch.argsort((scores + 0.0)[by_item], descending=True, stable=True)]   # -0.0 + 0.0 = +0.0


def tag_pass(tags, masks):
  """The attribute filter restated in numpy: tags int64 / uint64 [NV] and masks [NQ, 3] = (all_of, none_of, any_of) per
  row -- numpy arrays or torch tensors (copied to the host) -> bool [NQ, NV], True where item g is a candidate of row q:
  (t & all_of) == all_of and (t & none_of) == 0 and (any_of == 0 or (t & any_of) != 0), computed on the uint64 VIEW of
  both, so bit 63 is a bit like the others."""
  host = lambda x: np.ascontiguousarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
  t, m = host(tags), host(masks)
  if t.dtype not in (np.int64, np.uint64) or m.dtype not in (np.int64, np.uint64):
    raise ValueError('tag_pass: 64-bit integer tags and masks expected, got %s and %s' % (t.dtype, m.dtype))
  t, m = t.view(np.uint64).reshape(1, -1), m.view(np.uint64).reshape(-1, 3)
  a, n, y = m[:, 0:1], m[:, 1:2], m[:, 2:3]
  zero = np.uint64(0)
  return ((t & a) == a) & ((t & n) == zero) & ((y == zero) | ((t & y) != zero))


def cell_lists(cell_ids, num_cells):
  """The CSR of `cells` restated in numpy: cell_ids int64 [num_items], values -1 .. num_cells - 1 (-1 = in no cell; a numpy
  array or a torch tensor, copied to the host) -> (offsets int64 [num_cells + 1], items int64 [offsets[-1]]): the item
  numbers sorted by (cell, item), cell c at offsets[c] .. offsets[c + 1]."""
  ids = np.asarray(cell_ids.detach().cpu().numpy() if torch.is_tensor(cell_ids) else cell_ids, dtype=np.int64)
  items = np.flatnonzero(ids >= 0)
  items = items[np.argsort(ids[items], kind='stable')]
  offsets = np.concatenate([[0], np.cumsum(np.bincount(ids[ids >= 0], minlength=num_cells))])
  return offsets.astype(np.int64), items.astype(np.int64)


def probe_plan(probes, offsets, piece=CELL_PIECE):
  """The regrouping of `search_probed` (`_probe_plan`, which runs on the device) restated in numpy: probes int64 [NQ, P]
  and the cells' offsets int64 [num_cells + 1] (numpy arrays or torch tensors, copied to the host) -> (pair_row int32 [n],
  pair_slot int32 [n], work int32 [w, 5]), the tables of mmt_search_topk_cells without the device plan's padding.  A probe
  outside 0 .. num_cells - 1 (-1 = none), an empty cell and a cell listed again in its row are dropped.  Every row is sorted
  by cell, a dropped probe behind the others, and a pair's SLOT is its place in that sorted row; the pairs that stay are
  ordered by (cell, row).  Each cell's pairs are cut into row groups of at most 64 and its items into ceil(size / piece)
  pieces of at most `piece`; the work items go cell by cell, group by group, piece by piece, each (first pair, rows, first
  position in the item table, end position, piece).  A function of the probes and the offsets alone.  The number of 64 x
  128 tile K loops the scan runs is the sum over the work items of ceil((end - first) / 128)."""
  host = lambda x: np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, dtype=np.int64)
  p, off = host(probes), host(offsets)
  c, sizes = off.shape[0] - 1, np.diff(off)
  ok = (p >= 0) & (p < c)
  ok &= sizes[np.where(ok, p, 0)] > 0
  s = np.sort(np.where(ok, p, c), axis=1)
  live = s < c
  live[:, 1:] &= s[:, 1:] != s[:, :-1]
  rows, slots = np.nonzero(live)
  cell = s[rows, slots]
  order = np.lexsort((rows, cell))
  rows, slots, cell = rows[order], slots[order], cell[order]
  work, start = [], 0
  for ci, count in zip(*np.unique(cell, return_counts=True)):
    for g in range(0, count, 64):
      for pc in range(-(-sizes[ci] // piece)):
        first = off[ci] + pc * piece
        work.append((start + g, min(64, count - g), first, min(first + piece, off[ci + 1]), pc))
    start += count
  return rows.astype(np.int32), slots.astype(np.int32), np.array(work, dtype=np.int32).reshape(-1, 5)


def _probe_plan(probes, offsets, max_pieces, piece=CELL_PIECE):
  """`probe_plan` in torch, where the probes are (the device; any device works): probes int64 [NQ, P], offsets int64
  [num_cells + 1 >= 2], max_pieces >= the largest cell's piece count -> (pair_row int32 [NQ * P], pair_slot int32 [NQ * P],
  work int32 [W, 5]).  Nothing here waits for the device, so the lengths are upper bounds: the kept pairs come first in the
  pair tables (behind them what the sort leaves of the dropped ones, which no work item refers to), and W = max_pieces *
  min(NQ * P, num_cells + NQ * P // 64) bounds the work items -- a cell's row groups number ceil(pairs / 64) <= 1 + pairs //
  64 and no more than its pairs -- the entries past the real count being zero: rows = 0, no work.  Two stable sorts (every
  row by cell; the pairs by cell * NQ + row, a key no two kept pairs share), two searchsorted and a prefix sum: the same
  probes give the same tables."""
  nq, width = probes.shape
  c, dev = offsets.shape[0] - 1, probes.device
  sizes = offsets[1:] - offsets[:-1]
  ok = (probes >= 0) & (probes < c)
  ok &= sizes[probes.clamp(0, c - 1)] > 0
  s, _ = torch.sort(torch.where(ok, probes, torch.full_like(probes, c)), dim=1, stable=True)
  live = s < c
  live[:, 1:] &= s[:, 1:] != s[:, :-1]
  row = torch.arange(nq, device=dev, dtype=torch.int64).unsqueeze(1)
  key, order = torch.sort(torch.where(live, s * nq + row, torch.full_like(s, c * nq)).reshape(-1), stable=True)
  pair_row, pair_slot = (key % nq).to(torch.int32), (order % width).to(torch.int32)
  bounds = torch.searchsorted(key, torch.arange(c + 1, device=dev, dtype=torch.int64) * nq)
  start, count = bounds[:-1], bounds[1:] - bounds[:-1]            # a cell's first pair, its pairs
  pieces = (sizes + (piece - 1)) // piece
  per_cell = (count + 63) // 64 * pieces                           # row groups x pieces
  end = torch.cumsum(per_cell, 0)
  w = torch.arange(max_pieces * min(nq * width, c + nq * width // 64), device=dev, dtype=torch.int64)
  cell = torch.searchsorted(end, w, right=True)
  none = (cell >= c).unsqueeze(1)
  cell = cell.clamp(max=c - 1)
  local = w - (end - per_cell)[cell]
  pcs = pieces[cell].clamp(min=1)
  group, pc = local // pcs, local % pcs
  first = offsets[cell] + pc * piece
  work = torch.stack([start[cell] + 64 * group, (count[cell] - 64 * group).clamp(max=64), first,
                      torch.minimum(first + piece, offsets[cell + 1]), pc], 1)
  return pair_row, pair_slot, torch.where(none, torch.zeros_like(work), work).to(torch.int32).contiguous()


def cell_sums_ref(rows, weights, offsets, items, piece=SUM_PIECE):
  """The order of `cell_sums` (mmt_search_cell_sums, mmt_search_cell_centroids) restated in numpy: rows float32
  [num_items, M * d], the stored rows dequantised; weights float32 [num_items, M]; offsets and items the cells' CSR (numpy
  arrays or torch tensors, copied to the host) -> (sums float32 [C, M * d], wsums float32 [C, M], counts int64 [C]).  A
  cell's list is cut into pieces of at most `piece` positions; a piece's rows are added in ascending position, one fp32
  add each from +0, and the pieces' partial rows in ascending order, again from +0.  Bit for bit what the kernels give."""
  host = lambda x: np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
  rows, weights = host(rows).astype(np.float32, copy=False), host(weights).astype(np.float32, copy=False)
  off, items = host(offsets).astype(np.int64), host(items).astype(np.int64)
  c = off.shape[0] - 1
  sums, wsums = np.zeros((c, rows.shape[1]), np.float32), np.zeros((c, weights.shape[1]), np.float32)
  for ci in range(c):
    for first in range(off[ci], off[ci + 1], piece):
      part, wpart = np.zeros(rows.shape[1], np.float32), np.zeros(weights.shape[1], np.float32)
      for g in items[first:min(first + piece, off[ci + 1])]:
        part, wpart = part + rows[g], wpart + weights[g]
      sums[ci], wsums[ci] = sums[ci] + part, wsums[ci] + wpart
  return sums, wsums, np.diff(off)


def _exponent_of(largest):
  """The least integer E with largest <= 2^E for a finite float largest >= 0; 0 for 0.  Exactly 1.0 gives 0, the next
  float up 1."""
  if not largest > 0:
    return 0
  mantissa, e = math.frexp(largest)   # largest = mantissa * 2^e, 0.5 <= mantissa < 1
  return e - 1 if mantissa == 0.5 else e


class SumScale:
  """The fixed-point scale of the exact cell sums (module docstring; `sum_scale`): `exponent` E and `wexponent`, the least
  integers with |stored value| <= 2^E and |weight| <= 2^wexponent over the index; `bits` B = lse_bits(num_items); and the
  `num_items` it was made for.  A term is rint(value * 2^(B - E)) as int64.  Indexes whose sums are to be added share one
  scale: a ShardedVideoIndex hands its own to every shard.  One made by hand (exponents at or above the index's own,
  |exponent| <= MAX_SUM_EXPONENT) is accepted by the index whose num_items it names."""

  def __init__(self, exponent, wexponent, bits, num_items):
    for name, v in (('exponent', exponent), ('wexponent', wexponent)):
      if isinstance(v, bool) or not isinstance(v, int) or abs(v) > MAX_SUM_EXPONENT:
        raise ValueError('SumScale: %s must be an int in -%d .. %d, got %r' % (name, MAX_SUM_EXPONENT, MAX_SUM_EXPONENT, v))
    if isinstance(bits, bool) or not isinstance(bits, int) or bits != lse_bits(num_items):
      raise ValueError('SumScale: bits must be lse_bits(num_items) = %d, got %r' % (lse_bits(num_items), bits))
    self.exponent, self.wexponent, self.bits, self.num_items = exponent, wexponent, bits, num_items
    self._index = None   # the index whose `sum_scale` made it

  def __eq__(self, other):
    return isinstance(other, SumScale) and (self.exponent, self.wexponent, self.bits, self.num_items) == (
        other.exponent, other.wexponent, other.bits, other.num_items)

  __hash__ = None

  def __repr__(self):
    return 'SumScale(exponent=%d, wexponent=%d, bits=%d, num_items=%d)' % (
        self.exponent, self.wexponent, self.bits, self.num_items)


def _host(x):
  return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)


def sum_scale_ref(rows, weights):
  """`sum_scale` restated in numpy: rows float32 [num_items, M * d], the stored rows dequantised; weights float32
  [num_items, M] (numpy arrays or torch tensors, copied to the host) -> SumScale.  The exponents are those of the largest
  magnitudes, and a maximum does not care how the rows are split: over the shards of a ShardedVideoIndex they are the
  largest of the shards' exponents, and bits comes from the global num_items."""
  rows, weights = _host(rows).astype(np.float32, copy=False), _host(weights).astype(np.float32, copy=False)
  n = rows.shape[0]
  return SumScale(_exponent_of(float(np.abs(rows).max(initial=0))), _exponent_of(float(np.abs(weights).max(initial=0))),
                  lse_bits(n), n)


def _exact_terms(values, exponent, bits):
  """float32 values -> int64 rint(value * 2^(bits - exponent)): scaled in fp64 (exact), rounded to nearest even, clamped
  to +-2^bits."""
  scaled = np.ldexp(values.astype(np.float64), bits - exponent)
  return np.clip(np.rint(scaled), -2.0 ** bits, 2.0 ** bits).astype(np.int64)


def cell_sums_exact_ref(rows, weights, offsets, items, scale):
  """The definition of `cell_sums_exact` (mmt_search_cell_sums_exact) restated in numpy: rows, weights, offsets and items
  as `cell_sums_ref` takes them, scale a SumScale -> (sums int64 [C, M * d], wsums int64 [C, M], counts int64 [C]): per
  cell the integer sum of its members' terms.  Integer addition is associative, so the order of a cell's list and any
  split of the items into parts whose results are added give the same numbers."""
  rows, weights = _host(rows).astype(np.float32, copy=False), _host(weights).astype(np.float32, copy=False)
  off, items = _host(offsets).astype(np.int64), _host(items).astype(np.int64)
  c = off.shape[0] - 1
  sums, wsums = np.zeros((c, rows.shape[1]), np.int64), np.zeros((c, weights.shape[1]), np.int64)
  for ci in range(c):
    members = items[off[ci]:off[ci + 1]]
    sums[ci] = _exact_terms(rows[members], scale.exponent, scale.bits).sum(0, dtype=np.int64)
    wsums[ci] = _exact_terms(weights[members], scale.wexponent, scale.bits).sum(0, dtype=np.int64)
  return sums, wsums, np.diff(off)


def exact_sums_float(sums, exponent, bits):
  """Exact sums back in fp32, restated in numpy: int64 sums (any shape) -> float32 ldexp(float32(sum), exponent - bits).
  float32(sum) is the direct int64 -> fp32 conversion, rounded once to nearest even (__ll2float_rn on the device); a
  detour through fp64 would round twice and give other bits (2^53 + 2^29 + 1)."""
  return np.ldexp(_host(sums).astype(np.int64).astype(np.float32), np.int32(exponent - bits)).astype(np.float32)


class ExactCellSums:
  """What `cell_sums_exact` returns, on the index device (the primary of a sharded index): `sums` int64 [C, M * d] and
  `wsums` int64 [C, M], the integer sums of the members' terms under `scale` (a SumScale); `counts` int64 [C].  `float()`
  gives (sums, wsums, counts) with the sums in fp32, as `cell_sums` shapes them."""

  def __init__(self, sums, wsums, counts, scale):
    self.sums, self.wsums, self.counts, self.scale, self.device = sums, wsums, counts, scale, sums.device

  def float(self):
    """(sums float32 [C, M * d], wsums float32 [C, M], counts): ldexp(float32(sum), E - B) on the device, the conversion
    rounded once (mmt_search_cell_centroids_exact without a centroid; `exact_sums_float` restates it)."""
    offsets = torch.cat([self.counts.new_zeros(1), torch.cumsum(self.counts, 0)])
    fsums, fwsums = _exact_finish(self.sums, self.wsums, offsets, self.scale, None, None)
    return fsums, fwsums, self.counts.clone()


def _exact_finish(sums, wsums, offsets, scale, embds, weights):
  """int64 sums [C, M * d] / wsums [C, M] and the cells' offsets int64 [C + 1] on one device, a SumScale and the in/out
  centroid buffers (embds [C, M, d], weights [C, M]) or None -> (sums, wsums) float32 there; the centroids of the cells
  that have items are written (mmt_search_cell_centroids_exact).  Nothing here waits for the device."""
  c, m = wsums.shape
  d = sums.shape[1] // m
  fsums, fwsums = torch.empty(c, m * d, device=sums.device), torch.empty(c, m, device=sums.device)
  with torch.cuda.device(sums.device):
    check(_lib.lib().mmt_search_cell_centroids_exact(
        ops._p(sums), ops._p(wsums), ops._p(offsets), max(scale.num_items, 1), c, m, d, scale.bits, scale.exponent,
        scale.wexponent, ops._p(fsums), ops._p(fwsums), ops._p(embds), ops._p(weights), ops._stream()),
          'mmt_search_cell_centroids_exact')
  return fsums, fwsums


def reseed_ref(ids, scores, items, num_cells):
  """The re-seeding rule of `train_cells` restated in numpy: ids int64 [num_items], the labels after an assignment (-1 =
  not in the sample); items int64 [T] ascending, the training sample; scores float32 [T], the score of items[i] under its
  best centroid -> the labels with the empty cells filled.  The E cells without an item, in ascending cell number,
  receive the E items of the sample with the lowest scores -- a stable sort by score over ascending item numbers, so equal
  scores go to the smaller number -- and those items are relabelled.  A cell the relabelling empties stays empty."""
  ids, items = np.array(ids, dtype=np.int64), np.asarray(items, dtype=np.int64)
  empty = np.flatnonzero(np.bincount(ids[items], minlength=num_cells) == 0)
  worst = items[np.argsort(np.asarray(scores, dtype=np.float32), kind='stable')[:len(empty)]]
  ids[worst] = empty
  return ids


def _reseed(ids, scores, items, num_cells):
  """`reseed_ref` in torch, where the labels are: nothing here waits for the device.  Cell c, when empty, is the e-th empty
  cell and takes the e-th item of the stable sort; the cells that have items write to a slot behind the labels."""
  n = ids.shape[0]
  empty = torch.bincount(ids[items], minlength=num_cells) == 0
  nth = (torch.cumsum(empty, 0) - 1).clamp(min=0, max=items.shape[0] - 1)
  worst = items[torch.sort(scores, stable=True)[1]][nth]
  out = torch.cat([ids, ids.new_zeros(1)])
  out.scatter_(0, torch.where(empty, worst, torch.full_like(worst, n)), torch.arange(num_cells, device=ids.device))
  return out[:n]


def _sum_plan(offsets, n_work, piece=SUM_PIECE):
  """The piece tables of `cell_sums`, in torch where the offsets are (the device; any device works): offsets int64
  [num_cells + 1], n_work >= the number of pieces, a bound the host knows without waiting (ceil(labelled / piece) +
  num_cells) -> (work int32 [n_work, 3] = (cell, first position, end position), cell by cell, piece by piece, the entries
  past the real count zero: no work; piece_start int32 [num_cells + 1]: cell c's pieces are piece_start[c] ..
  piece_start[c + 1] - 1)."""
  c = offsets.shape[0] - 1
  sizes = offsets[1:] - offsets[:-1]
  pieces = (sizes + (piece - 1)) // piece
  end = torch.cumsum(pieces, 0)
  w = torch.arange(n_work, device=offsets.device, dtype=torch.int64)
  cell = torch.searchsorted(end, w, right=True)
  none = (cell >= c).unsqueeze(1)
  cell = cell.clamp(max=c - 1)
  first = offsets[cell] + (w - (end - pieces)[cell]) * piece
  work = torch.stack([cell, first, torch.minimum(first + piece, offsets[cell + 1])], 1)
  start = torch.cat([end.new_zeros(1), end])
  return torch.where(none, torch.zeros_like(work), work).to(torch.int32).contiguous(), start.to(torch.int32)


class CellQuantiser:
  """A trained coarse quantiser (VideoIndex.train_cells).  `centroids`: a VideoIndex of num_cells items in the gallery's
  dtype, M and d -- item c is the centroid of cell c, folded and rounded by `add`; `embds` [num_cells, M, d] and `weights`
  [num_cells, M]: the unrounded fp32 values it was built from; `objective` and `moved`: device tensors [iterations], the
  mean score of a training item under its best centroid at each assignment and the labels that changed against the
  iteration before; `iterations`: the iterations run (fewer than asked when an assignment moved nothing); `num_cells`;
  `exact`: whether the updates used the exact integer sums (train_cells(exact=True)), and then `scale`, their SumScale,
  else None."""

  def __init__(self, centroids, embds, weights, objective, moved, exact=False, scale=None):
    self.centroids, self.embds, self.weights = centroids, embds, weights
    self.objective, self.moved = objective, moved
    self.iterations, self.num_cells = objective.shape[0], centroids.num_items
    self.exact, self.scale = exact, scale

  def assign(self, index, **unsupported):
    """index: a VideoIndex with the centroids' dtype, num_experts and dim on their device -> its IndexCells over ALL its
    items: item g joins the cell of its best centroid, centroids.neighbours(k=1, source=index), ties to the lower cell.
    The cells carry `.quantiser`, so `cells.probes` and `index.search_cells` work on them.  Not on a ShardedVideoIndex."""
    for name in unsupported:
      if name not in _NOT_TRAINED:
        raise TypeError('assign() got an unexpected keyword argument %r' % name)
      raise ValueError('assign: %s= is out of scope: every item joins the cell of its best centroid' % name)
    if hasattr(index, 'shards'):
      raise ValueError('assign: not available on a ShardedVideoIndex; call its assign_cells(quantiser)')
    _, best = self.centroids.neighbours(k=1, source=index)
    cells = index.cells(best[:, 0].contiguous(), self.num_cells)
    cells.quantiser = self
    return cells

  def probes(self, embds, weights, nprobe):
    """Queries as for `search` -> probes int64 [NQ, min(nprobe, num_cells)] for `search_probed`: per row the cells of its
    nprobe best centroids, best first -- centroids.search(k=nprobe)[1]: the item numbers of the centroid index are the cell
    numbers.  nprobe an int in 1 .. MAX_PROBES."""
    if isinstance(nprobe, bool) or not isinstance(nprobe, int) or not 1 <= nprobe <= MAX_PROBES:
      raise ValueError('probes: nprobe must be an int in 1..%d, got %r' % (MAX_PROBES, nprobe))
    return self.centroids.search(embds, weights, k=min(nprobe, self.num_cells))[1]


class IndexCells:
  """A partition of a VideoIndex's items into cells (VideoIndex.cells, cells_from_centres): the inverted file that
  `search_probed` reads.  `offsets` int64 [num_cells + 1] and `items` int64: the item numbers sorted by (cell, item), cell c
  at offsets[c] .. offsets[c + 1], so a cell's items ascend; `sizes` int64 [num_cells]; `num_cells`, `num_items` (the index
  size it was built for), `device`; `max_pieces`: the pieces of CELL_PIECE items the largest cell is cut into, known here so
  that no call has to ask the device.  `centres`: int64 [num_cells], the centre items of cells made by `cells_from_centres`
  -- cell c is the cell of item centres[c] -- else None; `quantiser`: the CellQuantiser of cells made by its `assign`, else
  None; only cells with one of the two answer `probes`.  The stored rows are not moved or copied: the scan reads them
  through `items`."""

  def __init__(self, index, offsets, items, num_items):
    self._index = index
    self.offsets, self.items = offsets, items
    self.sizes = offsets[1:] - offsets[:-1]
    self.num_cells, self.num_items, self.device = offsets.shape[0] - 1, num_items, offsets.device
    self.max_pieces = max(1, -(-int(self.sizes.max()) // CELL_PIECE))   # the one wait for the device of the build
    self.centres = self._subset = self._cell_of = self.quantiser = None

  def probes(self, embds, weights, nprobe):
    """Queries as for `search` -> probes int64 [NQ, min(nprobe, num_cells)] for `search_probed`: per row the cells of its
    nprobe best centres, best first -- search(embds, weights, k=nprobe, subset=subset(centres)) on the cells' index, the
    item numbers mapped to cell numbers through a table, a vacant slot staying -1.  nprobe an int in 1 .. MAX_PROBES.
    Only on cells made by `cells_from_centres`; with a quantiser of their own a caller takes the probes from its
    coarse_index.search(...)[1]."""
    if self.quantiser is not None:
      if self._index.num_items != self.num_items:
        raise ValueError('probes: the cells were built for %d items, the index holds %d' % (self.num_items, self._index.num_items))
      return self.quantiser.probes(embds, weights, nprobe)
    if self.centres is None:
      raise ValueError('probes: these cells were not made from centres; take the probes from a coarse index of your own')
    if isinstance(nprobe, bool) or not isinstance(nprobe, int) or not 1 <= nprobe <= MAX_PROBES:
      raise ValueError('probes: nprobe must be an int in 1..%d, got %r' % (MAX_PROBES, nprobe))
    if self._index.num_items != self.num_items:
      raise ValueError('probes: the cells were built for %d items, the index holds %d' % (self.num_items, self._index.num_items))
    _, best = self._index.search(embds, weights, k=nprobe, subset=self._subset)
    return torch.where(best >= 0, self._cell_of[best.clamp(min=0)], best)


class ShardedCells(IndexCells):
  """The cells of a ShardedVideoIndex: IndexCells in global item numbers on the primary device, and `parts[s]`: shard s's
  IndexCells -- the restriction of every cell to the items the shard holds, in its own numbers on its own device (None for
  a shard without items)."""

  def __init__(self, index, offsets, items, num_items, parts):
    super().__init__(index, offsets, items, num_items)
    self.parts = parts


def connected_components(num_items, src, dst):
  """The connected components of the undirected graph on 0 .. num_items - 1 with the edges (src[i], dst[i]) -- int64 [E]
  each, on one device, CPU included; direction, order and repeats do not matter -> labels int64 [num_items] there:
  labels[g] is the smallest number in g's component.  Minimum-label propagation with pointer jumping: labels start as
  the item's own number; a round pulls the two ends of every edge down to the smaller of their labels (scatter amin) and
  then replaces labels by labels[labels] until that changes nothing -- a label is always a member of the item's own
  component and never above the item, so the jump is safe and roughly halves the rounds a long chain needs.  It stops when
  a round changes nothing: then both ends of every edge carry one label, a component carries one label, and that label,
  a member no larger than any member, is its minimum.  Each comparison is one host sync."""
  labels = torch.arange(num_items, device=src.device, dtype=torch.int64)
  if src.numel() == 0:
    return labels
  while True:
    low = torch.minimum(labels[src], labels[dst])
    new = labels.scatter_reduce(0, src, low, 'amin').scatter_reduce(0, dst, low, 'amin')
    while True:
      jumped = new[new]
      if torch.equal(jumped, new):
        break
      new = jumped
    if torch.equal(new, labels):
      return labels
    labels = new


def _check_beta(beta, who='hub_norm'):
  if isinstance(beta, bool) or not isinstance(beta, float) or not 0 < beta < math.inf:
    raise ValueError('%s: beta must be a float with 0 < beta < inf, got %r' % (who, beta))


def lse_bits(num_items):
  """F of `query_lse` for an index of num_items items: 62 - ceil(log2(max(num_items, 2))), the fixed-point position of the
  terms of the integer sum.  A term is at most 2^F and there are at most num_items <= 2^(62 - F) of them, so the int64
  sum stays at or below 2^62."""
  if isinstance(num_items, bool) or not isinstance(num_items, int) or not 1 <= num_items < 2 ** 62:
    raise ValueError('lse_bits: num_items must be an int in 1 .. 2^62 - 1, got %r' % (num_items,))
  return 62 - max(1, (num_items - 1).bit_length())


def fixed_terms(e, bits):
  """The terms of the integer sum: float32 e in [0, 1] (any shape, any device) -> int64 rint(ldexp(e, bits)).  The scaling
  by 2^bits is exact; the rounding is to nearest, ties to even, and changes only values below 2^24 (a float32 at or above
  that is an integer already).  e = 1 gives 2^bits, a value below 2^-(bits + 1) gives 0."""
  return torch.ldexp(e.to(torch.float32), torch.tensor(bits, device=e.device)).round().to(torch.int64)


def lse_from_sums(xmax, sums, bits):
  """The log-sum-exp of `query_lse` from its integer sums: float32 xmax [NQ] and int64 sums [NQ] (same device) ->
  float32(float64(xmax) + log(float64(sums)) - bits * ln 2), evaluated in float64 in that order."""
  return (xmax.to(torch.float64) + torch.log(sums.to(torch.float64)) - bits * math.log(2.0)).to(torch.float32)


class QueryLse:
  """The softmax normaliser of a batch of queries over an index (VideoIndex.query_lse), on the index device (the primary of
  a sharded index): `lse` float32 [NQ], lse[q] = log sum_g exp(fl(beta * score(q, g))) over the query's `count`
  candidates; `beta`; `top_scores` float32 [NQ] / `top_items` int64 [NQ], the search(k=1) row of each query; `sums` int64
  [NQ], the integer sums T[q] of the terms rint(exp(x - xmax) * 2^bits); `bits` = lse_bits(num_items); `num_items` and
  `device` it was built for.  `log_prob` and `prob` put scores of THESE queries on THIS index on the softmax's scale."""

  def __init__(self, lse, beta, top_scores, top_items, sums, bits, num_items, count):
    self.lse, self.beta, self.top_scores, self.top_items = lse, beta, top_scores, top_items
    self.sums, self.bits, self.num_items, self.count, self.device = sums, bits, num_items, count, lse.device

  def log_prob(self, scores):
    """scores float32 [NQ, ...] of these queries on that index (`search`'s list, `target_scores`, a RangeResult row by
    row) -> fl(fl(beta * score) - lse[q]) of their shape: a rounded multiply, then a rounded subtract, as the norm= slot.
    A vacant slot (-inf) stays -inf."""
    if not torch.is_tensor(scores) or scores.dtype != torch.float32:
      raise ValueError('log_prob: scores must be a float32 tensor, got %s' % (
          scores.dtype if torch.is_tensor(scores) else type(scores).__name__))
    if scores.dim() < 1 or scores.shape[0] != self.lse.shape[0]:
      raise ValueError('log_prob: scores [%d, ...] expected, got %s' % (self.lse.shape[0], tuple(scores.shape)))
    if scores.device != self.device:
      raise ValueError('log_prob: scores must be on %s, got %s' % (self.device, scores.device))
    x = scores * torch.tensor(self.beta, device=self.device, dtype=torch.float32)
    return x - self.lse.reshape((-1,) + (1,) * (scores.dim() - 1))

  def prob(self, scores):
    """exp(log_prob(scores)): the share of the candidates' probability mass each scored item holds for its query."""
    return torch.exp(self.log_prob(scores))


def _where_option(full):
  """Gives a public call the keyword-only option where= without putting it into the call's own parameter list, which
  the tests of earlier changes pin name for name (DESIGN 9.21 kept `search`'s list by making the schedule a property; a
  filter belongs to the call, so it cannot go that way).  The decorated method is the call as it was and is what runs
  without a filter; with one, `full` runs -- the same call with `where` as its last parameter, whose docstring the
  public name shows.  `inspect.signature` follows the wrapper to the decorated method and so does NOT list where=; the
  docstring does."""
  def decorate(method):
    @functools.wraps(method)
    def call(self, *args, where=None, **kwargs):
      if where is None:
        return method(self, *args, **kwargs)
      return full(self, *args, where=where, **kwargs)
    call.__doc__ = full.__doc__
    return call
  return decorate


def _refuses_where(method):
  """The same for a call that takes no filter: where= is a ValueError by the call's name, before anything is looked at,
  instead of the TypeError of an unknown keyword."""
  @functools.wraps(method)
  def call(self, *args, where=None, **kwargs):
    if where is not None:
      raise ValueError('%s: where= is out of scope: this call takes no per-query filter' % method.__name__)
    return method(self, *args, **kwargs)
  return call


def _check_rk(who, k):
  if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_RK:
    raise ValueError('%s: k must be an int in 1..%d, got %r' % (who, MAX_RK, k))


def _check_dynamic(dynamic, norm, who):
  """The `dynamic` of a call with norm= -> whether QB-Norm's per-query rule applies: None follows the norm (it applies
  when the norm carries `hubs`), False normalises every query, True demands a norm built with dynamic=True."""
  if dynamic is not None and not isinstance(dynamic, bool):
    raise ValueError('%s: dynamic must be None, False or True, got %r' % (who, dynamic))
  if norm is None:
    if dynamic:
      raise ValueError('%s: dynamic=True needs norm=' % who)
    return False
  if dynamic and norm.hubs is None:
    raise ValueError('%s: dynamic=True needs a norm built with hub_norm(..., dynamic=True)' % who)
  return norm.hubs is not None if dynamic is None else dynamic


def _pick(use, normed, plain):
  """Per query row: the normalised result where `use`, else the plain one (tensors of equal shape, rows first)."""
  return torch.where(use.reshape((-1,) + (1,) * (normed.dim() - 1)), normed, plain)


class _Scan:
  """What a scan is asked to do beside its queries: subset (an IndexSubset, on a sharded index a ShardedSubset), ex (int64
  [NQ, E] exclusions, checked), norm (a HubNorm / ShardedHubNorm: every query normalised), pooling (a QueryPooling) and
  item_pooling (an ItemPooling / ShardedItemPooling), each None unless given and already checked against the index, and
  after (the cursor of a paged `search`, checked: scores float32 [NQ] and first int64 [NQ], the lowest item number still
  admitted at that score in the index's own numbers, -1 where the score is a sentinel: _limits), and stream: whether the
  top-k pass takes the streaming schedule (`search` on an index whose schedule is 'stream'; every shard's view keeps it), and
  where (a TagFilter, checked against the index and the call's query rows: the per-query attribute filter, which sends the
  top-k, count and range passes to their `_where` entries).  A public call builds it
  once and every internal call takes it whole; the sizes that depend on which options are there are answered here."""

  def __init__(self, subset=None, ex=None, norm=None, pooling=None, item_pooling=None, after=None, stream=False,
               where=None):
    self.subset, self.ex, self.norm, self.pooling, self.item_pooling = subset, ex, norm, pooling, item_pooling
    self.after, self.where = after, where
    # `search` on an index set to 'stream': the top-k pass goes to mmt_search_topk_stream (checked: no norm, no sets)
    self.stream = stream
    # MmtSearchScan.sets: whose rows come in sets
    self.sets = (_lib.SEARCH_SETS_ITEM if item_pooling is not None else
                 _lib.SEARCH_SETS_QUERY if pooling is not None else _lib.SEARCH_SETS_NONE)

  def plain(self):
    """The same candidates without the norm, the cursor kept: the result the dynamic rule falls back to."""
    return _Scan(self.subset, self.ex, after=self.after, where=self.where)

  def uncursored(self):
    """The candidates of the whole list, without norm or cursor: what the dynamic rule DECIDES on -- a query's plain top-1,
    which is then the same on every page of that query."""
    return _Scan(self.subset, self.ex, where=self.where)

  def at(self, after):
    """The same scan from another cursor (None = from the top): the pages of `search_deep`."""
    return _Scan(self.subset, self.ex, self.norm, self.pooling, self.item_pooling, after, self.stream, self.where)

  def rows(self, q):
    """The rows of the outputs: one per query, or with a pooling one per query set."""
    return q.shape[0] if self.pooling is None else self.pooling.num_sets

  def numbered(self, index):
    """How many things the indices, targets and subset of the scan number: the index's items, or the item pooling's sets."""
    return index.num_items if self.item_pooling is None else self.item_pooling.num_sets

  def candidates(self, index):
    """The bound of k': the allowed ones among them."""
    return self.numbered(index) if self.subset is None else self.subset.count

  def columns(self, index):
    """The gallery columns the chunk estimates of the batches count."""
    return index.num_items if self.item_pooling is None else self.item_pooling._columns

  def scored(self):
    """What a threshold pass takes of it: how a pair is scored, not which items are candidates."""
    return _Scan(norm=self.norm, pooling=self.pooling, item_pooling=self.item_pooling)

  def shard(self, s, index):
    """Shard s's view of it on the ShardedVideoIndex `index`: its part of the subset, the norm and the item pooling (None
    where the shard has none), the pooling as it is, the exclusions in the shard's item numbers on its device, and the
    cursor with `first` in the shard's numbers: the count of its items numbered at or below the cursor's item
    (ShardedVideoIndex._first), which restates the global tie rule locally, and the filter as the shard's part of the
    tagging with the masks on its device."""
    part = lambda whole: None if whole is None else whole.parts[s]
    device = index.shards[s].device
    ex = None if self.ex is None else index._local(self.ex, s).to(device)
    after = None if self.after is None else (self.after[0].to(device), index._first(self.after[1], s).to(device))
    where = None if self.where is None else TagFilter(self.where.masks.to(device), self.where.tagging.parts[s],
                                                      self.where.num_rows)
    return _Scan(part(self.subset), ex, part(self.norm), self.pooling, part(self.item_pooling), after, self.stream, where)


def _column_groups(src, outs, r0, r1):
  """Rows r0 .. r1 - 1 of src [NQ, T] and of every tensor of outs, in column groups of at most MAX_T (the launches' limit):
  yields (the src slice, the out slices), all contiguous.  A column slice of a wider list is not contiguous: it is copied
  in, and the outs are copied back when the caller asks for the next group."""
  t_all = src.shape[1]
  for t0 in range(0, t_all, MAX_T):
    t1 = min(t_all, t0 + MAX_T)
    whole = t1 - t0 == t_all
    parts = [o[r0:r1] if whole else torch.empty(r1 - r0, t1 - t0, device=o.device, dtype=o.dtype) for o in outs]
    yield src[r0:r1] if whole else src[r0:r1, t0:t1].contiguous(), parts
    if not whole:
      for o, part in zip(outs, parts):
        o[r0:r1, t0:t1] = part


def _lists(count, device, *shape, vacant=False):
  """`count` result lists of `shape`: float32 scores, then int64 numbers -- unwritten, or (vacant) holding (-inf, -1), a
  slot without a candidate."""
  if vacant:
    return tuple([torch.full(shape, float('-inf'), device=device, dtype=torch.float32)] +
                 [torch.full(shape, -1, device=device, dtype=torch.int64) for _ in range(count - 1)])
  return tuple([torch.empty(*shape, device=device, dtype=torch.float32)] +
               [torch.empty(*shape, device=device, dtype=torch.int64) for _ in range(count - 1)])


class _Index:
  """What VideoIndex and ShardedVideoIndex share: the checks of every public call, the calls that are the same on both
  (`search`, `rank_counts`, `ranks`, `hub_norm` up to the scan, `search_groups`) and QB-Norm's dynamic rule.  It reads the
  bookkeeping both have -- num_experts, dim, num_items, device (the primary of a sharded index).  Behind its checks a
  public call puts its options into one _Scan and makes one call with it, wrapped in `_dynamic`; the class supplies
  what happens there -- _search(q, qw, k, scan), _rank_counts(q, qw, tg, scan), _hub_norm, _search_groups, and
  _rescore(q, qw, cand, k) for `rescore`, which takes no scan options -- and names
  its own kinds of subset, norm and grouping for `_made_here` (_subset / _norm / _grouping)."""

  @staticmethod
  def _items(embds, weights, who):
    g = _cuda_f32(embds, 'embds')
    gw = _cuda_f32(weights, 'weights')
    if g.dim() != 3 or gw.shape != g.shape[:2]:
      raise ValueError('%s expects embds (NV, M, d) and weights (NV, M), got %s and %s' % (
          who, tuple(g.shape), tuple(gw.shape)))
    if g.shape[0] < 1:
      raise ValueError('%s: need NV >= 1, got %s' % (who, tuple(g.shape)))
    return g, gw

  def _queries(self, embds, weights):
    q = _cuda_f32(embds, 'embds')
    qw = _cuda_f32(weights, 'weights')
    m, d = self.num_experts, self.dim
    if q.dim() == 4:  # CENet text layout (B, M, C, d) / (B, C, M) -> rows b*C + c, as metric.eval_similarity
      b, qm, c, qd = q.shape
      if (qm, qd) != (m, d) or tuple(qw.shape) != (b, c, m):
        raise ValueError('search: text embds (B, %d, C, %d) with weights (B, C, %d) expected, got %s and %s' % (
            m, d, m, tuple(q.shape), tuple(qw.shape)))
      q = q.permute(0, 2, 1, 3).reshape(b * c, m, d).contiguous()
      qw = qw.reshape(b * c, m).contiguous()
    elif q.dim() != 3 or tuple(q.shape[1:]) != (m, d) or tuple(qw.shape) != (q.shape[0], m):
      raise ValueError('search: embds (NQ, %d, %d) with weights (NQ, %d) expected, got %s and %s' % (
          m, d, m, tuple(q.shape), tuple(qw.shape)))
    if q.device != self.device or qw.device != self.device:
      raise ValueError('search: queries must be on the index device %s' % self.device)
    return q, qw

  def _no_fp8(self, who, what):
    """What an fp8 index does not answer yet is refused by name, before anything is scored."""
    if getattr(self, 'dtype', None) == FP8:
      raise ValueError('%s: %s is not available on a %s index' % (who, what, FP8))

  def _made_here(self, thing, who, noun, kind, maker, item_pooling=None):
    """`thing` (a `noun`: subset, norm or grouping) was built by this index -- it is a `kind`, which `maker` returns --
    for this many items (a subset beside an item pooling: for its sets) and on this device; a sharded kind (it has
    `parts`) also for this many shards."""
    if not isinstance(thing, kind):
      raise ValueError('%s: %s must come from %s, got %s' % (who, noun, maker, type(thing).__name__))
    if item_pooling is not None:
      if thing.num_items != item_pooling.num_sets:
        raise ValueError('%s: the %s was built for %d sets, the item pooling has %d' % (
            who, noun, thing.num_items, item_pooling.num_sets))
    elif thing.num_items != self.num_items:
      raise ValueError('%s: the %s was built for %d items, the index holds %d' % (who, noun, thing.num_items, self.num_items))
    if not hasattr(thing, 'parts'):
      if thing.device != self.device:
        raise ValueError('%s: the %s is on %s, the index on %s' % (who, noun, thing.device, self.device))
    elif thing.device != self.device or len(thing.parts) != len(self.shards):
      raise ValueError('%s: the %s belongs to another index' % (who, noun))

  def _subset_mask(self, items):
    """The checks of `subset` -> (the set as a bool mask [num_items] of its own, the number of allowed items)."""
    if self.num_items == 0:
      raise ValueError('subset: the index holds no items')
    return _mask_of(items, self.num_items, self.device)

  def _exclude(self, exclude):
    """Type, device and width of `exclude`: all that can be said about it before the queries are known."""
    if not torch.is_tensor(exclude) or exclude.dtype != torch.int64:
      raise ValueError('search: exclude must be an int64 tensor, got %s' % (
          exclude.dtype if torch.is_tensor(exclude) else type(exclude).__name__))
    if exclude.dim() not in (1, 2) or exclude.dim() == 2 and not 1 <= exclude.shape[1] <= MAX_E:
      raise ValueError('search: exclude [NQ] or [NQ, 1 <= E <= %d] expected, got %s' % (MAX_E, tuple(exclude.shape)))
    if exclude.device != self.device:
      raise ValueError('search: exclude must be on the index device %s, got %s' % (self.device, exclude.device))

  def _targets(self, targets):
    """Type, device and rank of `targets`: all that can be said about them before the queries are known."""
    if not torch.is_tensor(targets) or targets.dtype != torch.int64:
      raise ValueError('ranks: targets must be an int64 tensor, got %s' % (
          targets.dtype if torch.is_tensor(targets) else type(targets).__name__))
    if targets.device != self.device:
      raise ValueError('ranks: targets must be on the index device %s, got %s' % (self.device, targets.device))
    if targets.dim() not in (1, 2) or targets.dim() == 2 and targets.shape[1] < 1:
      raise ValueError('ranks: targets [NQ] or [NQ, T >= 1] expected, got %s' % (tuple(targets.shape),))

  def _target_range(self, targets, scan):
    """The values of the (non-empty) targets against -1 .. num_items - 1 (with an item pooling: num_sets - 1): one small
    reduction and a host sync."""
    n = scan.numbered(self)
    lo, hi = (int(v) for v in torch.aminmax(targets))
    if lo < -1 or hi >= n:
      raise ValueError('ranks: targets must lie in -1 .. %d, got %d .. %d' % (n - 1, lo, hi))

  def _tags(self, tags):
    """The checks of `tagging` -> the tags as int64 [num_items] of their own."""
    if self.num_items == 0:
      raise ValueError('tagging: the index holds no items')
    if not torch.is_tensor(tags) or tags.dtype != torch.int64:
      raise ValueError('tagging: tags must be an int64 tensor, got %s' % (
          tags.dtype if torch.is_tensor(tags) else type(tags).__name__))
    if tags.device != self.device:
      raise ValueError('tagging: tags must be on the index device %s, got %s' % (self.device, tags.device))
    if tuple(tags.shape) != (self.num_items,):
      raise ValueError('tagging: tags of shape (%d,) expected, got %s' % (self.num_items, tuple(tags.shape)))
    return tags.contiguous().clone()

  def _where(self, where, who, norm=None, pooling=None, item_pooling=None):
    """Type and age of `where`, and what it does not combine with: all that can be said before the queries are known."""
    for name, given in (('norm', norm), ('pooling', pooling), ('item_pooling', item_pooling)):
      if given is not None:
        raise ValueError('%s: where= does not combine with %s=' % (who, name))
    if not isinstance(where, TagFilter):
      raise ValueError('%s: where must come from the where() of a tagging, got %s' % (who, type(where).__name__))
    self._made_here(where.tagging, who, 'tagging', self._tagging_type, '%s.tagging' % type(self).__name__)

  @staticmethod
  def _where_rows(where, who, nq):
    """The filter's row count against the call's query rows."""
    if where is not None and where.num_rows is not None and where.num_rows != nq:
      raise ValueError('%s: %d query rows but the where= filter holds %d rows' % (who, nq, where.num_rows))

  @staticmethod
  def _no_where(who, where):
    """The calls that take no filter say so by name, before anything is scored."""
    if where is not None:
      raise ValueError('%s: where= is out of scope: this call takes no per-query filter' % who)

  def pooling(self, set_size, num_sets, row_weights=None, mode='mean'):
    """The query sets of a pooled scan -> QueryPooling, built once like a subset and passed as pooling= to `search`,
    `rank_counts`, `ranks`, `target_scores` and `threshold_counts`: the queries of such a call are num_sets * set_size rows,
    set s is rows s * set_size .. s * set_size + set_size - 1 (1 <= set_size <= MAX_SET = 64), and the call answers per SET.
    row_weights: float32 [num_sets * set_size] or [num_sets, set_size] on the index device, finite; a row whose weight
    is 0 takes no part (a padded caption), and every set needs a row that does.  None = float32(1 / set_size) on every
    row, the reference's 'avg' (model/model.py:826-831).  mode='mean': the weighted sum over the participating rows in
    row order, each product and each sum rounded to fp32 on its own; mode='max': the largest score, the weights acting
    as a mask only.  The checks cost one small reduction and one host sync.  A pooling does not describe the stored
    items: it stays valid after `add`."""
    def count():
      if num_sets < 0 or num_sets * set_size >= 2 ** 31:
        raise ValueError('pooling: num_sets must be >= 0 with num_sets * set_size < 2^31, got %d' % num_sets)
      return num_sets
    _, w = _check_sets('pooling', 'a row', (('set_size', set_size), ('num_sets', num_sets)), MAX_SET, count, True, mode,
                       row_weights, self.device)
    return QueryPooling(set_size, num_sets, w, mode)

  def _pooling(self, pooling, who, exclude=None, norm=None):
    """Type and device of `pooling`, and what it does not combine with: all that can be said before the queries are known."""
    if not isinstance(pooling, QueryPooling):
      raise ValueError('%s: pooling must come from pooling(), got %s' % (who, type(pooling).__name__))
    if pooling.device != self.device:
      raise ValueError('%s: the pooling is on %s, the index on %s' % (who, pooling.device, self.device))
    if exclude is not None or norm is not None:
      raise ValueError('%s: pooling= does not combine with exclude= or norm=' % who)

  def _item_pooling(self, item_pooling, who, pooling=None, exclude=None, norm=None):
    """Type, device and age of `item_pooling`, and what it does not combine with."""
    if not isinstance(item_pooling, self._item_pooling_type):
      raise ValueError('%s: item_pooling must come from item_pooling(), got %s' % (who, type(item_pooling).__name__))
    if item_pooling.device != self.device:
      raise ValueError('%s: the item pooling is on %s, the index on %s' % (who, item_pooling.device, self.device))
    if item_pooling.num_items != self.num_items:
      raise ValueError('%s: the item pooling was built for %d items, the index holds %d' % (
          who, item_pooling.num_items, self.num_items))
    if pooling is not None or exclude is not None or norm is not None:
      raise ValueError('%s: item_pooling= does not combine with pooling=, exclude= or norm=' % who)

  def _scan_args(self, who, embds, weights, norm, dynamic, subset=None, exclude=None, pooling=None, item_pooling=None,
                 where=None):
    """The checks every scan shares once its own arguments have passed -> q, qw, whether the dynamic rule applies.  With
    a pooling the query count must be its num_rows: nothing is scored otherwise.  With an item pooling the subset is one
    of its sets."""
    if where is not None:
      self._where(where, who, norm, pooling, item_pooling)
    for what, given in (('item_pooling=', item_pooling), ('pooling=', pooling), ('norm=', norm)):
      if given is not None:
        self._no_fp8(who, what)
    if item_pooling is not None:
      self._item_pooling(item_pooling, who, pooling, exclude, norm)
    if pooling is not None:
      self._pooling(pooling, who, exclude, norm)
    if subset is not None:
      self._subset(subset, who, item_pooling)
    if exclude is not None:
      self._exclude(exclude)
    if norm is not None:
      self._norm(norm, who)
    dynamic = _check_dynamic(dynamic, norm, who)
    q, qw = self._queries(embds, weights)
    if pooling is not None and q.shape[0] != pooling.num_rows:
      raise ValueError('%s: %d queries but the pooling has %d rows (%d sets of %d)' % (
          who, q.shape[0], pooling.num_rows, pooling.num_sets, pooling.set_size))
    self._where_rows(where, who, q.shape[0])
    return q, qw, dynamic

  def _use_norm(self, q, qw, scan):
    """QB-Norm's dynamic rule: bool [NQ], True where the query's plain top-1 among its candidates (after subset and
    exclusions) is one of the norm's hubs.  A query without a candidate keeps its plain result.  A cursor plays no part:
    the decision belongs to the query, not to the page."""
    top1 = self._search(q, qw, 1, scan.uncursored())[1][:, 0]
    return (top1 >= 0) & scan.norm.hubs[top1.clamp(min=0)]

  def _dynamic(self, dynamic, q, qw, scan, run, use=None):
    """The result of a public call: run(scan), a tuple of tensors -- with a norm every query normalised -- as it is, or
    under the dynamic rule (which takes a norm) mixed per query with what run gives without the norm.  use: `_use_norm`
    of the scan where the caller has it already (the pages of `search_deep`)."""
    out = run(scan)
    if not dynamic or q.shape[0] == 0:
      return out
    if use is None:
      use = self._use_norm(q, qw, scan)
    return tuple(_pick(use, a, b) for a, b in zip(out, run(scan.plain())))

  def hub_norm(self, bank_embds, bank_weights, beta, dynamic=False):
    """The querybank normaliser of this index (inverted softmax, the static half of QB-Norm): bank queries in either layout
    of `search`, NB >= 1 of them, and a temperature beta (a Python float, 0 < beta < inf) -> HubNorm (ShardedVideoIndex:
    ShardedHubNorm) with lse[g] = log sum_b exp(fl(beta * score(b, g))) per stored item, in fp32 (mmt_search_col_lse).
    Passed as norm= to `search`, `rank_counts`, `ranks`, `target_scores` and `threshold_counts` it replaces score(q, g) by
    score'(q, g) = fl(fl(beta * score(q, g)) - lse[g]), the log of the inverted-softmax probability.  The bank streams
    through in batches within _BATCH_BYTES; lse[g] does not depend on the batching, on num_items, on g's position or on the
    shard that holds g.  dynamic=True also records `hubs`, the items that are the plain top-1 of a bank query (one
    search(k=1) of the bank): a call with such a norm then normalises only the queries whose own plain top-1 is a hub
    (QB-Norm's dynamic inverted softmax).  Like a subset, a norm describes the num_items of this moment: after a further
    `add` it is refused."""
    self._no_fp8('hub_norm', 'the querybank normalisation')
    _check_beta(beta)
    if not isinstance(dynamic, bool):
      raise ValueError('hub_norm: dynamic must be False or True, got %r' % (dynamic,))
    if self.num_items == 0:
      raise ValueError('hub_norm: the index holds no items')
    b, bw = self._queries(bank_embds, bank_weights)
    if b.shape[0] < 1:
      raise ValueError('hub_norm: the bank holds no queries')
    return self._hub_norm(b, bw, beta, self._bank_hubs(b, bw, dynamic))

  def _bank_hubs(self, b, bw, dynamic):
    """`hubs` of a norm built with dynamic=True: the items that are the plain top-1 of a bank query; else None."""
    if not dynamic:
      return None
    top1 = self._search(b, bw, 1, _Scan())[1][:, 0]
    return torch.zeros(self.num_items, device=self.device, dtype=torch.bool).index_fill_(0, top1, True)

  def reverse_search(self, embds, weights, k=10, where=None):
    """The search run the other way: queries in either layout of `search` (the text layout numbers its rows b * C + c),
    NQ >= 1 of them -> (scores float32 [num_items, k'], rows int64 [num_items, k']) on the device, k' = min(k, NQ), k an
    int in 1 .. MAX_RK = 32: for every stored item the k' query rows that score best on it, best first, equal scores
    (-0 tied with +0) by ascending row.  A score has the bits `search` returns for the pair on this index, whatever its
    dtype (all three are supported), so a -0 comes back as +0.  The rows stream through in batches of whole 64-row blocks
    within _BATCH_BYTES and a running list per item is carried between them (mmt_search_col_topk): no NQ x num_items
    matrix, and the result does not depend on the batching, on num_items, on an item's position or on the shard that
    holds it -- ShardedVideoIndex.reverse_search (every shard takes all the rows and answers for its own items) is
    bit-identical.  It takes no options: subset=, exclude=, norm= and the poolings are not part of this call."""
    self._no_where('reverse_search', where)
    _check_rk('reverse_search', k)
    if self.num_items == 0:
      raise ValueError('reverse_search: the index holds no items')
    q, qw = self._queries(embds, weights)
    if q.shape[0] < 1:
      raise ValueError('reverse_search: need NQ >= 1 query rows, got %s' % (tuple(q.shape),))
    return self._reverse_search(q, qw, min(k, q.shape[0]))

  def csls_norm(self, bank_embds, bank_weights, k=10, dynamic=False):
    """The CSLS normaliser of this index (Cross-domain Similarity Local Scaling, Conneau et al., ICLR 2018; the other bank
    normaliser of QB-Norm): bank queries in either layout of `search`, NB >= 1 of them, and k, an int in 1 .. MAX_RK ->
    HubNorm (ShardedVideoIndex: ShardedHubNorm) with kind='csls', k=k, beta=2.0 and, in `lse`, r[g] = the mean of item
    g's k' = min(k, NB) best bank scores: with s_0 .. s_{k'-1} the scores `reverse_search(bank, k)` lists for the item, in
    list order, v = s_0, v = fl(v + s_i), r[g] = fl(v * float32(1 / k')) (mmt_search_col_topk).  CSLS ranks a query's
    items by 2 score(q, g) - r_q - r[g]; the query's own term r_q is constant within its row, so ranking by
    fl(fl(2 * score(q, g)) - r[g]) is ranking by CSLS, and that is the norm slot as it is: passed as norm= to `search`,
    `rank_counts`, `ranks`, `target_scores` and `threshold_counts` -- with subset=, exclude=, after= and the dynamic rule
    -- it needs no kernel of its own.  r[g] does not depend on the batching, on num_items, on g's position or on the
    shard.  dynamic=True records `hubs` as `hub_norm` does.  Like `hub_norm` it is refused on a float8_e4m3fn index,
    because norm= is."""
    self._no_fp8('csls_norm', 'the querybank normalisation')
    _check_rk('csls_norm', k)
    if not isinstance(dynamic, bool):
      raise ValueError('csls_norm: dynamic must be False or True, got %r' % (dynamic,))
    if self.num_items == 0:
      raise ValueError('csls_norm: the index holds no items')
    b, bw = self._queries(bank_embds, bank_weights)
    if b.shape[0] < 1:
      raise ValueError('csls_norm: the bank holds no queries')
    return self._csls_norm(b, bw, k, self._bank_hubs(b, bw, dynamic))

  def _lse_args(self, who, beta, subset, unsupported):
    """The checks of `query_lse` and `search_softmax` that look at no value, before anything touches the device."""
    for name in unsupported:
      if name not in _NOT_LSE:
        raise TypeError('%s() got an unexpected keyword argument %r' % (who, name))
      raise ValueError('%s: %s= is out of scope: the softmax runs over the plain scores of a subset' % (who, name))
    _check_beta(beta, who)
    if self.num_items == 0:
      raise ValueError('%s: the index holds no items' % who)
    if subset is not None:
      self._subset(subset, who)

  def query_lse(self, embds, weights, beta, subset=None, **unsupported):
    """The twelfth question: what a score is worth.  Queries in either layout of `search`, beta a Python float with
    0 < beta < inf, subset from this index's `subset` -> QueryLse: per query the log-partition of
    softmax(beta * score(q, .)) over its candidates (every stored item, or the subset's), without the NQ x NV matrix.
    All in fp32 unless stated, with s(q, g) the bits `search` gives the pair on this index (any of the three dtypes):
        x(q, g) = fl(beta * s(q, g))                     a rounded multiply
        xmax[q] = the largest x(q, g) = fl(beta * top-1 score): fl(beta * .) is monotone; from search(k=1, subset=)
        e(q, g) = expf(x(q, g) - xmax[q])                in [0, 1]; the top-1 item gives exactly 1
        t(q, g) = (int64) rint(ldexp(e(q, g), F))        F = lse_bits(num_items) = 62 - ceil(log2(max(num_items, 2)))
        T[q]    = sum_g t(q, g)                          an int64 sum: t <= 2^F, num_items <= 2^(62 - F), so T <= 2^62
        lse[q]  = float32(float64(xmax[q]) + log(float64(T[q])) - F ln 2)      torch float64 ops (lse_from_sums)
    An integer sum is associative, so T[q] -- and with it lse[q] -- is ONE number whatever the chunking, the row batching,
    the launch geometry, the order of the items or the shard: a function of the query and the set of candidates only, the
    rule every other call here keeps and no floating-point sum over 262 144 items can.  The price is the quantisation of
    a term, at most half a unit: at most num_items * 2^-(F + 1) relative on T (T >= 2^F: the top-1 term), which is at most
    2^(2c - 63) for num_items <= 2^c -- 2^-25 at 2^19 items, below half an fp32 ulp; 2^-15 at 2^24.  Two scans: the
    top-1 (`search`), then the sum (mmt_search_row_expsum: the scans' own score tile with the selection replaced by the
    sum; a tile without an allowed item is skipped before its K loop).  Rows go in batches of whole 64-row blocks within
    _BATCH_BYTES.  ShardedVideoIndex.query_lse takes xmax from the merged top-1 and F from the global num_items, every
    shard sums over its own items with its part of the subset, and the int64 partials are added on the primary:
    bit-identical to one VideoIndex over the same items, in `.sums` and `.lse` alike.  Out of scope: exclude=, norm=,
    pooling=, item_pooling=, after= and grouping= raise ValueError naming the option."""
    self._lse_args('query_lse', beta, subset, unsupported)
    q, qw = self._queries(embds, weights)
    return self._query_lse(q, qw, beta, subset)

  def _query_lse(self, q, qw, beta, subset, top=None):
    """`query_lse` behind its checks.  top: the (scores [NQ, >= 1], indices) of a `search` over the same candidates that the
    caller has already (search_softmax), whose first column is the top-1."""
    scan = _Scan(subset)
    if top is None:
      top = self._search(q, qw, 1, scan)
    bits = lse_bits(self.num_items)
    with torch.cuda.device(self.device):
      top_scores, top_items = top[0][:, 0].contiguous(), top[1][:, 0].contiguous()
      xmax = top_scores * torch.tensor(beta, device=self.device, dtype=torch.float32)
      sums = self._row_expsum(q, qw, beta, xmax, bits, scan)
      lse = lse_from_sums(xmax, sums, bits)
    return QueryLse(lse, beta, top_scores, top_items, sums, bits, self.num_items, scan.candidates(self))

  def search_softmax(self, embds, weights, k=10, beta=None, subset=None, **unsupported):
    """`search` with the probabilities: queries, k and subset as there, beta as `query_lse` -> (scores [NQ, k'] float32,
    indices [NQ, k'] int64, log_probs [NQ, k'] float32): `search`'s lists, bit for bit, and for every slot
    fl(fl(beta * score) - lse[q]), the log of the item's share of softmax(beta * score(q, .)) over the candidates; a vacant
    slot gets -inf.  Host code: `search`, then `query_lse` fed the top-1 that search has found already -- two scans, not
    three -- then QueryLse.log_prob."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('search_softmax: k must be an int in 1..%d, got %r' % (MAX_K, k))
    self._lse_args('search_softmax', beta, subset, unsupported)
    q, qw = self._queries(embds, weights)
    scores, indices = self._search(q, qw, k, _Scan(subset))
    return scores, indices, self._query_lse(q, qw, beta, subset, (scores, indices)).log_prob(scores)

  def _after(self, after, pooling=None, item_pooling=None):
    """Type, device and rank of `after`, and what it does not combine with: all that can be said before the queries are
    known."""
    if pooling is not None or item_pooling is not None:
      raise ValueError('search: after= does not combine with pooling= or item_pooling=')
    if (not isinstance(after, (tuple, list)) or len(after) != 2 or not all(torch.is_tensor(t) for t in after) or
        after[0].dtype != torch.float32 or after[1].dtype != torch.int64):
      raise ValueError('search: after must be None or a pair (scores float32 [NQ], items int64 [NQ]), got %s' % (
          '(%s)' % ', '.join(str(t.dtype) if torch.is_tensor(t) else type(t).__name__ for t in after)
          if isinstance(after, (tuple, list)) else type(after).__name__))
    for t in after:
      if t.device != self.device:
        raise ValueError('search: after must be on the index device %s, got %s' % (self.device, t.device))
    if after[0].dim() != 1 or after[0].shape != after[1].shape:
      raise ValueError('search: after (scores [NQ], items [NQ]) expected, got %s and %s' % (
          tuple(after[0].shape), tuple(after[1].shape)))

  _schedule = None   # a class default: an index made without a constructor call has the tile schedule too

  @property
  def schedule(self):
    """Which schedule `search` gives its plain top-k pass: None or 'tile' -- the launches tuned for thousands of queries,
    what every call has always taken -- or 'stream', the schedule for a handful of queries (`search`'s docstring; DESIGN
    9.21).  A setting of the index, not an argument of the call: a service sets it once on the index it serves from.
    It is plain state on a shared object: setting it is not synchronised with calls in flight on other threads, so a
    process that serves online queries and runs evaluation batches from the same stored items at the same time should
    not toggle it between calls -- the stored tensors are shared by a second index object made for the other schedule.
    Assigning anything else is a ValueError, and the index keeps what it had."""
    return self._schedule

  @schedule.setter
  def schedule(self, value):
    if value is not None and (not isinstance(value, str) or value not in ('tile', 'stream')):
      raise ValueError("schedule must be None, 'tile' or 'stream', got %r" % (value,))
    self._schedule = value

  def _streams(self, who, norm, dynamic, pooling, item_pooling):
    """Whether a `search` with these options takes the streaming schedule: it has no kernels for the querybank
    normalisation or for sets, and an index set to it says so by the argument's name instead of answering on the other
    schedule."""
    if self._schedule != 'stream':
      return False
    for name, given in (('norm', norm), ('dynamic', dynamic), ('pooling', pooling), ('item_pooling', item_pooling)):
      if given is not None:
        raise ValueError("%s: the index's schedule 'stream' does not combine with %s=" % (who, name))
    return True

  def _search_filtered(self, embds, weights, k=10, subset=None, exclude=None, norm=None, dynamic=None, pooling=None,
                       item_pooling=None, after=None, where=None):
    """Queries (NQ, M, d) / (NQ, M), or the text layout (B, M, C, d) / (B, C, M) -> (scores [NQ, k'] float32,
    indices [NQ, k'] int64) on the device, k' = min(k, NV), best first.  subset (from this index's `subset`): only its
    items are candidates and k' = min(k, subset.count).  exclude: int64 [NQ] or [NQ, E <= 32] on the index device, values
    -1 .. num_items - 1 (-1 = none; duplicates and items outside the subset are fine): items barred for that query; its
    range is checked as that of `rank_counts`' targets, before anything is scored.  A query with fewer than k' candidates
    left gets score -inf and index -1 in the remaining slots.  norm (from this index's `hub_norm`): the ranking and the
    returned scores are those of score' (mmt_search_topk [lse]); with a norm that has `hubs`, only the queries whose plain
    top-1 candidate is a hub are normalised and the others keep their plain result (dynamic=False normalises every query).
    pooling (from `pooling`): the queries are pooling.num_sets sets of pooling.set_size rows and the outputs have one row
    per SET: the k' best items by the set's pooled score (module docstring; mmt_search_topk [query sets]), ranked and tied as
    above; a returned score is the pooled value with -0 as +0.  pooling= does not combine with exclude= or norm=.
    item_pooling (from `item_pooling`): the STORED items are sets and the indices are set numbers: per query the k' best
    sets by the set's pooled score (mmt_search_topk [item sets]), k' = min(k, num_sets) or min(k, subset.count) with a subset
    from item_pooling.subset; does not combine with pooling=, exclude= or norm=.
    ShardedVideoIndex: every shard searches its own items for its best min(k', its candidates), with its part of the
    subset and the norm; the lists are copied to the primary and merged there in one launch.  With a pooling every shard
    sees all query rows, so a pooled score has the same bits wherever the item is stored.
    after: None, or a cursor (a_scores float32 [NQ], a_items int64 [NQ]) on the index device (the primary of a sharded
    index): the k' best items that come AFTER a position in this call's own order -- page 2 of a list is
    search(..., after=(scores[:, -1], indices[:, -1])) of page 1, with every other argument the same.  Row q with
    a_items[q] >= 0 is a position: the candidates are the items g with score(q, g) < a_scores[q], or score(q, g) ==
    a_scores[q] and g > a_items[q] (-0 compares as +0, as in the order itself; with norm= the scores compared are score',
    the values the call returns).  The position need not be that of a stored or allowed item: a_scores[q] is any float
    but NaN, a_items[q] any number in 0 .. num_items - 1.  (+inf, -1) is "no cursor": the row is what the call returns
    without after.  (-inf, -1) is "exhausted": the row has no candidates -- it is the vacant slot of an earlier page, so
    the last column of a page is always a valid cursor and a row that came back short gets nothing more.  Anything else
    (-1 with a finite score, a NaN, an item out of range) is a ValueError naming `after`, raised before anything is
    scored: one small reduction and one host sync, shared with the check of `exclude` where both are given; type, device
    and shape are checked before the queries are looked at.  The shape stays [NQ, k'] with k' as without a cursor, and a
    row with fewer than k' items left holds (-inf, -1) in the remaining slots.  A score has the bits the call without
    `after` gives the pair, and for every k and cursor the row is the slice that starts right behind the position in the
    complete ordered list of the query's candidates -- whatever the row batching, the launch geometry or the shards (the
    cursor is one more compare at selection time, on the keys the scan orders by: mmt_search_topk [after]).  Combines
    with subset=, exclude=, norm= and dynamic=; under the dynamic rule a query's plain top-1 is taken WITHOUT the cursor,
    so the choice is the same on every page.  after= with pooling= or item_pooling= is a ValueError; `search_groups` has
    no cursor (a group's representative may lie before a position while other members lie after it).  after=None takes
    exactly the calls above.
    The index's `schedule` (a property; None at first): None or 'tile' take exactly the calls above.  With
    index.schedule = 'stream' this call sends the top-k pass through the streaming schedule
    (mmt_search_topk_stream), built for a handful of queries -- a service answering one caption, or a few: it is MEANT FOR
    NQ <= 32, where the scan is a matter of reading the gallery once, and takes any NQ, the rows going through in tiles of
    32.  The results are `search`'s TO THE BIT, scores and indices, on all three storages: a pair's accumulator goes
    through the same instruction sequence and the same epilogue expression, keys and running top-k are shared, and the
    merge is by rank as well (measured over 262 144 items, k = 10: faster than 'tile' at every NQ from 1 to 64).
    Combines with subset=, exclude= and after=; with norm= (and so dynamic=), pooling= or item_pooling= it is a ValueError
    naming the argument, raised before anything is scored (any other value of the property is refused when it is
    assigned).  It is the schedule of THIS call alone (and of the coarse search of `search_refined`): `search_deep`, `search_groups`,
    the shortlist search of `search_diverse` and the searches inside `hub_norm`,
    `query_lse` and their kin keep the tile schedule.  ShardedVideoIndex: the property of the sharded index decides and
    every shard takes it; the shard merge is the same.
    where (a TagFilter from the `where` of this index's `tagging`): the per-query attribute filter -- item g is a candidate
    of row q only if its tag word passes the row's three masks (module docstring; `tag_pass`), ANDed with subset=,
    exclude= and after=.  Shapes as with exclude=: k' = min(k, the candidates after subset), and a row with fewer passing
    candidates ends in (-inf, -1).  A score has the bits the call without where= gives the pair; both schedules take it
    (mmt_search_topk_where, mmt_search_topk_stream_where) and give the same bits.  A filter whose row count is not this
    call's, or from another index's tagging, and where= with norm=, pooling= or item_pooling= are ValueErrors raised before
    anything is scored.  where=None takes exactly the calls above."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('search: k must be an int in 1..%d, got %r' % (MAX_K, k))
    return self._search_call(self._streams('search', norm, dynamic, pooling, item_pooling), embds, weights, k, subset,
                             exclude, norm, dynamic, pooling, item_pooling, after, where)

  @_where_option(_search_filtered)
  def search(self, embds, weights, k=10, subset=None, exclude=None, norm=None, dynamic=None, pooling=None,
             item_pooling=None, after=None):
    return self._search_filtered(embds, weights, k, subset, exclude, norm, dynamic, pooling, item_pooling, after)

  def _search_call(self, stream, embds, weights, k=10, subset=None, exclude=None, norm=None, dynamic=None, pooling=None,
                   item_pooling=None, after=None, where=None):
    """`search` behind its check of k and of the schedule: stream = whether the top-k pass takes the streaming schedule.
    Host code that builds on `search` without taking part in the schedule (`search_diverse`) calls this with False."""
    if self.num_items == 0:
      raise ValueError('search: the index holds no items')
    if after is not None:
      self._after(after, pooling, item_pooling)
    q, qw, dynamic = self._scan_args('search', embds, weights, norm, dynamic, subset, exclude, pooling, item_pooling,
                                     where)
    ex, cursor = _limits(exclude, after, q.shape[0], self.num_items)
    scan = _Scan(subset, ex, norm, pooling, item_pooling, cursor, stream, where)
    return self._dynamic(dynamic, q, qw, scan, lambda scan: self._search(q, qw, k, scan))

  def _search_deep_filtered(self, embds, weights, depth, page=DEEP_PAGE, subset=None, exclude=None, norm=None,
                            dynamic=None, where=None):
    """The sorted list deeper than MAX_K: queries, subset, exclude, norm, dynamic and where as for `search`; depth an int >= 1, page
    an int in 1 .. MAX_K -> (scores [NQ, w] float32, indices [NQ, w] int64), w = min(depth, the candidates after subset):
    column for column the complete ordered candidate list of each query, cut at w, a row with fewer candidates left
    (exclusions) ending in (-inf, -1).  Host code: the concatenation of ceil(w / page) pages, each a search(k = min(page,
    what is left), after = the last column of the page before); the arguments are checked once and under the dynamic rule
    the per-query choice is taken once.  The number of pages is known on the host and nothing waits for the device
    between them, so there is no early stop.  A page costs one scan of the gallery and a wide page costs more than a
    narrow one, so `page` trades the number of scans against the cost of each: the default, DEEP_PAGE = 64, is the width
    at which a scan cost least per column where it was measured (depth 256 took 404 ms at page 64, 568 ms at
    32 and 625 ms at 128 on a bf16 index of 262 144 items with 4 096 queries)."""
    if isinstance(depth, bool) or not isinstance(depth, int) or depth < 1:
      raise ValueError('search_deep: depth must be an int >= 1, got %r' % (depth,))
    if isinstance(page, bool) or not isinstance(page, int) or not 1 <= page <= MAX_K:
      raise ValueError('search_deep: page must be an int in 1..%d, got %r' % (MAX_K, page))
    if self.num_items == 0:
      raise ValueError('search: the index holds no items')
    q, qw, dynamic = self._scan_args('search', embds, weights, norm, dynamic, subset, exclude, where=where)
    scan = _Scan(subset, _limits(exclude, None, q.shape[0], self.num_items)[0], norm, where=where)
    width = min(depth, scan.candidates(self))
    use = self._use_norm(q, qw, scan) if dynamic and q.shape[0] else None
    pages, cursor = [], None
    for c0 in range(0, width, page):
      k = min(page, width - c0)
      pages.append(self._dynamic(dynamic, q, qw, scan.at(cursor), lambda scan: self._search(q, qw, k, scan), use))
      scores, items = (t[:, -1] for t in pages[-1])
      cursor = (scores, torch.where(items >= 0, items + 1, items))   # a vacant slot (-inf, -1) is "exhausted" as it is
    return tuple(torch.cat(parts, 1) for parts in zip(*pages))

  @_where_option(_search_deep_filtered)
  def search_deep(self, embds, weights, depth, page=DEEP_PAGE, subset=None, exclude=None, norm=None, dynamic=None):
    return self._search_deep_filtered(embds, weights, depth, page, subset, exclude, norm, dynamic)

  def rank_counts(self, embds, weights, targets, subset=None, norm=None, dynamic=None, pooling=None, item_pooling=None,
                  where=None):
    """Queries as for `search`; targets [NQ] or [NQ, T] int64 on the index device, values -1 .. num_items - 1 ->
    (greater, equal), int32 of targets' shape: how many of the num_items stored items score above / exactly equal to item
    targets[q, t] for query q (the item itself is one of the equal ones); 0 / 0 where the target is -1.  The range of the
    targets is checked here (one small reduction and a host sync); nothing is scored before it passes.  subset: only its
    items are counted; a target outside it is still scored but does not count itself, so its `equal` may be 0.  norm: the
    counts are those of score' -- the target's score' from the threshold pass, then the count pass against it
    (mmt_search_thresholds [lse], mmt_search_count [lse]); with a norm that has `hubs` only the queries whose plain top-1
    candidate is a hub, the others keep their plain counts (dynamic=False normalises every query).  pooling (from
    `pooling`): targets [NS] or [NS, T], one row per SET; the counts are those of the set's pooled score -- the target's
    pooled value from the threshold pass, then the count pass against it (mmt_search_thresholds [query sets],
    mmt_search_count [query sets]), so a target counts itself; not with norm=.  item_pooling (from `item_pooling`): targets are
    SET numbers -1 .. num_sets - 1 and the counts are over the sets, by the set's pooled score
    (mmt_search_thresholds [item sets], mmt_search_count [item sets]); a target counts itself; a subset is one of sets.
    ShardedVideoIndex: each
    shard scores the targets it holds, the primary picks the owner's value per (query, target), each shard counts its
    items against those thresholds and the int32 counts are summed on the primary.
    where (as `search`; not with norm=, pooling= or item_pooling=): only the items that pass the row's filter are counted;
    like a target outside the subset, a target that does not pass is still scored (the unfiltered threshold pass) and
    does not count itself (mmt_search_thresholds, then mmt_search_count_where)."""
    if self.num_items == 0:
      raise ValueError('ranks: the index holds no items')
    self._targets(targets)
    q, qw, dynamic = self._scan_args('ranks', embds, weights, norm, dynamic, subset, pooling=pooling, item_pooling=item_pooling,
                                     where=where)
    scan = _Scan(subset=subset, norm=norm, pooling=pooling, item_pooling=item_pooling, where=where)
    nq, shape = scan.rows(q), targets.shape
    if shape[0] != nq:
      raise ValueError('ranks: %d %s but targets %s' % (nq, 'queries' if pooling is None else 'query sets', tuple(shape)))
    if nq == 0:
      return tuple(torch.empty(shape, device=self.device, dtype=torch.int32) for _ in range(2))
    tg = targets.reshape(nq, -1).contiguous()
    self._target_range(tg, scan)
    out = self._dynamic(dynamic, q, qw, scan, lambda scan: self._rank_counts(q, qw, tg, scan))
    return out[0].reshape(shape), out[1].reshape(shape)

  def ranks(self, embds, weights, targets, subset=None, norm=None, dynamic=None, pooling=None, item_pooling=None,
            where=None):
    """The reference's tie-averaged 0-based rank (model/metric.py:90-121) of item targets[q, t] among the stored items for
    query q: greater + (equal - 1) / 2 from `rank_counts`, +inf where the target is -1.  float64 on the device, of
    targets' shape (float32 would not hold counts above 2^24).  subset: the rank among its items, +inf for a target that
    is not one of them.  norm, dynamic: as `rank_counts` -- the rank under the querybank-normalised score.  pooling: as
    `rank_counts` -- one row per query set, the rank under the set's pooled score.  item_pooling: as `rank_counts` -- the
    rank of the target SET among the sets.  where: as `rank_counts` -- the rank among the items that pass the row's filter,
    +inf for a target that does not."""
    greater, equal = self.rank_counts(embds, weights, targets, subset=subset, norm=norm, dynamic=dynamic, pooling=pooling,
                                      item_pooling=item_pooling, where=where)
    ranks = greater.double() + (equal.double() - 1) / 2
    none = targets < 0
    if subset is not None:
      none = none | ~subset.mask[targets.clamp(min=0)]
    if where is not None:
      none = none | ~where._passes(targets.reshape(targets.shape[0], -1)).reshape(targets.shape)
    return torch.where(none, torch.full_like(ranks, float('inf')), ranks)

  @_refuses_where
  def rescore(self, embds, weights, candidates, k=None):
    """Queries as for `search`; candidates int64 [NQ, C] on the index device, 1 <= C <= MAX_C = 1024, values
    -1 .. num_items - 1 (-1 = none), in any order, an item as often as it comes -> (scores [NQ, k'] float32, indices
    [NQ, k'] int64) on the device, k' = min(k, C); k an int in 1 .. MAX_K, None = min(C, MAX_K).  With S_q the distinct
    non-negative entries of candidates[q], row q holds the min(k', |S_q|) best items of S_q under `search`'s order -- score
    descending, -0 tied with +0, equal scores by ascending item number -- each once, and (-inf, -1) in the slots left: row q
    is search(q, k', subset=subset(S_q)), padded.  A score has the very bits `search` and `target_scores` give the pair on
    THIS index, whatever its dtype (float8_e4m3fn: the scaled score), decoded as `search` decodes it, so a -0 comes back as
    +0.  The result does not depend on the order of a query's candidates, the row batching or the launch geometry, and on
    a ShardedVideoIndex not on where an item is stored: it is bit-identical to one VideoIndex's.  The type, device and
    shape of the candidates are checked before the queries are looked at, their range like the targets of `rank_counts`
    (one small reduction and a host sync) before anything is scored; nothing after that waits for the device.  Two
    launches per row batch (mmt_search_rescore): the pairs' keys from the scoring tile of the scans, then a sort per
    query that drops repeated keys.  ShardedVideoIndex: every shard re-scores the candidates it holds, in its own
    numbers, and the lists are merged on the primary (mmt_search_merge_lists).  Out of scope: norm=, pooling=,
    item_pooling= and groupings are not part of this call; they would be further instantiations of the same kernels."""
    if not torch.is_tensor(candidates) or candidates.dtype != torch.int64:
      raise ValueError('rescore: candidates must be an int64 tensor, got %s' % (
          candidates.dtype if torch.is_tensor(candidates) else type(candidates).__name__))
    if candidates.device != self.device:
      raise ValueError('rescore: candidates must be on the index device %s, got %s' % (self.device, candidates.device))
    if candidates.dim() != 2 or not 1 <= candidates.shape[1] <= MAX_C:
      raise ValueError('rescore: candidates [NQ, 1 <= C <= %d] expected, got %s' % (MAX_C, tuple(candidates.shape)))
    c = candidates.shape[1]
    if k is None:
      k = min(c, MAX_K)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('rescore: k must be None or an int in 1..%d, got %r' % (MAX_K, k))
    if self.num_items == 0:
      raise ValueError('rescore: the index holds no items')
    q, qw = self._queries(embds, weights)
    nq = q.shape[0]
    if candidates.shape[0] != nq:
      raise ValueError('rescore: %d queries but candidates %s' % (nq, tuple(candidates.shape)))
    if nq == 0:
      return _lists(2, self.device, 0, min(k, c))
    cand = candidates.contiguous()
    lo, hi = (int(v) for v in torch.aminmax(cand))
    if lo < -1 or hi >= self.num_items:
      raise ValueError('rescore: candidates must lie in -1 .. %d, got %d .. %d' % (self.num_items - 1, lo, hi))
    return self._rescore(q, qw, cand, min(k, c))

  def _search_refined_filtered(self, embds, weights, coarse, k=10, shortlist=MAX_K, subset=None, exclude=None, where=None):
    """The two-stage search as one call: coarse.search(embds, weights, k=shortlist, subset=subset, exclude=exclude) on a
    cheap index of the same items -- typically a float8_e4m3fn one -- then self.rescore(embds, weights, that list, k) on
    this one -> (scores, indices) [NQ, min(k, shortlist, the coarse list's width)], scores with this index's bits.
    coarse: a VideoIndex or ShardedVideoIndex with this index's num_items, num_experts and dim on this index's (primary)
    device; shortlist an int in 1 .. MAX_K; subset and exclude are `coarse`'s (a subset from ITS `subset`) and are checked
    by it.  The two indexes are TAKEN to hold the same items under the same numbers: that cannot be checked here.
    The coarse search takes `coarse`'s own schedule: with coarse.schedule = 'stream' this is the online pipeline, an fp8
    shortlist streamed for a few queries and then re-scored, and the result is the same to the bit.  where: the filter of
    the COARSE stage, built from `coarse`'s tagging and checked by it; the re-scoring takes the shortlist as it is.  Host
    code only."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('search_refined: k must be an int in 1..%d, got %r' % (MAX_K, k))
    if isinstance(shortlist, bool) or not isinstance(shortlist, int) or not 1 <= shortlist <= MAX_K:
      raise ValueError('search_refined: shortlist must be an int in 1..%d, got %r' % (MAX_K, shortlist))
    if not isinstance(coarse, _Index):
      raise ValueError('search_refined: coarse must be a VideoIndex or ShardedVideoIndex, got %s' % type(coarse).__name__)
    mine, theirs = ((i.num_items, i.num_experts, i.dim) for i in (self, coarse))
    if mine != theirs:
      raise ValueError('search_refined: the coarse index holds (num_items, num_experts, dim) = %s, this one %s' % (theirs, mine))
    if coarse.device != self.device:
      raise ValueError('search_refined: the coarse index is on %s, this one on %s' % (coarse.device, self.device))
    _, shortlisted = coarse.search(embds, weights, k=shortlist, subset=subset, exclude=exclude, where=where)
    return self.rescore(embds, weights, shortlisted, k)

  @_where_option(_search_refined_filtered)
  def search_refined(self, embds, weights, coarse, k=10, shortlist=MAX_K, subset=None, exclude=None):
    return self._search_refined_filtered(embds, weights, coarse, k, shortlist, subset, exclude)

  def _cell_ids(self, cell_ids, num_cells):
    """The checks of `cells` -> (the labels as they came, contiguous; the number of cells).  One small reduction and a host
    sync."""
    if self.num_items == 0:
      raise ValueError('cells: the index holds no items')
    if not torch.is_tensor(cell_ids) or cell_ids.dtype != torch.int64:
      raise ValueError('cells: cell_ids must be an int64 tensor, got %s' % (
          cell_ids.dtype if torch.is_tensor(cell_ids) else type(cell_ids).__name__))
    if cell_ids.device != self.device:
      raise ValueError('cells: cell_ids must be on the index device %s, got %s' % (self.device, cell_ids.device))
    if tuple(cell_ids.shape) != (self.num_items,):
      raise ValueError('cells: cell_ids of shape (%d,) expected, got %s' % (self.num_items, tuple(cell_ids.shape)))
    if num_cells is not None and (isinstance(num_cells, bool) or not isinstance(num_cells, int) or
                                  not 1 <= num_cells < 2 ** 31):
      raise ValueError('cells: num_cells must be None or an int in 1 .. 2^31 - 1, got %r' % (num_cells,))
    lo, hi = (int(v) for v in torch.aminmax(cell_ids))
    if num_cells is None:
      num_cells = max(hi + 1, 1)
    if lo < -1 or hi >= num_cells:
      raise ValueError('cells: cell_ids must lie in -1 .. %d, got %d .. %d' % (num_cells - 1, lo, hi))
    return cell_ids.contiguous(), num_cells

  @staticmethod
  def _cell_csr(cell_ids, num_cells):
    """`cell_lists` on the device of the labels: -> (offsets int64 [num_cells + 1], items int64).  The length of `items`,
    the number of labelled items, is a wait for the device."""
    ids = torch.where(cell_ids >= 0, cell_ids, torch.full_like(cell_ids, num_cells))
    ids, items = torch.sort(ids, stable=True)
    offsets = torch.searchsorted(ids, torch.arange(num_cells + 1, device=ids.device, dtype=torch.int64))
    return offsets, items[:int(offsets[-1])].contiguous()

  def _cells(self, cells, who):
    """Type, origin and age of `cells`."""
    if type(cells) is not self._cells_type or cells._index is not self:
      raise ValueError('%s: cells must come from the cells() or cells_from_centres() of this index, got %s' % (
          who, type(cells).__name__ + (' of another index' if isinstance(cells, IndexCells) else '')))
    if cells.num_items != self.num_items:
      raise ValueError('%s: the cells were built for %d items, the index holds %d' % (who, cells.num_items, self.num_items))

  def sum_scale(self):
    """The SumScale of the exact cell sums for the items held now: bits = lse_bits(num_items), exponent / wexponent from
    the largest stored magnitude and the largest weight (mmt_search_absmax: one pass over the stored rows, per-block
    maxima joined by torch.amax -- on a ShardedVideoIndex every shard's, joined on the primary: a maximum does not depend
    on the order).  The one host sync of the exact path, taken once per index state: the result is kept until the next
    `add`."""
    if self.num_items == 0:
      raise ValueError('sum_scale: the index holds no items')
    cached = getattr(self, '_sum_scale', None)
    if cached is None or cached.num_items != self.num_items:
      largest, wlargest = self._absmax().tolist()
      cached = SumScale(_exponent_of(largest), _exponent_of(wlargest), lse_bits(self.num_items), self.num_items)
      cached._index = self
      self._sum_scale = cached
    return cached

  def _scale(self, scale, who):
    """scale=: None = this index's own `sum_scale`; else type, age and origin of the one given."""
    if scale is None:
      return self.sum_scale()
    if not isinstance(scale, SumScale):
      raise ValueError('%s: scale must be a SumScale (sum_scale() of this index), got %s' % (who, type(scale).__name__))
    if scale.num_items != self.num_items:
      raise ValueError('%s: the scale was built for %d items, the index holds %d' % (who, scale.num_items, self.num_items))
    if scale._index is not None and scale._index is not self:
      raise ValueError('%s: the scale belongs to another index' % who)
    return scale

  @staticmethod
  def _exact_flag(who, exact, scale=None):
    if not isinstance(exact, bool):
      raise ValueError('%s: exact must be a bool, got %r' % (who, exact))
    if scale is not None and not exact:
      raise ValueError('%s: scale= goes with exact=True' % who)

  def cell_sums_exact(self, cells, scale=None, **unsupported):
    """cells as for `cell_sums` -> ExactCellSums: per cell the int64 sums of its members' terms rint(f * 2^(B - E)) (module
    docstring, `cell_sums_exact_ref`) and of their weights' terms, and the counts.  scale: a SumScale, None = this index's
    `sum_scale()`; one built for another num_items or by another index is refused.  Integer sums: a function of a cell's
    member SET, so the same items inserted in another order, or spread over the shards of a ShardedVideoIndex in any way,
    give the same numbers -- there every shard sums its own part under the global scale on its own device
    (mmt_search_cell_sums_exact) and the int64 tensors are added on the primary.  `.float()` gives them in fp32."""
    self._not_trained('cell_sums_exact', unsupported)
    self._cells(cells, 'cell_sums_exact')
    scale = self._scale(scale, 'cell_sums_exact')
    sums, wsums = self._exact_sums(cells, scale)
    return ExactCellSums(sums, wsums, cells.sizes.clone(), scale)

  def _centroid_out(self, cells, out):
    """out= of `cell_centroids`: None -> a pair of zeros; else the checks of the pair given."""
    c, m, d = cells.num_cells, self.num_experts, self.dim
    if out is None:
      return torch.zeros(c, m, d, device=self.device), torch.zeros(c, m, device=self.device)
    if not isinstance(out, (tuple, list)) or len(out) != 2 or not all(torch.is_tensor(t) for t in out):
      raise ValueError('cell_centroids: out must be a pair of tensors (embds, weights)')
    for t, shape in zip(out, ((c, m, d), (c, m))):
      if t.dtype != torch.float32 or t.device != self.device or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError('cell_centroids: out must hold contiguous float32 tensors %s and %s on the index device %s' % (
            (c, m, d), (c, m), self.device))
    return out[0], out[1]

  def _exact_centroids(self, cells, out, scale):
    """`cell_centroids(exact=True)` behind its checks: the exact sums, then the finish on the index device (the primary)."""
    sums, wsums = self._exact_sums(cells, scale)
    _exact_finish(sums, wsums, cells.offsets, scale, out[0], out[1])
    return out

  @staticmethod
  def _not_trained(who, unsupported):
    for name in unsupported:
      if name not in _NOT_TRAINED:
        raise TypeError('%s() got an unexpected keyword argument %r' % (who, name))
      raise ValueError('%s: %s= is out of scope: the cells hold stored items and their plain sim assigns them' % (who, name))

  def assign_cells(self, quantiser):
    """quantiser: a CellQuantiser trained either way, with this index's dtype, num_experts and dim -> this index's cells
    over ALL its items, item g in the cell of its best centroid, ties to the lower cell, carrying `.quantiser`: on a
    VideoIndex quantiser.assign(self); on a ShardedVideoIndex every shard's items are assigned on the shard's device
    against a copy of the centroids there, and the labels are gathered into global order on the primary -- the same
    cells, bit for bit, since a score does not depend on where the item is stored."""
    if not isinstance(quantiser, CellQuantiser):
      raise ValueError('assign_cells: quantiser must be a CellQuantiser, got %s' % type(quantiser).__name__)
    if self.num_items == 0:
      raise ValueError('assign_cells: the index holds no items')
    held = quantiser.centroids
    if (held.dtype, held.num_experts, held.dim) != (self.dtype, self.num_experts, self.dim):
      raise ValueError('assign_cells: the quantiser holds (dtype, num_experts, dim) = (%s, %d, %d), this index (%s, %d, %d)'
                       % (held.dtype, held.num_experts, held.dim, self.dtype, self.num_experts, self.dim))
    _, best = self._assign(quantiser.embds, quantiser.weights, None)
    cells = self.cells(best[:, 0].contiguous(), quantiser.num_cells)
    cells.quantiser = quantiser
    return cells

  def _train_cells(self, num_cells, iters, init, seed, items, exact):
    """`train_cells` behind the options refused by name: the argument checks and the Lloyd loop, on the index device (the
    primary).  The class supplies the assignment (`_assign`) and the update (`cell_centroids`)."""
    if isinstance(num_cells, bool) or not isinstance(num_cells, int) or not 1 <= num_cells < 2 ** 31:
      raise ValueError('train_cells: num_cells must be an int in 1 .. 2^31 - 1, got %r' % (num_cells,))
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 1:
      raise ValueError('train_cells: iters must be an int >= 1, got %r' % (iters,))
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
      raise ValueError('train_cells: seed must be an int in 0 .. 2^32 - 1, got %r' % (seed,))
    for name, t, shape in (('items', items, '[T >= 1]'), ('init', init, '[num_cells]')):
      if t is None:
        continue
      if not torch.is_tensor(t) or t.dtype != torch.int64:
        raise ValueError('train_cells: %s must be an int64 tensor, got %s' % (
            name, t.dtype if torch.is_tensor(t) else type(t).__name__))
      if t.device != self.device:
        raise ValueError('train_cells: %s must be on the index device %s, got %s' % (name, self.device, t.device))
      if t.dim() != 1 or t.shape[0] < 1 or (name == 'init' and t.shape[0] != num_cells):
        raise ValueError('train_cells: %s %s expected, got %s' % (name, shape, tuple(t.shape)))
    if self.num_items == 0:
      raise ValueError('train_cells: the index holds no items')
    n, dev = self.num_items, self.device
    if items is None:
      train = torch.arange(n, device=dev, dtype=torch.int64)
    else:
      lo, hi = (int(v) for v in torch.aminmax(items))
      if lo < 0 or hi >= n:
        raise ValueError('train_cells: items must lie in 0 .. %d, got %d .. %d' % (n - 1, lo, hi))
      train = torch.unique(items)  # ascending
    if num_cells > train.shape[0]:
      raise ValueError('train_cells: %d cells but %d training items' % (num_cells, train.shape[0]))
    if init is None:
      init = train[torch.from_numpy(np.random.RandomState(seed).permutation(train.shape[0])[:num_cells]).to(dev)]
    else:
      lo, hi = (int(v) for v in torch.aminmax(init))
      if lo < 0 or hi >= n:
        raise ValueError('train_cells: init must lie in 0 .. %d, got %d .. %d' % (n - 1, lo, hi))
    ids = torch.full((n,), -1, device=dev, dtype=torch.int64)
    ids[init] = torch.arange(num_cells, device=dev, dtype=torch.int64)
    in_sample = torch.zeros(n, device=dev, dtype=torch.bool)
    in_sample[train] = True
    distinct, sampled = (int(v) for v in torch.stack([(ids >= 0).sum(), in_sample[init].sum()]).tolist())
    if distinct != num_cells:
      raise ValueError('train_cells: the items of init must be distinct')
    if sampled != num_cells:
      raise ValueError('train_cells: the items of init must belong to the training items')
    how = {'exact': True} if exact else {}
    embds, weights = self.cell_centroids(self.cells(ids, num_cells), **how)
    objective, moved = [], []
    for _ in range(iters):
      s, best = self._assign(embds, weights, train)
      new = torch.full_like(ids, -1)
      new[train] = best[:, 0]
      new = _reseed(new, s[:, 0], train, num_cells)
      cells = self.cells(new, num_cells)
      self.cell_centroids(cells, out=(embds, weights), **how)
      objective.append(s.mean())
      moved.append((new != ids).sum())
      ids = new
      if int(moved[-1]) == 0:
        break
    with torch.cuda.device(dev):
      centroids = VideoIndex(embds, weights, dtype=self.dtype)
    return CellQuantiser(centroids, embds, weights, torch.stack(objective), torch.stack(moved), exact,
                         self.sum_scale() if exact else None)

  def cells_from_centres(self, centres):
    """centres: int64 [C] of distinct item numbers on the index device -> the cells of the coarse quantiser that needs no
    second index and no trainer: cell c is the cell of item centres[c], and item g joins the cell of the centre that is
    g's best stored item among the centres in `neighbours`' order -- neighbours(k=1, subset=subset(centres)) -- while a
    centre belongs to its own cell.  `.centres` keeps them, and `.probes` then finds a query's cells with `search` over
    the same subset.  Host code over existing calls; the checks cost one small reduction and a host sync."""
    if not torch.is_tensor(centres) or centres.dtype != torch.int64:
      raise ValueError('cells_from_centres: centres must be an int64 tensor, got %s' % (
          centres.dtype if torch.is_tensor(centres) else type(centres).__name__))
    if centres.device != self.device:
      raise ValueError('cells_from_centres: centres must be on the index device %s, got %s' % (self.device, centres.device))
    if centres.dim() != 1 or centres.shape[0] < 1:
      raise ValueError('cells_from_centres: centres [C >= 1] expected, got %s' % (tuple(centres.shape),))
    if self.num_items == 0:
      raise ValueError('cells_from_centres: the index holds no items')
    centres = centres.contiguous().clone()
    lo, hi = (int(v) for v in torch.aminmax(centres))
    if lo < 0 or hi >= self.num_items:
      raise ValueError('cells_from_centres: centres must lie in 0 .. %d, got %d .. %d' % (self.num_items - 1, lo, hi))
    c = centres.shape[0]
    cell_of = torch.full((self.num_items,), -1, device=self.device, dtype=torch.int64)
    cell_of[centres] = torch.arange(c, device=self.device, dtype=torch.int64)
    if int((cell_of >= 0).sum()) != c:
      raise ValueError('cells_from_centres: the centres must be distinct items')
    subset = self.subset(centres)
    _, best = self.neighbours(k=1, subset=subset)      # an item's best centre other than itself; -1: none (C = 1)
    best = best[:, 0]
    ids = torch.where(cell_of >= 0, cell_of, torch.where(best >= 0, cell_of[best.clamp(min=0)], best))
    cells = self.cells(ids, c)
    cells.centres, cells._subset, cells._cell_of = centres, subset, cell_of
    return cells

  def search_probed(self, embds, weights, cells, probes, k=10, **unsupported):
    """Queries as for `search`; cells from this index's `cells` or `cells_from_centres`; probes int64 [NQ, P] on the index
    device, 1 <= P <= MAX_PROBES = 64: the cells row q looks into, in any order, -1 (or anything outside 0 .. num_cells - 1)
    = none, a cell listed twice counting once -> (scores [NQ, k] float32, indices [NQ, k] int64) on the device, k an int
    in 1 .. MAX_K.  Row q holds the k best items of the union of its probed cells under `search`'s order -- score
    descending, -0 tied with +0, equal scores by ascending ITEM NUMBER, across cells as within one -- and (-inf, -1) in the
    slots left: row q is search(q, k, subset=subset(the probed cells' items)), padded.  That is exact; what is approximate
    about an inverted file is the choice of cells, which is the caller's (`search_cells` makes it with the centres).
    Every score has the very bits `search`, `rescore` and `target_scores` give the pair on this index, whatever its
    dtype.  The result depends on a row's probes as a SET: not on their order, the other rows of the call, the row
    batching, the launch geometry, or on a ShardedVideoIndex the shard.  The (row, probe) pairs are regrouped on the
    device into blocks of at most 64 rows that want the same cell (`probe_plan` restates it), one launch scans them
    through the cells' item table (mmt_search_topk_cells) and the merge of `search` joins a row's lists; per row batch the
    workspace is 8 k P max_pieces bytes a row.  Nothing here waits for the device.  index.schedule has no effect.  Out
    of scope: subset=, exclude=, after=, where=, norm=, dynamic=, pooling=, item_pooling= and grouping= raise ValueError
    naming the option."""
    for name in unsupported:
      if name not in _NOT_PROBED:
        raise TypeError('search_probed() got an unexpected keyword argument %r' % name)
      raise ValueError('search_probed: %s= is out of scope: the candidates are the probed cells and nothing else' % name)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('search_probed: k must be an int in 1..%d, got %r' % (MAX_K, k))
    self._cells(cells, 'search_probed')
    if not torch.is_tensor(probes) or probes.dtype != torch.int64:
      raise ValueError('search_probed: probes must be an int64 tensor, got %s' % (
          probes.dtype if torch.is_tensor(probes) else type(probes).__name__))
    if probes.device != self.device:
      raise ValueError('search_probed: probes must be on the index device %s, got %s' % (self.device, probes.device))
    if probes.dim() != 2 or not 1 <= probes.shape[1] <= MAX_PROBES:
      raise ValueError('search_probed: probes [NQ, 1 <= P <= %d] expected, got %s' % (MAX_PROBES, tuple(probes.shape)))
    q, qw = self._queries(embds, weights)
    if probes.shape[0] != q.shape[0]:
      raise ValueError('search_probed: %d queries but probes %s' % (q.shape[0], tuple(probes.shape)))
    if q.shape[0] == 0 or cells.items.shape[0] == 0:
      return _lists(2, self.device, q.shape[0], k, vacant=True)
    return self._search_probed(q, qw, cells, probes.contiguous(), k)

  def search_cells(self, embds, weights, cells, nprobe=8, k=10):
    """The inverted-file search as one call: cells.probes(embds, weights, nprobe), then search_probed(embds, weights,
    cells, those probes, k) -> (scores, indices) [NQ, k].  cells from this index's `cells_from_centres`.  The probes follow
    index.schedule, as any `search` does; the probed scan does not.  Host code only."""
    self._cells(cells, 'search_cells')
    return self.search_probed(embds, weights, cells, cells.probes(embds, weights, nprobe), k)

  def _candidate_lists(self, who, candidates, widest=MAX_DC, rows='R'):
    """Type, device and shape of the candidate lists of `pair_scores` and `diversify` -- and, `widest` = MAX_C wide, of
    `expert_scores` and `pair_expert_scores` -- in the words of `rescore`'s checks."""
    if not torch.is_tensor(candidates) or candidates.dtype != torch.int64:
      raise ValueError('%s: candidates must be an int64 tensor, got %s' % (
          who, candidates.dtype if torch.is_tensor(candidates) else type(candidates).__name__))
    if candidates.device != self.device:
      raise ValueError('%s: candidates must be on the index device %s, got %s' % (who, self.device, candidates.device))
    if candidates.dim() != 2 or not 1 <= candidates.shape[1] <= widest:
      raise ValueError('%s: candidates [%s, 1 <= C <= %d] expected, got %s' % (who, rows, widest, tuple(candidates.shape)))

  def _candidate_range(self, who, cand):
    """The values of the (non-empty) candidates against -1 .. num_items - 1: one small reduction and a host sync."""
    lo, hi = (int(v) for v in torch.aminmax(cand))
    if lo < -1 or hi >= self.num_items:
      raise ValueError('%s: candidates must lie in -1 .. %d, got %d .. %d' % (who, self.num_items - 1, lo, hi))

  @staticmethod
  def _diverse_args(who, k, lam, unsupported):
    """The checks `diversify` and `search_diverse` share: the options that are out of scope by name, k and lam."""
    for name in unsupported:
      if name not in _NOT_DIVERSE:
        raise TypeError('%s() got an unexpected keyword argument %r' % (who, name))
      raise ValueError('%s: %s= is out of scope: the relevance of a diversified list is the plain score' % (who, name))
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('%s: k must be an int in 1..%d, got %r' % (who, MAX_K, k))
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0 <= lam <= 1:
      raise ValueError('%s: lam must be a number with 0 <= lam <= 1, got %r' % (who, lam))

  @staticmethod
  def _list_batches(rows, c):
    """Row ranges of the Gram launches: the [rows, C, C] fp32 workspace of a batch stays within _BATCH_BYTES."""
    batch = max(1, _BATCH_BYTES // (4 * c * c))
    return [(r0, min(rows, r0 + batch)) for r0 in range(0, rows, batch)]

  def pair_scores(self, candidates):
    """candidates int64 [R, C] on the index device, 1 <= C <= MAX_DC = 128, values -1 .. num_items - 1 (-1 = none), in any
    order, an item as often as it comes -> sims float32 [R, C, C] on the device: sims[r, i, j] = sim(candidates[r, i],
    candidates[r, j]), NaN where either is none, with
        sim(g, h) = <f_g, f_h> / sum_m gw[g][m] gw[h][m]     (0 -> 1e-5)
    f_g the dequantised stored row of item g (float32: the row; bfloat16: widened; float8_e4m3fn: code * scales[g]): the
    'indep' similarity with item g in the query's place, in fp32 on the matrix cores (mmt_search_pair_scores).  sim(g, h)
    has the bits of sim(h, g) and is a function of the two stored rows, their weights and scales only -- not of their
    places in the list, the other candidates, the row batching, num_items or the shard: ShardedVideoIndex.pair_scores is
    bit-identical.  No gathered copy of the rows is made on one index; one block per list reads them in place.  The range
    of the candidates is checked (one small reduction and a host sync) before anything is scored."""
    self._candidate_lists('pair_scores', candidates)
    if self.num_items == 0:
      raise ValueError('pair_scores: the index holds no items')
    r, c = candidates.shape
    sims = torch.empty(r, c, c, device=self.device, dtype=torch.float32)
    if r == 0:
      return sims
    cand = candidates.contiguous()
    self._candidate_range('pair_scores', cand)
    for r0, r1 in self._list_batches(r, c):
      self._pair_scores(cand[r0:r1], sims[r0:r1])
    return sims

  def diversify(self, embds, weights, candidates, k=10, lam=0.5, **unsupported):
    """Max marginal relevance over per-query shortlists (Carbonell & Goldstein, SIGIR 1998).  Queries as for `search`;
    candidates int64 [NQ, C <= MAX_DC = 128] as for `rescore` (-1 = none, any order, repeats allowed); k an int in
    1 .. MAX_K; 0 <= lam <= 1 -> (scores float32, indices int64, values float32), each [NQ, k'], k' = min(k, C).  First
    rescore(embds, weights, candidates, k=None): the distinct candidates of a row in `search`'s order with `search`'s score
    bits, rel -- nothing about relevance is new.  Then, with a = float32(lam), b = float32(1.0 - lam) and sim the
    `pair_scores` of that list, in fp32: slot 0 is the most relevant item, with value fl(a * rel); for every further slot
    each unselected item p has pen_p, the largest sim(p, s) over the selected s, and
        v_p = fl(fl(a * rel_p) - fl(b * pen_p))           two rounded multiplies and a rounded subtract, never an fma
    and the item with the largest v_p is selected: -0 ties with +0, equal values go to the item earlier in `search`'s
    order (mmt_search_mmr).  Slot t holds the item's relevance (the `search` bits), its number and v_p; a row with fewer
    than k' distinct candidates ends in (-inf, -1, -inf).  lam=1 is `rescore`, bit for bit, with values == scores; lam=0
    picks, after the most relevant item, whatever is least like the ones picked.  The result depends on a row's
    candidates as a set, not on their order, the row batching (the [rows, C, C] Gram workspace stays within
    _BATCH_BYTES) or the launch geometry, and ShardedVideoIndex.diversify is bit-identical.  Out of scope: norm=, pooling=,
    item_pooling=, grouping= and after= raise ValueError naming the option."""
    self._diverse_args('diversify', k, lam, unsupported)
    self._candidate_lists('diversify', candidates)
    shape = tuple(getattr(embds, 'shape', ()))  # the query rows as the shape alone says them (text layout: b * C + c)
    rows = shape[0] if len(shape) == 3 else shape[0] * shape[2] if len(shape) == 4 else None
    if rows is not None and candidates.shape[0] != rows:
      raise ValueError('diversify: %d queries but candidates %s' % (rows, tuple(candidates.shape)))
    if self.num_items == 0:
      raise ValueError('diversify: the index holds no items')
    q, qw = self._queries(embds, weights)   # (any other shape is refused here)
    nq, c = q.shape[0], candidates.shape[1]
    k = min(k, c)
    if nq == 0:
      return _lists(2, self.device, 0, k) + (torch.empty(0, k, device=self.device, dtype=torch.float32),)
    cand = candidates.contiguous()
    self._candidate_range('diversify', cand)
    rel, items = self._rescore(q, qw, cand, c)
    scores, indices = _lists(2, self.device, nq, k)
    values = torch.empty(nq, k, device=self.device, dtype=torch.float32)
    with torch.cuda.device(self.device):
      for r0, r1 in self._list_batches(nq, c):
        sims = torch.empty(r1 - r0, c, c, device=self.device, dtype=torch.float32)
        self._pair_scores(items[r0:r1], sims)
        check(_lib.lib().mmt_search_mmr(ops._p(items[r0:r1]), ops._p(rel[r0:r1]), ops._p(sims), r1 - r0, c, k, lam, 1.0 - lam,
                                        ops._p(scores[r0:r1]), ops._p(indices[r0:r1]), ops._p(values[r0:r1]), ops._stream()),
              'mmt_search_mmr')
    return scores, indices, values

  def search_diverse(self, embds, weights, k=10, lam=0.5, shortlist=MAX_K, subset=None, exclude=None, coarse=None,
                     **unsupported):
    """The diversified search as one call, host code in the manner of `search_refined`: (coarse or self).search(embds,
    weights, k=shortlist, subset=subset, exclude=exclude), then self.diversify(embds, weights, that list, k, lam) ->
    (scores, indices, values) [NQ, min(k, the list's width)].  shortlist an int in 1 .. MAX_K; coarse: None, or a
    VideoIndex / ShardedVideoIndex TAKEN to hold the same items under the same numbers (same num_items, num_experts, dim
    and device is all that can be checked) -- typically a float8_e4m3fn one; subset and exclude are the searching
    index's and are checked by it.  Relevance and item-item similarity are this index's.  The shortlist search keeps the
    tile schedule whatever the searching index's `schedule` says.  Out of scope as `diversify`."""
    self._diverse_args('search_diverse', k, lam, unsupported)
    if isinstance(shortlist, bool) or not isinstance(shortlist, int) or not 1 <= shortlist <= MAX_K:
      raise ValueError('search_diverse: shortlist must be an int in 1..%d, got %r' % (MAX_K, shortlist))
    if coarse is not None:
      if not isinstance(coarse, _Index):
        raise ValueError('search_diverse: coarse must be a VideoIndex or ShardedVideoIndex, got %s' % type(coarse).__name__)
      mine, theirs = ((i.num_items, i.num_experts, i.dim) for i in (self, coarse))
      if mine != theirs:
        raise ValueError('search_diverse: the coarse index holds (num_items, num_experts, dim) = %s, this one %s' % (theirs, mine))
      if coarse.device != self.device:
        raise ValueError('search_diverse: the coarse index is on %s, this one on %s' % (coarse.device, self.device))
    if self.num_items == 0:
      raise ValueError('search_diverse: the index holds no items')
    # `search` without the index's schedule: the diversified search is not one of the calls that take it
    _, shortlisted = (self if coarse is None else coarse)._search_call(False, embds, weights, shortlist, subset, exclude)
    return self.diversify(embds, weights, shortlisted, k, lam)

  def _no_scores(self, rows, c):
    return ExpertScores(*(torch.empty(rows, c, self.num_experts, device=self.device, dtype=torch.float32) for _ in range(2)))

  def expert_scores(self, embds, weights, candidates):
    """The thirteenth question: which expert produced a match, and with what share of the gate.  Queries as for `search`;
    candidates int64 [NQ, C] on the index device, 1 <= C <= MAX_C = 1024, values -1 .. num_items - 1 (-1 = none), in any
    order, an item as often as it comes -- the indices `search`, `rescore` or any other call returned -> ExpertScores:
    .parts and .mix float32 [NQ, C, M] on the device, NaN in all M slots of a -1.  With qf = fold_fp32(Q, qw)[q], f_g the
    dequantised stored row of item g (float32: the row; bfloat16: widened; float8_e4m3fn: code * scales[g]) and
    den = sum_m qw[q][m] gw[g][m] in fp32 in expert order (0 -> 1e-5):
        dot_m  = sum_{j < d} qf[m d + j] * f_g[m d + j]
        part_m = dot_m / den          float8_e4m3fn: fl(fl(dot_m * scales[g]) / den) on the codes, as the scans place the scale
        mix_m  = fl(qw[q][m] * gw[g][m]) / den
    so that sum_m part_m is the score of the pair on THIS index -- the quantity `search` returns, defined on the stored
    value -- sum_m mix_m is 1 (0 where the denominator was 0: all parts and mix are then 0) and .expert_sims = parts / mix
    is <Q_m[q], G_m[g]>, the pair's similarity under expert m alone.  dot_m is an fp32 fma chain in an order fixed by
    (d, dtype) and the element index alone and both quotients are correctly rounded divisions, so the values of a pair
    depend on the pair alone, bit for bit -- not on its place in the list, the other candidates, C, NQ, the row batching
    or the shard: ShardedVideoIndex.expert_scores is bit-identical -- and each part is within
    (d + M + 4) * 2^-24 * <|qf_m|, |f_g,m|> / |den| of the fp64 value of the definition.  Only the listed rows are touched:
    one wave per pair on the vector ALUs (mmt_search_expert_parts), no gathered copy of the rows, no dequantised gallery.
    The type, device and shape of the candidates are checked before the queries are looked at, their range like
    `rescore`'s (one small reduction and a host sync); nothing after that waits for the device.  The queries are folded in
    fp32 on every dtype, in row batches whose folded rows and outputs stay within _BATCH_BYTES."""
    self._candidate_lists('expert_scores', candidates, MAX_C, 'NQ')
    if self.num_items == 0:
      raise ValueError('expert_scores: the index holds no items')
    q, qw = self._queries(embds, weights)
    nq, c = q.shape[0], candidates.shape[1]
    if candidates.shape[0] != nq:
      raise ValueError('expert_scores: %d queries but candidates %s' % (nq, tuple(candidates.shape)))
    if nq == 0:
      return self._no_scores(0, c)
    cand = candidates.contiguous()
    self._candidate_range('expert_scores', cand)
    return ExpertScores(*self._expert_parts(q, qw, cand))

  def search_explained(self, embds, weights, k=10, subset=None, exclude=None, after=None, where=None, **unsupported):
    """`search` with its answer explained, host code in the manner of `search_refined`: search(embds, weights, k, subset=,
    exclude=, after=, where=) -- under the index's own `schedule` -- then `expert_scores` on the returned indices ->
    (scores, indices, ExpertScores).  The list is `search`'s to the bit; slot j of the breakdown belongs to indices[:, j],
    and a vacant slot (-inf, -1) has NaN parts.  Out of scope: norm=, dynamic=, pooling= and item_pooling= raise
    ValueError naming the option -- the parts explain the plain score."""
    for name in unsupported:
      if name not in _NOT_EXPLAINED:
        raise TypeError('search_explained() got an unexpected keyword argument %r' % name)
      raise ValueError('search_explained: %s= is out of scope: the parts explain the plain score' % name)
    scores, indices = self.search(embds, weights, k=k, subset=subset, exclude=exclude, after=after, where=where)
    return scores, indices, self.expert_scores(embds, weights, indices)

  def pair_expert_scores(self, items, candidates):
    """`expert_scores` with STORED items in the queries' place: what explains a hit of `pair_scores`, `neighbours` or
    `duplicate_groups` -- whether the picture or only the audio track of two videos agrees.  items int64 [R] on the index
    device, values 0 .. num_items - 1, repeats allowed; candidates int64 [R, C] as for `expert_scores` -> ExpertScores
    [R, C, M] of the pairs (items[r], candidates[r, c]).  The R rows of `items` are gathered and dequantised to fp32
    (exact: float32 as it is, bfloat16 widened, float8_e4m3fn code * scale), their stored weights serve as qw and the
    same kernel runs, so the parts sum to `pair_scores`' sim(g, h) = <f_g, f_h> / sum_m gw[g][m] gw[h][m] and mix_m is
    fl(gw[g][m] * gw[h][m]) over that denominator.  The accumulation order depends on the element index alone, every
    product commutes and the denominator is symmetric in its factors: the values of (g, h) have the bits of (h, g).
    ShardedVideoIndex.pair_expert_scores gathers the rows from their shards onto the primary first and is bit-identical.
    The ranges are checked with one small reduction and a host sync; nothing after that waits for the device."""
    self._candidate_lists('pair_expert_scores', candidates, MAX_C, 'NQ')
    if not torch.is_tensor(items) or items.dtype != torch.int64:
      raise ValueError('pair_expert_scores: items must be an int64 tensor, got %s' % (
          items.dtype if torch.is_tensor(items) else type(items).__name__))
    if items.device != self.device:
      raise ValueError('pair_expert_scores: items must be on the index device %s, got %s' % (self.device, items.device))
    if items.dim() != 1:
      raise ValueError('pair_expert_scores: items [R] expected, got %s' % (tuple(items.shape),))
    if self.num_items == 0:
      raise ValueError('pair_expert_scores: the index holds no items')
    r, c = items.shape[0], candidates.shape[1]
    if candidates.shape[0] != r:
      raise ValueError('pair_expert_scores: %d items but candidates %s' % (r, tuple(candidates.shape)))
    if r == 0:
      return self._no_scores(0, c)
    items, cand = items.contiguous(), candidates.contiguous()
    lo, hi, clo, chi = (int(v) for v in torch.stack(torch.aminmax(items) + torch.aminmax(cand)).tolist())
    if lo < 0 or hi >= self.num_items:
      raise ValueError('pair_expert_scores: items must lie in 0 .. %d, got %d .. %d' % (self.num_items - 1, lo, hi))
    if clo < -1 or chi >= self.num_items:
      raise ValueError('pair_expert_scores: candidates must lie in -1 .. %d, got %d .. %d' % (self.num_items - 1, clo, chi))
    rows, rw = self._stored_rows(items)
    return ExpertScores(*self._expert_parts(rows, rw, cand))

  def _self_args(self, who, items, subset, source, unsupported, k=...):
    """The checks of the self-join calls that look at no value, before anything touches the device -> the index whose
    items are the rows of the join: this one, or `source`."""
    for name in unsupported:
      if name not in _NOT_SELF:
        raise TypeError('%s() got an unexpected keyword argument %r' % (who, name))
      raise ValueError('%s: %s= is out of scope: the self-join scores stored items by their plain sim' % (who, name))
    if k is not ... and (isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K):
      raise ValueError('%s: k must be an int in 1..%d, got %r' % (who, MAX_K, k))
    if source is not None:
      if hasattr(self, 'shards'):
        raise ValueError('%s: source= is not available on a ShardedVideoIndex' % who)
      if not isinstance(source, VideoIndex):
        raise ValueError('%s: source must be a VideoIndex, got %s' % (who, type(source).__name__))
      mine, theirs = ((i.dtype, i.num_experts, i.dim) for i in (self, source))
      if mine != theirs:
        raise ValueError('%s: the source holds (dtype, num_experts, dim) = %s, this index %s' % (who, theirs, mine))
      if source.device != self.device:
        raise ValueError('%s: the source is on %s, this index on %s' % (who, source.device, self.device))
    if items is not None:
      if not torch.is_tensor(items) or items.dtype != torch.int64:
        raise ValueError('%s: items must be an int64 tensor, got %s' % (
            who, items.dtype if torch.is_tensor(items) else type(items).__name__))
      if items.device != self.device:
        raise ValueError('%s: items must be on the index device %s, got %s' % (who, self.device, items.device))
      if items.dim() != 1:
        raise ValueError('%s: items [R] expected, got %s' % (who, tuple(items.shape)))
    if subset is not None:
      self._subset(subset, who)
    if self.num_items == 0:
      raise ValueError('%s: the index holds no items' % who)
    if source is not None and source.num_items == 0:
      raise ValueError('%s: the source holds no items' % who)
    return self if source is None else source

  def _self_items(self, who, rows, items):
    """The rows of the join as int64 [R] of `rows`' item numbers: every item in order for None, else the given ones with
    their range checked as `rescore` checks its candidates (one small reduction and a host sync)."""
    n = rows.num_items
    if items is None:
      return torch.arange(n, device=self.device, dtype=torch.int64)
    items = items.contiguous()
    if items.numel():
      lo, hi = (int(v) for v in torch.aminmax(items))
      if lo < 0 or hi >= n:
        raise ValueError('%s: items must lie in 0 .. %d, got %d .. %d' % (who, n - 1, lo, hi))
    return items

  def neighbours(self, k=10, items=None, subset=None, source=None, **unsupported):
    """The gallery searched against itself: per stored item its k best stored items -> (scores [R, k] float32, indices
    [R, k] int64) on the device.  items: int64 [R] on the index device, the rows of the join, values 0 .. num_items - 1,
    repeats allowed; None = every stored item in order.  subset (from this index's `subset`): only its items are
    candidates; the rows are not restricted by it.  k an int in 1 .. MAX_K: the width of the outputs; the slots a row
    cannot fill hold (-inf, -1), as `rescore` pads.  Row r holds the best candidates other than items[r] itself under
    `search`'s order -- sim descending, -0 tied with +0, equal sims by ascending item number -- and the self pair is left
    out by item NUMBER, not by score: an exact copy of an item stays in its list.  Every score has exactly the bits
    `pair_scores` gives the pair on this index, on all three storage dtypes,
        sim(g, h) = <f_g, f_h> / sum_m gw[g][m] gw[h][m]     (0 -> 1e-5)
    whatever the row batching, the launch geometry, num_items, the items' positions or the shard:
    ShardedVideoIndex.neighbours is bit-identical.  source: another VideoIndex with this one's dtype, num_experts and dim
    on its device; its items are then the rows (`items` numbers them, None = all of it), the columns are this index and no
    self pair is removed -- de-duplicating an upload batch against the gallery before `add`.  Not on a ShardedVideoIndex.
    A streaming scan (mmt_search_self_topk): blocks of 64 rows x one gallery chunk keep a running top-k per row and a
    merge launch joins the chunk lists; the NV x NV matrix never exists.  The range of `items` is checked with one small
    reduction and a host sync; nothing after that waits for the device.  Out of scope: norm=, pooling=, item_pooling=,
    grouping=, after= and exclude= raise ValueError naming the option."""
    rows = self._self_args('neighbours', items, subset, source, unsupported, k)
    items = self._self_items('neighbours', rows, items)
    outs = _lists(2, self.device, items.shape[0], k, vacant=True)
    if items.shape[0]:
      self._neighbours(rows, items, items if source is None else None, k, subset, outs)
    return outs

  def neighbour_range(self, threshold, items=None, subset=None, source=None, order='index', max_hits=_MAX_HITS,
                      **unsupported):
    """Per row item EVERY candidate with sim >= threshold, however many, as a CSR over the R rows -> RangeResult.  items,
    subset and source as `neighbours`: the self pair is left out by item number, the scores have `pair_scores`' bits.
    threshold and order as `range_search`: a Python float, or float32 [R] on the index device; a plain `>=` compare, so
    NaN hits nothing and -inf every candidate; order='index' by ascending item number, 'score' in `search`'s order, so a
    row continues that item's `neighbours` list.  Two scans and no atomics (mmt_search_self_range_count,
    mmt_search_self_range_fill); the total is known after the first -- the call's wait for the device -- and a total above
    max_hits raises ValueError before anything of that size exists.  ShardedVideoIndex.neighbour_range is bit-identical."""
    rows = self._self_args('neighbour_range', items, subset, source, unsupported)
    self._range_options('neighbour_range', threshold, order, max_hits)
    items = self._self_items('neighbour_range', rows, items)
    r = items.shape[0]
    if torch.is_tensor(threshold):
      if threshold.device != self.device:
        raise ValueError('neighbour_range: threshold must be on the index device %s, got %s' % (self.device, threshold.device))
      if threshold.shape[0] != r:
        raise ValueError('neighbour_range: %d rows but threshold %s' % (r, tuple(threshold.shape)))
      thr = threshold.contiguous()
    else:
      thr = torch.full((r,), float(threshold), device=self.device, dtype=torch.float32)
    return self._neighbour_range(rows, items, items if source is None else None, thr, subset, order, max_hits,
                                 'neighbour_range')

  def duplicate_groups(self, threshold, subset=None, max_hits=_MAX_HITS, **unsupported):
    """The connected components of the threshold graph {g ~ h : sim(g, h) >= threshold, g != h} -> labels int64
    [num_items] on the device: labels[g] is the smallest item number in g's component.  threshold a Python float.  subset:
    both ends of an edge must be in it; items outside keep their own number.  The graph is undirected because sim is
    symmetric to the bit.  Built from `neighbour_range` in row batches: only the edge list (each edge once) and
    O(num_items) state are ever held, and more than max_hits hits raise ValueError.  The components come from
    `connected_components`, minimum-label propagation with pointer jumping in torch ops.  The result goes unchanged into
    `grouping`, so `search_groups` de-duplicates a list without anybody's labels."""
    self._self_args('duplicate_groups', None, subset, None, unsupported)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
      raise ValueError('duplicate_groups: threshold must be a float, got %s' % type(threshold).__name__)
    if isinstance(max_hits, bool) or not isinstance(max_hits, int) or max_hits < 0:
      raise ValueError('duplicate_groups: max_hits must be an int >= 0, got %r' % (max_hits,))
    n = self.num_items
    rows = torch.arange(n, device=self.device) if subset is None else torch.nonzero(subset.mask).reshape(-1)
    src, dst, spent = [], [], 0
    for r0 in range(0, rows.shape[0], _GROUP_ROWS):
      part = rows[r0:r0 + _GROUP_ROWS]
      thr = torch.full((part.shape[0],), float(threshold), device=self.device, dtype=torch.float32)
      hits = self._neighbour_range(self, part, part, thr, subset, 'index', max_hits, 'duplicate_groups', spent)
      spent += hits.indices.shape[0]
      at = part[_csr_rows(hits.offsets)]
      once = at < hits.indices   # an undirected edge is hit from both ends: kept from the lower one
      src.append(at[once])
      dst.append(hits.indices[once])
    return connected_components(n, torch.cat(src), torch.cat(dst))

  @staticmethod
  def _range_options(who, threshold, order, max_hits):
    """order, max_hits and the type of threshold of a range call, in the words of `range_search`."""
    if order not in ('index', 'score'):
      raise ValueError("%s: order must be 'index' or 'score', got %r" % (who, order))
    if isinstance(max_hits, bool) or not isinstance(max_hits, int) or max_hits < 0:
      raise ValueError('%s: max_hits must be an int >= 0, got %r' % (who, max_hits))
    if torch.is_tensor(threshold):
      if threshold.dtype != torch.float32:
        raise ValueError('%s: threshold must be a float or a float32 tensor, got %s' % (who, threshold.dtype))
      if threshold.dim() != 1:
        raise ValueError('%s: threshold [R] expected, got %s' % (who, tuple(threshold.shape)))
    elif isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
      raise ValueError('%s: threshold must be a float or a float32 tensor, got %s' % (who, type(threshold).__name__))

  def _group_ids(self, group_ids):
    """The checks of `grouping` -> (the ids as int32 [num_items] of their own, the number of distinct ids)."""
    if self.num_items == 0:
      raise ValueError('grouping: the index holds no items')
    if not torch.is_tensor(group_ids) or group_ids.dtype != torch.int64:
      raise ValueError('grouping: group_ids must be an int64 tensor, got %s' % (
          group_ids.dtype if torch.is_tensor(group_ids) else type(group_ids).__name__))
    if group_ids.device != self.device:
      raise ValueError('grouping: group_ids must be on the index device %s, got %s' % (self.device, group_ids.device))
    nv = self.num_items
    if tuple(group_ids.shape) != (nv,):
      raise ValueError('grouping: group_ids of shape (%d,) expected, got %s' % (nv, tuple(group_ids.shape)))
    lo, hi = (int(v) for v in torch.aminmax(group_ids))
    if lo < 0 or hi > MAX_GROUP_ID:
      raise ValueError('grouping: group_ids must lie in 0 .. %d, got %d .. %d' % (MAX_GROUP_ID, lo, hi))
    return group_ids.to(torch.int32).contiguous(), _count_groups(group_ids)

  @_refuses_where
  def search_groups(self, embds, weights, grouping, k=10, subset=None):
    """Queries as for `search`; grouping from this index's `grouping` -> (scores [NQ, k'] float32, groups [NQ, k'] int64,
    items [NQ, k'] int64) on the device, k' = min(k, grouping.num_groups): per query the k' best GROUPS, best first.  A
    group's representative is its member with the largest key under `search`'s order (score descending, -0 tied with +0,
    equal scores by ascending item number) and groups are ranked by their representatives under the same order; slot j
    holds the j-th best group's score, id and representative item, the score with the very bits `search` and
    `target_scores` give the pair.  subset (from this index's `subset`): only its items are candidates, a representative
    is the group's best allowed member, a group with no allowed member does not appear and the slots left without a group
    hold (-inf, -1, -1).  Per-query exclusions and the querybank normalisation are not part of this call.  The scan keeps
    the best k' distinct groups per query and gallery chunk and the merge de-duplicates across chunks
    (mmt_search_topk_groups); nothing here waits for the device.  ShardedVideoIndex: every shard searches its own items
    with its part of the grouping (ids are global: a group may have members on several shards), the lists are copied to
    the primary and merged there, de-duplicating across shards under the global tie rule
    (mmt_search_merge_group_lists)."""
    self._no_fp8('search_groups', 'grouped search')
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
      raise ValueError('search_groups: k must be an int in 1..%d, got %r' % (MAX_K, k))
    if self.num_items == 0:
      raise ValueError('search_groups: the index holds no items')
    self._grouping(grouping, 'search_groups')
    if subset is not None:
      self._subset(subset, 'search_groups')
    q, qw = self._queries(embds, weights)
    return self._search_groups(q, qw, min(k, grouping.num_groups), grouping, subset)

  def _range_args(self, embds, weights, threshold, subset, order, max_hits, where=None):
    """The checks of `range_search` -> q, qw, thr float32 [NQ]."""
    if order not in ('index', 'score'):
      raise ValueError("range_search: order must be 'index' or 'score', got %r" % (order,))
    if isinstance(max_hits, bool) or not isinstance(max_hits, int) or max_hits < 0:
      raise ValueError('range_search: max_hits must be an int >= 0, got %r' % (max_hits,))
    if self.num_items == 0:
      raise ValueError('range_search: the index holds no items')
    if torch.is_tensor(threshold):
      if threshold.dtype != torch.float32:
        raise ValueError('range_search: threshold must be a float or a float32 tensor, got %s' % threshold.dtype)
      if threshold.device != self.device:
        raise ValueError('range_search: threshold must be on the index device %s, got %s' % (self.device, threshold.device))
      if threshold.dim() != 1:
        raise ValueError('range_search: threshold [NQ] expected, got %s' % (tuple(threshold.shape),))
    elif isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
      raise ValueError('range_search: threshold must be a float or a float32 tensor, got %s' % type(threshold).__name__)
    if subset is not None:
      self._subset(subset, 'range_search')
    if where is not None:
      self._where(where, 'range_search')
    q, qw = self._queries(embds, weights)
    nq = q.shape[0]
    self._where_rows(where, 'range_search', nq)
    if torch.is_tensor(threshold):
      if threshold.shape[0] != nq:
        raise ValueError('range_search: %d queries but threshold %s' % (nq, tuple(threshold.shape)))
      thr = threshold.contiguous()
    else:
      thr = torch.full((nq,), float(threshold), device=self.device, dtype=torch.float32)
    return q, qw, thr


class VideoIndex(_Index):
  """A gallery of up to `capacity` items with M expert embeddings of width d (M <= 16), weighted per item and expert.
  dtype=torch.float32 (d % 4 == 0) stores the fold gw (.) G as it is; dtype=torch.bfloat16 (d % 8 == 0) stores it rounded
  once to bf16 -- half the bytes, scored on the bf16 matrix cores against the unrounded fp32 queries (module docstring);
  dtype=torch.float8_e4m3fn (d % 16 == 0) stores it divided by a power of two per item (`scales`) and rounded once to e4m3
  -- a quarter of the bytes, widened exactly to bf16 inside the same scan."""

  def __init__(self, embds, weights, dtype=torch.float32):
    _check_dtype(dtype, _width(embds))
    g, gw = self._items(embds, weights, 'VideoIndex')
    self._allocate(g.shape[0], g.shape[1], g.shape[2], g.device, dtype)
    self.add(g, gw)

  @classmethod
  def empty(cls, capacity, num_experts, dim, device, dtype=torch.float32):
    """An index with room for `capacity` items and none stored: [capacity, M*d] of `dtype` and [capacity, M] fp32 are
    allocated here (float8_e4m3fn: and the fp32 scales [capacity]), `add` fills them chunk by chunk (the unfolded gallery
    is never needed in one piece)."""
    _check_dtype(dtype, dim)
    device = torch.device(device)
    if device.type != 'cuda':
      raise ValueError('VideoIndex.empty: device must be a CUDA device, got %s' % device)
    if device.index is None:
      device = torch.device('cuda', torch.cuda.current_device())
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (capacity, num_experts, dim)):
      raise ValueError('VideoIndex.empty: capacity, num_experts and dim must be ints')
    self = cls.__new__(cls)
    self._allocate(capacity, num_experts, dim, device, dtype)
    return self

  def _allocate(self, capacity, m, d, device, dtype):
    mult = _DTYPES[dtype]
    if capacity < 1 or not 1 <= m <= 16 or d < mult or d % mult:
      raise ValueError('VideoIndex: need capacity >= 1, 1 <= M <= 16 and d %% %d == 0 for %s, got (%d, %d, %d)' % (
          mult, dtype, capacity, m, d))
    self.capacity, self.num_experts, self.dim = capacity, m, d
    self.num_items = 0
    self.device, self.dtype = device, dtype
    self.folded = torch.empty(capacity, m * d, device=device, dtype=dtype)   # gw (.) G; rows < num_items are valid
    self.weights = torch.empty(capacity, m, device=device, dtype=torch.float32)
    # float8_e4m3fn: the power of two each stored row was divided by
    self.scales = torch.empty(capacity, device=device, dtype=torch.float32) if dtype == FP8 else None

  @property
  def nbytes(self):
    """Bytes held by the index: the folded storage plus the weights (float8_e4m3fn: and the scales), at full capacity."""
    return (self.folded.numel() * self.folded.element_size() + self.weights.numel() * 4 +
            (0 if self.scales is None else self.scales.numel() * 4))

  def add(self, embds, weights):
    """Appends items (n, M, d) / (n, M): folded (and for bfloat16 rounded, for float8_e4m3fn scaled per item and rounded)
    straight into the preallocated rows.  Returns (first, last): the new items are numbers first .. last - 1.  Raises
    ValueError, leaving the index as it was, if they do not fit.  The values are taken to be finite and are not checked:
    on a float8_e4m3fn index a NaN or Inf spoils the stored row and the scale of its own item, whose scores then mean
    nothing, and no other item."""
    g, gw = self._items(embds, weights, 'VideoIndex.add')
    n, m, d = g.shape
    if (m, d) != (self.num_experts, self.dim):
      raise ValueError('VideoIndex.add: items (n, %d, %d) expected, got %s' % (self.num_experts, self.dim, tuple(g.shape)))
    if g.device != self.device or gw.device != self.device:
      raise ValueError('VideoIndex.add: items must be on the index device %s' % self.device)
    first, last = self.num_items, self.num_items + n
    if last > self.capacity:
      raise ValueError('VideoIndex.add: %d items do not fit (%d of %d in use)' % (n, first, self.capacity))
    L = _lib.lib()
    with torch.cuda.device(self.device):
      out = self.folded[first:last]
      if self.dtype == FP8:
        check(L.mmt_search_fold_fp8(ops._p(g), ops._p(gw), n, m, d, ops._p(out), ops._p(self.scales[first:last]),
                                    ops._stream()), 'mmt_search_fold_fp8')
      elif self.dtype == torch.bfloat16:
        check(L.mmt_search_fold_bf16(ops._p(g), ops._p(gw), n, m, d, ops._p(out), ops._stream()), 'mmt_search_fold_bf16')
      else:
        check(L.mmt_search_fold(ops._p(g), ops._p(gw), n, m, d, ops._p(out), ops._stream()), 'mmt_search_fold')
      self.weights[first:last].copy_(gw)
    self.num_items = last
    return first, last

  def subset(self, items):
    """items: bool [num_items] (True = allowed) or int64 item numbers (any shape, any order, duplicates allowed), on the
    index device -> IndexSubset for `search`, `rank_counts` and `ranks`.  Packed here, once; the range of the numbers is
    checked (one small reduction and a host sync).  It describes the num_items of this moment: after a further `add` it
    is refused.  Raises ValueError for an empty subset."""
    return IndexSubset(*self._subset_mask(items))

  _item_pooling_type = ItemPooling

  def item_pooling(self, set_size, item_weights=None, mode='mean'):
    """The item sets of an item-pooled scan -> ItemPooling, built once like a subset and passed as item_pooling= to
    `search`, `rank_counts`, `ranks`, `target_scores` and `threshold_counts`: the stored items are num_items / set_size
    sets of set_size consecutive items (1 <= set_size <= MAX_ITEM_SET = 128, num_items % set_size == 0) and such a call
    answers per SET.  item_weights: float32 [num_items] or [num_sets, set_size] on the index device, finite; an item
    whose weight is 0 takes no part, and every set needs an item that does.  None = float32(1 / set_size) on every item,
    the reference's 'avg' on the gallery axis.  mode as `pooling`.  The checks cost one small reduction and one host
    sync.  It describes the num_items of this moment: after a further `add` it is refused."""
    num_sets, w = _check_item_sets('item_pooling', set_size, self.num_items, item_weights, mode, self.device)
    return ItemPooling(set_size, num_sets, w, mode)

  def _subset(self, subset, who, item_pooling=None):
    self._made_here(subset, who, 'subset', IndexSubset, 'VideoIndex.subset', item_pooling)

  def _norm(self, norm, who):
    self._made_here(norm, who, 'norm', HubNorm, 'VideoIndex.hub_norm')

  def grouping(self, group_ids):
    """group_ids: int64 [num_items] on the index device, the group of every item, values 0 .. 2^31 - 2 in any labelling
    (ids need not be dense, members need not be stored next to each other) -> IndexGrouping for `search_groups`.  Stored
    as int32 here, once; the range is checked and the distinct ids are counted (one small reduction, one torch.unique and
    a host sync).  It describes the num_items of this moment: after a further `add` it is refused."""
    return IndexGrouping(*self._group_ids(group_ids))

  def _grouping(self, grouping, who):
    self._made_here(grouping, who, 'grouping', IndexGrouping, 'VideoIndex.grouping')

  _tagging_type = IndexTagging

  def tagging(self, tags):
    """tags: int64 [num_items] on the index device, one 64-bit tag word per stored item -- a bit pattern whose bits mean
    what the caller decides -> IndexTagging, whose `where` builds the filters that where= takes.  Copied here, once; the
    index's own storage and `nbytes` do not change.  It describes the num_items of this moment: after a further `add` it
    is refused.  Nothing here waits for the device."""
    return IndexTagging(self._tags(tags))

  _cells_type = IndexCells

  def cells(self, cell_ids, num_cells=None):
    """cell_ids: int64 [num_items] on the index device, the cell of every item, any labelling in 0 .. num_cells - 1, -1 =
    in no cell (num_cells None = the largest label + 1; a cell may be empty) -> IndexCells for `search_probed`: the
    inverted file, built here once like a grouping -- one stable sort and a searchsorted; the range check, the number of
    labelled items and the largest cell's size are its waits for the device.  The stored rows are not moved or copied and
    `nbytes` does not change: the scan reads them through the cells' item table.  It describes the num_items of this
    moment: after a further `add` it is refused."""
    ids, num_cells = self._cell_ids(cell_ids, num_cells)
    return IndexCells(self, *self._cell_csr(ids, num_cells), self.num_items)

  def _search_probed(self, q, qw, cells, probes, k):
    """`search_probed` behind its checks: q (NQ >= 1, M, d) / qw (NQ, M) fp32 and probes int64 [NQ, P] (contiguous) on the
    index device, cells this index's own with at least one item.  Per row batch the plan (torch, on the device), one
    workspace of P * max_pieces lists of k keys per row and one call.  Nothing here waits for the device."""
    nq, width, L, nothing = q.shape[0], probes.shape[1], _lib.lib(), _Scan()
    outs = _lists(2, self.device, nq, k)
    with torch.cuda.device(self.device):
      for r0, r1 in self._row_batches(nq, 8 * k * width * cells.max_pieces):
        pair_row, pair_slot, work = _probe_plan(probes[r0:r1], cells.offsets, cells.max_pieces)
        desc, _, _, _keep = self._describe(nothing, q, qw, r0, r1)
        ws = torch.empty(L.mmt_topk_cells_workspace_keys(r1 - r0, width, cells.max_pieces, k), device=self.device,
                         dtype=torch.int64)
        check(L.mmt_search_topk_cells(desc, ops._p(cells.items), cells.items.shape[0], ops._p(work), work.shape[0],
                                      ops._p(pair_row), ops._p(pair_slot), pair_row.shape[0], width, cells.max_pieces, k,
                                      ops._p(ws), ops._p(outs[0][r0:r1]), ops._p(outs[1][r0:r1]), ops._stream()),
              'mmt_search_topk_cells')
    return outs

  def cell_sums(self, cells, **unsupported):
    """cells from this index's `cells` (or a quantiser's `assign`) -> (sums [C, M * d] float32, wsums [C, M] float32,
    counts [C] int64) on the device: per cell the sum of its members' stored rows -- dequantised exactly: float32 as it
    is, bfloat16 widened, float8_e4m3fn code x the item's scale -- and of their weights, and the number of members; zero
    for an empty cell.  The update step of a k-means without an fp32 copy of the gallery and without atomics: a cell's
    list is cut into pieces of SUM_PIECE positions, a piece's rows are added in ascending position and the pieces in
    ascending order (`cell_sums_ref` restates it), so the sums of a cell depend on its member list alone -- not on the
    other cells, num_cells, num_items or the launch -- and two calls are bit-identical.  Every labelled row is read once
    (mmt_search_cell_sums, mmt_search_cell_centroids); nothing here waits for the device.  Not on a ShardedVideoIndex:
    `cell_sums_exact` is."""
    self._not_trained('cell_sums', unsupported)
    self._cells(cells, 'cell_sums')
    sums, wsums = self._cell_update(cells, None, None)
    return sums, wsums, cells.sizes.clone()

  def cell_centroids(self, cells, out=None, exact=False, scale=None, **unsupported):
    """cells as for `cell_sums` -> (embds [C, M, d], weights [C, M]) float32 on the device: the centroid of every cell as
    an item, G_c[m] = S[m] / |S[m]|_2 (a zero S[m] gives a zero row) and gw_c[m] = w[m] / n from the cell's `cell_sums`;
    the centroid of a one-item cell is the item.  out: a pair of contiguous float32 tensors of those shapes on the index
    device, written in place and returned; the rows of an EMPTY cell are left as they are (None: zeros).  exact=True
    takes S and w from `cell_sums_exact(cells, scale).float()` instead -- the same formula by the same device code, on
    sums that depend on a cell's member set alone; the default is untouched by it, bit for bit.  On a ShardedVideoIndex
    only exact=True."""
    self._not_trained('cell_centroids', unsupported)
    self._exact_flag('cell_centroids', exact, scale)
    self._cells(cells, 'cell_centroids')
    if exact:
      scale = self._scale(scale, 'cell_centroids')
      return self._exact_centroids(cells, self._centroid_out(cells, out), scale)
    out = self._centroid_out(cells, out)
    self._cell_update(cells, out[0], out[1])
    return out

  def _sum_tables(self, cells):
    """The piece tables of a sum over `cells` (torch, on the device) for a bound the host knows -> (n_work, work,
    piece_start)."""
    n_work = -(-cells.items.shape[0] // SUM_PIECE) + cells.num_cells
    return (n_work,) + _sum_plan(cells.offsets, n_work)

  def _cell_update(self, cells, embds, weights):
    """`cell_sums` and `cell_centroids` behind their checks -> (sums, wsums); embds / weights: the in/out centroid buffers
    or None.  The piece tables (torch, on the device) for a bound the host knows, one workspace of a partial row per
    piece and two calls.  Nothing here waits for the device."""
    c, m, d, L = cells.num_cells, self.num_experts, self.dim, _lib.lib()
    labelled = cells.items.shape[0]
    if labelled == 0:
      return torch.zeros(c, m * d, device=self.device), torch.zeros(c, m, device=self.device)
    sums, wsums = torch.empty(c, m * d, device=self.device), torch.empty(c, m, device=self.device)
    with torch.cuda.device(self.device):
      n_work, work, piece_start = self._sum_tables(cells)
      ws = torch.empty(L.mmt_cell_sums_workspace_floats(n_work, m, d), device=self.device, dtype=torch.float32)
      check(L.mmt_search_cell_sums(ops._p(self.folded), ops._p(self.weights), ops._p(self.scales), _STORAGE[self.dtype],
                                   self.num_items, m, d, ops._p(cells.items), labelled, ops._p(work), n_work, ops._p(ws),
                                   ops._stream()), 'mmt_search_cell_sums')
      check(L.mmt_search_cell_centroids(ops._p(ws), n_work, ops._p(piece_start), ops._p(cells.offsets), labelled, c, m, d,
                                        ops._p(sums), ops._p(wsums), ops._p(embds), ops._p(weights), ops._stream()),
            'mmt_search_cell_centroids')
    return sums, wsums

  def _exact_sums(self, cells, scale):
    """`cell_sums_exact` behind its checks -> (sums int64 [C, M * d], wsums int64 [C, M]) on the device; cells this
    index's own, scale any SumScale (a shard is handed the global one).  The piece tables of `_cell_update`, one int64
    workspace of a partial row per piece and one call.  Nothing here waits for the device."""
    c, m, d, L = cells.num_cells, self.num_experts, self.dim, _lib.lib()
    labelled = cells.items.shape[0]
    if labelled == 0:
      return (torch.zeros(c, m * d, device=self.device, dtype=torch.int64),
              torch.zeros(c, m, device=self.device, dtype=torch.int64))
    sums = torch.empty(c, m * d, device=self.device, dtype=torch.int64)
    wsums = torch.empty(c, m, device=self.device, dtype=torch.int64)
    with torch.cuda.device(self.device):
      n_work, work, piece_start = self._sum_tables(cells)
      ws = torch.empty(L.mmt_cell_sums_exact_workspace_bytes(n_work, m, d) // 8, device=self.device, dtype=torch.int64)
      check(L.mmt_search_cell_sums_exact(ops._p(self.folded), ops._p(self.weights), ops._p(self.scales),
                                         _STORAGE[self.dtype], self.num_items, m, d, ops._p(cells.items), labelled,
                                         ops._p(work), n_work, ops._p(piece_start), c, scale.bits, scale.exponent,
                                         scale.wexponent, ops._p(ws), ops._p(sums), ops._p(wsums), ops._stream()),
            'mmt_search_cell_sums_exact')
    return sums, wsums

  def _absmax(self):
    """float32 [2] on the device: the largest |stored value|, dequantised, and the largest |weight| of the items held
    (mmt_search_absmax and a torch.amax over its per-block maxima).  Nothing here waits for the device."""
    n, m, d = self.num_items, self.num_experts, self.dim
    blocks = max(1, min(_ABSMAX_BLOCKS, -(-(n * m * d // _DTYPES[self.dtype]) // 256)))
    with torch.cuda.device(self.device):
      out = torch.empty(2, blocks, device=self.device, dtype=torch.float32)
      check(_lib.lib().mmt_search_absmax(ops._p(self.folded), ops._p(self.weights), ops._p(self.scales),
                                         _STORAGE[self.dtype], n, m, d, ops._p(out), blocks, ops._stream()),
            'mmt_search_absmax')
      return out.amax(1)

  def _assign(self, embds, weights, train):
    """The assignment step: centroids (embds [C, M, d], weights [C, M] fp32 on the device) and the training items (int64
    ascending, None = every stored item) -> (scores [T, 1], cells [T, 1]) of each item's best centroid."""
    return VideoIndex(embds, weights, dtype=self.dtype).neighbours(k=1, source=self, items=train)

  def train_cells(self, num_cells, iters=10, init=None, seed=0, items=None, exact=False, **unsupported):
    """Spherical k-means over the stored items -> CellQuantiser with num_cells centroids.  num_cells an int in 1 .. the
    number of training items; iters an int >= 1; items: int64 [T] on the index device, the training sample (repeats count
    once; None = every stored item) -- the items outside it are labelled -1 during training; init: int64 [num_cells] of
    distinct item numbers of the sample on the index device, checked as `cells_from_centres` checks its centres (None:
    the first num_cells of a host permutation of the sample seeded with `seed`).  It starts from the cells {init[c]}.  An
    iteration builds the VideoIndex of the centroids in this index's dtype, assigns every training item to its best
    centroid -- centroids.neighbours(k=1, source=self, items=sample), ties to the lower cell -- re-seeds the cells left
    empty with the sample's lowest-scoring items (`reseed_ref`), and takes the new centroids from `cell_centroids`; a cell
    the re-seeding emptied keeps its previous centroid.  `objective[t]` is the mean score of that assignment, `moved[t]`
    the labels it changed; it stops early after an assignment that moved none.  Deterministic: the same index, arguments
    and seed give bit-identical centroids and labels.  exact=True takes every update from `cell_centroids(exact=True)`:
    the result then depends on the items as a set per cell, not on their order in the index, and
    ShardedVideoIndex.train_cells(exact=True) is bit-identical to it.  subset=, where=, norm=, pooling= and item_pooling=
    raise ValueError naming the option."""
    self._not_trained('train_cells', unsupported)
    self._exact_flag('train_cells', exact)
    return self._train_cells(num_cells, iters, init, seed, items, exact)

  @staticmethod
  def _filter_args(scan, r0, r1, nq):
    """The two arguments the `_where` entries take behind the descriptor for query rows r0 .. r1 - 1 of nq: (the tags, the
    rows' masks), and what keeps them alive."""
    masks = scan.where._rows(nq)[r0:r1]
    return (ops._p(scan.where.tagging.tags), ops._p(masks)), masks

  def _search_groups(self, q, qw, k, grouping, subset):
    """`search_groups` behind its argument checks: q (NQ, M, d) / qw (NQ, M) fp32 on the index device, 1 <= k <=
    grouping.num_groups: the width of the three outputs.  Nothing here waits for the device."""
    return self._search(q, qw, k, _Scan(subset), grouping)

  def _describe(self, scan, q, qw, r0, r1, bounds=None):
    """The MmtSearchScan of `scan` over this index for query rows r0 .. r1 - 1 (with a pooling: whole sets): the rows
    folded -- fp32, or the bf16 hi / lo pair of a bfloat16 or float8_e4m3fn index -- the stored rows, and every part the
    scan has, so a caller hands over a _Scan holding only what its operation takes.  bounds: the cursor's keys [NQ] of
    the whole call.  -> (the descriptor, by reference; the sizes its workspace-size function takes; the range of result
    rows the batch writes -- its rows, or its sets; the tensors the descriptor points into, to be kept until the call
    is made).  Fields are given in the struct's order: the cheapest way to fill a ctypes.Structure."""
    qb, wb = q[r0:r1], qw[r0:r1]
    n, m, d = qb.shape
    nv, c, mode, sw, dims, rows = self.num_items, 0, 0, None, None, (r0, r1)
    if self.dtype != torch.float32:
      keep = torch.empty(2, n, m * d, device=self.device, dtype=torch.bfloat16)  # hi = bf16(qf), lo = bf16(qf - hi)
      check(_lib.lib().mmt_search_fold_split_bf16(ops._p(qb), ops._p(wb), n, m, d, ops._p(keep[0]), ops._p(keep[1]),
                                                  ops._stream()), 'mmt_search_fold_split_bf16')
      q_hi, q_lo = keep[0].data_ptr(), keep[1].data_ptr()
    else:
      keep = _fold(qb, wb)
      q_hi, q_lo = keep.data_ptr(), None
    if scan.item_pooling is not None:
      ip = scan.item_pooling
      nv, c, mode, sw, dims = ip.num_sets * ip.set_size, ip.set_size, _POOL_MODES[ip.mode], ip.weights, (n, ip.num_sets, ip.set_size)
    elif scan.pooling is not None:
      pool, c = scan.pooling, scan.pooling.set_size
      n = n // c * c
      mode, sw, dims, rows = _POOL_MODES[pool.mode], pool._on(self.device)[r0:r1], (n // c, c, nv), (r0 // c, r1 // c)
    ex, norm = scan.ex, scan.norm
    desc = _lib.MmtSearchScan(
        q_hi, q_lo, wb.data_ptr(), self.folded.data_ptr(), self.weights.data_ptr(),
        None if self.scales is None else self.scales.data_ptr(),
        None if scan.subset is None else scan.subset.words.data_ptr(),
        None if ex is None else ex[r0:r1].data_ptr(),
        None if bounds is None else bounds[r0:r1].data_ptr(),
        None if norm is None else norm.lse.data_ptr(),
        None if sw is None else sw.data_ptr(),
        _STORAGE[self.dtype], n, nv, m, d, 0 if ex is None else ex.shape[1], 0.0 if norm is None else norm.beta,
        scan.sets, c, mode)
    return ctypes.byref(desc), dims or (n, nv), rows, (desc, keep, wb, sw)

  def _row_batches(self, nq, extra, pooling=None):
    """Row ranges of a scan: a multiple of 64 rows (the query block) whose folded rows (4 bytes per element, fp32 or the
    bf16 hi + lo pair) and `extra` bytes of workspace per row stay within _BATCH_BYTES.  With a pooling a block is
    64 // set_size whole sets, the batches are cut at whole blocks of whole sets and `extra` is per set."""
    per_row = self.num_experts * self.dim * 4 + extra
    block = 64
    if pooling is not None:
      block = 64 // pooling.set_size * pooling.set_size
      per_row = self.num_experts * self.dim * 4 + -(-extra // pooling.set_size)
    batch = max(block, (_BATCH_BYTES // per_row) // block * block)
    return [(r0, min(nq, r0 + batch)) for r0 in range(0, nq, batch)]

  def _batches(self, nq, t_max, pooling=None, columns=None):
    """Row ranges of the rank and range passes: a row's (pooled: a set's) thresholds and chunk counters at full-size
    chunks of the items (item-pooled: of the given virtual columns)."""
    return self._row_batches(nq, 4 * t_max * (1 + 2 * -(-(self.num_items if columns is None else columns) // 4096)), pooling)

  def _hub_norm(self, b, bw, beta, hubs):
    return HubNorm(self._col_lse(b, bw, beta), beta, b.shape[0], hubs)

  def _col_lse(self, b, bw, beta):
    """`hub_norm` behind its checks: b (NB, M, d) / bw (NB, M) fp32 on the index device -> lse fp32 [num_items].  The bank
    goes through in batches of whole 64-row blocks; the running (M, S) pair per item carries from one to the next."""
    nb, nv = b.shape[0], self.num_items
    L, nothing = _lib.lib(), _Scan()
    with torch.cuda.device(self.device):
      lse = torch.empty(nv, device=self.device, dtype=torch.float32)
      state = torch.empty(2, nv, device=self.device, dtype=torch.float32)
      # a row's share of the block's (m, p) pairs: 8 bytes per item / 64 rows
      batches = self._row_batches(nb, -(-nv // 8))
      ws = torch.empty(L.mmt_col_lse_workspace_floats(batches[0][1], nv), device=self.device, dtype=torch.float32)
      for r0, r1 in batches:
        desc, _, _, _keep = self._describe(nothing, b, bw, r0, r1)
        check(L.mmt_search_col_lse(desc, beta, ops._p(ws), ops._p(state), int(r0 == 0), ops._p(lse if r1 == nb else None),
                                   ops._stream()), 'mmt_search_col_lse')
    return lse

  def _row_expsum(self, q, qw, beta, xmax, bits, scan):
    """The sum pass of `query_lse` behind its checks: q (NQ, M, d) / qw (NQ, M) and xmax float32 [NQ] on the index device,
    the scan holding at most a subset of this index -> the integer sums int64 [NQ] over this index's candidates.  bits is
    the caller's: on a shard it comes from the whole gallery's item count.  Per row batch one launch and one torch.sum
    over the chunks of its workspace.  Nothing here waits for the device."""
    nq, nv, L = q.shape[0], self.num_items, _lib.lib()
    with torch.cuda.device(self.device):
      sums = torch.empty(nq, device=self.device, dtype=torch.int64)
      # A row's chunk sums at full-size chunks of 4096 items.  A launch of few blocks cuts the items into smaller chunks, down
      # to 128 (tk_chunk), and a row's workspace is then up to 32 times this estimate, so _BATCH_BYTES is not strictly kept
      # there.  It cannot matter: the chunk is halved only while the launch has fewer than 512 blocks, so a launch with
      # smaller chunks has fewer than 1024 blocks of 64 slots: a workspace below half a megabyte whatever nq and nv are.
      for r0, r1 in self._row_batches(nq, 8 * -(-nv // 4096)):
        desc, _, _, _keep = self._describe(scan, q, qw, r0, r1)
        ws = torch.empty(L.mmt_row_expsum_workspace_ints64(r1 - r0, nv), device=self.device, dtype=torch.int64)
        check(L.mmt_search_row_expsum(desc, beta, ops._p(xmax[r0:r1]), bits, ops._p(ws), ops._stream()),
              'mmt_search_row_expsum')
        torch.sum(ws.view(r1 - r0, -1), 1, out=sums[r0:r1])
    return sums

  def _reverse_search(self, q, qw, k):
    return self._col_topk(q, qw, k, False)[:2]

  def _csls_norm(self, b, bw, k, hubs):
    return HubNorm(self._col_topk(b, bw, min(k, b.shape[0]), True)[2], 2.0, b.shape[0], hubs, kind='csls', k=k)

  def _col_topk(self, q, qw, k, want_mean):
    """`reverse_search` and `csls_norm` behind their checks: q (NQ >= 1, M, d) / qw (NQ, M) fp32 on the index device,
    1 <= k <= min(MAX_RK, NQ) -> (scores fp32 [num_items, k], rows int64 [num_items, k], mean fp32 [num_items]); with
    want_mean only the mean is made, without it only the lists.  The rows go through in batches of whole 64-row blocks;
    the running list per item (`state`) carries from one to the next and the outputs are asked for with the last.  Beyond
    state and outputs nothing grows with NQ * num_items: a batch's partial lists are within _BATCH_BYTES, or one 64-row
    block's where that alone is more.  Nothing here waits for the device."""
    nq, nv = q.shape[0], self.num_items
    L, nothing = _lib.lib(), _Scan()
    scores = rows = mean = None
    with torch.cuda.device(self.device):
      if want_mean:
        mean = torch.empty(nv, device=self.device, dtype=torch.float32)
      else:
        scores, rows = _lists(2, self.device, nv, k)
      state = torch.empty(nv, k, device=self.device, dtype=torch.int64)   # uint64 keys
      # a row's share of its block's partial lists: 8 k bytes per item / 64 rows
      batches = self._row_batches(nq, -(-8 * k * nv // 64))
      ws = torch.empty(L.mmt_col_topk_workspace_keys(batches[0][1], nv, k), device=self.device, dtype=torch.int64)
      weight = float(torch.tensor(1.0 / k, dtype=torch.float32))
      for r0, r1 in batches:
        desc, _, _, _keep = self._describe(nothing, q, qw, r0, r1)
        last = r1 == nq
        check(L.mmt_search_col_topk(desc, k, r0, ops._p(ws), ops._p(state), int(r0 == 0), ops._p(scores if last else None),
                                    ops._p(rows if last else None), ops._p(mean if last else None), weight,
                                    ops._stream()), 'mmt_search_col_topk')
    return scores, rows, mean

  def _search(self, q, qw, k, scan, grouping=None):
    """The top-k pass of `search` and `search_groups` behind their argument checks: q (NQ, M, d) / qw (NQ, M) fp32 on the
    index device, the scan's parts this index's own -> (scores, indices), with a grouping (scores, groups, items), one
    row per query or query set, min(k, the candidates) wide (a grouping: k).  The unmasked plain scan is handed k as it
    is and writes min(k, NV) columns; only with exclusions or a cursor can a slot stay without a candidate, so only
    then are the outputs filled beforehand.  A cursor's bounds are built once, on the device (mmt_search_after_keys),
    and sliced per row batch next to the exclusions.  Nothing here waits for the device."""
    nq, nv, L = q.shape[0], self.num_items, _lib.lib()
    paged, filtered = scan.after is not None, scan.where is not None
    masked = scan.subset is not None or scan.ex is not None or paged or filtered
    if grouping is None and (masked or scan.sets):
      k = min(k, scan.candidates(self))  # lists no longer than the candidates: the outputs stay dense
    outs = _lists(2 if grouping is None else 3, self.device, scan.rows(q), min(k, nv),
                  vacant=scan.ex is not None or paged or filtered)
    if nq == 0:
      return outs
    name = 'mmt_search_topk'
    workspace = getattr(L, _WORKSPACES[scan.sets][0])
    if scan.stream:   # behind `search`'s checks: no norm, no sets; with a grouping nobody asks for it
      name, workspace = 'mmt_search_topk_stream', L.mmt_topk_stream_workspace_keys
    if filtered:      # behind the checks: no norm, no sets, no grouping; the unfiltered entry's workspace
      name += '_where'
    topk = getattr(L, name)
    bounds = None
    with torch.cuda.device(self.device):
      if paged:
        a_scores, first = (t.contiguous() for t in scan.after)
        bounds = torch.empty(nq, device=self.device, dtype=torch.int64)   # uint64 keys
        check(L.mmt_search_after_keys(ops._p(a_scores), ops._p(first), nq, ops._p(bounds), ops._stream()),
              'mmt_search_after_keys')
      # a row's (pooled: a set's) chunk lists at full-size chunks
      for r0, r1 in self._row_batches(nq, 8 * k * -(-scan.columns(self) // 4096), scan.pooling):
        desc, dims, (o0, o1), _keep = self._describe(scan, q, qw, r0, r1, bounds)
        ws = torch.empty(workspace(*dims, k), device=self.device, dtype=torch.int64)
        if grouping is None:
          tagged, _masks = self._filter_args(scan, r0, r1, nq) if filtered else ((), None)
          check(topk(desc, *tagged, k, ops._p(ws), ops._p(outs[0][o0:o1]), ops._p(outs[1][o0:o1]), ops._stream()), name)
        else:
          check(L.mmt_search_topk_groups(desc, k, ops._p(grouping.ids), ops._p(ws), ops._p(outs[0][o0:o1]),
                                         ops._p(outs[1][o0:o1]), ops._p(outs[2][o0:o1]), ops._stream()),
                'mmt_search_topk_groups')
    return outs

  def _rescore(self, q, qw, cand, k):
    """`rescore` behind its checks: q (NQ >= 1, M, d) / qw (NQ, M) fp32 and cand int64 [NQ, C] (contiguous, item numbers,
    one outside 0 .. num_items - 1 = none) on the index device, 1 <= k <= min(C, MAX_K): the width of the outputs.  One
    call and one workspace of C keys per row for every row batch.  Nothing here waits for the device."""
    nq, c, L, nothing = q.shape[0], cand.shape[1], _lib.lib(), _Scan()
    outs = _lists(2, self.device, nq, k)
    with torch.cuda.device(self.device):
      for r0, r1 in self._row_batches(nq, 8 * c):
        desc, _, _, _keep = self._describe(nothing, q, qw, r0, r1)
        ws = torch.empty(L.mmt_rescore_workspace_keys(r1 - r0, c), device=self.device, dtype=torch.int64)
        check(L.mmt_search_rescore(desc, ops._p(cand[r0:r1]), c, k, ops._p(ws), ops._p(outs[0][r0:r1]),
                                   ops._p(outs[1][r0:r1]), ops._stream()), 'mmt_search_rescore')
    return outs

  def _pair_scores(self, cand, sims):
    """`pair_scores` behind its checks, one row batch: cand int64 [R >= 1, C] (contiguous, item numbers, one outside
    0 .. num_items - 1 = none) -> sims float32 [R, C, C] (contiguous), both on the index device.  One launch; nothing here
    waits for the device."""
    r, c = cand.shape
    with torch.cuda.device(self.device):
      check(_lib.lib().mmt_search_pair_scores(ops._p(self.folded), ops._p(self.weights), ops._p(self.scales),
                                              _STORAGE[self.dtype], self.num_items, self.num_experts, self.dim, ops._p(cand),
                                              r, c, ops._p(sims), ops._stream()), 'mmt_search_pair_scores')

  def _expert_parts(self, q, qw, cand):
    """`expert_scores` and `pair_expert_scores` behind their checks: q (R >= 1, M, d) fp32 queries, folded here in fp32 batch
    by batch whatever the index's dtype, or (R, M * d) fp32 rows that stand folded already (dequantised stored rows);
    qw (R, M) and cand int64 [R, C] (contiguous, item numbers, one outside 0 .. num_items - 1 = none), all on the index
    device -> (parts, mix) float32 [R, C, M].  One launch per row batch, no workspace: a row's outputs are 8 C M bytes.
    Nothing here waits for the device."""
    r, c, m, L = q.shape[0], cand.shape[1], self.num_experts, _lib.lib()
    with torch.cuda.device(self.device):
      parts, mix = (torch.empty(r, c, m, device=self.device, dtype=torch.float32) for _ in range(2))
      for r0, r1 in self._row_batches(r, 8 * c * m):
        wb = qw[r0:r1]
        qf = _fold(q[r0:r1], wb) if q.dim() == 3 else q[r0:r1]
        check(L.mmt_search_expert_parts(ops._p(qf), ops._p(wb), ops._p(self.folded), ops._p(self.weights),
                                        ops._p(self.scales), _STORAGE[self.dtype], self.num_items, m, self.dim,
                                        ops._p(cand[r0:r1]), r1 - r0, c, ops._p(parts[r0:r1]), ops._p(mix[r0:r1]),
                                        ops._stream()), 'mmt_search_expert_parts')
    return parts, mix

  def _stored_rows(self, items):
    """The stored rows of `items` (int64 [R], 0 .. num_items - 1, on the index device) dequantised to fp32 -- exact on every
    dtype -- with their weights: (rows [R, M * d], weights [R, M]).  R rows only."""
    with torch.cuda.device(self.device):
      stored = self.folded.view(torch.uint8)[items]   # bytes: a gather, whatever the dtype
      return _dequantised(stored, self.dtype, None if self.scales is None else self.scales[items]), self.weights[items]

  def _self_rows(self):
    """This index's stored operand as the A side of the self-join entries: (rows, weights, scales or None, NA)."""
    return self.folded, self.weights, self.scales, self.num_items

  def _self_operands(self, a, items, own, r0, r1, subset):
    """The fifteen leading arguments of the self-join entries for rows r0 .. r1 - 1: a = (rows, weights, scales or None,
    NA), a stored operand on this device in this index's dtype; items int64 [R] or None (row r of the join is row r of a:
    the operand is then handed over from row r0 on); own int64 [R] or None, this index's item each row must not meet;
    then this index as the B side with the subset's words."""
    rows, aw, asc, na = a
    if items is None:
      rows, aw, asc, na = rows[r0:], aw[r0:], None if asc is None else asc[r0:], na - r0
    return (ops._p(rows), ops._p(aw), ops._p(asc), na, ops._p(None if items is None else items[r0:r1]),
            ops._p(None if own is None else own[r0:r1]), r1 - r0, ops._p(self.folded), ops._p(self.weights),
            ops._p(self.scales), self.num_items, ops._p(None if subset is None else subset.words), _STORAGE[self.dtype],
            self.num_experts, self.dim)

  def _neighbours(self, rows, items, own, k, subset, outs):
    self._self_topk(rows._self_rows(), items, own, k, subset, outs)

  def _self_topk(self, a, items, own, k, subset, outs):
    """`neighbours` behind its checks: a, items, own as `_self_operands`; outs (scores, indices) [R >= 1, k] on this
    device, prefilled with (-inf, -1): only the slots with a candidate are written.  Rows go in batches of whole 64-row
    blocks whose chunk lists stay within _BATCH_BYTES.  Nothing here waits for the device."""
    r, nv, L = outs[0].shape[0], self.num_items, _lib.lib()
    with torch.cuda.device(self.device):
      for r0, r1 in self._row_batches(r, 8 * k * -(-nv // 4096)):
        ws = torch.empty(L.mmt_self_topk_workspace_keys(r1 - r0, nv, k), device=self.device, dtype=torch.int64)
        check(L.mmt_search_self_topk(*self._self_operands(a, items, own, r0, r1, subset), k, ops._p(ws),
                                     ops._p(outs[0][r0:r1]), ops._p(outs[1][r0:r1]), ops._stream()), 'mmt_search_self_topk')

  def _self_range_count(self, a, items, own, thr, subset):
    """The count pass of `neighbour_range` (`_count_batches`): a, items, own as `_self_operands`."""
    return self._count_batches('mmt_self_range_workspace_ints', 'mmt_search_self_range_count',
                               lambda r0, r1: (self._self_operands(a, items, own, r0, r1, subset), None), thr)

  def _self_range_fill(self, a, items, own, thr, subset, kept, offsets, indices, scores):
    """The fill pass of `neighbour_range`: `kept` from `_self_range_count` of the same arguments (`_fill_batches`)."""
    self._fill_batches('mmt_search_self_range_fill',
                       lambda r0, r1: (self._self_operands(a, items, own, r0, r1, subset), None), thr, kept, offsets,
                       indices, scores)

  def _scan_lead(self, q, qw, subset, where=None):
    """The leading arguments of the range entries over queries: (r0, r1) -> ((the batch's descriptor, with a filter the
    tags and the rows' masks), what they point at)."""
    scan = _Scan(subset, where=where)

    def lead(r0, r1):
      desc, _, _, keep = self._describe(scan, q, qw, r0, r1)
      if where is None:
        return (desc,), keep
      tagged, masks = self._filter_args(scan, r0, r1, q.shape[0])
      return (desc,) + tagged, (keep, masks)
    return lead

  def _count_batches(self, workspace, entry, lead, thr):
    """The count pass of a range scan, batch by batch: thr float32 [R] on this device, one per row; lead(r0, r1) -> (the
    entry's arguments before the thresholds, what keeps them alive) -> (hits per row int64 [R], the batches' workspaces as
    the fill pass wants them).  Nothing here waits for the device."""
    r, nv, L = thr.shape[0], self.num_items, _lib.lib()
    counts = torch.empty(r, device=self.device, dtype=torch.int64)
    kept = []
    for r0, r1 in self._batches(r, 1):
      args, _keep = lead(r0, r1)
      ws = torch.empty(getattr(L, workspace)(r1 - r0, nv), device=self.device, dtype=torch.int32)
      check(getattr(L, entry)(*args, ops._p(thr[r0:r1]), ops._p(ws), ops._p(counts[r0:r1]), ops._stream()), entry)
      kept.append(ws)
    return counts, kept

  def _fill_batches(self, entry, lead, thr, kept, offsets, indices, scores):
    """The fill pass of a range scan: `kept` from `_count_batches` of the same arguments, offsets int64 [R + 1] into
    indices / scores."""
    L = _lib.lib()
    for (r0, r1), ws in zip(self._batches(thr.shape[0], 1), kept):
      args, _keep = lead(r0, r1)
      check(getattr(L, entry)(*args, ops._p(thr[r0:r1]), ops._p(ws), ops._p(offsets[r0:r1 + 1]), ops._p(indices),
                              ops._p(scores), ops._stream()), entry)

  def _csr(self, r, count, fill, order, max_hits, who, spent=0):
    """The CSR of a range scan of r rows, `range_search`'s and `neighbour_range`'s: count() -> (hits per row int64 [r], the
    batches' workspaces) counts every batch first, the sum of the counts places the rows -- the total is the call's one
    wait for the device, held against max_hits (spent: the hits an enclosing call has already used of it) before anything
    of output size exists -- then comes the one allocation, then fill(workspaces, offsets, indices, scores)."""
    with torch.cuda.device(self.device):
      offsets = torch.zeros(r + 1, device=self.device, dtype=torch.int64)
      total = 0
      if r:
        counts, kept = count()
        torch.cumsum(counts, 0, out=offsets[1:])
        total = int(offsets[-1])
      if spent + total > max_hits:
        raise ValueError('%s: %d hits exceed max_hits = %d' % (who, spent + total, max_hits))
      indices = torch.empty(total, device=self.device, dtype=torch.int64)
      scores = torch.empty(total, device=self.device, dtype=torch.float32)
      if total:
        fill(kept, offsets, indices, scores)
      return _range_result(offsets, indices, scores, order)

  def _neighbour_range(self, rows, items, own, thr, subset, order, max_hits, who, spent=0):
    """`neighbour_range` behind its checks (`_csr`): items int64 [R] of `rows`' numbers, own as `_self_operands`, thr
    float32 [R]."""
    a = rows._self_rows()
    return self._csr(items.shape[0], lambda: self._self_range_count(a, items, own, thr, subset),
                     lambda *outs: self._self_range_fill(a, items, own, thr, subset, *outs), order, max_hits, who, spent)


  def _rank_counts(self, q, qw, tg, scan):
    """`rank_counts` behind its checks: tg int64 [NQ >= 1, T] on the index device (with a pooling [num_sets, T], with an
    item pooling set numbers) -> (greater, equal) int32 of its shape.  Plain: the threshold and the count pass in one
    call per batch (mmt_search_rank); with a norm, a pooling, an item pooling or a filter: one after the other."""
    if scan.norm is not None or scan.sets or scan.where is not None:
      return self._threshold_counts(q, qw, self._target_scores(q, qw, tg, scan), scan)
    nq, nv, L = q.shape[0], self.num_items, _lib.lib()
    greater = torch.empty(tg.shape, device=self.device, dtype=torch.int32)
    equal = torch.empty(tg.shape, device=self.device, dtype=torch.int32)
    t_max = min(MAX_T, tg.shape[1])
    with torch.cuda.device(self.device):
      for r0, r1 in self._batches(nq, t_max):
        desc, _, _, _keep = self._describe(scan, q, qw, r0, r1)
        ws = torch.empty(L.mmt_rank_workspace_ints(r1 - r0, nv, t_max), device=self.device, dtype=torch.int32)
        for tgs, (gs, es) in _column_groups(tg, (greater, equal), r0, r1):
          check(L.mmt_search_rank(desc, ops._p(tgs), tgs.shape[1], ops._p(ws), ops._p(gs), ops._p(es), ops._stream()),
                'mmt_search_rank')
    return greater, equal

  def target_scores(self, embds, weights, targets, norm=None, dynamic=None, pooling=None, item_pooling=None):
    """Queries as for `search`; targets as for `rank_counts` -> float32 of targets' shape on the device:
    score(q, targets[q, t]) with the very bits `search` returns for that pair (the threshold pass of `rank_counts` on its
    own: mmt_search_thresholds), NaN where the target is -1.  norm (VideoIndex.hub_norm): score'(q, targets[q, t]), with
    the bits `search(norm=)` returns; the dynamic rule as there, the plain top-1 taken over all items.  pooling (from
    `pooling`; not with norm=): targets [NS] or [NS, T], one row per query SET -> the set's pooled score of the target with
    the bits the pooled scans compute for the pair, as they are (a -0 stays -0; mmt_search_thresholds [query sets]).
    item_pooling (from `item_pooling`; not with norm= or pooling=): targets are SET numbers -> the query's pooled score of
    the target set, likewise as it is (mmt_search_thresholds [item sets])."""
    if self.num_items == 0:
      raise ValueError('ranks: the index holds no items')
    self._targets(targets)
    q, qw, dynamic = self._scan_args('ranks', embds, weights, norm, dynamic, pooling=pooling, item_pooling=item_pooling)
    scan = _Scan(norm=norm, pooling=pooling, item_pooling=item_pooling)
    nq = scan.rows(q)
    if targets.shape[0] != nq:
      raise ValueError('ranks: %d %s but targets %s' % (nq, 'queries' if pooling is None else 'query sets',
                                                        tuple(targets.shape)))
    if nq:
      self._target_range(targets, scan)
    return self._dynamic(dynamic, q, qw, scan, lambda scan: (self._target_scores(q, qw, targets, scan),))[0]

  def _target_scores(self, q, qw, targets, scan):
    """The threshold pass behind the checks: targets int64 [R] or [R, T] on the index device, R the scan's result rows,
    item numbers (with an item pooling: set numbers); one outside 0 .. the last of them gives NaN.  The scan's subset
    plays no part: a target is scored wherever it lies.  Nothing here waits for the device."""
    nq, L, scored = q.shape[0], _lib.lib(), scan.scored()
    tg = targets.reshape(scan.rows(q), -1).contiguous()
    thr = torch.empty(tg.shape, device=self.device, dtype=torch.float32)
    if nq == 0:
      return thr.reshape(targets.shape)
    with torch.cuda.device(self.device):
      for r0, r1 in self._batches(nq, min(MAX_T, tg.shape[1]), scan.pooling, scan.columns(self)):
        desc, _, (o0, o1), _keep = self._describe(scored, q, qw, r0, r1)
        for tgs, (out,) in _column_groups(tg, (thr,), o0, o1):
          check(L.mmt_search_thresholds(desc, ops._p(tgs), tgs.shape[1], ops._p(out), ops._stream()), 'mmt_search_thresholds')
    return thr.reshape(targets.shape)

  def threshold_counts(self, embds, weights, thresholds, subset=None, norm=None, dynamic=None, pooling=None,
                       item_pooling=None, where=None):
    """Queries as for `search`; thresholds float32 [NQ] or [NQ, T] on the index device -> (greater, equal), int32 of
    thresholds' shape: how many stored items score above / exactly equal to thresholds[q, t] for query q (plain float
    compares; a NaN threshold counts nothing) -- the count pass of `rank_counts` against given values (mmt_search_count).
    Fed with `target_scores` it gives `rank_counts`.  subset: only its items are counted.  norm (VideoIndex.hub_norm): the
    items' score' is what is compared (mmt_search_count [lse]); the dynamic rule as in `rank_counts`.  pooling (from
    `pooling`; not with norm=): thresholds [NS] or [NS, T], one row per query SET; the items' pooled score for the set is
    what is compared (mmt_search_count [query sets]).  item_pooling (from `item_pooling`; not with norm= or pooling=): the
    SETS' pooled scores for the query are what is compared and counted (mmt_search_count [item sets]).  where (as `search`;
    not with norm=, pooling= or item_pooling=): only the items that pass the row's filter are counted
    (mmt_search_count_where)."""
    if self.num_items == 0:
      raise ValueError('ranks: the index holds no items')
    if not torch.is_tensor(thresholds) or thresholds.dtype != torch.float32:
      raise ValueError('ranks: thresholds must be a float32 tensor, got %s' % (
          thresholds.dtype if torch.is_tensor(thresholds) else type(thresholds).__name__))
    if thresholds.device != self.device:
      raise ValueError('ranks: thresholds must be on the index device %s, got %s' % (self.device, thresholds.device))
    if thresholds.dim() not in (1, 2) or thresholds.dim() == 2 and thresholds.shape[1] < 1:
      raise ValueError('ranks: thresholds [NQ] or [NQ, T >= 1] expected, got %s' % (tuple(thresholds.shape),))
    q, qw, dynamic = self._scan_args('ranks', embds, weights, norm, dynamic, subset, pooling=pooling, item_pooling=item_pooling,
                                     where=where)
    scan = _Scan(subset=subset, norm=norm, pooling=pooling, item_pooling=item_pooling, where=where)
    nq = scan.rows(q)
    if thresholds.shape[0] != nq:
      raise ValueError('ranks: %d %s but thresholds %s' % (nq, 'queries' if pooling is None else 'query sets',
                                                           tuple(thresholds.shape)))
    return self._dynamic(dynamic, q, qw, scan, lambda scan: self._threshold_counts(q, qw, thresholds, scan))

  def _threshold_counts(self, q, qw, thresholds, scan):
    """The count pass behind the checks: thresholds float32 [R] or [R, T] on the index device, R the scan's result rows ->
    (greater, equal) int32 of their shape, over the scan's candidates.  Nothing here waits for the device."""
    nq, L = q.shape[0], _lib.lib()
    thr = thresholds.reshape(scan.rows(q), -1).contiguous()
    greater = torch.empty(thr.shape, device=self.device, dtype=torch.int32)
    equal = torch.empty(thr.shape, device=self.device, dtype=torch.int32)
    if nq == 0:
      return greater.reshape(thresholds.shape), equal.reshape(thresholds.shape)
    workspace = getattr(L, _WORKSPACES[scan.sets][1])
    t_max = min(MAX_T, thr.shape[1])
    filtered = scan.where is not None   # behind the checks: no norm, no sets; the unfiltered entry's workspace
    name = 'mmt_search_count_where' if filtered else 'mmt_search_count'
    with torch.cuda.device(self.device):
      for r0, r1 in self._batches(nq, t_max, scan.pooling, scan.columns(self)):
        desc, dims, (o0, o1), _keep = self._describe(scan, q, qw, r0, r1)
        ws = torch.empty(workspace(*dims, t_max), device=self.device, dtype=torch.int32)
        tagged, _masks = self._filter_args(scan, r0, r1, nq) if filtered else ((), None)
        for ts, (gs, es) in _column_groups(thr, (greater, equal), o0, o1):
          check(getattr(L, name)(desc, *tagged, ops._p(ts), ts.shape[1], ops._p(ws), ops._p(gs), ops._p(es), ops._stream()),
                name)
    return greater.reshape(thresholds.shape), equal.reshape(thresholds.shape)

  def range_search(self, embds, weights, threshold, subset=None, order='index', max_hits=_MAX_HITS, where=None):
    """Queries as for `search`; threshold a Python float, or float32 [NQ] on the index device (one per query) ->
    RangeResult: for every query ALL items g with score(q, g) >= threshold[q], however many (`search` stops at MAX_K), as a
    CSR on the device -- offsets int64 [NQ + 1], indices int64 [total], scores float32 [total], counts int64 [NQ]; query q's
    hits are [offsets[q], offsets[q + 1]).  The compare is a plain float compare: a NaN threshold hits nothing, -inf every
    candidate.  A score has the very bits `search` and `target_scores` give that pair.  subset (VideoIndex.subset): only
    its items are candidates.  order='index': each row by ascending item number; order='score': by descending score, equal
    scores (-0 == +0) by ascending item -- `search`'s order, so a row continues that query's top-k list.

    Two scans (mmt_search_range_count, mmt_search_range_fill): the first counts the hits per query and gallery chunk, the
    sum of the counts places the rows, the second writes every hit to its slot -- no atomics, bit-reproducible.  The total
    is known after the first scan (the call's one wait for the device) and nothing of output size exists before: a total
    above max_hits raises ValueError naming it (the default is a guard against a mistyped threshold, not a tuned number).
    Queries run in batches of whole 64-row blocks within _BATCH_BYTES: every batch is counted first, across the whole
    call, then comes the one allocation, then the fills.  Each batch's count workspace is KEPT for its fill rather than
    recounted: it is 4 bytes per query and gallery chunk (at most 1 / 1024 of the score matrix, 1 MiB at 4 096 x 262 144),
    where a recount would be a third scan; the folded queries of a batch, which are large, are folded again instead.
    Exclusions per query are not part of this call: the caller applies them to the CSR.  where (as `search`): only the
    items that pass the row's filter are hits, in both scans alike (mmt_search_range_count_where,
    mmt_search_range_fill_where)."""
    q, qw, thr = self._range_args(embds, weights, threshold, subset, order, max_hits, where)
    return self._csr(q.shape[0], lambda: self._range_count(q, qw, thr, subset, where),
                     lambda *outs: self._range_fill(q, qw, thr, subset, where, *outs), order, max_hits, 'range_search')

  def _range_count(self, q, qw, thr, subset, where=None):
    """The count pass of `range_search` behind its checks (`_count_batches`)."""
    return self._count_batches('mmt_range_workspace_ints', 'mmt_search_range_count' + ('_where' if where is not None else ''),
                               self._scan_lead(q, qw, subset, where), thr)

  def _range_fill(self, q, qw, thr, subset, where, kept, offsets, indices, scores):
    """The fill pass of `range_search`: `kept` from `_range_count` of the same arguments (`_fill_batches`)."""
    self._fill_batches('mmt_search_range_fill' + ('_where' if where is not None else ''),
                       self._scan_lead(q, qw, subset, where), thr, kept, offsets, indices, scores)



MAX_SHARDS = 32  # lists per query of the merge kernel


def place(capacities, fills, n):
  """Where `add` puts n new items: (shard capacities, items held per shard, n) -> [(shard, count), ...] in item order.  The
  chunk goes to the shard that holds the fewest items among those with room (the lowest number on a tie) and what does not
  fit there spills to the next such shard, and so on.  Raises ValueError if the shards' free rows together are fewer than
  n.  Pure: the arguments are not changed."""
  fills = list(fills)
  if n > sum(c - f for c, f in zip(capacities, fills)):
    raise ValueError('%d items do not fit (%d of %d in use)' % (n, sum(fills), sum(capacities)))
  segments = []
  while n > 0:
    s = min((i for i in range(len(fills)) if fills[i] < capacities[i]), key=lambda i: (fills[i], i))
    take = min(n, capacities[s] - fills[s])
    segments.append((s, take))
    fills[s] += take
    n -= take
  return segments


class ShardedSubset:
  """A set of items of a ShardedVideoIndex (ShardedVideoIndex.subset): `parts[s]` is shard s's IndexSubset in its own item
  numbers on its own device (None where the shard holds no allowed item), `mask` the set as bool [num_items] on the primary
  device, `count` the number of allowed items, `num_items` the index size it was built for."""

  def __init__(self, parts, mask, count):
    self.parts, self.mask, self.count = parts, mask, count
    self.num_items, self.device = mask.shape[0], mask.device


class ShardedHubNorm:
  """The querybank normaliser of a ShardedVideoIndex (ShardedVideoIndex.hub_norm): `parts[s]` is shard s's HubNorm in its
  own item numbers on its own device (None for a shard without items); `lse` fp32 [num_items] and `hubs` (bool
  [num_items], or None) in global item order on the primary device; `beta`, `bank_size`, `num_items`, `device`; `kind`
  and `k` as HubNorm's ('csls' from ShardedVideoIndex.csls_norm)."""

  def __init__(self, parts, lse, beta, bank_size, hubs=None, *, kind='softmax', k=None):
    self.parts, self.lse, self.beta, self.bank_size, self.hubs = parts, lse, beta, bank_size, hubs
    self.num_items, self.device = lse.shape[0], lse.device
    self.kind, self.k = kind, k


class _Shard:
  """One shard: an ordinary VideoIndex on its device (None while the shard has no room at all) and its local -> global
  item table.  The table is kept on the primary device: it is written there by `add`, and its readers -- the merge kernel
  and `subset` -- run there, on the stream that wrote it, so no kernel ever follows a pointer into another device."""

  def __init__(self, capacity, m, d, device, dtype, primary):
    self.device = device
    self.capacity = capacity
    self.index = VideoIndex.empty(capacity, m, d, device, dtype=dtype) if capacity else None
    self.ids = torch.empty(capacity, device=primary, dtype=torch.int64)

  @property
  def num_items(self):
    return self.index.num_items if self.index is not None else 0


def _devices(devices):
  if not isinstance(devices, (list, tuple)) or not 1 <= len(devices) <= MAX_SHARDS:
    raise ValueError('ShardedVideoIndex: devices must be a list of 1..%d CUDA devices, got %r' % (MAX_SHARDS, devices))
  out = []
  for dev in devices:
    dev = torch.device(dev)
    if dev.type != 'cuda':
      raise ValueError('ShardedVideoIndex: devices must be CUDA devices, got %s' % dev)
    out.append(dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device()))
  return out


class ShardedVideoIndex(_Index):
  """One gallery held as S = len(devices) VideoIndex shards, one per entry of `devices` (the same device may appear more
  than once), with the surface of VideoIndex.  Item numbers are global insertion order 0 .. num_items - 1; every result is
  bit-identical to that of one VideoIndex over the same items in the same order: score(q, g) has the same bits wherever
  item g is stored, the shards' top-k lists are merged under the global tie rule on the device (mmt_search_merge_lists),
  and a target is scored on the shard that holds it and counted on every shard (mmt_search_thresholds,
  mmt_search_count), the int32 counts summed.  devices[0] is the primary: items to add, queries, targets, `exclude` and
  subset items are given on it and results are returned on it.  One host thread drives all devices; launches and
  cross-device copies are asynchronous, so the shards scan concurrently."""

  def __init__(self, embds, weights, devices, dtype=torch.float32):
    _check_dtype(dtype, _width(embds))
    devices = _devices(devices)
    g, gw = self._items(embds, weights, 'ShardedVideoIndex')
    n, s = g.shape[0], len(devices)
    sizes = [n // s + (i < n % s) for i in range(s)]   # contiguous near-equal ranges
    self._allocate(sizes, n, g.shape[1], g.shape[2], devices, dtype)
    self.add(g, gw)

  @classmethod
  def empty(cls, capacity, num_experts, dim, devices, dtype=torch.float32):
    """Room for `capacity` items and none stored: every shard gets ceil(capacity / S) rows; `add` fills them."""
    _check_dtype(dtype, dim)
    devices = _devices(devices)
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (capacity, num_experts, dim)):
      raise ValueError('ShardedVideoIndex.empty: capacity, num_experts and dim must be ints')
    self = cls.__new__(cls)
    self._allocate([-(-capacity // len(devices))] * len(devices), capacity, num_experts, dim, devices, dtype)
    return self

  def _allocate(self, sizes, capacity, m, d, devices, dtype):
    mult = _DTYPES[dtype]
    if capacity < 1 or capacity >= 2 ** 31 or not 1 <= m <= 16 or d < mult or d % mult:
      raise ValueError('ShardedVideoIndex: need 1 <= capacity < 2^31, 1 <= M <= 16 and d %% %d == 0 for %s, got (%d, %d, %d)'
                       % (mult, dtype, capacity, m, d))
    self.capacity, self.num_experts, self.dim = capacity, m, d
    self.num_items = 0
    self.devices, self.device, self.dtype = devices, devices[0], dtype
    self.shards = [_Shard(size, m, d, dev, dtype, devices[0]) for size, dev in zip(sizes, devices)]
    # global item -> (shard, local item), on the primary: exclusions, targets and subsets are translated there
    self._shard_of = torch.empty(capacity, device=self.device, dtype=torch.int64)
    self._local_of = torch.empty(capacity, device=self.device, dtype=torch.int64)
    self._table_cache = {}

  @property
  def shard_sizes(self):
    return [sh.num_items for sh in self.shards]

  @property
  def nbytes(self):
    """Bytes held: the shards' storage, their item tables and the primary's item map, at full capacity."""
    return (sum(sh.index.nbytes for sh in self.shards if sh.index is not None) + 8 * sum(sh.capacity for sh in self.shards) +
            16 * self.capacity)

  def add(self, embds, weights):
    """Appends items (n, M, d) / (n, M) given on the primary device; they get the next n global numbers.  Placement is
    `place`: the shard with the fewest items first, spilling when it is full.  Returns (first, last).  Raises ValueError,
    leaving the index as it was, if they do not fit."""
    g, gw = self._items(embds, weights, 'ShardedVideoIndex.add')
    n, m, d = g.shape
    if (m, d) != (self.num_experts, self.dim):
      raise ValueError('ShardedVideoIndex.add: items (n, %d, %d) expected, got %s' % (self.num_experts, self.dim, tuple(g.shape)))
    if g.device != self.device or gw.device != self.device:
      raise ValueError('ShardedVideoIndex.add: items must be on the primary device %s' % self.device)
    first, last = self.num_items, self.num_items + n
    if last > self.capacity:
      raise ValueError('ShardedVideoIndex.add: %d items do not fit (%d of %d in use)' % (n, first, self.capacity))
    segments = place([sh.capacity for sh in self.shards], self.shard_sizes, n)
    at = 0
    for s, count in segments:
      sh = self.shards[s]
      lo, hi = sh.index.add(g[at:at + count].to(sh.device), gw[at:at + count].to(sh.device))
      sh.ids[lo:hi] = torch.arange(first + at, first + at + count, device=self.device)
      self._shard_of[first + at:first + at + count] = s
      self._local_of[first + at:first + at + count] = torch.arange(lo, hi, device=self.device)
      at += count
    self.num_items = last
    return first, last

  def _tables(self, shards, item_pooling=None):
    """The addresses of the given shards' item tables -- with an item pooling: of its set tables -- as a device array on
    the primary, where the tables themselves are: the `ids` of the merge kernels.  Built once per owner and shard tuple."""
    cache = (self if item_pooling is None else item_pooling)._table_cache
    if shards not in cache:
      tables = [sh.ids for sh in self.shards] if item_pooling is None else item_pooling.tables
      cache[shards] = torch.tensor([tables[s].data_ptr() for s in shards], dtype=torch.int64).to(self.device)
    return cache[shards]

  def _live(self, subset=None):
    """(number, shard) of the shards that hold items -- with a subset: allowed items."""
    return [(s, sh) for s, sh in enumerate(self.shards) if sh.num_items and (subset is None or subset.parts[s] is not None)]

  def _local(self, items, s, maps=None):
    """Global item numbers (-1 = none) on the primary -> shard s's numbers, -1 for none and for items held elsewhere.
    maps: (global -> shard, global -> local) in place of the item maps: an item pooling's set maps."""
    shard_of, local_of = (self._shard_of, self._local_of) if maps is None else maps
    at = items.clamp(min=0)
    return torch.where((items >= 0) & (shard_of[at] == s), local_of[at], torch.full_like(items, -1))

  def _first(self, first, s):
    """The cursor's `first` (the lowest GLOBAL item number still admitted at the cursor's score, -1 = a sentinel) on the
    primary -> shard s's: the count of its items numbered below it -- searchsorted(ids_s, cursor item, right=True) on the
    shard's increasing local -> global table -- which may be 0 or the shard's item count.  -1 stays -1."""
    ids = self.shards[s].ids[:self.shards[s].num_items]
    return torch.where(first >= 0, torch.searchsorted(ids, (first - 1).clamp(min=0), right=True), first)

  _item_pooling_type = ShardedItemPooling

  def item_pooling(self, set_size, item_weights=None, mode='mean'):
    """As VideoIndex.item_pooling, item_weights in global item order on the primary -> ShardedItemPooling.  Accepted when
    every set is stored whole on one shard, in order, starting at a local item number that is a multiple of set_size
    (checked from the item maps with one reduction; ValueError otherwise).  To fill an index so that this holds: `.empty`
    with a capacity of len(devices) * n * set_size, so that every shard's capacity is a multiple of set_size, then `add`
    in pieces of whole sets that fit one shard (a piece that spills is cut at the shard's free rows, a multiple of
    set_size, so its sets stay whole too).  Each shard gets its own ItemPooling in local set numbers and a local-set ->
    global-set table on the primary, so results are bit-identical to one VideoIndex."""
    num_sets, w = _check_item_sets('item_pooling', set_size, self.num_items, item_weights, mode, self.device)
    n = self.num_items
    if not bool(sets_whole(self._shard_of[:n], self._local_of[:n], set_size)):
      raise ValueError('item_pooling: a set of %d items is split across shards or starts off a multiple of %d there'
                       % (set_size, set_size))
    parts, tables = [], []
    for sh in self.shards:
      part, table = None, None
      if sh.num_items:
        ids = sh.ids[:sh.num_items]
        table = ids[::set_size] // set_size          # on the primary, where the item table is
        with torch.cuda.device(sh.device):
          part = ItemPooling(set_size, sh.num_items // set_size, w[ids].to(sh.device), mode)
      parts.append(part)
      tables.append(table)
    return ShardedItemPooling(set_size, num_sets, w, mode, parts, tables, self._shard_of[:n:set_size].clone(),
                              self._local_of[:n:set_size] // set_size)

  def subset(self, items):
    """items: bool [num_items] or int64 item numbers on the primary device, as VideoIndex.subset -> ShardedSubset: the set
    cut into one IndexSubset per shard, in the shard's own numbers.  After a further `add` it is refused."""
    return _cut_subset(*self._subset_mask(items),
                       [(sh.ids[:sh.num_items] if sh.num_items else None, sh.device) for sh in self.shards])

  def _subset(self, subset, who, item_pooling=None):
    self._made_here(subset, who, 'subset', ShardedSubset, 'ShardedVideoIndex.subset', item_pooling)

  def _norm(self, norm, who):
    self._made_here(norm, who, 'norm', ShardedHubNorm, 'ShardedVideoIndex.hub_norm')

  def _hub_norm(self, b, bw, beta, hubs):
    """`hub_norm` behind its checks -> ShardedHubNorm: the bank (given on the primary) is copied to every shard, which
    computes the lse of its own items; lse[g] does not depend on where item g is stored, so `lse` -- and every result under
    norm= -- is bit-identical to that of one VideoIndex."""
    lse = torch.empty(self.num_items, device=self.device, dtype=torch.float32)
    parts = []
    for sh in self.shards:
      part = None
      if sh.num_items:
        ids = sh.ids[:sh.num_items]
        with torch.cuda.device(sh.device):
          mine = sh.index._col_lse(b.to(sh.device), bw.to(sh.device), beta)
          part = HubNorm(mine, beta, b.shape[0], None if hubs is None else hubs[ids].to(sh.device))
        lse[ids] = mine.to(self.device)
      parts.append(part)
    return ShardedHubNorm(parts, lse, beta, b.shape[0], hubs)

  def _row_expsum(self, q, qw, beta, xmax, bits, scan):
    """The sum pass of `query_lse` behind its checks: q, qw and xmax (the merged top-1 times beta) on the primary, bits from
    the global item count.  Every shard that holds candidates sums over its own items with its part of the subset; the
    int64 partials are added on the primary -- integers, so the order of the shards does not matter."""
    with torch.cuda.device(self.device):
      sums = torch.zeros(q.shape[0], device=self.device, dtype=torch.int64)
    for s, sh in self._live(scan.subset):
      with torch.cuda.device(sh.device):
        mine = sh.index._row_expsum(q.to(sh.device), qw.to(sh.device), beta, xmax.to(sh.device), bits, scan.shard(s, self))
      sums += mine.to(self.device)
    return sums

  def _per_item(self, run, outs):
    """Fills outs -- per-item tensors [num_items, ...] on the primary -- from the shards: run(sh), called under the device
    of every shard that holds items, gives that shard's tensors in its own item order; they are scattered to global item
    order through sh.ids[:sh.num_items], as `_hub_norm` does with lse.  -> the shards' own results, None for an empty
    shard."""
    parts = []
    for sh in self.shards:
      part = None
      if sh.num_items:
        ids = sh.ids[:sh.num_items]
        with torch.cuda.device(sh.device):
          part = run(sh)
        for out, mine in zip(outs, part):
          out[ids] = mine.to(self.device)
      parts.append(part)
    return parts

  def _reverse_search(self, q, qw, k):
    """`reverse_search` behind its checks: every shard reverse-searches its own items with all the query rows, copied to
    its device; a list depends on its item and the rows only, so the lists, scattered to global item order on the
    primary, are bit-identical to those of one VideoIndex."""
    outs = _lists(2, self.device, self.num_items, k)
    self._per_item(lambda sh: sh.index._reverse_search(q.to(sh.device), qw.to(sh.device), k), outs)
    return outs

  def _csls_norm(self, b, bw, k, hubs):
    """`csls_norm` behind its checks -> ShardedHubNorm, as `_hub_norm`: one 'csls' HubNorm per shard, r in global order."""
    r = torch.empty(self.num_items, device=self.device, dtype=torch.float32)
    kk = min(k, b.shape[0])
    means = self._per_item(lambda sh: (sh.index._col_topk(b.to(sh.device), bw.to(sh.device), kk, True)[2],), (r,))
    parts = []
    for sh, mine in zip(self.shards, means):
      part = None
      if mine is not None:
        with torch.cuda.device(sh.device):
          part = HubNorm(mine[0], 2.0, b.shape[0], None if hubs is None else hubs[sh.ids[:sh.num_items]].to(sh.device),
                         kind='csls', k=k)
      parts.append(part)
    return ShardedHubNorm(parts, r, 2.0, b.shape[0], hubs, kind='csls', k=k)

  def _merged(self, outs, live, kin, merge, tables, lists):
    """Fills outs -- result lists [NQ, kout] on the primary -- from the live shards: lists(s, sh), called under shard s's
    device, gives its lists, at most kin wide, in its own numbers; they are staged on the primary (the slots a shorter
    list leaves are empty) and merged there in one launch of `merge` through `tables`, the shards' local -> global tables."""
    nq, kout = outs[0].shape
    with torch.cuda.device(self.device):
      staged = _lists(len(outs), self.device, len(live), nq, kin, vacant=True)
    for i, (s, sh) in enumerate(live):
      with torch.cuda.device(sh.device):
        part = lists(s, sh)
      for st, mine in zip(staged, part):
        st[i, :, :mine.shape[1]].copy_(mine)
    with torch.cuda.device(self.device):
      check(getattr(_lib.lib(), merge)(*[ops._p(st) for st in staged], ops._p(tables), len(live), nq, kin, kout,
                                       *[ops._p(o) for o in outs], ops._stream()), merge)
    return outs

  def _search(self, q, qw, k, scan):
    """`search` behind its checks: q, qw and the scan's exclusions (global numbers) on the primary, its parts this index's
    own.  Every live shard searches with its view of the scan -- with a pooling it gets all the rows and returns one list
    per set, with an item pooling it searches its own sets and the merge goes through the set tables."""
    kout = min(k, scan.candidates(self))
    outs = _lists(2, self.device, scan.rows(q), kout)
    if q.shape[0] == 0:
      return outs
    live = self._live(scan.subset)
    views = {s: scan.shard(s, self) for s, _ in live}
    kin = min(kout, max(views[s].candidates(sh.index) for s, sh in live))
    return self._merged(outs, live, kin, 'mmt_search_merge_lists', self._tables(tuple(views), scan.item_pooling),
                        lambda s, sh: sh.index._search(q.to(sh.device), qw.to(sh.device), kout, views[s]))

  def _rescore(self, q, qw, cand, k):
    """`rescore` behind its checks: q, qw and cand (global numbers) on the primary.  Every shard that holds items re-scores
    the candidates it holds -- the others are -1, none, in its view -- and returns them best first in its own numbers;
    an item lives on one shard, so the merge has nothing to de-duplicate, and it keeps a slot without a candidate vacant
    (an index of -1 is an empty slot of its input lists)."""
    outs = _lists(2, self.device, q.shape[0], k)
    live = self._live()
    local = {s: self._local(cand, s) for s, _ in live}  # translated on the primary, where the item maps are
    lists = lambda s, sh: sh.index._rescore(q.to(sh.device), qw.to(sh.device), local[s].to(sh.device), k)
    return self._merged(outs, live, k, 'mmt_search_merge_lists', self._tables(tuple(s for s, _ in live)), lists)

  def _pair_scores(self, cand, sims):
    """`pair_scores` behind its checks, one row batch: cand (global numbers) and sims on the primary.  The stored rows of
    two candidates may lie on different shards, so every shard copies the stored bytes, weights and scales of the batch's
    distinct candidates it holds into a staging VideoIndex on the primary (item j of it is the j-th smallest distinct
    candidate); the candidates are renumbered into it and the one kernel runs there.  sim depends on the two stored rows,
    their weights and scales alone, so the bits are those of one VideoIndex.  The staging's size is the one wait for the
    device."""
    live = cand >= 0
    distinct = torch.unique(cand[live])   # ascending
    n = distinct.numel()
    if n == 0:
      sims.fill_(float('nan'))
      return
    with torch.cuda.device(self.device):
      staging = VideoIndex.empty(n, self.num_experts, self.dim, self.device, dtype=self.dtype)
    stored = staging.folded.view(torch.uint8)   # bytes: a copy, whatever the dtype
    where, local = self._shard_of[distinct], self._local_of[distinct]
    for s, sh in self._live():
      at = torch.nonzero(where == s).reshape(-1)
      if at.numel() == 0:
        continue
      with torch.cuda.device(sh.device):
        rows = local[at].to(sh.device)
        parts = [sh.index.folded.view(torch.uint8)[rows], sh.index.weights[rows],
                 None if sh.index.scales is None else sh.index.scales[rows]]
      stored[at] = parts[0].to(self.device)
      staging.weights[at] = parts[1].to(self.device)
      if parts[2] is not None:
        staging.scales[at] = parts[2].to(self.device)
    staging.num_items = n
    renumbered = torch.where(live, torch.searchsorted(distinct, cand.clamp(min=0)), torch.full_like(cand, -1))
    staging._pair_scores(renumbered, sims)

  def _expert_parts(self, q, qw, cand):
    """`expert_scores` and `pair_expert_scores` behind their checks: q, qw and cand (global numbers) on the primary.  Every
    shard that holds items gets the rows and the candidates in its own numbers -- what it does not hold is -1, none, and
    comes back NaN -- and the primary takes each pair from the shard that owns it.  A pair's values depend on the pair
    alone, so the bits are those of one VideoIndex."""
    out = None
    for s, sh in self._live():
      local = self._local(cand, s)   # translated on the primary, where the item maps are
      with torch.cuda.device(sh.device):
        mine = sh.index._expert_parts(q.to(sh.device), qw.to(sh.device), local.to(sh.device))
      mine = tuple(t.to(self.device) for t in mine)
      own = (local >= 0).unsqueeze(-1)
      out = mine if out is None else tuple(torch.where(own, a, b) for a, b in zip(mine, out))
    return out

  def _stored_rows(self, items):
    """As VideoIndex._stored_rows, items in global numbers on the primary: the rows' stored bytes, weights and scales are
    gathered from their shards onto the primary (`_stage`) and dequantised there."""
    stored, weights, scales = self._stage(items)
    with torch.cuda.device(self.device):
      return _dequantised(stored, self.dtype, scales), weights

  def _stage_batches(self, r):
    """Row ranges of the self-join's staging blocks: whole 64-row blocks whose stored bytes, weights and scales stay
    within _BATCH_BYTES."""
    per_row = self.num_experts * self.dim * torch.empty(0, dtype=self.dtype).element_size() + 4 * self.num_experts + 4
    batch = max(64, (_BATCH_BYTES // per_row) // 64 * 64)
    return [(r0, min(r, r0 + batch)) for r0 in range(0, r, batch)]

  def _stage(self, part):
    """The staging block of the self-join: the stored bytes, weights and scales of the items `part` (int64 [n] global
    numbers on the primary, repeats allowed), gathered from the shards that hold them -> (bytes uint8 [n, row bytes],
    weights float32 [n, M], scales float32 [n] or None) on the primary, row j = item part[j]."""
    n, m = part.shape[0], self.num_experts
    row_bytes = m * self.dim * torch.empty(0, dtype=self.dtype).element_size()
    with torch.cuda.device(self.device):
      stored = torch.empty(n, row_bytes, device=self.device, dtype=torch.uint8)
      weights = torch.empty(n, m, device=self.device, dtype=torch.float32)
      scales = torch.empty(n, device=self.device, dtype=torch.float32) if self.dtype == FP8 else None
    where, local = self._shard_of[part], self._local_of[part]
    for s, sh in self._live():
      at = torch.nonzero(where == s).reshape(-1)
      if at.numel() == 0:
        continue
      with torch.cuda.device(sh.device):
        rows = local[at].to(sh.device)
        parts = [sh.index.folded.view(torch.uint8)[rows], sh.index.weights[rows],
                 None if scales is None else sh.index.scales[rows]]
      stored[at] = parts[0].to(self.device)
      weights[at] = parts[1].to(self.device)
      if scales is not None:
        scales[at] = parts[2].to(self.device)
    return stored, weights, scales

  def _staged(self, items, r0, r1, thr, subset, live):
    """What every live shard runs a self-join entry with for rows r0 .. r1 - 1: {shard: (the staging block on its device
    as the A side, the rows' local numbers there or -1, the rows' thresholds or None, its part of the subset)}."""
    part = items[r0:r1]
    block = self._stage(part)
    out = {}
    for s, sh in live:
      with torch.cuda.device(sh.device):
        a = tuple(None if t is None else t.to(sh.device) for t in block) + (r1 - r0,)
        out[s] = (a, self._local(part, s).to(sh.device), None if thr is None else thr[r0:r1].to(sh.device),
                  None if subset is None else subset.parts[s])
    return out

  def _neighbours(self, rows, items, own, k, subset, outs):
    """`neighbours` behind its checks: items (global numbers) and outs on the primary.  Per row batch the rows' stored
    bytes, weights and scales are gathered from their shards into a staging block, the block is copied to every shard's
    device, every shard runs the one entry with A = the block, B = its own items and self = the row's local number there
    or -1, and the lists are renumbered and merged on the primary (mmt_search_merge_lists).  sim depends on the two
    stored rows alone, so the bits are those of one VideoIndex."""
    live = self._live(subset)
    tables = self._tables(tuple(s for s, _ in live))
    for r0, r1 in self._stage_batches(items.shape[0]):
      staged = self._staged(items, r0, r1, None, subset, live)

      def lists(s, sh):
        a, local, _, part = staged[s]
        mine = _lists(2, sh.device, r1 - r0, k, vacant=True)
        sh.index._self_topk(a, None, local, k, part, mine)
        return mine
      self._merged(tuple(o[r0:r1] for o in outs), live, k, 'mmt_search_merge_lists', tables, lists)

  def _neighbour_range(self, rows, items, own, thr, subset, order, max_hits, who, spent=0):
    """`neighbour_range` behind its checks, over all shards (`_range_csr`): a batch is a staging batch of the rows' stored
    bytes, staged once for the count and again for the fill."""
    live = self._live(subset)
    return self._range_csr(items.shape[0], live, self._stage_batches(items.shape[0]),
                           lambda r0, r1: self._staged(items, r0, r1, thr, subset, live),
                           lambda sh, mine: sh.index._self_range_count(mine[0], None, *mine[1:]),
                           lambda sh, mine, *outs: sh.index._self_range_fill(mine[0], None, *mine[1:], *outs),
                           order, max_hits, who, spent)

  def _range_csr(self, r, live, batches, stage, count, fill, order, max_hits, who, spent=0):
    """The CSR of a range scan of r rows over all shards, assembled as VideoIndex._csr assembles one index's: per batch
    (r0, r1) of `batches`, stage(r0, r1) -> {shard: its operands} and every shard counts the hits among its own items
    (count(shard, operands) -> (hits per row, workspaces)); the totals are summed on the primary -- the call's one wait for
    the devices -- and held against max_hits (spent: the hits an enclosing call has already used of it) before any shard
    allocates its outputs; the batches are staged again, every shard fills a CSR of its own (fill(shard, operands,
    workspaces, offsets, indices, scores)), whose local numbers go through its table to global ones, and the primary orders
    the hits by (row, global item) with two stable torch sorts."""
    counted = {}
    for b, (r0, r1) in enumerate(batches):
      staged = stage(r0, r1)
      for s, sh in live:
        with torch.cuda.device(sh.device):
          counted[b, s] = count(sh, staged[s])
    with torch.cuda.device(self.device):
      per_shard = torch.zeros(len(live), r, device=self.device, dtype=torch.int64)
      for b, (r0, r1) in enumerate(batches):
        for i, (s, _) in enumerate(live):
          per_shard[i, r0:r1] = counted[b, s][0].to(self.device)
      cells = [per_shard[:, r0:r1].sum(1) for r0, r1 in batches]
      cells = torch.stack(cells).tolist() if cells else []   # [batch][shard]: the call's one wait for the devices
      total = sum(sum(c) for c in cells)
      if spent + total > max_hits:
        raise ValueError('%s: %d hits exceed max_hits = %d' % (who, spent + total, max_hits))
      offsets = torch.zeros(r + 1, device=self.device, dtype=torch.int64)
      if r:
        torch.cumsum(per_shard.sum(0), 0, out=offsets[1:])
    at, hit, sims = [], [], []
    for b, (r0, r1) in enumerate(batches):
      if not any(cells[b]):
        continue
      staged = stage(r0, r1)
      for i, (s, sh) in enumerate(live):
        if not cells[b][i]:
          continue
        with torch.cuda.device(sh.device):
          local = torch.zeros(r1 - r0 + 1, device=sh.device, dtype=torch.int64)
          torch.cumsum(counted[b, s][0], 0, out=local[1:])
          idx = torch.empty(cells[b][i], device=sh.device, dtype=torch.int64)
          sc = torch.empty(cells[b][i], device=sh.device, dtype=torch.float32)
          fill(sh, staged[s], counted[b, s][1], local, idx, sc)
        at.append(_csr_rows(local.to(self.device)) + r0)
        hit.append(sh.ids[idx.to(self.device)])
        sims.append(sc.to(self.device))
    with torch.cuda.device(self.device):
      if not at:
        return RangeResult(offsets, torch.empty(0, device=self.device, dtype=torch.int64),
                           torch.empty(0, device=self.device, dtype=torch.float32))
      at, hit, sims = torch.cat(at), torch.cat(hit), torch.cat(sims)
      by_item = torch.argsort(hit, stable=True)
      perm = by_item[torch.argsort(at[by_item], stable=True)]
      return _range_result(offsets, hit[perm], sims[perm], order)

  def grouping(self, group_ids):
    """group_ids: int64 [num_items] on the primary device, as VideoIndex.grouping -> ShardedGrouping: the ids cut into one
    IndexGrouping per shard, in the shard's item order, with the ids as given -- they are global, so a group may have
    members on several shards.  After a further `add` it is refused."""
    ids, num_groups = self._group_ids(group_ids)
    parts = []
    for sh in self.shards:
      part = None
      if sh.num_items:
        local = ids[sh.ids[:sh.num_items]]  # gathered on the primary, where the table is
        with torch.cuda.device(sh.device):
          local = local.to(sh.device)
          part = IndexGrouping(local, _count_groups(local))
      parts.append(part)
    return ShardedGrouping(parts, ids, num_groups)

  def _grouping(self, grouping, who):
    self._made_here(grouping, who, 'grouping', ShardedGrouping, 'ShardedVideoIndex.grouping')

  _tagging_type = ShardedTagging

  def tagging(self, tags):
    """tags: int64 [num_items] on the primary device, as VideoIndex.tagging -> ShardedTagging: the tags cut into one
    IndexTagging per shard, in the shard's item order on its device.  After a further `add` it is refused."""
    tags = self._tags(tags)
    parts = []
    for sh in self.shards:
      part = None
      if sh.num_items:
        local = tags[sh.ids[:sh.num_items]]  # gathered on the primary, where the table is
        with torch.cuda.device(sh.device):
          part = IndexTagging(local.to(sh.device))
      parts.append(part)
    return ShardedTagging(parts, tags)

  _cells_type = ShardedCells

  def cells(self, cell_ids, num_cells=None):
    """cell_ids: int64 [num_items] on the primary device, as VideoIndex.cells -> ShardedCells: every shard gets the
    restriction of each cell to the items it holds, in its own numbers (a shard's item table is increasing, so a cell's
    items ascend there as they do globally).  After a further `add` it is refused."""
    ids, num_cells = self._cell_ids(cell_ids, num_cells)
    parts = []
    for sh in self.shards:
      part = None
      if sh.num_items:
        local = ids[sh.ids[:sh.num_items]]  # gathered on the primary, where the table is
        with torch.cuda.device(sh.device):
          part = IndexCells(sh.index, *self._cell_csr(local.to(sh.device), num_cells), sh.num_items)
      parts.append(part)
    return ShardedCells(self, *self._cell_csr(ids, num_cells), self.num_items, parts)

  @staticmethod
  def _float_sums_refused(who, instead):
    """The fp32 sums depend on the order of a cell's list, which no placement of the items over shards preserves: only
    the exact integer sums can be bit-identical to one VideoIndex, so here they have to be asked for by name."""
    raise ValueError('%s: not available on a ShardedVideoIndex with the fp32 accumulator, whose sums depend on the order '
                     'of the additions; %s' % (who, instead))

  def cell_sums(self, *args, **kwargs):
    """Refused: the fp32 sums are not order-independent.  `cell_sums_exact` is the sharded form."""
    self._float_sums_refused('cell_sums', 'call cell_sums_exact(cells), whose integer sums add across shards')

  def cell_centroids(self, cells=None, out=None, exact=False, scale=None, **unsupported):
    """VideoIndex.cell_centroids(cells, out, exact=True, scale) on cells of this index, out on the primary -> bit-identical
    to one VideoIndex over the same items, however they are placed: `cell_sums_exact`, then the finish on the primary
    (mmt_search_cell_centroids_exact).  Without exact=True it raises ValueError."""
    self._not_trained('cell_centroids', unsupported)
    self._exact_flag('cell_centroids', exact, scale)
    if not exact:
      self._float_sums_refused('cell_centroids', 'pass exact=True for the integer sums, which add across shards')
    self._cells(cells, 'cell_centroids')
    scale = self._scale(scale, 'cell_centroids')
    return self._exact_centroids(cells, self._centroid_out(cells, out), scale)

  def train_cells(self, num_cells=None, iters=10, init=None, seed=0, items=None, exact=False, **unsupported):
    """VideoIndex.train_cells(..., exact=True) over the shards -> a CellQuantiser on the primary, bit-identical to one
    VideoIndex over the same items in every part: centroids, objective, moved, iterations.  init and items are global item
    numbers on the primary.  The assignment runs shard by shard against a copy of the centroids on the shard's device
    (`assign_cells` describes it), the update is `cell_centroids(exact=True)`.  Without exact=True it raises ValueError."""
    self._not_trained('train_cells', unsupported)
    self._exact_flag('train_cells', exact)
    if not exact:
      self._float_sums_refused('train_cells', 'pass exact=True for the integer sums, which add across shards')
    return self._train_cells(num_cells, iters, init, seed, items, True)

  def _absmax(self):
    """The largest magnitudes over the shards, float32 [2] on the primary: a maximum of maxima."""
    parts = [sh.index._absmax().to(self.device) for _, sh in self._live()]
    with torch.cuda.device(self.device):
      return torch.stack(parts).amax(0)

  def _exact_sums(self, cells, scale):
    """`cell_sums_exact` behind its checks: every shard that holds labelled items sums its part of the cells under the
    GLOBAL scale on its own device; the int64 results are copied to the primary and added there -- integers, so neither
    the placement nor the order of the shards matters."""
    c, m, d = cells.num_cells, self.num_experts, self.dim
    with torch.cuda.device(self.device):
      sums = torch.zeros(c, m * d, device=self.device, dtype=torch.int64)
      wsums = torch.zeros(c, m, device=self.device, dtype=torch.int64)
    for s, sh in self._live():
      if cells.parts[s].items.shape[0]:
        mine, wmine = sh.index._exact_sums(cells.parts[s], scale)
        with torch.cuda.device(self.device):
          sums += mine.to(self.device)
          wsums += wmine.to(self.device)
    return sums, wsums

  def _assign(self, embds, weights, train):
    """The assignment step over the shards: centroids on the primary and the training items (global numbers, int64
    ascending on the primary, None = every item) -> (scores [T, 1], cells [T, 1]) on the primary in the order of the
    training items.  One VideoIndex of the centroids per distinct device, in the gallery's dtype; every shard's part of
    the sample -- its local numbers, ascending as the global ones are -- is assigned by centroids.neighbours(k=1,
    source=shard.index, items=...) and the rows are scattered to their places.  With a sample, finding a shard's part
    waits for the device once per shard."""
    total = self.num_items if train is None else train.shape[0]
    with torch.cuda.device(self.device):
      scores = torch.empty(total, 1, device=self.device, dtype=torch.float32)
      best = torch.empty(total, 1, device=self.device, dtype=torch.int64)
    centroids = {}
    for s, sh in self._live():
      if train is None:
        at, local = sh.ids[:sh.num_items], None
      else:
        at = torch.nonzero(self._shard_of[train] == s)[:, 0]
        if at.shape[0] == 0:
          continue
        local = self._local_of[train[at]].to(sh.device)
      with torch.cuda.device(sh.device):
        if sh.device not in centroids:
          centroids[sh.device] = VideoIndex(embds.to(sh.device), weights.to(sh.device), dtype=self.dtype)
        mine, cell = centroids[sh.device].neighbours(k=1, source=sh.index, items=local)
      with torch.cuda.device(self.device):
        scores[at] = mine.to(self.device)
        best[at] = cell.to(self.device)
    return scores, best

  def _search_probed(self, q, qw, cells, probes, k):
    """`search_probed` behind its checks: q, qw and probes on the primary.  Every shard that holds items of a cell answers
    for the same probes over its part of the cells and returns its lists in its own numbers, the slots it cannot fill
    vacant; an item lives on one shard, and the merge applies the global tie rule (mmt_search_merge_lists)."""
    outs = _lists(2, self.device, q.shape[0], k)
    live = [(s, sh) for s, sh in self._live() if cells.parts[s].items.shape[0]]
    lists = lambda s, sh: sh.index._search_probed(q.to(sh.device), qw.to(sh.device), cells.parts[s],
                                                  probes.to(sh.device), k)
    return self._merged(outs, live, k, 'mmt_search_merge_lists', self._tables(tuple(s for s, _ in live)), lists)

  def _search_groups(self, q, qw, k, grouping, subset):
    """`search_groups` behind its checks: q, qw on the primary, 1 <= k <= grouping.num_groups.  Every live shard returns its
    best min(k, its groups) groups; the merge on the primary keeps one entry per group."""
    outs = _lists(3, self.device, q.shape[0], k)
    if q.shape[0] == 0:
      return outs
    scan, live = _Scan(subset), self._live(subset)
    kin = min(k, max(grouping.parts[s].num_groups for s, _ in live))

    def lists(s, sh):
      part = grouping.parts[s]
      return sh.index._search_groups(q.to(sh.device), qw.to(sh.device), min(k, part.num_groups), part,
                                     scan.shard(s, self).subset)
    return self._merged(outs, live, kin, 'mmt_search_merge_group_lists', self._tables(tuple(s for s, _ in live)), lists)

  def _rank_counts(self, q, qw, tg, scan):
    """`rank_counts` behind its checks: tg int64 [NQ, T] global numbers on the primary -> (greater, equal) int32 [NQ, T];
    with a pooling tg is [num_sets, T] and every shard gets all the rows; with an item pooling tg holds global set
    numbers, translated through its set maps.  A target is scored by the shard that holds it and counted by every shard
    that has candidates."""
    live = self._live()
    maps = None if scan.item_pooling is None else scan.item_pooling._maps
    queries, views = {}, {}
    thr = torch.full(tg.shape, float('nan'), device=self.device, dtype=torch.float32)
    for s, sh in live:
      local = self._local(tg, s, maps)
      queries[s], views[s] = (q.to(sh.device), qw.to(sh.device)), scan.shard(s, self)
      with torch.cuda.device(sh.device):
        mine = sh.index._target_scores(*queries[s], local.to(sh.device), views[s])
      thr = torch.where(local >= 0, mine.to(self.device), thr)
    greater = torch.zeros(tg.shape, device=self.device, dtype=torch.int32)
    equal = torch.zeros(tg.shape, device=self.device, dtype=torch.int32)
    for s, sh in live:
      if scan.subset is not None and views[s].subset is None:
        continue  # no allowed item here: nothing to count
      with torch.cuda.device(sh.device):
        gs, es = sh.index._threshold_counts(*queries[s], thr.to(sh.device), views[s])
      greater += gs.to(self.device)
      equal += es.to(self.device)
    return greater, equal

  def range_search(self, embds, weights, threshold, subset=None, order='index', max_hits=_MAX_HITS, where=None):
    """VideoIndex.range_search over all shards -> RangeResult on the primary, in global item numbers, bit-identical to that
    of one VideoIndex.  Every shard counts the hits among its own items (with its part of the subset); the shards' totals
    are summed on the primary -- the call's one wait for the devices -- and held against max_hits before any shard
    allocates its outputs; every shard then fills a CSR of its own, whose local item numbers go through the shard's table
    to global ones; the primary concatenates the shards' hits and orders them by (query, global item) with two stable
    torch sorts.  order='score' as VideoIndex.range_search.  Exclusions are applied to the CSR by the caller.  where: every
    shard filters with its part of the tagging and the masks on its device."""
    q, qw, thr = self._range_args(embds, weights, threshold, subset, order, max_hits, where)
    scan, live, args = _Scan(subset, where=where), self._live(subset), {}

    def stage(r0, r1):  # one batch: the queries go to every shard once, for both passes
      for s, sh in live:
        if s not in args:
          view = scan.shard(s, self)
          args[s] = (q.to(sh.device), qw.to(sh.device), thr.to(sh.device), view.subset, view.where)
      return args
    return self._range_csr(q.shape[0], live, [(0, q.shape[0])] if q.shape[0] else [], stage,
                           lambda sh, mine: sh.index._range_count(*mine),
                           lambda sh, mine, *outs: sh.index._range_fill(*mine, *outs), order, max_hits, 'range_search')
