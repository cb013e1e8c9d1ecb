// The item bitmap of the masked scans (search.py: VideoIndex.subset; mmt_search_topk [subset, exclude], mmt_search_rank [subset] and their
// bf16 forms): bit i & 31 of word i >> 5 is item i.  The word count is padded to a multiple of 4, so the 128 bits of one
// scan tile (TK_G = 128 columns, tiles start at multiples of 128) are one aligned 16-byte load; bits at or past NV are 0.
//
//   subset_pack_kernel : mask [NV] bytes (nonzero = allowed) -> words.  A wave takes 64 consecutive items: one ballot,
//                        lane 0 stores its low word and lane 32 its high word.  Every word has exactly one writer, the
//                        padding words included, so the output needs no clearing and the result is reproducible.
#include "search_scan.h"

__global__ __launch_bounds__(256) void subset_pack_kernel(const uint8_t* __restrict__ mask, int NV, int n_words,
                                                          uint32_t* __restrict__ words) {
  const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t word = (i >> 6) * 2 + (lane >> 5);  // n_words is even: both words of a wave are inside or both outside
  const uint64_t bits = __ballot(i < NV && mask[i] != 0);
  if (!(lane & 31) && word < n_words) words[word] = (uint32_t)(bits >> (lane & 32));
}

extern "C" int mmt_search_subset_pack(const uint8_t* mask, int NV, uint32_t* words, void* stream) {
  if (!mask || !words || NV <= 0) return MMT_ERR_ARG;
  if ((uintptr_t)words & 15) return MMT_ERR_ALIGN;
  const int64_t tiles = ((int64_t)NV + TK_G - 1) / TK_G;  // words: 4 per tile; threads: one per bit, 2 tiles per block
  hipLaunchKernelGGL(subset_pack_kernel, dim3((unsigned)((tiles + 1) / 2)), dim3(256), 0, (hipStream_t)stream, mask, NV,
                     (int)(tiles * (TK_G / 32)), words);
  return (int)hipGetLastError();
}
