// K14 recall hits, the per-shard top-k merge and the per-query exclusion
// filter of sorted top-k lists; the loss reduction.
//
// tt_recall_hits restates IndexRecall.__call__
// (/root/reference/pkg/modelling/metrics/index_recall.py:52-58):
//   hits[k] += sum(equal(true_ids[B,1], candidates[:, :k]))
// (every equal position counts, as the reference's reduce_sum does).
//
// tt_topk_merge merges sorted per-shard top-k lists (score desc, index asc)
// into the global top-k with the same order as tf.math.top_k over the
// concatenated candidates (brute_force.py:81): one wave per query, a k-way
// head merge with a wave-wide argmax over the list heads per output slot.
#include "tt_common.h"

namespace tt {
namespace {

constexpr int kMaxKs = 16;

// loss = scale * sum(x[0..n)): one workgroup, thread t sums t, t+1024, ...
// in order, then a fixed-shape LDS tree (deterministic; the reference's
// reduce_sum over the per-example CE, runner.py:78-83 with reduction SUM).
__global__ void __launch_bounds__(1024) sum_kernel(const float* __restrict__ x, int64_t n, float scale,
                                                   float* __restrict__ out) {
  __shared__ float red[1024];
  float acc = 0.0f;
  int64_t i = threadIdx.x;
  for (; i + 3 * 1024 < n; i += 4 * 1024) {
    const float a = x[i], b = x[i + 1024], c = x[i + 2048], d = x[i + 3072];
    acc = ((acc + a) + b) + c;
    acc = acc + d;
  }
  for (; i < n; i += 1024) acc += x[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (static_cast<int>(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0] * scale;
}

struct RecallArgs {
  const int32_t* true_ids;
  const int32_t* cand;
  int64_t batch;
  int32_t k_total;
  int32_t num_ks;
  int32_t ks[kMaxKs];
  unsigned long long* hits;
};

__global__ void __launch_bounds__(256) recall_hits_kernel(const RecallArgs a) {
  __shared__ unsigned long long part[kMaxKs];
  if (threadIdx.x < kMaxKs) part[threadIdx.x] = 0;
  __syncthreads();
  const int64_t b = blockIdx.x * 256ll + threadIdx.x;
  unsigned cnt[kMaxKs];
#pragma unroll
  for (int t = 0; t < kMaxKs; ++t) cnt[t] = 0;
  if (b < a.batch) {
    const int32_t want = a.true_ids[b];
    const int32_t* row = a.cand + b * a.k_total;
    for (int j = 0; j < a.k_total; ++j) {
      if (row[j] == want) {
#pragma unroll
        for (int t = 0; t < kMaxKs; ++t)
          if (t < a.num_ks && j < a.ks[t]) ++cnt[t];
      }
    }
  }
#pragma unroll
  for (int t = 0; t < kMaxKs; ++t) {
    if (t < a.num_ks) {
      unsigned long long s = static_cast<unsigned long long>(wave_sum_i32(static_cast<int>(cnt[t])));
      if (lane_id() == 0 && s) atomicAdd(&part[t], s);
    }
  }
  __syncthreads();
  if (threadIdx.x < a.num_ks && part[threadIdx.x]) atomicAdd(&a.hits[threadIdx.x], part[threadIdx.x]);
}

// Composite ordering key: larger = better (higher score, then lower index).
__device__ __forceinline__ unsigned long long merge_key(float s, int32_t idx) {
  return (static_cast<unsigned long long>(float_order_key(s)) << 32) |
         static_cast<unsigned long long>(0xFFFFFFFFu - static_cast<unsigned>(idx));
}

__global__ void __launch_bounds__(256) topk_merge_kernel(const float* __restrict__ scores,
                                                         const int32_t* __restrict__ idx, int num_lists,
                                                         int64_t n_queries, int k_in, int k_out,
                                                         float* __restrict__ out_s, int32_t* __restrict__ out_i) {
  const int64_t q = blockIdx.x * 4ll + threadIdx.x / kWave;
  if (q >= n_queries) return;
  const int lane = lane_id();
  const int64_t list_stride = n_queries * static_cast<int64_t>(k_in);
  int ptr = 0;  // head position of list `lane`
  const bool owner = lane < num_lists;
  const float* ls = scores + lane * list_stride + q * k_in;
  const int32_t* li = idx + lane * list_stride + q * k_in;
  unsigned long long head = 0;
  float hs = 0.f;
  int32_t hi = 0;
  auto load_head = [&]() {
    if (owner && ptr < k_in) {
      hs = ls[ptr];
      hi = li[ptr];
      head = merge_key(hs, hi);
    } else {
      head = 0;  // exhausted
    }
  };
  load_head();
  for (int o = 0; o < k_out; ++o) {
    unsigned long long best = head;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const unsigned long long other = __shfl_xor(best, m, kWave);
      best = other > best ? other : best;
    }
    if (head == best && head != 0) {  // keys are unique per query (distinct indices)
      out_s[q * k_out + o] = hs;
      out_i[q * k_out + o] = hi;
      ++ptr;
      load_head();
    }
  }
}

// ---- tt_topk_exclude --------------------------------------------------------
// Removes each query's excluded candidates from its sorted list and compacts
// to k_out, in O(k_in + |E_q|) with no sort: the list's indices go into an
// open-addressing hash table in LDS (>= 2 * k_in slots, linear probing,
// value = list position), the exclusions are streamed one per lane and flag
// the positions they hit, and the unflagged entries are compacted in order
// with ballot + popcount prefixes.  The result depends only on membership,
// so the order the LDS atomics land in does not matter.
//
// One group of NW waves per query: NW = 1 runs four queries per 256-thread
// workgroup (each wave on its own LDS region, no workgroup barrier), NW = 4
// one query per workgroup.  The switch point follows from the NW = 1 form's
// LDS: at k_in = 256 a workgroup takes 4 x 3.3 KB, so the 160 KB of a CU
// hold eleven workgroups and the 32-waves-per-CU cap (eight) stays the
// limit; at 512 it would take 26 KB and LDS would cut that to six.  The
// NW = 4 form needs at most 52 KB (k_in = 4096): three workgroups per CU.
constexpr int32_t kPadIndex = 0x7FFFFFFF;
constexpr int kExcludeSmallK = 256;
constexpr int kExcludeMaxK = 4096;

template <int NW>
__device__ __forceinline__ void group_sync() {
  if constexpr (NW == 1) {
    // a wave's LDS operations execute in order; this keeps the compiler from moving them across
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    __syncthreads();
  }
}

// LDS of one group: table [1 << log2p] int, list indices [k_in] int32, flags
// [k_in] bytes, then (16-B aligned) the per-wave kept counts.
inline int exclude_group_bytes(int k_in, int log2p) {
  return static_cast<int>(round_up((int64_t{1} << log2p) * 4 + k_in * 4ll + k_in, 16)) + 16;
}

template <int NW>
__global__ void __launch_bounds__(256) topk_exclude_kernel(const float* __restrict__ scores,
                                                           const int32_t* __restrict__ idx, int64_t n_queries,
                                                           int k_in, int k_out, const int64_t* __restrict__ excl_off,
                                                           const int32_t* __restrict__ excl_idx,
                                                           float* __restrict__ out_s, int32_t* __restrict__ out_i,
                                                           int32_t* __restrict__ n_kept, int log2p, int group_bytes) {
  extern __shared__ __align__(16) unsigned char exclude_lds[];
  constexpr int NT = NW * kWave;
  const int wave = static_cast<int>(threadIdx.x) / kWave;
  const int lane = lane_id();
  const int64_t q = NW == 1 ? blockIdx.x * 4ll + wave : static_cast<int64_t>(blockIdx.x);
  if (q >= n_queries) return;  // NW = 1 only: a whole wave, and no workgroup barrier follows
  const int t = NW == 1 ? lane : static_cast<int>(threadIdx.x);
  const float* ls = scores + q * k_in;
  const int32_t* li = idx + q * k_in;
  float* os = out_s + q * k_out;
  int32_t* oi = out_i + q * k_out;
  const int64_t eb = excl_off[q], ee = excl_off[q + 1];
  if (ee <= eb) {  // nothing to exclude (uniform over the group): the first k_out entries as they are
    for (int j = t; j < k_out; j += NT) {
      os[j] = ls[j];
      oi[j] = li[j];
    }
    if (t == 0 && n_kept) n_kept[q] = k_out;
    return;
  }
  unsigned char* base = exclude_lds + (NW == 1 ? wave * group_bytes : 0);
  const int P = 1 << log2p;
  int* table = reinterpret_cast<int*>(base);
  int32_t* lidx = table + P;
  unsigned char* flag = reinterpret_cast<unsigned char*>(lidx + k_in);
  int* wcnt = reinterpret_cast<int*>(base + group_bytes - 16);
  const unsigned mask = static_cast<unsigned>(P - 1);
  const int shift = 32 - log2p;  // log2p >= 1
  auto slot_of = [&](int32_t v) { return (static_cast<unsigned>(v) * 2654435761u) >> shift; };

  for (int j = t; j < P; j += NT) table[j] = -1;
  for (int j = t; j < k_in; j += NT) {
    lidx[j] = li[j];
    flag[j] = 0;
  }
  group_sync<NW>();
  // at most k_in inserts into >= 2 * k_in slots: every probe sequence ends
  for (int j = t; j < k_in; j += NT) {
    const int32_t v = lidx[j];
    if (v == kPadIndex) continue;
    unsigned s = slot_of(v);
    while (atomicCAS(&table[s], -1, j) != -1) s = (s + 1) & mask;
  }
  group_sync<NW>();
  for (int64_t e = eb + t; e < ee; e += NT) {
    const int32_t v = excl_idx[e];
    if (v < 0 || v == kPadIndex) continue;  // match nothing
    unsigned s = slot_of(v);
    for (;;) {
      const int p = table[s];
      if (p < 0) break;
      if (lidx[p] == v) flag[p] = 1;  // on to the empty slot: a repeated list index is flagged too
      s = (s + 1) & mask;
    }
  }
  group_sync<NW>();

  // each wave compacts one contiguous segment of the list
  const int seg = ((k_in + NW - 1) / NW + kWave - 1) / kWave * kWave;
  const int sb = NW == 1 ? 0 : wave * seg;
  const int se = sb + seg < k_in ? sb + seg : k_in;
  const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int n = 0, total = 0;
  if constexpr (NW > 1) {
    int cnt = 0;
    for (int j0 = sb; j0 < se; j0 += kWave) {
      const int j = j0 + lane;
      cnt += __popcll(__ballot(j < se && !flag[j]));
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int c = wcnt[w];
      n += w < wave ? c : 0;
      total += c;
    }
  }
  for (int j0 = sb; j0 < se && n < k_out; j0 += kWave) {
    const int j = j0 + lane;
    const bool keep = j < se && !flag[j];
    const uint64_t m = __ballot(keep);
    const int p = n + __popcll(m & lt);
    if (keep && p < k_out) {
      os[p] = ls[j];
      oi[p] = lidx[j];
    }
    n += __popcll(m);
  }
  if constexpr (NW == 1) total = n;  // stops counting at k_out: min(k_out, .) below is unaffected
  const int kept = total < k_out ? total : k_out;
  for (int j = kept + t; j < k_out; j += NT) {
    os[j] = -INFINITY;
    oi[j] = kPadIndex;
  }
  if (t == 0 && n_kept) n_kept[q] = kept;
}

}  // namespace
}  // namespace tt

using namespace tt;

extern "C" int tt_recall_hits(const int32_t* true_ids, const int32_t* cand_ids, int64_t batch, int32_t k_total,
                              const int32_t* ks_host, int32_t num_ks, int64_t* hits, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(num_ks >= 1 && num_ks <= kMaxKs, "tt_recall_hits: num_ks=%d outside [1,%d]", num_ks, kMaxKs);
  TT_REQUIRE(ks_host && hits, "tt_recall_hits: NULL ks/hits");
  TT_REQUIRE(batch >= 0 && k_total >= 1, "tt_recall_hits: bad batch/k_total");
  if (batch == 0) return TT_OK;
  TT_REQUIRE(true_ids && cand_ids, "tt_recall_hits: NULL ids");
  RecallArgs a{};
  a.true_ids = true_ids;
  a.cand = cand_ids;
  a.batch = batch;
  a.k_total = k_total;
  a.num_ks = num_ks;
  for (int t = 0; t < num_ks; ++t) {
    TT_REQUIRE(ks_host[t] >= 0, "tt_recall_hits: negative k");
    a.ks[t] = ks_host[t] < k_total ? ks_host[t] : k_total;
  }
  a.hits = reinterpret_cast<unsigned long long*>(hits);
  hipLaunchKernelGGL(recall_hits_kernel, dim3(ceil_div(batch, 256)), dim3(256), 0, to_stream(stream), a);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_sum(const float* x, int64_t n, float scale, float* out, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(n >= 0 && out != nullptr && (n == 0 || x != nullptr), "tt_sum: bad arguments");
  hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(1024), 0, to_stream(stream), x, n, scale, out);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_topk_merge(const float* scores, const int32_t* idx, int32_t num_lists, int64_t n_queries,
                             int32_t k_in, int32_t k_out, float* out_scores, int32_t* out_idx,
                             tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(num_lists >= 1 && num_lists <= kWave, "tt_topk_merge: num_lists=%d outside [1,64]", num_lists);
  TT_REQUIRE(k_in >= 1 && k_out >= 1 && k_out <= static_cast<int64_t>(num_lists) * k_in,
             "tt_topk_merge: need 1 <= k_out <= num_lists*k_in");
  TT_REQUIRE(n_queries >= 0, "tt_topk_merge: negative n_queries");
  if (n_queries == 0) return TT_OK;
  TT_REQUIRE(scores && idx && out_scores && out_idx, "tt_topk_merge: NULL pointer");
  hipLaunchKernelGGL(topk_merge_kernel, dim3(ceil_div(n_queries, 4)), dim3(256), 0, to_stream(stream), scores, idx,
                     num_lists, n_queries, k_in, k_out, out_scores, out_idx);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_topk_exclude(const float* scores, const int32_t* idx, int64_t n_queries, int32_t k_in,
                               int32_t k_out, const int64_t* excl_off, const int32_t* excl_idx, float* out_scores,
                               int32_t* out_idx, int32_t* n_kept, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(k_out >= 1 && k_out <= k_in && k_in <= kExcludeMaxK,
             "tt_topk_exclude: need 1 <= k_out <= k_in <= %d (got k_in=%d, k_out=%d)", kExcludeMaxK, k_in, k_out);
  TT_REQUIRE(n_queries >= 0 && n_queries <= INT32_MAX, "tt_topk_exclude: n_queries outside [0, 2^31)");
  if (n_queries == 0) return TT_OK;
  TT_REQUIRE(scores && idx && excl_off && out_scores && out_idx, "tt_topk_exclude: NULL pointer");
  int log2p = 1;
  while ((1 << log2p) < 2 * k_in) ++log2p;
  const int group_bytes = exclude_group_bytes(k_in, log2p);
  if (k_in <= kExcludeSmallK) {
    hipLaunchKernelGGL(topk_exclude_kernel<1>, dim3(ceil_div(n_queries, 4)), dim3(256), 4 * group_bytes,
                       to_stream(stream), scores, idx, n_queries, k_in, k_out, excl_off, excl_idx, out_scores,
                       out_idx, n_kept, log2p, group_bytes);
  } else {
    hipLaunchKernelGGL(topk_exclude_kernel<4>, dim3(n_queries), dim3(256), group_bytes, to_stream(stream), scores,
                       idx, n_queries, k_in, k_out, excl_off, excl_idx, out_scores, out_idx, n_kept, log2p,
                       group_bytes);
  }
  TT_CHECK_LAUNCH();
  return TT_OK;
}
