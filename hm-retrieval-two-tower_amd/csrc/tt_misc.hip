// K14 recall hits, the per-shard top-k merge and the per-query exclusion
// filter of sorted top-k lists; set-valued ranking metrics (MAP@K, NDCG@K,
// MRR, recall) of ranked lists; the loss reduction.
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

// ---- tt_rank_metrics --------------------------------------------------------
// Set-valued ranking metrics of one ranked list against one truth row, in
// O(T + k_list) per query with no sort.  The distinct valid truth ids go into
// an open-addressing hash table in LDS (>= 2 * T slots, linear probing;
// inserting with atomicCAS counts them, which is m).  Every list position
// probes the table and atomicMin's itself into the slot of its id, so a slot
// ends up holding the FIRST position of that id: the hit positions are a
// function of membership alone, whatever order the LDS atomics land in.  The
// slots then set one bit per hit position; one wave turns the (at most 64 x
// 64-bit) bitmap into the ascending list of hit positions with popcount
// prefixes, and lane j < num_ks walks that list up to ks[j] — the sequential
// fp32 sums the contract fixes, at most min(m, k) trips.
//
// As for topk_exclude_kernel: NW = 1 runs four queries per 256-thread
// workgroup, each wave on its own LDS region with no workgroup barrier
// (T <= 64 and k_list <= 256: at most 1.3 KB per wave, so the
// 32-waves-per-CU cap stays the limit); NW = 4 runs one query per workgroup
// (at most 2 x 8 KB table + 512 B bitmap + 4 KB hit list).
constexpr int kRankMaxK = 4096;
constexpr int kRankMaxT = 1024;
constexpr int kRankSmallK = 256;
constexpr int kRankSmallT = 64;
constexpr int kRankNoPos = 0x7FFFFFFF;

struct RankArgs {
  const int32_t* cand;
  int64_t ld_cand;
  const int32_t* truth;
  int64_t ld_truth;
  int64_t n_queries;
  int32_t k_list;
  int32_t T;
  int32_t num_ks;
  int32_t ks[kMaxKs];
  const float* disc;
  const float* idcg;
  float* vals;
  int32_t* hits;
  int32_t* m_out;
  unsigned long long* n_valid;
  int32_t log2p;
  int32_t group_bytes;
};

// LDS of one group: keys [P] int, first positions [P] int, the hit bitmap
// (64 bits per 64 list positions), the hit list [min(T, k_list)] int, then
// (16-B aligned) the per-wave distinct counts.
inline int rank_group_bytes(int k_list, int T, int log2p) {
  const int64_t words = (k_list + 63) / 64;
  const int64_t hit_cap = T < k_list ? T : k_list;
  return static_cast<int>(round_up((int64_t{1} << log2p) * 8 + words * 8 + hit_cap * 4, 16)) + 16;
}

template <int NW>
__global__ void __launch_bounds__(256) rank_metrics_kernel(const RankArgs a) {
  extern __shared__ __align__(16) unsigned char rank_lds[];
  constexpr int NT = NW * kWave;
  const int wave = static_cast<int>(threadIdx.x) / kWave;
  const int lane = lane_id();
  const int64_t q = NW == 1 ? blockIdx.x * 4ll + wave : static_cast<int64_t>(blockIdx.x);
  if (q >= a.n_queries) return;  // NW = 1 only: a whole wave, and no workgroup barrier follows
  const int t = NW == 1 ? lane : static_cast<int>(threadIdx.x);
  unsigned char* base = rank_lds + (NW == 1 ? wave * a.group_bytes : 0);
  const int P = 1 << a.log2p;
  const int words = (a.k_list + 63) / 64;
  int* keys = reinterpret_cast<int*>(base);
  int* first = keys + P;
  unsigned* bits = reinterpret_cast<unsigned*>(first + P);
  int* hitpos = reinterpret_cast<int*>(bits + 2 * words);
  int* wcnt = reinterpret_cast<int*>(base + a.group_bytes - 16);
  const unsigned mask = static_cast<unsigned>(P - 1);
  const int shift = 32 - a.log2p;  // log2p >= 1
  auto slot_of = [&](int32_t v) { return (static_cast<unsigned>(v) * 2654435761u) >> shift; };
  auto valid = [](int32_t v) { return v >= 0 && v != kPadIndex; };

  for (int j = t; j < P; j += NT) {
    keys[j] = -1;
    first[j] = kRankNoPos;
  }
  for (int j = t; j < 2 * words; j += NT) bits[j] = 0u;
  group_sync<NW>();
  // at most T inserts into >= 2 * T slots: every probe sequence ends
  const int32_t* tr = a.truth + q * a.ld_truth;
  int mine = 0;
  for (int j = t; j < a.T; j += NT) {
    const int32_t v = tr[j];
    if (!valid(v)) continue;
    unsigned s = slot_of(v);
    for (;;) {
      const int old = atomicCAS(&keys[s], -1, v);
      if (old == -1) ++mine;  // this thread's insert: a new distinct id
      if (old == -1 || old == v) break;
      s = (s + 1) & mask;
    }
  }
  int m = wave_sum_i32(mine);
  if constexpr (NW > 1) {
    if (lane == 0) wcnt[wave] = m;
    __syncthreads();
    m = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) m += wcnt[w];
  } else {
    group_sync<NW>();
  }
  if (m == 0) {  // no truth (uniform over the group): zeros, and the query is in no average
    for (int j = t; j < a.num_ks; j += NT) {
      float* v = a.vals + (q * a.num_ks + j) * 4;
      v[0] = v[1] = v[2] = v[3] = 0.0f;
      a.hits[q * a.num_ks + j] = 0;
    }
    if (t == 0 && a.m_out) a.m_out[q] = 0;
    return;
  }
  const int32_t* li = a.cand + q * a.ld_cand;
  for (int j = t; j < a.k_list; j += NT) {
    const int32_t v = li[j];
    if (!valid(v)) continue;
    unsigned s = slot_of(v);
    for (;;) {
      const int key = keys[s];
      if (key == v) atomicMin(&first[s], j);
      if (key == v || key == -1) break;
      s = (s + 1) & mask;
    }
  }
  group_sync<NW>();
  for (int j = t; j < P; j += NT) {
    const int p = first[j];
    if (p != kRankNoPos) atomicOr(&bits[p >> 5], 1u << (p & 31));
  }
  group_sync<NW>();
  if (NW > 1 && wave != 0) return;

  // one wave: lane l owns list positions [64 l, 64 l + 64)
  unsigned long long w = 0ull;
  if (lane < words) w = (static_cast<unsigned long long>(bits[2 * lane + 1]) << 32) | bits[2 * lane];
  const int cnt = __popcll(w);
  int incl = cnt;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const int o = __shfl_up(incl, d, kWave);
    if (lane >= d) incl += o;
  }
  const int n_hits = __shfl(incl, kWave - 1, kWave);  // <= min(m, k_list): distinct truth ids, distinct positions
  int at = incl - cnt;
  while (w) {
    hitpos[at++] = lane * 64 + static_cast<int>(__builtin_ctzll(w));
    w &= w - 1;
  }
  group_sync<1>();

  if (lane < a.num_ks) {
    int k = a.ks[0];
#pragma unroll
    for (int j = 1; j < kMaxKs; ++j) k = lane == j ? a.ks[j] : k;
    int c = 0, f = 0;
    float ap = 0.0f, dcg = 0.0f;
    for (int n = 0; n < n_hits; ++n) {
      const int p = hitpos[n];
      if (p >= k) break;
      ++c;
      ap = ap + static_cast<float>(c) / static_cast<float>(p + 1);
      dcg = dcg + a.disc[p];
      if (n == 0) f = p + 1;
    }
    const int mk = m < k ? m : k;
    float* v = a.vals + (q * a.num_ks + lane) * 4;
    v[0] = static_cast<float>(c) / static_cast<float>(m);
    v[1] = ap / static_cast<float>(mk);
    v[2] = dcg / a.idcg[mk];
    v[3] = f ? 1.0f / static_cast<float>(f) : 0.0f;
    a.hits[q * a.num_ks + lane] = c;
  }
  if (lane == 0) {
    if (a.m_out) a.m_out[q] = m;
    if (a.n_valid) atomicAdd(a.n_valid, 1ull);
  }
}

// The accumulators' second launch.  Workgroup b < 4 * num_ks owns (j, metric) =
// (b / 4, b % 4): thread t adds the fp32 values of queries t, t + 256, ... in
// ascending order as doubles, a fixed LDS tree follows, then acc += x[0] — no
// floating-point atomics, so the sums are the same bits every run.  A query
// with m = 0 holds +0.0f in every slot, and s + 0.0 == s for every s these
// sums reach (they start at +0.0), so adding it is skipping it.  Workgroup
// 4 * num_ks + j sums hits@k and counts the queries with a hit (integers);
// one more counts the queries with m > 0 when the caller asked for m.
__global__ void __launch_bounds__(256) rank_reduce_kernel(const float* __restrict__ vals,
                                                          const int32_t* __restrict__ hits, int64_t n_queries,
                                                          int num_ks, double* __restrict__ acc_f64,
                                                          unsigned long long* __restrict__ acc_i64,
                                                          const int32_t* __restrict__ m,
                                                          unsigned long long* __restrict__ n_valid) {
  __shared__ double x[256];
  __shared__ unsigned long long xs[256], xc[256];
  const int t = static_cast<int>(threadIdx.x);
  const int b = static_cast<int>(blockIdx.x);
  if (b < 4 * num_ks) {
    const float* src = vals + b;  // (q * num_ks + j) * 4 + metric with b = 4 j + metric
    const int64_t stride = 4ll * num_ks;
    constexpr int kAhead = 16;  // loads in flight per lane; the additions keep their order
    double s = 0.0;
    int64_t qi = t;
    for (; qi + (kAhead - 1) * 256ll < n_queries; qi += kAhead * 256ll) {
      float v[kAhead];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) v[u] = src[(qi + u * 256ll) * stride];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) s += static_cast<double>(v[u]);
    }
    for (; qi < n_queries; qi += 256) s += static_cast<double>(src[qi * stride]);
    x[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) x[t] += x[t + w];
      __syncthreads();
    }
    if (t == 0) acc_f64[b] += x[0];
  } else {
    // j < num_ks: column j of hits; j == num_ks (launched only with m): the scored queries, counted in xc
    const int j = b - 4 * num_ks;
    const int32_t* src = j < num_ks ? hits + j : m;
    const int64_t stride = j < num_ks ? num_ks : 1;
    unsigned long long s = 0ull, c = 0ull;
#pragma unroll 8
    for (int64_t qi = t; qi < n_queries; qi += 256) {
      const int32_t h = src[qi * stride];
      s += static_cast<unsigned long long>(h);
      c += h > 0 ? 1ull : 0ull;
    }
    xs[t] = s;
    xc[t] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) {
        xs[t] += xs[t + w];
        xc[t] += xc[t + w];
      }
      __syncthreads();
    }
    if (t == 0) {
      if (j < num_ks) {
        acc_i64[2 * j] += xs[0];
        acc_i64[2 * j + 1] += xc[0];
      } else {
        n_valid[0] += xc[0];
      }
    }
  }
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

extern "C" int tt_rank_metrics(const int32_t* cand, int64_t ld_cand, int32_t k_list, const int32_t* truth,
                               int64_t ld_truth, int32_t T, int64_t n_queries, const int32_t* ks_host, int32_t num_ks,
                               const float* disc, const float* idcg, float* vals, int32_t* hits, int32_t* m_out,
                               double* acc_f64, int64_t* acc_i64, int64_t* n_valid, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(k_list >= 1 && k_list <= kRankMaxK, "tt_rank_metrics: k_list=%d outside [1,%d]", k_list, kRankMaxK);
  TT_REQUIRE(T >= 1 && T <= kRankMaxT, "tt_rank_metrics: T=%d outside [1,%d]", T, kRankMaxT);
  TT_REQUIRE(num_ks >= 1 && num_ks <= kMaxKs, "tt_rank_metrics: num_ks=%d outside [1,%d]", num_ks, kMaxKs);
  TT_REQUIRE(ks_host != nullptr, "tt_rank_metrics: NULL ks_host");
  for (int j = 0; j < num_ks; ++j)
    TT_REQUIRE(ks_host[j] >= 1 && ks_host[j] <= k_list, "tt_rank_metrics: ks[%d]=%d outside [1, k_list=%d]", j,
               ks_host[j], k_list);
  TT_REQUIRE(ld_cand >= k_list, "tt_rank_metrics: ld_cand=%lld below k_list=%d", static_cast<long long>(ld_cand),
             k_list);
  TT_REQUIRE(ld_truth >= T, "tt_rank_metrics: ld_truth=%lld below T=%d", static_cast<long long>(ld_truth), T);
  TT_REQUIRE(n_queries >= 0 && n_queries <= INT32_MAX, "tt_rank_metrics: n_queries outside [0, 2^31)");
  const int n_acc = (acc_f64 != nullptr) + (acc_i64 != nullptr) + (n_valid != nullptr);
  TT_REQUIRE(n_acc == 0 || n_acc == 3, "tt_rank_metrics: acc_f64, acc_i64 and n_valid go together (all or none)");
  if (n_queries == 0) return TT_OK;
  TT_REQUIRE(cand != nullptr, "tt_rank_metrics: NULL cand");
  TT_REQUIRE(truth != nullptr, "tt_rank_metrics: NULL truth");
  TT_REQUIRE(disc != nullptr && idcg != nullptr, "tt_rank_metrics: NULL disc / idcg table");
  TT_REQUIRE(vals != nullptr, "tt_rank_metrics: NULL vals");
  TT_REQUIRE(hits != nullptr, "tt_rank_metrics: NULL hits");
  RankArgs a{};
  a.cand = cand;
  a.ld_cand = ld_cand;
  a.truth = truth;
  a.ld_truth = ld_truth;
  a.n_queries = n_queries;
  a.k_list = k_list;
  a.T = T;
  a.num_ks = num_ks;
  for (int j = 0; j < num_ks; ++j) a.ks[j] = ks_host[j];
  a.disc = disc;
  a.idcg = idcg;
  a.vals = vals;
  a.hits = hits;
  a.m_out = m_out;
  // with m_out the reduction counts the scored queries from it; without, each scored query adds itself
  a.n_valid = m_out ? nullptr : reinterpret_cast<unsigned long long*>(n_valid);
  a.log2p = 1;
  while ((1 << a.log2p) < 2 * T) ++a.log2p;
  a.group_bytes = rank_group_bytes(k_list, T, a.log2p);
  if (k_list <= kRankSmallK && T <= kRankSmallT) {
    hipLaunchKernelGGL(rank_metrics_kernel<1>, dim3(ceil_div(n_queries, 4)), dim3(256), 4 * a.group_bytes,
                       to_stream(stream), a);
  } else {
    hipLaunchKernelGGL(rank_metrics_kernel<4>, dim3(n_queries), dim3(256), a.group_bytes, to_stream(stream), a);
  }
  TT_CHECK_LAUNCH();
  if (n_acc) {
    hipLaunchKernelGGL(rank_reduce_kernel, dim3(5 * num_ks + (m_out ? 1 : 0)), dim3(256), 0, to_stream(stream), vals,
                       hits, n_queries, num_ks, acc_f64, reinterpret_cast<unsigned long long*>(acc_i64), m_out,
                       reinterpret_cast<unsigned long long*>(n_valid));
    TT_CHECK_LAUNCH();
  }
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
