// K8+K9 (+K10): duplicate-id dedup, segmented gradient sum and the optimizer
// apply for embedding tables; dense optimizers for the tower MLP weights.
//
// Reference semantics (legacy Keras optimizer reached from
// /root/reference/pkg/modelling/models/two_tower_model.py:124 with
// /root/reference/pkg/modelling/optimizer_factory.py:15-18):
//   _resource_apply_sparse_duplicate_indices -> tf.unique + UnsortedSegmentSum
//   (per distinct id, rows summed in increasing batch position, starting from
//   0), then ResourceSparseApplyAdagradV2 per distinct row:
//       acc += g*g;  w -= lr*g / (sqrt(acc) + eps)
//
// MI355X design (every stage uses the whole GPU):
//  1+2. keys + sort — every table's lookups become 32-bit keys (table index |
//     row id) with the lookup index as value, each table's region padded to a
//     multiple of kBlock with an "invalid" id that sorts last, sorted stably so
//     each table's lookups come out grouped by row id in increasing batch
//     position.  Three paths, chosen by size alone (run_sparse):
//     chunked — every region cut into chunks of 2048 lookups, each sorted in
//       LDS by its own workgroup (chunk_sort_kernel), then merged
//       (chunk_merge_kernel): two launches.  Taken when every region fits the
//       merge: <= 131072 lookups for tables of <= 255 rows, <= 32768 otherwise.
//       The train step's tables all do.
//     small tables — else, when every table of the call has <= 255 rows: one
//       launch, one workgroup per table doing one counting pass on the whole
//       row id (small_table_sort_kernel; any region size).
//     device — else: a key-build launch + one rocPRIM radix sort over the key
//       bits in use.
//  3. blocks — one (sub-)wave per kBlock consecutive sorted lookups of a
//     table, lanes over embedding columns (coalesced row reads): sequential
//     fp32 sums of each segment piece; a segment that starts and ends inside
//     the block is applied immediately, the pieces of longer segments (Zipf
//     heavy hitters repeated thousands of times) are written out.
//  4. join   — inside the same launch, by the LAST block to arrive: a block
//     that wrote a piece of a segment spanning blocks stores it write-through,
//     drains its stores and adds 1 to the segment's counter (one counter per
//     block in the workspace, indexed by the block where the segment starts;
//     zeroed by the key/sort stage of every call and again by the joiner).
//     The block whose add returns span - 1 reads every piece past the caches,
//     adds them in block order starting from the start block's and applies
//     the update; every other block returns.  Nobody waits, polls or spins,
//     and the sum does not depend on which block came last.  A piece block
//     finds its segment's first and last block from probes of the sorted keys
//     in both directions, one per lane and block, loaded in the same round as
//     its own keys; a segment reaching past P blocks goes on with a (P+1)-ary
//     search.  Tables
//     of at most 255 rows (nearly all pieces, little row traffic) take the
//     lowest wave indices, so their joins run under the large tables' traffic.
// Summation order = per table, sorted lookups cut into aligned blocks of
// kBlock; each piece summed sequentially from 0, pieces added in order from 0.
// This equals TF's flat order whenever an id occurs within one block and is
// bitwise reproducible always; oracle/tt_oracle.c restates the same order.
// All arithmetic goes through ieee_op<> (one correctly rounded IEEE operation
// each; the file is built with -ffp-contract=off and HIP's default correctly
// rounded fp32 divide/sqrt) so results match the CPU restatement bit for bit.
// (HIP's __fsqrt_rn maps to the approximate native sqrt on this toolchain.)
#include <algorithm>
#include <cmath>
#include <rocprim/device/device_radix_sort.hpp>

#include "tt_common.h"
#include "tt_wg_sort.h"

namespace tt {
namespace {

template <char OP>
__device__ __forceinline__ float ieee_op(float a, float b) {
  if constexpr (OP == '+') return a + b;
  if constexpr (OP == '-') return a - b;
  if constexpr (OP == '*') return a * b;
  return a / b;
}

constexpr int kBlock = 32;            // sorted lookups per block (summation granule)
constexpr int kTablesPerLaunch = 16;
constexpr int kThreads = 256;
constexpr int kPFJoin = 32;           // pieces per column in flight per batch of a join
constexpr int kPFShort = 4;           // ... of a join of at most this many pieces
constexpr int kSmallRows = 255;       // tables of at most this many rows go first in the block launch
constexpr int64_t kMaxLookups = int64_t(1) << 24;
constexpr int kSrcShift = 28;  // sorted values: source << 28 | batch row (batch < 2^28)

// Workspace header (first 256 B of every sparse workspace).  The sort stage
// stamps the fingerprint of the lookups it sorted; the block pass
// compares it with its own call's before touching a table, and records a
// mismatch (a presorted apply on another call's keys) or an out-of-call
// (source, row) in `error` instead of applying anything from that block (such a
// block does not arrive at its segments' counters either: they stay unapplied).
// tt_sparse_status() reads and clears `error`.
constexpr uint32_t kHdrMagic = 0x54545350u;  // "TTSP"
constexpr int kHdrBytes = 256;
enum : uint32_t { kErrStaleKeys = 1u, kErrOutOfCall = 2u };
struct SparseHeader {
  uint32_t magic;
  uint32_t error;
  uint32_t fp0, fp1;  // fingerprint of the sorted call
};

struct TableDesc {
  const int32_t* ids[TT_MAX_SOURCES];
  int32_t goff[TT_MAX_SOURCES];  // source column offsets in the table's grad
  const float* grad;             // the table's gradient rows (call grad or per-table override)
  int32_t gld;                   // its row stride (floats)
  float* table;
  float* slot0;
  float* slot1;
  int64_t num_rows;
  int32_t dim;
  int32_t num_sources;
  int32_t n;           // valid lookups = num_sources * batch
  int32_t base;        // first sorted index of this table's region
  int32_t n_pad;       // region size, multiple of kBlock
  int32_t lanes;       // P: lanes per block slot (pow2 <= 64)
  int32_t wave_begin;  // first global wave of this table in the block kernels
  int32_t chunk_begin; // first global chunk of this table in the chunked sort
  int64_t piece_off;   // first float of this table's pieces [blocks][2][dim]
};

struct Job {
  TableDesc t[kTablesPerLaunch];
  int32_t num;
  int32_t id_bits;
  int64_t batch;
  uint32_t* keys_in;
  uint32_t* vals_in;
  const uint32_t* keys;  // sorted
  const uint32_t* vals;  // sorted
  float* pieces;
  uint32_t* arrived;     // per block of kBlock sorted lookups: pieces arrived of the segment starting there
  uint32_t* chunk_hist;  // chunked sort of small tables: digit counts [chunks][256]
  int32_t num_chunks;
  float* dense_out;      // kWriteSum: per-sorted-index segment sums [total][dim_max]
  int32_t dense_dim;
  SparseHeader* hdr;     // workspace header
  uint32_t fp0, fp1;     // this call's fingerprint
};

// The apply passes' guard: the sorted keys must be this call's.  Wave-uniform.
__device__ __forceinline__ bool keys_are_mine(const Job& j) {
  const uint32_t f0 = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&j.hdr->fp0, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_AGENT));
  const uint32_t f1 = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&j.hdr->fp1, __ATOMIC_RELAXED,
                                                                        __HIP_MEMORY_SCOPE_AGENT));
  if (f0 == j.fp0 && f1 == j.fp1) return true;
  if (lane_id() == 0) atomicOr(&j.hdr->error, kErrStaleKeys);
  return false;
}

// The sort stage's stamp: the workspace carries this call's fingerprint (one
// thread of the launch).
__device__ __forceinline__ void stamp_header(const Job& j) {
  if (j.hdr->magic != kHdrMagic) {  // fresh workspace: no recorded error yet
    j.hdr->error = 0u;
    j.hdr->magic = kHdrMagic;
  }
  j.hdr->fp0 = j.fp0;
  j.hdr->fp1 = j.fp1;
}

enum ApplyOp { kWriteSum = 0, kAdagrad = 1, kAdamScatter = 2, kScatterSum = 3 };

struct ApplyParams {
  float lr;
  float eps;
  float one_minus_beta1;
  float one_minus_beta2;
};

// the table whose wave range holds gw: the largest wave_begin <= gw (the ranges
// are disjoint and start at 0, in an order make_plan chooses)
__device__ __forceinline__ int table_of_wave(const Job& j, int gw) {
  int t = 0, best = -1;
#pragma unroll 1
  for (int i = 0; i < j.num; ++i) {
    const int wb = j.t[i].wave_begin;
    if (gw >= wb && wb > best) {
      t = i;
      best = wb;
    }
  }
  return t;
}

// 1. keys / values of every lookup (+ padding) of every table.
__global__ void __launch_bounds__(kThreads) build_keys_kernel(const Job j, int total) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  int t = 0;
#pragma unroll 1
  for (int k = 1; k < j.num; ++k)
    if (i >= j.t[k].base) t = k;
  const TableDesc& T = j.t[t];
  const int loc = i - T.base;
  const uint32_t invalid = (1u << j.id_bits) - 1u;
  uint32_t id = invalid, val = 0xFFFFFFFFu;
  if (loc < T.n) {
    const int s = static_cast<int>(loc / j.batch);
    const int64_t b = loc - s * j.batch;
    const int32_t r = T.ids[s][b];
    const bool ok = r >= 0 && r < T.num_rows;
    id = ok ? static_cast<uint32_t>(r) : invalid;
    // invalid lookups keep no gradient offset: nothing reads their rows
    val = ok ? (static_cast<uint32_t>(s) << kSrcShift) | static_cast<uint32_t>(b) : 0xFFFFFFFFu;
  }
  j.keys_in[i] = (static_cast<uint32_t>(t) << j.id_bits) | id;
  j.vals_in[i] = val;
  if (i % kBlock == 0) j.arrived[i / kBlock] = 0u;  // this call's join counters
  if (i == 0) stamp_header(j);
}

// 1+2 fused in LDS (the small-table and chunked sorts below): workgroups build
// their region's row keys from the ids and sort them by the pieces of
// tt_wg_sort.h over the bits the table's row ids use (8-bit digits at most),
// then write the same sorted (key, value) arrays the rocPRIM path writes.  The
// table index is the key's high part and each table owns its region, so
// sorting the regions one by one equals the global sort.

// One region's descriptor in registers (a reference into the kernel's
// by-value Job indexed by blockIdx.x made the compiler copy the whole Job to
// scratch).
struct Region {
  const int32_t *ids0, *ids1, *ids2, *ids3;  // no array: a dynamically indexed one lands in scratch
  int64_t batch;
  uint32_t* keys;  // sorted outputs, offset to this region
  uint32_t* vals;
  int n;           // valid lookups
  uint32_t nr;     // rows: row key of invalid ids and padding
  uint32_t khi;    // table index << id_bits
  uint32_t invalid;
};

__device__ __forceinline__ Region region_of(const Job& j, int t) {
  const TableDesc& T = j.t[t];
  Region R;
  R.ids0 = T.ids[0];
  R.ids1 = T.ids[1];
  R.ids2 = T.ids[2];
  R.ids3 = T.ids[3];
  R.batch = j.batch;
  R.keys = const_cast<uint32_t*>(j.keys) + T.base;
  R.vals = const_cast<uint32_t*>(j.vals) + T.base;
  R.n = T.n;
  R.nr = static_cast<uint32_t>(T.num_rows);
  R.khi = static_cast<uint32_t>(t) << j.id_bits;
  R.invalid = (1u << j.id_bits) - 1u;
  return R;
}

__device__ __forceinline__ int source_of(const Region& R, int64_t i) {  // i / batch for i < 4 * batch
  return (i >= R.batch) + (i >= 2 * R.batch) + (i >= 3 * R.batch);
}

// row key of region position i: the row id, or nr for invalid ids and padding
// Branch-free (padding positions load ids[0][0] and discard it), so a caller's
// unrolled loads all issue before the first wait.
__device__ __forceinline__ uint32_t region_key(const Region& R, int i) {
  const bool valid = i < R.n;
  const int iv = valid ? i : 0;
  const int s = source_of(R, iv);
  const int b = iv - s * static_cast<int>(R.batch);
  const int32_t* ids = R.ids0;
  ids = s >= 1 ? R.ids1 : ids;
  ids = s >= 2 ? R.ids2 : ids;
  ids = s >= 3 ? R.ids3 : ids;
  const int32_t r = ids[b];
  return (valid && r >= 0 && static_cast<uint32_t>(r) < R.nr) ? static_cast<uint32_t>(r) : R.nr;
}

// Small-table sort: one 1024-thread workgroup per table of at most 255 rows
// (row keys of <= 8 bits, host-checked) sorts its whole region, of any size,
// by ONE counting pass on the row key.  Run when a call is all such tables and
// one of them is too long for the chunked sort's merge: one launch on one CU
// per table instead of a key build and a multi-launch device sort.
//   LDS: the per-wave digit counts [digit][wave], then the region's row keys
//   as bytes for the regions that fit kStStageMax (dynamic, sized by the host
//   to the longest such region of the call); a longer region re-reads its ids.
constexpr int kStThreads = 1024;
constexpr int kStWaves = kStThreads / kWave;
constexpr int kStStageMax = 131072;  // most row keys staged in LDS (bytes)
using StHist = DigitHist<kStWaves>;

// row keys of one source's positions [s*batch, (s+1)*batch) into LDS, 16
// independent id loads in flight per thread (the source's pointer is uniform
// and written out per call: a select among the four made the compiler index
// them from scratch)
__device__ __forceinline__ void stage_source(const Region& R, const int32_t* __restrict__ ids, int s, uint8_t* dst) {
  const int nb = static_cast<int>(R.batch);
  for (int base = 0; base < nb; base += 16 * kStThreads) {
    int32_t r[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int b = base + u * kStThreads + static_cast<int>(threadIdx.x);
      r[u] = ids[b < nb ? b : 0];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int b = base + u * kStThreads + static_cast<int>(threadIdx.x);
      const uint32_t k = (r[u] >= 0 && static_cast<uint32_t>(r[u]) < R.nr) ? static_cast<uint32_t>(r[u]) : R.nr;
      if (b < nb) dst[s * nb + b] = static_cast<uint8_t>(k);
    }
  }
}

// row keys of positions [0, n) into LDS (padding past the lookups: nr)
__device__ __forceinline__ void stage_keys(const Region& R, int n, uint8_t* dst) {
  stage_source(R, R.ids0, 0, dst);
  if (R.n > R.batch) stage_source(R, R.ids1, 1, dst);
  if (R.n > 2 * R.batch) stage_source(R, R.ids2, 2, dst);
  if (R.n > 3 * R.batch) stage_source(R, R.ids3, 3, dst);
  for (int i = R.n + static_cast<int>(threadIdx.x); i < n; i += kStThreads) dst[i] = static_cast<uint8_t>(R.nr);
}

// sorted (key, value) at output slot `out` of region position ps with row key k
__device__ __forceinline__ void region_store(const Region& R, int out, uint32_t ps, uint32_t k) {
  uint32_t val = 0xFFFFFFFFu;  // padding and invalid ids keep no gradient offset
  if (k < R.nr) {
    const uint32_t s = static_cast<uint32_t>(source_of(R, ps));
    val = (s << kSrcShift) | static_cast<uint32_t>(ps - s * R.batch);
  }
  R.keys[out] = R.khi | (k < R.nr ? k : R.invalid);
  R.vals[out] = val;
}

__global__ void __launch_bounds__(kStThreads) small_table_sort_kernel(const Job j) {
  extern __shared__ __attribute__((aligned(16))) char lsm[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(lsm);  // [256 digits][StHist::kStride]
  uint8_t* k8 = reinterpret_cast<uint8_t*>(lsm + StHist::kWords * 4);
  __shared__ uint32_t wsum[kStWaves];
  const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
  const int t = blockIdx.x;
  const Region R = region_of(j, t);
  const int n = j.t[t].n_pad;
  for (int e = tid; e < n / kBlock; e += kStThreads) j.arrived[j.t[t].base / kBlock + e] = 0u;  // join counters
  if (t == 0 && tid == 0) stamp_header(j);
  const int bits = 32 - __builtin_clz(R.nr);  // row keys lie in [0, nr]: <= 8 bits
  const WaveSlice<kStWaves> s(n);
  StHist::clear(hist);
  // the keys are staged in LDS as bytes when they fit, else re-read from the ids
  const bool staged = n <= kStStageMax;
  if (staged) stage_keys(R, n, k8);
  __syncthreads();
  for (int t0 = s.beg; t0 < s.end; t0 += kWave) {  // counts: peers per tile, no LDS atomics
    const int i = t0 + lane;
    const bool act = i < s.end;
    const uint32_t d = act ? (staged ? k8[i] : region_key(R, i)) : 0u;
    StHist::count(hist, d, digit_peers(d, act, bits), w);
  }
  StHist::scan(hist, wsum);
  for (int t0 = s.beg; t0 < s.end; t0 += kWave) {
    const int i = t0 + lane;
    const bool act = i < s.end;
    const uint32_t d = act ? (staged ? k8[i] : region_key(R, i)) : 0u;
    const uint64_t m = digit_peers(d, act, bits);
    if (act)
      StHist::place(hist, d, m, w, [&](uint32_t o) { region_store(R, static_cast<int>(o), static_cast<uint32_t>(i), d); });
  }
}

// Chunked region sort (default): the same stable sort of every region by
// (row key, position), spread over many small workgroups so that it finishes
// in a few microseconds wherever the graph places it and sits beside other
// kernels on a CU (~13 KB of LDS instead of 150 KB).
//   chunk_sort_kernel: one 512-thread workgroup per kChunk consecutive
//   positions of a region sorts them in LDS (LSD passes of tt_wg_sort.h, 4
//   tiles per wave) into the key/value staging buffers: chunk-sorted row keys and
//   region positions; small tables (<= 8 key bits) also write the chunk's
//   digit counts.
//   chunk_merge_kernel: the final slot of a chunk's i-th element with row key
//   k is i + #{keys <= k in earlier chunks} + #{keys < k in later chunks}
//   (stable: equal keys keep chunk order, and chunks are in position order),
//   found by binary search of each other chunk's sorted keys, all staged in
//   LDS by one round of loads (regions <= 32768 lookups: <= 16 chunks), or
//   for small tables from the digit counts of all chunks (<= 64 chunks).
constexpr int kChunk = 2048;
constexpr int kCsThreads = 512;
constexpr int kCsWaves = kCsThreads / kWave;
constexpr int kCsTiles = kChunk / kCsThreads;
using CsHist = DigitHist<kCsWaves>;
constexpr int kChunkMaxSmall = 64 * kChunk;  // small tables: the merge reads every chunk's counts

__device__ __forceinline__ int table_of_chunk(const Job& j, int c) {
  int t = 0;
#pragma unroll 1
  for (int i = 1; i < j.num; ++i)
    if (c >= j.t[i].chunk_begin) t = i;
  return __builtin_amdgcn_readfirstlane(t);
}

__global__ void __launch_bounds__(kCsThreads) chunk_sort_kernel(const Job j) {
  __shared__ uint32_t lkey[kChunk];
  __shared__ uint16_t pbuf[2][kChunk];
  __shared__ uint32_t hist[CsHist::kWords];
  __shared__ uint32_t wsum[kCsWaves];
  const int tid = threadIdx.x;
  const int t = table_of_chunk(j, blockIdx.x);
  const Region R = region_of(j, t);
  const int c0 = (static_cast<int>(blockIdx.x) - j.t[t].chunk_begin) * kChunk;
  const int n = min(kChunk, j.t[t].n_pad - c0);
  uint32_t* ck = j.keys_in + j.t[t].base + c0;  // chunk-sorted row keys
  uint32_t* cp = j.vals_in + j.t[t].base + c0;  // their region positions
  if (tid < n / kBlock) j.arrived[(j.t[t].base + c0) / kBlock + tid] = 0u;  // this call's join counters
  if (blockIdx.x == 0 && tid == 0) stamp_header(j);
  {  // row keys of the chunk: kCsTiles independent id loads in flight per thread
    uint32_t k[kCsTiles];
#pragma unroll
    for (int u = 0; u < kCsTiles; ++u) k[u] = region_key(R, c0 + u * kCsThreads + tid);
#pragma unroll
    for (int u = 0; u < kCsTiles; ++u) {
      const int i = u * kCsThreads + tid;
      if (i < n) {
        lkey[i] = k[u];
        pbuf[0][i] = static_cast<uint16_t>(i);
      }
    }
  }
  CsHist::clear(hist);
  const int bits = 32 - __builtin_clz(R.nr);  // row keys lie in [0, nr]
  const WaveSlice<kCsWaves> s(n);
  const int passes = (bits + 7) / 8;
  const int width = (bits + passes - 1) / passes;
  const uint32_t dmask = (1u << width) - 1u;
  int cur = 0;
  for (int p = 0; p < passes; ++p) {
    if (p > 0) CsHist::clear(hist);
    __syncthreads();
    LsdPass<kCsWaves, kCsTiles> pass;
    pass.load(s, pbuf[cur], lkey, p * width, dmask);
    pass.count(s, hist, width);
    if (passes == 1) {  // small table: the chunk's digit counts (block-uniform)
      __syncthreads();
      if (tid < 256) {
        uint32_t c = 0;
#pragma unroll
        for (int v = 0; v < kCsWaves; ++v) c += hist[tid * CsHist::kStride + v];
        j.chunk_hist[static_cast<int64_t>(blockIdx.x) * 256 + tid] = c;
      }
    }
    CsHist::scan(hist, wsum);
    const bool last = p == passes - 1;
    pass.scatter(s, hist, [&](uint32_t o, uint16_t ps) {
      if (last) {
        ck[o] = lkey[ps];
        cp[o] = static_cast<uint32_t>(c0) + ps;
      } else {
        pbuf[cur ^ 1][o] = ps;
      }
    });
    cur ^= 1;
    __syncthreads();  // the scatter is complete before hist is cleared / the order read
  }
}

// binary-search merge: every chunk's sorted keys staged in LDS (up to 16
// chunks = 128 KB: regions of <= 32768 lookups, e.g. an owner's requests in
// the row-sharded step)
constexpr int kMergeMaxChunks = 16;
constexpr int kChunkMaxLarge = kMergeMaxChunks * kChunk;
constexpr int kMergeLdsMax = kMergeMaxChunks * kChunk * 4;

__global__ void __launch_bounds__(kCsThreads) chunk_merge_kernel(const Job j) {
  extern __shared__ __attribute__((aligned(16))) uint32_t allk[];  // [chunks][kChunk] sorted keys (large tables)
  __shared__ uint32_t base[256], first[256], wsum[2][kCsWaves];
  const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
  const int t = table_of_chunk(j, blockIdx.x);
  const Region R = region_of(j, t);
  const TableDesc& T = j.t[t];
  const int ci = static_cast<int>(blockIdx.x) - T.chunk_begin;
  const int nch = (T.n_pad + kChunk - 1) / kChunk;
  const int c0 = ci * kChunk;
  const int n = min(kChunk, T.n_pad - c0);
  const uint32_t* ck = j.keys_in + T.base;
  const uint32_t* cp = j.vals_in + T.base;
  uint32_t key[kCsTiles], pos[kCsTiles], out[kCsTiles];
#pragma unroll
  for (int u = 0; u < kCsTiles; ++u) {
    const int i = u * kCsThreads + tid;
    key[u] = i < n ? ck[c0 + i] : 0u;
    pos[u] = i < n ? cp[c0 + i] : 0u;
    out[u] = static_cast<uint32_t>(i);
  }
  const int bits = 32 - __builtin_clz(R.nr);
  if (bits <= 8) {
    // digit d: base = #{keys < d in the region} + #{keys == d in earlier
    // chunks}; first = #{keys < d in this chunk} (threads 0..255: one digit each)
    uint32_t tot = 0, before = 0, mine = 0;
    if (tid < 256) {
      const uint32_t* h = j.chunk_hist + static_cast<int64_t>(T.chunk_begin) * 256 + tid;
#pragma unroll 4
      for (int c = 0; c < nch; ++c) {
        const uint32_t x = h[static_cast<int64_t>(c) * 256];
        tot += x;
        before += c < ci ? x : 0u;
        mine = c == ci ? x : mine;
      }
    }
    uint32_t it = tot, im = mine;  // inclusive scans over the digits
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t yt = __shfl_up(it, o, kWave), ym = __shfl_up(im, o, kWave);
      if (lane >= o) {
        it += yt;
        im += ym;
      }
    }
    if (lane == kWave - 1) {
      wsum[0][w] = it;
      wsum[1][w] = im;
    }
    __syncthreads();
    uint32_t et = it - tot, em = im - mine;
    for (int v = 0; v < w; ++v) {
      et += wsum[0][v];
      em += wsum[1][v];
    }
    if (tid < 256) {
      base[tid] = et + before;
      first[tid] = em;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kCsTiles; ++u) out[u] = base[key[u]] + (out[u] - first[key[u]]);
  } else {
    // every chunk's sorted keys into LDS at once (one round trip), padded
    // with keys above every row key
    for (int e = tid; e < nch * kChunk; e += kCsThreads) allk[e] = e < T.n_pad ? ck[e] : 0xFFFFFFFFu;
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
      if (c == ci) continue;  // block-uniform
      const uint32_t* other = allk + c * kChunk;
      // earlier chunk: keys <= k come first; later chunk: keys < k (k + 0 vs
      // k + 1 against the sorted keys; keys < 2^31, the padding compares high)
      const uint32_t bump = c < ci ? 1u : 0u;
#pragma unroll
      for (int u = 0; u < kCsTiles; ++u) {
        const uint32_t kk = key[u] + bump;
        int b = 0;
#pragma unroll
        for (int s = kChunk / 2; s >= 1; s >>= 1) b += other[b + s - 1] < kk ? s : 0;
        b += other[kChunk - 1] < kk ? 1 : 0;
        out[u] += static_cast<uint32_t>(b);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kCsTiles; ++u)
    if (u * kCsThreads + tid < n) region_store(R, static_cast<int>(out[u]), pos[u], key[u]);
}

// The optimizer update of one distinct row, split into a load phase and a
// compute/store phase so that a lane can have every row of its block in
// flight at once (the applies are independent, the latency is not).
struct RowState {
  float x0, x1;
};

template <int OP>
__device__ __forceinline__ RowState load_row(const TableDesc& T, int64_t o) {
  RowState r{0.0f, 0.0f};
  if (OP == kAdagrad) {
    r.x0 = T.slot0[o];
    r.x1 = T.table[o];
  } else if (OP == kAdamScatter) {
    r.x0 = T.slot0[o];
    r.x1 = T.slot1[o];
  }
  return r;
}

template <int OP>
__device__ __forceinline__ void store_row(const TableDesc& T, const ApplyParams& ap, int64_t o, RowState r, float g) {
  if (OP == kAdagrad) {
    const float a = ieee_op<'+'>(r.x0, ieee_op<'*'>(g, g));
    T.slot0[o] = a;
    T.table[o] = ieee_op<'-'>(r.x1, ieee_op<'/'>(ieee_op<'*'>(ap.lr, g), ieee_op<'+'>(sqrtf(a), ap.eps)));
  } else if (OP == kAdamScatter) {  // scatter-add of the scaled distinct-id gradient into the decayed slots
    T.slot0[o] = ieee_op<'+'>(r.x0, ieee_op<'*'>(g, ap.one_minus_beta1));
    T.slot1[o] = ieee_op<'+'>(r.x1, ieee_op<'*'>(ieee_op<'*'>(g, g), ap.one_minus_beta2));
  } else if (OP == kScatterSum) {  // dense per-row gradient: each distinct row written once
    T.table[o] = g;
  }
}

// Pieces pass between workgroups inside the launch.  They are stored
// write-through and read past the caches (relaxed agent-scope atomics: sc1
// stores and loads), so neither side needs a release of the L2 — which holds
// this kernel's dirty table rows — or an invalidate; the store drain before
// the counter add orders them.
__device__ __forceinline__ void publish_piece(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float read_piece(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// N pieces i0 .. i0 + N - 1 of two columns, all loads issued before the first
// add (indices past piece n repeat piece n and are not added); piece 0 is the
// first block's tail piece, the others are head pieces
template <int N>
__device__ __forceinline__ void add_pieces(const float* pcs, int dim, int i0, int n, int col, int col1, float& g0,
                                           float& g1) {
  float v0[N], v1[N];
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const int i = min(i0 + q, n);
    const float* p = pcs + static_cast<int64_t>(i) * 2 * dim + (i == 0 ? dim : 0);
    v0[q] = read_piece(p + col);
    v1[q] = read_piece(p + col1);
  }
#pragma unroll
  for (int q = 0; q < N; ++q) {
    const bool in = i0 + q <= n;
    g0 = in ? ieee_op<'+'>(g0, v0[q]) : g0;
    g1 = in ? ieee_op<'+'>(g1, v1[q]) : g1;
  }
}

// 4. the join of one segment spanning blocks first .. last of table T, run by
// the last block to arrive at its counter: 0 + the first block's tail piece,
// then the head pieces of the following blocks in block order, then the
// update of the row — the same chain whichever block runs it.  Two column
// passes at a time; the row's state is loaded in the same round as the first
// pieces, and kPFJoin pieces per column are in flight per batch (kPFShort for
// the common segment of a few blocks).
template <int OP>
__device__ __forceinline__ void join_segment(const Job& j, const TableDesc& T, const ApplyParams& ap, uint32_t key,
                                             int seg_start_sorted, int first, int last, int P, int li) {
  const float* pcs = j.pieces + T.piece_off + static_cast<int64_t>(first) * 2 * T.dim;
  const int dim = T.dim, n = last - first;  // pieces 0 .. n
  const int64_t row = static_cast<int64_t>(key & ((1u << j.id_bits) - 1u)) * dim;  // a valid id: only those are joined
  for (int col = li; col < dim; col += 2 * P) {
    const bool two = col + P < dim;
    const int col1 = two ? col + P : col;
    RowState r0{0.0f, 0.0f}, r1{0.0f, 0.0f};
    if (OP != kWriteSum) {
      r0 = load_row<OP>(T, row + col);
      r1 = load_row<OP>(T, row + col1);
    }
    float g0 = 0.0f, g1 = 0.0f;
    if (n < kPFShort) {
      add_pieces<kPFShort>(pcs, dim, 0, n, col, col1, g0, g1);
    } else {
      for (int i0 = 0; i0 <= n; i0 += kPFJoin) add_pieces<kPFJoin>(pcs, dim, i0, n, col, col1, g0, g1);
    }
    if (OP == kWriteSum) {
      j.dense_out[static_cast<int64_t>(seg_start_sorted) * j.dense_dim + col] = g0;
      if (two) j.dense_out[static_cast<int64_t>(seg_start_sorted) * j.dense_dim + col1] = g1;
    } else {
      store_row<OP>(T, ap, row + col, r0, g0);
      if (two) store_row<OP>(T, ap, row + col1, r1, g1);
    }
  }
}

// 3. per block of kBlock sorted lookups: piece sums; complete segments applied;
// 4. the last block to arrive at a longer segment's counter joins its pieces.
template <int OP>
__global__ void __launch_bounds__(kThreads) block_sum_kernel(const Job j, const ApplyParams ap) {
  // wave-uniform (readfirstlane): the table descriptor is then read with scalar loads
  const int gw = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave));
  const int t = table_of_wave(j, gw);
  const TableDesc& T = j.t[t];
  const int P = T.lanes;
  const int lane = lane_id();
  const int blk = (gw - T.wave_begin) * (kWave / P) + lane / P;
  const int nblk = T.n_pad / kBlock;
  if (blk >= nblk) return;
  const int b0 = T.base + blk * kBlock;   // first sorted index of the block
  const uint32_t id_mask = (1u << j.id_bits) - 1u;
  uint32_t key[kBlock], off[kBlock];
#pragma unroll
  for (int r = 0; r < kBlock; ++r) {
    key[r] = j.keys[b0 + r];
    off[r] = j.vals[b0 + r];
  }
  // In the same round of loads, the extent of the segments that leave and
  // enter the block, in blocks: the segment of key[kBlock - 1] reaches block
  // blk + 1 + i iff that block's first key equals it, the segment of key[0]
  // reaches back to block blk - 1 - i iff that block's last key does (equal
  // keys are contiguous; nothing else of the order is used).  Lane i of the
  // slot's P probes both; the key holds on a prefix of the probes.
  const int li = lane % P;
  const uint64_t gmask = (P == kWave) ? ~0ull : (((1ull << P) - 1ull) << (lane - li));
  const int nfwd = nblk - 1 - blk, nbwd = blk;  // blocks after / before this one
  const uint32_t fk0 = j.keys[b0 + (li < nfwd ? kBlock * (1 + li) : 0)];
  const uint32_t bk0 = j.keys[b0 - (li < nbwd ? 1 + kBlock * li : 0)];
  // the fingerprint check in the same round of loads as the keys
  const bool mine = keys_are_mine(j);
  // blocks the two segments reach beyond this one, as far as the P probes see
  int flo = __popcll(__ballot(li < nfwd && fk0 == key[kBlock - 1]) & gmask);
  int blo = __popcll(__ballot(li < nbwd && bk0 == key[0]) & gmask);
  if (!mine) return;
  // grad offsets (validated to fit 32 bits) and the segment structure; both are
  // the same for every column this lane visits.  The table's source offsets
  // are read ONCE into registers (indexing T.goff[] by a per-lane source made
  // the compiler re-load it from the kernarg block with a full wait per row).
  const uint32_t gld = static_cast<uint32_t>(T.gld);
  const uint32_t go0 = T.goff[0], go1 = T.goff[1], go2 = T.goff[2], go3 = T.goff[3];
  const float* __restrict__ grad = T.grad;
  uint32_t ends = 0, apply = 0;
  bool out_of_call = false;
#pragma unroll
  for (int r = 0; r < kBlock; ++r) {
    const uint32_t s = off[r] >> kSrcShift;
    const uint32_t b = off[r] & ((1u << kSrcShift) - 1u);
    const uint32_t o = b * gld + (s == 0 ? go0 : s == 1 ? go1 : s == 2 ? go2 : go3);
    // a (source, row) outside this call's gradient can only come from keys
    // that are not this call's: reported, and the block applies nothing
    const bool in = s < static_cast<uint32_t>(T.num_sources) && b < static_cast<uint32_t>(j.batch);
    out_of_call = out_of_call || (off[r] != 0xFFFFFFFFu && !in);
    off[r] = (off[r] != 0xFFFFFFFFu && in) ? o : 0xFFFFFFFFu;
    if (r == kBlock - 1 || key[r + 1] != key[r]) ends |= 1u << r;
  }
  if (out_of_call) {
    atomicOr(&j.hdr->error, kErrOutOfCall);
    return;
  }
  const bool head_cont = blo > 0;  // key[0] is the previous block's last key
  const bool tail_cont = flo > 0;  // key[kBlock - 1] is the next block's first key
  {
    int seg_begin = 0;
#pragma unroll
    for (int r = 0; r < kBlock; ++r) {
      if (ends >> r & 1u) {
        const bool piece = (seg_begin == 0 && head_cont) || (r == kBlock - 1 && tail_cont);
        const bool valid = OP == kWriteSum || (key[r] & id_mask) < static_cast<uint32_t>(T.num_rows);
        if (!piece && valid) apply |= 1u << r;
        seg_begin = r + 1;
      }
    }
  }
  float* pc = j.pieces + T.piece_off + static_cast<int64_t>(blk) * 2 * T.dim;
  for (int col = lane % P; col < T.dim; col += P) {
    float v[kBlock];
#pragma unroll
    for (int r = 0; r < kBlock; ++r) v[r] = off[r] != 0xFFFFFFFFu ? grad[off[r] + col] : 0.0f;
    // segment sums, left in v[r] at each segment's last row
    float acc = 0.0f;
    int seg_begin = 0;
#pragma unroll
    for (int r = 0; r < kBlock; ++r) {
      acc = ieee_op<'+'>(acc, v[r]);
      v[r] = acc;
      if (ends >> r & 1u) {
        if (seg_begin == 0 && head_cont) publish_piece(&pc[col], acc);                // piece of an earlier segment
        else if (r == kBlock - 1 && tail_cont) publish_piece(&pc[T.dim + col], acc);  // first piece of a continuing one
        acc = 0.0f;
        seg_begin = r + 1;
      }
    }
    if (OP == kWriteSum) {
      int sb = 0;
#pragma unroll
      for (int r = 0; r < kBlock; ++r) {
        if (apply >> r & 1u) j.dense_out[static_cast<int64_t>(b0 + sb) * j.dense_dim + col] = ieee_op<'+'>(0.0f, v[r]);
        if (ends >> r & 1u) sb = r + 1;
      }
    } else {
      RowState st[kBlock];
#pragma unroll
      for (int r = 0; r < kBlock; ++r)
        if (apply >> r & 1u) st[r] = load_row<OP>(T, static_cast<int64_t>(key[r] & id_mask) * T.dim + col);
      // one wait for every row's state: the loads sit under branches, so the
      // compiler cannot count them and would otherwise drain the queue (the
      // stores included) before each row's stores
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0) expcnt(7) lgkmcnt(15)
#pragma unroll
      for (int r = 0; r < kBlock; ++r)
        if (apply >> r & 1u)
          store_row<OP>(T, ap, static_cast<int64_t>(key[r] & id_mask) * T.dim + col, st[r], ieee_op<'+'>(0.0f, v[r]));
    }
  }
  // 4. Hand-off of the pieces, last arriver joins; nobody waits.  Only valid
  // segments are joined (the invalid-id run never is).  All of this is uniform
  // over the P lanes of a block slot; the slots of a wave diverge.
  const uint32_t rows = static_cast<uint32_t>(T.num_rows);
  const uint32_t kf = key[kBlock - 1], kb = key[0];
  const bool whole = ends == 1u << (kBlock - 1);              // one key fills the block
  const bool head_seg = head_cont && (kb & id_mask) < rows;   // a segment enters the block
  const bool fwd = tail_cont && (kf & id_mask) < rows;        // a segment leaves it
  const bool tail_seg = fwd && !(whole && head_cont);         // ... and starts in it
  if (!head_seg && !fwd) return;
  // A segment that reaches past the P probed blocks (flo == P, blo == P): the
  // rest of its extent by a (P + 1)-ary search over the remaining blocks, both
  // directions in the same rounds.  [lo, hi): the key holds at probe lo - 1
  // and at no probe >= hi.
  int fhi = (fwd && flo == P) ? nfwd : flo, bhi = (head_seg && blo == P) ? nbwd : blo;
  while (fhi > flo || bhi > blo) {
    const int fs = (fhi - flo + P) / (P + 1) + (fhi == flo), bs = (bhi - blo + P) / (P + 1) + (bhi == blo);  // >= 1
    const int fp = flo - 1 + (li + 1) * fs, bp = blo - 1 + (li + 1) * bs;  // fp >= flo: unknown probes only
    const bool fin = fp < fhi, bin = bp < bhi;
    const uint32_t fk = j.keys[b0 + (fin ? kBlock * (1 + fp) : 0)], bk = j.keys[b0 - (bin ? 1 + kBlock * bp : 0)];
    const int fc = __popcll(__ballot(fin && fk == kf) & gmask);  // equal probes: lanes 0 .. c-1 of the slot
    const int bc = __popcll(__ballot(bin && bk == kb) & gmask);
    if (fc < P && flo + (fc + 1) * fs - 1 < fhi) fhi = flo + (fc + 1) * fs - 1;
    if (bc < P && blo + (bc + 1) * bs - 1 < bhi) bhi = blo + (bc + 1) * bs - 1;
    flo += fc * fs;
    blo += bc * bs;
  }
  const int last = blk + flo;    // last block of the leaving segment
  const int first = blk - blo;   // first block of the entering segment
  const int head_last = (whole && fwd) ? last : blk;
  const int tail_start = kBlock - __clz(ends & ~(1u << (kBlock - 1)));  // first row of the block's last segment
  // every piece this wave stored has reached memory before its tickets are drawn
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint32_t* arrived = j.arrived + T.base / kBlock;
  uint32_t th = ~0u, tk = ~0u;  // both tickets in one round trip
  if (li == 0 && head_seg) th = __hip_atomic_fetch_add(&arrived[first], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (li == 0 && tail_seg) tk = __hip_atomic_fetch_add(&arrived[blk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // the ticket span - 1 is the last arriver's (~0u: no ticket drawn; a span is at most 2^19 blocks)
  const bool join_head = (__ballot(th == static_cast<uint32_t>(head_last - first)) & gmask) != 0;
  const bool join_tail = (__ballot(tk == static_cast<uint32_t>(last - blk)) & gmask) != 0;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the piece loads below the tickets
#pragma unroll 1
  for (int s = 0; s < 2; ++s) {
    if (!(s == 0 ? join_head : join_tail)) continue;
    const int f = s == 0 ? first : blk;
    int start_sorted = b0 + tail_start;
    if (OP == kWriteSum && s == 0) {  // the segment's first sorted index: the block's keys before it differ
      int same = 0;
      for (int r = li; r - li < kBlock; r += P)  // every lane of the slot takes every trip
        same += __popcll(__ballot(r < kBlock && j.keys[T.base + f * kBlock + min(r, kBlock - 1)] == kb) & gmask);
      start_sorted = T.base + (f + 1) * kBlock - same;
    }
    join_segment<OP>(j, T, ap, s == 0 ? kb : kf, start_sorted, f, s == 0 ? head_last : last, P, li);
    // a repeated apply on the same sorted keys starts from zero again
    if (li == 0) __hip_atomic_store(&arrived[f], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// kWriteSum only: compact the per-sorted-index sums into [U, dim] in id order.
__global__ void __launch_bounds__(1024) compact_kernel(const Job j, int32_t* out_uniq, float* out_sum,
                                                       int32_t* out_count) {
  const TableDesc& T = j.t[0];
  __shared__ int scratch[17];
  const int n = T.n_pad;
  const uint32_t mask = (1u << j.id_bits) - 1u;
  const int per = (n + 1023) / 1024;
  const int r0 = threadIdx.x * per, r1 = min(r0 + per, n);
  int heads = 0;
  for (int i = r0; i < r1; ++i) {
    const uint32_t k = j.keys[i];
    if ((k & mask) < static_cast<uint32_t>(T.num_rows) && (i == 0 || j.keys[i - 1] != k)) ++heads;
  }
  // block exclusive scan
  const int lane = lane_id(), w = threadIdx.x / kWave;
  int x = heads;
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const int y = __shfl_up(x, off, kWave);
    if (lane >= off) x += y;
  }
  if (lane == kWave - 1) scratch[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int i = 0; i < 16; ++i) {
      const int tt = scratch[i];
      scratch[i] = run;
      run += tt;
    }
    scratch[16] = run;
  }
  __syncthreads();
  int u = scratch[w] + x - heads;
  for (int i = r0; i < r1; ++i) {
    const uint32_t k = j.keys[i];
    if ((k & mask) < static_cast<uint32_t>(T.num_rows) && (i == 0 || j.keys[i - 1] != k)) {
      out_uniq[u] = static_cast<int32_t>(k & mask);
      for (int c = 0; c < T.dim; ++c) out_sum[static_cast<int64_t>(u) * T.dim + c] = j.dense_out[static_cast<int64_t>(i) * j.dense_dim + c];
      ++u;
    }
  }
  if (threadIdx.x == 0) *out_count = scratch[16];
}

int bits_for(int64_t x) {  // bits needed to represent values in [0, x]
  int b = 1;
  while ((int64_t(1) << b) <= x) ++b;
  return b;
}

int lanes_per_slot(int dim) {
  int p = 1;
  while (p < dim && p < kWave) p <<= 1;
  return p;
}

// Host-side plan of one launch group (<= kTablesPerLaunch tables).
struct Plan {
  Job job;
  int total;          // sorted elements
  int waves;          // block-kernel waves
  int64_t piece_floats;
  size_t sort_bytes;
  int end_bit;
};

// grad / grad_stride: the call's gradient (tables may override it); NULL for
// a workspace-size query.
int make_plan(const tt_sparse_table* tables, int cnt, int64_t batch, const float* grad, int64_t grad_stride,
              Plan* p, bool size_query = false) {
  Job& j = p->job;
  j = Job{};
  j.num = cnt;
  j.batch = batch;
  int64_t max_rows = 1;
  for (int i = 0; i < cnt; ++i) max_rows = std::max<int64_t>(max_rows, tables[i].num_rows);
  j.id_bits = bits_for(max_rows);  // (1<<id_bits)-1 >= max_rows: never a valid row
  const int table_bits = bits_for(std::max(cnt - 1, 1));
  p->end_bit = j.id_bits + table_bits;
  if (p->end_bit > 32) return fail(TT_ERR_UNSUPPORTED, "sparse: %d tables x %lld rows exceed 32-bit keys", cnt,
                                   static_cast<long long>(max_rows));
  int base = 0, waves = 0, chunks = 0;
  int64_t poff = 0;
  for (int i = 0; i < cnt; ++i) {
    const tt_sparse_table& s = tables[i];
    TableDesc& T = j.t[i];
    for (int q = 0; q < TT_MAX_SOURCES; ++q) {
      T.ids[q] = (q < s.num_sources) ? s.ids[q] : nullptr;
      T.goff[q] = (q < s.num_sources) ? s.grad_col_offset[q] : 0;
    }
    T.grad = s.grad ? s.grad : grad;
    T.gld = static_cast<int32_t>(s.grad ? s.grad_ld : grad_stride);
    if (batch > 0 && !T.grad && !size_query) return fail(TT_ERR_BAD_ARG, "sparse: table %d has no gradient (NULL grad)", i);
    int32_t max_off = 0;
    for (int q = 0; q < s.num_sources; ++q) max_off = std::max(max_off, s.grad_col_offset[q]);
    const int64_t gld = s.grad ? s.grad_ld : grad_stride;
    if (gld < 0 || max_off < 0 || (batch > 0 && (batch - 1) * gld + max_off + s.dim >= (int64_t(1) << 31)))
      return fail(TT_ERR_UNSUPPORTED, "sparse: table %d gradient rows exceed 2^31 floats", i);
    T.table = s.table;
    T.slot0 = s.slot0;
    T.slot1 = s.slot1;
    T.num_rows = s.num_rows;
    T.dim = s.dim;
    T.num_sources = s.num_sources;
    T.n = static_cast<int32_t>(s.num_sources * batch);
    T.base = base;
    T.n_pad = static_cast<int32_t>(round_up(std::max<int64_t>(T.n, 1), kBlock));
    T.lanes = lanes_per_slot(s.dim);
    T.chunk_begin = chunks;
    T.piece_off = poff;
    base += T.n_pad;
    chunks += static_cast<int>(ceil_div(T.n_pad, kChunk));
    poff += static_cast<int64_t>(T.n_pad / kBlock) * 2 * s.dim;
  }
  // Wave order of the block launch: tables of at most kSmallRows rows first.
  // Their blocks are nearly all pieces of long segments and load no row state,
  // so their joins run under the large tables' row traffic, not after it.
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < cnt; ++i) {
      TableDesc& T = j.t[i];
      if ((T.num_rows <= kSmallRows) != (pass == 0)) continue;
      T.wave_begin = waves;
      waves += static_cast<int>(ceil_div(T.n_pad / kBlock, kWave / T.lanes));
    }
  p->total = base;
  p->waves = waves;
  j.num_chunks = chunks;
  p->piece_floats = poff;
  // fingerprint of what the sort stage sorts (ids, tables, batch): two
  // independent 32-bit FNV-1a hashes
  uint32_t h0 = 2166136261u, h1 = 0x9747b28cu;
  auto mix = [&](uint64_t v) {
    for (int b = 0; b < 8; ++b) {
      const uint32_t byte = static_cast<uint32_t>(v >> (8 * b)) & 0xFFu;
      h0 = (h0 ^ byte) * 16777619u;
      h1 = (h1 ^ (byte + 0x5bu)) * 0x01000193u + 0x3c6ef372u;
    }
  };
  mix(static_cast<uint64_t>(batch));
  mix(static_cast<uint64_t>(cnt));
  for (int i = 0; i < cnt; ++i) {
    const tt_sparse_table& s = tables[i];
    mix(reinterpret_cast<uintptr_t>(s.table));
    mix(static_cast<uint64_t>(s.num_rows));
    mix((static_cast<uint64_t>(s.dim) << 32) | static_cast<uint32_t>(s.num_sources));
    for (int q = 0; q < s.num_sources; ++q) mix(reinterpret_cast<uintptr_t>(s.ids[q]));
  }
  j.fp0 = h0;
  j.fp1 = h1;
  size_t sb = 0;
  uint32_t* np = nullptr;
  hipError_t e = rocprim::radix_sort_pairs<SortConfig>(nullptr, sb, np, np, np, np, static_cast<unsigned>(base), 0, p->end_bit,
                                           nullptr, false);
  // rocPRIM picks its config from the device; on a host without one (size
  // queries only) use a bound: a key/value ping-pong copy plus 4 MiB.
  p->sort_bytes = (e == hipSuccess) ? sb : static_cast<size_t>(base) * 8 + (size_t(4) << 20);
  return TT_OK;
}

// Workspace carve for one plan (also used for the size query with base=null).
struct PlanWs {
  SparseHeader* hdr;
  uint32_t *keys_in, *vals_in, *keys, *vals;
  float* pieces;
  uint32_t* arrived;
  uint32_t* chunk_hist;
  float* dense_out;
  void* sort_tmp;
};
PlanWs carve_plan(Carver& cv, const Plan& p, int dense_dim) {
  PlanWs w;
  w.hdr = reinterpret_cast<SparseHeader*>(cv.take<char>(kHdrBytes));  // always at offset 0
  w.keys_in = cv.take<uint32_t>(p.total);
  w.vals_in = cv.take<uint32_t>(p.total);
  w.keys = cv.take<uint32_t>(p.total);
  w.vals = cv.take<uint32_t>(p.total);
  w.pieces = cv.take<float>(std::max<int64_t>(p.piece_floats, 1));
  w.arrived = cv.take<uint32_t>(p.total / kBlock);  // one join counter per block
  w.chunk_hist = cv.take<uint32_t>(static_cast<int64_t>(p.job.num_chunks) * 256);
  w.dense_out = dense_dim > 0 ? cv.take<float>(static_cast<int64_t>(p.total) * dense_dim) : nullptr;
  w.sort_tmp = cv.take<char>(static_cast<int64_t>(p.sort_bytes) + 256);
  return w;
}

int validate_tables(const tt_sparse_table* tables, int32_t num_tables, int64_t batch, bool adam,
                    bool need_slot0 = true) {
  TT_REQUIRE(tables != nullptr && num_tables >= 1, "sparse: no tables");
  TT_REQUIRE(batch >= 0, "sparse: negative batch");
  int64_t total = 0;
  for (int i = 0; i < num_tables; ++i) {
    const tt_sparse_table& t = tables[i];
    TT_REQUIRE(t.table && (t.slot0 || !need_slot0), "sparse: table %d has NULL parameter/slot pointer", i);
    TT_REQUIRE(!adam || t.slot1, "sparse: table %d needs slot1 for Adam", i);
    TT_REQUIRE(t.num_rows >= 1 && t.num_rows < (int64_t(1) << 30), "sparse: table %d num_rows out of range", i);
    TT_REQUIRE(t.dim >= 1 && t.dim <= 4096, "sparse: table %d dim=%d out of range", i, t.dim);
    TT_REQUIRE(t.num_sources >= 1 && t.num_sources <= TT_MAX_SOURCES, "sparse: table %d num_sources=%d", i,
               t.num_sources);
    for (int s = 0; s < t.num_sources; ++s) TT_REQUIRE(t.ids[s] || batch == 0, "sparse: table %d source %d ids NULL", i, s);
    total += t.num_sources * batch;
  }
  TT_REQUIRE(total < kMaxLookups, "sparse: %lld lookups in one call (max %lld)", static_cast<long long>(total),
             static_cast<long long>(kMaxLookups));
  return TT_OK;
}

size_t tables_ws_bytes(const tt_sparse_table* tables, int32_t num_tables, int64_t batch, int dense_dim) {
  size_t total = 0;
  for (int first = 0; first < num_tables; first += kTablesPerLaunch) {
    const int cnt = std::min(num_tables - first, kTablesPerLaunch);
    Plan p;
    if (make_plan(tables + first, cnt, batch, nullptr, 0, &p, true)) return 0;
    Carver cv(nullptr, 0);
    carve_plan(cv, p, dense_dim);
    total = std::max(total, cv.used());
  }
  return total;
}

// Stages: the key build + sort depends only on the ids, so a caller may run
// it early on a side stream (kStageSort) and the gradient-dependent block
// launch (sums, joins, applies) later (kStageApply) with the same tables, batch
// and workspace.
enum SparseStage { kStageAll = 0, kStageSort = 1, kStageApply = 2 };

template <int OP>
int run_sparse(const tt_sparse_table* tables, int32_t num_tables, int64_t batch, const float* grad,
               int64_t grad_stride, const ApplyParams& ap, void* workspace, size_t ws_bytes, hipStream_t st,
               int32_t* out_uniq = nullptr, float* out_sum = nullptr, int32_t* out_count = nullptr,
               int stage = kStageAll) {
  TT_REQUIRE(batch < (int64_t(1) << kSrcShift), "sparse: batch %lld too large", static_cast<long long>(batch));
  TT_REQUIRE(stage == kStageAll || num_tables <= kTablesPerLaunch,
             "sparse: a split sort/apply call takes at most %d tables", kTablesPerLaunch);
  for (int first = 0; first < num_tables; first += kTablesPerLaunch) {
    const int cnt = std::min(num_tables - first, kTablesPerLaunch);
    Plan p;
    int rc = make_plan(tables + first, cnt, batch, grad, grad_stride, &p, stage == kStageSort);
    if (rc) return rc;
    Carver cv(workspace, ws_bytes);
    const int dense_dim = (OP == kWriteSum) ? tables[first].dim : 0;
    PlanWs w = carve_plan(cv, p, dense_dim);
    if (cv.used() > ws_bytes) return fail(TT_ERR_WORKSPACE, "sparse: workspace %zu < required %zu", ws_bytes, cv.used());
    Job& j = p.job;
    j.keys_in = w.keys_in;
    j.vals_in = w.vals_in;
    j.keys = w.keys;
    j.vals = w.vals;
    j.pieces = w.pieces;
    j.arrived = w.arrived;
    j.chunk_hist = w.chunk_hist;
    j.dense_out = w.dense_out;
    j.dense_dim = dense_dim;
    j.hdr = w.hdr;
    if (stage != kStageApply) {
      // by size alone: the chunked sort when every region fits its merge, else
      // the small-table sort when every table is small (row keys of <= 8
      // bits), else key build + rocPRIM
      bool chunked = true, all_small = true;
      int merge_chunks = 0;  // most chunks of a large-key region: the merge's LDS
      int staged = 0;        // longest region the small-table sort stages in LDS
      for (int i = 0; i < cnt; ++i) {
        const bool small = bits_for(j.t[i].num_rows) <= 8;
        all_small = all_small && small;
        chunked = chunked && j.t[i].n_pad <= (small ? kChunkMaxSmall : kChunkMaxLarge);
        if (!small) merge_chunks = std::max(merge_chunks, static_cast<int>(ceil_div(j.t[i].n_pad, kChunk)));
        if (j.t[i].n_pad <= kStStageMax) staged = std::max(staged, j.t[i].n_pad);
      }
      if (chunked) {
        hipLaunchKernelGGL(chunk_sort_kernel, dim3(j.num_chunks), dim3(kCsThreads), 0, st, j);
        TT_CHECK_LAUNCH();
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(chunk_merge_kernel),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, kMergeLdsMax);
        TT_CHECK_HIP(attr);
        hipLaunchKernelGGL(chunk_merge_kernel, dim3(j.num_chunks), dim3(kCsThreads), merge_chunks * kChunk * 4, st,
                           j);
        TT_CHECK_LAUNCH();
      } else if (all_small) {
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void*>(small_table_sort_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, StHist::kWords * 4 + kStStageMax);
        TT_CHECK_HIP(attr);
        hipLaunchKernelGGL(small_table_sort_kernel, dim3(cnt), dim3(kStThreads), StHist::kWords * 4 + staged, st, j);
        TT_CHECK_LAUNCH();
      } else {
        hipLaunchKernelGGL(build_keys_kernel, dim3(ceil_div(p.total, kThreads)), dim3(kThreads), 0, st, j, p.total);
        TT_CHECK_LAUNCH();
        size_t sb = p.sort_bytes;
        TT_CHECK_HIP(rocprim::radix_sort_pairs<SortConfig>(w.sort_tmp, sb, w.keys_in, w.keys, w.vals_in, w.vals,
                                               static_cast<unsigned>(p.total), 0, p.end_bit, st, false));
      }
    }
    if (stage == kStageSort) continue;
    const int blocks = static_cast<int>(ceil_div(p.waves, kThreads / kWave));
    hipLaunchKernelGGL(block_sum_kernel<OP>, dim3(blocks), dim3(kThreads), 0, st, j, ap);
    TT_CHECK_LAUNCH();
    if (OP == kWriteSum) {
      hipLaunchKernelGGL(compact_kernel, dim3(1), dim3(1024), 0, st, j, out_uniq, out_sum, out_count);
      TT_CHECK_LAUNCH();
    }
  }
  return TT_OK;
}

// Dense elementwise passes (grid-stride).
__global__ void scale2_kernel(float* a, float sa, float* b, float sb, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    a[i] = ieee_op<'*'>(a[i], sa);
    b[i] = ieee_op<'*'>(b[i], sb);
  }
}

// Legacy Adam sparse path, final dense step: var -= lr*m / (sqrt(v) + eps).
__global__ void adam_var_kernel(float* var, const float* m, const float* v, float lr, float eps, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    var[i] = ieee_op<'-'>(var[i], ieee_op<'/'>(ieee_op<'*'>(lr, m[i]), ieee_op<'+'>(sqrtf(v[i]), eps)));
}

// ResourceApplyAdagradV2: accum += g^2; var -= g*lr / (sqrt(accum) + eps).
__global__ void dense_adagrad_kernel(float* p, float* acc, const float* g, int64_t n, float lr, float eps) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i];
    const float a = ieee_op<'+'>(acc[i], ieee_op<'*'>(gi, gi));
    acc[i] = a;
    p[i] = ieee_op<'-'>(p[i], ieee_op<'/'>(ieee_op<'*'>(gi, lr), ieee_op<'+'>(sqrtf(a), eps)));
  }
}

// ResourceApplyAdam (use_nesterov=false):
//   m += (g - m)*(1-b1); v += (g*g - v)*(1-b2); var -= m*alpha / (sqrt(v) + eps)
// tt_dense_adagrad on up to kDenseMaxJobs buffers in one launch: a
// grid-stride loop over their concatenation (the same per-element arithmetic)
constexpr int kDenseMaxJobs = 8;
struct DenseJobs {
  float* p[kDenseMaxJobs];
  float* acc[kDenseMaxJobs];
  const float* g[kDenseMaxJobs];
  int64_t begin[kDenseMaxJobs + 1];
  int num;
  float lr, eps;
};
__global__ void dense_adagrad_many_kernel(const DenseJobs d) {
  const int64_t total = d.begin[d.num];
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int t = 0;
#pragma unroll 1
    for (int q = 1; q < d.num; ++q)
      if (i >= d.begin[q]) t = q;
    const int64_t k = i - d.begin[t];
    const float gi = d.g[t][k];
    const float a = ieee_op<'+'>(d.acc[t][k], ieee_op<'*'>(gi, gi));
    d.acc[t][k] = a;
    d.p[t][k] = ieee_op<'-'>(d.p[t][k], ieee_op<'/'>(ieee_op<'*'>(gi, d.lr), ieee_op<'+'>(sqrtf(a), d.eps)));
  }
}

__global__ void dense_adam_kernel(float* p, float* m, float* v, const float* g, int64_t n, float alpha,
                                  float omb1, float omb2, float eps) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = g[i];
    const float mi = ieee_op<'+'>(m[i], ieee_op<'*'>(ieee_op<'-'>(gi, m[i]), omb1));
    const float vi = ieee_op<'+'>(v[i], ieee_op<'*'>(ieee_op<'-'>(ieee_op<'*'>(gi, gi), v[i]), omb2));
    m[i] = mi;
    v[i] = vi;
    p[i] = ieee_op<'-'>(p[i], ieee_op<'/'>(ieee_op<'*'>(mi, alpha), ieee_op<'+'>(sqrtf(vi), eps)));
  }
}

// ---- Adam with the step count in device memory (tt_adam_clock) ------------
// The host entries above take `step` and compute their coefficient with the
// host's powf; a captured graph cannot.  The _dev entries read the step's
// coefficients from a tt_adam_clock that one tiny launch advances from a
// host-filled table (tt_adam_coef_fill), so a replay takes the next step's
// pair without any host work, and the pair is the host entries' to the bit.
__global__ void adam_clock_kernel(tt_adam_clock* c, const float* alpha_tab, const float* lr_t_tab, int64_t len) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t s = c->step + 1;
  int64_t k = (s < len ? s : len) - 1;  // past the table's end both coefficients stay at its last entry
  if (k < 0) k = 0;
  c->step = s;
  c->alpha = alpha_tab[k];
  c->lr_t = lr_t_tab[k];
}

// dense_adam_kernel on up to kDenseMaxJobs buffers in one launch, alpha from
// the clock (dense_adagrad_many_kernel's loop over the concatenation)
struct DenseAdamJobs {
  float* p[kDenseMaxJobs];
  float* m[kDenseMaxJobs];
  float* v[kDenseMaxJobs];
  const float* g[kDenseMaxJobs];
  int64_t begin[kDenseMaxJobs + 1];
  int num;
  float omb1, omb2, eps;
  const tt_adam_clock* clock;
};
__global__ void dense_adam_many_dev_kernel(const DenseAdamJobs d) {
  const int64_t total = d.begin[d.num];
  const float alpha = d.clock->alpha;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int t = 0;
#pragma unroll 1
    for (int q = 1; q < d.num; ++q)
      if (i >= d.begin[q]) t = q;
    const int64_t k = i - d.begin[t];
    const float gi = d.g[t][k];
    const float m0 = d.m[t][k], v0 = d.v[t][k];
    const float mi = ieee_op<'+'>(m0, ieee_op<'*'>(ieee_op<'-'>(gi, m0), d.omb1));
    const float vi = ieee_op<'+'>(v0, ieee_op<'*'>(ieee_op<'-'>(ieee_op<'*'>(gi, gi), v0), d.omb2));
    d.m[t][k] = mi;
    d.v[t][k] = vi;
    d.p[t][k] = ieee_op<'-'>(d.p[t][k], ieee_op<'/'>(ieee_op<'*'>(mi, alpha), ieee_op<'+'>(sqrtf(vi), d.eps)));
  }
}

// The two whole-table stages of the legacy sparse Adam step (scale2_kernel and
// adam_var_kernel, the same per-element arithmetic) over up to kAdamMaxTables
// tables in ONE launch each.  Pure streaming: a thread takes a unit of 4
// consecutive elements of one table (found by a search over the prefix sums of
// the tables' unit counts) with 16-byte accesses when the table's three bases
// are 16-byte aligned; a table's last, shorter unit and unaligned tables take
// the elements one by one.  The grid is capped at 8 blocks per CU and strides.
constexpr int kAdamMaxTables = 16;
constexpr int kAdamUnit = 4;
constexpr int kAdamGridMax = 2048;
struct AdamTables {
  float* var[kAdamMaxTables];
  float* m[kAdamMaxTables];
  float* v[kAdamMaxTables];
  int64_t n[kAdamMaxTables];          // elements
  int64_t begin[kAdamMaxTables + 1];  // prefix sums of ceil(n / kAdamUnit)
  uint32_t vec;                       // bit t: table t takes 16-byte accesses
  int num;
};

__device__ __forceinline__ int adam_table_of(const AdamTables& d, int64_t u) {
  int t = 0;
#pragma unroll 1
  for (int q = 1; q < d.num; ++q)
    if (u >= d.begin[q]) t = q;
  return t;
}

__global__ void __launch_bounds__(256) adam_decay_many_kernel(const AdamTables d, float b1, float b2) {
  const int64_t total = d.begin[d.num];
  for (int64_t u = blockIdx.x * (int64_t)256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int t = adam_table_of(d, u);
    const int64_t e = (u - d.begin[t]) * kAdamUnit, left = d.n[t] - e;
    float* m = d.m[t] + e;
    float* v = d.v[t] + e;
    if (((d.vec >> t) & 1u) && left >= kAdamUnit) {
      f32x4 a = *reinterpret_cast<const f32x4*>(m), b = *reinterpret_cast<const f32x4*>(v);
#pragma unroll
      for (int c = 0; c < kAdamUnit; ++c) {
        a[c] = ieee_op<'*'>(a[c], b1);
        b[c] = ieee_op<'*'>(b[c], b2);
      }
      *reinterpret_cast<f32x4*>(m) = a;
      *reinterpret_cast<f32x4*>(v) = b;
    } else {
      const int cnt = left < kAdamUnit ? static_cast<int>(left) : kAdamUnit;
      for (int c = 0; c < cnt; ++c) {
        m[c] = ieee_op<'*'>(m[c], b1);
        v[c] = ieee_op<'*'>(v[c], b2);
      }
    }
  }
}

__global__ void __launch_bounds__(256) adam_var_many_kernel(const AdamTables d, const tt_adam_clock* clock,
                                                            float eps) {
  const int64_t total = d.begin[d.num];
  const float lr = clock->lr_t;
  for (int64_t u = blockIdx.x * (int64_t)256 + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int t = adam_table_of(d, u);
    const int64_t e = (u - d.begin[t]) * kAdamUnit, left = d.n[t] - e;
    float* var = d.var[t] + e;
    const float* m = d.m[t] + e;
    const float* v = d.v[t] + e;
    if (((d.vec >> t) & 1u) && left >= kAdamUnit) {
      f32x4 x = *reinterpret_cast<const f32x4*>(var);
      const f32x4 a = *reinterpret_cast<const f32x4*>(m), b = *reinterpret_cast<const f32x4*>(v);
#pragma unroll
      for (int c = 0; c < kAdamUnit; ++c)
        x[c] = ieee_op<'-'>(x[c], ieee_op<'/'>(ieee_op<'*'>(lr, a[c]), ieee_op<'+'>(sqrtf(b[c]), eps)));
      *reinterpret_cast<f32x4*>(var) = x;
    } else {
      const int cnt = left < kAdamUnit ? static_cast<int>(left) : kAdamUnit;
      for (int c = 0; c < cnt; ++c)
        var[c] = ieee_op<'-'>(var[c], ieee_op<'/'>(ieee_op<'*'>(lr, m[c]), ieee_op<'+'>(sqrtf(v[c]), eps)));
    }
  }
}

// Adagrad on rows that are distinct (tt_sparse_adagrad_rows): slot j applies
// grad row j to row rows[j] of table tags[j]; one thread per 4 columns of a
// slot (dim % 4 == 0) or per column.  g = 0 + (0 + grad): the block sums'
// arithmetic for a segment of one lookup, so the result is bit-identical to
// tt_sparse_adagrad on the same (distinct) rows.
constexpr int kRowsMaxTables = 16;
struct RowsArgs {
  float* table[kRowsMaxTables];
  float* slot0[kRowsMaxTables];
  int64_t num_rows[kRowsMaxTables];
  int num_tables;
  int dim;
  const int32_t* tags;
  const int32_t* rows;
  int64_t n;
  const float* grad;
  int64_t grad_ld;
  float lr, eps;
};

__device__ __forceinline__ void adagrad_elem(float* tab, float* acc, float gsrc, float lr, float eps) {
  const float g = ieee_op<'+'>(0.0f, ieee_op<'+'>(0.0f, gsrc));
  const float a = ieee_op<'+'>(*acc, ieee_op<'*'>(g, g));
  *acc = a;
  *tab = ieee_op<'-'>(*tab, ieee_op<'/'>(ieee_op<'*'>(lr, g), ieee_op<'+'>(sqrtf(a), eps)));
}

template <bool V4>
__global__ void __launch_bounds__(256) adagrad_rows_kernel(const RowsArgs a) {
  const int per = V4 ? a.dim / 4 : a.dim;  // threads per slot
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t j = i / per;
  if (j >= a.n) return;
  const int c = static_cast<int>(i - j * per) * (V4 ? 4 : 1);
  const int t = a.tags[j];
  const int64_t r = a.rows[j];
  if (t < 0 || t >= a.num_tables || r < 0 || r >= a.num_rows[t]) return;
  const int64_t o = r * a.dim + c;
  const float* gp = a.grad + j * a.grad_ld + c;
  if constexpr (V4) {
    f32x4 tv = *reinterpret_cast<const f32x4*>(a.table[t] + o);
    f32x4 av = *reinterpret_cast<const f32x4*>(a.slot0[t] + o);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(gp);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float tt = tv[e], aa = av[e];
      adagrad_elem(&tt, &aa, gv[e], a.lr, a.eps);
      tv[e] = tt;
      av[e] = aa;
    }
    *reinterpret_cast<f32x4*>(a.slot0[t] + o) = av;
    *reinterpret_cast<f32x4*>(a.table[t] + o) = tv;
  } else {
    adagrad_elem(a.table[t] + o, a.slot0[t] + o, *gp, a.lr, a.eps);
  }
}

// Keys of a routed call (tt_sparse_routed) taken from the route's own sort:
// the route lists lookups by (owner, tag, row, lookup), so table i's lookups
// (one tag) in slot order are that tag's route positions in order, and a
// lookup's sorted position in the table's region is its rank among them:
// (lookups of the tag at earlier owners) + (its offset in its (owner, tag)
// group).  One thread per route position writes the (table | key, source |
// batch row) pair the sort stage would have written; the trailing threads
// write each region's padding.  Every block first turns the group sizes into
// per-tag prefixes over the owners in LDS (world <= 1024, world * tags <=
// kRoutedMaxGroups).
constexpr int kRoutedMaxLookups = TT_ROUTE_MAX_LOOKUPS;
constexpr int kRoutedMaxGroups = 4096;
constexpr int kRoutedThreads = 1024;
struct RoutedArgs {
  const int32_t* order;
  const int32_t* grp_first;
  const int32_t* grp_last;
  const int32_t* slot;
  const int32_t* slot_row;
  int64_t cap;
  int64_t total;  // routed lookups = num_lookups * batch
  int32_t world, num_tags, num_lookups, num_tables;
  int32_t lk_tag[kRoutedMaxLookups];
  uint32_t lk_khi[kRoutedMaxLookups];   // table index << id_bits
  uint32_t lk_shi[kRoutedMaxLookups];   // source << kSrcShift
  int32_t lk_base[kRoutedMaxLookups];   // region start of the lookup's table
  int32_t pad_begin[kTablesPerLaunch + 1];  // prefix of the regions' padding entries
  int32_t pad_dst[kTablesPerLaunch];        // first padding position of each region
  uint32_t pad_key[kTablesPerLaunch];       // (table << id_bits) | invalid
};

__global__ void __launch_bounds__(kRoutedThreads) routed_keys_kernel(const Job j, const RoutedArgs r) {
  __shared__ int pre[kRoutedMaxGroups];
  __shared__ int wsum[kRoutedThreads / kWave];
  const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
  const int T = r.num_tags, G = r.world * r.num_tags;
  for (int g = tid; g < G; g += kRoutedThreads) pre[g] = r.grp_last[g] - r.grp_first[g] + 1;
  for (int t = 0; t < T; ++t) {  // exclusive prefix over the owners, per tag
    __syncthreads();
    const int v = tid < r.world ? pre[tid * T + t] : 0;
    int x = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int y = __shfl_up(x, o, kWave);
      if (lane >= o) x += y;
    }
    if (lane == kWave - 1) wsum[w] = x;
    __syncthreads();
    int ex = x - v;
    for (int q = 0; q < w; ++q) ex += wsum[q];
    if (tid < r.world) pre[tid * T + t] = ex;
  }
  __syncthreads();
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kRoutedThreads + tid;
  const uint32_t invalid = (1u << j.id_bits) - 1u;
  if (i < r.total) {
    const int lk = r.order[i];
    const int l = static_cast<int>(lk / j.batch);
    const int b = static_cast<int>(lk - static_cast<int64_t>(l) * j.batch);
    // a request dropped by a small route capacity carries the slot sentinel
    // -1 - owner: its lookups keep their place in the (owner, tag) group and
    // take the invalid key with no gradient (like an out-of-range id: never
    // applied, never written — an invalid run may sit mid-region; block_sum
    // and its join only need equal keys contiguous)
    const int s = r.slot[lk];
    const int o = s >= 0 ? static_cast<int>(s / r.cap) : -1 - s;
    const int g = o * T + r.lk_tag[l];
    const int dst = r.lk_base[l] + pre[g] + static_cast<int>(i - r.grp_first[g]);
    uint32_t id = s >= 0 ? static_cast<uint32_t>(s) : invalid;
    if (r.slot_row && s >= 0) {
      const int32_t row = r.slot_row[s];
      id = row >= 0 ? static_cast<uint32_t>(row) : invalid;
    }
    const_cast<uint32_t*>(j.keys)[dst] = r.lk_khi[l] | id;
    const_cast<uint32_t*>(j.vals)[dst] = id == invalid ? 0xFFFFFFFFu : (r.lk_shi[l] | static_cast<uint32_t>(b));
  } else {
    const int k = static_cast<int>(i - r.total);
    int t = 0;
#pragma unroll 1
    for (int q = 1; q < r.num_tables; ++q)
      if (k >= r.pad_begin[q]) t = q;
    if (k < r.pad_begin[r.num_tables]) {
      const int dst = r.pad_dst[t] + (k - r.pad_begin[t]);
      const_cast<uint32_t*>(j.keys)[dst] = r.pad_key[t];
      const_cast<uint32_t*>(j.vals)[dst] = 0xFFFFFFFFu;
    }
  }
  if (i < r.total + r.pad_begin[r.num_tables] && i % kBlock == 0) j.arrived[i / kBlock] = 0u;  // join counters
  if (i == 0) stamp_header(j);
}

dim3 stride_grid(int64_t n) {
  int64_t b = ceil_div(n, 256);
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return dim3(static_cast<unsigned>(b));
}

// The step-dependent part of Adam, in fp32 with the host's powf: the ONE place
// the coefficients are computed (tt_dense_adam, tt_sparse_adam and the table
// fill of the device clock all call it).
//   alpha: TF ApplyAdamOp, (lr * sqrt(1 - beta2^t)) / (1 - beta1^t)
//   lr_t:  legacy Adam._prepare_local, lr * (sqrt(1 - beta2^t) / (1 - beta1^t))
// saturated: 1 - beta^t == 1 for both betas, so both coefficients are lr itself.
struct AdamCoef {
  float alpha, lr_t;
  bool saturated;
};
AdamCoef adam_coef(float lr, float beta1, float beta2, int64_t step) {
  const float b1p = powf(beta1, static_cast<float>(step));
  const float b2p = powf(beta2, static_cast<float>(step));
  const float rad = 1.0f - b2p, den = 1.0f - b1p;
  AdamCoef c;
  c.alpha = (lr * sqrtf(rad)) / den;
  c.lr_t = lr * (sqrtf(rad) / den);
  c.saturated = rad == 1.0f && den == 1.0f;
  return c;
}

bool adam_beta_ok(float b) { return b >= 0.0f && b < 1.0f; }  // false for NaN

constexpr int64_t kAdamCoefMaxLen = int64_t(1) << 22;

// Whole-table launches of tt_sparse_adam_dev over tables [first, first + cnt).
AdamTables adam_tables(const tt_sparse_table* tables, int cnt) {
  AdamTables d{};
  d.num = cnt;
  int64_t units = 0;
  for (int i = 0; i < cnt; ++i) {
    const tt_sparse_table& t = tables[i];
    d.var[i] = t.table;
    d.m[i] = t.slot0;
    d.v[i] = t.slot1;
    d.n[i] = t.num_rows * t.dim;
    d.begin[i] = units;
    units += ceil_div(d.n[i], static_cast<int64_t>(kAdamUnit));
    const uintptr_t bits = reinterpret_cast<uintptr_t>(t.table) | reinterpret_cast<uintptr_t>(t.slot0) |
                           reinterpret_cast<uintptr_t>(t.slot1);
    if (bits % 16 == 0) d.vec |= 1u << i;
  }
  d.begin[cnt] = units;
  return d;
}

dim3 adam_grid(int64_t units) {
  return dim3(static_cast<unsigned>(std::min<int64_t>(std::max<int64_t>(ceil_div(units, int64_t(256)), 1), kAdamGridMax)));
}

}  // namespace
}  // namespace tt

using namespace tt;

extern "C" size_t tt_sparse_workspace_size(const tt_sparse_table* tables, int32_t num_tables, int64_t batch) {
  if (!tables || num_tables < 1 || batch < 0) return 0;
  return tables_ws_bytes(tables, num_tables, batch, 0);
}

namespace tt {
namespace {
int sparse_adagrad_stage(const tt_sparse_table* tables, int32_t num_tables, int64_t batch, const float* grad,
                         int64_t grad_stride, float lr, float epsilon, void* workspace, size_t workspace_bytes,
                         tt_stream_t stream, int stage, const char* name) {
  clear_error();
  // the sort stage reads only the ids: no slot needed (also sorts for a scatter sum)
  int rc = validate_tables(tables, num_tables, batch, false, stage != kStageSort);
  if (rc) return rc;
  if (batch == 0) return TT_OK;
  const size_t need = tables_ws_bytes(tables, num_tables, batch, 0);
  if (!workspace || workspace_bytes < need)
    return fail(TT_ERR_WORKSPACE, "%s: workspace %zu < required %zu", name, workspace_bytes, need);
  ApplyParams ap{};
  ap.lr = lr;
  ap.eps = epsilon;
  return run_sparse<kAdagrad>(tables, num_tables, batch, grad, grad_stride, ap, workspace, workspace_bytes,
                              to_stream(stream), nullptr, nullptr, nullptr, stage);
}
}  // namespace
}  // namespace tt

extern "C" int tt_sparse_adagrad(const tt_sparse_table* tables, int32_t num_tables, int64_t batch,
                                 const float* grad, int64_t grad_stride, float lr, float epsilon,
                                 void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  return sparse_adagrad_stage(tables, num_tables, batch, grad, grad_stride, lr, epsilon, workspace, workspace_bytes,
                              stream, kStageAll, "tt_sparse_adagrad");
}

extern "C" int tt_sparse_sort(const tt_sparse_table* tables, int32_t num_tables, int64_t batch, void* workspace,
                              size_t workspace_bytes, tt_stream_t stream) {
  return sparse_adagrad_stage(tables, num_tables, batch, nullptr, 0, 0.0f, 0.0f, workspace, workspace_bytes, stream,
                              kStageSort, "tt_sparse_sort");
}

extern "C" int tt_sparse_adagrad_sorted(const tt_sparse_table* tables, int32_t num_tables, int64_t batch,
                                        const float* grad, int64_t grad_stride, float lr, float epsilon,
                                        void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  return sparse_adagrad_stage(tables, num_tables, batch, grad, grad_stride, lr, epsilon, workspace, workspace_bytes,
                              stream, kStageApply, "tt_sparse_adagrad_sorted");
}

extern "C" int tt_sparse_adam(const tt_sparse_table* tables, int32_t num_tables, int64_t batch,
                              const float* grad, int64_t grad_stride, float lr, float beta1, float beta2,
                              float epsilon, int64_t step, void* workspace, size_t workspace_bytes,
                              tt_stream_t stream) {
  clear_error();
  int rc = validate_tables(tables, num_tables, batch, true);
  if (rc) return rc;
  TT_REQUIRE(step >= 1, "tt_sparse_adam: step must be >= 1");
  const size_t need = tables_ws_bytes(tables, num_tables, batch, 0);
  if (batch > 0 && (!workspace || workspace_bytes < need))
    return fail(TT_ERR_WORKSPACE, "tt_sparse_adam: workspace %zu < required %zu", workspace_bytes, need);
  hipStream_t st = to_stream(stream);
  // Coefficients exactly as legacy Adam._prepare_local computes them in fp32.
  const float b1 = beta1, b2 = beta2;
  const float lr_t = adam_coef(lr, beta1, beta2, step).lr_t;
  for (int i = 0; i < num_tables; ++i) {
    const int64_t n = tables[i].num_rows * tables[i].dim;
    hipLaunchKernelGGL(scale2_kernel, stride_grid(n), dim3(256), 0, st, tables[i].slot0, b1, tables[i].slot1, b2, n);
    TT_CHECK_LAUNCH();
  }
  if (batch > 0) {
    ApplyParams ap{};
    ap.one_minus_beta1 = 1.0f - b1;
    ap.one_minus_beta2 = 1.0f - b2;
    rc = run_sparse<kAdamScatter>(tables, num_tables, batch, grad, grad_stride, ap, workspace, workspace_bytes, st);
    if (rc) return rc;
  }
  for (int i = 0; i < num_tables; ++i) {
    const int64_t n = tables[i].num_rows * tables[i].dim;
    hipLaunchKernelGGL(adam_var_kernel, stride_grid(n), dim3(256), 0, st, tables[i].table, tables[i].slot0,
                       tables[i].slot1, lr_t, epsilon, n);
    TT_CHECK_LAUNCH();
  }
  return TT_OK;
}

extern "C" size_t tt_dedup_workspace_size(int64_t n, int32_t dim) {
  if (n < 1 || dim < 1) return 0;
  tt_sparse_table t{};
  t.num_rows = (int64_t(1) << 30) - 1;  // worst case key bits
  t.dim = dim;
  t.num_sources = 1;
  return tables_ws_bytes(&t, 1, n, dim);
}

extern "C" int tt_dedup_sum(const int32_t* ids, int64_t n, int64_t num_rows, const float* grad,
                            int64_t grad_stride, int32_t dim, int32_t* unique_ids, float* summed,
                            int32_t* num_unique, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(ids && grad && unique_ids && summed && num_unique, "tt_dedup_sum: NULL pointer");
  TT_REQUIRE(n >= 1 && n < kMaxLookups, "tt_dedup_sum: n=%lld out of range", static_cast<long long>(n));
  tt_sparse_table t{};
  t.table = summed;  // not written by kWriteSum
  t.slot0 = summed;
  t.num_rows = num_rows;
  t.dim = dim;
  t.num_sources = 1;
  t.ids[0] = ids;
  t.grad_col_offset[0] = 0;
  int rc = validate_tables(&t, 1, n, false);
  if (rc) return rc;
  const size_t need = tables_ws_bytes(&t, 1, n, dim);
  if (!workspace || workspace_bytes < need)
    return fail(TT_ERR_WORKSPACE, "tt_dedup_sum: workspace %zu < required %zu", workspace_bytes, need);
  ApplyParams ap{};
  return run_sparse<kWriteSum>(&t, 1, n, grad, grad_stride, ap, workspace, workspace_bytes, to_stream(stream),
                               unique_ids, summed, num_unique);
}

extern "C" int tt_sparse_status(void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(workspace && workspace_bytes >= static_cast<size_t>(kHdrBytes), "tt_sparse_status: no workspace");
  hipStream_t st = to_stream(stream);
  SparseHeader h{};
  TT_CHECK_HIP(hipMemcpyAsync(&h, workspace, sizeof(h), hipMemcpyDeviceToHost, st));
  TT_CHECK_HIP(hipStreamSynchronize(st));
  if (h.magic != kHdrMagic || h.error == 0u) return TT_OK;
  const uint32_t zero = 0u;
  TT_CHECK_HIP(hipMemcpyAsync(static_cast<char*>(workspace) + offsetof(SparseHeader, error), &zero, sizeof(zero),
                              hipMemcpyHostToDevice, st));
  TT_CHECK_HIP(hipStreamSynchronize(st));
  return fail(TT_ERR_BAD_ARG, "sparse: %s%s(error word 0x%x); those blocks applied nothing",
              (h.error & kErrStaleKeys) ? "an apply found sorted keys of another call (stale presorted workspace) " : "",
              (h.error & kErrOutOfCall) ? "a sorted lookup pointed outside the call's gradient " : "", h.error);
}

extern "C" int tt_sparse_adagrad_rows(const tt_sparse_table* tables, int32_t num_tables, const int32_t* tags,
                                      const int32_t* rows, int64_t n, const float* grad, int64_t grad_ld, float lr,
                                      float epsilon, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(n >= 0, "tt_sparse_adagrad_rows: negative n");
  if (n == 0) return TT_OK;
  TT_REQUIRE(tables && tags && rows && grad, "tt_sparse_adagrad_rows: NULL pointer");
  TT_REQUIRE(num_tables >= 1 && num_tables <= kRowsMaxTables, "tt_sparse_adagrad_rows: 1..%d tables, got %d",
             kRowsMaxTables, num_tables);
  RowsArgs a{};
  a.num_tables = num_tables;
  a.dim = tables[0].dim;
  for (int t = 0; t < num_tables; ++t) {
    TT_REQUIRE(tables[t].table && tables[t].slot0, "tt_sparse_adagrad_rows: table %d NULL", t);
    TT_REQUIRE(tables[t].dim == a.dim, "tt_sparse_adagrad_rows: tables must share one dim");
    a.table[t] = tables[t].table;
    a.slot0[t] = tables[t].slot0;
    a.num_rows[t] = tables[t].num_rows;
  }
  TT_REQUIRE(a.dim >= 1 && grad_ld >= a.dim, "tt_sparse_adagrad_rows: bad dim %d / grad_ld", a.dim);
  a.tags = tags;
  a.rows = rows;
  a.n = n;
  a.grad = grad;
  a.grad_ld = grad_ld;
  a.lr = lr;
  a.eps = epsilon;
  bool v4 = a.dim % 4 == 0 && grad_ld % 4 == 0 && reinterpret_cast<uintptr_t>(grad) % 16 == 0;
  for (int t = 0; t < num_tables; ++t)
    v4 = v4 && reinterpret_cast<uintptr_t>(a.table[t]) % 16 == 0 && reinterpret_cast<uintptr_t>(a.slot0[t]) % 16 == 0;
  const int64_t threads = n * (v4 ? a.dim / 4 : a.dim);
  const dim3 grid(static_cast<unsigned>(ceil_div(threads, 256)));
  if (v4) hipLaunchKernelGGL(adagrad_rows_kernel<true>, grid, dim3(256), 0, to_stream(stream), a);
  else hipLaunchKernelGGL(adagrad_rows_kernel<false>, grid, dim3(256), 0, to_stream(stream), a);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_dense_adagrad(float* param, float* accum, const float* grad, int64_t n, float lr,
                                float epsilon, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(n >= 0, "tt_dense_adagrad: negative n");
  if (n == 0) return TT_OK;
  TT_REQUIRE(param && accum && grad, "tt_dense_adagrad: NULL pointer");
  hipLaunchKernelGGL(dense_adagrad_kernel, stride_grid(n), dim3(256), 0, to_stream(stream), param, accum, grad, n,
                     lr, epsilon);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_dense_adagrad_many(const tt_dense_job* jobs, int32_t num_jobs, float lr, float epsilon,
                                     tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(jobs && num_jobs >= 1 && num_jobs <= kDenseMaxJobs, "tt_dense_adagrad_many: 1..%d jobs, got %d",
             kDenseMaxJobs, num_jobs);
  DenseJobs d{};
  d.num = num_jobs;
  d.lr = lr;
  d.eps = epsilon;
  int64_t total = 0;
  for (int i = 0; i < num_jobs; ++i) {
    TT_REQUIRE(jobs[i].n >= 0, "tt_dense_adagrad_many: job %d negative n", i);
    TT_REQUIRE(jobs[i].n == 0 || (jobs[i].param && jobs[i].accum && jobs[i].grad),
               "tt_dense_adagrad_many: job %d NULL pointer", i);
    d.p[i] = jobs[i].param;
    d.acc[i] = jobs[i].accum;
    d.g[i] = jobs[i].grad;
    d.begin[i] = total;
    total += jobs[i].n;
  }
  d.begin[num_jobs] = total;
  if (total == 0) return TT_OK;
  hipLaunchKernelGGL(dense_adagrad_many_kernel, stride_grid(total), dim3(256), 0, to_stream(stream), d);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_dense_adam(float* param, float* m, float* v, const float* grad, int64_t n, float lr,
                             float beta1, float beta2, float epsilon, int64_t step, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(n >= 0 && step >= 1, "tt_dense_adam: bad n/step");
  if (n == 0) return TT_OK;
  TT_REQUIRE(param && m && v && grad, "tt_dense_adam: NULL pointer");
  // TF ApplyAdamOp: alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power).
  const float alpha = adam_coef(lr, beta1, beta2, step).alpha;
  hipLaunchKernelGGL(dense_adam_kernel, stride_grid(n), dim3(256), 0, to_stream(stream), param, m, v, grad, n,
                     alpha, 1.0f - beta1, 1.0f - beta2, epsilon);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int64_t tt_adam_coef_len(float beta1, float beta2) {
  if (!adam_beta_ok(beta1) || !adam_beta_ok(beta2)) return 0;
  for (int64_t t = 1; t <= kAdamCoefMaxLen; ++t)
    if (adam_coef(1.0f, beta1, beta2, t).saturated) return t;
  return 0;
}

extern "C" int tt_adam_coef_fill(float lr, float beta1, float beta2, int64_t len, float* alpha, float* lr_t) {
  clear_error();
  TT_REQUIRE(std::isfinite(lr), "tt_adam_coef_fill: learning rate is not finite");
  TT_REQUIRE(adam_beta_ok(beta1) && adam_beta_ok(beta2), "tt_adam_coef_fill: betas must lie in [0, 1), got %g / %g",
             static_cast<double>(beta1), static_cast<double>(beta2));
  TT_REQUIRE(len >= 1, "tt_adam_coef_fill: len must be >= 1");
  TT_REQUIRE(alpha && lr_t, "tt_adam_coef_fill: NULL pointer");
  for (int64_t t = 1; t <= len; ++t) {
    const AdamCoef c = adam_coef(lr, beta1, beta2, t);
    alpha[t - 1] = c.alpha;
    lr_t[t - 1] = c.lr_t;
  }
  return TT_OK;
}

extern "C" int tt_adam_clock_advance(tt_adam_clock* clock, const float* alpha_tab, const float* lr_t_tab,
                                     int64_t len, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(clock && alpha_tab && lr_t_tab, "tt_adam_clock_advance: NULL pointer");
  TT_REQUIRE(len >= 1, "tt_adam_clock_advance: len must be >= 1");
  hipLaunchKernelGGL(adam_clock_kernel, dim3(1), dim3(64), 0, to_stream(stream), clock, alpha_tab, lr_t_tab, len);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_dense_adam_many_dev(const tt_dense_adam_job* jobs, int32_t num_jobs, float beta1, float beta2,
                                      float epsilon, const tt_adam_clock* clock, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(jobs && num_jobs >= 1 && num_jobs <= kDenseMaxJobs, "tt_dense_adam_many_dev: 1..%d jobs, got %d",
             kDenseMaxJobs, num_jobs);
  TT_REQUIRE(clock, "tt_dense_adam_many_dev: NULL clock");
  DenseAdamJobs d{};
  d.num = num_jobs;
  d.omb1 = 1.0f - beta1;
  d.omb2 = 1.0f - beta2;
  d.eps = epsilon;
  d.clock = clock;
  int64_t total = 0;
  for (int i = 0; i < num_jobs; ++i) {
    TT_REQUIRE(jobs[i].n >= 0, "tt_dense_adam_many_dev: job %d negative n", i);
    TT_REQUIRE(jobs[i].n == 0 || (jobs[i].param && jobs[i].m && jobs[i].v && jobs[i].grad),
               "tt_dense_adam_many_dev: job %d NULL pointer", i);
    d.p[i] = jobs[i].param;
    d.m[i] = jobs[i].m;
    d.v[i] = jobs[i].v;
    d.g[i] = jobs[i].grad;
    d.begin[i] = total;
    total += jobs[i].n;
  }
  d.begin[num_jobs] = total;
  if (total == 0) return TT_OK;
  hipLaunchKernelGGL(dense_adam_many_dev_kernel, stride_grid(total), dim3(256), 0, to_stream(stream), d);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_sparse_adam_dev(const tt_sparse_table* tables, int32_t num_tables, int64_t batch,
                                  const float* grad, int64_t grad_stride, float beta1, float beta2, float epsilon,
                                  const tt_adam_clock* clock, void* workspace, size_t workspace_bytes,
                                  tt_stream_t stream) {
  clear_error();
  int rc = validate_tables(tables, num_tables, batch, true);
  if (rc) return rc;
  TT_REQUIRE(clock, "tt_sparse_adam_dev: NULL clock");
  const size_t need = tables_ws_bytes(tables, num_tables, batch, 0);
  if (batch > 0 && (!workspace || workspace_bytes < need))
    return fail(TT_ERR_WORKSPACE, "tt_sparse_adam_dev: workspace %zu < required %zu", workspace_bytes, need);
  hipStream_t st = to_stream(stream);
  // stage 1: every table's slots decayed, kAdamMaxTables tables a launch
  for (int first = 0; first < num_tables; first += kAdamMaxTables) {
    const AdamTables d = adam_tables(tables + first, std::min(num_tables - first, kAdamMaxTables));
    hipLaunchKernelGGL(adam_decay_many_kernel, adam_grid(d.begin[d.num]), dim3(256), 0, st, d, beta1, beta2);
    TT_CHECK_LAUNCH();
  }
  // stage 2: tt_sparse_adam's scatter, unchanged
  if (batch > 0) {
    ApplyParams ap{};
    ap.one_minus_beta1 = 1.0f - beta1;
    ap.one_minus_beta2 = 1.0f - beta2;
    rc = run_sparse<kAdamScatter>(tables, num_tables, batch, grad, grad_stride, ap, workspace, workspace_bytes, st);
    if (rc) return rc;
  }
  // stage 3: every table updated from its slots, lr_t read from the clock
  for (int first = 0; first < num_tables; first += kAdamMaxTables) {
    const AdamTables d = adam_tables(tables + first, std::min(num_tables - first, kAdamMaxTables));
    hipLaunchKernelGGL(adam_var_many_kernel, adam_grid(d.begin[d.num]), dim3(256), 0, st, d, clock, epsilon);
    TT_CHECK_LAUNCH();
  }
  return TT_OK;
}

extern "C" int tt_sparse_scatter_sum(const tt_sparse_table* tables, int32_t num_tables, int64_t batch,
                                     const float* grad, int64_t grad_stride, void* workspace,
                                     size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  int rc = validate_tables(tables, num_tables, batch, false, false);
  if (rc) return rc;
  if (batch == 0) return TT_OK;
  const size_t need = tables_ws_bytes(tables, num_tables, batch, 0);
  if (!workspace || workspace_bytes < need)
    return fail(TT_ERR_WORKSPACE, "tt_sparse_scatter_sum: workspace %zu < required %zu", workspace_bytes, need);
  ApplyParams ap{};
  return run_sparse<kScatterSum>(tables, num_tables, batch, grad, grad_stride, ap, workspace, workspace_bytes,
                                 to_stream(stream));
}

extern "C" int tt_sparse_routed(const tt_sparse_table* tables, int32_t num_tables, int64_t batch, const float* grad,
                                int64_t grad_stride, const tt_route_sorted* rs, int32_t op, float lr, float epsilon,
                                void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(rs && rs->order && rs->grp_first && rs->grp_last && rs->slot, "tt_sparse_routed: NULL route pointer");
  TT_REQUIRE(op == 0 || op == 1, "tt_sparse_routed: op must be 0 (scatter sum) or 1 (Adagrad), got %d", op);
  TT_REQUIRE(num_tables >= 1 && num_tables <= kTablesPerLaunch, "tt_sparse_routed: 1..%d tables, got %d",
             kTablesPerLaunch, num_tables);
  int rc = validate_tables(tables, num_tables, batch, false, op == 1);
  if (rc) return rc;
  if (batch == 0) return TT_OK;
  const int L = rs->num_lookups, W = rs->world, T = rs->num_tags;
  TT_REQUIRE(L >= 1 && L <= kRoutedMaxLookups, "tt_sparse_routed: 1..%d lookups, got %d", kRoutedMaxLookups, L);
  TT_REQUIRE(W >= 1 && W <= kRoutedThreads && T >= 1 && static_cast<int64_t>(W) * T <= kRoutedMaxGroups,
             "tt_sparse_routed: world %d x tags %d out of range", W, T);
  TT_REQUIRE(rs->cap >= 1, "tt_sparse_routed: cap must be >= 1");
  // every lookup belongs to one (table, source); each table takes one tag and
  // lists exactly its lookups as sources 0..num_sources-1
  int tag_of_table[kTablesPerLaunch], seen[kTablesPerLaunch][TT_MAX_SOURCES] = {};
  for (int t = 0; t < num_tables; ++t) tag_of_table[t] = -1;
  for (int l = 0; l < L; ++l) {
    const int t = rs->lookup_table[l], s = rs->lookup_source[l], g = rs->lookup_tag[l];
    TT_REQUIRE(t >= 0 && t < num_tables && s >= 0 && s < tables[t].num_sources && g >= 0 && g < T,
               "tt_sparse_routed: lookup %d maps to table %d source %d tag %d: out of range", l, t, s, g);
    TT_REQUIRE(tag_of_table[t] < 0 || tag_of_table[t] == g, "tt_sparse_routed: table %d takes two tags", t);
    TT_REQUIRE(!seen[t][s], "tt_sparse_routed: table %d source %d listed twice", t, s);
    tag_of_table[t] = g;
    seen[t][s] = 1;
  }
  for (int t = 0; t < num_tables; ++t)
    for (int s = 0; s < tables[t].num_sources; ++s)
      TT_REQUIRE(seen[t][s], "tt_sparse_routed: table %d source %d has no routed lookup", t, s);
  for (int t = 0; t < num_tables; ++t)
    for (int u = t + 1; u < num_tables; ++u)
      TT_REQUIRE(tag_of_table[t] != tag_of_table[u], "tt_sparse_routed: tables %d and %d take one tag", t, u);
  const size_t need = tables_ws_bytes(tables, num_tables, batch, 0);
  if (!workspace || workspace_bytes < need)
    return fail(TT_ERR_WORKSPACE, "tt_sparse_routed: workspace %zu < required %zu", workspace_bytes, need);
  TT_REQUIRE(batch < (int64_t(1) << kSrcShift), "tt_sparse_routed: batch too large");
  Plan p;
  rc = make_plan(tables, num_tables, batch, grad, grad_stride, &p);
  if (rc) return rc;
  Carver cv(workspace, workspace_bytes);
  PlanWs w = carve_plan(cv, p, 0);
  Job& j = p.job;
  j.keys = w.keys;
  j.vals = w.vals;
  j.arrived = w.arrived;
  j.hdr = w.hdr;
  RoutedArgs a{};
  a.order = rs->order;
  a.grp_first = rs->grp_first;
  a.grp_last = rs->grp_last;
  a.slot = rs->slot;
  a.slot_row = rs->slot_row;
  a.cap = rs->cap;
  a.total = static_cast<int64_t>(L) * batch;
  a.world = W;
  a.num_tags = T;
  a.num_lookups = L;
  a.num_tables = num_tables;
  for (int l = 0; l < L; ++l) {
    const int t = rs->lookup_table[l];
    a.lk_tag[l] = rs->lookup_tag[l];
    a.lk_khi[l] = static_cast<uint32_t>(t) << j.id_bits;
    a.lk_shi[l] = static_cast<uint32_t>(rs->lookup_source[l]) << kSrcShift;
    a.lk_base[l] = j.t[t].base;
  }
  int pads = 0;
  for (int t = 0; t < num_tables; ++t) {
    a.pad_begin[t] = pads;
    a.pad_dst[t] = j.t[t].base + j.t[t].n;
    a.pad_key[t] = (static_cast<uint32_t>(t) << j.id_bits) | ((1u << j.id_bits) - 1u);
    pads += j.t[t].n_pad - j.t[t].n;
  }
  a.pad_begin[num_tables] = pads;
  TT_REQUIRE(a.total + pads == p.total, "tt_sparse_routed: %lld routed lookups + %d padding != %d sorted entries",
             static_cast<long long>(a.total), pads, p.total);
  hipStream_t st = to_stream(stream);
  hipLaunchKernelGGL(routed_keys_kernel, dim3(static_cast<unsigned>(ceil_div(p.total, kRoutedThreads))),
                     dim3(kRoutedThreads), 0, st, j, a);
  TT_CHECK_LAUNCH();
  ApplyParams ap{};
  ap.lr = lr;
  ap.eps = epsilon;
  if (op == 1)
    return run_sparse<kAdagrad>(tables, num_tables, batch, grad, grad_stride, ap, workspace, workspace_bytes, st,
                                nullptr, nullptr, nullptr, kStageApply);
  return run_sparse<kScatterSum>(tables, num_tables, batch, grad, grad_stride, ap, workspace, workspace_bytes, st,
                                 nullptr, nullptr, nullptr, kStageApply);
}

extern "C" int tt_sparse_scatter_sum_sorted(const tt_sparse_table* tables, int32_t num_tables, int64_t batch,
                                            const float* grad, int64_t grad_stride, void* workspace,
                                            size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(num_tables <= kTablesPerLaunch, "tt_sparse_scatter_sum_sorted: at most %d tables", kTablesPerLaunch);
  int rc = validate_tables(tables, num_tables, batch, false, false);
  if (rc) return rc;
  if (batch == 0) return TT_OK;
  const size_t need = tables_ws_bytes(tables, num_tables, batch, 0);
  if (!workspace || workspace_bytes < need)
    return fail(TT_ERR_WORKSPACE, "tt_sparse_scatter_sum_sorted: workspace %zu < required %zu", workspace_bytes,
                need);
  ApplyParams ap{};
  return run_sparse<kScatterSum>(tables, num_tables, batch, grad, grad_stride, ap, workspace, workspace_bytes,
                                 to_stream(stream), nullptr, nullptr, nullptr, kStageApply);
}
