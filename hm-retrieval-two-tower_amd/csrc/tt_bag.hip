// Pooled embedding bags for sequence features (tt_gather_bag,
// tt_bag_grad_expand; contract in include/tt.h): the forward of "the last L
// ids of this example, looked up and pooled" and the expansion of its output
// gradient into one gradient row per lookup, which the existing sparse
// optimizer entries then apply as a flat [batch * L] problem.
//
// One sub-wave of TPB lanes (16 or 64) per bag, 256 / TPB bags per workgroup,
// no LDS, no atomics and no workgroup barrier.  Lane l owns the 4-float chunks
// l, l + TPB, ... of the row (NCH chunks per lane): a chunk is one 16-B access
// where the operand's base and leading dimension allow it and up to four
// scalar accesses where they do not, with the same element -> lane map.  Every
// output element is the sum of one column over the bag's valid slots in slot
// order, formed by the one lane that owns it, so no result bit depends on the
// launch form, on alignment, on the other bags or on the other jobs.
//
// Ids: lane l of the sub-wave reads slot k * TPB + l of id block k with one
// load and the sub-wave shares it by shuffle; block k + 1 is read before block
// k's rows are consumed.  A bag of L <= TPB slots has all its ids before its
// first row load.  Rows: the slots are walked in groups of kBagU = 4; the
// loads of group g + 1 are issued before the adds of group g, so four to
// eight row loads are in flight per lane.  Invalid slots issue no row load.
#include <cmath>

#include "tt_common.h"

namespace tt {
namespace {

constexpr int kBagThreads = 256;
constexpr int kBagU = 4;  // slots per group
constexpr int kBagMaxDim = 1024;
constexpr int kBagMaxL = 1024;
constexpr int64_t kBagMaxLookups = int64_t{1} << 24;  // tt_sparse's lookup bound

struct BagJob {
  const float* src;    // forward: the table; expansion: dOut + col_offset
  float* dst;          // forward: out + col_offset; expansion: G
  float* scale;        // [batch]: written by the forward, read by the expansion
  const int32_t* ids;
  int32_t* ids_flat;   // expansion only
  int64_t num_rows;
  int64_t ids_row_stride, ids_pos_stride;
  int64_t ld;          // leading dimension of out / dOut
  int32_t dim, L, pooling;
  int32_t vec;         // bit 0: src, bit 1: dst take 16-B accesses
  int32_t block_begin; // first workgroup of this job
};

struct BagArgs {
  BagJob job[TT_BAG_MAX_JOBS];
  int32_t num_jobs;
  int64_t batch;
};

// Elements [0, n) of the chunk at p (n >= 1; the rest read as 0).
__device__ __forceinline__ f32x4 bag_load(const float* p, int n, bool vec) {
  f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (n >= 4) {
    if (vec) {
      v = *reinterpret_cast<const f32x4*>(p);
    } else {
      v.x = p[0];
      v.y = p[1];
      v.z = p[2];
      v.w = p[3];
    }
  } else {
    v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
  }
  return v;
}

__device__ __forceinline__ void bag_store(float* p, int n, bool vec, f32x4 v) {
  if (n >= 4) {
    if (vec) {
      *reinterpret_cast<f32x4*>(p) = v;
    } else {
      p[0] = v.x;
      p[1] = v.y;
      p[2] = v.z;
      p[3] = v.w;
    }
  } else {
    p[0] = v.x;
    if (n > 1) p[1] = v.y;
    if (n > 2) p[2] = v.z;
  }
}

__device__ __forceinline__ int bag_job_of_block(const BagArgs& a) {
  int ji = 0;
#pragma unroll 1
  for (int i = 1; i < a.num_jobs; ++i)
    if (static_cast<int>(blockIdx.x) >= a.job[i].block_begin) ji = i;
  return ji;
}

// Slot k * TPB + lane of the bag at idp, or -1 past the bag's end.
template <int TPB>
__device__ __forceinline__ int bag_id_block(const int32_t* idp, int64_t pos_stride, int L, int k, int lane) {
  const int slot = k * TPB + lane;
  return slot < L ? idp[slot * pos_stride] : -1;
}

template <int TPB, int NCH>
__global__ void __launch_bounds__(kBagThreads) gather_bag_kernel(const BagArgs a) {
  const BagJob& J = a.job[bag_job_of_block(a)];
  constexpr int kBags = kBagThreads / TPB;
  const int lane = static_cast<int>(threadIdx.x) % TPB;
  const int64_t b = static_cast<int64_t>(static_cast<int>(blockIdx.x) - J.block_begin) * kBags +
                    static_cast<int>(threadIdx.x) / TPB;
  if (b >= a.batch) return;  // a whole sub-wave; shuffles stay inside a sub-wave
  const int dim = J.dim, L = J.L;
  const int64_t num_rows = J.num_rows;
  const bool vs = J.vec & 1, vd = J.vec & 2;
  const int32_t* idp = J.ids + b * J.ids_row_stride;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

  int idA = bag_id_block<TPB>(idp, J.ids_pos_stride, L, 0, lane);
  int idB = bag_id_block<TPB>(idp, J.ids_pos_stride, L, 1, lane);

  f32x4 acc[NCH], cur[kBagU][NCH], nxt[kBagU][NCH];
#pragma unroll
  for (int t = 0; t < NCH; ++t) acc[t] = zero;
  int cnt = 0;
  unsigned okc = 0, okn = 0;

  // the row loads of slots [s0, s0 + kBagU), whose ids are in `ids`
  auto issue = [&](f32x4(&buf)[kBagU][NCH], unsigned& ok, int s0, int ids) {
    ok = 0;
#pragma unroll
    for (int u = 0; u < kBagU; ++u) {
      const int id = __shfl(ids, (s0 + u) & (TPB - 1), TPB);
      const bool valid = s0 + u < L && id >= 0 && id < num_rows;
      ok |= valid ? 1u << u : 0u;
      const float* row = J.src + static_cast<int64_t>(id) * dim;
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        const int e = 4 * (lane + TPB * t);
        buf[u][t] = zero;
        if (valid && e < dim) buf[u][t] = bag_load(row + e, dim - e, vs);
      }
    }
  };

  const int groups = (L + kBagU - 1) / kBagU;
  issue(cur, okc, 0, idA);
#pragma unroll 1
  for (int g = 0; g < groups; ++g) {
    if (g + 1 < groups) {
      const int s0 = (g + 1) * kBagU;
      if ((s0 & (TPB - 1)) == 0) {  // the next group opens id block s0 / TPB
        idA = idB;
        idB = bag_id_block<TPB>(idp, J.ids_pos_stride, L, s0 / TPB + 1, lane);
      }
      issue(nxt, okn, s0, idA);
    }
#pragma unroll
    for (int u = 0; u < kBagU; ++u) {
      const bool valid = (okc >> u) & 1u;
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        const f32x4 sum = acc[t] + cur[u][t];
        acc[t] = valid ? (cnt == 0 ? cur[u][t] : sum) : acc[t];  // the first valid row starts the sum
      }
      cnt += valid ? 1 : 0;
    }
#pragma unroll
    for (int u = 0; u < kBagU; ++u) {
#pragma unroll
      for (int t = 0; t < NCH; ++t) cur[u][t] = nxt[u][t];
    }
    okc = okn;
  }

  float scale = 0.0f;
  if (cnt > 0) {
    const float n = static_cast<float>(cnt);
    scale = J.pooling == TT_BAG_SUM ? 1.0f : (J.pooling == TT_BAG_MEAN ? 1.0f / n : 1.0f / sqrtf(n));
  }
  float* out = J.dst + b * J.ld;
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int e = 4 * (lane + TPB * t);
    if (e >= dim) continue;
    f32x4 v = zero;  // an empty bag writes +0.0
    if (cnt > 0) v = J.pooling == TT_BAG_SUM ? acc[t] : acc[t] * scale;
    bag_store(out + e, dim - e, vd, v);
  }
  if (lane == 0) J.scale[b] = scale;
}

template <int TPB, int NCH>
__global__ void __launch_bounds__(kBagThreads) bag_expand_kernel(const BagArgs a) {
  const BagJob& J = a.job[bag_job_of_block(a)];
  constexpr int kBags = kBagThreads / TPB;
  const int lane = static_cast<int>(threadIdx.x) % TPB;
  const int64_t b = static_cast<int64_t>(static_cast<int>(blockIdx.x) - J.block_begin) * kBags +
                    static_cast<int>(threadIdx.x) / TPB;
  if (b >= a.batch) return;
  const int dim = J.dim, L = J.L;
  const int64_t num_rows = J.num_rows;
  const bool vs = J.vec & 1, vd = J.vec & 2;
  const int32_t* idp = J.ids + b * J.ids_row_stride;
  const float scale = J.scale[b];
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

  f32x4 g[NCH];
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int e = 4 * (lane + TPB * t);
    g[t] = zero;
    if (e < dim) {
      g[t] = bag_load(J.src + b * J.ld + e, dim - e, vs);
      if (J.pooling != TT_BAG_SUM) g[t] = g[t] * scale;
    }
  }
  const int64_t j0 = b * L;  // < 2^24 lookups per job (host check)
#pragma unroll 1
  for (int k = 0; k * TPB < L; ++k) {
    int id = bag_id_block<TPB>(idp, J.ids_pos_stride, L, k, lane);
    if (!(id >= 0 && id < num_rows)) id = -1;
    if (k * TPB + lane < L) J.ids_flat[j0 + k * TPB + lane] = id;
    const int n = L - k * TPB < TPB ? L - k * TPB : TPB;
#pragma unroll 1
    for (int s = 0; s < n; ++s) {
      if (__shfl(id, s, TPB) < 0) continue;  // rows of invalid slots are not written
      float* row = J.dst + (j0 + k * TPB + s) * dim;
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        const int e = 4 * (lane + TPB * t);
        if (e < dim) bag_store(row + e, dim - e, vd, g[t]);
      }
    }
  }
}

inline bool takes_vec(const void* p, int64_t ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0; }

// The launch form follows the widest job: 16 lanes per bag up to dim 64, a
// whole wave up to 256, four chunks per lane up to 1024.
template <template <int, int> class Launch>
int dispatch(BagArgs& a, int max_dim, hipStream_t st) {
  if (max_dim <= 64) return Launch<16, 1>::run(a, st);
  if (max_dim <= 256) return Launch<64, 1>::run(a, st);
  return Launch<64, 4>::run(a, st);
}

int place_blocks(BagArgs& a, int tpb) {
  const int64_t per_job = ceil_div(a.batch, kBagThreads / tpb);
  TT_REQUIRE(per_job * a.num_jobs < (int64_t{1} << 31), "tt_bag: grid too large");
  for (int i = 0; i < a.num_jobs; ++i) a.job[i].block_begin = static_cast<int32_t>(per_job * i);
  return TT_OK;
}

template <int TPB, int NCH>
struct LaunchForward {
  static int run(BagArgs& a, hipStream_t st) {
    if (int rc = place_blocks(a, TPB)) return rc;
    const int64_t blocks = ceil_div(a.batch, kBagThreads / TPB) * a.num_jobs;
    hipLaunchKernelGGL((gather_bag_kernel<TPB, NCH>), dim3(static_cast<unsigned>(blocks)), dim3(kBagThreads), 0, st,
                       a);
    TT_CHECK_LAUNCH();
    return TT_OK;
  }
};

template <int TPB, int NCH>
struct LaunchExpand {
  static int run(BagArgs& a, hipStream_t st) {
    if (int rc = place_blocks(a, TPB)) return rc;
    const int64_t blocks = ceil_div(a.batch, kBagThreads / TPB) * a.num_jobs;
    hipLaunchKernelGGL((bag_expand_kernel<TPB, NCH>), dim3(static_cast<unsigned>(blocks)), dim3(kBagThreads), 0, st,
                       a);
    TT_CHECK_LAUNCH();
    return TT_OK;
  }
};

}  // namespace
}  // namespace tt

using namespace tt;

// The checks both entries share; `J` is a tt_bag_job or a tt_bag_grad_job.
#define TT_BAG_COMMON(fn, J, i)                                                                                  \
  TT_REQUIRE((J).L >= 1 && (J).L <= kBagMaxL, fn ": job %d L=%d outside [1,%d]", i, (J).L, kBagMaxL);            \
  TT_REQUIRE((J).dim >= 1, fn ": job %d dim=%d below 1", i, (J).dim);                                            \
  if ((J).dim > kBagMaxDim)                                                                                      \
    return ::tt::fail(TT_ERR_UNSUPPORTED, fn ": job %d dim=%d above %d", i, (J).dim, kBagMaxDim);                \
  TT_REQUIRE(batch * (J).L < kBagMaxLookups, fn ": job %d batch*L=%lld reaches 2^24", i,                         \
             static_cast<long long>(batch * (J).L));                                                             \
  TT_REQUIRE((J).num_rows >= 1, fn ": job %d has an empty table", i);                                            \
  TT_REQUIRE((J).pooling >= TT_BAG_SUM && (J).pooling <= TT_BAG_SQRTN, fn ": job %d pooling=%d unknown", i,      \
             (J).pooling);                                                                                       \
  TT_REQUIRE((J).ids_row_stride >= 0 && (J).ids_pos_stride >= 0, fn ": job %d negative id stride", i)

extern "C" int tt_gather_bag(const tt_bag_job* jobs, int32_t num_jobs, int64_t batch, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(jobs != nullptr, "tt_gather_bag: NULL jobs");
  TT_REQUIRE(num_jobs >= 1 && num_jobs <= TT_BAG_MAX_JOBS, "tt_gather_bag: num_jobs=%d outside [1,%d]", num_jobs,
             TT_BAG_MAX_JOBS);
  TT_REQUIRE(batch >= 0 && batch < kBagMaxLookups, "tt_gather_bag: batch outside [0, 2^24)");
  BagArgs a{};
  a.num_jobs = num_jobs;
  a.batch = batch;
  int max_dim = 0;
  for (int i = 0; i < num_jobs; ++i) {
    const tt_bag_job& J = jobs[i];
    TT_BAG_COMMON("tt_gather_bag", J, i);
    TT_REQUIRE(J.table != nullptr, "tt_gather_bag: job %d table is NULL", i);
    TT_REQUIRE(J.col_offset >= 0 && static_cast<int64_t>(J.col_offset) + J.dim <= J.out_stride,
               "tt_gather_bag: job %d columns [%d,%d) exceed out_stride %lld", i, J.col_offset, J.col_offset + J.dim,
               static_cast<long long>(J.out_stride));
    TT_REQUIRE(batch == 0 || (J.ids && J.out && J.scale_out), "tt_gather_bag: job %d NULL pointer", i);
    BagJob& q = a.job[i];
    q.src = J.table;
    q.dst = J.out ? J.out + J.col_offset : nullptr;
    q.scale = J.scale_out;
    q.ids = J.ids;
    q.num_rows = J.num_rows;
    q.ids_row_stride = J.ids_row_stride, q.ids_pos_stride = J.ids_pos_stride;
    q.ld = J.out_stride;
    q.dim = J.dim, q.L = J.L, q.pooling = J.pooling;
    q.vec = (takes_vec(q.src, q.dim) ? 1 : 0) | (takes_vec(q.dst, q.ld) ? 2 : 0);
    max_dim = J.dim > max_dim ? J.dim : max_dim;
  }
  if (batch == 0) return TT_OK;
  return dispatch<LaunchForward>(a, max_dim, to_stream(stream));
}

extern "C" int tt_bag_grad_expand(const tt_bag_grad_job* jobs, int32_t num_jobs, int64_t batch, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(jobs != nullptr, "tt_bag_grad_expand: NULL jobs");
  TT_REQUIRE(num_jobs >= 1 && num_jobs <= TT_BAG_MAX_JOBS, "tt_bag_grad_expand: num_jobs=%d outside [1,%d]",
             num_jobs, TT_BAG_MAX_JOBS);
  TT_REQUIRE(batch >= 0 && batch < kBagMaxLookups, "tt_bag_grad_expand: batch outside [0, 2^24)");
  BagArgs a{};
  a.num_jobs = num_jobs;
  a.batch = batch;
  int max_dim = 0;
  for (int i = 0; i < num_jobs; ++i) {
    const tt_bag_grad_job& J = jobs[i];
    TT_BAG_COMMON("tt_bag_grad_expand", J, i);
    TT_REQUIRE(J.col_offset >= 0 && static_cast<int64_t>(J.col_offset) + J.dim <= J.dout_stride,
               "tt_bag_grad_expand: job %d columns [%d,%d) exceed dout_stride %lld", i, J.col_offset,
               J.col_offset + J.dim, static_cast<long long>(J.dout_stride));
    TT_REQUIRE(batch == 0 || (J.ids && J.dout && J.scale && J.ids_flat && J.grad),
               "tt_bag_grad_expand: job %d NULL pointer", i);
    BagJob& q = a.job[i];
    q.src = J.dout ? J.dout + J.col_offset : nullptr;
    q.dst = J.grad;
    q.scale = const_cast<float*>(J.scale);
    q.ids = J.ids;
    q.ids_flat = J.ids_flat;
    q.num_rows = J.num_rows;
    q.ids_row_stride = J.ids_row_stride, q.ids_pos_stride = J.ids_pos_stride;
    q.ld = J.dout_stride;
    q.dim = J.dim, q.L = J.L, q.pooling = J.pooling;
    q.vec = (takes_vec(q.src, q.ld) ? 1 : 0) | (takes_vec(q.dst, q.dim) ? 2 : 0);
    max_dim = J.dim > max_dim ? J.dim : max_dim;
  }
  if (batch == 0) return TT_OK;
  return dispatch<LaunchExpand>(a, max_dim, to_stream(stream));
}
