// Gradient clipping (tt_grad_sumsq, tt_grad_clip_apply; contract in
// include/tt.h): Keras' clipvalue / clipnorm / global_clipnorm over the
// gradient values the optimizer entries consume, in place, on the device.
//
// A region is a [rows, cols] range of fp32 with a leading dimension and,
// optionally, one id per row (rows with id < 0 are neither read nor written).
// It is walked as rows * ceil(cols / 4) chunks of 4 floats: chunk q is columns
// 4c .. 4c + 3 of row q / cpr (c = q % cpr).  A region owns nb = min(ceil(
// chunks / 1024), 256) workgroups (at least one); workgroup b of them takes
// the tiles b, b + nb, ... of 1024 chunks, thread t of it chunks t, t + 256,
// t + 512, t + 768 of a tile.  A chunk is one 16-B access where the region's
// base and leading dimension allow it and up to four scalar accesses where
// they do not, so the element -> thread map, every thread's order of
// additions and with them every result bit are the same on either path.
//
// Norm pass: a thread adds the fp64 squares (exact products of fp32 values) of
// its elements in ascending order, the workgroup's 256 sums meet in a fixed
// LDS tree and land in the workspace; a second launch (one workgroup per
// variable) adds a variable's partials in a fixed order.  No floating-point
// atomics: the sums are the same bits every run.  Apply pass: thread 0 of each
// workgroup derives the variable's factor from the sums (the global form adds
// the num_vars sums in index order), the workgroup clamps and scales in place.
// A factor of exactly 1 with no clamp leaves the region untouched (x * 1.0f
// is x).  Regions reach the kernels by value, kClipMaxRegions per launch.
#include <cmath>

#include "tt_common.h"

namespace tt {
namespace {

constexpr int kClipThreads = 256;
constexpr int kClipU = 4;                          // chunks per thread per tile
constexpr int kClipTile = kClipThreads * kClipU;   // chunks per workgroup per trip
constexpr int kClipRegionBlocks = 256;             // grid cap per region
constexpr int kClipMaxRegions = TT_CLIP_MAX_REGIONS;  // per launch
constexpr int64_t kClipMaxChunks = (int64_t{1} << 31) - 1;

struct ClipRegion {
  float* g;
  const int32_t* row_ids;
  int64_t ld;
  uint32_t chunks;       // rows * cpr
  uint32_t cpr;          // chunks per row
  int32_t cols;
  int32_t var;
  int32_t vec;           // 16-B accesses
  int32_t block_begin;   // first workgroup of this region
};

struct ClipArgs {
  ClipRegion r[kClipMaxRegions];
  int32_t num_regions;
  int32_t first;  // the call's first launch: the final reduction stores, later ones add
};

__device__ __forceinline__ f32x4 clip_load(const float* p, int n, bool vec) {
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

__device__ __forceinline__ void clip_store(float* p, int n, bool vec, f32x4 v) {
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

// min(max(g, -v), v) with comparisons: a NaN stays a NaN, -0.0 stays -0.0.
__device__ __forceinline__ float clamp1(float g, float v) { return g < -v ? -v : (g > v ? v : g); }
__device__ __forceinline__ f32x4 clamp4(f32x4 g, float v) {
  g.x = clamp1(g.x, v);
  g.y = clamp1(g.y, v);
  g.z = clamp1(g.z, v);
  g.w = clamp1(g.w, v);
  return g;
}

__device__ __forceinline__ int clip_region_of_block(const ClipArgs& a) {
  int ri = 0;
#pragma unroll 1
  for (int i = 1; i < a.num_regions; ++i)
    if (static_cast<int>(blockIdx.x) >= a.r[i].block_begin) ri = i;
  return ri;
}

// Where chunk q of the region lies, or nullptr when there is nothing to touch
// (past the end, or a skipped row); n: its element count (1..4).
__device__ __forceinline__ float* clip_chunk(const ClipRegion& R, uint64_t q, int& n) {
  n = 0;
  if (q >= R.chunks) return nullptr;
  const uint32_t row = static_cast<uint32_t>(q) / R.cpr;
  const uint32_t c = static_cast<uint32_t>(q) - row * R.cpr;
  if (R.row_ids && R.row_ids[row] < 0) return nullptr;
  const int rest = R.cols - 4 * static_cast<int>(c);
  n = rest < 4 ? rest : 4;
  return R.g + static_cast<int64_t>(row) * R.ld + 4 * static_cast<int64_t>(c);
}

__device__ __forceinline__ double block_sum_f64(double s, double* x) {
  const int t = static_cast<int>(threadIdx.x);
  x[t] = s;
  __syncthreads();
  for (int w = kClipThreads / 2; w > 0; w >>= 1) {
    if (t < w) x[t] += x[t + w];
    __syncthreads();
  }
  return x[0];
}

__global__ void __launch_bounds__(kClipThreads) clip_sumsq_kernel(const ClipArgs a, float clipvalue,
                                                                  double* __restrict__ partial) {
  __shared__ double x[kClipThreads];
  const int ri = clip_region_of_block(a);
  const ClipRegion& R = a.r[ri];
  const int t = static_cast<int>(threadIdx.x);
  const uint32_t end = ri + 1 < a.num_regions ? a.r[ri + 1].block_begin : gridDim.x;
  const uint32_t nb = end - R.block_begin;
  const uint32_t b = blockIdx.x - R.block_begin;
  const bool vec = R.vec != 0, clamp = clipvalue > 0.0f;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
  double s = 0.0;
#pragma unroll 1
  for (uint64_t base = static_cast<uint64_t>(b) * kClipTile; base < R.chunks;
       base += static_cast<uint64_t>(nb) * kClipTile) {
    f32x4 v[kClipU];
#pragma unroll
    for (int u = 0; u < kClipU; ++u) {  // every load of the tile before its first add
      int n;
      const float* p = clip_chunk(R, base + u * kClipThreads + t, n);
      v[u] = p ? clip_load(p, n, vec) : zero;  // elements that are not there add +0.0
    }
#pragma unroll
    for (int u = 0; u < kClipU; ++u) {
      const f32x4 g = clamp ? clamp4(v[u], clipvalue) : v[u];
      const double dx = g.x, dy = g.y, dz = g.z, dw = g.w;
      s += dx * dx;
      s += dy * dy;
      s += dz * dz;
      s += dw * dw;
    }
  }
  const double total = block_sum_f64(s, x);
  if (t == 0) partial[blockIdx.x] = total;
}

// Workgroup v: variable v's partials of this launch's regions, thread t adding
// partials t, t + 256, ... of each region in region order, then the LDS tree.
__global__ void __launch_bounds__(kClipThreads) clip_sumsq_final_kernel(const ClipArgs a, int32_t grid_blocks,
                                                                        const double* __restrict__ partial,
                                                                        double* __restrict__ sumsq) {
  __shared__ double x[kClipThreads];
  const int v = static_cast<int>(blockIdx.x);
  const int t = static_cast<int>(threadIdx.x);
  double s = 0.0;
#pragma unroll 1
  for (int i = 0; i < a.num_regions; ++i) {
    if (a.r[i].var != v) continue;
    const int begin = a.r[i].block_begin;
    const int end = i + 1 < a.num_regions ? a.r[i + 1].block_begin : grid_blocks;
    for (int k = begin + t; k < end; k += kClipThreads) s += partial[k];
  }
  const double total = block_sum_f64(s, x);
  if (t == 0) sumsq[v] = a.first ? total : sumsq[v] + total;
}

// c / max(n, c) with n = fp32(sqrt(ss)): exactly 1 for n <= c (and for ss = 0);
// a NaN norm gives a NaN factor.
__device__ __forceinline__ float clip_factor(double ss, float c) {
  const float n = static_cast<float>(sqrt(ss));
  const float d = !(n <= c) ? n : c;
  return c / d;
}

__global__ void __launch_bounds__(kClipThreads) clip_apply_kernel(const ClipArgs a, float clipvalue, float clipnorm,
                                                                  float global_clipnorm,
                                                                  const double* __restrict__ sumsq,
                                                                  int32_t num_vars, float* __restrict__ factor) {
  __shared__ float fs;
  const int ri = clip_region_of_block(a);
  const ClipRegion& R = a.r[ri];
  const int t = static_cast<int>(threadIdx.x);
  const uint32_t end = ri + 1 < a.num_regions ? a.r[ri + 1].block_begin : gridDim.x;
  const uint32_t nb = end - R.block_begin;
  const uint32_t b = blockIdx.x - R.block_begin;
  if (t == 0) {
    float f = 1.0f;
    if (clipnorm > 0.0f) {
      f = clip_factor(sumsq[R.var], clipnorm);
    } else if (global_clipnorm > 0.0f) {
      double ss = 0.0;
#pragma unroll 1
      for (int v = 0; v < num_vars; ++v) ss += sumsq[v];
      f = clip_factor(ss, global_clipnorm);
    }
    fs = f;
    if (b == 0 && factor) factor[R.var] = f;  // every region of a variable stores the same value
  }
  __syncthreads();
  const float f = fs;
  const bool vec = R.vec != 0, clamp = clipvalue > 0.0f;
  if (!clamp && f == 1.0f) return;  // x * 1.0f is x: nothing to read or write
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
  for (uint64_t base = static_cast<uint64_t>(b) * kClipTile; base < R.chunks;
       base += static_cast<uint64_t>(nb) * kClipTile) {
    f32x4 v[kClipU];
    float* p[kClipU];
    int n[kClipU];
#pragma unroll
    for (int u = 0; u < kClipU; ++u) {
      p[u] = clip_chunk(R, base + u * kClipThreads + t, n[u]);
      v[u] = p[u] ? clip_load(p[u], n[u], vec) : zero;
    }
#pragma unroll
    for (int u = 0; u < kClipU; ++u) {
      if (!p[u]) continue;
      f32x4 g = clamp ? clamp4(v[u], clipvalue) : v[u];
      if (f != 1.0f) g = g * f;  // (no norm set, or one that did not trigger: the clamp alone)
      clip_store(p[u], n[u], vec, g);
    }
  }
}

inline bool takes_vec(const void* p, int64_t ld, int64_t rows) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (rows <= 1 || ld % 4 == 0);
}

inline int64_t region_chunks(const tt_clip_region& r) { return r.rows * ceil_div(r.cols, 4); }
inline int64_t region_blocks(int64_t chunks) {
  const int64_t nb = ceil_div(chunks, kClipTile);
  return nb < 1 ? 1 : (nb > kClipRegionBlocks ? kClipRegionBlocks : nb);
}

int check_regions(const char* fn, const tt_clip_region* regions, int32_t num_regions, int32_t num_vars) {
  TT_REQUIRE(num_regions >= 0, "%s: num_regions=%d is negative", fn, num_regions);
  TT_REQUIRE(num_vars >= 1, "%s: num_vars=%d below 1", fn, num_vars);
  TT_REQUIRE(num_regions == 0 || regions != nullptr, "%s: NULL regions", fn);
  for (int i = 0; i < num_regions; ++i) {
    const tt_clip_region& r = regions[i];
    TT_REQUIRE(r.var >= 0 && r.var < num_vars, "%s: region %d var=%d outside [0,%d)", fn, i, r.var, num_vars);
    TT_REQUIRE(r.rows >= 0 && r.cols >= 0, "%s: region %d has a negative size", fn, i);
    TT_REQUIRE(r.rows <= 1 || r.ld >= r.cols, "%s: region %d ld=%lld below cols=%d", fn, i,
               static_cast<long long>(r.ld), r.cols);
    if (r.rows == 0 || r.cols == 0) continue;
    TT_REQUIRE(r.g != nullptr, "%s: region %d g is NULL", fn, i);
    if (r.rows > kClipMaxChunks / ceil_div(r.cols, 4))
      return ::tt::fail(TT_ERR_UNSUPPORTED, "%s: region %d has 2^31 or more 4-float chunks", fn, i);
  }
  return TT_OK;
}

// Regions [i0, i0 + n) packed for one launch; returns its grid.
int64_t pack(ClipArgs& a, const tt_clip_region* regions, int i0, int n, bool first) {
  a.num_regions = n;
  a.first = first ? 1 : 0;
  int64_t blocks = 0;
  for (int i = 0; i < n; ++i) {
    const tt_clip_region& r = regions[i0 + i];
    ClipRegion& q = a.r[i];
    const int64_t chunks = region_chunks(r);
    q.g = r.g;
    q.row_ids = r.row_ids;
    q.ld = r.ld;
    q.chunks = static_cast<uint32_t>(chunks);
    q.cpr = static_cast<uint32_t>(ceil_div(r.cols, 4));
    q.cols = r.cols;
    q.var = r.var;
    q.vec = chunks > 0 && takes_vec(r.g, r.ld, r.rows) ? 1 : 0;
    q.block_begin = static_cast<int32_t>(blocks);
    blocks += region_blocks(chunks);
  }
  return blocks;
}

}  // namespace
}  // namespace tt

using namespace tt;

extern "C" size_t tt_grad_clip_workspace_size(const tt_clip_region* regions, int32_t num_regions) {
  if (!regions || num_regions <= 0) return 256;
  int64_t blocks = 0;
  for (int i = 0; i < num_regions; ++i) {
    const tt_clip_region& r = regions[i];
    if (r.rows < 0 || r.cols < 0 || (r.cols > 0 && r.rows > kClipMaxChunks / ceil_div(r.cols, 4))) return 0;
    blocks += region_blocks(region_chunks(r));
  }
  return static_cast<size_t>(round_up(blocks * static_cast<int64_t>(sizeof(double)), 256));
}

extern "C" int tt_grad_sumsq(const tt_clip_region* regions, int32_t num_regions, int32_t num_vars, float clipvalue,
                             double* sumsq, void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  if (int rc = check_regions("tt_grad_sumsq", regions, num_regions, num_vars)) return rc;
  TT_REQUIRE(sumsq != nullptr, "tt_grad_sumsq: NULL sumsq");
  TT_REQUIRE(!std::isnan(clipvalue), "tt_grad_sumsq: clipvalue is NaN");
  const size_t need = tt_grad_clip_workspace_size(regions, num_regions);
  TT_REQUIRE(workspace != nullptr, "tt_grad_sumsq: NULL workspace");
  if (workspace_bytes < need)
    return ::tt::fail(TT_ERR_WORKSPACE, "tt_grad_sumsq: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t st = to_stream(stream);
  double* partial = static_cast<double*>(workspace);
  ClipArgs a{};
  int i0 = 0;
  do {  // no region at all: one launch of the final reduction stores the zeros
    const int n = num_regions - i0 < kClipMaxRegions ? num_regions - i0 : kClipMaxRegions;
    const int64_t blocks = pack(a, regions, i0, n, i0 == 0);
    if (blocks > 0) {
      hipLaunchKernelGGL(clip_sumsq_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kClipThreads), 0, st, a,
                         clipvalue, partial);
      TT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(clip_sumsq_final_kernel, dim3(static_cast<unsigned>(num_vars)), dim3(kClipThreads), 0, st, a,
                       static_cast<int32_t>(blocks), partial, sumsq);
    TT_CHECK_LAUNCH();
    partial += blocks;
    i0 += n;
  } while (i0 < num_regions);
  return TT_OK;
}

extern "C" int tt_grad_clip_apply(const tt_clip_region* regions, int32_t num_regions, int32_t num_vars,
                                  float clipvalue, float clipnorm, float global_clipnorm, const double* sumsq,
                                  float* factor, tt_stream_t stream) {
  clear_error();
  if (int rc = check_regions("tt_grad_clip_apply", regions, num_regions, num_vars)) return rc;
  TT_REQUIRE(!std::isnan(clipvalue) && !std::isnan(clipnorm) && !std::isnan(global_clipnorm),
             "tt_grad_clip_apply: a NaN setting");
  TT_REQUIRE(!(clipnorm > 0.0f && global_clipnorm > 0.0f),
             "tt_grad_clip_apply: clipnorm and global_clipnorm are both set");
  const bool norm = clipnorm > 0.0f || global_clipnorm > 0.0f;
  TT_REQUIRE(!norm || sumsq != nullptr, "tt_grad_clip_apply: a norm is set and sumsq is NULL");
  hipStream_t st = to_stream(stream);
  ClipArgs a{};
  for (int i0 = 0; i0 < num_regions; i0 += kClipMaxRegions) {
    const int n = num_regions - i0 < kClipMaxRegions ? num_regions - i0 : kClipMaxRegions;
    const int64_t blocks = pack(a, regions, i0, n, i0 == 0);
    hipLaunchKernelGGL(clip_apply_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kClipThreads), 0, st, a,
                       clipvalue, clipnorm, global_clipnorm, sumsq, num_vars, factor);
    TT_CHECK_LAUNCH();
  }
  return TT_OK;
}
