// Row L2 normalisation of the towers' joint embeddings and its gradient
// (tt_l2norm_rows, tt_l2norm_rows_grad; contract in include/tt.h): the cosine
// scoring option's two launches per train step, each over both towers'
// operands.
//
// One wave64 per row at a time, four waves per workgroup, no LDS and no
// workgroup barrier; a wave takes R consecutive rows (4, 2 or 1) and issues
// all their loads before the first sum, so a narrow row's one 16-B load per
// lane is not the only one in flight.  Lane l owns the 4-float chunks l, l + 64, l + 128, ...
// of its row (elements 4c .. 4c + 3 of chunk c), whatever the row's address:
// a chunk is one 16-B load where the job's base and leading dimension allow
// it and up to four scalar loads where they do not, so the element -> lane
// map, the per-lane summation order (chunks ascending, elements ascending)
// and with them every result bit are the same on either path.  The 64 lane
// sums meet in an xor butterfly (32, 16, ..., 1): both lanes of a pair form
// the same a + b, so every lane ends with the same total.  The whole row is
// in registers before its first store (NCH chunks per lane: 1, 4 or 16 for
// dim <= 256, 1024, 4096), which is what makes the in-place gradient safe.
// The launch's NCH and R follow the widest job; a narrower job only skips the
// chunks it does not have, and R only says which wave holds a row, so a row's
// arithmetic depends on neither the other job nor the number of rows.
#include <cmath>

#include "tt_common.h"

namespace tt {
namespace {

constexpr int kNormMaxDim = 4096;
constexpr int kNormWaves = 4;  // per workgroup

struct NormJobs {
  const float* x[2];
  int64_t ldx[2];
  const float* dy[2];  // gradient only
  int64_t lddy[2];
  float* out[2];  // y (forward) or dx (gradient)
  int64_t ldo[2];
  float* inv[2];  // written by the forward, read by the gradient
  int64_t rows[2];
  int32_t dim[2];
  float scale[2];
  int32_t vec[2];     // bit 0: x, bit 1: out, bit 2: dy take 16-B accesses
  int64_t block1;     // first workgroup of job 1 (grid size when there is none)
};

// Elements [0, n) of the chunk at p (n >= 1; the rest read as 0).
__device__ __forceinline__ f32x4 load_chunk(const float* p, int n, bool vec) {
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

__device__ __forceinline__ void store_chunk(float* p, int n, bool vec, f32x4 v) {
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

template <int NCH, int R, bool GRAD>
__global__ void __launch_bounds__(256) l2norm_rows_kernel(const NormJobs a) {
  const int j = static_cast<int64_t>(blockIdx.x) >= a.block1 ? 1 : 0;
  const int64_t blk = static_cast<int64_t>(blockIdx.x) - (j ? a.block1 : 0);
  const int64_t row0 = (blk * kNormWaves + static_cast<int>(threadIdx.x) / kWave) * R;
  const int64_t rows = a.rows[j];
  if (row0 >= rows) return;  // a whole wave; no barrier follows
  const int lane = lane_id();
  const int dim = a.dim[j];
  const float scale = a.scale[j];
  const bool vx = a.vec[j] & 1, vo = a.vec[j] & 2, vd = a.vec[j] & 4;
  const int64_t ldx = a.ldx[j], ldo = a.ldo[j];
  const float* x = a.x[j] + row0 * ldx;
  float* out = a.out[j] + row0 * ldo;
  const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};

  // this wave's R rows: every load of all of them is issued before the first
  // sum (rows past the end, wave-uniform, stay zero and are not stored)
  f32x4 xv[R][NCH];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int t = 0; t < NCH; ++t) {
      const int e = 4 * (lane + kWave * t);
      xv[r][t] = zero;
      if (row0 + r < rows && e < dim) xv[r][t] = load_chunk(x + r * ldx + e, dim - e, vx);
    }
  }

  if constexpr (!GRAD) {
    float ss[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        acc += xv[r][t].x * xv[r][t].x;
        acc += xv[r][t].y * xv[r][t].y;
        acc += xv[r][t].z * xv[r][t].z;
        acc += xv[r][t].w * xv[r][t].w;
      }
      ss[r] = acc;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {  // R independent butterflies, step by step
#pragma unroll
      for (int r = 0; r < R; ++r) ss[r] += __shfl_xor(ss[r], m, kWave);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row0 + r >= rows) break;
      const float inv = ss[r] > 0.0f ? 1.0f / sqrtf(ss[r]) : 0.0f;
      const float s = scale * inv;
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        const int e = 4 * (lane + kWave * t);
        if (e < dim) store_chunk(out + r * ldo + e, dim - e, vo, inv > 0.0f ? xv[r][t] * s : zero);
      }
      if (lane == 0) a.inv[j][row0 + r] = inv;
    }
  } else {
    const int64_t lddy = a.lddy[j];
    const float* dy = a.dy[j] + row0 * lddy;
    f32x4 gv[R][NCH];
    float inv[R], dot[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      inv[r] = row0 + r < rows ? a.inv[j][row0 + r] : 0.0f;
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        const int e = 4 * (lane + kWave * t);
        gv[r][t] = zero;
        if (row0 + r < rows && e < dim) gv[r][t] = load_chunk(dy + r * lddy + e, dim - e, vd);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float acc = 0.0f;
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        xv[r][t] = xv[r][t] * inv[r];  // u
        acc += xv[r][t].x * gv[r][t].x;
        acc += xv[r][t].y * gv[r][t].y;
        acc += xv[r][t].z * gv[r][t].z;
        acc += xv[r][t].w * gv[r][t].w;
      }
      dot[r] = acc;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
      for (int r = 0; r < R; ++r) dot[r] += __shfl_xor(dot[r], m, kWave);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row0 + r >= rows) break;
      const float s = scale * inv[r];
#pragma unroll
      for (int t = 0; t < NCH; ++t) {
        const int e = 4 * (lane + kWave * t);
        if (e < dim)
          store_chunk(out + r * ldo + e, dim - e, vo, inv[r] > 0.0f ? (gv[r][t] - xv[r][t] * dot[r]) * s : zero);
      }
    }
  }
}

inline bool takes_vec(const void* p, int64_t ld) { return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 4 == 0; }

// The jobs that have rows, packed for one launch.  The widest job picks the
// kernel form (chunks per lane NCH, rows per wave R); job 1 of the launch
// starts at workgroup block1.
struct Packed {
  NormJobs a{};
  int n = 0;
  int max_dim = 0;
  void add(const float* x, int64_t ldx, const float* dy, int64_t lddy, float* out, int64_t ldo, float* inv,
           int64_t rows, int32_t dim, float scale) {
    a.x[n] = x, a.ldx[n] = ldx, a.dy[n] = dy, a.lddy[n] = lddy, a.out[n] = out, a.ldo[n] = ldo, a.inv[n] = inv;
    a.rows[n] = rows, a.dim[n] = dim, a.scale[n] = scale;
    a.vec[n] = (takes_vec(x, ldx) ? 1 : 0) | (takes_vec(out, ldo) ? 2 : 0) | (dy && takes_vec(dy, lddy) ? 4 : 0);
    max_dim = dim > max_dim ? dim : max_dim;
    ++n;
  }
  template <int NCH, int R, bool GRAD>
  int run(hipStream_t st) {
    a.block1 = ceil_div(a.rows[0], kNormWaves * R);
    const int64_t blocks = a.block1 + (n > 1 ? ceil_div(a.rows[1], kNormWaves * R) : 0);
    hipLaunchKernelGGL((l2norm_rows_kernel<NCH, R, GRAD>), dim3(blocks), dim3(kNormWaves * kWave), 0, st, a);
    TT_CHECK_LAUNCH();
    return TT_OK;
  }
  template <bool GRAD>
  int launch(hipStream_t st) {
    if (n == 0) return TT_OK;
    if (max_dim <= 256) return run<1, 4, GRAD>(st);
    if (max_dim <= 1024) return run<4, 2, GRAD>(st);
    return run<16, 1, GRAD>(st);
  }
};

}  // namespace
}  // namespace tt

using namespace tt;

#define TT_NORM_COMMON(fn, J, i)                                                                              \
  TT_REQUIRE((J).rows >= 0 && (J).rows <= (int64_t{1} << 31), fn ": job %d rows outside [0, 2^31]", i);       \
  TT_REQUIRE((J).dim >= 1 && (J).dim <= kNormMaxDim, fn ": job %d dim=%d outside [1,%d]", i, (J).dim,         \
             kNormMaxDim);                                                                                    \
  TT_REQUIRE(std::isfinite((J).scale), fn ": job %d scale is not finite", i)

extern "C" int tt_l2norm_rows(const tt_l2norm_job* jobs, int32_t num_jobs, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(jobs != nullptr, "tt_l2norm_rows: NULL jobs");
  TT_REQUIRE(num_jobs >= 1 && num_jobs <= 2, "tt_l2norm_rows: num_jobs=%d outside [1,2]", num_jobs);
  Packed p;
  for (int i = 0; i < num_jobs; ++i) {
    const tt_l2norm_job& J = jobs[i];
    TT_NORM_COMMON("tt_l2norm_rows", J, i);
    TT_REQUIRE(J.ldx >= J.dim && J.ldy >= J.dim, "tt_l2norm_rows: job %d leading dimension below dim=%d", i, J.dim);
    if (J.rows == 0) continue;
    TT_REQUIRE(J.x && J.y && J.inv, "tt_l2norm_rows: job %d NULL pointer", i);
    p.add(J.x, J.ldx, nullptr, 0, J.y, J.ldy, J.inv, J.rows, J.dim, J.scale);
  }
  return p.launch<false>(to_stream(stream));
}

extern "C" int tt_l2norm_rows_grad(const tt_l2norm_grad_job* jobs, int32_t num_jobs, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(jobs != nullptr, "tt_l2norm_rows_grad: NULL jobs");
  TT_REQUIRE(num_jobs >= 1 && num_jobs <= 2, "tt_l2norm_rows_grad: num_jobs=%d outside [1,2]", num_jobs);
  Packed p;
  for (int i = 0; i < num_jobs; ++i) {
    const tt_l2norm_grad_job& J = jobs[i];
    TT_NORM_COMMON("tt_l2norm_rows_grad", J, i);
    TT_REQUIRE(J.ldx >= J.dim && J.lddy >= J.dim && J.lddx >= J.dim,
               "tt_l2norm_rows_grad: job %d leading dimension below dim=%d", i, J.dim);
    if (J.rows == 0) continue;
    TT_REQUIRE(J.x && J.inv && J.dy && J.dx, "tt_l2norm_rows_grad: job %d NULL pointer", i);
    p.add(J.x, J.ldx, J.dy, J.lddy, J.dx, J.lddx, const_cast<float*>(J.inv), J.rows, J.dim, J.scale);
  }
  return p.launch<true>(to_stream(stream));
}
