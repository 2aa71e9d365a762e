// Per-example sample weights of the in-batch loss (tt_inbatch_weight_rows;
// contract in include/tt.h): the one launch between the rows pass and the
// cols pass of a weighted step.  It folds each row's normalised weight w into
// the two per-row scalars the cols pass reads (lse, row_loss), forms the
// weighted loss term, and scales the rows pass's dq by w in place.
//
// One wave64 takes kWeightRows consecutive rows at a time, four waves per
// workgroup, rows grid-strided; no LDS, no atomics, no barrier.  Lane l <
// kWeightRows owns row l of the wave's block: it alone reads that row's w,
// lse and row_loss, calls libm for it and stores its three scalars, so the
// transcendental work is done once per row.  The dq rows are then scaled by
// all 64 lanes: a row is split into 4-float chunks, LPR lanes (a power of
// two, 4..64, the smallest covering the row's chunks) share a row, 64 / LPR
// rows go in one pass, and the row's w reaches its lanes by shuffle from the
// lane that owns the row.  Chunk c of a row is elements 4c .. 4c + 3 and
// belongs to lane (c mod LPR) of the row's group whatever the row's address:
// one 16-B access where dq's base and leading dimension allow it, up to four
// scalar accesses where not.  Every element is one load, one multiply, one
// store (or a plain store of +0 / NaN, or nothing at all for w == 1), so the
// two paths give the same bits.  Four passes' loads are issued before the
// first multiply.
#include <cmath>
#include <limits>

#include "tt_common.h"

namespace tt {
namespace {

constexpr int kWeightRows = 16;  // per wave and block of rows
constexpr int kWeightWaves = 4;  // per workgroup
constexpr int kWeightBatch = 4;  // passes whose loads are in flight together

struct WeightArgs {
  const float* w;
  const float* lse;
  const float* row_loss;
  int64_t n;
  float* lse_w;
  float* row_loss_w;
  float* wloss;  // may be NULL
  float* dq;     // may be NULL
  int64_t lddq;
  int32_t dim;
  int32_t lpr_log2;  // lanes per dq row: 1 << lpr_log2, 4..64
  int32_t vec;       // dq takes 16-B accesses
};

__device__ __forceinline__ f32x4 load4(const float* p, int n, bool vec) {
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

__device__ __forceinline__ void store4(float* p, int n, bool vec, f32x4 v) {
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

__global__ void __launch_bounds__(kWeightWaves * kWave) weight_rows_kernel(const WeightArgs a) {
  const int lane = lane_id();
  const int64_t wave = static_cast<int64_t>(blockIdx.x) * kWeightWaves + static_cast<int>(threadIdx.x) / kWave;
  const int64_t waves = static_cast<int64_t>(gridDim.x) * kWeightWaves;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float inf = std::numeric_limits<float>::infinity();
  const int lpr = 1 << a.lpr_log2;
  const int rows_per_pass = kWave >> a.lpr_log2;          // 1..16
  const int passes = kWeightRows / rows_per_pass;         // 1..16
  const int sub = lane >> a.lpr_log2;                     // this lane's row of a pass
  const int c0 = lane & (lpr - 1);                        // its first chunk of that row
  const int chunks = (a.dim >> 2) + ((a.dim & 3) != 0);
  const bool vec = a.vec != 0;

  for (int64_t row0 = wave * kWeightRows; row0 < a.n; row0 += waves * kWeightRows) {  // wave-uniform
    // the block's scalars: lane l owns row row0 + l
    float w = 1.0f;  // rows past the end read as "not touched"
    if (lane < kWeightRows && row0 + lane < a.n) {
      const int64_t i = row0 + lane;
      w = a.w[i];
      const float l = a.lse[i], r = a.row_loss[i];
      float lw, rw, wl;
      if (w == 1.0f) {
        lw = l, rw = r, wl = r;
      } else if (w == 0.0f) {
        lw = inf, rw = 0.0f, wl = 0.0f;
      } else if (w > 0.0f && w < 1.0f) {
        lw = l - logf(w);
        rw = -log1pf(w * expm1f(-r));
        wl = w * r;
      } else {  // < 0, > 1 or NaN: shown, not clamped
        lw = nan, rw = nan, wl = nan;
      }
      a.lse_w[i] = lw;
      a.row_loss_w[i] = rw;
      if (a.wloss) a.wloss[i] = wl;
    }
    if (a.dq == nullptr || chunks == 0) continue;

    for (int p0 = 0; p0 < passes; p0 += kWeightBatch) {
      // rows of this batch of passes, and their weights from the owning lanes
      float wr[kWeightBatch];
      int64_t row[kWeightBatch];
#pragma unroll
      for (int u = 0; u < kWeightBatch; ++u) {
        const int local = (p0 + u) * rows_per_pass + sub;  // >= kWeightRows past the last pass
        wr[u] = __shfl(w, local & (kWeightRows - 1), kWave);
        row[u] = row0 + local;
        if (p0 + u >= passes || row[u] >= a.n) wr[u] = 1.0f;  // nothing to do
      }
      for (int c = c0; c < chunks; c += lpr) {
        const int e = 4 * c;
        f32x4 v[kWeightBatch];
#pragma unroll
        for (int u = 0; u < kWeightBatch; ++u) {
          v[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
          if (wr[u] > 0.0f && wr[u] < 1.0f) v[u] = load4(a.dq + row[u] * a.lddq + e, a.dim - e, vec);
        }
#pragma unroll
        for (int u = 0; u < kWeightBatch; ++u) {
          if (wr[u] == 1.0f) continue;
          f32x4 o;
          if (wr[u] > 0.0f && wr[u] < 1.0f) {
            o = v[u] * wr[u];
          } else {
            const float f = wr[u] == 0.0f ? 0.0f : nan;
            o = f32x4{f, f, f, f};
          }
          store4(a.dq + row[u] * a.lddq + e, a.dim - e, vec, o);
        }
      }
    }
  }
}

}  // namespace
}  // namespace tt

using namespace tt;

extern "C" int tt_inbatch_weight_rows(const float* w, const float* lse, const float* row_loss, int64_t n,
                                      float* lse_w, float* row_loss_w, float* wloss, float* dq, int64_t lddq,
                                      int32_t dim, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(n >= 0, "tt_inbatch_weight_rows: n=%lld is negative", static_cast<long long>(n));
  TT_REQUIRE(dim >= 0, "tt_inbatch_weight_rows: dim=%d is negative", dim);
  TT_REQUIRE(lddq >= dim, "tt_inbatch_weight_rows: lddq=%lld below dim=%d", static_cast<long long>(lddq), dim);
  if (n == 0) return TT_OK;  // no work: the pointers are not looked at
  TT_REQUIRE(w && lse && row_loss, "tt_inbatch_weight_rows: NULL w, lse or row_loss");
  TT_REQUIRE(lse_w && row_loss_w, "tt_inbatch_weight_rows: NULL lse_w or row_loss_w");
  WeightArgs a{};
  a.w = w, a.lse = lse, a.row_loss = row_loss, a.n = n;
  a.lse_w = lse_w, a.row_loss_w = row_loss_w, a.wloss = wloss;
  a.dq = dim > 0 ? dq : nullptr, a.lddq = lddq, a.dim = dim;
  const int64_t chunks = ceil_div(dim, 4);
  a.lpr_log2 = 2;
  while (a.lpr_log2 < 6 && (int64_t{1} << a.lpr_log2) < chunks) ++a.lpr_log2;
  a.vec = a.dq && reinterpret_cast<uintptr_t>(dq) % 16 == 0 && lddq % 4 == 0;
  const int64_t blocks = ceil_div(n, int64_t{kWeightRows} * kWeightWaves);
  const int64_t grid = blocks < 8192 ? blocks : 8192;  // the rest by the grid stride
  hipLaunchKernelGGL(weight_rows_kernel, dim3(static_cast<unsigned>(grid)), dim3(kWeightWaves * kWave), 0,
                     to_stream(stream), a);
  TT_CHECK_LAUNCH();
  return TT_OK;
}
