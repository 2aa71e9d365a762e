// Input pipeline on the device: batches assembled from a
// dataset resident in HBM.
//
// Reference: /root/reference/pkg/modelling/tfrecord_dataset.py:59-98 reads
// TFRecord shards, shuffles with a buffer of shuffle_size and batches
// (drop_remainder=False); the StringLookup then runs per batch inside the
// model (input_layer.py:33-36).  Here the encoded columns (int32 rows /
// float32 values, one 32-bit word per example and column) live in HBM for the
// whole run — H&M's ~31M transactions x 12 columns are ~1.5 GB of the 288 GB
// — and a step's batch is one gather by the epoch's permutation:
//   dst[c, b] = src[c, perm[*cursor + b]],   then *cursor += batch.
// The position lives in device memory, so the take can sit inside the
// replayed train-step graph: an epoch is nothing but graph replays.
#include "tt_common.h"

namespace tt {
namespace {

constexpr int kTakeThreads = 256;

// One thread per example: its permutation entry is read once, then every
// column's word; the writes of a wave are 256 contiguous bytes per column.
__global__ void __launch_bounds__(kTakeThreads)
    batch_take_kernel(const uint32_t* __restrict__ src, int64_t src_ld, int32_t ncols,
                      const int64_t* __restrict__ perm, int64_t n_rows, const int64_t* __restrict__ cursor,
                      int64_t batch, uint32_t* __restrict__ dst, int64_t dst_ld, int32_t* __restrict__ status) {
  const int64_t b = blockIdx.x * static_cast<int64_t>(kTakeThreads) + threadIdx.x;
  if (b >= batch) return;
  const int64_t pos = *cursor + b;
  int64_t r = (pos >= 0 && pos < n_rows) ? perm[pos] : -1;
  if (r < 0 || r >= n_rows) {
    // past the dataset (or a corrupt permutation): zero words and a flag the
    // host reads back (tt_batch_status); never a silent wrap-around
    if (status) atomicOr(status, 1);
    for (int32_t c = 0; c < ncols; ++c) dst[c * dst_ld + b] = 0u;
    return;
  }
  for (int32_t c = 0; c < ncols; ++c) dst[c * dst_ld + b] = src[c * src_ld + r];
}

__global__ void cursor_advance_kernel(int64_t* cursor, int64_t step) { *cursor += step; }

// Mixed negative sampling (Yang et al. 2020): the candidate side of a step is
// the batch's B candidates followed by M rows of the catalogue drawn
// uniformly with replacement.  One thread per slot of dst: slot b < B copies
// the batch's words, slot B + m draws s_m from Philox4x32-10 — counter
// (m >> 2, step lo, step hi, 0), key (seed lo, seed hi), word m & 3 — as
// s_m = (u * N) >> 32 and copies catalogue row s_m.  Every workgroup reads
// the same *step; it is advanced by a one-thread launch behind this one (the
// cursor of batch_take_kernel), so a replayed graph draws fresh rows.
constexpr int kMaxMixedCols = 32;
struct MixedCols {
  const uint32_t* col[kMaxMixedCols];  // the batch's columns, [B] words each
};

__device__ __forceinline__ uint32_t philox_word(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                uint32_t k1, uint32_t which) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return which == 0 ? c0 : which == 1 ? c1 : which == 2 ? c2 : c3;
}

__global__ void __launch_bounds__(kTakeThreads)
    mixed_candidates_kernel(const MixedCols bc, const uint32_t* __restrict__ cat, int64_t cat_ld, int32_t ncols,
                            int64_t batch, int64_t m_extra, int64_t n_cat, uint32_t seed_lo, uint32_t seed_hi,
                            const int64_t* __restrict__ step, uint32_t* __restrict__ dst, int64_t dst_ld,
                            int32_t* __restrict__ status) {
  const int64_t x = blockIdx.x * static_cast<int64_t>(kTakeThreads) + threadIdx.x;
  if (x >= batch + m_extra) return;
  if (x < batch) {
    for (int32_t f = 0; f < ncols; ++f) dst[f * dst_ld + x] = bc.col[f][x];
    return;
  }
  if (n_cat < 1 || n_cat >= (1ll << 31)) {
    // no row to draw from (or one the 32-bit mapping cannot reach): zero
    // words and a flag, never an out-of-range read
    if (status) atomicOr(status, 1);
    for (int32_t f = 0; f < ncols; ++f) dst[f * dst_ld + x] = 0u;
    return;
  }
  const uint64_t m = static_cast<uint64_t>(x - batch);
  const uint64_t s = static_cast<uint64_t>(*step);
  const uint32_t u = philox_word(static_cast<uint32_t>(m >> 2), static_cast<uint32_t>(s),
                                 static_cast<uint32_t>(s >> 32), 0u, seed_lo, seed_hi, static_cast<uint32_t>(m & 3));
  const int64_t r = static_cast<int64_t>((static_cast<uint64_t>(u) * static_cast<uint64_t>(n_cat)) >> 32);  // < n_cat
  for (int32_t f = 0; f < ncols; ++f) dst[f * dst_ld + x] = cat[f * cat_ld + r];
}

}  // namespace
}  // namespace tt

using namespace tt;

extern "C" int tt_batch_take(const void* src, int64_t src_ld, int32_t ncols, const int64_t* perm, int64_t n_rows,
                             int64_t* cursor, int64_t batch, int32_t advance, void* dst, int64_t dst_ld,
                             int32_t* status, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(ncols >= 1, "tt_batch_take: ncols=%d < 1", ncols);
  TT_REQUIRE(batch >= 1 && n_rows >= 0, "tt_batch_take: bad batch / n_rows");
  TT_REQUIRE(src_ld >= n_rows && dst_ld >= batch, "tt_batch_take: leading dimensions too small");
  TT_REQUIRE(src && perm && cursor && dst, "tt_batch_take: NULL pointer");
  hipStream_t st = to_stream(stream);
  hipLaunchKernelGGL(batch_take_kernel, dim3(ceil_div(batch, kTakeThreads)), dim3(kTakeThreads), 0, st,
                     static_cast<const uint32_t*>(src), src_ld, ncols, perm, n_rows, cursor, batch,
                     static_cast<uint32_t*>(dst), dst_ld, status);
  TT_CHECK_LAUNCH();
  if (advance) {
    hipLaunchKernelGGL(cursor_advance_kernel, dim3(1), dim3(1), 0, st, cursor, batch);
    TT_CHECK_LAUNCH();
  }
  return TT_OK;
}

extern "C" int tt_mixed_candidates(const void* const* batch_cols, const void* cat, int64_t cat_ld, int32_t ncols,
                                   int64_t batch, int64_t m, int64_t n_cat, uint64_t seed, int64_t* step, void* dst,
                                   int64_t dst_ld, int32_t* status, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(ncols >= 1, "tt_mixed_candidates: ncols=%d < 1", ncols);
  if (ncols > kMaxMixedCols)
    return fail(TT_ERR_UNSUPPORTED, "tt_mixed_candidates: ncols=%d > %d", ncols, kMaxMixedCols);
  TT_REQUIRE(batch >= 1 && m >= 1, "tt_mixed_candidates: bad batch / m");
  TT_REQUIRE(batch < (1ll << 31) && m < (1ll << 31), "tt_mixed_candidates: batch / m too large");
  TT_REQUIRE(batch_cols && cat && step && dst, "tt_mixed_candidates: NULL pointer");
  TT_REQUIRE(dst_ld >= batch + m, "tt_mixed_candidates: dst_ld < batch + m");
  const bool bad_n = n_cat < 1 || n_cat >= (1ll << 31);
  // a catalogue size the mapping cannot serve: flagged on the device when the
  // caller gave a status word (the call may sit in a graph), refused otherwise
  TT_REQUIRE(!bad_n || status, "tt_mixed_candidates: n_cat=%lld outside [1, 2^31)", (long long)n_cat);
  TT_REQUIRE(bad_n || cat_ld >= n_cat, "tt_mixed_candidates: cat_ld < n_cat");
  MixedCols bc{};
  for (int32_t f = 0; f < ncols; ++f) {
    TT_REQUIRE(batch_cols[f], "tt_mixed_candidates: NULL batch column %d", f);
    bc.col[f] = static_cast<const uint32_t*>(batch_cols[f]);
  }
  hipStream_t st = to_stream(stream);
  hipLaunchKernelGGL(mixed_candidates_kernel, dim3(ceil_div(batch + m, kTakeThreads)), dim3(kTakeThreads), 0, st, bc,
                     static_cast<const uint32_t*>(cat), cat_ld, ncols, batch, m, n_cat,
                     static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), step,
                     static_cast<uint32_t*>(dst), dst_ld, status);
  TT_CHECK_LAUNCH();
  hipLaunchKernelGGL(cursor_advance_kernel, dim3(1), dim3(1), 0, st, step, int64_t{1});
  TT_CHECK_LAUNCH();
  return TT_OK;
}
