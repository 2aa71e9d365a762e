// Pieces of a workgroup-local, stable LSD radix sort in LDS, shared by the
// embedding update's id sorts (tt_sparse.hip) and the fused route
// (tt_route.hip).  A workgroup of WAVES waves sorts n positions by digits of
// at most 8 bits: each wave owns a contiguous slice of the current order, cut
// into 64-lane tiles; ranks inside a tile come from ballots of equal digits
// (digit_peers), ranks across tiles and waves from a [digit][wave] histogram
// scanned in (digit, wave) order — so equal digits keep their order: stable.
//
// A pass is: DigitHist::clear, LsdPass::load, LsdPass::count, DigitHist::scan,
// LsdPass::scatter.  The kernels string these together in their own loops; what
// differs between them (where the last pass stores, what happens between
// count and scan, when the histogram is cleared) stays in the kernels.
#pragma once
#include "tt_common.h"

namespace tt {

// lanes of this wave holding the same digit (among the `act` lanes): one
// ballot per digit bit (d < 2^nbits, nbits <= 8, wave-uniform), each lane
// keeping the lanes that agree with its bit
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool act, int nbits) {
  const uint64_t a = __ballot(act);
  uint32_t lo = static_cast<uint32_t>(a), hi = static_cast<uint32_t>(a >> 32);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    if (b >= nbits) break;
    const uint32_t bit = (d >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    const uint32_t flip = bit - 1u;  // 0 when the bit is set, all ones when clear
    lo &= static_cast<uint32_t>(bal) ^ flip;
    hi &= static_cast<uint32_t>(bal >> 32) ^ flip;
  }
  return act ? (static_cast<uint64_t>(hi) << 32 | lo) : 0;
}

// Digit counts [256 digits][WAVES] at a row stride of WAVES + 1 words, so the
// distinct digits of one wave's lanes fall in distinct LDS banks.
template <int WAVES>
struct DigitHist {
  static constexpr int kStride = WAVES + 1;
  static constexpr int kWords = 256 * kStride;
  static constexpr int kThreads = WAVES * kWave;
  // word of entry L = digit * WAVES + wave
  static __device__ __forceinline__ int word(int L) { return (L / WAVES) * kStride + L % WAVES; }

  static __device__ __forceinline__ void clear(uint32_t* hist) {
    for (int e = threadIdx.x; e < kWords; e += kThreads) hist[e] = 0u;
  }

  // one wave's count of a tile: the lowest lane of each digit adds its peers
  // (distinct digits, distinct words; the wave's own tiles run in order)
  static __device__ __forceinline__ void count(uint32_t* hist, uint32_t d, uint64_t m, int w) {
    if (m != 0 && __builtin_ctzll(m) == lane_id()) hist[d * kStride + w] += __builtin_popcountll(m);
  }

  // after scan: emit(slot) for a lane with digit d and peers m (m != 0) in
  // wave w's tile — the (digit, wave) offset plus the peers below the lane;
  // the lowest peer then moves the offset past the tile
  template <typename Emit>
  static __device__ __forceinline__ void place(uint32_t* hist, uint32_t d, uint64_t m, int w, Emit emit) {
    const int lane = lane_id();
    uint32_t* slot = &hist[d * kStride + w];
    const uint32_t off = *slot;
    emit(off + __builtin_popcountll(m & ((uint64_t(1) << lane) - 1u)));
    if (__builtin_ctzll(m) == lane) *slot = off + __builtin_popcountll(m);
  }

  // counts -> exclusive offsets in (digit, wave) order, 4 entries per thread;
  // wsum: WAVES words.  Barriers before, inside and after.
  static __device__ __forceinline__ void scan(uint32_t* hist, uint32_t* wsum) {
    const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
    __syncthreads();
    uint32_t h[4], run = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      h[u] = hist[word(4 * tid + u)];
      run += h[u];
    }
    uint32_t inc = run;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const uint32_t y = __shfl_up(inc, o, kWave);
      if (lane >= o) inc += y;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t ex = inc - run;
    for (int v = 0; v < w; ++v) ex += wsum[v];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      hist[word(4 * tid + u)] = ex;
      ex += h[u];
    }
    __syncthreads();
  }
};

// the slice [beg, end) of n positions that this thread's wave sorts: whole
// 64-lane tiles, the same number for every wave
template <int WAVES>
struct WaveSlice {
  int beg, end;
  __device__ __forceinline__ explicit WaveSlice(int n) {
    const int per = ((n + WAVES - 1) / WAVES + kWave - 1) / kWave * kWave;
    beg = static_cast<int>(threadIdx.x / kWave) * per;
    end = min(n, beg + per);
  }
};

// One LSD pass over a wave's slice of at most TILES tiles, in registers: the
// positions and digits of the lane's element of each tile, and the lanes of
// the tile with the same digit (found by the count, reused by the scatter).
template <int WAVES, int TILES>
struct LsdPass {
  using Hist = DigitHist<WAVES>;
  uint16_t pos[TILES];
  uint32_t dig[TILES];
  uint64_t peer[TILES];

  // pos = the current order, dig = digit (key >> sh) & dmask of key[pos]
  __device__ __forceinline__ void load(const WaveSlice<WAVES>& s, const uint16_t* order, const uint32_t* key, int sh,
                                       uint32_t dmask) {
#pragma unroll
    for (int q = 0; q < TILES; ++q) {
      const int i = s.beg + q * kWave + lane_id();
      pos[q] = 0;
      dig[q] = 0;
      if (i < s.end) {
        pos[q] = order[i];
        dig[q] = (key[pos[q]] >> sh) & dmask;
      }
    }
  }

  // peers of every tile, counted into hist[digit][this wave]
  __device__ __forceinline__ void count(const WaveSlice<WAVES>& s, uint32_t* hist, int width) {
    const int w = threadIdx.x / kWave;
#pragma unroll
    for (int q = 0; q < TILES; ++q) {
      peer[q] = 0;
      if (s.beg + q * kWave < s.end) {  // wave-uniform
        peer[q] = digit_peers(dig[q], s.beg + q * kWave + lane_id() < s.end, width);
        Hist::count(hist, dig[q], peer[q], w);
      }
    }
  }

  // after Hist::scan: emit(slot, pos) for every element, slot = its place in
  // the order by this digit
  template <typename Emit>
  __device__ __forceinline__ void scatter(const WaveSlice<WAVES>& s, uint32_t* hist, Emit emit) const {
    const int w = threadIdx.x / kWave;
#pragma unroll
    for (int q = 0; q < TILES; ++q) {
      if (s.beg + q * kWave < s.end) {  // wave-uniform
        const uint64_t m = peer[q];
        if (m != 0) Hist::place(hist, dig[q], m, w, [&](uint32_t o) { emit(o, pos[q]); });
      }
    }
  }
};

// workgroup-wide exclusive scan of one int per thread; *total = the sum.
// wsum: WAVES words, free again once every thread has returned and passed a
// barrier of its own or the next call's first.
template <int WAVES>
__device__ __forceinline__ int wg_exclusive_scan(int v, int* wsum, int* total) {
  const int lane = lane_id(), w = threadIdx.x / kWave;
  int x = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int y = __shfl_up(x, o, kWave);
    if (lane >= o) x += y;
  }
  __syncthreads();  // wsum free (an earlier scan's readers are done)
  if (lane == kWave - 1) wsum[w] = x;
  __syncthreads();
  int ex = x - v, t = 0;
  for (int q = 0; q < WAVES; ++q) {
    const int c = wsum[q];
    ex += q < w ? c : 0;
    t += c;
  }
  *total = t;
  return ex;
}

}  // namespace tt
