// K4 (tower MLP), row-streaming form: C = epi(maskA(A) . B) for a tall fp32
// activation A [M, K] and a small weight operand B [K, N] (N <= 4096; K any,
// M * lda < 2^30 for the 32-bit buffer offsets),
// the shape of every Dense-layer GEMM of the towers except the weight
// gradients (/root/reference/pkg/modelling/models/tower.py:41-49):
//   forward   h = relu(x W + b)                       B = W,   epi bias + relu
//   backward  g_in = (g_out * relu'(y) * s) W^T        B = W^T, maskA = relu'(y) * s,
//             (optionally * relu'(x) for the layer below: epi cmask)
//
// Precision: bf16x3 on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
// a = a_hi + a_lo, b = b_hi + b_lo (hi = bf16(x), lo = bf16(x - hi)),
// a_lo b_hi + a_hi b_lo + a_hi b_hi — every product to ~2^-17 relative,
// i.e. fp32-faithful (the model-level parity tests hold the fp32 tolerance).
//
// Layout (MI355X): B is tiny and read by every workgroup, so it is split
// ONCE per call into a bf16 hi/lo image already in MFMA B-fragment order
// (tt_mlp_pack): one wave's fragment for (k-step, 32-column block, plane) is
// 1 KiB contiguous, so each wave loads its fragments straight from L2 into
// VGPRs with fully coalesced 16-B-per-lane loads, 3 k-steps ahead.  A is
// streamed once: 64 rows per workgroup (256 workgroups fill the 256 CUs at
// M = 16384), 64-deep fp32 stages loaded row-contiguous by range-checked
// buffer loads two stages ahead (rows past M and depths past K read as 0),
// masked, split into hi/lo and written to a double-buffered XOR-swizzled LDS
// tile, read back as A fragments with conflict-free ds_read_b128.  The main
// loop is branch-free (the image is zero-padded to whole stages and to 4
// column blocks per wave row), so the compiler's vmcnt waits are exact; the
// two stages it asks for past the last are offset past the descriptor's range
// and cost no traffic (fetch_a).
// 4 waves; wave w computes rows 0..63 x the 32-column blocks w, w+4, w+8
// (each B fragment is loaded by exactly one wave of the workgroup); a block
// that lies wholly past N is skipped by its wave, and an unmasked width whose
// last 128-column unit has one real block (N = 258) runs in a slim width
// class with a 73 KiB tile and under 256 registers, two workgroups per CU
// (mlp_rows_block has both).
// Epilogue: the operands that do not depend on the accumulators are in flight
// before they are needed — the bias before the main loop, a thread's whole
// share of the epilogue mask (8 NCB 16-B loads) before the accumulators go
// through LDS — and the stores are 8 NCB unrolled trips of range-checked
// buffer stores: no per-trip division, branch or wait on the previous store.
// The LDS tile's pitch is the workgroup's own columns (n4 + 4), not the
// 128 NCB its blocks span.
//
// N > 384 (a workgroup keeps at most 3 blocks per wave = 384 columns in
// accumulators and a 97 KiB output tile): the launch covers (row blocks) x
// (column groups).  The image is padded to whole 128-column units (4 blocks,
// one per wave); G = ceil(units / 3) groups take base = units / G units each,
// the first units % G one more, and a workgroup runs the NCB = 1, 2 or 3
// instantiation of the same block code for ITS group's unit count, chosen at
// run time (a workgroup-uniform branch, as mlp_rows_pair_kernel chooses
// between its two problems).  Chosen over a uniform NCB with guarded blocks
// because a group then only ever addresses whole units below NBp: no image
// block past the padding can be loaded, the main loop stays branch-free, no
// MFMAs are spent on blocks that do not exist (772 columns = 7 units run as
// 3 + 2 + 2, not 3 x 3), and the even deal keeps N <= 512 at two 2-unit groups
// whose 66.5 KiB tile lets two workgroups share a CU.  A group offsets only
// the image block, the bias / cmask / C / parts column and the store width;
// the A stages, the k-steps, their order and the three MFMAs per step are the
// narrow kernel's, so an output element does not depend on the grouping (the
// result on a 128-aligned window equals the narrow kernel on that slice of
// B, bit for bit).  The groups of a row block re-read its A rows: while the
// image is smaller than an XCD's L2, block ids are laid out so they run back
// to back on one XCD; a larger image runs group by group (rows_order).
// N <= 384 launches exactly the ungrouped kernels.
#include <type_traits>

#include <cstdlib>
#include <cstring>

#include "tt_common.h"
#include "tt_mlp_pack.h"

namespace tt {
namespace {

constexpr int kMlpThreads = 256;
constexpr int kMlpBM = 64;       // rows per workgroup
constexpr int kMlpRB = kMlpBM / 32;  // 32-row MFMA blocks per wave
constexpr int kMlpUQ = kMlpBM / 16;  // A rows per thread per stage
constexpr int kMlpBK = 64;       // depth per A stage (4 MFMA k-steps)
constexpr int kMlpMaxCB = 3;     // 32-column blocks per wave: 384 columns per workgroup
constexpr int kMlpMaxN = 4096;   // widest B (tt_mlp_wgrad's bound); over 384 in column groups


struct MlpArgs {
  const float* A;
  int64_t lda;
  const float* amask;  // A := (amask > 0) ? A * s : 0   (HAS_MASK)
  int64_t ldam;
  const float* scale;  // device scalar s (NULL: 1)
  const __bf16* img;   // B image [KSp][NBp][2][64][8]
  int64_t M;
  int K, N, KSp, NBp;
  const float* bias;   // epilogue + bias[n] (NULL: none)
  int relu;
  const float* cmask;  // epilogue: C := (cmask > 0) ? C : 0 (NULL: none)
  int64_t ldcm;
  float* C;
  int64_t ldc;
  float* parts;        // optional [row blocks][N]: per-workgroup column sums of C
  int G;               // column groups (1: N <= 384, the whole width in one workgroup)
  int order;           // grouped launches: block id -> (row block, group), see mlp_rows_grouped
};

// Raw buffer resource over `bytes` bytes: loads past the end return 0.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mlp_desc(const void* base, uint64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0,
                                           static_cast<int>(bytes > 0x7fffffffull ? 0x7fffffffu : bytes),
                                           0x00020000);
}
// added to a byte offset: past the range of every mlp_desc descriptor
constexpr unsigned kMlpPastEnd = 0x80000000u;
constexpr int64_t kMlpMaxPitch = int64_t(1) << 22;  // widest C / cmask pitch of the epilogue's vector stores

__device__ __forceinline__ f32x4 mlp_load4(__amdgpu_buffer_rsrc_t d, unsigned voff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(d, voff, 0, 0));
}
// range-checked like the loads: a store past the descriptor's range is dropped
__device__ __forceinline__ void mlp_store4(__amdgpu_buffer_rsrc_t d, unsigned voff, f32x4 v) {
  using raw4 = decltype(__builtin_amdgcn_raw_buffer_load_b128(d, 0u, 0, 0));
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(raw4, v), d, voff, 0, 0);
}
// voff per lane (loop-invariant), soff uniform (e.g. the stage's row offset)
__device__ __forceinline__ f32x4 mlp_load4s(__amdgpu_buffer_rsrc_t d, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(d, voff, soff, 0));
}

using pack::bf16_bits;
using pack::bf16_val;
using pack::pack_fragment;
using pack::PackJob;
using pack::PackJobs;
using pack::kMaxPackJobs;
using pack::mlp_ks;
using pack::mlp_nb;

// LDS A tile: plane p, row r (0..63), 16-B chunk c (0..7) of the 64-deep stage
// at byte (p * 64 + r) * 128 + ((c ^ ((r >> 1) & 7)) << 4): the 16 lanes of
// one ds_read_b128 cycle (16 consecutive rows, one chunk) cover all 64 banks.
__device__ __forceinline__ int a_lds_off(int plane, int row, int chunk) {
  return ((plane * kMlpBM + row) << 7) + ((chunk ^ ((row >> 1) & 7)) << 4);
}

// A stages (2 x 2 planes x 64 rows x 128 B = 32 KiB), then the output tile
// [64][n4 + 4] fp32 of the epilogue, n4 = the workgroup's own columns rounded
// up to 4 (not the NCB * 128 its waves' blocks span).  Two compile-time width
// classes size it: the full one holds any n4 <= COLS = 128 NCB (<= 97 KiB);
// SLIM holds the widths whose last 128-column unit has real columns in its
// first 32-column block only, n4 <= COLS = 128 (NCB - 1) + 32 (NCB = 3:
// 64 x 292 x 4 = 73 KiB, two workgroups per CU; N = 258 is such a width).
// TRIPS: 16-B store trips per thread that cover 64 rows x COLS columns.
template <int NCB, bool SLIM = false>
struct MlpSmem {
  static constexpr int COLS = SLIM ? (NCB - 1) * 128 + 32 : NCB * 128;
  static constexpr int TRIPS = kMlpBM * (COLS / 4) / kMlpThreads;
  static constexpr int BYTES =
      kMlpBM * (COLS + 4) * 4 > 2 * 2 * kMlpBM * 128 ? kMlpBM * (COLS + 4) * 4 : 2 * 2 * kMlpBM * 128;
};
// the widths of an NCB-block problem that fit the SLIM class
constexpr bool mlp_slim_fits(int ncb, int n) { return (n + 3) / 4 * 4 <= (ncb - 1) * 128 + 32; }
// The problems that run in it: NCB = 3, the one width class whose tile and not
// its registers sets the workgroups per CU (97 KiB: one; 73 KiB: two), without
// an A mask: the masked form's mask stages take it past 256 registers (282),
// so it would still run one workgroup per CU and stays in the full class.
constexpr bool mlp_slim_class(int ncb, bool has_mask, int n) { return ncb == 3 && !has_mask && mlp_slim_fits(3, n); }

// One workgroup's rows [bid * kMlpBM, +kMlpBM) of one problem; smem_raw holds
// MlpSmem<NCB, SLIM>::BYTES (SLIM: the caller checked mlp_slim_fits).
// A column block that lies wholly at or past N (a ragged last unit: blocks
// 9..11 of N = 258 belong to waves 1..3) is skipped by its wave: only a
// wave's LAST block can be such a block (a narrower problem runs a smaller
// NCB, a group owns whole units below NBp), so the wave picks, once and
// wave-uniformly, the main loop compiled for NCB or for NCB - 1 live blocks.
// Either loop is branch-free as before, and a live block's k-steps, their
// order and its three MFMAs per step are the same in both: the skip changes
// no output bit.  A skipped block loads no B fragment, issues no MFMA and
// writes no tile column (the stores never read one: its columns are >= n4).
// SLIM (ungrouped): the last unit is one real block, 4 (NCB - 1), and a
// whole-block deal would give all of it to wave 0 (6 MFMA tiles of 32 x 32
// against 4 on the other waves, and 96 accumulator registers for every wave
// of the kernel).  Its two row halves go to waves 0 and 1 instead: wave w < 2
// owns the tile (rows 32 w .., block 4 (NCB - 1)) as the one tile of its last
// block, waves 2 and 3 skip the block.  5 + 5 + 4 + 4 tiles, 80 accumulator
// registers; B fragments are prefetched 2 k-steps ahead instead of 3 (a
// quarter fewer in flight), which brings the class under 256 registers: two
// waves per SIMD to go with its two tiles per CU.  Which wave runs a tile's
// MFMA chain does not change the chain.
// GROUPED: the workgroup owns the 4 NCB image blocks
// from cb0 (a multiple of 4, cb0 + 4 NCB <= NBp), i.e. columns [32 cb0,
// min(N, 32 cb0 + 128 NCB)) of B, bias, cmask, C and parts; everything else
// (the A stages, the k-steps and their order, the three MFMAs per step) is the
// ungrouped code, so an output element does not depend on the grouping.
template <int NCB, bool HAS_MASK, bool GROUPED = false, bool SLIM = false>
__device__ __forceinline__ void mlp_rows_block(const MlpArgs& a, const int64_t bid, char* smem_raw,
                                               const int cb0 = 0) {
  char (*smem)[2 * kMlpBM * 128] = reinterpret_cast<char (*)[2 * kMlpBM * 128]>(smem_raw);
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = lane_id();
  const int l32 = lane & 31, h = lane >> 5;
  const int64_t m0 = bid * kMlpBM;
  const float s = a.scale ? *a.scale : 1.0f;

  // ---- A stages: thread -> rows qrow + 16 u (u < 4), depths qk .. qk + 3 ------
  // (16 threads per row: 256 contiguous bytes per row per stage)
  const int qrow = tid >> 4, qk = (tid & 15) * 4;
  const __amdgpu_buffer_rsrc_t da = mlp_desc(a.A + m0 * a.lda, static_cast<uint64_t>(a.M - m0) * a.lda * 4);
  const __amdgpu_buffer_rsrc_t dm = mlp_desc(HAS_MASK ? a.amask + m0 * a.ldam : a.A, static_cast<uint64_t>(a.M - m0) * a.ldam * 4);
  f32x4 ra[2][kMlpUQ], rm[2][kMlpUQ];
  const int nstage = (a.K + kMlpBK - 1) / kMlpBK;  // KSp = 4 nstage
  // The loop prefetches two stages ahead without a branch, so it asks for two
  // stages past the last.  The descriptors span the rest of the matrix (those
  // depths are the next rows' data), so a stage at or past nstage gets
  // kMlpPastEnd added to its offsets (a wave-uniform select): past every
  // descriptor's range (mlp_desc caps it at 2^31 - 1), the loads return zeros
  // without memory traffic.
  auto fetch_a = [&](int k0, auto slot_c) {
    constexpr int SL = decltype(slot_c)::value;
    const unsigned ko = static_cast<unsigned>(k0) * 4 + (k0 < nstage * kMlpBK ? 0u : kMlpPastEnd);
#pragma unroll
    for (int u = 0; u < kMlpUQ; ++u) {
      const int row = qrow + 16 * u;
      ra[SL][u] = mlp_load4(da, static_cast<unsigned>((row * a.lda + qk) * 4) + ko);
      if constexpr (HAS_MASK) rm[SL][u] = mlp_load4(dm, static_cast<unsigned>((row * a.ldam + qk) * 4) + ko);
    }
  };
  auto stash_a = [&](int k0, auto slot_c, int buf) {
    constexpr int SL = decltype(slot_c)::value;
    char* base = smem[buf];
#pragma unroll
    for (int u = 0; u < kMlpUQ; ++u) {
      const int row = qrow + 16 * u;
      unsigned hb[4], lb[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = (k0 + qk + e < a.K) ? ra[SL][u][e] : 0.0f;  // depths past K (or a ragged row's tail)
        if constexpr (HAS_MASK) v = (rm[SL][u][e] > 0.0f) ? v * s : 0.0f;
        hb[e] = bf16_bits(v);
        lb[e] = bf16_bits(v - bf16_val(hb[e]));
      }
      const int chunk = qk >> 3, half = (qk >> 2) & 1;
      *reinterpret_cast<uint2*>(base + a_lds_off(0, row, chunk) + 8 * half) =
          make_uint2(hb[0] | (hb[1] << 16), hb[2] | (hb[3] << 16));
      *reinterpret_cast<uint2*>(base + a_lds_off(1, row, chunk) + 8 * half) =
          make_uint2(lb[0] | (lb[1] << 16), lb[2] | (lb[3] << 16));
    }
  };

  // ---- B fragments: k-step ks, block i (column block wave + 4 i), plane p ----
  const bf16x8* img = reinterpret_cast<const bf16x8*>(a.img) + lane + (GROUPED ? cb0 * 2 * 64 : 0);
  const int64_t kstride = static_cast<int64_t>(a.NBp) * 2 * 64;  // bf16x8 per k-step

  static_assert(!(SLIM && GROUPED), "the slim class is an ungrouped one");
  // block i of this wave; SLIM: its last is the unit's one real block, of
  // which the wave owns row half `wave` (acc[0][NCB - 1]; acc[1][NCB - 1] unused)
  auto blk = [&](int i) { return SLIM && i == NCB - 1 ? 4 * (NCB - 1) : wave + 4 * i; };
  constexpr int PF = SLIM ? 2 : 3;  // k-steps a B fragment is loaded ahead of its use
  f32x16 acc[kMlpRB][NCB];
#pragma unroll
  for (int rb = 0; rb < kMlpRB; ++rb)
#pragma unroll
    for (int i = 0; i < NCB; ++i) acc[rb][i] = f32x16{};

  const int ks_end = (a.K + 15) / 16;  // k-steps holding data
  // the epilogue's bias, issued here so its round trip passes under the main loop
  const int c0 = GROUPED ? cb0 * 32 : 0;  // first column of the group: tile column c is column c0 + c
  float bias[NCB];
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int col = c0 + blk(i) * 32 + l32;
    bias[i] = (a.bias && col < a.N) ? a.bias[col] : 0.0f;
  }
  // The main loop for a wave with LIVE live blocks (its first LIVE of NCB).
  // Every wave of the workgroup passes the same barriers in either form: the
  // A stages and their hand-offs do not depend on LIVE.
  auto main_loop = [&](auto live_c) {
    constexpr int LIVE = decltype(live_c)::value;
    bf16x8 bq[4][LIVE > 0 ? LIVE : 1][2];  // k-step ks in slot ks % 4 (static under the 2-stage unroll)
    auto load_b = [&](int ks, auto slot_c) {
      constexpr int SL = decltype(slot_c)::value;
      const int kc = ks < a.KSp ? ks : a.KSp - 1;  // past the end: a harmless re-read
#pragma unroll
      for (int i = 0; i < LIVE; ++i) {
        const bf16x8* p = img + kc * kstride + (blk(i) * 2) * 64;
        bq[SL][i][0] = p[0];
        bq[SL][i][1] = p[64];
      }
    };
    load_b(0, std::integral_constant<int, 0>());
    load_b(1, std::integral_constant<int, 1>());
    if constexpr (PF == 3) load_b(2, std::integral_constant<int, 2>());
    fetch_a(0, std::integral_constant<int, 0>());
    fetch_a(kMlpBK, std::integral_constant<int, 1>());
    stash_a(0, std::integral_constant<int, 0>(), 0);
    __syncthreads();
    // stage st (parity PAR): A of stage st + 1 sits in ra[1 - PAR], stage st + 2
    // is fetched into ra[PAR]; k-steps 4 st .. 4 st + 3 use B slots 0..3 and
    // prefetch k-steps 4 st + PF .. 4 st + PF + 3.
    auto stage = [&](int st, auto par_c) {
      constexpr int PAR = decltype(par_c)::value;
      fetch_a((st + 2) * kMlpBK, std::integral_constant<int, PAR>());
      const char* base = smem[PAR];
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const int ks = 4 * st + kk;
        if (kk == 0) load_b(ks + PF, std::integral_constant<int, PF & 3>());
        if (kk == 1) load_b(ks + PF, std::integral_constant<int, (PF + 1) & 3>());
        if (kk == 2) load_b(ks + PF, std::integral_constant<int, (PF + 2) & 3>());
        if (kk == 3) load_b(ks + PF, std::integral_constant<int, (PF + 3) & 3>());
        if (ks >= ks_end) continue;  // the zero padding of the last stage (uniform)
        bf16x8 ah[kMlpRB], al[kMlpRB];
#pragma unroll
        for (int rb = 0; rb < kMlpRB; ++rb) {
          const int row = 32 * rb + l32, chunk = 2 * kk + h;
          ah[rb] = *reinterpret_cast<const bf16x8*>(base + a_lds_off(0, row, chunk));
          al[rb] = *reinterpret_cast<const bf16x8*>(base + a_lds_off(1, row, chunk));
        }
#pragma unroll
        for (int i = 0; i < LIVE; ++i) {
          if constexpr (SLIM && LIVE == NCB) {
            if (i == NCB - 1) {  // the one tile of the last block: row half `wave` (read again: no register select)
              const int row = 32 * wave + l32, chunk = 2 * kk + h;
              const bf16x8 ahw = *reinterpret_cast<const bf16x8*>(base + a_lds_off(0, row, chunk));
              const bf16x8 alw = *reinterpret_cast<const bf16x8*>(base + a_lds_off(1, row, chunk));
              acc[0][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(alw, bq[kk][i][0], acc[0][i], 0, 0, 0);
              acc[0][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahw, bq[kk][i][1], acc[0][i], 0, 0, 0);
              acc[0][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ahw, bq[kk][i][0], acc[0][i], 0, 0, 0);
              continue;
            }
          }
#pragma unroll
          for (int rb = 0; rb < kMlpRB; ++rb) {
            acc[rb][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rb], bq[kk][i][0], acc[rb][i], 0, 0, 0);
            acc[rb][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rb], bq[kk][i][1], acc[rb][i], 0, 0, 0);
            acc[rb][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rb], bq[kk][i][0], acc[rb][i], 0, 0, 0);
          }
        }
      }
      if (st + 1 < nstage) {
        stash_a((st + 1) * kMlpBK, std::integral_constant<int, 1 - PAR>(), 1 - PAR);
        lds_barrier();  // LDS hand-off only: the A / B prefetches stay in flight
      }
    };
    for (int st = 0; st < nstage; st += 2) {
      stage(st, std::integral_constant<int, 0>());
      if (st + 1 < nstage) stage(st + 1, std::integral_constant<int, 1>());
    }
  };
  // the wave's last block starts at or past N: not a column of it is real
  // (wave-uniform); SLIM: the last block has a tile for waves 0 and 1 only
  const bool last_dead = SLIM ? wave >= kMlpRB : c0 + (wave + 4 * (NCB - 1)) * 32 >= a.N;
  if (last_dead) main_loop(std::integral_constant<int, NCB - 1>());
  else main_loop(std::integral_constant<int, NCB>());

  // ---- epilogue: lane (l32, h), register r -> row (r & 3) + 8 (r >> 2) + 4 h, column l32
  // acc (+ bias, relu) -> LDS tile [64][OUT_LD] (column = 32 cb + l32 of this
  // wave's blocks, in block order cb = wave + 4 i), then row-contiguous vector
  // stores of C with the epilogue mask read the same way (coalesced).
  const int64_t rows = a.M - m0 < kMlpBM ? a.M - m0 : kMlpBM;
  float* C = a.C + m0 * a.ldc + c0;
  const float* cm = a.cmask ? a.cmask + m0 * a.ldcm + c0 : nullptr;
  // this workgroup's columns: all N, or the group's (c0 is a multiple of 128,
  // so the group's rows are 16-B aligned exactly when the problem's are)
  const int N = GROUPED ? (a.N - c0 < NCB * 128 ? a.N - c0 : NCB * 128) : a.N;
  // 16-B stores of whole rows; a ragged N writes its row's padding columns
  // (zeros: the image is zero there) when the row pitch has room for them
  // (pitches below kMlpMaxPitch: 64 rows' byte offsets stay below 2^31)
  const int n4 = (N + 3) / 4 * 4;
  const int OUT_LD = n4 + 4;  // tile pitch: the workgroup's own columns (n4 <= MlpSmem<NCB, SLIM>::COLS)
  const bool v4 = (a.ldc % 4 == 0) && (a.ldc >= c0 + n4) && (a.ldc < kMlpMaxPitch) &&
                  (reinterpret_cast<uintptr_t>(a.C) % 16 == 0) &&
                  (!cm || ((N % 4 == 0) && (a.ldcm % 4 == 0) && (a.ldcm < kMlpMaxPitch) &&
                           (reinterpret_cast<uintptr_t>(a.cmask) % 16 == 0)));
  // Vector trips: a thread's trip t is 16-B element tid + 256 t of the
  // [rows][n4 / 4] tile, row-major.  The tile has at most 64 x COLS / 4
  // elements, so kEpiTrips = COLS / 16 trips cover it and the loops unroll fully;
  // (row, col) start from one division and step by constants of the launch.
  // A trip past the last row loads and stores at kMlpPastEnd: the mask reads
  // zeros without traffic, the store is dropped.
  constexpr int kEpiTrips = MlpSmem<NCB, SLIM>::TRIPS;
  const int per_row = n4 / 4;
  const int drow = kMlpThreads / per_row, dcol = kMlpThreads - drow * per_row;
  const int row0 = tid / per_row, col0 = tid - row0 * per_row;
  const int nrows = static_cast<int>(rows);
  auto next_trip = [&](int& row, int& col) {
    row += drow;
    col += dcol;
    if (col >= per_row) {
      col -= per_row;
      ++row;
    }
  };
  // the epilogue mask of the thread's whole share, issued before the
  // accumulators go through LDS: one exposed round trip instead of one per trip
  f32x4 mk[kEpiTrips];
  if (v4 && cm) {
    const __amdgpu_buffer_rsrc_t dcm = mlp_desc(cm, static_cast<uint64_t>((rows - 1) * a.ldcm + N) * 4);
    const unsigned ldcm4 = static_cast<unsigned>(a.ldcm) * 4;
    int row = row0, col = col0;
#pragma unroll
    for (int t = 0; t < kEpiTrips; ++t) {
      mk[t] = mlp_load4(dcm, row < nrows ? row * ldcm4 + col * 16 : kMlpPastEnd);
      next_trip(row, col);
    }
  }
  __syncthreads();  // every wave is done reading the A stages
  float* tile = reinterpret_cast<float*>(smem_raw);
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int col = blk(i) * 32 + l32;
    const float b = bias[i];
    // a row holds n4 columns: a lane past them would write into the next row;
    // a skipped block writes nothing
    if (col < n4 && !(i == NCB - 1 && last_dead)) {
      if constexpr (SLIM) {
        if (i == NCB - 1) {  // one tile: row half `wave`
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            float v = acc[0][i][r] + b;
            if (a.relu) v = v > 0.0f ? v : 0.0f;
            tile[(32 * wave + (r & 3) + 8 * (r >> 2) + 4 * h) * OUT_LD + col] = v;
          }
          continue;
        }
      }
#pragma unroll
      for (int rb = 0; rb < kMlpRB; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float v = acc[rb][i][r] + b;
          if (a.relu) v = v > 0.0f ? v : 0.0f;
          tile[(32 * rb + (r & 3) + 8 * (r >> 2) + 4 * h) * OUT_LD + col] = v;
        }
    }
  }
  __syncthreads();
  if (v4) {
    const __amdgpu_buffer_rsrc_t dc = mlp_desc(C, static_cast<uint64_t>((rows - 1) * a.ldc + n4) * 4);
    const unsigned ldc4 = static_cast<unsigned>(a.ldc) * 4;
    auto store_rows = [&](auto masked_c) {
      constexpr bool MASKED = decltype(masked_c)::value;
      int row = row0, col = col0;
#pragma unroll
      for (int t = 0; t < kEpiTrips; ++t) {
        const bool live = row < nrows;
        float* at = tile + (live ? row : 0) * OUT_LD + col * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(at);
        if constexpr (MASKED) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = mk[t][e] > 0.0f ? v[e] : 0.0f;
          if (a.parts && live) *reinterpret_cast<f32x4*>(at) = v;  // masked, for the column sums
        }
        mlp_store4(dc, live ? row * ldc4 + col * 16 : kMlpPastEnd, v);
        next_trip(row, col);
      }
    };
    if (cm) store_rows(std::true_type());
    else store_rows(std::false_type());
  } else {
    for (int idx = tid; idx < rows * N; idx += kMlpThreads) {
      const int row = idx / N, c = idx - row * N;
      float v = tile[row * OUT_LD + c];
      if (cm && !(cm[row * a.ldcm + c] > 0.0f)) v = 0.0f;
      if (cm && a.parts) tile[row * OUT_LD + c] = v;
      C[row * a.ldc + c] = v;
    }
  }
  if (a.parts == nullptr) return;
  // column sums (the bias gradient of the layer below when C is its masked
  // output gradient): this workgroup's rows in order; mlp_colsum_kernel then
  // adds the workgroups' partials in workgroup order (deterministic).
  __syncthreads();
  for (int c = tid; c < N; c += kMlpThreads) {
    float sum = 0.0f;
    for (int row = 0; row < rows; ++row) sum += tile[row * OUT_LD + c];  // already masked
    a.parts[bid * a.N + c0 + c] = sum;
  }
}

// N > 384: workgroup `id` of a problem's nrb * G, one (row block, column group)
// each.  The NBp / 4 128-column units are dealt evenly, G = ceil(units / 3)
// groups of base or base + 1 units (the first `units % G` groups get the extra
// one), and each group runs the instantiation for its own unit count, picked
// at run time (workgroup-uniform) like the pair kernel's two problems: every
// group touches only whole units below NBp, so no image block past the
// padding is loaded and no guard sits in the main loop.  XMAX (2 or 3) is the
// largest group of the launch, which sizes the LDS: N <= 512 is two 2-unit
// groups with a 66.5 KiB tile, two workgroups per CU.
// a.order (chosen by rows_order on the host):
// 0: row-major over the XCDs.  Block ids are dealt round-robin to the 8 XCDs;
// XCD x takes a contiguous chunk of the (row block, group) list in its
// dispatch order (chunks differ by at most one when 8 does not divide the
// count), so the G groups of a row block run back to back on one XCD and the
// later ones read the block's A rows from that XCD's L2.
// 1: group-major, id = g * nrb + rb.
__device__ __forceinline__ int mlp_xcd_chunk(int id, int n) {
  const int q = n >> 3, r = n & 7, x = id & 7;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (id >> 3);
}

template <int XMAX, bool HAS_MASK>
__device__ __forceinline__ void mlp_rows_grouped(const MlpArgs& a, const int id, char* smem_raw) {
  const int nrb = static_cast<int>((a.M + kMlpBM - 1) / kMlpBM);
  int rb, g;
  if (a.order == 0) {
    const int t = mlp_xcd_chunk(id, nrb * a.G);
    rb = t / a.G;
    g = t - rb * a.G;
  } else {
    g = id / nrb;
    rb = id - g * nrb;
  }
  const int units = a.NBp >> 2, base = units / a.G, extra = units - base * a.G;
  const int ncb = base + (g < extra ? 1 : 0);
  const int cb0 = 4 * (g * base + (g < extra ? g : extra));
  if (ncb == 1) mlp_rows_block<1, HAS_MASK, true>(a, rb, smem_raw, cb0);
  else if (XMAX == 2 || ncb == 2) mlp_rows_block<2, HAS_MASK, true>(a, rb, smem_raw, cb0);
  else mlp_rows_block<3, HAS_MASK, true>(a, rb, smem_raw, cb0);
}

// SLIM is instantiated where mlp_slim_class says; the grouped and pair kernels
// keep the full class of their widest problem.
template <int NCB, bool HAS_MASK, bool SLIM = false>
__global__ void __launch_bounds__(kMlpThreads) mlp_rows_kernel(const MlpArgs a) {
  __shared__ __attribute__((aligned(16))) char smem_raw[MlpSmem<NCB, SLIM>::BYTES];
  mlp_rows_block<NCB, HAS_MASK, false, SLIM>(a, blockIdx.x, smem_raw);
}

template <int XMAX, bool HAS_MASK>
__global__ void __launch_bounds__(kMlpThreads) mlp_rows_grouped_kernel(const MlpArgs a) {
  __shared__ __attribute__((aligned(16))) char smem_raw[MlpSmem<XMAX>::BYTES];
  mlp_rows_grouped<XMAX, HAS_MASK>(a, blockIdx.x, smem_raw);
}

// Two problems in one launch when at least one is wider than 384: blocks
// [0, split) are a0's nrb0 * G0 (row block, group) pairs, the rest a1's (a
// narrow problem is one group of NBp / 4 units).
template <int XMAX, bool HAS_MASK>
__global__ void __launch_bounds__(kMlpThreads) mlp_rows_grouped_pair_kernel(const MlpArgs a0, const MlpArgs a1,
                                                                            const int split) {
  __shared__ __attribute__((aligned(16))) char smem_raw[MlpSmem<XMAX>::BYTES];
  const int b = blockIdx.x;
  if (b < split) mlp_rows_grouped<XMAX, HAS_MASK>(a0, b, smem_raw);
  else mlp_rows_grouped<XMAX, HAS_MASK>(a1, b - split, smem_raw);
}

// Two independent problems in one launch (the two towers' layers): blocks
// [0, split) are a0's, the rest a1's.
template <int NCB0, int NCB1, bool HAS_MASK>
__global__ void __launch_bounds__(kMlpThreads) mlp_rows_pair_kernel(const MlpArgs a0, const MlpArgs a1,
                                                                    const int split) {
  constexpr int B0 = MlpSmem<NCB0>::BYTES, B1 = MlpSmem<NCB1>::BYTES;
  __shared__ __attribute__((aligned(16))) char smem_raw[B0 > B1 ? B0 : B1];
  const int b = blockIdx.x;
  if (b < split) mlp_rows_block<NCB0, HAS_MASK>(a0, b, smem_raw);
  else mlp_rows_block<NCB1, HAS_MASK>(a1, b - split, smem_raw);
}

// out[c] = sum over b of parts[b][c] in b order; 64 columns x 16 row groups
// per block, the 16 group sums added in order in LDS.
__global__ void __launch_bounds__(1024) mlp_colsum_kernel(const float* __restrict__ parts, int nblk, int N,
                                                          float* __restrict__ out) {
  __shared__ float red[16][65];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63);
  const int grp = threadIdx.x >> 6;
  const int per = (nblk + 15) / 16;
  float sum = 0.0f;
  if (c < N) {
    const int b1 = min(nblk, (grp + 1) * per);
    for (int bb = grp * per; bb < b1; bb += 16) {  // 16 loads in flight (index clamped), added in order
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = parts[static_cast<int64_t>(min(bb + u, b1 - 1)) * N + c];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (bb + u < b1) sum += v[u];
    }
  }
  red[grp][threadIdx.x & 63] = sum;
  __syncthreads();
  if (grp == 0 && c < N) {
    float t = red[0][threadIdx.x];
#pragma unroll
    for (int g = 1; g < 16; ++g) t += red[g][threadIdx.x];
    out[c] = t;
  }
}


// ---------------------------------------------------------------------------
// Weight gradient of a Dense layer (the tape's MatMul for the kernel and
// BiasAddGrad for the bias, tower.py:41-49):
//   [dW; db] = [A | 1]^T . Gm    (A [M, Ka] activations, Gm [M, N] the
//   layer's output gradient, optionally Gm = (gmask > 0) ? G * s : 0 — the
//   ReluGrad of the layer's own relu folded into the load)
// The output [Ka + 1, N] is exactly the flat parameter layout (kernel rows
// then the bias row).
//
// One kernel template, mlp_wgrad_block<MASK, WI, WJ>, for every output tile
// of 64 WI x 64 WJ (64 x 64, 128 x 64, 64 x 128, 128 x 128; wgrad_tile() below
// picks, DESIGN section 9 has what each measured).
// Split-K over the batch: grid = S splits x output tiles; each workgroup
// reduces its split's rows for one tile into its split's partial
// [Ka + 1, N], and mlp_sum_parts_kernel adds the partials in split order
// (deterministic).  The tiles of one split sit on one XCD (blockIdx % 8
// picks the XCD), so the split's rows that its tiles all stage come from
// that XCD's L2.
// Stage: both MFMA operands need 8 consecutive BATCH rows per lane; the
// 32-row stages (planes A hi, A lo, G hi, G lo) are written ROW-major (as
// loaded: each thread converts 8 consecutive columns of one row to bf16
// hi / lo and stores 16 B per plane) and the fragments are read with the
// hardware transposing read ds_read_b64_tr_b16 (4 rows x 16 columns per
// 16-lane group, delivered column-major).  A 64-column plane has rows 192 B
// apart (128 B of data), a 128-column one 320 B (256 B of data).  Banks: a
// transposing read serves a 32-lane half per cycle over 64 banks; its 4 rows
// x 2 16-lane groups are 8 banks wide each and start at bank 48 q + 8 g
// (mod 64) for the 192-B pitch and 80 q + 8 g = 16 q + 8 g for 320 B past
// the fragment's first column: eight disjoint ranges that cover the 64 banks.
// The stash stores 16 B per lane with the 8 (16) lanes of a row writing its
// 128 (256) contiguous bytes: every 8-lane group of a ds_write_b128 covers
// the 32 store banks once.
// 4 waves; wave w owns the quadrant (w & 1, w >> 1) of the tile; bf16x3
// (a_lo b_hi, then a_hi b_lo, then a_hi b_hi), fp32 accumulation.
//
// What WI and WJ change.  A wave's quadrant is WI x WJ MFMA blocks of
// 32 x 32, so per k-step it reads WI + WJ fragments per plane and issues
// 3 WI WJ MFMAs (3 per 8 transposing reads at 64 x 64, 12 per 16 at
// 128 x 128); each A element is re-read and split by N / (64 WJ) column
// tiles and each G element by (Ka + 1) / (64 WI) row tiles.  The splits, the
// 16-row k-steps from the split's first row, the k -> lane mapping of the
// fragments and the order of the three products do not depend on WI, WJ, so
// every output element sums the same terms in the same order: all tiles are
// bit-identical.  LDS, double-buffered: 48 KiB at 64 x 64, 64 KiB for the two
// half-wide shapes, 80 KiB at 128 x 128 (40 KiB per stage); at most 256
// registers (2 waves per SIMD), so at least two workgroups share a CU — the
// two towers' launches run side by side.  Two stages of loads are in flight
// for every tile (three do not fit the registers beside the accumulators:
// the 128 x 128 build spilled ~100 registers), with the stash of the next
// stage under the MFMAs of this one.  The splits are not the tile's to
// change, so a wide tile has 2-4 x fewer workgroups (96-256 at the C3
// shapes, one per CU at most): what it saves in staged bytes and conversions
// it partly pays back in exposed load latency.
constexpr int kWgThreads = 256;
constexpr int kWgTile = 64;       // tile unit: 64 rows of [A | 1]^T x 64 columns of Gm
constexpr int kWgBK = 32;         // batch rows per stage (2 MFMA k-steps)

struct WgradArgs {
  const float* A;
  int64_t lda;
  const float* G;
  int64_t ldg;
  const float* gmask;  // (MASK) Gm = (gmask > 0) ? G * s : 0
  int64_t ldgm;
  const float* scale;
  int64_t M;
  int Ka, N;
  int TI, TJ, S;       // tiles along [A | 1] columns and Gm columns, splits
  int64_t rows_per_split;
  float* parts;        // [S][(Ka + 1) * N]
};

typedef __bf16 wg_bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) wg_bf16x4 lds_bf16x4_t;

constexpr int wg_pitch(int w) { return w == 2 ? 320 : 192; }
typedef float wg_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 wg_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned wg_pack2(float lo, float hi) {  // bf16(lo) | bf16(hi) << 16
  return __builtin_bit_cast(unsigned, __builtin_convertvector(wg_f32x2{lo, hi}, wg_bf16x2));
}
template <int WI, int WJ>
constexpr int kWgStageB = 2 * kWgBK * (wg_pitch(WI) + wg_pitch(WJ));

// Workgroup b of one problem; wsm holds 2 * kWgStageB<WI, WJ> bytes.
template <bool MASK, int WI, int WJ>
__device__ __forceinline__ void mlp_wgrad_block(const WgradArgs& a, const int b, char* wsm) {
  constexpr int TA = 64 * WI, TG = 64 * WJ;
  constexpr int PA = wg_pitch(WI), PG = wg_pitch(WJ);
  constexpr int PLA = kWgBK * PA, PLG = kWgBK * PG;  // plane bytes
  constexpr int STAGE = kWgStageB<WI, WJ>;
  constexpr int RA = kWgBK / WI, RG = kWgBK / WJ;  // rows per loader pass
  constexpr int D = 2;                             // stages of global loads in flight
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int lane = lane_id();
  // b -> (split, tile); the tiles of a split on one XCD when S % 8 == 0
  const int tiles = a.TI * a.TJ;
  int split, tile;
  if (a.S % 8 == 0) {
    const int q = b >> 3;
    tile = q % tiles;
    split = (q / tiles) * 8 + (b & 7);
  } else {
    tile = b % tiles;
    split = b / tiles;
  }
  const int i0 = (tile / a.TJ) * TA;
  const int j0 = (tile % a.TJ) * TG;
  const int64_t r0 = static_cast<int64_t>(split) * a.rows_per_split;
  int64_t r1 = r0 + a.rows_per_split;
  if (r1 > a.M) r1 = a.M;
  // a split starting past M (rows_per_split is rounded up to whole stages)
  // has no rows: its descriptors get 0 bytes, so every load returns zeros
  // instead of reading past the operands
  if (r1 < r0) r1 = r0;
  const int nstage = r1 > r0 ? static_cast<int>((r1 - r0 + kWgBK - 1) / kWgBK) : 0;
  const float s = a.scale ? *a.scale : 1.0f;

  // loader: an operand tile of 64 W columns has 8 W lanes per row (8 columns
  // each) and is staged in W passes of 32 / W rows; range-checked buffer loads
  // (rows past the split read 0)
  const int rowa = tid / (8 * WI), cola = (tid % (8 * WI)) * 8;
  const int rowg = tid / (8 * WJ), colg = (tid % (8 * WJ)) * 8;
  const __amdgpu_buffer_rsrc_t dA = mlp_desc(a.A + r0 * a.lda, static_cast<uint64_t>(r1 - r0) * a.lda * 4);
  const __amdgpu_buffer_rsrc_t dG = mlp_desc(a.G + r0 * a.ldg, static_cast<uint64_t>(r1 - r0) * a.ldg * 4);
  const __amdgpu_buffer_rsrc_t dM =
      mlp_desc(MASK ? a.gmask + r0 * a.ldgm : a.G, static_cast<uint64_t>(r1 - r0) * (MASK ? a.ldgm : a.ldg) * 4);
  const unsigned lda4 = static_cast<unsigned>(a.lda) * 4, ldg4 = static_cast<unsigned>(a.ldg) * 4,
                 ldm4 = static_cast<unsigned>(MASK ? a.ldgm : a.ldg) * 4;
  const int ca = i0 + cola, cg = j0 + colg;
  const unsigned oa = rowa * lda4 + static_cast<unsigned>(ca) * 4;
  const unsigned og = rowg * ldg4 + static_cast<unsigned>(cg) * 4;
  const unsigned om = rowg * ldm4 + static_cast<unsigned>(cg) * 4;
  f32x4 va[D][WI][2], vg[D][WJ][2], vm[D][MASK ? WJ : 1][2];
  auto fetch = [&](int st, auto slot_c) {
    constexpr int SL = decltype(slot_c)::value;
#pragma unroll
    for (int p = 0; p < WI; ++p) {
      const unsigned sa = static_cast<unsigned>(st * kWgBK + p * RA) * lda4;
      va[SL][p][0] = mlp_load4s(dA, oa, sa);
      va[SL][p][1] = mlp_load4s(dA, oa + 16, sa);
    }
#pragma unroll
    for (int p = 0; p < WJ; ++p) {
      const unsigned sg = static_cast<unsigned>(st * kWgBK + p * RG) * ldg4;
      vg[SL][p][0] = mlp_load4s(dG, og, sg);
      vg[SL][p][1] = mlp_load4s(dG, og + 16, sg);
      if constexpr (MASK) {
        const unsigned sm = static_cast<unsigned>(st * kWgBK + p * RG) * ldm4;
        vm[SL][p][0] = mlp_load4s(dM, om, sm);
        vm[SL][p][1] = mlp_load4s(dM, om + 16, sm);
      }
    }
  };
  // 8 values -> 16 B of hi at p and 16 B of lo one plane on; two values per
  // conversion (v_cvt_pk_bf16_f32: the rounding of bf16_bits)
  auto put8 = [&](char* p, int plane, const float (&x)[8]) {
    unsigned hw[4], lw[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      hw[e] = wg_pack2(x[2 * e], x[2 * e + 1]);
      lw[e] = wg_pack2(x[2 * e] - __uint_as_float(hw[e] << 16), x[2 * e + 1] - __uint_as_float(hw[e] & 0xffff0000u));
    }
    *reinterpret_cast<u32x4*>(p) = u32x4{hw[0], hw[1], hw[2], hw[3]};
    *reinterpret_cast<u32x4*>(p + plane) = u32x4{lw[0], lw[1], lw[2], lw[3]};
  };
  // EDGE: the tile reaches past column Ka - 1 of A (the ones column, padding)
  // or past column N - 1 of Gm: those columns are set after the load (their
  // loads read on into the row's padding or the next row, or 0 past the
  // split); an interior tile stages what it loaded
  auto stash = [&](int st, int buf, auto slot_c, auto edge_c) {
    constexpr int SL = decltype(slot_c)::value;
    constexpr bool EDGE = decltype(edge_c)::value;
    char* base = wsm + buf * STAGE;
    float x[8];
#pragma unroll
    for (int p = 0; p < WI; ++p) {
      const int row = rowa + p * RA;
      const bool live = EDGE && r0 + static_cast<int64_t>(st) * kWgBK + row < r1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // [A | 1]: the ones column is the bias row of the output
        const int col = ca + e;
        const float v = va[SL][p][e >> 2][e & 3];
        x[e] = !EDGE || col < a.Ka ? v : ((col == a.Ka && live) ? 1.0f : 0.0f);
      }
      put8(base + row * PA + cola * 2, PLA, x);
    }
#pragma unroll
    for (int p = 0; p < WJ; ++p) {
      const int row = rowg + p * RG;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int col = cg + e;
        float v = !EDGE || col < a.N ? vg[SL][p][e >> 2][e & 3] : 0.0f;
        if constexpr (MASK) v = vm[SL][p][e >> 2][e & 3] > 0.0f ? v * s : 0.0f;
        x[e] = v;
      }
      put8(base + 2 * PLA + row * PG + colg * 2, PLG, x);
    }
  };

  // fragments: 16-lane group g -> MFMA rows / columns 16 (g & 1) .. + 15 of
  // a 32-block, batch rows 8 (g >> 1) .. + 7 of the k-step; lane 4q + p4 of
  // the group addresses row q, columns 4 p4 .. 4 p4 + 3
  const int ib = wave & 1, jb = wave >> 1;
  const int g = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
  const int frow = 8 * (g >> 1) + q;
  const int fa = frow * PA + (32 * WI * ib + 16 * (g & 1) + 4 * p4) * 2;
  const int fg = 2 * PLA + frow * PG + (32 * WJ * jb + 16 * (g & 1) + 4 * p4) * 2;
  auto frag = [&](const char* at, int pitch) {
    const wg_bf16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(at));
    const wg_bf16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)(at + 4 * pitch));
    return __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
  };
  f32x16 acc[WI][WJ] = {};
  auto compute = [&](int buf) {
    const char* base = wsm + buf * STAGE;
#pragma unroll
    for (int ks = 0; ks < kWgBK / 16; ++ks) {
      bf16x8 ah[WI], al[WI], gh[WJ], gl[WJ];
#pragma unroll
      for (int bi = 0; bi < WI; ++bi) {
        ah[bi] = frag(base + fa + ks * 16 * PA + bi * 64, PA);
        al[bi] = frag(base + PLA + fa + ks * 16 * PA + bi * 64, PA);
      }
#pragma unroll
      for (int bj = 0; bj < WJ; ++bj) {
        gh[bj] = frag(base + fg + ks * 16 * PG + bj * 64, PG);
        gl[bj] = frag(base + PLG + fg + ks * 16 * PG + bj * 64, PG);
      }
#pragma unroll
      for (int bi = 0; bi < WI; ++bi)
#pragma unroll
        for (int bj = 0; bj < WJ; ++bj) {
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[bi], gh[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[bi], gl[bj], acc[bi][bj], 0, 0, 0);
          acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[bi], gh[bj], acc[bi][bj], 0, 0, 0);
        }
    }
  };

  // pipeline: stage st + 1 is split and stashed into the other buffer in the
  // same scheduling region as the MFMAs of stage st, so one wave's conversions
  // run under its own MFMAs (with one or two waves per SIMD nothing else
  // would); one barrier per stage: past it every wave has computed stage st
  // (its buffer is free for stage st + 2) and stashed stage st + 1.  Stage X
  // is fetched into slot X & 1 two steps before it is stashed.
  auto pipeline = [&](auto edge_c) {
    fetch(0, std::integral_constant<int, 0>());
    __builtin_amdgcn_sched_barrier(0);
    fetch(1, std::integral_constant<int, 1>());
    __builtin_amdgcn_sched_barrier(0);
    stash(0, 0, std::integral_constant<int, 0>(), edge_c);
    __builtin_amdgcn_sched_barrier(0);
    fetch(2, std::integral_constant<int, 0>());
    __builtin_amdgcn_sched_barrier(0);
    lds_barrier();
    auto step = [&](int st, auto slot_c) {  // slot_c: the slot of stage st + 1
      __builtin_amdgcn_sched_barrier(0);
      compute(st & 1);
      stash(st + 1, (st + 1) & 1, slot_c, edge_c);  // past the split: zeros, unused
      __builtin_amdgcn_sched_barrier(0);
      fetch(st + 1 + D, slot_c);
      __builtin_amdgcn_sched_barrier(0);
      lds_barrier();
    };
    for (int st = 0; st < nstage; st += 2) {
      step(st, std::integral_constant<int, 1>());
      step(st + 1, std::integral_constant<int, 0>());
    }
  };
  // branch-free loop bodies (stages past the split stage zeros, which add
  // nothing), so the compiler's vmcnt waits stay exact across the stages in
  // flight; the edge test is workgroup-uniform: a scalar branch, every lane
  // stays active for the transposing reads
  if (i0 + TA > a.Ka || j0 + TG > a.N) pipeline(std::true_type());
  else pipeline(std::false_type());

  // block (bi, bj) of the split's partial: lane (l32, h), register r -> row
  // 32 (WI ib + bi) + (r & 3) + 8 (r >> 2) + 4 h, column 32 (WJ jb + bj) + l32
  const int rows_out = a.Ka + 1;
  float* P = a.parts + static_cast<int64_t>(split) * rows_out * a.N;
#pragma unroll
  for (int bi = 0; bi < WI; ++bi)
#pragma unroll
    for (int bj = 0; bj < WJ; ++bj) {
      const int n = j0 + 32 * (WJ * jb + bj) + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = i0 + 32 * (WI * ib + bi) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (n < a.N && row < rows_out) P[static_cast<int64_t>(row) * a.N + n] = acc[bi][bj][r];
      }
    }
}

template <bool MASK, int WI, int WJ>
__global__ void __launch_bounds__(kWgThreads, 2) mlp_wgrad_kernel(const WgradArgs a) {
  __shared__ __attribute__((aligned(16))) char wsm[2 * kWgStageB<WI, WJ>];
  mlp_wgrad_block<MASK, WI, WJ>(a, blockIdx.x, wsm);
}

// Two problems in one launch: blocks [0, split) are a0's (split % 8 == 0
// keeps the second problem's split -> XCD mapping).
template <bool MASK, int WI, int WJ>
__global__ void __launch_bounds__(kWgThreads, 2) mlp_wgrad_pair_kernel(const WgradArgs a0, const WgradArgs a1,
                                                                            const int split) {
  __shared__ __attribute__((aligned(16))) char wsm[2 * kWgStageB<WI, WJ>];
  const int b = blockIdx.x;
  if (b < split) mlp_wgrad_block<MASK, WI, WJ>(a0, b, wsm);
  else mlp_wgrad_block<MASK, WI, WJ>(a1, b - split, wsm);
}

// out[e] = sum over splits of parts[sp][e] (deterministic): a block covers 64
// float4 of the output; group g of 16 adds splits [g S/16, (g+1) S/16) in
// order (their loads all in flight), then the 16 group sums are added in
// group order.  len % 4 == 0.
// Optional Adagrad on the summed gradient (tt_mlp_wgrad_adagrad): the layer's
// parameters and accumulator, the same per-element arithmetic as
// tt_dense_adagrad.
struct PartsAdagrad {
  float* param;  // NULL: none
  float* accum;
  float lr, eps;
};

__device__ __forceinline__ void mlp_sum_parts_block(const float* __restrict__ parts, int S, int64_t len,
                                                    float* __restrict__ out, const int64_t bid, f32x4 (*red)[64],
                                                    const PartsAdagrad& ad = PartsAdagrad{}) {
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t e4 = (bid * 64 + lane) * 4;
  const int per = (S + 15) / 16;
  const int s0 = grp * per, s1 = min(S, s0 + per);
  f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  // the Adagrad operands of the threads that apply it (group 0) do not depend
  // on the sum: loaded with the partials, not in a round trip of their own
  // after it (the plain sum, ad.param == NULL, loads nothing here)
  const bool apply = ad.param != nullptr && grp == 0 && e4 < len;
  f32x4 pa = {0.0f, 0.0f, 0.0f, 0.0f}, ac = pa;
  if (apply) {
    pa = *reinterpret_cast<const f32x4*>(ad.param + e4);
    ac = *reinterpret_cast<const f32x4*>(ad.accum + e4);
  }
  if (e4 < len) {
    f32x4 v[8];
    for (int sb = s0; sb < s1; sb += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (sb + u < s1) v[u] = *reinterpret_cast<const f32x4*>(parts + (sb + u) * len + e4);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (sb + u < s1) {
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[q] += v[u][q];
        }
    }
  }
  red[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && e4 < len) {
    f32x4 t = red[0][lane];
    for (int g = 1; g < 16; ++g) {
      const f32x4 r = red[g][lane];
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] += r[q];
    }
    *reinterpret_cast<f32x4*>(out + e4) = t;
    if (apply) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gi = t[q];
        const float a = ac[q] + gi * gi;
        ac[q] = a;
        pa[q] = pa[q] - (gi * ad.lr) / (sqrtf(a) + ad.eps);
      }
      *reinterpret_cast<f32x4*>(ad.accum + e4) = ac;
      *reinterpret_cast<f32x4*>(ad.param + e4) = pa;
    }
  }
}

__global__ void __launch_bounds__(1024) mlp_sum_parts_kernel(const float* __restrict__ parts, int S, int64_t len,
                                                             float* __restrict__ out, const PartsAdagrad ad) {
  __shared__ f32x4 red[16][64];
  mlp_sum_parts_block(parts, S, len, out, blockIdx.x, red, ad);
}

// Both problems' partial sums in one launch: blocks [0, split) are the first's.
__global__ void __launch_bounds__(1024) mlp_sum_parts_pair_kernel(const float* __restrict__ p0, int S0, int64_t len0,
                                                                  float* __restrict__ o0, const float* __restrict__ p1,
                                                                  int S1, int64_t len1, float* __restrict__ o1,
                                                                  const int split) {
  __shared__ f32x4 red[16][64];
  const int b = blockIdx.x;
  if (b < split) mlp_sum_parts_block(p0, S0, len0, o0, b, red);
  else mlp_sum_parts_block(p1, S1, len1, o1, b - split, red);
}

// 256-thread form of mlp_sum_parts_block for a launch whose other block roles
// are 256 threads: the same 16 split groups, each summed from 0 in split
// order, then the 16 group sums added in group order, then the same Adagrad
// arithmetic on operands loaded with the partials — bit-identical.  Thread
// (q4, lane) adds groups 4 q4 .. 4 q4 + 3, their loads in flight together.
__device__ __forceinline__ void mlp_sum_parts_block256(const float* __restrict__ parts, int S, int64_t len,
                                                       float* __restrict__ out, const int64_t bid, f32x4 (*red)[64],
                                                       const PartsAdagrad& ad) {
  const int lane = threadIdx.x & 63, q4 = threadIdx.x >> 6;
  const int64_t e4 = (bid * 64 + lane) * 4;
  const int per = (S + 15) / 16;
  const bool apply = ad.param != nullptr && q4 == 0 && e4 < len;
  f32x4 pa = {0.0f, 0.0f, 0.0f, 0.0f}, ac = pa;
  if (apply) {
    pa = *reinterpret_cast<const f32x4*>(ad.param + e4);
    ac = *reinterpret_cast<const f32x4*>(ad.accum + e4);
  }
  f32x4 acc[4];
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) acc[gg] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  if (e4 < len) {
    for (int o = 0; o < per; o += 8) {
      f32x4 v[4][8];
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const int s0 = (4 * q4 + gg) * per, s1 = min(S, s0 + per);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (s0 + o + u < s1) v[gg][u] = *reinterpret_cast<const f32x4*>(parts + (s0 + o + u) * len + e4);
      }
#pragma unroll
      for (int gg = 0; gg < 4; ++gg) {
        const int s0 = (4 * q4 + gg) * per, s1 = min(S, s0 + per);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (s0 + o + u < s1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[gg][q] += v[gg][u][q];
          }
      }
    }
  }
#pragma unroll
  for (int gg = 0; gg < 4; ++gg) red[4 * q4 + gg][lane] = acc[gg];
  __syncthreads();
  if (q4 == 0 && e4 < len) {
    f32x4 t = red[0][lane];
#pragma unroll
    for (int g = 1; g < 16; ++g) {
      const f32x4 r = red[g][lane];
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] += r[q];
    }
    *reinterpret_cast<f32x4*>(out + e4) = t;
    if (apply) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float gi = t[q];
        const float a = ac[q] + gi * gi;
        ac[q] = a;
        pa[q] = pa[q] - (gi * ad.lr) / (sqrtf(a) + ad.eps);
      }
      *reinterpret_cast<f32x4*>(ad.accum + e4) = ac;
      *reinterpret_cast<f32x4*>(ad.param + e4) = pa;
    }
  }
}

// A layer's pending partial sums (+ its Adagrad step): the sum launch of
// tt_mlp_wgrad(_adagrad) as a block role of another launch.
struct SumJob {
  const float* parts;
  int S;
  int64_t len;
  float* out;
  PartsAdagrad ad;
};

// One Dense layer's backward as ONE launch of independent block roles:
// [0, nw) the layer's weight-gradient split partials (mlp_wgrad_block, the
// default tile of its kind: 128 x 64 masked, 64 x 128 unmasked),
// [nw, nw + nr) the input-gradient GEMM of the layer below (mlp_rows_block;
// WC = 0: none, 1..3: NCB = WC, 4: NCB = 3 in the SLIM class), then the
// previous (upper) layer's partial sums + Adagrad (the grid ends before them
// when there are none).
// INVARIANT: no data flows between the roles inside a launch.  The
// input-gradient role reads the packed weight IMAGE of its layer (written by
// the step's forward), never the parameters the sum role updates; the sum role
// reads the partials of the PREVIOUS launch, never those the weight-gradient
// role writes (tt_mlp_backward_layer refuses overlapping buffers).
// LDS: the largest role's (the weight-gradient stages are 64 KiB, the rows
// tile 66.5 KiB at WC = 2 and 73 KiB at WC = 4), each role carving the one
// buffer its own way; at most 256 registers: two workgroups per CU except at
// WC = 3 (97 KiB, over 256 registers: one).
template <bool WMASK, int WC, bool RMASK>
__global__ void __launch_bounds__(kWgThreads, WC == 3 ? 1 : 2) mlp_bwd_layer_kernel(const WgradArgs w, const int nw,
                                                                       const MlpArgs r, const int nr,
                                                                       const SumJob sj) {
  static_assert(kWgThreads == kMlpThreads, "one block size for every role");
  constexpr int WI = WMASK ? 2 : 1, WJ = WMASK ? 1 : 2;
  constexpr int NCB = WC > 3 ? 3 : WC;
  constexpr bool SLIM = WC == 4;
  constexpr int WB = 2 * kWgStageB<WI, WJ>, RB = WC > 0 ? MlpSmem<(NCB > 0 ? NCB : 1), SLIM>::BYTES : 0,
                SB = 16 * 64 * static_cast<int>(sizeof(f32x4));
  constexpr int BYTES = WB > RB ? (WB > SB ? WB : SB) : (RB > SB ? RB : SB);
  __shared__ __attribute__((aligned(16))) char smem[BYTES];
  int b = blockIdx.x;
  if (b < nw) {
    mlp_wgrad_block<WMASK, WI, WJ>(w, b, smem);
    return;
  }
  b -= nw;
  if constexpr (WC > 0) {
    if (b < nr) {
      mlp_rows_block<NCB, RMASK, false, SLIM>(r, b, smem);
      return;
    }
    b -= nr;
  }
  mlp_sum_parts_block256(sj.parts, sj.S, sj.len, sj.out, b, reinterpret_cast<f32x4(*)[64]>(smem), sj.ad);
}

__global__ void __launch_bounds__(256) mlp_pack_kernel(const float* __restrict__ w, int64_t ldw, int K, int N,
                                                       int trans, int KS, int NB, __bf16* __restrict__ img) {
  const int64_t t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= static_cast<int64_t>(KS) * NB * 64) return;
  const int lane = static_cast<int>(t & 63);
  pack_fragment(w, ldw, K, N, trans, static_cast<int>((t >> 6) / NB), static_cast<int>((t >> 6) % NB), NB, lane, img);
}

__global__ void __launch_bounds__(256) mlp_pack_many_kernel(const PackJobs jobs, int64_t total) {
  const int64_t t = blockIdx.x * 256ll + threadIdx.x;
  if (t >= total) return;
  pack::pack_many_thread(jobs, t);
}



}  // namespace
}  // namespace tt

using namespace tt;

extern "C" size_t tt_mlp_pack_bytes(int32_t K, int32_t N) {
  if (K < 1 || N < 1) return 0;
  return static_cast<size_t>(mlp_ks(K)) * mlp_nb(N) * 2 * 64 * 8 * sizeof(__bf16);
}

extern "C" int tt_mlp_pack(const float* w, int64_t ldw, int32_t K, int32_t N, int32_t trans, void* img,
                           size_t img_bytes, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(w && img, "tt_mlp_pack: NULL pointer");
  TT_REQUIRE(K >= 1 && N >= 1, "tt_mlp_pack: bad K/N");
  TT_REQUIRE(ldw >= (trans ? K : N), "tt_mlp_pack: ldw too small");
  TT_REQUIRE(img_bytes >= tt_mlp_pack_bytes(K, N), "tt_mlp_pack: image too small");
  const int KS = mlp_ks(K), NB = mlp_nb(N);
  const int64_t threads = static_cast<int64_t>(KS) * NB * 64;
  hipLaunchKernelGGL(mlp_pack_kernel, dim3(ceil_div(threads, 256)), dim3(256), 0, to_stream(stream), w, ldw, K, N,
                     trans ? 1 : 0, KS, NB, static_cast<__bf16*>(img));
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_mlp_pack_many(const tt_mlp_pack_job* jobs, int32_t num_jobs, tt_stream_t stream) {
  clear_error();
  PackJobs pj;
  int64_t total = 0;
  if (int rc = pack::make_pack_jobs(jobs, num_jobs, &pj, &total, "tt_mlp_pack_many")) return rc;
  hipLaunchKernelGGL(mlp_pack_many_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, to_stream(stream), pj, total);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" size_t tt_mlp_rows_workspace_size(int64_t M, int32_t N) {
  if (M < 0 || N < 1) return 0;
  return static_cast<size_t>(ceil_div(M, kMlpBM)) * N * sizeof(float);
}

// The block order of a grouped launch (mlp_rows_grouped).  Concurrent
// workgroups of order 0 cover every group, so each XCD's L2 streams the whole
// B image; those of order 1 share one group's <= 384 columns of it but
// re-read A from further away.  Measured: order 0 wins
// while the image is smaller than an XCD's 4 MiB L2 (0.5-2.4 us per launch at
// M = 16384), order 1 from there on (5 % at 4 MiB, 9-10 % at 8 and 32 MiB).
// TT_MLP_ROWS_ORDER = "xcd" / "group" forces order 0 / 1 (read at every
// call, so one process can time both); -1: set to anything else.
static int rows_order(size_t image_bytes) {
  const char* e = std::getenv("TT_MLP_ROWS_ORDER");
  if (!e || !*e) return image_bytes < (size_t(4) << 20) ? 0 : 1;
  if (!std::strcmp(e, "xcd")) return 0;
  return std::strcmp(e, "group") ? -1 : 1;
}

// Validates one tt_mlp_rows problem (no colsum) into its kernel arguments;
// ncb = column blocks per wave of its widest column group (a.G groups: one
// for N <= 384).  TT_OK or the error code (message set).
static int rows_setup(const char* fn, const float* A, int64_t lda, const float* amask, int64_t ldam,
                      const float* scale, int64_t M, int32_t K, const void* img, int32_t N, const float* bias,
                      int32_t relu, const float* cmask, int64_t ldcm, float* C, int64_t ldc, MlpArgs& a, int& ncb) {
  // a problem of no rows may come with NULL A / C (empty tensors have no storage)
  TT_REQUIRE(img && (M == 0 || (A && C)), "%s: NULL A/img/C", fn);
  TT_REQUIRE(M >= 0 && K >= 1 && N >= 1, "%s: bad M/K/N", fn);
  const int NB = mlp_nb(N);
  if (N > kMlpMaxN) return fail(TT_ERR_UNSUPPORTED, "%s: N=%d > %d unsupported", fn, N, kMlpMaxN);
  TT_REQUIRE(M * lda < (int64_t(1) << 30) && (!amask || M * ldam < (int64_t(1) << 30)),
             "%s: operand too large for 32-bit buffer offsets", fn);
  TT_REQUIRE(lda >= K && ldc >= N && (!amask || ldam >= K) && (!cmask || ldcm >= N),
             "%s: leading dimension too small", fn);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(A) % 16 == 0 && lda % 4 == 0 &&
                 (!amask || (reinterpret_cast<uintptr_t>(amask) % 16 == 0 && ldam % 4 == 0)),
             "%s: A / amask rows must be 16-B aligned (ld %% 4 == 0)", fn);
  a = MlpArgs{};
  a.A = A;
  a.lda = lda;
  a.amask = amask;
  a.ldam = ldam;
  a.scale = scale;
  a.img = static_cast<const __bf16*>(img);
  a.M = M;
  a.K = K;
  a.N = N;
  a.KSp = mlp_ks(K);
  a.NBp = NB;
  a.bias = bias;
  a.relu = relu ? 1 : 0;
  a.cmask = cmask;
  a.ldcm = ldcm;
  a.C = C;
  a.ldc = ldc;
  a.G = static_cast<int>(ceil_div(NB / 4, kMlpMaxCB));
  ncb = static_cast<int>(ceil_div(NB / 4, a.G));
  if (a.G > 1) {
    a.order = rows_order(tt_mlp_pack_bytes(K, N));
    TT_REQUIRE(a.order >= 0, "%s: TT_MLP_ROWS_ORDER must be xcd or group", fn);
  }
  return TT_OK;
}

template <bool HM>
static void launch_rows(const MlpArgs& a, int ncb, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(ceil_div(a.M, kMlpBM) * a.G));
  if (a.G > 1) {  // N > 384: (row blocks) x (column groups), ncb is 2 or 3
    if (ncb == 2) hipLaunchKernelGGL((mlp_rows_grouped_kernel<2, HM>), grid, dim3(kMlpThreads), 0, st, a);
    else hipLaunchKernelGGL((mlp_rows_grouped_kernel<3, HM>), grid, dim3(kMlpThreads), 0, st, a);
    return;
  }
  if (ncb == 1) hipLaunchKernelGGL((mlp_rows_kernel<1, HM>), grid, dim3(kMlpThreads), 0, st, a);
  else if (ncb == 2) hipLaunchKernelGGL((mlp_rows_kernel<2, HM>), grid, dim3(kMlpThreads), 0, st, a);
  else if (mlp_slim_class(ncb, HM, a.N)) hipLaunchKernelGGL((mlp_rows_kernel<3, false, true>), grid, dim3(kMlpThreads), 0, st, a);
  else hipLaunchKernelGGL((mlp_rows_kernel<3, HM>), grid, dim3(kMlpThreads), 0, st, a);
}

template <int NCB0, bool HM>
static void launch_rows_pair1(const MlpArgs& a0, const MlpArgs& a1, int ncb1, int split, dim3 grid,
                              hipStream_t st) {
  if (ncb1 == 1) hipLaunchKernelGGL((mlp_rows_pair_kernel<NCB0, 1, HM>), grid, dim3(kMlpThreads), 0, st, a0, a1, split);
  else if (ncb1 == 2) hipLaunchKernelGGL((mlp_rows_pair_kernel<NCB0, 2, HM>), grid, dim3(kMlpThreads), 0, st, a0, a1, split);
  else hipLaunchKernelGGL((mlp_rows_pair_kernel<NCB0, 3, HM>), grid, dim3(kMlpThreads), 0, st, a0, a1, split);
}

template <bool HM>
static void launch_rows_pair(const MlpArgs& a0, int ncb0, const MlpArgs& a1, int ncb1, hipStream_t st) {
  const int split = static_cast<int>(ceil_div(a0.M, kMlpBM) * a0.G);
  const dim3 grid(static_cast<unsigned>(split + ceil_div(a1.M, kMlpBM) * a1.G));
  if (a0.G > 1 || a1.G > 1) {  // a wide problem: the grouped blocks of both (a wide one's ncb is 2 or 3)
    if (ncb0 < 3 && ncb1 < 3)
      hipLaunchKernelGGL((mlp_rows_grouped_pair_kernel<2, HM>), grid, dim3(kMlpThreads), 0, st, a0, a1, split);
    else hipLaunchKernelGGL((mlp_rows_grouped_pair_kernel<3, HM>), grid, dim3(kMlpThreads), 0, st, a0, a1, split);
    return;
  }
  if (ncb0 == 1) launch_rows_pair1<1, HM>(a0, a1, ncb1, split, grid, st);
  else if (ncb0 == 2) launch_rows_pair1<2, HM>(a0, a1, ncb1, split, grid, st);
  else launch_rows_pair1<3, HM>(a0, a1, ncb1, split, grid, st);
}

extern "C" int tt_mlp_rows(const float* A, int64_t lda, const float* amask, int64_t ldam, const float* scale,
                           int64_t M, int32_t K, const void* img, int32_t N, const float* bias, int32_t relu,
                           const float* cmask, int64_t ldcm, float* C, int64_t ldc, float* colsum, void* workspace,
                           size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  MlpArgs a;
  int ncb = 0;
  const int rc = rows_setup("tt_mlp_rows", A, lda, amask, ldam, scale, M, K, img, N, bias, relu, cmask, ldcm, C, ldc,
                            a, ncb);
  if (rc != TT_OK) return rc;
  if (M == 0) return TT_OK;
  if (colsum) {
    TT_REQUIRE(workspace && workspace_bytes >= tt_mlp_rows_workspace_size(M, N),
               "tt_mlp_rows: colsum needs a workspace of tt_mlp_rows_workspace_size bytes");
    a.parts = static_cast<float*>(workspace);
  }
  hipStream_t st = to_stream(stream);
  if (amask) launch_rows<true>(a, ncb, st);
  else launch_rows<false>(a, ncb, st);
  TT_CHECK_LAUNCH();
  if (colsum) {
    hipLaunchKernelGGL(mlp_colsum_kernel, dim3(ceil_div(N, 64)), dim3(1024), 0, st, a.parts,
                       static_cast<int>(ceil_div(M, kMlpBM)), N, colsum);
  }
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_mlp_rows_pair(const tt_mlp_rows_problem* p, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(p, "tt_mlp_rows_pair: NULL problems");
  MlpArgs a[2];
  int ncb[2];
  for (int i = 0; i < 2; ++i) {
    const tt_mlp_rows_problem& q = p[i];
    const int rc = rows_setup("tt_mlp_rows_pair", q.A, q.lda, q.amask, q.ldam, q.scale, q.M, q.K, q.img, q.N,
                              q.bias, q.relu, q.cmask, q.ldcm, q.C, q.ldc, a[i], ncb[i]);
    if (rc != TT_OK) return rc;
  }
  if (a[0].M == 0 && a[1].M == 0) return TT_OK;  // nothing to launch (as tt_mlp_rows)
  hipStream_t st = to_stream(stream);
  const bool hm0 = a[0].amask != nullptr, hm1 = a[1].amask != nullptr;
  if (a[0].M == 0 || a[1].M == 0 || hm0 != hm1) {  // one problem, or masks differ: one launch each
    for (int i = 0; i < 2; ++i) {
      if (a[i].M == 0) continue;
      if (a[i].amask) launch_rows<true>(a[i], ncb[i], st);
      else launch_rows<false>(a[i], ncb[i], st);
    }
  } else if (hm0) {
    launch_rows_pair<true>(a[0], ncb[0], a[1], ncb[1], st);
  } else {
    launch_rows_pair<false>(a[0], ncb[0], a[1], ncb[1], st);
  }
  TT_CHECK_LAUNCH();
  return TT_OK;
}

static int wgrad_splits(int64_t M, int Ka, int N) {
  const int tiles = static_cast<int>(ceil_div(Ka + 1, kWgTile) * ceil_div(N, kWgTile));
  // TT_WGRAD_WGS: workgroups to aim for (default 1024: ~4 per CU, so the
  // loads of co-resident workgroups hide each other's latency)
  static const int64_t target = [] {
    const char* e = std::getenv("TT_WGRAD_WGS");
    return static_cast<int64_t>(e ? std::atoi(e) : 1024);
  }();
  int64_t S = 1;
  while (S < 256 && tiles * S * 2 <= target && M / (2 * S) >= 128) S *= 2;
  return static_cast<int>(S);
}

extern "C" size_t tt_mlp_wgrad_workspace_size(int64_t M, int32_t Ka, int32_t N) {
  if (M < 0 || Ka < 0 || N < 1) return 0;
  return static_cast<size_t>(wgrad_splits(M, Ka, N)) * (Ka + 1) * N * sizeof(float);
}

// The output tile of the weight-gradient launches, in 64-wide units per side
// ([A | 1] columns x Gm columns).  TT_WGRAD_TILE (read at every call, so one
// process can run every form): unset = 128 x 64 for a masked problem (Gm and
// its mask are the doubled stream: half as many row tiles re-read them) and
// 64 x 128 otherwise; 128 = 128 x 128; 128x64 / 64x128 / 64 = that shape
// (64: 64 x 64) for every problem.
struct WgradTile {
  int wi, wj;
};
static WgradTile wgrad_default_tile(bool masked) { return masked ? WgradTile{2, 1} : WgradTile{1, 2}; }
static WgradTile wgrad_tile(bool masked) {
  const char* e = std::getenv("TT_WGRAD_TILE");
  if (!e || !*e) return wgrad_default_tile(masked);
  if (!std::strcmp(e, "128")) return {2, 2};
  if (!std::strcmp(e, "64")) return {1, 1};
  if (!std::strcmp(e, "128x64")) return {2, 1};
  if (!std::strcmp(e, "64x128")) return {1, 2};
  return {0, 0};
}
#define TT_REQUIRE_WGRAD_TILE(t, fn) \
  TT_REQUIRE((t).wi != 0, "%s: TT_WGRAD_TILE must be 128, 64, 128x64 or 64x128", fn)

// Validates one tt_mlp_wgrad problem into its kernel arguments (parts unset).
static int wgrad_setup(const char* fn, const float* A, int64_t lda, const float* G, int64_t ldg, const float* gmask,
                       int64_t ldgm, const float* scale, int64_t M, int32_t Ka, int32_t N, float* dwb,
                       const WgradTile t, WgradArgs& a) {
  TT_REQUIRE(dwb && (M == 0 || (A && G)), "%s: NULL A/G/dwb", fn);
  TT_REQUIRE(M >= 0 && Ka >= 1 && Ka <= 4096, "%s: Ka=%d outside [1, 4096]", fn, Ka);
  TT_REQUIRE(N >= 4 && N <= 4096 && N % 4 == 0, "%s: N=%d must be a multiple of 4 in [4, 4096]", fn, N);
  TT_REQUIRE(lda >= Ka && ldg >= N && (!gmask || ldgm >= N), "%s: leading dimension too small", fn);
  // 16-B vector loads of 8-column groups
  TT_REQUIRE(lda % 4 == 0, "%s: lda must be a multiple of 4", fn);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(A) % 16 == 0 && ldg % 4 == 0 && reinterpret_cast<uintptr_t>(G) % 16 == 0 &&
                 (!gmask || (ldgm % 4 == 0 && reinterpret_cast<uintptr_t>(gmask) % 16 == 0)),
             "%s: A / G / gmask rows must be 16-B aligned", fn);
  const int S = wgrad_splits(M, Ka, N);
  const int64_t rps = round_up(ceil_div(M > 0 ? M : 1, S), kWgBK);
  // per-split byte offsets are 32-bit (buffer loads)
  TT_REQUIRE(rps * std::max<int64_t>(lda, std::max<int64_t>(ldg, gmask ? ldgm : 0)) * 4 < (int64_t(1) << 31),
             "%s: a split's rows exceed 2 GiB", fn);
  a = WgradArgs{};
  a.A = A;
  a.lda = lda;
  a.G = G;
  a.ldg = ldg;
  a.gmask = gmask;
  a.ldgm = ldgm;
  a.scale = scale;
  a.M = M;
  a.Ka = Ka;
  a.N = N;
  a.TI = static_cast<int>(ceil_div(Ka + 1, kWgTile * t.wi));
  a.TJ = static_cast<int>(ceil_div(N, kWgTile * t.wj));
  a.S = S;
  a.rows_per_split = rps;
  return TT_OK;
}

// (tile, masked) -> the kernels' <MASK, WI, WJ>: calls f(mask, wi, wj) with
// the three as integral constants (a validated tile: wi, wj in {1, 2})
template <class F>
static void wgrad_dispatch(const WgradTile t, const bool masked, F&& f) {
  using one = std::integral_constant<int, 1>;
  using two = std::integral_constant<int, 2>;
  auto tile = [&](auto mask) {
    if (t.wi == 2 && t.wj == 2) f(mask, two(), two());
    else if (t.wi == 2) f(mask, two(), one());
    else if (t.wj == 2) f(mask, one(), two());
    else f(mask, one(), one());
  };
  if (masked) tile(std::true_type());
  else tile(std::false_type());
}

static void launch_wgrad(const WgradArgs& a, const WgradTile t, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>(a.S * a.TI * a.TJ));
  wgrad_dispatch(t, a.gmask != nullptr, [&](auto mask, auto wi, auto wj) {
    hipLaunchKernelGGL((mlp_wgrad_kernel<decltype(mask)::value, decltype(wi)::value, decltype(wj)::value>), grid,
                       dim3(kWgThreads), 0, st, a);
  });
}

namespace {
int wgrad_one(const char* fn, const float* A, int64_t lda, const float* G, int64_t ldg, const float* gmask,
              int64_t ldgm, const float* scale, int64_t M, int32_t Ka, int32_t N, float* dwb, void* workspace,
              size_t workspace_bytes, tt_stream_t stream, const PartsAdagrad& ad) {
  WgradArgs a;
  const WgradTile t = wgrad_tile(gmask != nullptr);
  TT_REQUIRE_WGRAD_TILE(t, fn);
  const int rc = wgrad_setup(fn, A, lda, G, ldg, gmask, ldgm, scale, M, Ka, N, dwb, t, a);
  if (rc != TT_OK) return rc;
  TT_REQUIRE(workspace && workspace_bytes >= tt_mlp_wgrad_workspace_size(M, Ka, N), "%s: workspace %zu < %zu", fn,
             workspace_bytes, tt_mlp_wgrad_workspace_size(M, Ka, N));
  a.parts = static_cast<float*>(workspace);
  hipStream_t st = to_stream(stream);
  launch_wgrad(a, t, st);
  TT_CHECK_LAUNCH();
  const int64_t len = static_cast<int64_t>(Ka + 1) * N;
  hipLaunchKernelGGL(mlp_sum_parts_kernel, dim3(ceil_div(len, 256)), dim3(1024), 0, st, a.parts, a.S, len, dwb, ad);
  TT_CHECK_LAUNCH();
  return TT_OK;
}
}  // namespace

extern "C" int tt_mlp_wgrad(const float* A, int64_t lda, const float* G, int64_t ldg, const float* gmask,
                            int64_t ldgm, const float* scale, int64_t M, int32_t Ka, int32_t N, float* dwb,
                            void* workspace, size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  return wgrad_one("tt_mlp_wgrad", A, lda, G, ldg, gmask, ldgm, scale, M, Ka, N, dwb, workspace, workspace_bytes,
                   stream, PartsAdagrad{});
}

extern "C" int tt_mlp_wgrad_adagrad(const float* A, int64_t lda, const float* G, int64_t ldg, const float* gmask,
                                    int64_t ldgm, const float* scale, int64_t M, int32_t Ka, int32_t N, float* dwb,
                                    float* param, float* accum, float lr, float epsilon, void* workspace,
                                    size_t workspace_bytes, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(param && accum, "tt_mlp_wgrad_adagrad: NULL param / accum");
  TT_REQUIRE(reinterpret_cast<uintptr_t>(param) % 16 == 0 && reinterpret_cast<uintptr_t>(accum) % 16 == 0,
             "tt_mlp_wgrad_adagrad: param / accum must be 16-B aligned");
  return wgrad_one("tt_mlp_wgrad_adagrad", A, lda, G, ldg, gmask, ldgm, scale, M, Ka, N, dwb, workspace,
                   workspace_bytes, stream, PartsAdagrad{param, accum, lr, epsilon});
}

// the second problem's partials start 256-B aligned after the first's
static size_t wgrad_pair_offset(const tt_mlp_wgrad_problem* p) {
  return static_cast<size_t>(round_up(static_cast<int64_t>(tt_mlp_wgrad_workspace_size(p[0].M, p[0].Ka, p[0].N)), 256));
}

extern "C" size_t tt_mlp_wgrad_pair_workspace_size(const tt_mlp_wgrad_problem* p) {
  if (!p) return 0;
  return wgrad_pair_offset(p) + tt_mlp_wgrad_workspace_size(p[1].M, p[1].Ka, p[1].N);
}

extern "C" int tt_mlp_wgrad_pair(const tt_mlp_wgrad_problem* p, void* workspace, size_t workspace_bytes,
                                 tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(p, "tt_mlp_wgrad_pair: NULL problems");
  WgradArgs a[2];
  WgradTile t[2];
  for (int i = 0; i < 2; ++i) {
    const tt_mlp_wgrad_problem& q = p[i];
    t[i] = wgrad_tile(q.gmask != nullptr);
    TT_REQUIRE_WGRAD_TILE(t[i], "tt_mlp_wgrad_pair");
    const int rc = wgrad_setup("tt_mlp_wgrad_pair", q.A, q.lda, q.G, q.ldg, q.gmask, q.ldgm, q.scale, q.M, q.Ka, q.N,
                               q.dwb, t[i], a[i]);
    if (rc != TT_OK) return rc;
  }
  const size_t need = tt_mlp_wgrad_pair_workspace_size(p);
  TT_REQUIRE(workspace && workspace_bytes >= need, "tt_mlp_wgrad_pair: workspace %zu < %zu", workspace_bytes, need);
  a[0].parts = static_cast<float*>(workspace);
  a[1].parts = reinterpret_cast<float*>(static_cast<char*>(workspace) + wgrad_pair_offset(p));
  hipStream_t st = to_stream(stream);
  const int nb0 = a[0].S * a[0].TI * a[0].TJ, nb1 = a[1].S * a[1].TI * a[1].TJ;
  if ((a[0].gmask != nullptr) != (a[1].gmask != nullptr) || nb0 % 8 != 0) {
    launch_wgrad(a[0], t[0], st);
    launch_wgrad(a[1], t[1], st);
  } else {  // both masked or both not: one tile shape
    const dim3 grid(static_cast<unsigned>(nb0 + nb1));
    wgrad_dispatch(t[0], a[0].gmask != nullptr, [&](auto mask, auto wi, auto wj) {
      hipLaunchKernelGGL((mlp_wgrad_pair_kernel<decltype(mask)::value, decltype(wi)::value, decltype(wj)::value>),
                         grid, dim3(kWgThreads), 0, st, a[0], a[1], nb0);
    });
  }
  TT_CHECK_LAUNCH();
  const int64_t len0 = static_cast<int64_t>(a[0].Ka + 1) * a[0].N, len1 = static_cast<int64_t>(a[1].Ka + 1) * a[1].N;
  const int sb0 = static_cast<int>(ceil_div(len0, 256));
  hipLaunchKernelGGL(mlp_sum_parts_pair_kernel, dim3(static_cast<unsigned>(sb0 + ceil_div(len1, 256))), dim3(1024), 0,
                     st, a[0].parts, a[0].S, len0, p[0].dwb, a[1].parts, a[1].S, len1, p[1].dwb, sb0);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

// ---- one Dense layer's backward in one launch ------------------------------
namespace {

// One weight-gradient job into its kernel arguments (the default tile of its
// kind: every tile is bit-identical, TT_WGRAD_TILE picks among the separate
// launches only) and its sum role.
int wgrad_job_setup(const char* fn, const tt_mlp_wgrad_job* j, WgradArgs& a, SumJob& s) {
  const tt_mlp_wgrad_problem& q = j->p;
  if (int rc = wgrad_setup(fn, q.A, q.lda, q.G, q.ldg, q.gmask, q.ldgm, q.scale, q.M, q.Ka, q.N, q.dwb,
                           wgrad_default_tile(q.gmask != nullptr), a))
    return rc;
  const size_t need = tt_mlp_wgrad_workspace_size(q.M, q.Ka, q.N);
  TT_REQUIRE(j->parts && j->parts_bytes >= need, "%s: partials buffer %zu < %zu bytes", fn, j->parts_bytes, need);
  TT_REQUIRE(reinterpret_cast<uintptr_t>(q.dwb) % 16 == 0 && reinterpret_cast<uintptr_t>(j->parts) % 16 == 0,
             "%s: dwb / parts must be 16-B aligned", fn);
  TT_REQUIRE(!j->param || (j->accum && reinterpret_cast<uintptr_t>(j->param) % 16 == 0 &&
                           reinterpret_cast<uintptr_t>(j->accum) % 16 == 0),
             "%s: Adagrad param / accum must both be set and 16-B aligned", fn);
  a.parts = static_cast<float*>(j->parts);
  s = SumJob{a.parts, a.S, static_cast<int64_t>(q.Ka + 1) * q.N, q.dwb,
             PartsAdagrad{j->param, j->param ? j->accum : nullptr, j->lr, j->eps}};
  return TT_OK;
}

template <bool WM, int WC>
void launch_bwd2(bool rm, const WgradArgs& w, int nw, const MlpArgs& r, int nr, const SumJob& s, dim3 grid,
                 hipStream_t st) {
  if (rm) hipLaunchKernelGGL((mlp_bwd_layer_kernel<WM, WC, true>), grid, dim3(kWgThreads), 0, st, w, nw, r, nr, s);
  else hipLaunchKernelGGL((mlp_bwd_layer_kernel<WM, WC, false>), grid, dim3(kWgThreads), 0, st, w, nw, r, nr, s);
}

// wc: the rows role's width class (mlp_bwd_layer_kernel's WC)
template <bool WM>
void launch_bwd1(int wc, bool rm, const WgradArgs& w, int nw, const MlpArgs& r, int nr, const SumJob& s, dim3 grid,
                 hipStream_t st) {
  switch (wc) {
    case 0: launch_bwd2<WM, 0>(false, w, nw, r, nr, s, grid, st); break;
    case 1: launch_bwd2<WM, 1>(rm, w, nw, r, nr, s, grid, st); break;
    case 2: launch_bwd2<WM, 2>(rm, w, nw, r, nr, s, grid, st); break;
    case 3: launch_bwd2<WM, 3>(rm, w, nw, r, nr, s, grid, st); break;
    default:  // the slim class has no A mask (mlp_slim_class)
      hipLaunchKernelGGL((mlp_bwd_layer_kernel<WM, 4, false>), grid, dim3(kWgThreads), 0, st, w, nw, r, nr, s);
      break;
  }
}

}  // namespace

extern "C" int tt_mlp_backward_layer(const tt_mlp_wgrad_job* w, const tt_mlp_rows_problem* r,
                                     const tt_mlp_wgrad_job* prev, tt_stream_t stream) {
  clear_error();
  const char* fn = "tt_mlp_backward_layer";
  TT_REQUIRE(w, "%s: NULL weight-gradient job", fn);
  WgradArgs wa;
  SumJob cur;
  if (int rc = wgrad_job_setup(fn, w, wa, cur)) return rc;
  MlpArgs ra{};
  int ncb = 0;
  const bool has_r = r != nullptr && r->M > 0;
  if (has_r) {
    if (int rc = rows_setup(fn, r->A, r->lda, r->amask, r->ldam, r->scale, r->M, r->K, r->img, r->N, r->bias, r->relu,
                            r->cmask, r->ldcm, r->C, r->ldc, ra, ncb))
      return rc;
    if (ra.G > 1) return fail(TT_ERR_UNSUPPORTED, "%s: input-gradient width %d > %d runs as tt_mlp_rows", fn, ra.N,
                              kMlpMaxCB * 128);
  }
  SumJob ps{};
  int64_t ns = 0;
  if (prev) {
    WgradArgs pa;
    if (int rc = wgrad_job_setup(fn, prev, pa, ps)) return rc;
    // the previous layer's partials are read while this layer's are written
    const char *p0 = static_cast<const char*>(prev->parts), *w0 = static_cast<const char*>(w->parts);
    const size_t pn = tt_mlp_wgrad_workspace_size(prev->p.M, prev->p.Ka, prev->p.N),
                 wn = tt_mlp_wgrad_workspace_size(w->p.M, w->p.Ka, w->p.N);
    TT_REQUIRE(p0 + pn <= w0 || w0 + wn <= p0, "%s: the previous layer's partials overlap this layer's", fn);
    ns = ceil_div(ps.len, 256);
  }
  const int nw = wa.S * wa.TI * wa.TJ;
  const int nr = has_r ? static_cast<int>(ceil_div(ra.M, kMlpBM)) : 0;
  const dim3 grid(static_cast<unsigned>(nw + nr + ns));
  hipStream_t st = to_stream(stream);
  const bool rm = has_r && ra.amask != nullptr;
  const int wc = !has_r ? 0 : (mlp_slim_class(ncb, rm, ra.N) ? 4 : ncb);
  if (wa.gmask) launch_bwd1<true>(wc, rm, wa, nw, ra, nr, ps, grid, st);
  else launch_bwd1<false>(wc, rm, wa, nw, ra, nr, ps, grid, st);
  TT_CHECK_LAUNCH();
  return TT_OK;
}

extern "C" int tt_mlp_wgrad_finish(const tt_mlp_wgrad_job* w, tt_stream_t stream) {
  clear_error();
  TT_REQUIRE(w, "tt_mlp_wgrad_finish: NULL job");
  WgradArgs wa;
  SumJob s;
  if (int rc = wgrad_job_setup("tt_mlp_wgrad_finish", w, wa, s)) return rc;
  hipLaunchKernelGGL(mlp_sum_parts_kernel, dim3(static_cast<unsigned>(ceil_div(s.len, 256))), dim3(1024), 0,
                     to_stream(stream), s.parts, s.S, s.len, s.out, s.ad);
  TT_CHECK_LAUNCH();
  return TT_OK;
}
