/*
 * tt.h — C ABI of libtt.so, the MI355X (gfx950) hot path of the two-tower
 * retrieval trainer and brute-force index.
 *
 * Every entry point is stream-ordered and asynchronous: it validates its
 * arguments on the host, enqueues HIP kernels on `stream` and returns.  No
 * entry point allocates device memory or synchronises; scratch comes from a
 * caller-owned workspace whose size is given by the matching *_workspace_size
 * query.  All pointers are device pointers unless stated otherwise; all
 * matrices are row-major with an explicit leading dimension (in elements).
 *
 * Return value: TT_OK (0) or a TT_ERR_* code; tt_last_error() returns a
 * thread-local message describing the last failure on the calling thread.
 *
 * Reference interfaces each entry point replaces are cited as
 * /root/reference/<file>:<line> (SelvinSelbaraju/hm-retrieval-two-tower).
 * The reference has no FFI: its "operator API" is the Keras layer/model
 * classes, so the citations name the TF op call sites.
 */
#ifndef TT_H_
#define TT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tt_stream_t; /* a hipStream_t; NULL selects the null stream */

enum {
  TT_OK = 0,
  TT_ERR_BAD_ARG = 1,     /* invalid shape / pointer / parameter            */
  TT_ERR_HIP = 2,         /* a HIP runtime call failed                      */
  TT_ERR_UNSUPPORTED = 3, /* valid request this build does not implement    */
  TT_ERR_WORKSPACE = 4    /* workspace missing or smaller than required     */
};

/* Library version string, e.g. "tt 0.1.0 gfx950". */
const char* tt_version(void);
/* Thread-local description of the last error ("" if none). */
const char* tt_last_error(void);

/* Measurement hook (no reference counterpart): the NEXT launch of `kernel`
 * issued by the calling thread is bracketed by hipEventRecord(ev_start) and
 * hipEventRecord(ev_stop) on its launch stream; the probe then disarms.  Lets
 * a benchmark time one kernel of a multi-launch entry point with HIP events
 * on the stream it runs on.  ev_start/ev_stop are hipEvent_t (NULL disarms). */
enum {
  TT_PROBE_INBATCH_ROWS = 0, /* inbatch_pass_kernel<D,0> (rows pass)        */
  TT_PROBE_INBATCH_COLS = 1, /* inbatch_pass_kernel<D,1> (cols pass)        */
  TT_PROBE_INDEX_SCREEN = 2, /* screen kernel of tt_bruteforce_search       */
  TT_PROBE_INDEX_FINALIZE = 3, /* finalize kernel of tt_bruteforce_search   */
  TT_PROBE_COUNT = 4
};
int tt_probe_arm(int32_t kernel, void* ev_start, void* ev_stop);
/* As tt_probe_arm, and the armed launch is issued `reps` (>= 1) times back to
 * back between the two events (in-batch passes only: they are idempotent), so
 * the per-launch time is (stop - start) / reps without one event pair per
 * launch.  Other kernels ignore reps. */
int tt_probe_arm_repeat(int32_t kernel, void* ev_start, void* ev_stop, int32_t reps);

/* ------------------------------------------------------------------------ *
 * K2+K3  Grouped embedding gather + concat.
 * Replaces InputLayer.call  (pkg/modelling/layers/input_layer.py:45-69):
 * numeric features copied first, then per categorical feature
 * Embedding(table)[ids] (input_layer.py:37-41,67), concatenated on the last
 * axis (input_layer.py:68).  One launch for all features; each segment
 * writes straight into its column range of `out`.
 * Out-of-range ids produce zero rows (TF GPU gather semantics).
 * ------------------------------------------------------------------------ */
#define TT_MAX_SEGMENTS 32

typedef struct {
  const float* table;   /* [num_rows, dim] fp32, or [batch] values if ids==NULL */
  const int32_t* ids;   /* [batch] row ids; NULL = numeric pass-through column  */
  int64_t num_rows;     /* rows of `table` (ignored for numeric columns)        */
  int32_t dim;          /* embedding size (1 for numeric columns)               */
  int32_t col_offset;   /* first column of this segment in `out`                */
} tt_gather_segment;

int tt_gather_grouped(const tt_gather_segment* segs, int32_t num_segs,
                      int64_t batch, float* out, int64_t out_stride,
                      tt_stream_t stream);

/* Several InputLayer.call's of one batch (e.g. the query and the candidate
 * tower, two_tower_model.py:65-92) in ONE launch: call i gathers its
 * `num_segs` segments into its own `out` [batch, out_stride].  At most
 * TT_MAX_SEGMENTS segments in total. */
typedef struct {
  const tt_gather_segment* segs;
  int32_t num_segs;
  float* out;
  int64_t out_stride;
} tt_gather_call;

int tt_gather_multi(const tt_gather_call* calls, int32_t num_calls,
                    int64_t batch, tt_stream_t stream);

/* Row-sharded tables (data parallel / SURVEY C5): the owner of a shard
 * answers row requests from every rank in one launch.  Request j reads row
 * rows[j] of tables[tags[j]] into out[j, 0:dim] (zeros for an invalid tag or
 * row).  All tables must share `dim`. */
typedef struct {
  const float* table;  /* [num_rows, dim] fp32 */
  int64_t num_rows;
} tt_row_table;

int tt_gather_tagged(const tt_row_table* tables, int32_t num_tables, int32_t dim,
                     const int32_t* tags, const int32_t* rows, int64_t n,
                     float* out, int64_t out_stride, tt_stream_t stream);

/* Request routing for row-sharded tables (no reference counterpart: the
 * reference trains on one CPU; this is the exchange the data-parallel step
 * needs).  Global row r of a sharded table lives on rank
 * r % world.  tt_route_requests deduplicates a rank's lookups into ONE
 * request list, owner-major (inside an owner: by tag, then row ascending; an
 * id outside its table becomes row -1, owned by rank world-1, sorted first):
 *   send [R, 2] int32 (global row, tag), counts [world] int64 (requests per
 *   owner, R = their sum, also written to *num_requests), idx [num_lookups,
 *   batch] int32 = the position in `send` of each lookup's request.
 * Capacity: send holds num_lookups*batch pairs.  tt_route_owner expands the
 * n requests an owner received (recv [n, 2]) into tags [n], local rows [n]
 * (gid / world, -1 if invalid) and per tag the local rows of that tag's
 * requests with -1 elsewhere (table_ids [num_tags, n]). */
typedef struct {
  const int32_t* ids; /* [batch] row ids of one lookup (one feature)        */
  int64_t num_rows;   /* rows of the (global) table it reads               */
  int32_t tag;        /* table index, 0..num_tags-1                         */
} tt_route_lookup;

size_t tt_route_workspace_size(int32_t num_lookups, int64_t batch, int32_t world,
                               int64_t max_rows, int32_t num_tags);
int tt_route_requests(const tt_route_lookup* lookups, int32_t num_lookups,
                      int64_t batch, int32_t world, int32_t num_tags,
                      int32_t* send, long long* counts, int32_t* num_requests,
                      int32_t* idx, void* workspace, size_t workspace_bytes,
                      tt_stream_t stream);
/* tt_route_requests plus the route's sorted order, so a sparse sum / update
 * keyed by the requests needs no second sort (tt_sparse_routed):
 *   order [num_lookups*batch] = the lookup (l*batch + b) at each sorted
 *   position (owner, tag, row ascending; a request's lookups in lookup
 *   order), grp_first / grp_last [world*num_tags] = the first / last sorted
 *   position of each (owner, tag) group (empty: 0 / -1).  Any of the three
 *   may be NULL (grp_first and grp_last together). */
int tt_route_requests_ordered(const tt_route_lookup* lookups, int32_t num_lookups,
                              int64_t batch, int32_t world, int32_t num_tags,
                              int32_t* send, long long* counts, int32_t* num_requests,
                              int32_t* idx, int32_t* order, int32_t* grp_first,
                              int32_t* grp_last, void* workspace,
                              size_t workspace_bytes, tt_stream_t stream);
int tt_route_owner(const int32_t* recv, int64_t n, int32_t world,
                   int32_t num_tags, int32_t* tags, int32_t* rows,
                   int32_t* table_ids, tt_stream_t stream);

/* Fixed-capacity routing (no host sync, graph-capturable): the compact
 * owner-major requests of tt_route_requests (send, counts on the device, idx
 * [num_lookups]) laid into `cap` slots per owner: request j of owner o at
 * slot o*cap + j of send_padded [world*cap, 2], unused slots (-1, -1) (an
 * owner answers them with zero rows and applies nothing); idx_padded
 * [num_lookups] = each lookup's slot.  Every exchange of the step then has
 * the split sizes [cap]*world.  cap = num_lookups never overflows; a smaller
 * cap drops an owner's requests past it, adds their number to *overflow
 * (optional, zero it first) and marks their lookups idx_padded = -1 - owner:
 * the lookup reads a zero row and contributes no gradient (the step reports
 * the overflow and the sharded trainer raises on it). */
int tt_route_pad(const int32_t* send, const long long* counts, const int32_t* idx,
                 int64_t num_lookups, int32_t world, int64_t cap,
                 int32_t* send_padded, int32_t* idx_padded, int32_t* overflow,
                 tt_stream_t stream);

/* The whole fixed-capacity route in one call: the outputs of
 * tt_route_requests_ordered (counts, optional order / grp_first / grp_last)
 * and tt_route_pad (send_padded, idx_padded, optional overflow), and at world
 * 1 optionally tt_route_owner's view of the slots (owner_tags / owner_rows
 * [cap], owner_table_ids [num_tags, cap]: at one rank the slots ARE the
 * owner's requests).  Up to 8192 lookups whose keys fit 32 bits run as ONE
 * workgroup launch (LDS radix sort + scan + slot writes; TT_ROUTE_FUSED=0
 * forces the multi-launch path); otherwise the three calls above.  Results
 * are identical either way.  Workspace: tt_route_fixed_workspace_size. */
size_t tt_route_fixed_workspace_size(int32_t num_lookups, int64_t batch, int32_t world,
                                     int64_t max_rows, int32_t num_tags);
int tt_route_fixed(const tt_route_lookup* lookups, int32_t num_lookups, int64_t batch,
                   int32_t world, int32_t num_tags, int64_t cap, int32_t* send_padded,
                   int32_t* idx_padded, long long* counts, int32_t* overflow,
                   int32_t* order, int32_t* grp_first, int32_t* grp_last,
                   int32_t* owner_tags, int32_t* owner_rows, int32_t* owner_table_ids,
                   void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* Opt-in fp32-faithful products: tt_inbatch_softmax_xent_loss's contract
 * (prepped = 0; loss may be NULL) with every score S_ij AND the softmax-
 * weighted sums P.V from bf16x3 products (x = hi + lo, both bf16: hi.hi +
 * hi.lo + lo.hi, fp32 accumulation — the reference's fp32 logits and
 * gradients, two_tower_model.py:92,124, to ~2^-16 relative) in both passes.
 * Accuracy at trained score magnitudes (|S| ~ 100), where the default bf16
 * operands drift to ~8e-3: asserted 1e-3 in dQ/dC and 1e-4 in loss against
 * fp64, measured <= 8.5e-6.
 * Three MFMAs where the default issues one, one workgroup per CU. */
size_t tt_inbatch_fused_x3_workspace_size(int64_t n, int32_t dim);
int tt_inbatch_softmax_xent_x3(const float* q, int64_t ldq, const float* c,
                               int64_t ldc, int64_t n, int32_t dim,
                               const float* logq, float* lse, float* row_loss,
                               float* dq, float* dc, float loss_scale,
                               float* loss, void* workspace,
                               size_t workspace_bytes, tt_stream_t stream);

/* tt_inbatch_xent_rows / tt_inbatch_xent_cols (K5+K6+K7 below: same
 * arguments, checks and error codes; dq, row_loss and logq optional as
 * there) with the same bf16x3 products and the accuracy stated above: the
 * entries every rank of the global-negatives step runs in this mode.  A
 * workspace of their own size (the bf16 images plus both operands' residual
 * planes). */
size_t tt_inbatch_x3_workspace_size(int64_t n_rows, int64_t n_cols, int32_t dim);
int tt_inbatch_xent_rows_x3(const float* q, int64_t ldq, int64_t n_rows,
                            const float* c, int64_t ldc, int64_t n_cols,
                            int32_t dim, const float* logq, int64_t pos_offset,
                            float* lse, float* row_loss, float* dq,
                            void* workspace, size_t workspace_bytes,
                            tt_stream_t stream);
int tt_inbatch_xent_cols_x3(const float* q, int64_t ldq, int64_t n_rows,
                            const float* lse, const float* row_loss,
                            const float* c, int64_t ldc, int64_t n_cols,
                            int32_t dim, const float* logq, int64_t pos_offset,
                            float* dc, void* workspace, size_t workspace_bytes,
                            tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K8+K9  Sparse optimizer step on embedding tables.
 * Replaces the legacy Keras optimizer's sparse path reached from
 * TwoTowerModel.train_step -> optimizer.minimize
 * (pkg/modelling/models/two_tower_model.py:124, optimizer_factory.py:15-18):
 * _deduplicate_indexed_slices (Unique + UnsortedSegmentSum, duplicates summed
 * in batch order) followed by ResourceSparseApplyAdagradV2 /
 * the legacy Adam sparse update.
 *
 * A table may be looked up by several features of one batch (the reference's
 * duplicated `product_type_name`, main.py:57-68 with input_layer.py:31,66-67):
 * list each lookup as a source; the index list is the concatenation of the
 * sources' ids in source order and duplicates are summed in that order.
 * ------------------------------------------------------------------------ */
#define TT_MAX_SOURCES 4

typedef struct {
  float* table;        /* [num_rows, dim] parameters, updated in place          */
  float* slot0;        /* Adagrad accumulator / Adam first moment [num_rows,dim] */
  float* slot1;        /* Adam second moment, NULL for Adagrad                  */
  int64_t num_rows;
  int32_t dim;
  int32_t num_sources; /* 1..TT_MAX_SOURCES                                     */
  const int32_t* ids[TT_MAX_SOURCES];      /* [batch] row ids per source         */
  int32_t grad_col_offset[TT_MAX_SOURCES]; /* column of the source's slice in grad */
  /* Optional per-table gradient buffer: when non-NULL, this table's sources
   * read rows b of grad + b*grad_ld (+ grad_col_offset[s]) instead of the
   * call's grad / grad_stride — so ONE call (one sort) updates the tables of
   * both towers, whose input gradients are separate buffers.                */
  const float* grad;
  int64_t grad_ld;
} tt_sparse_table;

size_t tt_sparse_workspace_size(const tt_sparse_table* tables, int32_t num_tables,
                                int64_t batch);

/* acc += g*g ; w -= lr*g / (sqrt(acc) + epsilon) on every touched row, g the
 * duplicate-summed gradient (TF ResourceSparseApplyAdagradV2 CPU kernel). */
int tt_sparse_adagrad(const tt_sparse_table* tables, int32_t num_tables,
                      int64_t batch, const float* grad, int64_t grad_stride,
                      float lr, float epsilon, void* workspace,
                      size_t workspace_bytes, tt_stream_t stream);

/* The same update in two stages.  tt_sparse_sort builds and sorts the
 * (table | row id, lookup) keys — it reads only the ids, so it can run early
 * on a side stream, overlapped with the forward/backward compute;
 * tt_sparse_adagrad_sorted then does the segmented sums and the apply in ONE
 * launch: a segment longer than a 32-lookup block is joined inside it by the
 * last of its blocks to arrive at the segment's counter (one counter per
 * block in the workspace, zeroed by the sort stage and again by the joiner,
 * so the apply may be repeated on one sort); no block waits for another.
 * Both calls must see the same tables (<= 16), batch and workspace, in that
 * order.  Results are identical to tt_sparse_adagrad. */
int tt_sparse_sort(const tt_sparse_table* tables, int32_t num_tables,
                   int64_t batch, void* workspace, size_t workspace_bytes,
                   tt_stream_t stream);
int tt_sparse_adagrad_sorted(const tt_sparse_table* tables, int32_t num_tables,
                             int64_t batch, const float* grad, int64_t grad_stride,
                             float lr, float epsilon, void* workspace,
                             size_t workspace_bytes, tt_stream_t stream);

/* Adagrad on DISTINCT rows (no sort, no duplicate sums): slot j (< n) applies
 * grad row j (grad + j*grad_ld, tables[*].dim columns) to row rows[j] of
 * tables[tags[j]] (tags[j] < 0 or a row outside the table: nothing).  Every
 * (tag, row) must occur at most once — e.g. the requests a one-rank owner
 * receives from tt_route_requests.  Bit-identical to tt_sparse_adagrad on
 * those rows.  Tables share one dim; ids / grad_col_offset are ignored. */
int tt_sparse_adagrad_rows(const tt_sparse_table* tables, int32_t num_tables,
                           const int32_t* tags, const int32_t* rows, int64_t n,
                           const float* grad, int64_t grad_ld, float lr,
                           float epsilon, tt_stream_t stream);

/* The sparse calls never fault on a mismatched workspace: the sort stage
 * stamps the first 256 bytes of the workspace with a fingerprint of the
 * lookups it sorted, and the apply launch (of every sparse entry point above
 * and below) checks it before touching a table.  A presorted apply that finds
 * another call's keys (or a sorted lookup pointing outside the call's
 * gradient) applies nothing from the affected blocks (nor from a longer
 * segment they hold a piece of) and records the error in the header.  tt_sparse_status synchronises `stream`, returns
 * TT_ERR_BAD_ARG (message in tt_last_error) if an error was recorded since
 * the last check, and clears it.  A fresh workspace should start zeroed. */
int tt_sparse_status(void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* Legacy Keras Adam sparse path: m,v decayed over the WHOLE slot, the scaled
 * duplicate-summed gradient scatter-added, then the WHOLE table updated with
 * lr_t = lr*sqrt(1-beta2^step)/(1-beta1^step) (step is 1-based). */
int tt_sparse_adam(const tt_sparse_table* tables, int32_t num_tables,
                   int64_t batch, const float* grad, int64_t grad_stride,
                   float lr, float beta1, float beta2, float epsilon,
                   int64_t step, void* workspace, size_t workspace_bytes,
                   tt_stream_t stream);

/* Dense gradient of each table from its lookups: every touched row of
 * `table` (a zero-filled [num_rows, dim] gradient buffer; slots unused) is
 * set to its duplicate-summed gradient, in the same summation order as
 * tt_sparse_adagrad.  Used by data-parallel training to all-reduce the
 * gradients of small replicated tables. */
int tt_sparse_scatter_sum(const tt_sparse_table* tables, int32_t num_tables,
                          int64_t batch, const float* grad, int64_t grad_stride,
                          void* workspace, size_t workspace_bytes,
                          tt_stream_t stream);

/* The per-request sums / updates of routed lookups, keyed by the route's own
 * sort (tt_route_requests_ordered + tt_route_pad): no second sort.  Table i
 * lists its lookups as sources (ids = the lookups' slots, idx_padded rows, in
 * lookup order) exactly as for tt_sparse_scatter_sum; `rs` maps every routed
 * lookup l to (tag, table, source).  Each table must take the lookups of one
 * tag.  Keys: the lookup's slot, or slot_row[slot] when slot_row is given
 * (e.g. tt_route_owner's local rows at world 1; -1 = nothing).  op 0: the
 * duplicate-summed rows written into each table (tt_sparse_scatter_sum);
 * op 1: Adagrad on them (tt_sparse_adagrad, lr / epsilon).  Results equal
 * those calls' on the same keys whenever the route lists each table's
 * lookups in the order that call sorts them (world 1: always). */
#define TT_ROUTE_MAX_LOOKUPS 32
typedef struct {
  const int32_t* order;     /* [num_lookups*batch], tt_route_requests_ordered */
  const int32_t* grp_first; /* [world*num_tags]                              */
  const int32_t* grp_last;
  const int32_t* slot;      /* [num_lookups*batch] slot of each lookup (idx_padded) */
  const int32_t* slot_row;  /* optional [world*cap]: key = slot_row[slot]     */
  int64_t cap;
  int32_t world;
  int32_t num_tags;
  int32_t num_lookups;
  int32_t lookup_tag[TT_ROUTE_MAX_LOOKUPS];
  int32_t lookup_table[TT_ROUTE_MAX_LOOKUPS];
  int32_t lookup_source[TT_ROUTE_MAX_LOOKUPS];
} tt_route_sorted;

int tt_sparse_routed(const tt_sparse_table* tables, int32_t num_tables, int64_t batch,
                     const float* grad, int64_t grad_stride, const tt_route_sorted* rs,
                     int32_t op, float lr, float epsilon, void* workspace,
                     size_t workspace_bytes, tt_stream_t stream);

/* tt_sparse_scatter_sum's block launch (sums and joins) on keys tt_sparse_sort sorted
 * earlier (same tables, batch and workspace; the sort reads only the ids and
 * accepts tables without slots): the sort can run beside other work. */
int tt_sparse_scatter_sum_sorted(const tt_sparse_table* tables, int32_t num_tables,
                                 int64_t batch, const float* grad, int64_t grad_stride,
                                 void* workspace, size_t workspace_bytes,
                                 tt_stream_t stream);

/* Dedup only (K8), for parity checks: writes the U distinct ids of
 * ids[0..n) in ascending order, the per-id gradient sums [U, dim] (rows of
 * `grad` summed in index order) and U (device int32).  Capacity n rows. */
size_t tt_dedup_workspace_size(int64_t n, int32_t dim);
int tt_dedup_sum(const int32_t* ids, int64_t n, int64_t num_rows,
                 const float* grad, int64_t grad_stride, int32_t dim,
                 int32_t* unique_ids, float* summed, int32_t* num_unique,
                 void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* K10  Dense optimizer steps on a flat parameter buffer (tower MLP weights).
 * ResourceApplyAdagradV2 / ResourceApplyAdam (optimizer_factory.py:15-18). */
int tt_dense_adagrad(float* param, float* accum, const float* grad, int64_t n,
                     float lr, float epsilon, tt_stream_t stream);
/* tt_dense_adagrad on up to 8 buffers in one launch (bit-identical to one
 * call per buffer). */
typedef struct {
  float* param;
  float* accum;
  const float* grad;
  int64_t n;
} tt_dense_job;
int tt_dense_adagrad_many(const tt_dense_job* jobs, int32_t num_jobs, float lr, float epsilon,
                          tt_stream_t stream);
int tt_dense_adam(float* param, float* m, float* v, const float* grad,
                  int64_t n, float lr, float beta1, float beta2, float epsilon,
                  int64_t step, tt_stream_t stream);

/* Adam with the step count in device memory, for a captured train step.
 *
 * Adam depends on the step t only through two fp32 coefficients, which
 * tt_dense_adam and tt_sparse_adam compute on the host with powf:
 *   alpha = (lr * sqrt(1 - beta2^t)) / (1 - beta1^t)      (dense, TF ApplyAdamOp)
 *   lr_t  = lr * (sqrt(1 - beta2^t) / (1 - beta1^t))      (sparse, legacy Keras)
 * The device's powf is not the host's, so the _dev entries below never compute
 * them: the host fills a table of both, one entry per step, with the same
 * function the two entries above use, and a one-thread launch moves a device
 * clock one step along it.  The table is finite because the coefficients
 * saturate: once beta^t <= 2^-25, 1 - beta^t == 1 in fp32 and both equal lr
 * for every later step (the host's powers are monotone in t over the 2^22 steps
 * a table may hold), so the clock clamps its index at the table's last entry.
 *
 * tt_adam_coef_len: L, the first step at which 1 - beta^t == 1 for both betas
 * as that host function evaluates them (found by evaluating it step by step,
 * not from a formula: the fp32 value of beta moves L); from step L on both
 * coefficients are lr.  0 when a beta is outside [0, 1) (NaN included) or L
 * would exceed 2^22.  beta1 = beta2 = 0 gives 1.  (0.9, 0.999) gives 17321.
 * tt_adam_coef_fill: HOST arrays alpha[len], lr_t[len]; entry t-1 holds step
 * t's pair, bit for bit what tt_dense_adam / tt_sparse_adam use at `step` = t.
 * TT_ERR_BAD_ARG for a non-finite lr, a beta outside [0, 1), len < 1 or NULL. */
int64_t tt_adam_coef_len(float beta1, float beta2);
int tt_adam_coef_fill(float lr, float beta1, float beta2, int64_t len, float* alpha, float* lr_t);

/* The device clock: 16 bytes of device memory, 8-byte aligned.
 *   offset 0  int64  step   steps taken so far (the last advance made it step t)
 *   offset 8  float  alpha  step t's dense coefficient
 *   offset 12 float  lr_t   step t's sparse coefficient
 * The host sets `step` (e.g. to the optimizer's iteration count) before the
 * first advance; alpha / lr_t are valid after it. */
typedef struct {
  int64_t step;
  float alpha;
  float lr_t;
} tt_adam_clock;

/* One launch of one thread, plain stores: step += 1, then (alpha, lr_t) =
 * entry min(step, len) - 1 of the DEVICE copies of the filled tables (entry 0
 * for a step below 1).  It synchronises with nothing and can be captured:
 * every replay advances the clock, as tt_mixed_candidates' step word does.
 * Kernels ordered after it on the stream read the new pair. */
int tt_adam_clock_advance(tt_adam_clock* clock, const float* alpha_tab, const float* lr_t_tab,
                          int64_t len, tt_stream_t stream);

/* tt_dense_adam on up to 8 buffers in ONE launch (a grid-stride loop over
 * their concatenation), alpha read from *clock on the device: bit-identical
 * to one tt_dense_adam per buffer at step clock->step with the lr the table
 * was filled for.  n may be 0 (pointers then unused). */
typedef struct {
  float* param;
  float* m;
  float* v;
  const float* grad;
  int64_t n;
} tt_dense_adam_job;
int tt_dense_adam_many_dev(const tt_dense_adam_job* jobs, int32_t num_jobs, float beta1, float beta2,
                           float epsilon, const tt_adam_clock* clock, tt_stream_t stream);

/* tt_sparse_adam with lr_t read from *clock on the device: the same three
 * stages in the same order (whole slots decayed, tt_sparse_adam's scatter,
 * whole tables updated), bit-identical to it at step clock->step.  The decay
 * of ALL tables is one launch and so is the update (16 tables a launch; 16-byte
 * accesses for a table whose three buffers are 16-byte aligned), where
 * tt_sparse_adam takes one of each per table.  Same validation, workspace
 * (tt_sparse_workspace_size) and fingerprint checks; batch == 0 still decays
 * and updates. */
int tt_sparse_adam_dev(const tt_sparse_table* tables, int32_t num_tables,
                       int64_t batch, const float* grad, int64_t grad_stride,
                       float beta1, float beta2, float epsilon,
                       const tt_adam_clock* clock, void* workspace,
                       size_t workspace_bytes, tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K5+K6+K7  Fused in-batch scores, logQ correction and softmax
 * cross-entropy (reduction SUM) with its gradient.
 * Replaces TwoTowerModel.call's matmul (two_tower_model.py:92),
 * LogQCorrection.__call__ (logq_correction.py:66-71), the eye-label
 * CategoricalCrossentropy(from_logits, SUM) (two_tower_model.py:119-122,
 * runner.py:78-83) and the tape gradient of that chain.
 *
 *   S'[i][j] = q_i . c_j - logq[j]
 *   loss_i   = logsumexp_j S'[i][j] - S'[i][pos(i)]
 *   dq_i     = sum_j softmax_j(S'[i]) c_j - c_pos(i)
 *   dc_j     = sum_i softmax(S'[i])_j q_i - q_pos^-1(j)
 *
 * Arithmetic contract: the NEGATIVE pairs are scored with bf16 (RNE)
 * operands and fp32 accumulation, and their exp weights enter the P.C /
 * P^T.Q products rounded to bf16 (relative to a power-of-two scale, so the
 * rounding is reproducible: oracle.inbatch_softmax_xent_bf16); the positive
 * pair is scored in fp32 and enters through the exact 1 - P_pos
 * (row_loss = softplus(lse_neg - pos), dq = (1 - P_pos)(mean_neg c - c_pos)),
 * so there is no P - I cancellation.  fp32 outputs; the [rows, cols]
 * score matrix is never materialised.  Rows and columns are given
 * separately so a rank can score its local rows against all-gathered
 * columns (global in-batch negatives): the positive column of local row i
 * is i + pos_offset, the positive row of local column j is j + pos_offset.
 * ------------------------------------------------------------------------ */
size_t tt_inbatch_workspace_size(int64_t n_rows, int64_t n_cols, int32_t dim);

/* Row pass: lse[i], row_loss[i] = lse[i] - S'[i][i+pos_offset], and (if dq
 * != NULL) dq [n_rows, dim] (ld = dim). */
int tt_inbatch_xent_rows(const float* q, int64_t ldq, int64_t n_rows,
                         const float* c, int64_t ldc, int64_t n_cols,
                         int32_t dim, const float* logq, int64_t pos_offset,
                         float* lse, float* row_loss, float* dq,
                         void* workspace, size_t workspace_bytes,
                         tt_stream_t stream);

/* Column pass: dc [n_cols, dim] (ld = dim) from all rows' q, lse and
 * row_loss (the rows pass's outputs; 1 - P_pos = -expm1(-row_loss).
 * row_loss may be NULL: then 1 - P_pos comes from lse and the fp32 positive
 * score, which cancels when the positive dominates). */
int tt_inbatch_xent_cols(const float* q, int64_t ldq, int64_t n_rows,
                         const float* lse, const float* row_loss,
                         const float* c, int64_t ldc, int64_t n_cols,
                         int32_t dim, const float* logq, int64_t pos_offset,
                         float* dc, void* workspace, size_t workspace_bytes,
                         tt_stream_t stream);

/* Single-device form of the two passes above (rows = cols = the batch,
 * positive of row i is column i): one shared bf16 preparation of q and c,
 * outputs lse, row_loss [n], dq, dc [n, dim] (ld = dim). */
size_t tt_inbatch_fused_workspace_size(int64_t n, int32_t dim);
int tt_inbatch_softmax_xent(const float* q, int64_t ldq, const float* c,
                            int64_t ldc, int64_t n, int32_t dim,
                            const float* logq, float* lse, float* row_loss,
                            float* dq, float* dc, void* workspace,
                            size_t workspace_bytes, tt_stream_t stream);

/* The same entry split at its preparation, so each tower's bf16 copy can be
 * made on the stream that produced that tower's output (the two towers that
 * TwoTowerModel.train_step runs, pkg/modelling/models/two_tower_model.py:
 * 111, finish on separate streams): tt_inbatch_prep with operand 0
 * prepares q, with operand 1 prepares c and the logQ bias vectors (logq may
 * be NULL, as above); both must be ordered before
 * tt_inbatch_softmax_xent_prepped on the same workspace, which then runs the
 * passes only.  Results are bit-identical to tt_inbatch_softmax_xent. */
int tt_inbatch_prep(const float* x, int64_t ldx, int64_t n, int32_t dim,
                    int32_t operand, const float* logq, void* workspace,
                    size_t workspace_bytes, tt_stream_t stream);
int tt_inbatch_softmax_xent_prepped(const float* q, int64_t ldq,
                                    const float* c, int64_t ldc, int64_t n,
                                    int32_t dim, const float* logq,
                                    float* lse, float* row_loss, float* dq,
                                    float* dc, void* workspace,
                                    size_t workspace_bytes,
                                    tt_stream_t stream);

/* tt_inbatch_softmax_xent (prepped = 0) or tt_inbatch_softmax_xent_prepped
 * (prepped = 1), also writing the step's loss *loss = loss_scale *
 * sum(row_loss) (the reference's SUM reduction, two_tower_model.py:122,
 * runner.py:78-83): one extra workgroup of the last launch sums the row
 * losses in tt_sum's order, so the value equals a tt_sum call bit for bit
 * without its launch. */
int tt_inbatch_softmax_xent_loss(const float* q, int64_t ldq, const float* c,
                                 int64_t ldc, int64_t n, int32_t dim,
                                 const float* logq, float* lse,
                                 float* row_loss, float* dq, float* dc,
                                 float loss_scale, float* loss,
                                 int32_t prepped, void* workspace,
                                 size_t workspace_bytes, tt_stream_t stream);

/* Opt-in removal of accidental hits (duplicate candidates in the batch;
 * TensorFlow Recommenders' remove_accidental_hits).  The reference has no
 * such option (two_tower_model.py:113-124 takes every other column as a
 * negative): these entries depart from its loss, the entries above do not
 * change.  With row_ids[i] / col_ids[j] the int32 candidate ids of row i and
 * column j:
 *
 *   S'[i][j] = q_i . c_j - logq[j]   for j == pos(i), or col_ids[j] != row_ids[i]
 *   S'[i][j] = -inf                  for j != pos(i) and col_ids[j] == row_ids[i]
 *
 * and loss_i, dq_i, dc_j as above over this S'.  A masked pair has weight 0
 * in the rows pass (nothing to lse_i or dq_i) and in the cols pass (nothing
 * to dc_j); the mask is the score accumulator's initial value inside the
 * pass kernel (subtracting the duplicates' terms from lse afterwards would
 * cancel: they equal the positive's).  The positive pair is excluded by
 * position and added in fp32 exactly as above, whatever its ids say.  A row
 * whose every other column is a hit has loss 0 and dq row 0 exactly and adds
 * nothing to any dc.  Ids are compared for equality only: all
 * out-of-vocabulary rows (id 0) count as one candidate.  With pairwise
 * distinct ids the results equal the plain entries' bit for bit.
 *
 * x3 != 0: the bf16x3 products of tt_inbatch_softmax_xent_x3; otherwise the
 * bf16 contract of K5+K6+K7.  Arguments, checks and error codes otherwise as
 * the plain entries'; NULL ids are TT_ERR_BAD_ARG.  The workspaces are the
 * plain ones plus the padded id vectors.  There is no split-preparation
 * (tt_inbatch_prep) form. */
size_t tt_inbatch_hits_workspace_size(int64_t n_rows, int64_t n_cols,
                                      int32_t dim, int32_t x3);
int tt_inbatch_xent_rows_hits(const float* q, int64_t ldq, int64_t n_rows,
                              const float* c, int64_t ldc, int64_t n_cols,
                              int32_t dim, const float* logq,
                              int64_t pos_offset, const int32_t* row_ids,
                              const int32_t* col_ids, int32_t x3, float* lse,
                              float* row_loss, float* dq, void* workspace,
                              size_t workspace_bytes, tt_stream_t stream);
int tt_inbatch_xent_cols_hits(const float* q, int64_t ldq, int64_t n_rows,
                              const float* lse, const float* row_loss,
                              const float* c, int64_t ldc, int64_t n_cols,
                              int32_t dim, const float* logq,
                              int64_t pos_offset, const int32_t* row_ids,
                              const int32_t* col_ids, int32_t x3, float* dc,
                              void* workspace, size_t workspace_bytes,
                              tt_stream_t stream);
/* Single device (rows = cols = the batch, ids [n] serve both), with
 * tt_inbatch_softmax_xent_loss's in-launch *loss = loss_scale *
 * sum(row_loss) (loss may be NULL). */
size_t tt_inbatch_fused_hits_workspace_size(int64_t n, int32_t dim, int32_t x3);
int tt_inbatch_softmax_xent_hits(const float* q, int64_t ldq, const float* c,
                                 int64_t ldc, int64_t n, int32_t dim,
                                 const float* logq, const int32_t* ids,
                                 int32_t x3, float* lse, float* row_loss,
                                 float* dq, float* dc, float loss_scale,
                                 float* loss, void* workspace,
                                 size_t workspace_bytes, tt_stream_t stream);

/* Opt-in hard-negative mining (TensorFlow Recommenders' Retrieval task,
 * num_hard_negatives = K): of each row's negatives only the K with the
 * largest logits enter the cross-entropy.  The reference has no such option;
 * the entries above do not change.  Order as in TFRS: temperature (applied
 * before the loss), logQ, accidental hits, then hard negatives.
 *
 * S'[i][j] = q_i . c_j - logq[j] is the score the pass kernels form, in
 * either arithmetic (bf16 operands, or the bf16x3 products for x3 != 0), and
 * -inf on an accidental hit when ids are given.  For k >= 1 and each row i,
 * over the row's negatives j != pos(i) (hits included, as -inf):
 *
 *   a >= b      the k-th and (k+1)-th largest S'[i][j]
 *   thr[i]      = fl32(0.5 a + 0.5 b); if that rounds to b while a > b: a
 *   thr[i]      = -inf if the row has <= k negatives, or b = -inf
 *   (i, j) kept iff S'[i][j] >= thr[i]
 *
 * TIES: every negative that ties the k-th value is kept, so a row may keep
 * more than k.  This is the one departure from tf.math.top_k, which breaks
 * ties by index and keeps exactly k.
 *
 * A dropped pair has weight 0 in lse_i, dq_i and dc_j, exactly like a masked
 * accidental hit (its score becomes -inf after the score MFMAs).  The
 * positive is always kept and enters in fp32 exactly as in the plain entries.
 *
 * Why the midpoint: under x3 the rows pass streams c and the cols pass
 * streams q, so the two cross products hi.lo / lo.hi are added in different
 * orders and one S'[i][j] can differ in its last bits between the passes.  A
 * threshold inside the gap (a, b) gives both passes the same kept set
 * whenever that difference is below half the gap.  With bf16 operands the
 * products are exact and both passes add them in the same k order: the bits
 * agree.
 *
 * tt_inbatch_hard_threshold computes thr [n_rows] from the rows pass's own
 * MFMA sequence (same operand roles, k order and accumulator start), so its
 * S' is the rows pass's bit for bit.  It is exact and deterministic (an
 * 8-bit-digit radix select on the order-preserving integer key of S', integer
 * histograms only), puts no cap on k, and synchronises with nothing: it
 * captures into a graph.  k < 1 is TT_ERR_BAD_ARG.
 *
 * Invariants: with k >= the number of negatives, or thr all -inf, every
 * output of the _hard entries equals the corresponding plain, x3 or hits
 * entry's bit for bit.  Sample weights (tt_inbatch_weight_rows) compose as
 * before: select, rows, fold, cols.
 *
 * Arguments, checks, error codes and the x3 flag as the _hits entries';
 * row_ids / col_ids (ids for the fused form) may both be NULL: no hits are
 * removed.  The rows form takes thr [n_rows]; the cols form takes thr of all
 * n_rows rows, as it takes lse.  The fused form (single device: one
 * preparation, then select, rows, cols) returns thr [n] to the caller and
 * writes the in-launch *loss (loss may be NULL).  The workspaces are the
 * _hits ones plus a padded threshold vector. */
size_t tt_inbatch_hard_workspace_size(int64_t n_rows, int64_t n_cols,
                                      int32_t dim, int32_t x3);
int tt_inbatch_hard_threshold(const float* q, int64_t ldq, int64_t n_rows,
                              const float* c, int64_t ldc, int64_t n_cols,
                              int32_t dim, const float* logq,
                              int64_t pos_offset, const int32_t* row_ids,
                              const int32_t* col_ids, int32_t x3, int64_t k,
                              float* thr, void* workspace,
                              size_t workspace_bytes, tt_stream_t stream);
int tt_inbatch_xent_rows_hard(const float* q, int64_t ldq, int64_t n_rows,
                              const float* c, int64_t ldc, int64_t n_cols,
                              int32_t dim, const float* logq,
                              int64_t pos_offset, const int32_t* row_ids,
                              const int32_t* col_ids, int32_t x3,
                              const float* thr, float* lse, float* row_loss,
                              float* dq, void* workspace,
                              size_t workspace_bytes, tt_stream_t stream);
int tt_inbatch_xent_cols_hard(const float* q, int64_t ldq, int64_t n_rows,
                              const float* lse, const float* row_loss,
                              const float* c, int64_t ldc, int64_t n_cols,
                              int32_t dim, const float* logq,
                              int64_t pos_offset, const int32_t* row_ids,
                              const int32_t* col_ids, int32_t x3,
                              const float* thr, float* dc, void* workspace,
                              size_t workspace_bytes, tt_stream_t stream);
size_t tt_inbatch_fused_hard_workspace_size(int64_t n, int32_t dim, int32_t x3);
int tt_inbatch_softmax_xent_hard(const float* q, int64_t ldq, const float* c,
                                 int64_t ldc, int64_t n, int32_t dim,
                                 const float* logq, const int32_t* ids,
                                 int32_t x3, int64_t k, float* lse,
                                 float* row_loss, float* dq, float* dc,
                                 float* thr, float loss_scale, float* loss,
                                 void* workspace, size_t workspace_bytes,
                                 tt_stream_t stream);

/* Opt-in mixed negative sampling (Yang et al., "Mixed Negative Sampling for
 * Learning Two-tower Neural Networks in Recommendations", 2020): the columns
 * are the batch's candidates followed by extra candidates, drawn from the
 * whole catalogue (tt_mixed_candidates), that are negatives of every row.
 * The reference has no such option; the entries above do not change.
 *
 * The rows entries and tt_inbatch_hard_threshold take n_cols > n_rows as they
 * are.  tt_inbatch_xent_cols_mixed is tt_inbatch_xent_cols_hard without the
 * rule that every column has a positive row: column j's positive is row
 * j + pos_offset when that lies in [0, n_rows); otherwise it has none and
 *
 *   dc_j = exp(-logq[j]) * sum_i p_ij q_i
 *
 * with no positive term and no read of q / lse / row_loss outside [0, n_rows).
 * row_ids / col_ids (both or neither) and thr may each be NULL: no hits
 * removed / no mining; x3 as everywhere.  With n_cols + pos_offset <= n_rows
 * and pos_offset >= 0 every output equals the _cols, _cols_x3, _cols_hits or
 * _cols_hard entry's bit for bit.  Sample weights compose as before: (select,)
 * rows, tt_inbatch_weight_rows, tt_inbatch_xent_cols_mixed.
 *
 * tt_inbatch_softmax_xent_mixed is the fused single-device form: q [n] rows
 * against c [n + m] columns, row i's positive column i, columns [n, n + m)
 * negatives of every row; logq and ids (either may be NULL) have n + m
 * entries, ids[i] being row i's id too; k = 0: no mining, k >= 1: as
 * tt_inbatch_softmax_xent_hard (thr [n] returned, NULL allowed for k = 0).
 * One preparation of each operand, then (select,) rows, cols and the
 * in-launch *loss (may be NULL).  lse, row_loss, dq (and thr) equal the rows
 * (and threshold) entries called at n_cols = n + m bit for bit; with m = 0
 * every output equals the square fused entry's bit for bit. */
size_t tt_inbatch_mixed_workspace_size(int64_t n_rows, int64_t n_cols,
                                       int32_t dim, int32_t x3);
int tt_inbatch_xent_cols_mixed(const float* q, int64_t ldq, int64_t n_rows,
                               const float* lse, const float* row_loss,
                               const float* c, int64_t ldc, int64_t n_cols,
                               int32_t dim, const float* logq,
                               int64_t pos_offset, const int32_t* row_ids,
                               const int32_t* col_ids, int32_t x3,
                               const float* thr, float* dc, void* workspace,
                               size_t workspace_bytes, tt_stream_t stream);
size_t tt_inbatch_fused_mixed_workspace_size(int64_t n, int64_t m, int32_t dim,
                                             int32_t x3);
int tt_inbatch_softmax_xent_mixed(const float* q, int64_t ldq, int64_t n,
                                  const float* c, int64_t ldc, int64_t m,
                                  int32_t dim, const float* logq,
                                  const int32_t* ids, int32_t x3, int64_t k,
                                  float* lse, float* row_loss, float* dq,
                                  float* dc, float* thr, float loss_scale,
                                  float* loss, void* workspace,
                                  size_t workspace_bytes, tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K11+K12  Brute-force scoring with fused top-K.
 * Replaces BruteForceIndex.call (pkg/modelling/indices/brute_force.py:76-81):
 * matmul(queries, candidates^T) then tf.math.top_k(k) (sorted descending,
 * ties -> lower index).  A bf16 MFMA screen keeps, per query, the scores
 * above a sampled rank estimate; the finalize certifies that list against
 * the bf16 error bound (or answers the query by an exact scan), rescores it
 * in fp32 as a k-ordered fmaf chain and returns the exact top-k.  Indices
 * are candidate positions + index_offset (the global offset of a shard).
 * ------------------------------------------------------------------------ */
/* Bytes of a prepared candidate image: 64-B header (sizes, max row norms),
 * bf16 copy [n_pad, D], then per row (|bf16(c)|_2, |c - bf16(c)|_2) for the
 * finalize's per-row screen bound. */
size_t tt_bruteforce_index_bytes(int64_t n_cand, int32_t dim);
int tt_bruteforce_build(const float* cand, int64_t ldc, int64_t n_cand,
                        int32_t dim, void* index, size_t index_bytes,
                        tt_stream_t stream);
size_t tt_bruteforce_workspace_size(int64_t n_queries, int64_t n_cand,
                                    int32_t dim, int32_t k);
/* Host-only: dynamic LDS bytes a search at this k asks of one workgroup, for
 * the finalize (which = 0) or the exact fallback (which = 1); at most 163840
 * for every k in [1, 4000].  0: k or which out of range. */
size_t tt_bruteforce_lds_bytes(int32_t k, int32_t which);
int tt_bruteforce_search(const void* index, const float* cand, int64_t ldc,
                         int64_t n_cand, int32_t dim, const float* queries,
                         int64_t ldq, int64_t n_queries, int32_t k,
                         int64_t index_offset, float* out_scores,
                         int32_t* out_idx, void* workspace,
                         size_t workspace_bytes, tt_stream_t stream);

/* Candidate-sharded two-phase search (ShardedBruteForceIndex).
 * Replaces the same BruteForceIndex.call (brute_force.py:76-83) with the
 * candidate rows split over G ranks, each holding only its rows:
 *  1. tt_bruteforce_shard_screen on the rank's rows: bf16 screen + the
 *     finalize's select; kth_lb[q] = a lower bound on the k-th largest exact
 *     score of these rows (-inf when the query's certificate failed);
 *  2. the caller all-reduces kth_lb with MAX over the ranks: floor[q] bounds
 *     the GLOBAL k-th exact score from below;
 *  3. tt_bruteforce_shard_finalize: rescoring of the screened entries that
 *     can still reach floor, the shard's exact top-k of them with global
 *     indices (index_offset = the shard's first global row), padded with
 *     (-inf, INT32_MAX) past the survivors; failed certificates are scanned
 *     exactly over the shard.  Merging the G lists (tt_topk_merge) gives the
 *     exact global top-k.
 * Queries go in chunks of n_queries <= plan_queries; every call pair of one
 * search passes the same plan_queries, which must be equal on every rank
 * (tt_bruteforce_shard_chunk(total, n_g, ...) is rank g's recommendation: take
 * the minimum over the ranks) and the workspace is sized for it
 * (tt_bruteforce_shard_workspace_size(plan_queries, n_g, ...)).  A screen /
 * finalize pair of one chunk shares the workspace. */
int64_t tt_bruteforce_shard_chunk(int64_t n_queries, int64_t n_cand,
                                  int32_t dim, int32_t k);
size_t tt_bruteforce_shard_workspace_size(int64_t plan_queries, int64_t n_cand,
                                          int32_t dim, int32_t k);
int tt_bruteforce_shard_screen(const void* index, int64_t n_cand, int32_t dim,
                               const float* queries, int64_t ldq,
                               int64_t n_queries, int64_t plan_queries, int32_t k,
                               int64_t index_offset, float* kth_lb,
                               void* workspace, size_t workspace_bytes,
                               tt_stream_t stream);
int tt_bruteforce_shard_finalize(const void* index, const float* cand,
                                 int64_t ldc, int64_t n_cand, int32_t dim,
                                 const float* queries, int64_t ldq,
                                 int64_t n_queries, int64_t plan_queries,
                                 int32_t k, int64_t index_offset,
                                 const float* floor,
                                 float* out_scores, int32_t* out_idx,
                                 void* workspace, size_t workspace_bytes,
                                 tt_stream_t stream);

/* Merge `num_lists` per-shard sorted top-k_in lists laid out
 * [num_lists][n_queries][k_in] into the global top-k_out with the same
 * order (score descending, index ascending on ties). */
int tt_topk_merge(const float* scores, const int32_t* idx, int32_t num_lists,
                  int64_t n_queries, int32_t k_in, int32_t k_out,
                  float* out_scores, int32_t* out_idx, tt_stream_t stream);

/* Exact top-k with per-query exclusions (TensorFlow Recommenders'
 * query_with_exclusions): remove each query's excluded candidates from its
 * sorted list and compact to k_out.  scores / idx are [n_queries][k_in],
 * sorted as tt_bruteforce_search and tt_topk_merge write them; query q's
 * exclusions are E_q = excl_idx[excl_off[q] .. excl_off[q + 1]) (candidate
 * indices in the lists' numbering, any order; excl_off is device int64
 * [n_queries + 1], non-decreasing, and every offset lies inside excl_idx).
 *   - Output row q holds the input entries, in input order, whose index is
 *     not in E_q; only the first k_out of them are written.  Scores and
 *     indices are copied, never recomputed.  Run on the exact top-(k +
 *     |E_q|) this leaves the exact top-k of the remaining candidates in the
 *     same order (score descending, ties to the lower index).
 *   - Positions past the kept entries hold (-inf, 0x7FFFFFFF), the padding
 *     tt_bruteforce_shard_finalize writes and tt_topk_merge sorts last.
 *   - n_kept (int32 [n_queries], or NULL) receives min(k_out, kept entries).
 *   - E_q may be empty, longer than k_in (no upper bound), unordered, and
 *     may hold duplicates and values that are not in the list; negative
 *     values and 0x7FFFFFFF match nothing, so an input padding entry
 *     (idx == 0x7FFFFFFF) is never removed: it counts as a kept entry and
 *     stays at the tail.
 *   - The outputs must not overlap the inputs.
 * Needs 1 <= k_out <= k_in <= 4096 and n_queries >= 0 (0: TT_OK, no launch);
 * every pointer but n_kept non-NULL when n_queries > 0, except that excl_idx
 * may be NULL when the caller guarantees that every list is empty
 * (excl_off[q] == excl_off[q + 1] for all q).  One launch, O(k_in + |E_q|)
 * per query, no workspace. */
int tt_topk_exclude(const float* scores, const int32_t* idx, int64_t n_queries,
                    int32_t k_in, int32_t k_out, const int64_t* excl_off,
                    const int32_t* excl_idx, float* out_scores, int32_t* out_idx,
                    int32_t* n_kept, tt_stream_t stream);

/* The in-batch loss's batch reduction (CategoricalCrossentropy reduction
 * SUM, runner.py:78-83): out[0] = scale * sum(x[0..n)), one deterministic
 * single-workgroup launch. */
int tt_sum(const float* x, int64_t n, float scale, float* out, tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K14  Recall hits (IndexRecall.__call__, metrics/index_recall.py:52-58):
 * hits[t] += #{b : true_ids[b] in cand_ids[b, 0:ks[t]]}.  hits is int64
 * [num_ks], accumulated (not overwritten).
 * ------------------------------------------------------------------------ */
int tt_recall_hits(const int32_t* true_ids, const int32_t* cand_ids,
                   int64_t batch, int32_t k_total, const int32_t* ks_host,
                   int32_t num_ks, int64_t* hits, tt_stream_t stream);

/* Ranking metrics on multi-item ground truth: recall@k, AP@k (its mean is
 * MAP@k, the H&M task's MAP@12), NDCG@k and the reciprocal rank, per query
 * and for every k = ks[j].  cand is [n_queries][k_list] with row stride
 * ld_cand (indices or integer identifiers, as tt_bruteforce_search,
 * tt_topk_merge and tt_topk_exclude write them), truth [n_queries][T] with row
 * stride ld_truth (both strides in elements).  A value < 0 or == 0x7FFFFFFF
 * is padding on either side: it matches nothing and is not counted; padding
 * may sit anywhere in a truth row.
 *   - m = number of DISTINCT valid truth ids.  Position i (1-based) is a hit,
 *     h_i = 1, when cand[i] is valid, is in the truth set and i is the first
 *     list position holding that id (a repeated list entry is credited once);
 *     c_i = h_1 + ... + h_i.
 *   - hits[q][j] = c_k (int32), and vals[q][j][0..3] in fp32, one IEEE
 *     operation per step, no contraction:
 *       recall = float(c_k) / float(m)
 *       ap     = (sum over hits i <= k of float(c_i) / float(i)) / float(min(m, k))
 *       ndcg   = (sum over hits i <= k of disc[i - 1]) / idcg[min(m, k)]
 *       rr     = 1 / float(first hit) when it is <= k, else 0
 *     both sums sequential in ascending i, starting from their first term.
 *   - disc [k_list] and idcg [k_list + 1] are device fp32 tables built by the
 *     caller (no transcendental runs on the device): disc[i] = float(1 /
 *     log2(i + 2)) computed in double and rounded once, idcg[0] = 0 and
 *     idcg[n] the sequential fp32 prefix sum of disc.
 *   - A query with m = 0 gets zeros in vals and hits, reports m = 0 and is left
 *     out of every accumulator.  m_out (int32 [n_queries], or NULL) receives m.
 *   - Accumulators (all three or none), added to like tt_recall_hits' hits:
 *     acc_f64 double [num_ks][4] += the sums of recall, ap, ndcg, rr; acc_i64
 *     int64 [num_ks][2] += the sum of c_k and the number of queries with
 *     c_k > 0; n_valid int64 [1] += the number of queries with m > 0.  The
 *     double sums are deterministic (a second launch, no floating-point
 *     atomics): per (j, metric), lane t of 256 adds queries t, t + 256, ... in
 *     ascending order as doubles, then x[t] += x[t + s] for s = 128 .. 1, then
 *     acc += x[0].
 *   - ks is a host array, any order, repeats allowed.  The outputs must not
 *     overlap the inputs.
 * Needs 1 <= k_list <= 4096, 1 <= T <= 1024, 1 <= num_ks <= 16, every ks[j]
 * in [1, k_list], ld_cand >= k_list, ld_truth >= T, 0 <= n_queries < 2^31
 * (0: TT_OK, no launch) and every pointer but m_out and the accumulators
 * non-NULL when n_queries > 0.  O(T + k_list) per query, no workspace. */
int tt_rank_metrics(const int32_t* cand, int64_t ld_cand, int32_t k_list,
                    const int32_t* truth, int64_t ld_truth, int32_t T,
                    int64_t n_queries, const int32_t* ks_host, int32_t num_ks,
                    const float* disc, const float* idcg,
                    float* vals, int32_t* hits, int32_t* m_out,
                    double* acc_f64, int64_t* acc_i64, int64_t* n_valid,
                    tt_stream_t stream);


/* ------------------------------------------------------------------------ *
 * K15  Input pipeline.
 * Replaces the TFRecord dataset (pkg/modelling/tfrecord_dataset.py:59-98)
 * and the per-batch StringLookup (pkg/modelling/layers/input_layer.py:33-36).
 *
 * Host vocabulary (CPU only, no device memory): strings are passed as an
 * Arrow-style arena — `data` bytes and `offsets[n + 1]` (int64, value i is
 * data[offsets[i] .. offsets[i+1])).  vocab[i] -> row i + 1, any other value
 * -> row 0 (StringLookup num_oov_indices=1); a value listed twice maps to its
 * last row.  tt_vocab_create copies the arena; `num_threads` <= 0 uses every
 * hardware thread (at most 64).
 * ------------------------------------------------------------------------ */
int tt_vocab_create(const char* data, const int64_t* offsets, int64_t n, void** out_vocab);
int64_t tt_vocab_size(const void* vocab);
int tt_vocab_encode(const void* vocab, const char* data, const int64_t* offsets, int64_t n,
                    int32_t* out_rows, int32_t num_threads);
int tt_vocab_destroy(void* vocab);

/* Device batch assembly from an HBM-resident dataset of 32-bit words
 * (int32 rows / float32 values), column-major `src[ncols][src_ld]`:
 *   dst[c * dst_ld + b] = src[c * src_ld + perm[*cursor + b]],  b < batch,
 * then (advance != 0) *cursor += batch.  perm (int64 [n_rows]) is the
 * epoch's example order (the reference's shuffle buffer), cursor an int64 in
 * device memory, so the call can be captured in a replayed graph.  A position
 * or permutation entry outside [0, n_rows) writes zero words and ORs 1 into
 * *status (optional device int32). */
int tt_batch_take(const void* src, int64_t src_ld, int32_t ncols, const int64_t* perm, int64_t n_rows,
                  int64_t* cursor, int64_t batch, int32_t advance, void* dst, int64_t dst_ld,
                  int32_t* status, tt_stream_t stream);

/* Mixed negative sampling, the candidate side of a step: the batch's `batch`
 * candidates followed by `m` catalogue rows drawn uniformly with replacement,
 * sampled and assembled in one pass over dst (32-bit words, column-major):
 *   dst[f * dst_ld + b]         = batch_cols[f][b]             b < batch
 *   dst[f * dst_ld + batch + j] = cat[f * cat_ld + s_j]        j < m
 * batch_cols is a HOST array of ncols (<= 32) device pointers, one [batch]
 * column each; cat is the catalogue, column-major [ncols][cat_ld] with n_cat
 * rows.  s_j = (u_j * n_cat) >> 32 with u_j word j & 3 of Philox4x32-10
 * (multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85) at
 * counter (j >> 2, step lo, step hi, 0) and key (seed lo, seed hi).  `step`
 * is an int64 in device memory: every slot of one call sees the same value
 * and the call leaves step + 1 behind, so the call can be captured and every
 * replay of the graph draws fresh rows; it synchronises with nothing.
 * BIAS: the multiply-high mapping sends 2^32 words onto n_cat rows, so a
 * row's probability is floor or ceil of 2^32 / n_cat over 2^32: it departs
 * from 1 / n_cat by less than 2^-32, a relative bias of at most n_cat / 2^32
 * (2.5e-5 at the 105,542 articles of H&M).  n_cat < 1 or n_cat >= 2^31 draws
 * nothing: the sampled slots get zero words and 1 is ORed into *status
 * (optional device int32; without it such an n_cat is TT_ERR_BAD_ARG). */
int tt_mixed_candidates(const void* const* batch_cols, const void* cat, int64_t cat_ld, int32_t ncols,
                        int64_t batch, int64_t m, int64_t n_cat, uint64_t seed, int64_t* step, void* dst,
                        int64_t dst_ld, int32_t* status, tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * K4  Tower MLP, row-streaming GEMM (Dense layers, pkg/modelling/models/
 * tower.py:41-49): C[M, N] = epi(maskA(A) . B) for a tall fp32 activation
 * A [M, K] and a small weight operand B [K, N], on bf16x3 MFMA
 * (fp32-faithful: a_lo b_hi + a_hi b_lo + a_hi b_hi, fp32 accumulation).
 * Bounds: N <= 4096 (tt_mlp_wgrad's; above it TT_ERR_UNSUPPORTED) and
 * M * lda < 2^30, M * ldam < 2^30 (32-bit buffer offsets); K is bounded only
 * by lda.  A workgroup holds 64 rows x at most 384 columns: N <= 384 is one
 * workgroup per 64 rows, a wider N runs (row blocks) x ceil(N / 384) column
 * groups in the same launch, each output element with the arithmetic of the
 * narrow kernel (the result over any 128-aligned column window equals a call
 * on that window's slice of B bit for bit).
 *   maskA (amask != NULL):  A := (amask > 0) ? A * (*scale) : 0   (ReluGrad)
 *   epilogue:  + bias[n] (bias != NULL), relu (relu != 0), then
 *              C := (cmask > 0) ? C : 0 (cmask != NULL)
 * B is first packed by tt_mlp_pack into a bf16 hi/lo image in MFMA fragment
 * order (img_bytes >= tt_mlp_pack_bytes(K, N)); trans != 0 packs B = W^T of a
 * row-major W [N, K] (the input-gradient GEMMs).  scale is a device scalar.
 * ------------------------------------------------------------------------ */
size_t tt_mlp_pack_bytes(int32_t K, int32_t N);
int tt_mlp_pack(const float* w, int64_t ldw, int32_t K, int32_t N, int32_t trans, void* img, size_t img_bytes,
                tt_stream_t stream);
/* Up to 8 packs in one launch (a tower's forward and transposed images). */
typedef struct {
  const float* w;
  int64_t ldw;
  int32_t K, N, trans;
  void* img;
  size_t img_bytes;
} tt_mlp_pack_job;
int tt_mlp_pack_many(const tt_mlp_pack_job* jobs, int32_t num_jobs, tt_stream_t stream);
/* tt_gather_multi and tt_mlp_pack_many in ONE launch (independent work: the
 * towers' input gather and the weight images their forward reads), so the
 * train step's forward starts with no pack launch and no fork in front of
 * it.  Results identical to the two calls.  batch >= 1, 1..8 jobs. */
int tt_gather_multi_pack(const tt_gather_call* calls, int32_t num_calls, int64_t batch,
                         const tt_mlp_pack_job* jobs, int32_t num_jobs, tt_stream_t stream);
/* colsum != NULL: also colsum[n] = sum_m C[m][n] (the bias gradient of the
 * layer below, BiasAddGrad): per-workgroup partial sums in the epilogue, then
 * one small launch adds them in workgroup order (deterministic); needs a
 * caller workspace of tt_mlp_rows_workspace_size(M, N) bytes. */
size_t tt_mlp_rows_workspace_size(int64_t M, int32_t N);
int tt_mlp_rows(const float* A, int64_t lda, const float* amask, int64_t ldam, const float* scale, int64_t M,
                int32_t K, const void* img, int32_t N, const float* bias, int32_t relu, const float* cmask,
                int64_t ldcm, float* C, int64_t ldc, float* colsum, void* workspace, size_t workspace_bytes,
                tt_stream_t stream);
/* Weight + bias gradient of a Dense layer (the tape's MatMul and BiasAddGrad):
 * dwb[Ka + 1, N] = [A | 1]^T . Gm, Gm = G, or (gmask > 0) ? G * (*scale) : 0
 * (gmask != NULL: the layer's own ReluGrad).  dwb row-major with ld N — the
 * flat parameter layout of kernel [Ka, N] followed by bias [N].  bf16x3 MFMA,
 * batch split over workgroups, partials added in split order (deterministic;
 * workspace of tt_mlp_wgrad_workspace_size bytes).  Ka in [1, 4096], N a
 * multiple of 4 in [4, 4096]. */
size_t tt_mlp_wgrad_workspace_size(int64_t M, int32_t Ka, int32_t N);
int tt_mlp_wgrad(const float* A, int64_t lda, const float* G, int64_t ldg, const float* gmask, int64_t ldgm,
                 const float* scale, int64_t M, int32_t Ka, int32_t N, float* dwb, void* workspace,
                 size_t workspace_bytes, tt_stream_t stream);
/* tt_mlp_wgrad plus the layer's Adagrad step (ResourceApplyAdagradV2 on
 * param / accum, the layer's [Ka + 1, N] region of the flat buffer and its
 * accumulator, 16-B aligned) applied by the partial-sum launch to the summed
 * gradient — tt_dense_adagrad's arithmetic, without its launch. */
int tt_mlp_wgrad_adagrad(const float* A, int64_t lda, const float* G, int64_t ldg, const float* gmask,
                         int64_t ldgm, const float* scale, int64_t M, int32_t Ka, int32_t N, float* dwb,
                         float* param, float* accum, float lr, float epsilon, void* workspace,
                         size_t workspace_bytes, tt_stream_t stream);

/* The two towers' layers as ONE launch each (the query and the candidate
 * tower are independent chains of the same shape of work: one stream, no
 * fork/join).  p points at 2 problems with tt_mlp_rows' / tt_mlp_wgrad's
 * arguments and contracts (rows: no colsum); the results equal two single
 * calls bit for bit.  The two rows problems may differ in width and in their
 * number of column groups (N <= 4096 each).  Replaces the two towers' Dense
 * layers of two_tower_model.py:90-91 (query_tower(x), candidate_tower(x)). */
typedef struct {
  const float* A;
  int64_t lda;
  const float* amask;
  int64_t ldam;
  const float* scale;
  int64_t M;
  int32_t K;
  const void* img;
  int32_t N;
  const float* bias;
  int32_t relu;
  const float* cmask;
  int64_t ldcm;
  float* C;
  int64_t ldc;
} tt_mlp_rows_problem;
int tt_mlp_rows_pair(const tt_mlp_rows_problem* p, tt_stream_t stream);
typedef struct {
  const float* A;
  int64_t lda;
  const float* G;
  int64_t ldg;
  const float* gmask;
  int64_t ldgm;
  const float* scale;
  int64_t M;
  int32_t Ka, N;
  float* dwb;
} tt_mlp_wgrad_problem;
size_t tt_mlp_wgrad_pair_workspace_size(const tt_mlp_wgrad_problem* p);
int tt_mlp_wgrad_pair(const tt_mlp_wgrad_problem* p, void* workspace, size_t workspace_bytes, tt_stream_t stream);

/* One Dense layer's backward (the tape's MatMul / BiasAddGrad / ReluGrad of
 * one layer) in ONE launch of three independent block roles: the layer's
 * weight-gradient split partials (job w), the input-gradient GEMM of the
 * layer below (r: tt_mlp_rows' problem, no colsum, N <= 384; NULL or M == 0:
 * none) and the PREVIOUS (upper) layer's partial sums plus its optional
 * Adagrad step (prev: the job passed as w to the previous call; NULL: none).
 * A tower's backward chain is then one launch per layer plus
 * tt_mlp_wgrad_finish(last job), where tt_mlp_wgrad(_adagrad) + tt_mlp_rows
 * take three per layer, one after another.  Results equal those calls bit
 * for bit.  The roles exchange no data inside a launch: r reads the packed
 * image, never the parameters prev's Adagrad step updates.  A job's partials
 * (parts, tt_mlp_wgrad_workspace_size bytes, 16-B aligned like dwb) must stay
 * untouched until its sums ran, so consecutive layers use different partial
 * buffers (overlap is refused). */
typedef struct {
  tt_mlp_wgrad_problem p;
  void* parts;
  size_t parts_bytes;
  float* param; /* optional Adagrad on the summed gradient (NULL: none) */
  float* accum;
  float lr, eps;
} tt_mlp_wgrad_job;
int tt_mlp_backward_layer(const tt_mlp_wgrad_job* w, const tt_mlp_rows_problem* r, const tt_mlp_wgrad_job* prev,
                          tt_stream_t stream);
/* The partial sums (+ Adagrad) of one job on their own (the last layer of a
 * chain). */
int tt_mlp_wgrad_finish(const tt_mlp_wgrad_job* w, tt_stream_t stream);

/* Cosine scoring: L2 normalisation of the rows of the towers' joint
 * embeddings, and its gradient (TensorFlow Recommenders'
 * Retrieval(temperature=...) on normalised tower outputs; the reference has
 * no such option).  1 or 2 jobs (the two towers' operands) in ONE launch;
 * stream-ordered, no workspace, no allocation, no synchronisation.
 *
 * Forward, per row i:  ss_i = sum_k x_ik^2 in fp32;  inv_i = 1 / sqrt(ss_i)
 * if ss_i > 0, else 0;  y_i = x_i * (scale * inv_i).  inv [rows] is written
 * and holds the UNSCALED reciprocal norm.
 * Gradient, per row i:  u_i = x_i * inv_i;
 *   dx_i = scale * inv_i * (dy_i - u_i (u_i . dy_i)).
 * Zero rows: a row with ss_i == 0 gives y_i = 0, inv_i = 0 and dx_i = 0
 * exactly (+0.0f in every element): a dead embedding gets no gradient, as
 * through its ReLU.  There is no epsilon (and none of the 1 / epsilon
 * gradient an epsilon brings).
 * Shapes: dim in 1..4096; every leading dimension (in floats) >= dim; rows
 * need not be 16-byte aligned (any dim, odd leading dimensions): 16-byte
 * accesses are used only for an operand whose base is 16-byte aligned and
 * whose leading dimension is a multiple of 4.  Columns dim..ld of an output
 * are never written.
 * Aliasing: dx == dy (in place) is allowed; a row is read completely before
 * any of it is written.  No other overlap of an output with an operand.
 * Determinism: the summation order over a row is fixed (by column index
 * only), so a row's result depends only on that row, dim and scale: not on
 * rows, on addresses or leading dimensions, on which job holds it or on the
 * other job.  A two-job launch equals two one-job launches bit for bit.
 * rows == 0: TT_OK for that job, no work (its pointers are not looked at).
 * TT_ERR_BAD_ARG (with a message, checked on the host before any launch):
 * NULL jobs or a NULL pointer of a job with rows, num_jobs outside 1..2, dim
 * outside 1..4096, a leading dimension < dim, rows outside 0..2^31, or a
 * scale that is not finite. */
typedef struct {
  const float* x;
  int64_t ldx;
  float* y;
  int64_t ldy;
  float* inv;
  int64_t rows;
  int32_t dim;
  float scale;
} tt_l2norm_job;
int tt_l2norm_rows(const tt_l2norm_job* jobs, int32_t num_jobs, tt_stream_t stream);
typedef struct {
  const float* x;
  int64_t ldx;
  const float* inv;
  const float* dy;
  int64_t lddy;
  float* dx;
  int64_t lddx;
  int64_t rows;
  int32_t dim;
  float scale;
} tt_l2norm_grad_job;
int tt_l2norm_rows_grad(const tt_l2norm_grad_job* jobs, int32_t num_jobs, tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Sequence features: pooled embedding bags (Keras Embedding + masked pooling,
 * TF safe_embedding_lookup_sparse(combiner=...); the reference has no such
 * feature).  A bag is the L id slots of one example for one sequence
 * feature; slot l of example b is ids[b * ids_row_stride + l *
 * ids_pos_stride] (strides in elements, so a [batch, L] tensor and the
 * transposed view of an [L, batch] block are both read in place).  A slot is
 * valid when 0 <= id < num_rows (row 0, the OOV row, is valid); the padding
 * id is -1 and any other id out of range is treated like padding.  cnt_b is
 * the number of valid slots of example b.  1..TT_BAG_MAX_JOBS jobs (every
 * sequence feature of every tower of the call) in ONE launch; stream-ordered,
 * no workspace, no allocation, no synchronisation, no atomics.
 *
 * tt_gather_bag, per example b of each job:
 *   s = ((row(l0) + row(l1)) + ...) over the valid slots in slot order, in
 *   fp32, one IEEE add per step;  scale = 1 (sum), 1 / cnt (mean) or
 *   1 / sqrt(cnt) (sqrtn), IEEE division and square root, and 0 when cnt = 0;
 *   out[b, col_offset : col_offset + dim] = s * scale (sum: s itself, no
 *   multiply);  an empty bag writes +0.0;  scale_out[b] = scale.
 * Columns outside the job's range are not touched.
 * tt_bag_grad_expand, per lookup j = b * L + l of each job:
 *   ids_flat[j] = id if the slot is valid, else -1;  for a valid slot
 *   grad[j, 0:dim] = dout[b, col_offset : col_offset + dim] * scale[b] (one
 *   fp32 multiply; a copy for sum).  Rows of invalid slots are not written.
 * (ids_flat, grad) is then a flat sparse problem of batch * L lookups for
 * tt_sparse_adagrad / tt_sparse_adam: one source, grad_ld = dim,
 * grad_col_offset = 0.
 * Determinism: every output element is formed by one lane in slot order, so
 * a bag's result depends only on that bag: not on batch, on addresses or
 * leading dimensions (16-byte accesses are used only where base and leading
 * dimension allow them, with the same element order), on which job holds it
 * or on the other jobs.  A two-job launch equals two one-job launches.
 * TT_ERR_BAD_ARG (checked on the host before any launch): NULL jobs,
 * num_jobs outside 1..TT_BAG_MAX_JOBS, a NULL table, L outside 1..1024,
 * dim < 1, batch * L >= 2^24 (tt_sparse's lookup bound), an empty table, an
 * unknown pooling, a negative id stride, columns outside the leading
 * dimension, or (batch > 0) a NULL pointer.  dim > 1024: TT_ERR_UNSUPPORTED.
 * batch == 0: TT_OK, no work. */
#define TT_BAG_MAX_JOBS 8
#define TT_BAG_SUM 0
#define TT_BAG_MEAN 1
#define TT_BAG_SQRTN 2
typedef struct {
  const float* table;      /* [num_rows, dim], contiguous */
  int64_t num_rows;
  int32_t dim;
  int32_t L;
  const int32_t* ids;
  int64_t ids_row_stride;
  int64_t ids_pos_stride;
  int32_t pooling;         /* TT_BAG_SUM / TT_BAG_MEAN / TT_BAG_SQRTN */
  int32_t col_offset;
  float* out;              /* [batch, out_stride] */
  int64_t out_stride;
  float* scale_out;        /* [batch] */
} tt_bag_job;
int tt_gather_bag(const tt_bag_job* jobs, int32_t num_jobs, int64_t batch, tt_stream_t stream);
typedef struct {
  int64_t num_rows;
  int32_t dim;
  int32_t L;
  const int32_t* ids;
  int64_t ids_row_stride;
  int64_t ids_pos_stride;
  int32_t pooling;
  int32_t col_offset;
  const float* dout;       /* [batch, dout_stride] */
  int64_t dout_stride;
  const float* scale;      /* [batch], tt_gather_bag's scale_out */
  int32_t* ids_flat;       /* [batch * L] */
  float* grad;             /* [batch * L, dim], contiguous */
} tt_bag_grad_job;
int tt_bag_grad_expand(const tt_bag_grad_job* jobs, int32_t num_jobs, int64_t batch, tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Per-example sample weights of the in-batch loss (TensorFlow Recommenders'
 * Retrieval task sample_weight, Keras fit(sample_weight=...); the reference
 * has no such option):  L = sum_i w_i l_i.  ONE launch between the rows pass
 * and the cols pass; no pass kernel changes.  w [n] holds the NORMALISED
 * weights w_i / w_max in [0, 1]; the loss is linear in w, so the caller puts
 * w_max into the loss scale and the backward's scalar.
 *
 * The cols entries use lse and row_loss only in exp(S'_ij - lse_i) (negative
 * pairs) and in -expm1(-row_loss_i) = 1 - P_ii (the positive pair).  Handed
 *   lse_w_i      = lse_i - ln w_i                       and
 *   row_loss_w_i = -log1p(w_i expm1(-row_loss_i)),  so that
 *   -expm1(-row_loss_w_i) = w_i (1 - P_ii),
 * the unchanged cols entry returns sum_{i != r} w_i P_ij q_i - w_r (1 - P_rr)
 * q_r, the weighted loss's gradient.  d L / d q_i is the rows pass's dq row
 * scaled by w_i, done here in place.  Per row i:
 *   w_i == 1:     wloss = row_loss_i, lse_w = lse_i, row_loss_w = row_loss_i
 *                 (the same bits: copies, not the formulas); dq row not touched.
 *   w_i == 0:     wloss = +0, lse_w = +inf, row_loss_w = +0; dq row STORED as
 *                 +0 (not multiplied: an inf or NaN in it does not survive).
 *   0 < w_i < 1:  wloss = w_i * row_loss_i (one IEEE multiply),
 *                 lse_w = lse_i - logf(w_i),
 *                 row_loss_w = -log1pf(w_i * expm1f(-row_loss_i)),
 *                 dq[i, e] = w_i * dq[i, e] (one IEEE multiply per element).
 *   w_i < 0, w_i > 1 or NaN: NaN in all three scalars and in the dq row (the
 *                 loss goes NaN in sight; no silent clamp).
 * dq [n, lddq] may be NULL (and is not looked at when dim == 0: the
 * evaluation loss); wloss may be NULL; lse_w / row_loss_w may alias lse /
 * row_loss (each row's scalars are read before they are written, by one
 * lane).  dq rows need not be 16-byte aligned: 16-byte accesses are used
 * only where dq's base is 16-byte aligned and lddq is a multiple of 4, with
 * the same result bits.  Columns dim..lddq are never written.  A row's
 * results depend only on that row's inputs.  Stream-ordered, no workspace,
 * no allocation, no synchronisation, no atomics; n is not bounded by the
 * grid.  n == 0: TT_OK, no work (the pointers are not looked at).
 * TT_ERR_BAD_ARG (with a message, checked on the host before the launch):
 * n < 0, dim < 0, lddq < dim, or (n > 0) NULL w, lse, row_loss, lse_w or
 * row_loss_w. */
int tt_inbatch_weight_rows(const float* w, const float* lse, const float* row_loss, int64_t n,
                           float* lse_w, float* row_loss_w, float* wloss,
                           float* dq, int64_t lddq, int32_t dim, tt_stream_t stream);

/* ------------------------------------------------------------------------ *
 * Gradient clipping (tf.keras.optimizers.legacy clipvalue / clipnorm /
 * global_clipnorm, in the order of _transform_gradients), in place over the
 * gradient values the optimizer entries consume, entirely on the device.
 *
 * A region is a [rows, cols] range of fp32 (row r at g + r * ld; any column
 * offset, any ld >= cols) that belongs to variable `var`; several regions may
 * share a variable (a table looked up by several features).  With row_ids,
 * row r is skipped (neither read nor written) when row_ids[r] < 0: the rows
 * tt_bag_grad_expand leaves unwritten.  Regions reach the kernels by value,
 * TT_CLIP_MAX_REGIONS per launch; any number is taken, in chunks.
 *
 * tt_grad_sumsq: sumsq[v] = sum over variable v's values of c(g)^2 with
 *   c(g) = min(max(g, -clipvalue), clipvalue) (clipvalue <= 0: c(g) = g).
 *   Accumulated in fp64 from the exact products in a fixed order (per thread,
 *   a fixed tree per workgroup into the workspace, then one workgroup per
 *   variable over its partials; region chunks of one call add in call order):
 *   no floating-point atomics, equal bits every run, and equal bits for the
 *   same values at another address or leading dimension (16-byte accesses are
 *   used only where base and ld allow them, with the same element -> thread
 *   map).  A variable with no value gets 0.  Launches: 2 per region chunk.
 * tt_grad_clip_apply: g <- c(g) * f per element (one fp32 multiply), with
 *   f = 1                                   (neither norm set),
 *   f = clipnorm / max(n_v, clipnorm),  n_v = fp32(sqrt(sumsq[var]))  or
 *   f = global_clipnorm / max(n, global_clipnorm),  n = fp32(sqrt(sumsq[0] +
 *   sumsq[1] + ... in index order)): one IEEE fp32 division, exactly 1.0f for
 *   n <= c (an all-zero gradient included), so a clip that does not trigger
 *   changes no bit; a NaN norm gives a NaN factor.  factor[var] = f when
 *   factor is not NULL.  With neither norm set sumsq may be NULL.  Setting
 *   both norms is an error, as in Keras.  Launches: 1 per region chunk.
 * Stream-ordered; no allocation, no host read, no host-to-device copy.
 * TT_ERR_BAD_ARG (checked on the host before any launch): NULL regions with
 * num_regions > 0, num_regions < 0, num_vars < 1, var outside [0, num_vars),
 * negative rows or cols, ld < cols with rows > 1, a NULL g with values, NULL
 * sumsq where it is read, a NULL workspace, a NaN setting.  A workspace below
 * tt_grad_clip_workspace_size: TT_ERR_WORKSPACE.  A region of 2^31 or more
 * 4-float chunks: TT_ERR_UNSUPPORTED. */
#define TT_CLIP_MAX_REGIONS 32
typedef struct {
  float* g;
  int64_t rows;
  int32_t cols;
  int64_t ld;
  const int32_t* row_ids;  /* NULL, or [rows]: rows with id < 0 are skipped */
  int32_t var;
} tt_clip_region;
size_t tt_grad_clip_workspace_size(const tt_clip_region* regions, int32_t num_regions);
int tt_grad_sumsq(const tt_clip_region* regions, int32_t num_regions, int32_t num_vars, float clipvalue,
                  double* sumsq, void* workspace, size_t workspace_bytes, tt_stream_t stream);
int tt_grad_clip_apply(const tt_clip_region* regions, int32_t num_regions, int32_t num_vars, float clipvalue,
                       float clipnorm, float global_clipnorm, const double* sumsq, float* factor,
                       tt_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TT_H_ */
