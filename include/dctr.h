/*
 * dctr.h -- C-ABI of libdctr_hip.so: the MI355X (gfx950) hot path of DeepCTR-Torch.
 *
 * The reference (shenweichen/DeepCTR-Torch v0.2.9) has no native seam: every op on this path is a
 * chain of ATen calls issued from Python.  This header is the seam a maintainer would bind instead
 * (ctypes stub in INTEGRATION.md).  Each entry point names the reference lines it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (a PyTorch tensor) unless stated
 *     otherwise; the library never allocates, frees or retains memory.
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued, never synchronised, so every
 *     call is hipGraph-capturable.
 *   - return value: 0 ok, <0 a DCTR_E* code (bad argument; nothing was launched), >0 the hipError_t
 *     of the failed launch.  Nothing throws.
 *   - all arithmetic is fp32 (the reference computes in fp32).
 *   - ids travel as float32 inside X exactly as in the reference (basemodel.py:242) and are
 *     truncated toward zero like Tensor.long() (basemodel.py:369).
 */
#ifndef DCTR_H
#define DCTR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCTR_ABI_VERSION 35

#define DCTR_OK 0
#define DCTR_EINVAL (-1) /* null / negative / inconsistent argument            */
#define DCTR_ENOSUP (-2) /* shape outside what the kernels are built for        */
#define DCTR_EALIGN (-3) /* pointer or leading dimension violates an alignment  */

typedef void* dctr_stream_t; /* hipStream_t */

/* pooling of a VarLenSparseFeat (inputs.py:41-46, sequence.py:49-77); 0 = plain SparseFeat */
#define DCTR_POOL_NONE 0
#define DCTR_POOL_SUM 1
#define DCTR_POOL_MEAN 2
#define DCTR_POOL_MAX 3

/* One embedding "field": a SparseFeat / VarLenSparseFeat bound to its table.  64 bytes.
 * A deep field gathers dim-wide rows (inputs.py:158-180, basemodel.py:368-375); a wide field is the
 * same thing with dim == 1 (Linear's 1-dim tables, basemodel.py:45-46,65-67).                      */
typedef struct dctr_field {
  float* table;    /* [vocab, dim] rows `ld` floats apart, embedding_dict[embedding_name].weight     */
  float* gacc;     /* [vocab, dim] contiguous gradient slab, zero at rest (NULL when never accumulated) */
  float* state;    /* [vocab, dim] rows `ld_state` floats apart: optimizer state (Adagrad sum) or NULL */
  int64_t vocab;   /* rows                                                                           */
  int32_t dim;     /* embedding_dim (1 for wide)                                                     */
  int32_t col;     /* first column of X holding the id(s)        (inputs.py:99-123)                  */
  int32_t len;     /* 1 for SparseFeat, maxlen for VarLenSparseFeat                                  */
  int32_t pool;    /* DCTR_POOL_*                                                                    */
  int32_t len_col; /* column of X holding the valid length, or -1: mask = (id != 0) (inputs.py:146)  */
  int32_t out_off; /* float offset of this field's slice inside one output row (deep only)          */
  int32_t ld;      /* floats between consecutive rows of `table`; 0 = dim (contiguous).  A table may be a */
  int32_t ld_state;/* strided view of a slab that interleaves a row with its optimizer state (and the    */
                   /* wide weight of the same id): what is updated together then shares one 128-byte line */
} dctr_field_t;

/* ---- general update units (round 5): pooled VarLen fields and shared tables on the deterministic update ------
 * The reference pools a VarLenSparseFeat with SequencePoolingLayer (inputs.py:141-155, sequence.py:49-77) and lets
 * several feature columns share one nn.Embedding through `embedding_name` (inputs.py:158-180); autograd then sends
 * every (sample, position) of every such column to embedding_dense_backward of the ONE table.  Here a UNIT is a
 * (deep table | none, wide table | none) pair with every X column that feeds it -- its SLOTS (virtual columns):
 *   ids_t / parts_t are [n_vcols, B]; a unit's slots are consecutive virtual columns [c0, c0 + n_slots), so its entries
 *   are the contiguous run ids_t[c0 * B ... (c0 + n_slots) * B) and an entry is named by v = slot_local * B + b;
 *   a slot whose position is masked out for a sample (sum / mean pooling: id == 0, or t >= length) carries the tag
 *   0xFFFF in parts_t and is no entry; a max-pooled slot is always an entry, its gradient is masked per element by
 *   the forward's arg-max side output;
 *   a unit of n_slots slots is split over k = n_slots groups of P partitions (rows {id : id mod (k P) == j P + p} belong
 *   to workgroup (vunit (unit, j), p)), so a partition holds ~96 entries whatever the number of slots.
 * A plan without `ext` is the simple case the kernels have always run: unit u = one X column (units[u]) over its own
 * tables, n_vcols = n_vunits = n_units.                                                                              */
typedef struct dctr_uslot {
  int32_t col;      /* X column of the id                                                                            */
  int32_t goff;     /* float offset of the deep field's slice in `out` / `g_out` rows; -1: no deep side              */
  int32_t wide;     /* 1: the entry carries the wide gradient too                                                    */
  int32_t pool;     /* DCTR_POOL_* of the field(s) of this slot                                                      */
  int32_t t;        /* position inside a pooled field (0 otherwise)                                                  */
  int32_t len;      /* positions of the field                                                                        */
  int32_t len_col;  /* X column of the valid length, -1: mask = (id != 0)                                            */
  int32_t den;      /* row of den_t holding mean pooling's divisor count + 1e-8 (sequence.py:72-74); -1              */
  int32_t am_deep;  /* byte offset in an amax row of the deep field's per-element arg-max positions (max pooling); -1 */
  int32_t am_wide;  /* the same for the wide field (one byte); -1                                                    */
  int32_t vu0;      /* first vunit of the slot's unit                                                                */
  int32_t wfield;   /* index of the slot's wide field (its column of a per-field g_wide, DCTR_PLAN_WIDE_PER_FIELD); -1   */
} dctr_uslot_t;

typedef struct dctr_vunit {
  int32_t di, wi;        /* field whose descriptor supplies the unit's deep / wide table; -1: none                   */
  int32_t c0, n_slots;   /* the unit's virtual columns                                                               */
  int32_t k, j;          /* the unit has k * P partitions; this vunit's workgroups own [j P, (j + 1) P)              */
  int32_t kshift, pad_;  /* q / k == (q * kmagic) >> kshift for 0 <= q < 2^31 (kshift = 32 + ceil_log2 k)            */
  uint64_t kmagic;
} dctr_vunit_t;

/* host struct; `slots`, `vunits`, `am_deep_off`, `am_wide_off`, `den_t`, `amax` are DEVICE pointers, `h_*` host arrays.
 * den_t / amax are PER-STEP buffers the caller points at before each call:
 *   den_t [n_den, B] float  written by dctr_embed_ids, read by dctr_embed_update
 *   amax  [B, ld_amax] u8   written by dctr_embed_fwd (arg-max position per element of every max-pooled field, first
 *                           maximum wins like torch.max), read by dctr_embed_update                                  */
typedef struct dctr_plan_ext {
  const dctr_uslot_t* slots;    /* [n_vcols]                                                                         */
  const dctr_vunit_t* vunits;   /* [n_vunits]                                                                        */
  const int32_t* am_deep_off;   /* [n_deep] byte offset in an amax row, -1: not max-pooled                           */
  const int32_t* am_wide_off;   /* [n_wide]                                                                          */
  const dctr_vunit_t* h_vunits; /* host copy of vunits                                                               */
  const int64_t* h_vocab;       /* [n_vunits] rows of the vunit's tables                                             */
  float* den_t;
  uint8_t* amax;
  int32_t n_vcols, n_vunits, n_units, max_unit_slots;
  int32_t n_den, ld_amax;
  /* the pooled fields' positions, flattened in field order, for the fused gather + tower launch                     */
  /* (dctr_embed_tower_train_step): entry = (field index << 16) | position                                           */
  const int32_t* gslot_deep;    /* [n_gslot_deep] device                                                             */
  const int32_t* gslot_wide;    /* [n_gslot_wide] device                                                             */
  int32_t n_gslot_deep, n_gslot_wide;
} dctr_plan_ext_t;
#define DCTR_MAX_UNIT_SLOTS 128
size_t dctr_sizeof_uslot(void);
size_t dctr_sizeof_vunit(void);
size_t dctr_sizeof_plan_ext(void);

/* The compiled feature-column schema of one model: what build_input_features + create_embedding_matrix
 * + Linear.__init__ establish in the reference (inputs.py:99-180, basemodel.py:34-61).
 * The struct itself lives in HOST memory; the arrays it points to live on the device.              */
typedef struct dctr_plan {
  const dctr_field_t* deep;   /* [n_deep] fixed-length fields first, then VarLen (basemodel.py:380)  */
  const dctr_field_t* wide;   /* [n_wide]                                                            */
  const int32_t* dense_cols;  /* [n_dense]  X column of every dense scalar of dnn_feature_columns    */
  const int32_t* wdense_cols; /* [n_wdense] X column of every dense scalar of linear_feature_columns */
  const float* wdense_w;      /* [n_wdense] Linear.weight (basemodel.py:58-61), may be NULL          */
  int32_t n_deep;
  int32_t n_deep_fixed;       /* leading deep fields with len == 1                                   */
  int32_t n_wide;
  int32_t n_dense;
  int32_t n_wdense;
  int32_t dense_off;          /* float offset in an output row where the dense block goes, -1: skip  */
  int32_t emb_dim;            /* common dim of all deep fields, 0 if they differ (then no FM)        */
  int32_t n_xcols;            /* number of columns of X (width of the staged tile)                   */
  int32_t n_wide_fixed;       /* leading wide fields with len == 1                                   */
  int32_t max_dim;            /* max dim over deep fields (0 if none)                                */
  int32_t vec;                /* 4, 2 or 1: every deep dim, out_off, ld and base pointer is a        */
                              /* multiple of `vec` floats -- lets rows move as dwordx4/x2            */
  int32_t flags;              /* DCTR_PLAN_* : facts about the device arrays the host cannot see     */
  const uint64_t* out_chunks; /* nullable, device: dctr_embed_fwd writes output row b (and its wide logit, which must lie   */
  int32_t chunk_rows;         /* inside the row: wide = out + k, ld_wide = ld_out) to (float*)out_chunks[b / chunk_rows] +  */
  int32_t pad_;               /* (b % chunk_rows) * ld_out instead of out + b * ld_out: the owner's gather of the sharded   */
                              /* step pushes every rank's rows straight into that rank's receive buffer (peer memory)      */
  const dctr_plan_ext_t* ext; /* nullable (host): general update units -- pooled VarLen fields, shared tables (above)     */
} dctr_plan_t;

#define DCTR_PLAN_HAS_GACC 1    /* every field has a gacc slab                       */
#define DCTR_PLAN_HAS_STATE 2   /* every field has an optimizer state slab           */
#define DCTR_PLAN_HAS_MAXPOOL 4 /* some VarLen field uses DCTR_POOL_MAX              */
/* The first-order weights PER FIELD instead of summed (IFM / DIFM re-weight them per sample before the sum,
 * basemodel.py:80-91).  dctr_embed_fwd then writes wide[b * ld_wide + f] = w_f[id] for f < n_wide (a VarLen wide field
 * pooled as always) and the dense half of Linear, sum_j X[b, wdense_cols[j]] * wdense_w[j], into column n_wide
 * (ld_wide >= n_wide + 1); dctr_embed_update / dctr_embed_update_lazy read the gradient of wide field f at
 * g_wide[b * ld_gw + f] and that of the dense half (for g_wdense) at column n_wide; dctr_embed_bwd, which has no ld_gw,
 * takes g_wide as dense rows of n_wide + 1 floats.  Entry points that cannot honour the bit refuse it:
 * dctr_embed_tower_train_supported returns 0, plan->out_chunks and the shard kernels' callers get DCTR_ENOSUP.       */
#define DCTR_PLAN_WIDE_PER_FIELD 8

int dctr_abi_version(void);
const char* dctr_strerror(int code);
size_t dctr_sizeof_field(void); /* binding self-check */
size_t dctr_sizeof_plan(void);

/* ---- fused multi-table lookup (+VarLen pooling, +wide logit, +FM, +DNN-input layout) -------------
 * Replaces, in ONE launch: BaseModel.input_from_feature_columns (basemodel.py:354-380),
 * varlen_embedding_lookup + get_varlen_pooling_list + SequencePoolingLayer (inputs.py:141-155,213-227,
 * sequence.py:49-77), Linear.forward (basemodel.py:63-92), FM.forward (interaction.py:26-34) and
 * combined_dnn_input (inputs.py:126-138).
 *   X     [B, ldx]   the model input matrix (ids as float32)
 *   out   [B, ld_out] row b = [ deep field slices at field.out_off | dense block at plan.dense_off ]; only those are
 *         written: the padding of a row (and of a wide / fm_s row) keeps what the caller left there
 *   wide  [B]  sum_f w_f[id] (+pooled VarLen) + dense . Linear.weight     (nullable); element b lives at
 *         wide[b * ld_wide] (ld_wide = 1 for a plain vector; a column of `out` for the sharded exchange)
 *   fm    [B]  0.5 * sum_d ((sum_f e)^2 - sum_f e^2) over ALL deep fields (nullable; needs emb_dim)
 *   err   int32 flag; bit0 is set when an id falls outside [0, vocab) -- such a row reads as row 0
 *         (the reference raises IndexError on CPU; here the flag is polled by the host) (nullable)
 * A plan with general units (plan->ext) takes its ids / tags from dctr_embed_ids instead (ids_t must be NULL here); when
 * ext->amax is set the launch writes, for every max-pooled field, the position of the first maximum per element
 * (uint8 [B, ext->ld_amax] at ext->am_deep_off[f] / am_wide_off[f]): max pooling's backward in dctr_embed_update.
 * Optional side outputs feed dctr_embed_update (all nullable):
 *   ids_t [n_units, B] int32: ids_t[u][b] = (int) X[b, units[u].col]  (units: see dctr_embed_update)
 *   parts_t [n_units, B] uint16: clamp(ids_t[u][b]) mod dctr_embed_update_partitions(plan, B)  (needs ids_t)
 *   fm_s  [B, ld_s]    S[b, d] = sum_f e[b, f, d], the per-sample field sum FM's backward needs      */
int dctr_embed_fwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B, float* out,
                   int64_t ld_out, float* wide, int64_t ld_wide, float* fm, int32_t* err,
                   const int32_t* units, int32_t n_units, int32_t* ids_t, uint16_t* parts_t, float* fm_s,
                   int64_t ld_s, dctr_stream_t stream);

/* ---- backward of the above = embedding_dense_backward + FM backward, as an O(batch) scatter -------
 * Replaces autograd's aten::embedding_dense_backward x(n_deep+n_wide), the pooling backward and
 * FM's backward (called from basemodel.py:261).  Duplicate ids add (atomics).
 *   g_out  [B, ld_g]  gradient w.r.t. `out` (deep slices are read; dense block ignored)  (nullable)
 *   out    [B, ld_out] the forward output (read only when g_fm != NULL: FM backward needs e and sum e)
 *   g_fm   [B]  gradient w.r.t. fm          (nullable)
 *   g_wide [B]  gradient w.r.t. wide        (nullable)
 *   mode   DCTR_BWD_ACCUM: field.gacc[row] += g          (exact dense-gradient semantics, or pass 1
 *                          of a two-pass sparse optimizer)
 *          DCTR_BWD_SGD  : field.table[row] -= lr * g    (torch.optim.SGD(lr), basemodel.py:449-450;
 *                          only legal without max-pooled fields, whose backward re-reads the table) */
#define DCTR_BWD_ACCUM 0
#define DCTR_BWD_SGD 1
int dctr_embed_bwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B,
                   const float* g_out, int64_t ld_g, const float* out, int64_t ld_out,
                   const float* g_fm, const float* g_wide, int32_t mode, float lr,
                   dctr_stream_t stream);

/* ---- pass 2 of the sparse optimizers: consume + re-zero gacc rows touched by this batch -----------
 * For every id occurrence in X: G = exchange(gacc[row], 0); then per element with G != 0
 *   DCTR_OPT_SGD     p -= lr * G                                   (torch.optim.SGD, basemodel.py:450)
 *   DCTR_OPT_ADAGRAD s += G*G ; p -= lr * G / (sqrt(s) + eps)      (torch.optim.Adagrad, :454)
 * Rows whose gradient is zero do not move under these two optimizers, so the result equals the
 * reference's dense update.                                                      */
#define DCTR_OPT_SGD 0
#define DCTR_OPT_ADAGRAD 1
int dctr_embed_apply(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B, int32_t opt,
                     float lr, float eps, dctr_stream_t stream);

/* ---- deterministic fused backward + optimizer (csrc/update.hip) ------------------------------------
 * The O(batch) replacement of embedding_dense_backward + the pooling's backward + FM backward + the optimizer's walk
 * over the tables (basemodel.py:261-262).  Plans of fixed-length fields over distinct tables run one-column units
 * (`units` below); pooled VarLen fields and tables shared through embedding_name run GENERAL units (plan->ext,
 * dctr_plan_ext_t above: then n_units = ext->n_vunits, ids_t / parts_t are [ext->n_vcols, B], parts_t is required, `out`
 * must be the forward's rows when g_fm is given, ext->den_t / ext->amax must point at this step's side buffers).  No atomics:
 * workgroup (unit, partition) owns rows {id : id mod P == partition}, sorts its (id, b) entries in LDS
 * and read-modify-writes each touched row exactly once, summing duplicate ids in (id, b) order, so the
 * result is bit-reproducible (needed for replica equality under data parallelism).
 *   units  [n_units][4] int32 (device): {deep field index | -1, wide field index | -1, X column, 0};
 *          a unit is one id column with the deep and/or wide table it feeds
 *   ids_t  [n_units, B] int32 from dctr_embed_fwd / dctr_embed_ids;  parts_t [n_units, B] uint16 from the same
 *          call (nullable: every workgroup then divides every id of its unit itself)
 *   g_out / out / fm_s / g_fm / g_wide as in dctr_embed_bwd (fm_s = side output of dctr_embed_fwd);
 *          g_wide[b] lives at g_wide[b * ld_gw]
 *   opt    DCTR_UPD_SGD      table[row] -= lr * G                          (torch.optim.SGD)
 *          DCTR_UPD_ADAGRAD  state[row] += G*G ; table[row] -= lr*G/(sqrt(state[row])+eps)
 *          DCTR_UPD_ACCUM    gacc[row]  += G          (exact dense-gradient semantics: param.grad; a second launch
 *                            onto a non-zero gacc adds to it)
 *          Rows whose id is not in the batch are not written, in any of the three modes.
 *   max_vocab  largest vocab over the plan's fields (sizes the 32-bit sort keys)
 *   g_wdense [plan.n_wdense] (nullable): when given, n_wdense extra workgroups also write the gradient of the dense
 *          half of Linear, g_wdense[j] = sum_b g_wide[b] * X[b, wdense_cols[j]] (basemodel.py:86-90), in a
 *          fixed order; X / ld_x are only read for this.  wdense_step (nullable): they also step Linear.weight.
 * dctr_embed_update_supported returns 1 when the plan / batch fit (B <= 2^20, keys fit 32 bits).    */
#define DCTR_UPD_SGD 0
#define DCTR_UPD_ADAGRAD 1
#define DCTR_UPD_ACCUM 2
#define DCTR_UPD_LAZY 3   /* dctr_embed_update_lazy only: the lazily regularised / Adam step at the row (see below) */
/* One optimizer step on dense parameters, applied by the kernel that finishes their gradient (instead of a separate
 * dctr_dense_opt launch and the cross-queue join in front of it): the gradient tensor lives at grad_base + k inside
 * a flat gradient slab, its parameter at param_base + k, its Adagrad state at state_base + k.
 *   kind  DCTR_UPD_SGD: p -= lr * g        DCTR_UPD_ADAGRAD: s += g*g ; p -= lr * g / (sqrt(s) + eps)
 * (torch.optim.SGD / Adagrad, basemodel.py:447-461).  Host struct.                                                */
typedef struct dctr_dense_step {
  int32_t kind;
  float lr, eps;
  int32_t pad_;
  const float* grad_base;
  float* param_base;
  float* state_base; /* NULL for SGD */
} dctr_dense_step_t;
size_t dctr_sizeof_dense_step(void);

int dctr_embed_update_supported(const dctr_plan_t* plan, int64_t max_vocab, int32_t B);
/* P = partitions per unit that dctr_embed_update uses for this plan at batch B (0 on bad arguments).  The optional
 * side output parts_t [n_units, B] uint16 of dctr_embed_fwd / dctr_embed_ids holds clamp(id) mod P (clamp: an id
 * outside [0, vocab) counts as 0): with it a workgroup's scan over its unit's B entries is a 16-bit compare per
 * entry instead of an integer division per entry.                                                              */
int32_t dctr_embed_update_partitions(const dctr_plan_t* plan, int32_t B);
#ifdef DCTR_DIAG
/* diagnostics, only in the DCTR_DIAG build (make -C csrc diag -> libdctr_hip_diag.so; tools/upd_trace.py): buf != NULL
 * makes every workgroup of dctr_embed_update record 8 u64 (wall_clock64 at start / scan / sort / loads issued / loads
 * landed / tile 0 done / end, then its entry count); force_p > 0 overrides the number of partitions per unit.
 * dctr_dbg_update_trace(NULL, -1) restores normal operation.  The shipped library has no mutable global state.   */
void dctr_dbg_update_trace(unsigned long long* buf, int32_t force_p);
#endif
/* plan is only needed (non-NULL) when parts_t is requested.  A plan with general units (plan->ext): n_units =
 * ext->n_vunits, ids_t / parts_t are [ext->n_vcols, B] (one row per X column feeding a unit; a position that sum / mean
 * pooling masks out gets the tag 0xFFFF), and ext->den_t [ext->n_den, B] receives mean pooling's divisors count + 1e-8. */
int dctr_embed_ids(const dctr_plan_t* plan, const int32_t* units, int32_t n_units, const float* X, int64_t ldx,
                   int32_t B, int32_t* ids_t, uint16_t* parts_t, dctr_stream_t stream);
int dctr_embed_update(const dctr_plan_t* plan, const int32_t* units, int32_t n_units, int64_t max_vocab,
                      const int32_t* ids_t, const uint16_t* parts_t, int32_t B, const float* g_out, int64_t ld_g,
                      const float* out, int64_t ld_out, const float* fm_s, int64_t ld_s, const float* g_fm,
                      const float* g_wide, int64_t ld_gw, int32_t opt, float lr, float eps, const float* X,
                      int64_t ld_x, float* g_wdense, const dctr_dense_step_t* wdense_step, int32_t* workspace,
                      int64_t workspace_ints, int32_t presorted, dctr_stream_t stream);
/* The part of dctr_embed_update that needs nothing but the ids, as its own launch: every (unit, partition)'s entries
 * found, sorted by (id, sample) and parked in `workspace` (dctr_embed_update_workspace_ints ints; zero before the
 * first use).  Enqueue it any time after the forward -- on another stream, in the shadow of the tower -- and pass the
 * same workspace with presorted = 1 to dctr_embed_update: its workgroups then start with one coalesced read of their
 * keys (no scan, no sort).  Same results, bit for bit.  dctr_embed_update leaves the workspace ready for the next
 * dctr_embed_segments.                                                                                         */
int dctr_embed_segments(const dctr_plan_t* plan, const int32_t* units, int32_t n_units, int64_t max_vocab,
                        const int32_t* ids_t, const uint16_t* parts_t, int32_t B, int32_t* workspace,
                        int64_t workspace_ints, dctr_stream_t stream);
/* workspace (nullable): dctr_embed_update_workspace_ints(plan, n_units, B) int32, ZERO before the first use (the
 * kernels leave it ready for the next launch: its first n_units * P counters are zero again once dctr_embed_update's
 * launch has run, nothing behind the advertised size is touched).  With it (and presorted = 0) a pre-pass buckets
 * the (unit, sample) entries by partition, so no workgroup scans a unit's B ids: worth it for large (global)
 * batches; without it every workgroup scans.  presorted = 1: see dctr_embed_segments.                          */
int64_t dctr_embed_update_workspace_ints(const dctr_plan_t* plan, int32_t n_units, int32_t B);

/* ---- FM on an explicit [B, F, D] tensor (interaction.py:26-34) ------------------------------------
 * E is addressed as E[b*ld_b + f*D + d].  y[b] = 0.5 * sum_d((sum_f e)^2 - sum_f e^2).
 * backward: gE[b,f,d] (+)= gy[b] * (S[b,d] - E[b,f,d]);  accumulate != 0 adds into gE.             */
int dctr_fm_fwd(const float* E, int64_t ld_b, int32_t B, int32_t F, int32_t D, float* y,
                dctr_stream_t stream);
int dctr_fm_bwd(const float* E, int64_t ld_b, int32_t B, int32_t F, int32_t D, const float* gy,
                float* gE, int64_t ld_gb, int32_t accumulate, dctr_stream_t stream);

/* ---- input-aware FM of IFM / DIFM (ifm.py:74-83, difm.py:96-102, basemodel.py:80-91; csrc/iafm.hip) -------------
 * One launch per direction for the reference's softmax, two broadcasts, concat, FM and refined wide sum:
 *   m      = F * softmax_f(Z1)   DCTR_IAFM_SOFTMAX (stable: the row maximum is subtracted)   |   Z1 + Z2   DCTR_IAFM_SUM
 *   y_lin  = sum_f m_f * wl_f + wl_dense
 *   y_fm   = 0.5 * sum_d ((sum_f m_f e_fd)^2 - sum_f (m_f e_fd)^2)
 *   E  [B, F, D] rows at E + b*ld_e: the gather's buffer read in place (ld_e >= F*D)
 *   Wl [B, ld_w] the per-field wide buffer of a DCTR_PLAN_WIDE_PER_FIELD plan: columns 0 .. n_wl-1 are wl_f, column
 *      n_wl the dense half; n_wl is F or 0 (then only the dense column counts); Wl = NULL: y_lin = 0
 *   Z1 / Z2 [B, F] rows ld_z1 / ld_z2 apart (Z2 only in SUM mode);  m [B, F] is written for the backward
 * backward, with S_d = sum_f m_f e_fd and v_fd = m_f e_fd:
 *   gE_fd = g_fm m_f (S_d - v_fd);  gm_f = g_lin wl_f + g_fm sum_d e_fd (S_d - v_fd);  gWl_f = g_lin m_f, gWl[n_wl] = g_lin
 *   gZ = gm (SUM: one buffer serves Z1 and Z2)  |  gZ_k = m_k (gm_k - (1/F) sum_f gm_f m_f) (SOFTMAX)
 *   gE has E's row layout (columns past F*D are not written), gWl has Wl's (NULL when Wl is).
 * A group of lanes per sample holds the row in registers (read once), reductions by wave shuffles in a fixed order:
 * no atomics, identical bits from run to run.  dctr_iafm_supported(F, D) != 0 iff the shape fits (1 <= F <= 64, the row
 * in 8 strips per lane of a 64-lane group); the entry points return DCTR_ENOSUP otherwise.                          */
#define DCTR_IAFM_SOFTMAX 0
#define DCTR_IAFM_SUM 1
int dctr_iafm_supported(int32_t F, int32_t D);
int dctr_iafm_fwd(const float* E, int64_t ld_e, const float* Wl, int64_t ld_w, int32_t n_wl, const float* Z1,
                  int64_t ld_z1, const float* Z2, int64_t ld_z2, int32_t mode, int32_t B, int32_t F, int32_t D, float* m,
                  int64_t ld_m, float* y_lin, float* y_fm, dctr_stream_t stream);
int dctr_iafm_bwd(const float* E, int64_t ld_e, const float* Wl, int64_t ld_w, int32_t n_wl, const float* m, int64_t ld_m,
                  int32_t mode, int32_t B, int32_t F, int32_t D, const float* g_lin, const float* g_fm, float* gE,
                  int64_t ld_ge, float* gWl, int64_t ld_gw, float* gZ, int64_t ld_gz, dctr_stream_t stream);

/* ---- BiInteractionPooling (interaction.py:54-61) + NFM's combined_dnn_input (nfm.py:66-71) ---------------------
 *   bi[b, d] = 0.5 * ((sum_f e[b,f,d])^2 - sum_f e[b,f,d]^2)           out row b = [ bi (D) | dense (n_dense) ]
 * G is dctr_embed_fwd's `out` ([B, ld_g], fields first, the dense block at dense_off); the backward writes a gradient
 * with G's layout (what dctr_embed_update consumes): gG[b, f*D+d] = g[b,d] * (S[b,d] - e[b,f,d]), gG[b, dense_off+j]
 * = g[b, D+j].  Columns of gG outside the field / dense blocks are not written.                                  */
int dctr_bi_pooling_fwd(const float* G, int64_t ld_g, int32_t B, int32_t F, int32_t D, int32_t dense_off,
                        int32_t n_dense, float* out, int64_t ld_o, dctr_stream_t stream);
int dctr_bi_pooling_bwd(const float* G, int64_t ld_g, int32_t B, int32_t F, int32_t D, int32_t dense_off,
                        int32_t n_dense, const float* gout, int64_t ld_go, float* gG, int64_t ld_gg,
                        dctr_stream_t stream);

/* ---- ONN / NFFM: the second-order pair lookup (models/onn.py:14-34, :98-120, :139-148; csrc/pair_embed.hip) ---------
 * Every ordered pair p = (i < j) of sparse features owns two tables: emb1 indexed by feature i's id, emb2 by feature j's
 * (pairs in the reference's order: i ascending, then j).  The reference runs 2 P aten::embedding calls, P multiplies and a
 * cat, and 2 P dense [V, D] gradients backward; here one launch per direction.
 *   plan->deep holds 2 P FIXED-LENGTH fields of one common dim D: fields 2p and 2p + 1 are emb1 and emb2 of pair p, each
 *   with its own X column, table pointer, ld (row stride; 0 = D), vocab, and an out_off that is its offset in a
 *   ROW-GRADIENT row (2 p D and (2 p + 1) D) -- not in `out`, which holds one slice per PAIR.
 * forward:
 *   out[b, p D + d] = T_{2p}[id(b, col_{2p})][d] * T_{2p+1}[id(b, col_{2p+1})][d]      (one fp32 multiply)
 *   out[b, P D + k] = X[b, dense_cols[k]]   when plan->dense_off >= 0 (it must equal P D): combined_dnn_input's order
 *   (inputs.py:126-138); ld_out >= P D + n_dense, a multiple of plan->vec (gather buffers are padded to 4)
 *   wide[b * ld_wide] = the first-order logit exactly as dctr_embed_fwd computes it for the same plan -- the same device
 *   code (csrc/embed_tile.hpp), the same bits (nullable; a max-pooled wide field's arg-max goes to ext->amax likewise)
 *   err: bit 0 is set when an id falls outside [0, vocab); such a row reads as row 0 (nullable)
 * backward (re-reads the rows; nothing of size [B, 2 P D] is saved by the forward):
 *   g_rows[b, out_off_{2p}   + d] = g_out[b, p D + d] * T_{2p+1}[id(b, col_{2p+1})][d]
 *   g_rows[b, out_off_{2p+1} + d] = g_out[b, p D + d] * T_{2p}[id(b, col_{2p})][d]
 *   g_rows [B, ld_rows] is then what dctr_embed_update / dctr_embed_update_lazy / dctr_embed_bwd take as their g_out
 *   (ld_g = ld_rows): fixed-length fields over distinct tables are simple units.  Columns outside the 2 P slices are not
 *   written.  No atomics, no scratch.
 * plan->vec (4 / 2 / 1) is honoured -- D need not be a multiple of 4.  Refused with DCTR_ENOSUP: pooled or VarLen deep
 * fields (n_deep_fixed != n_deep), deep fields of different dims, plan->out_chunks, DCTR_PLAN_WIDE_PER_FIELD, an odd
 * n_deep, more than 65535 pairs, a tile beyond the LDS.                                                              */
int dctr_pair_embed_fwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B, float* out, int64_t ld_out,
                        float* wide, int64_t ld_wide, int32_t* err, dctr_stream_t stream);
int dctr_pair_embed_bwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B, const float* g_out, int64_t ld_g,
                        float* g_rows, int64_t ld_rows, dctr_stream_t stream);

/* ---- MLR / LS-PLM: the piece-wise linear mixture (models/mlr.py:78-100; csrc/mlr.hip) -------------------------------
 * R region Linear modules are a softmax gate and, read again, the learners; an optional bias Linear scales the result:
 *   z_h  = sum of head h's first-order weights (fixed-length fields, then pooled VarLen ones, in plan order)
 *          + sum_j X[b, dense_cols[j]] * dense_w[h][j - dense_off[h]]   for j in [dense_off[h], dense_off[h + 1])
 *   s    = softmax(z_0 .. z_{R-1})  (max-subtracted);   l_r = sigmoid(z_r) (DCTR_MLR_BINARY) | z_r (DCTR_MLR_REGRESSION)
 *   p0   = sum_r s_r l_r;   c = sigmoid(z_R) when has_bias, else 1;   y = p0 * c
 * The plan is wide-only (n_deep = 0, no dense block, no wdense_w) with DCTR_PLAN_WIDE_PER_FIELD: wide field f belongs to
 * head head_of[f]; heads 0 .. R-1 are the regions, head R the bias.  A head without fields and a head without dense
 * columns are ordinary.  H = n_regions + has_bias.
 * forward, one launch: the gather's workgroup geometry (64 samples, 4 waves that split the fields), X rows and descriptors
 *   staged in LDS once, 8 weight loads in flight per lane; VarLen fields pooled by the gather's device code (a max pool's
 *   arg-max byte goes to ext->amax at am_wide_off[f]).  y [B]; z [B, ld_z >= H] keeps the H logits for the backward.
 *   err: bit 0 is set when an id falls outside [0, vocab); such a row reads as row 0 (nullable).  ids_t / parts_t / units /
 *   n_units: the side outputs of dctr_embed_fwd for the sorted update (nullable; NULL for a plan with ext).  Nothing of
 *   size [B, n_wide] is written.  A sample's y and z depend neither on B nor on its position in the batch.
 * backward (recomputes s, l, c from z), g = g_y[b]:
 *   g_z[b, r] = g * c * (s_r (l_r - p0) + s_r l_r (1 - l_r))   (regression: the second term is s_r)
 *   g_z[b, R] = g * p0 * c * (1 - c)
 *   g_wide[b * ld_gw + f] = g_z[b, head_of[f]] for f < n_wide, g_wide[b * ld_gw + n_wide] = 0 (ld_gw >= n_wide + 1): the
 *   per-field layout dctr_embed_update / _update_lazy / _bwd read (nullable when n_wide = 0)
 *   g_dense[j] = sum_b g_z[b, head(j)] * X[b, dense_cols[j]]  for j < n_dense (nullable when n_dense = 0): per-tile partials
 *   in ws (dctr_mlr_bwd_workspace_floats(mlr, B) floats), added in tile order by a second launch.  No atomics: every
 *   output is bit-identical run to run.
 * dctr_mlr_supported: 1 when both entry points take (plan, mlr); they return DCTR_ENOSUP otherwise: a deep side or a dense
 * block, no DCTR_PLAN_WIDE_PER_FIELD, wdense_w, out_chunks, n_regions outside [2, 16], a tile beyond the LDS.          */
#define DCTR_MLR_BINARY 0
#define DCTR_MLR_REGRESSION 1
#define DCTR_MLR_MAX_REGIONS 16
typedef struct {
  const int32_t* head_of;      /* device [n_wide]                                                                     */
  const int32_t* dense_cols;   /* device [n_dense]: X columns of every head's dense features, head after head         */
  const int32_t* dense_off;    /* device [H + 1]: head h owns dense_cols[dense_off[h] .. dense_off[h + 1])             */
  const float* const* dense_w; /* device [H]: each head's Linear.weight (separate parameters; NULL without dense cols) */
  int32_t n_regions, has_bias, task, n_dense;
} dctr_mlr_t;
size_t dctr_sizeof_mlr(void);
int dctr_mlr_supported(const dctr_plan_t* plan, const dctr_mlr_t* mlr);
int dctr_mlr_fwd(const dctr_plan_t* plan, const dctr_mlr_t* mlr, const float* X, int64_t ldx, int32_t B, float* y, float* z,
                 int64_t ld_z, int32_t* err, int32_t* ids_t, uint16_t* parts_t, const int32_t* units, int32_t n_units,
                 dctr_stream_t stream);
size_t dctr_mlr_bwd_workspace_floats(const dctr_mlr_t* mlr, int32_t B);
int dctr_mlr_bwd(const dctr_plan_t* plan, const dctr_mlr_t* mlr, const float* X, int64_t ldx, int32_t B, const float* g_y,
                 const float* z, int64_t ld_z, float* g_wide, int64_t ld_gw, float* g_dense, float* ws,
                 dctr_stream_t stream);

/* ---- AFMLayer (interaction.py:251-325): attentional pooling of the pairwise products (csrc/afm.hip) -----------
 *   bi_k = e_i (.) e_j (pairs i < j, itertools.combinations order);  t_k = relu(bi_k W + bias);  s_k = t_k . h;
 *   a = softmax_k(s);  out = sum_k a_k bi_k;  y[b] = out . p
 *   E [B, F, D] rows at E + b*ld_e;  W [D, A] (attention_W), bias [A] (attention_b), h [A] (projection_h), p [D]
 *   (projection_p).  One wave per sample, everything between E and y stays in LDS.  The backward recomputes the
 *   forward, writes gE [B, F*D] rows at gE + b*ld_ge and the four parameter gradients (fixed-order sums, no
 *   atomics); workspace: dctr_afm_bwd_workspace_floats(B, D, A) floats.  Needs D <= 64, A <= 32, F <= 64.      */
size_t dctr_afm_bwd_workspace_floats(int32_t B, int32_t D, int32_t A);
int dctr_afm_fwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t A, const float* W,
                 const float* bias, const float* h, const float* p, float* y, dctr_stream_t stream);
int dctr_afm_bwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t A, const float* W,
                 const float* bias, const float* h, const float* p, const float* gy, float* gE, int64_t ld_ge,
                 float* gW, float* gbias, float* gh, float* gp, float* workspace, dctr_stream_t stream);

/* ---- ConvLayer of CCPM (interaction.py:675-717: Conv2dSame / Tanh / KMaxPooling per layer; csrc/ccpm.hip) -------
 * Layers i = 1..n_layers on one sample's image x [C_{i-1}][n_{i-1}][D];  C_0 = 1, C_i = filters[i-1];  n_0 = F, n_i = k[i-1]:
 *   a[co, f, d] = bias[co] + sum_ci sum_t W[co, ci, t] * x[ci, f + t - top, d]      w = width[i-1], top = (w - 1) / 2
 *                 (cross-correlation; rows outside [0, n_{i-1}) are 0: top zero rows above, w - 1 - top below)
 *   y = tanh(a);  per column (co, d) the k_i largest y over f, in descending order (torch.topk(sorted=True)).
 *   TIE RULE: equal values keep their field order, the lower index first (the reference leaves ties unspecified).
 * E [B, F, D] rows at E + b*ld_e;  out [B, C_L * k_L * D] ([C_L][k_L][D] per sample) rows at out + b*ld_out.
 * width / filters / k are HOST arrays of n_layers entries, 1 <= k[i-1] <= n_{i-1}.  params is one device vector: layer 1
 * weight [C_1, C_0, w_1] (the nn.Conv2d weight), layer 1 bias [C_1], layer 2 weight, ...; g_params has the same layout.
 * sel: one byte per pooled element of every layer, [B][sum_i C_i * k_i * D] (per sample: layer 1 [C_1][k_1][D], layer 2,
 * ...), the row f each pooled element came from; the forward writes it when the pointer is not NULL.  The backward routes
 * the gradient by sel and recomputes the selected activations from E; nothing else is saved.  It writes gE [B, F*D] rows
 * at gE + b*ld_ge and g_params (fixed-order sums, no atomics: identical bits from run to run); workspace:
 * dctr_ccpm_bwd_workspace_floats(B, n_params) floats, n_params = sum_i (C_i * C_{i-1} * w_i + C_i).
 * One wave per sample, everything between E and out stays in LDS.  B == 0 returns DCTR_OK before any buffer check.
 * DCTR_ENOSUP unless F <= 64, D <= 64, n_layers <= 4, C_i <= 16, w_i <= 16 and both per-sample LDS images fit 64 KB (two or
 * more workgroups per CU), with img_i = C_i * n_i * D, max_img = max_{i>=0} img_i, max_act = max_{i>=1} C_i * n_{i-1} * D:
 *   forward   4 * (n_params + max_img + max_act)
 *   backward  4 * (2 * n_params + sum_{i>=0} img_i + 2 * max_img) + sum_{i>=1} img_i                                    */
size_t dctr_ccpm_bwd_workspace_floats(int32_t B, int32_t n_params);
int dctr_ccpm_fwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t n_layers, const int32_t* width,
                  const int32_t* filters, const int32_t* k, const float* params, float* out, int64_t ld_out, uint8_t* sel,
                  dctr_stream_t stream);
int dctr_ccpm_bwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t n_layers, const int32_t* width,
                  const int32_t* filters, const int32_t* k, const float* params, const uint8_t* sel, const float* g_out,
                  int64_t ld_gout, float* gE, int64_t ld_ge, float* g_params, float* workspace, dctr_stream_t stream);

/* ---- LogTransformLayer of AFN (interaction.py:720-757; csrc/log_transform.hip) -------------------------------------
 * X [B, F, E] rows at X + b*ld_e (element (f, e) at f*E + e), W [F, H], bias [H], two BatchNorm1d(E) (eps 1e-5):
 *   a[b,e,f] = log(max(|X[b,f,e]|, 1e-7f))
 *   n[b,e,f] = bn0_w[e] * (a - mean0[e]) / sqrt(var0[e] + eps) + bn0_b[e]          statistics per e over (b, f)
 *   z[b,e,h] = sum_f n[b,e,f] * W[f,h] + bias[h]        y = exp(z)
 *   out[b, e*H + h] = bn1_w[e] * (y - mean1[e]) / sqrt(var1[e] + eps) + bn1_b[e]   statistics per e over (b, h)
 * fwd_train: the statistics are the batch's (mean and BIASED variance, held to float64: per-workgroup (count, mean, M2)
 *   merged by Chan's formula) and are returned in stats [4][E] = mean0 | var0 | mean1 | var1 as DOUBLES -- what is left
 *   of a gradient after BatchNorm's backward projection is eps / (var + eps) of its terms, so a float rstd would move it
 *   by 1e-7 / that; the kernels normalise in double.  The caller applies torch's running-statistics rule.  Three launches: BN0 partials; BN1 partials from a recomputed y that is never written; out.
 * fwd_eval: one launch on the statistics handed in (the running ones).
 * bwd (of fwd_train, given its stats): with yhat = (y - mean1) / sqrt(var1 + eps), N1 = B*H, N0 = B*F, g = g_out:
 *   g_bn1_b[e] = sum g          g_bn1_w[e] = sum g * yhat                                            over (b, h)
 *   gz = bn1_w * rstd1 * (g - g_bn1_b / N1 - yhat * g_bn1_w / N1) * y
 *   gbias[h] = sum_{b,e} gz     gW[f,h] = sum_{b,e} n * gz     gn[b,e,f] = sum_h gz * W[f,h]
 *   g_bn0_b[e] = sum gn         g_bn0_w[e] = sum gn * nhat      (nhat = (a - mean0) * rstd0)          over (b, f)
 *   ga = bn0_w * rstd0 * (gn - g_bn0_b / N0 - nhat * g_bn0_w / N0)
 *   gX[b,f,e] = ga / X[b,f,e] where |X| >= 1e-7f, 0 elsewhere        (rows at gX + b*ld_gx)
 *   Three launches; g_out (rows at g_out + b*ld_g) is read twice, y is recomputed, nothing else of its size is touched.
 * Every cross-workgroup sum is a fixed-order sum of per-workgroup partials (no atomics): identical bits run to run.
 * workspace: dctr_log_transform_workspace_floats(B, F, E, H) floats (covers both directions; nothing is carried from the
 * forward to the backward in it), 8-byte aligned (DCTR_EALIGN): the partials are doubles.  B == 0 returns DCTR_OK (the backward zeroes the parameter gradients).
 * DCTR_ENOSUP unless 1 <= F <= 64, 1 <= E <= 64, 1 <= H <= 1024.  A workgroup (256 threads) owns one e, 32 samples at a
 * time and 128 columns of H; static LDS: W slice 64 x 128 floats (32 KB) + n tile 32 x 65 (8.1 KB) + bias 0.5 KB forward,
 * plus a second 32 x 65 tile and gz 32 x 129 (16.1 KB) in the backward's main pass: 41 KB / 66 KB, whatever the shape. */
size_t dctr_log_transform_workspace_floats(int32_t B, int32_t F, int32_t E, int32_t H);
int dctr_log_transform_fwd_train(const float* X, int64_t ld_e, int32_t B, int32_t F, int32_t E, int32_t H, const float* W,
                                 const float* bias, const float* bn0_w, const float* bn0_b, const float* bn1_w,
                                 const float* bn1_b, float* out, int64_t ld_out, double* stats, float* workspace,
                                 dctr_stream_t stream);
int dctr_log_transform_fwd_eval(const float* X, int64_t ld_e, int32_t B, int32_t F, int32_t E, int32_t H, const float* W,
                                const float* bias, const float* bn0_w, const float* bn0_b, const float* bn0_mean,
                                const float* bn0_var, const float* bn1_w, const float* bn1_b, const float* bn1_mean,
                                const float* bn1_var, float* out, int64_t ld_out, dctr_stream_t stream);
int dctr_log_transform_bwd(const float* X, int64_t ld_e, int32_t B, int32_t F, int32_t E, int32_t H, const float* W,
                           const float* bias, const float* bn0_w, const float* bn0_b, const float* bn1_w,
                           const double* stats, const float* g_out, int64_t ld_g, float* gX, int64_t ld_gx, float* gW,
                           float* gbias, float* g_bn0_w, float* g_bn0_b, float* g_bn1_w, float* g_bn1_b, float* workspace,
                           dctr_stream_t stream);

/* ---- AttentionSequencePoolingLayer of DIN / DIEN (sequence.py:80-154 over core.py:10-64; csrc/din.hip) -----------------
 * Per sample, with query q [E], keys k_t [E] (t < T), hidden layers l = 1..n_layers of hidden[l-1] units:
 *   x_t = [q, k_t, q - k_t, q * k_t]   a_0 = x_t   a_l = act(W_l a_{l-1} + b_l)   s_t = dense.w . a_L + dense.b
 *   softmax == 0:  w_t = s_t on valid positions, 0 elsewhere: an invalid position contributes nothing and gets no gradient
 *   softmax != 0:  invalid scores are -2^32 + 1 before the softmax: weight exactly 0 whenever one position is valid; a
 *                  sample WITHOUT a valid position gets w_t = 1/T on all T keys, its key gradient is g / T and nothing
 *                  flows from it to the scores or the parameters
 *   out = sum_t w_t k_t.  Invalid positions are never evaluated (every position is independent).
 * Addressing, n_seg <= 4 segments of dim[j] floats, E = sum_j dim[j] (dim, q_off, k_off, k_step: HOST arrays):
 *   q(b, j) = Q + b*ld_q + q_off[j]        k(b, t, j) = K + b*ld_k + k_off[j] + t*k_step[j]        out + b*ld_out [E]
 *   (one contiguous [B, T, E]: n_seg = 1, k_step = E; the model's gathered row: k_step[j] = dim[j], Q == K allowed).
 * Validity from exactly ONE of len [B] int32 (t valid iff t < len[b]; above T: all, 0 or less: none) and mask [B, T] bytes
 * (non-zero = valid); the other pointer is NULL.
 * act: 0 linear, 1 relu, 2 sigmoid, 3 prelu (one slope per layer), 4 frozen Dice, FORWARD ONLY (the backward returns
 * DCTR_ENOSUP): a = z * (alpha + (1 - alpha) * sigmoid(s*z + t)) per unit, s and t folded from BatchNorm's running
 * statistics, affine pair and eps.  Dice with batch statistics is not in the kernel.
 * params, one device vector (g_params likewise): per hidden layer W [H_l, in_l] row-major (in_1 = 4E, in_l = H_{l-1}),
 * b [H_l], then the activation's own (prelu: slope [1]; Dice: alpha [H_l] | s [H_l] | t [H_l]; else nothing); then
 * dense.weight [H_L], dense.bias [1].
 * weights [B, T] (contiguous): the w_t; the forward writes them when the pointer is not NULL, the backward needs them and
 * recomputes everything else from Q, K and params.  The backward writes every element of every q segment at
 * gQ + b*ld_gq + q_off[j] and of every k segment at gK + b*ld_gk + k_off[j] + t*k_step[j] (zeros at invalid positions
 * included), nothing outside the segments, and g_params: fixed-order sums, no atomics, identical bits from run to run.
 * workspace: dctr_din_attn_bwd_workspace_floats(B, n_params) floats.
 * DCTR_ENOSUP (dctr_din_attn_supported == 0) unless E <= 64, 1 <= T <= 128 (= DCTR_MAX_UNIT_SLOTS: a model whose history
 * shares its table with the query column is bounded by T <= 127), n_seg <= 4, 1 <= n_layers <= 3, hidden[l] <= 128.  No
 * further LDS condition: 32 (forward) / 16 (backward) valid positions are in LDS at a time, which at the largest shape is
 *   forward   4 * (11 E + 3 T + 1 + 32 (E + 1 + sum_l (H_l + 1)))                                           <= 62.3 KB
 *   backward  4 * (9 E + 5 T + 1 + 16 (2 E + 1 + sum_l (H_l + 1) + 3 (max_l H_l + 1)) + max_l H_l)         <= 63.2 KB
 * B == 0 returns DCTR_OK before any buffer check.                                                                          */
int dctr_din_attn_supported(int32_t T, int32_t n_seg, const int32_t* dim, int32_t n_layers, const int32_t* hidden,
                            int32_t act);
size_t dctr_din_attn_bwd_workspace_floats(int32_t B, int32_t n_params);
int dctr_din_attn_fwd(const float* Q, int64_t ld_q, const float* K, int64_t ld_k, int32_t B, int32_t T, int32_t n_seg,
                      const int32_t* dim, const int64_t* q_off, const int64_t* k_off, const int64_t* k_step,
                      const int32_t* len, const uint8_t* mask, int32_t n_layers, const int32_t* hidden, int32_t act,
                      int32_t softmax, const float* params, float* out, int64_t ld_out, float* weights,
                      dctr_stream_t stream);
int dctr_din_attn_bwd(const float* Q, int64_t ld_q, const float* K, int64_t ld_k, int32_t B, int32_t T, int32_t n_seg,
                      const int32_t* dim, const int64_t* q_off, const int64_t* k_off, const int64_t* k_step,
                      const int32_t* len, const uint8_t* mask, int32_t n_layers, const int32_t* hidden, int32_t act,
                      int32_t softmax, const float* params, const float* weights, const float* g_out, int64_t ld_gout,
                      float* gQ, int64_t ld_gq, float* gK, int64_t ld_gk, float* g_params, float* workspace,
                      dctr_stream_t stream);

/* ---- Variable-length GRU / AIGRU / AGRU / AUGRU of DIEN (dien.py:181-381, sequence.py's AGRUCell / AUGRUCell / DynamicGRU,
 * torch.nn.GRU on packed sequences; csrc/gru_seq.hip) -------------------------------------------------------------------
 * Per sample b, with n = clamp(len[b], 0, T), h_0 = 0 and, for t < n, x_t = X(b, t) (mode 1: x_t = a_t * X(b, t)):
 *   r = sigmoid(W_ir x_t + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x_t + b_iz + W_hz h + b_hz)
 *   c = tanh(W_in x_t + b_in + r * (W_hn h + b_hn))
 *   mode 0 GRU, 1 AIGRU:  h' = (1 - z) * c + z * h                          (torch.nn.GRU's convention)
 *   mode 2 AGRU:          h' = (1 - a_t) * h + a_t * c                      (z unused: its rows of g_params are exactly 0)
 *   mode 3 AUGRU:         u = a_t * z;  h' = (1 - u) * h + u * c            (the opposite convention from nn.GRU)
 * One launch per direction (the backward is followed by a fixed-order reduction); no length ever travels to the host.
 * len [B] int32 on the device: above T counts as T, 0 or less means no step (dctr_din_attn_fwd's conventions).
 * Addressing as for the attention's keys, n_seg <= 4 segments of dim[j] floats, H = sum_j dim[j] (input size == hidden
 * size; dim, x_off, x_step: HOST arrays):   x(b, t, j) = X + b*ld_x + x_off[j] + t*x_step[j]
 *   (the gathered row read in place: x_step[j] = dim[j]; one contiguous [B, T, H]: n_seg = 1, x_step = H, ld_x = T*H).
 * The segments' elements must be pairwise distinct addresses (segments may interleave, not overlap): this is the caller's
 * to guarantee and is not checked; the backward writes every element of gX once, and an overlap would be two writers.
 * params, one device vector of 6 H^2 + 6 H floats (g_params likewise): W_ih [3H, H] | W_hh [3H, H] | b_ih [3H] | b_hh [3H],
 * gate order r, z, n as in torch.  att [B, T] contiguous: required in modes 1 to 3, ignored (NULL) in mode 0.
 * Forward outputs, either of which may be NULL (not both): states(b, t, :) = states + b*ld_states + t*H, h_{t+1} for
 * t < n and exact zeros for t >= n (pad_packed_sequence's padding), ld_states >= T*H;  last + b*ld_last [H] = h_n (zero
 * for n = 0).  gates [B, T, 4, H] contiguous or NULL: r, z, c and W_hn h + b_hn of every evaluated step, 16 T H bytes per
 * sample -- what a backward needs beside `states` (both must then be non-NULL in the forward); positions t >= n are not
 * written and never read.
 * The backward takes g_states (same layout, row stride ld_gstates; values at t >= n are ignored) and / or g_last, and
 * recomputes nothing.  It writes gX with X's addressing (row stride ld_gx): every element of every segment, zeros at
 * t >= n, nothing outside the segments; g_att [B, T] in modes 1 to 3 (zeros at t >= n; NULL allowed in mode 0); g_params:
 * every thread owns elements of W_ih / W_hh and adds step after step, sample after sample, the workgroups' rows are added
 * in order -- no atomics, identical bits from run to run.  workspace: dctr_gru_seq_bwd_workspace_floats(B, H) floats.
 * DCTR_ENOSUP (dctr_gru_seq_supported == 0) unless H <= 64, 1 <= T <= 128, n_seg <= 4.  The bound on T a MODEL meets first
 * is DCTR_MAX_UNIT_SLOTS: history (and, under negative sampling, negative history) positions share the candidate's table,
 * one update slot each plus the candidate's own, so T <= 127 without and 2 T + 1 <= 128, T <= 63, with negative sampling.
 * H need not be a multiple of 4.  A missing att in modes 1 to 3 is DCTR_EINVAL.  B == 0 returns DCTR_OK before any buffer
 * check (the backward then zeroes g_params when the shape is valid).                                                       */
int dctr_gru_seq_supported(int32_t T, int32_t n_seg, const int32_t* dim, int32_t mode);
size_t dctr_gru_seq_bwd_workspace_floats(int32_t B, int32_t H);
int dctr_gru_seq_fwd(const float* X, int64_t ld_x, int32_t B, int32_t T, int32_t n_seg, const int32_t* dim,
                     const int64_t* x_off, const int64_t* x_step, const int32_t* len, const float* att, int32_t mode,
                     const float* params, float* states, int64_t ld_states, float* last, int64_t ld_last, float* gates,
                     dctr_stream_t stream);
int dctr_gru_seq_bwd(const float* X, int64_t ld_x, int32_t B, int32_t T, int32_t n_seg, const int32_t* dim,
                     const int64_t* x_off, const int64_t* x_step, const int32_t* len, const float* att, int32_t mode,
                     const float* params, const float* states, int64_t ld_states, const float* gates,
                     const float* g_states, int64_t ld_gstates, const float* g_last, int64_t ld_glast, float* gX,
                     int64_t ld_gx, float* g_att, float* g_params, float* workspace, dctr_stream_t stream);

/* ---- Gate mix of the multi-task models (MMOE's gates, one CGC level of PLE; csrc/gate_mix.hip) ---------------------------
 * One launch per direction for ALL G gates that draw on one pool of P expert outputs x_e [B, dim] (rows at
 * x[e] + b*ld_x[e]).  Gate g reads h_g [B, H_g] (rows at h + b*ld_h), the bias-free weight W_g [n_g, H_g] (rows at
 * W + j*ld_w) and n_g indices member[0..n_g) into the pool (repeats allowed), in the order of the mix:
 *   z[j] = h_g[b] . W_g[j]        w = softmax(z) (maximum subtracted first)        out_g[b, :] = sum_j w[j] x_{member[j]}[b, :]
 * The forward writes out_g [B, dim] (rows at out + b*ld_out) and, when w is not NULL, the weights w_g [B, n_g] (contiguous).
 * Nothing of size [B, n, dim] exists; an expert row is read once per sample for all the gates that use it.
 * The backward needs w of the forward and takes g_out_g [B, dim] (rows at g_out + b*ld_gout) per gate.  It writes
 *   g_x[e][b, :] = sum over the gates that use e, in gate order, of (sum_{j: member[j] == e} w_g[b, j]) * g_out_g[b, :]
 *                  -- every element of every pool member, one writer each, no atomics (zeros for an unused member);
 *   g_h_g[b, :]  = sum_j dz[j] W_g[j, :],   dz[j] = w[j] * (s[j] - sum_k w[k] s[k]),   s[j] = g_out_g[b] . x_{member[j]}[b]
 *                  (rows at g_h + b*ld_gh; two gates that read one h get one buffer each);
 *   gW_g[j, :]   = sum_b dz[j] h_g[b, :]   as [n_g, ld_w]: columns H_g .. ld_w are written as 0.  Every workgroup keeps its
 *                  partial sums in registers, writes them to the workspace once, and a second kernel adds them in workgroup
 *                  order: identical bits from run to run.
 * A gate whose g_out is NULL (nothing downstream used its output) adds nothing to any g_x; its g_h and gW are zeros.
 * n_g == 1 is legal: the weight is 1, dz is 0.
 * workspace: dctr_gate_mix_bwd_workspace_floats(B, G, n, ld_w) floats (n, ld_w: HOST arrays of G entries).
 * DCTR_ENOSUP (dctr_gate_mix_supported == 0) unless 1 <= P <= 32, 1 <= G <= 8, 1 <= n_g <= 16, dim <= 1152, H_g <= 1152
 * -- every combination inside these bounds runs; there is no LDS condition (the backward stages 16 KB, the forward none).
 * B == 0 returns DCTR_OK before any buffer check and touches nothing.                                                     */
#define DCTR_GATE_MAX_GATES 8
#define DCTR_GATE_MAX_MEMBERS 16
#define DCTR_GATE_MAX_POOL 32
#define DCTR_GATE_MAX_WIDTH 1152
typedef struct {
  const float* h;      /* [B, H] gate input                                  */
  const float* W;      /* [n, H] rows at W + j*ld_w                          */
  float* out;          /* fwd: [B, dim]                                      */
  float* w;            /* fwd: [B, n] contiguous or NULL; bwd: read          */
  const float* g_out;  /* bwd: [B, dim] or NULL                              */
  float* g_h;          /* bwd: [B, H]                                        */
  float* gW;           /* bwd: [n, ld_w]                                     */
  int64_t ld_h, ld_w, ld_out, ld_gout, ld_gh;
  int32_t H, n;
  int32_t member[DCTR_GATE_MAX_MEMBERS];
} dctr_gate_t;
size_t dctr_sizeof_gate(void);
int dctr_gate_mix_supported(int32_t P, int32_t dim, int32_t G, const int32_t* n, const int32_t* H);
size_t dctr_gate_mix_bwd_workspace_floats(int32_t B, int32_t G, const int32_t* n, const int32_t* ld_w);
int dctr_gate_mix_fwd(const float* const* x, const int64_t* ld_x, int32_t P, int32_t dim, int32_t B,
                      const dctr_gate_t* gates, int32_t G, dctr_stream_t stream);
int dctr_gate_mix_bwd(const float* const* x, const int64_t* ld_x, int32_t P, int32_t dim, int32_t B,
                      const dctr_gate_t* gates, int32_t G, float* const* g_x, const int64_t* ld_gx, float* workspace,
                      dctr_stream_t stream);

/* ---- InteractingLayer of AutoInt (interaction.py:328-394): multi-head self-attention over the fields (csrc/interact.hip)
 *   Q = E Wq, K = E Wk, V = E Wv;  head n = columns [n*A, (n+1)*A), A = D / H;  P_n = softmax_rows(Q_n K_n^T (/ sqrt(A)
 *   when scaling));  out = relu([P_0 V_0 | ... | P_{H-1} V_{H-1}] + E Wr)          (Wr = NULL: no residual)
 *   E [B, F, D] rows at E + b*ld_e;  W* [D, D] row-major (x @ W);  out [B, F*D] rows at out + b*ld_o.
 * One wave per sample, everything between E and out stays in LDS; the backward recomputes the forward, writes gE and
 * the four weight gradients (fixed-order sums, no atomics); workspace: dctr_interacting_bwd_workspace_floats(B, D).
 * dctr_interacting_supported(F, D, H) != 0 iff the shape fits (D <= 32, F <= 64, LDS).                               */
int dctr_interacting_supported(int32_t F, int32_t D, int32_t H);
size_t dctr_interacting_bwd_workspace_floats(int32_t B, int32_t D);
int dctr_interacting_fwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t H, int32_t scaling,
                         const float* Wq, const float* Wk, const float* Wv, const float* Wr, float* out, int64_t ld_o,
                         dctr_stream_t stream);
int dctr_interacting_bwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t H, int32_t scaling,
                         const float* Wq, const float* Wk, const float* Wv, const float* Wr, const float* gout,
                         int64_t ld_g, float* gE, int64_t ld_ge, float* gWq, float* gWk, float* gWv, float* gWr,
                         float* workspace, dctr_stream_t stream);

/* ---- lazy regularised / Adam embedding update (csrc/lazy.hip) -------------------------------------------------
 * Replaces, without the O(vocabulary) memory traffic, what the reference does whenever every row of a table moves at
 * every step: the dense L2 gradient 2*lambda*w of get_regularization_loss (basemodel.py:412-428; l2_reg_embedding /
 * l2_reg_linear default to 1e-5) and torch.optim.Adam's moment-driven updates of untouched rows
 * (basemodel.py:447-461).  A row's trajectory between two batches that touch it depends on the row alone, so it is
 * replayed -- the same recurrence, step by step -- when the row is next needed.  One "unit" = one id column of X with
 * the deep and / or wide table it feeds (as in dctr_embed_update); `stamp[row]` = optimizer steps already applied
 * to the row, `*step` (device) = steps completed so far.  Per train step the caller enqueues
 *   dctr_embed_ids -> dctr_lazy_catchup -> dctr_embed_fwd -> ... -> dctr_embed_update(DCTR_UPD_ACCUM)
 *   -> dctr_lazy_apply -> dctr_lazy_step_inc,
 * and dctr_lazy_flush before anything else reads the tables (predict / evaluate / state_dict).
 * dctr_lazy_sweep (optional, once per step) goes BEHIND the catch-up -- never beside it: sweep and catch-up read and write
 * the stamps non-atomically and skip a row only when its stamp is already current, so a sweep that overlaps a catch-up
 * replays rows twice -- and must have finished before dctr_lazy_step_inc (it reads the step counter).  Between the two it
 * may run on a stream of its own beside the gather, the tower, the update and dctr_lazy_apply: they touch the batch's
 * rows, which the catch-up has stamped current and the sweep therefore skips.
 *   *_s1  Adagrad `sum` | Adam `exp_avg`     *_s2  Adam `exp_avg_sq`     *_g  gradient slab, zero at rest
 *   vec   1 or 4: every deep dim and base pointer is a multiple of `vec` floats;  max_dim <= 64*vec                */
#define DCTR_LAZY_SGD 0
#define DCTR_LAZY_ADAGRAD 1
#define DCTR_LAZY_ADAM 2
#define DCTR_LAZY_RMSPROP 3 /* torch.optim.RMSprop (momentum 0, not centered): s1 = square_avg, beta2 = alpha,  */
                            /* beta1 = 1 - alpha.  A row no sample refers to still has its square_avg decayed at */
                            /* every step: replayed like Adam's moments                                          */
typedef struct dctr_lazy_unit {
  float* deep;    /* [vocab, dim] (rows ld_deep floats apart) or NULL */
  float* deep_s1; /* rows ld_deep_s1 floats apart; deep_s2 / deep_g are contiguous */
  float* deep_s2;
  float* deep_g;
  float* wide;    /* [vocab] or NULL */
  float* wide_s1;
  float* wide_s2;
  float* wide_g;
  int32_t* stamp; /* [vocab] */
  int64_t vocab;
  int32_t dim;
  int32_t col;
  float l2_deep;  /* lambda of the L2 term lambda * sum(w^2) on the deep table */
  float l2_wide;
  int32_t ld_deep, ld_deep_s1; /* row strides in floats, 0 = dim */
  int32_t ld_wide, ld_wide_s1; /* row strides in floats, 0 = 1   */
} dctr_lazy_unit_t;
typedef struct dctr_lazy_opt {
  int32_t kind; /* DCTR_LAZY_* */
  float lr, eps, beta1, beta2;
  /* Adam only, optional (NULL: the kernels compute the scalars themselves, in double, per step and lane): DEVICE tables of
   * the step-dependent scalars torch.optim.Adam computes on the host (adam.py: bias_correction = 1 - beta ** step),
   *   adam_ss[T - 1] = (float)(lr / (1 - beta1^T))     adam_bc[T - 1] = (float)sqrt(1 - beta2^T)      T = 1 .. n
   * each long enough that its last entry is the limit (1 - beta^T == 1 in double: 358 / 37 414 entries at the default
   * betas as LazyState.adam_tables builds them): steps past the end read the last entry -- adam_ss[min(T, n_ss) - 1],
   * adam_bc[min(T, n_bc) - 1]; the two lengths differ.  A row that slept k steps replays k optimizer steps in its catch-up:
   * the tables take two double multiplies, a division and a square root per replayed step and lane out of that loop.   */
  int32_t n_ss, n_bc;
  int32_t any_l2; /* some unit carries an L2 term (SGD / Adagrad rows then move between two touches: the catch-up has steps
                     to replay and orders its entries by gap) */
  const float* adam_ss;
  const float* adam_bc;
  const float* adam_rbc; /* optional (ABI 24), n_bc entries: (float)(1 / sqrt(1 - beta2^T)) -- the replay loop divides by
                            adam_bc[T - 1] through this reciprocal; NULL: it takes the hardware reciprocal of adam_bc itself,
                            one quarter-rate instruction per replayed step and wavefront */
  float beta1_c, beta2_c; /* optional (ABI 35), Adam: (float)(1 - beta1), (float)(1 - beta2) rounded from DOUBLE, the scalars
                             torch.optim.Adam hands its kernels (lerp weight, addcmul value).  0: the kernels use
                             1.f - beta1 / 1.f - beta2 as before -- float(0.999) is 1.3e-8 off 0.999, so that 1.f - beta2 is
                             1.3e-5 (relative) off 0.001: the same in every increment of exp_avg_sq */
} dctr_lazy_opt_t;
size_t dctr_sizeof_lazy_unit(void);
/* Round 6 -- the step that carries the batch's DATA gradient, inside the sorted update: dctr_embed_update's gradient sums
 * (same arguments, same order of additions) meet g = G + 2 lambda w and ONE optimizer step of `lazy_opt` on (w, s1, s2) at the
 * row, which is stamped t + 1 (*step = t is read, not advanced: dctr_lazy_step_inc follows as before).  Replaces
 * dctr_embed_update(DCTR_UPD_ACCUM) + dctr_lazy_apply -- no gradient slab, no second pass over the batch's rows.  Needs what
 * csrc/lazy.hip needs (simple units, the batch's rows caught up to t by dctr_lazy_catchup) and pre-sorted entries
 * (dctr_embed_segments on the same ids: `workspace`); DCTR_ENOSUP otherwise -- the caller keeps the two-pass route.       */
int dctr_embed_update_lazy(const dctr_plan_t* plan, const int32_t* units, int32_t n_units, int64_t max_vocab,
                           const int32_t* ids_t, const uint16_t* parts_t, int32_t B, const float* g_out, int64_t ld_g,
                           const float* out, int64_t ld_out, const float* fm_s, int64_t ld_s, const float* g_fm,
                           const float* g_wide, int64_t ld_gw, const float* X, int64_t ld_x, float* g_wdense,
                           int32_t* workspace, int64_t workspace_ints, const struct dctr_lazy_unit* lazy_units,
                           const int32_t* step, const struct dctr_lazy_opt* lazy_opt, dctr_stream_t stream);
size_t dctr_sizeof_lazy_opt(void);
/* order_ws (nullable): n_units * B ints of scratch -- with it the catch-up first deals every unit's entries by the number of
 * steps their rows slept (one launch, a counting sort per unit), so that the rows one wavefront replays side by side need
 * about the same number of steps: geometric gaps otherwise leave a wave waiting for its longest row (3.4 x the mean of 16).
 * The ordering pass runs for 64 <= B <= 2^18 and an optimizer with steps to replay (Adam, RMSprop; SGD / Adagrad only with
 * any_l2): it then writes a permutation of 0 .. B-1 per unit; otherwise order_ws is left untouched.  Results do not depend
 * on it. */
int dctr_lazy_catchup(const dctr_lazy_unit_t* units, int32_t n_units, const int32_t* ids_t, int32_t B,
                      const int32_t* step, const dctr_lazy_opt_t* opt, int32_t vec, int32_t max_dim,
                      int32_t* order_ws, dctr_stream_t stream);
int dctr_lazy_apply(const dctr_lazy_unit_t* units, int32_t n_units, const int32_t* ids_t, int32_t B,
                    const int32_t* step, const dctr_lazy_opt_t* opt, int32_t vec, int32_t max_dim,
                    dctr_stream_t stream);
int dctr_lazy_flush(const dctr_lazy_unit_t* units, int32_t n_units, int64_t max_vocab, const int32_t* step,
                    const dctr_lazy_opt_t* opt, int32_t vec, int32_t max_dim, dctr_stream_t stream);
/* dctr_lazy_sweep: bring the (*step mod K)-th of K windows of every table's rows ([w * ceil(vocab / K), ...)) to the current
 * step -- the flush of one K-th of the rows, called once per train step BEHIND the catch-up (see above).  No row then sleeps
 * longer than K steps: a row's replay is a sequential loop over its missed steps, so without the sweep a rarely drawn id
 * stalls the step it finally appears in for its whole history (one lane group, gap x ~0.5 us), and a flush after N steps
 * pays N steps for every row nobody drew.  The arithmetic is the same and each (row, step) is still applied exactly once,
 * in order: results are unchanged.  The window follows the device-side step counter: replayable from a hipGraph.           */
int dctr_lazy_sweep(const dctr_lazy_unit_t* units, int32_t n_units, int64_t max_vocab, int32_t K, const int32_t* step,
                    const dctr_lazy_opt_t* opt, int32_t vec, int32_t max_dim, dctr_stream_t stream);
int dctr_lazy_step_inc(int32_t* step, dctr_stream_t stream);
/* The same optimizer step (number *step + 1) over a flat dense slab with an optional per-element lambda
 * (g = grad + 2*lambda*p): what torch.optim.SGD / Adagrad / Adam do to the dense parameters when the model carries
 * L2 terms (l2_reg_linear on Linear.weight, l2_reg_dnn) -- one launch, no dense autograd node for the L2 term.  */
int dctr_dense_opt_reg(float* p, const float* g, float* s1, float* s2, const float* lam, int64_t n,
                       const dctr_lazy_opt_t* opt, const int32_t* step, dctr_stream_t stream);

/* ---- CIN layer (interaction.py:207-248) on fp32 MFMA (csrc/cin.hip) -------------------------------
 * One Compressed-Interaction layer without ever materialising Z = H (x) X0:
 *     Y[b, o, d] = sum_{h, m} W[o, h*M + m] * H[b, h, d] * X0[b, m, d] + bias[o];   A = relu(Y) if relu
 *   H    [B, h, D]  rows at H  + b*ld_h   (previous layer's "next_hidden", or X0 for layer 0)
 *   X0   [B, M, D]  rows at X0 + b*ld_x0  (the field embeddings; a view of dctr_embed_fwd's `out`)
 *   W    [O, h*M]   conv1ds.<k>.weight with its trailing 1 squeezed;  bias [O] (nullable)
 *   A    [B, O, D]  rows at A + b*ld_a
 *   workspace  dctr_cin_workspace_floats(h, M, O) floats (the kernel's re-laid-out copy of W)
 * Needs M <= 32.  The split_half / sum over d / concat of the reference stay with the caller.
 * Backward, given gA = d loss / d A (and the saved A when relu):
 *   gH   [B, h, D]  (written)      gX0 [B, M, D] (accumulated: += when accumulate_x0 != 0)
 *   gW   [O, h*M]   (written)      gbias [O]     (written, nullable)
 * gA and A share the leading dimension ld_a.  The backward needs dctr_cin_bwd_workspace_floats(B, h, M, D, O)
 * floats of scratch: the weight gradient is a [O, h*M] x (B*D) GEMM whose batch reduction is split over
 * workgroups; their partial tiles go to the workspace and are summed in a fixed order (no atomics).
 * Both calls return DCTR_EINVAL for a leading dimension shorter than its row (ld_h < h*D, ld_x0 < M*D, ld_a < O*D,
 * ld_gh < h*D, ld_gx < M*D) and DCTR_ENOSUP for M > 32, before anything is launched.
 * The symmetric layer -- H == X0 as POINTERS, ld_h == ld_x0 and h == M: layer 1 of a CIN -- walks every unordered field
 * pair a <= b once, with the folded weight Wf[o, a, b] = W[o, a*M + b] + W[o, b*M + a] (a < b), W[o, a*M + a] (a == b).
 * With t(a, b)[n, d] = sum_o Wf[o, a, b] * gY[n, o, d] (gY = gA under the relu mask) and Hh = (M + 1) / 2:
 *     a <  Hh:   gH[n, a, d] += t(a, b) X0[n, b, d]      gX0[n, b, d] += t(a, b) X0[n, a, d]
 *     a >= Hh:   gH[n, b, d] += t(a, b) X0[n, a, d]      gX0[n, a, d] += t(a, b) X0[n, b, d]
 * (a pair a == b adds the same term to both).  Neither buffer is then a gradient by itself; gH + gX0 (gX0 without what
 * accumulate_x0 found there) is d loss / d X0 of the layer, which is what the caller adds up.  gW and gbias are as in
 * the general case.  The same values in two distinct buffers take the general kernels: gH = d loss / d H,
 * gX0 (+)= d loss / d X0.                                                                                            */
size_t dctr_cin_workspace_floats(int32_t h, int32_t M, int32_t O);
size_t dctr_cin_bwd_workspace_floats(int32_t B, int32_t h, int32_t M, int32_t D, int32_t O);
int dctr_cin_layer_fwd(const float* H, int64_t ld_h, const float* X0, int64_t ld_x0, const float* W,
                       const float* bias, int32_t B, int32_t h, int32_t M, int32_t D, int32_t O, int32_t relu,
                       float* A, int64_t ld_a, float* workspace, dctr_stream_t stream);
int dctr_cin_layer_bwd(const float* gA, const float* A, int64_t ld_a, int32_t relu, const float* H, int64_t ld_h,
                       const float* X0, int64_t ld_x0, const float* W, int32_t B, int32_t h, int32_t M, int32_t D,
                       int32_t O, float* gH, int64_t ld_gh, float* gX0, int64_t ld_gx, int32_t accumulate_x0,
                       float* gW, float* gbias, float* workspace, dctr_stream_t stream);

/* The layer's "direct connect" rows as xDeepFM consumes them (interaction.py:226-246: split / cat / sum(-1)):
 *   dctr_cin_pool_fwd: pooled[b * ld_pooled + o] = sum_d A[b, pool_from + o, d]   (A [B, O, D] contiguous; `pooled` may be
 *                      the layer's block of the CIN's [B, featuremap_num] output: no torch.cat behind the layers)
 *   dctr_cin_pool_bwd: gA[b, o, :] = (o < n_hidden ? g_hidden[b, o, :] : 0) + (o >= pool_from ? gp(b, o - pool_from) : 0)
 *                      g_hidden [B, n_hidden, D] contiguous (NULL = 0); gp(b, j) = g_pooled[b * ld_gp + j] (NULL = 0), or,
 *                      with w_head: g_pooled[b * ld_gp] * w_head[j] -- the backward of the bias-free 1-unit Linear xDeepFM
 *                      puts on the CIN output (xdeepfm.py:72, :97) folded in: g_pooled is then the logit's gradient.
 *                      split_half: pool_from == n_hidden (disjoint row sets); otherwise pool_from = 0 and every row below
 *                      n_hidden receives both terms (interaction.py:240-242).
 *                      A_relu (nullable, [B, O, D]): the layer's saved relu output -- gA is zeroed where it is not > 0, i.e.
 *                      the relu's backward is applied HERE and dctr_cin_layer_bwd is then called with relu = 0 (its two
 *                      kernels stage 16 gradient rows per memory round trip instead of 8 + 8 mask rows)               */
int dctr_cin_pool_fwd(const float* A, int32_t B, int32_t O, int32_t D, int32_t pool_from, float* pooled,
                      int64_t ld_pooled, dctr_stream_t stream);
int dctr_cin_pool_bwd(const float* g_hidden, const float* g_pooled, int64_t ld_gp, const float* w_head,
                      const float* A_relu, int32_t B, int32_t O, int32_t D, int32_t n_hidden, int32_t pool_from,
                      float* gA, dctr_stream_t stream);

/* out[b] = sum_j x[b * ld_x + j] * w[j]   (csrc/head.hip): nn.Linear(N, 1, bias=False) over narrow rows -- xDeepFM's
 * cin_linear (xdeepfm.py:72, :97).  One wave per row, fixed summation order.                                          */
int dctr_rows_dot(const float* x, int64_t ld_x, const float* w, int32_t B, int32_t N, float* out, dctr_stream_t stream);
/* out[j] = sum_b w[b] * x[b * ld_x + j]   (ABI 24): the weight gradient of that projection, g_w = g^T X -- torch.mm of a
 * [1, B] row with the [B, N] feature maps before (a 16 us library GEMM at B = 4096, N = 192).  Rows in groups of 32, the
 * groups' sums added in group order: deterministic.  workspace: dctr_relu_bwd_bias_workspace_floats(B, N) floats.   */
int dctr_rows_tdot(const float* x, int64_t ld_x, const float* w, int32_t B, int32_t N, float* out, float* workspace,
                   dctr_stream_t stream);

/* ---- SENET / Bilinear / InnerProduct (csrc/pairwise.hip) ----------------------------------------------
 * SENETLayer (interaction.py:93-101): z = mean_d E; a1 = relu(z W1^T); a = relu(a1 W2^T); V = E * a[:, :, None]
 *   E [B, F, D] rows at E + b*ld_e;  W1 [R, F], W2 [F, R] (excitation.0 / .2 weights);  V [B, F*D] contiguous;
 *   a [B, F] and a1 [B, R] are saved for the backward.  Backward writes gE [B, F*D], gW1, gW2
 *   (workspace: dctr_senet_bwd_workspace_floats(B, F, R) floats of per-workgroup partials, summed in fixed order). */
int dctr_senet_fwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, const float* W1, const float* W2,
                   int32_t R, float* V, float* a, float* a1, dctr_stream_t stream);
size_t dctr_senet_bwd_workspace_floats(int32_t B, int32_t F, int32_t R);
int dctr_senet_bwd(const float* gV, const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, const float* W1,
                   const float* W2, int32_t R, const float* a, const float* a1, float* gE, float* gW1, float* gW2,
                   float* workspace, dctr_stream_t stream);

/* BilinearInteraction (interaction.py:140-156): p_k = (x_i W_w^T) (.) x_j for the pairs k = (i, j), i < j.
 *   Wf    [n_w, D, D]  the nn.Linear weights stacked: n_w = 1 ("all"), F ("each", w = i), P ("interaction", w = k)
 *   sched [n_sched][4] int32 (device): {i, j, w, k}.  The FORWARD takes the entries in output order (k ascending, no
 *         idle entries, n_sched = P): the waves of a workgroup then write neighbouring pieces of a sample's row
 *         together.  The BACKWARD takes two tables: `sched` in round-robin-tournament order, `slots` entries per round,
 *         i = -1 for an idle slot (its data kernel lets four waves accumulate into LDS rows without conflicts: a round
 *         is a perfect matching of the fields), and `sched_k` in output order like the forward's (its weight kernel
 *         gives every wave 8 consecutive pairs, i.e. whole lines of the incoming gradient; NULL: `sched` is used).
 *         pair_w [P] int32: weight index of pair k
 *   V     optional second input (FiBiNET's SENET output, fibinet.py:82-83).  With V: out row =
 *         [ V pairs (P*D) | E pairs (P*D) ], else [ E pairs ].  `dense` (nullable): n_dense floats per sample copied
 *         to out[:, dense_off ...) so that `out` IS the reference's DNN input (fibinet.py:86-87).  D <= 16.
 *   backward: gout has out's layout; writes gE (and gV) [B, F*D] and gW [n_w, D, D];
 *         workspace = dctr_bilinear_bwd_workspace_floats(B, P, D) floats.                                     */
int dctr_bilinear_fwd(const float* E, int64_t ld_e, const float* V, int64_t ld_v, const float* Wf,
                      const int32_t* sched, int32_t n_sched, int32_t P, int32_t F, int32_t D, int32_t B, float* out,
                      int64_t ld_o, const float* dense, int64_t ld_d, int32_t n_dense, int32_t dense_off,
                      dctr_stream_t stream);
size_t dctr_bilinear_bwd_workspace_floats(int32_t B, int32_t P, int32_t D);
int dctr_bilinear_bwd(const float* E, int64_t ld_e, const float* V, int64_t ld_v, const float* Wf,
                      const int32_t* sched, int32_t n_sched, int32_t slots, const int32_t* pair_w, int32_t n_w,
                      int32_t P, int32_t F, int32_t D, int32_t B, const float* gout, int64_t ld_g, float* gE,
                      float* gV, float* gW, float* workspace, const int32_t* sched_k, int32_t n_sched_k,
                      dctr_stream_t stream);

/* FiBiNET's bilinear pairs TOGETHER WITH the first tower layer behind them, backward direction (fibinet.py:82-99:
 * dnn_input = [ Bilinear(senet) | Bilinear(raw) | dense ], h1 = act(W0 dnn_input + b0); core.py:123-133).  Replaces
 * `gout = gh W0` (a [B, 2 P D] slab) followed by dctr_bilinear_bwd: the gradient of a (16 samples x one pair) piece is
 * produced on the matrix cores where it is consumed, the slab is neither written nor read.
 *   gh     [B, H] at gh + b*ld_gh: gradient at the first layer's pre-activation (after the activation's backward)
 *   W0     [H, >= 2 P D] at W0 + h*ld_w0: the nn.Linear weight; columns [0, P D) belong to V's pairs, [P D, 2 P D) to E's
 *   sched4 [n_groups][8][4] int32 (device): groups of eight field-disjoint pairs {i, j, w, k} (one per wave of a
 *          512-thread workgroup), i = -1 for an idle entry
 *   writes gE, gV [B, F*D] and gW [n_w, D, D]; workspace = dctr_bilinear_wide_bwd_workspace_floats(B, P) floats.
 *   DCTR_ENOSUP unless D == 16, n_w == P (one weight per pair: "interaction"), H <= 128, H % 4 == 0, 16-byte aligned rows. */
size_t dctr_bilinear_wide_bwd_workspace_floats(int32_t B, int32_t P);
/* The same node, forward direction: h [B, H] = act(W0 x + b0) with the pairs of x made where they are consumed (no
 * [B, 2 P D + n_dense] x [.., H] library GEMM).  x (row stride ld_x, 16-byte aligned rows, ALLOCATED for whole tiles of
 * 32 rows: ceil(B / 32) * 32 rows, the rows past B receive zeros) is still written -- the
 * backward's weight-gradient GEMM reads it -- with bits equal to dctr_bilinear_fwd's.  sched_k: the pairs in output
 * order as dctr_bilinear_fwd takes them; relu != 0: act = relu, else identity; b0 nullable.  The eight per-wave partial
 * sums of a sample's row meet in wave order, the two inputs' shares in input order: bit-reproducible.
 * workspace = dctr_bilinear_wide_fwd_workspace_floats(B, P) floats.  DCTR_ENOSUP unless D == 16, H <= 128, n_dense <= 32.  (fibinet.py:82-99, interaction.py:140-156, core.py:123-133)           */
size_t dctr_bilinear_wide_fwd_workspace_floats(int32_t B, int32_t P);
int dctr_bilinear_wide_fwd(const float* E, int64_t ld_e, const float* V, int64_t ld_v, const float* Wf,
                           const int32_t* sched_k, int32_t P, int32_t F, int32_t D, int32_t B, const float* dense,
                           int64_t ld_d, int32_t n_dense, const float* W0, int64_t ld_w0, int32_t H, const float* b0,
                           int32_t relu, float* x, int64_t ld_x, float* h, int64_t ld_h, float* workspace,
                           float* wpk_bwd, dctr_stream_t stream);
/* wpk_bwd (nullable, dctr_bilinear_wide_pack_floats(P) floats, 16-byte aligned): W0 in the BACKWARD's operand layout,
 * written by the forward's packing launch; handed to dctr_bilinear_wide_bwd as `wpk` (NULL there: it packs W0 itself)
 * it saves that launch.  Valid as long as W0 is unchanged.                                                           */
size_t dctr_bilinear_wide_pack_floats(int32_t P);
int dctr_bilinear_wide_bwd(const float* E, int64_t ld_e, const float* V, int64_t ld_v, const float* Wf,
                           const int32_t* sched4, int32_t n_groups, const int32_t* pair_w, int32_t n_w, int32_t P,
                           int32_t F, int32_t D, int32_t B, const float* gh, int64_t ld_gh, const float* W0,
                           int64_t ld_w0, int32_t H, float* gE, float* gV, float* gW, float* workspace,
                           const float* wpk, dctr_stream_t stream);

/* InnerProductLayer (interaction.py:557-577): out[b, k] = sum_d e_i e_j (reduce != 0) or out[b, k*D + d] = e_i e_j;
 * pair order i < j, i outer.  Backward: gE[b, f, :] = sum_{g != f} gp[b, pair(f, g)] e_g.                    */
int dctr_inner_product_fwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t reduce, float* out,
                           int64_t ld_o, dctr_stream_t stream);
int dctr_inner_product_bwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t reduce,
                           const float* gp, int64_t ld_g, float* gE, int64_t ld_ge, dctr_stream_t stream);

/* ---- CrossNet, vector parameterisation (interaction.py:438-447; csrc/cross.hip) --------------------------
 *     x_{l+1} = x_0 * (x_l . w_l) + b_l + x_l ,  l = 0..L-1
 *   X [B, W] rows at X + b*ld_x;  kernels [L, W] (crossnet.kernels [L, W, 1]);  bias [L, W];  Y [B, W].  W <= 2048.
 * Backward writes gX [B, W], g_kernels [L, W], g_bias [L, W];
 * workspace = dctr_crossnet_vec_bwd_workspace_floats(B, W, L) floats (per-workgroup partials, fixed-order sum).
 * (The matrix parameterisation: dctr_crossnet_mat_fwd / _bwd below.)                                             */
int dctr_crossnet_vec_fwd(const float* X, int64_t ld_x, int32_t B, int32_t W, int32_t L, const float* kernels,
                          const float* bias, float* Y, int64_t ld_y, dctr_stream_t stream);
size_t dctr_crossnet_vec_bwd_workspace_floats(int32_t B, int32_t W, int32_t L);
int dctr_crossnet_vec_bwd(const float* X, int64_t ld_x, int32_t B, int32_t W, int32_t L, const float* kernels,
                          const float* bias, const float* gY, int64_t ld_g, float* gX, int64_t ld_gx,
                          float* g_kernels, float* g_bias, float* workspace, dctr_stream_t stream);

/* ---- CrossNet, matrix parameterisation (interaction.py:448-451; csrc/cross_tower.hip, on the tower's MFMA machinery)
 *     x_{l+1} = x_0 (.) (x_l W_l^T + b_l) + x_l ,  l = 0..L-1          W_l = crossnet.kernels[l]  [W, W]
 * described as a dctr_mlp_t (declared below) whose layers are all W x W: layer[l].W (rows ld_w floats apart, ld_w % 4
 * == 0), .bias [W], .h [B, ld_h] receives x_{l+1} (the last one IS the result), .dh [B, ld_h] is scratch shared by
 * the two calls (the forward parks u_l = x_l W_l^T + b_l there, the backward turns it into d loss / d u_l);  w_out must
 * be NULL.  A workgroup carries 16 samples through all layers (x_0 and x_l stay in LDS); fp32 MFMA 16x16x4.
 * The backward takes gY = d loss / d x_L [B, ld_g] and writes gx [B, ld_gx] = d loss / d x_0, layer[l].gW [W, ld_w]
 * and layer[l].gbias [W] (split-batch partials summed in a fixed order: no atomics).  All W * ld_w floats of a gW are
 * written: its padding columns [W, ld_w) receive 0, as the tower's do, and so do gx's [W, ld_gx); the padding of h is
 * never written.  x and every leading dimension (ld_x, ld_w, ld_h, ld_gx) follow the tower's alignment rule in both
 * calls: DCTR_EALIGN otherwise.
 * workspace = dctr_crossnet_mat_bwd_workspace_floats(m, B) floats.  dctr_crossnet_mat_supported: W <= 512 (LDS).   */
struct dctr_mlp;
int dctr_crossnet_mat_supported(int32_t W, int32_t n_layers);
int dctr_crossnet_mat_fwd(const struct dctr_mlp* m, const float* x, int64_t ld_x, int32_t B, dctr_stream_t stream);
size_t dctr_crossnet_mat_bwd_workspace_floats(const struct dctr_mlp* m, int32_t B);
int dctr_crossnet_mat_bwd(const struct dctr_mlp* m, const float* x, int64_t ld_x, int32_t B, const float* gY,
                          int64_t ld_g, float* gx, int64_t ld_gx, float* workspace, dctr_stream_t stream);

/* ---- CrossNetMix of DCN-Mix (interaction.py:499-534; csrc/cross_tower.hip) ---------------------------------------
 * Per cross layer, with E experts of rank R over W inputs (G = the gating weights [E, W], shared by all layers):
 *     s = softmax(x_l G^T)                      v1_e = tanh(x_l V_e)                  v2_e = tanh(v1_e C_e^T)
 *     x_{l+1} = x_0 (.) (sum_e s_e v2_e U_e^T + b) + x_l
 * described as a dctr_mlp_t of THREE dense layers per cross layer (the caller packs the weights):
 *   layer 3l   : W1 [E*R + E, W]   rows e*R + r = V_e[:, r], rows E*R + e = G[e];   h = [v1 | s],  dh scratch
 *   layer 3l+1 : W2 [E*R, E*R]     block-diagonal, block e = C_e;   h = s (.) v2 (what feeds the next product),
 *                                  dh: the forward parks the unscaled v2 there (the backward needs it)
 *   layer 3l+2 : W3 [W, E*R]       W3[w, e*R + r] = U_e[w, r];  bias = b;   h = x_{l+1} (the last one IS the result),
 *                                  dh: the forward parks u = sum_e s_e v2_e U_e^T + b
 * ld_w % 4 == 0 with zero padding, w_out NULL, n_layers = 3 * cross layers <= DCTR_MLP_MAX_LAYERS.
 * A workgroup carries 16 samples through all layers (x_0, x_l and the rank-space tiles in LDS; fp32 MFMA 16x16x4).
 * The backward takes gY = d loss / d x_L and writes gx = d loss / d x_0 and, per dense layer, gW / gbias in the packed
 * form (the caller unpacks: gV, gG (summed over the cross layers), the diagonal blocks gC, gU, gb).
 * dctr_crossnet_mix_supported: W <= 512, E*R + E <= 512, E <= 8 (LDS).                                              */
int dctr_crossnet_mix_supported(int32_t W, int32_t n_cross_layers, int32_t E, int32_t R);
int dctr_crossnet_mix_fwd(const struct dctr_mlp* m, int32_t E, int32_t R, const float* x, int64_t ld_x, int32_t B,
                          dctr_stream_t stream);
size_t dctr_crossnet_mix_bwd_workspace_floats(const struct dctr_mlp* m, int32_t B);
int dctr_crossnet_mix_bwd(const struct dctr_mlp* m, int32_t E, int32_t R, const float* x, int64_t ld_x, int32_t B,
                          const float* gY, int64_t ld_g, float* gx, int64_t ld_gx, float* workspace,
                          dctr_stream_t stream);

/* ---- DNN tower + dnn_linear on fp32 MFMA (csrc/mlp.hip) ---------------------------------------------------
 * DNN.forward (layers/core.py:120-134) with relu (or linear) activations, no BatchNorm, dropout inactive:
 *     h_0 = x ;  h_{l+1} = act(h_l W_l^T + bias_l)            W_l = dnn.linears.<l>.weight [N_l, K_l]
 * optionally followed by the bias-free projection of deepfm.py:61,84 (xdeepfm / fibinet / pnn alike):
 *     logit[b] = h_L[b, :] . w_out                              w_out = dnn_linear.weight [1, N_L]
 * The struct lives in HOST memory.  W rows are addressed W + n*ld_w with ld_w % 4 == 0 and a 16-byte aligned
 * base; floats in the row padding [K, ld_w) must be finite (they are multiplied by zero).  gW is written with
 * the same leading dimension (padding columns receive 0).  Floats in x's row padding [K, ld_x) never enter a
 * product (every kernel selects them away before it multiplies): they may hold anything, NaN included.
 *   h   [B, ld_h] post-activation output of the layer: written by dctr_mlp_fwd when non-NULL (needed by the
 *                 backward for every layer; without w_out the last layer's h IS the result)
 *   dh  [B, ld_h] backward scratch: d loss / d pre-activation, written by dctr_mlp_bwd
 * Columns [N, ld_h) of h and dh are padding: those below round_up(N, 4) are set to 0 or left as they were, those
 * from round_up(N, 4) on are never written.  Columns [K, ld_gx) of gx are padding: those below round_up(K, 32) are
 * set to 0, those below round_up(K, 64) are set to 0 or left as they were, those from there on are never written.
 * dctr_mlp_bwd takes g = d loss / d logit [B] (with w_out) or d loss / d h_L [B, ld_g] (without) and writes
 *   gx [B, ld_gx] = d loss / d x (nullable), layer[l].gW, layer[l].gbias, g_w_out.
 * Replaces autograd's mm / addmm / threshold_backward / sum chains under basemodel.py:261.  Everything is
 * summed in a fixed order (no atomics): results are bit-reproducible.
 *   workspace  dctr_mlp_bwd_workspace_floats(m, B) floats (split-batch partials of the weight gradients)   */
#define DCTR_MLP_MAX_LAYERS 12
typedef struct dctr_mlp_layer {
  const float* W;
  const float* bias; /* [N] nullable                   */
  float* h;
  float* dh;
  float* gW;         /* [N, ld_w] nullable: not written */
  float* gbias;      /* [N] nullable                    */
  int32_t K, N;
  int32_t ld_w, ld_h;
  int32_t relu;      /* 1: relu, 0: identity            */
  int32_t pad_;
} dctr_mlp_layer_t;
typedef struct dctr_mlp {
  dctr_mlp_layer_t layer[DCTR_MLP_MAX_LAYERS];
  const float* w_out; /* [N_last] nullable */
  float* g_w_out;     /* [N_last] nullable */
  int32_t n_layers;
  int32_t pad_;
} dctr_mlp_t;
size_t dctr_sizeof_mlp(void);
#ifdef DCTR_DIAG
/* diagnostics, DCTR_DIAG build only (tools/mlp_trace.py): buf = 3 x 4096 x 16 u64 of per-workgroup wall_clock64
 * stamps (forward | backward-data | wgrad); NULL switches tracing off.  Batches above 65536 samples are not traced
 * correctly.  */
void dctr_dbg_mlp_trace(unsigned long long* buf);
#endif
int dctr_mlp_fwd(const dctr_mlp_t* m, const float* x, int64_t ld_x, int32_t B, float* logit, dctr_stream_t stream);
size_t dctr_mlp_bwd_workspace_floats(const dctr_mlp_t* m, int32_t B);
int dctr_mlp_bwd(const dctr_mlp_t* m, const float* x, int64_t ld_x, int32_t B, const float* g, int64_t ld_g,
                 float* gx, int64_t ld_gx, float* workspace, dctr_stream_t stream);

/* The fused train step of a binary model whose logit is part0 + part1 + tower(x) + bias: tower forward, prediction
 * head, BCE(sum), backward-data (ONE launch per 16-sample row tile: the logits never leave the workgroup), then the
 * weight gradients and their reduction -- 3 launches for what dctr_mlp_fwd + dctr_bce_head + dctr_mlp_bwd do in 5.
 * Outputs: y_pred [B], loss [1], g_logit [B] (= d loss / d part0 = d loss / d part1), g_bias [1] (nullable), gx,
 * layer[l].gW / gbias, g_w_out.  Needs w_out and every layer's h / dh.
 * workspace: dctr_mlp_train_workspace_floats(m, B) floats.
 * defer_wgrad != 0: only the first launch is enqueued (y_pred, g_logit, gx, the h / dh activations are then
 * complete); the caller enqueues the weight-gradient half itself with dctr_mlp_train_wgrad (same m, x, workspace)
 * -- on another stream if it wants it to overlap with work that needs only gx / g_logit (the embedding update).
 * loss, g_bias, layer[l].gW / gbias and g_w_out are written by that second call.                               */
size_t dctr_mlp_train_workspace_floats(const dctr_mlp_t* m, int32_t B);
int dctr_mlp_train_step(const dctr_mlp_t* m, const float* x, int64_t ld_x, int32_t B, const float* part0,
                        const float* part1, const float* bias, const float* y, float* y_pred, float* loss,
                        float* g_logit, float* g_bias, float* gx, int64_t ld_gx, float* workspace,
                        int32_t defer_wgrad, const dctr_dense_step_t* step, dctr_stream_t stream);
/* step (nullable, both calls): the reduction that finishes layer[l].gW / gbias, g_w_out and g_bias also applies this
 * optimizer step to the parameters behind them -- no dctr_dense_opt launch, no join in front of it.               */
int dctr_mlp_train_wgrad(const dctr_mlp_t* m, const float* x, int64_t ld_x, int32_t B, const float* g_logit,
                         float* workspace, float* loss, float* g_bias, const dctr_dense_step_t* step,
                         dctr_stream_t stream);

/* ---- the embedding lookup as the fused train launch's input stage (round 4) ------------------------------------------
 * dctr_embed_fwd + dctr_mlp_train_step(defer_wgrad = 1) as ONE launch for a DeepFM / WDL-shaped model -- logit =
 * linear(X) [+ FM(embeddings)] + tower(combined_dnn_input) + bias (deepfm.py:67-86, wdl.py): every workgroup gathers the
 * table rows of its own 16 samples (basemodel.py:354-380), computes the linear logit (basemodel.py:63-92) and the FM
 * term (interaction.py:26-34) in LDS, and goes on with the tower, the head, BCE(sum) and the backward-data pass.  The
 * gather kernel, its output's round trip through memory and one kernel boundary leave the step's critical cycle.
 *   plan   fixed-length fields only, one embedding_dim in {4, 8, 16, 32, 64}, at most 32 wide fields; the tower's input is
 *          the plan's whole row (layer[0].K == n_deep * emb_dim + n_dense)
 *   out    [B, ld_out]  written: the gathered row of every sample (what dctr_embed_fwd's `out` holds): the operand of
 *          dctr_mlp_train_wgrad(m, out, ld_out, ...), which the caller enqueues as after dctr_mlp_train_step(defer_wgrad)
 *   fm_s   [B, ld_s]    written when non-NULL: sum_f e (FM's backward inside dctr_embed_update); required with want_fm
 *   y_pred, g_logit, gx, workspace, err: as in dctr_mlp_train_step / dctr_embed_fwd.
 * Same arithmetic, in the same order, as the two calls it replaces: results are bit-identical to theirs.
 * dctr_embed_tower_train_supported: 1 when plan + tower fit (else the caller keeps the two-launch path).            */
int dctr_embed_tower_train_supported(const dctr_plan_t* plan, const dctr_mlp_t* m, int32_t B);
int dctr_embed_tower_train_step(const dctr_plan_t* plan, const float* X, int64_t ldx, const dctr_mlp_t* m, int32_t B,
                                int32_t want_fm, const float* bias, const float* y, float* y_pred, float* g_logit,
                                float* gx, int64_t ld_gx, float* out, int64_t ld_out, float* fm_s, int64_t ld_s,
                                int32_t* err, float* workspace, dctr_stream_t stream);

/* *dst (device) = the 100 MHz device wall clock at the moment a one-thread launch runs on `stream`: put between two kernels
 * of a queue it dates their boundary -- the only way to time a kernel INSIDE a hipGraph replay (bench.py: the graph-replayed
 * duration of the step's dominant kernels).                                                                           */
int dctr_stamp(uint64_t* dst, dctr_stream_t stream);

/* ---- direct exchange between the ranks of a table-sharded job (one process per GPU; deepctr_torch/parallel.py) ----------
 * Replaces the host-issued RCCL all-to-alls / all-reduce of the sharded step (basemodel.py:206-209 is nn.DataParallel in
 * the reference) by copies into the peers' IPC-mapped receive buffers + a word per (exchange, sender): everything is an
 * ordinary stream operation, so the WHOLE step -- exchanges included -- is one hipGraph.  `step`: this rank's exchange
 * counter (device int32); peer_words[r]: rank r's word array for this exchange (device pointers, IPC-mapped), my_index:
 * this rank's slot in it.  Post behind the copies (same stream); wait in front of the consumer; next advances the counter.
 * A wait gives up after timeout_us and raises bit 1 of *err.  dctr_sum_ranks: dst[i] = sum_r src[r * ld + i] in rank
 * order (the dense gradients' all-reduce = all-gather by copy + this sum: every rank lands on the same bits).          */
/* hipMemcpyAsync(device to device) on the caller's stream (dst may be another device's memory mapped through IPC);
 * dctr_enable_peer_access(d): the current device may reach device d's memory (no-op for d == current device,
 * DCTR_ENOSUP when the devices have no peer path).                                                                  */
int dctr_copy_async(void* dst, const void* src, size_t bytes, dctr_stream_t stream);
int dctr_enable_peer_access(int32_t peer_device);
int dctr_exchange_post(int32_t* const* peer_words, int32_t n, int32_t my_index, const int32_t* step, dctr_stream_t stream);
int dctr_exchange_wait(const int32_t* words, int32_t n, const int32_t* step, int32_t timeout_us, int32_t* err,
                       dctr_stream_t stream);
int dctr_exchange_next(int32_t* step, dctr_stream_t stream);
int dctr_sum_ranks(float* dst, const float* src, const uint64_t* src_tbl, int32_t n_ranks, int64_t n, int64_t ld,
                   const dctr_dense_step_t* step, int32_t store, dctr_stream_t stream);
/* step (nullable): the optimizer step on the elements it finishes.  src_tbl [n_ranks] (device, nullable): rank r's slab
 * is read where it lies, at (const float*)src_tbl[r] (16-byte aligned, peer memory) -- a pull, no copies; store == 0
 * (needs step): the sum itself is not written, dst only names the gradients' slab positions and may alias a source.  */
/* post + wait (+ advance != 0: the counter's advance, behind a step's last exchange) as one launch */
int dctr_exchange_sync(int32_t* const* peer_words, const int32_t* words, int32_t n, int32_t my_index, int32_t* step,
                       int32_t advance, int32_t timeout_us, int32_t* err, dctr_stream_t stream);
/* One launch in front of a sharded step: this rank's batch (xb [B, ncols], yb [B]) into the static buffers the captured
 * step reads, and -- x_next non-NULL -- the next batch's id columns id_cols [n_ranks * n_slots] into columns
 * [ids_col, ids_col + n_slots) of the gradient chunks send [n_ranks][B][ld_chunk] (they ride in the gradient exchange). */
int dctr_shard_stage(const float* xb, int64_t ld_xb, const float* yb, int32_t B, int32_t ncols, float* x_dst,
                     int64_t ld_xd, float* y_dst, const float* x_next, int64_t ld_xn, const int32_t* id_cols,
                     int32_t n_ranks, int32_t n_slots, float* send, int64_t ld_chunk, int32_t ids_col,
                     dctr_stream_t stream);

/* ---- prediction head + loss (layers/core.py:154-160, basemodel.py:254, F.binary_cross_entropy(reduction='sum'))
 *     z = sum_i part_i[b] + bias ;  y_pred = sigmoid(z) ;  loss = sum_b -(y log p + (1-y) log(1-p))   (logs clamped
 *     at -100 like ATen) ;  g_logit = d loss / d z as autograd computes it:
 *     (p - y) / max((1-p) p, 1e-12) * (1-p) p ;  g_bias = sum_b g_logit.
 * Up to four logit parts (linear, FM, DNN, CIN ...), each [B], nullable.  One workgroup, tree reductions:
 * deterministic.  Replaces ~12 elementwise / reduce launches per step.                                      */
int dctr_bce_head(const float* part0, const float* part1, const float* part2, const float* part3, const float* bias,
                  const float* y, int32_t B, float* y_pred, float* loss, float* g_logit, float* g_bias,
                  dctr_stream_t stream);

/* ---- autograd glue as single launches (models on torch.autograd: xDeepFM, FiBiNET, DCN, PNN, ...) ------------------------
 * dctr_rows_join: out[b, 0:W) = a[b, :] (+ c[b, :]), out[b, W:W+n_d) = d[b, :], out[b, W+n_d:ld_out) = 0 -- the gradient of
 * the gather's output [B, ld_out] from the gradients of its two views (replaces the slice backward's copies + fill, and
 * autograd's add when c is given; a, c, d nullable).  W, ld_* multiples of 4, 16-byte aligned rows.  out may BE a (same
 * leading dimension): every lane reads the words it writes -- "a[:, :W] += c, a[:, W:] = 0" in one launch.
 * dctr_relu_bwd_bias: g_out = g * (h > 0) (aten::threshold_backward; h NULL: g_out = g; g_out NULL: not written) and
 * g_bias[n] = sum_b g_out[b, n] in a fixed order (replaces threshold_backward + sum(0) behind a wide nn.Linear,
 * layers/core.py:120-134).  workspace: dctr_relu_bwd_bias_workspace_floats(B, N) floats.                             */
int dctr_rows_join(const float* a, int64_t ld_a, const float* c, int64_t ld_c, int32_t W, const float* d, int64_t ld_d,
                   int32_t n_d, float* out, int64_t ld_out, int32_t B, dctr_stream_t stream);
size_t dctr_relu_bwd_bias_workspace_floats(int32_t B, int32_t N);
int dctr_relu_bwd_bias(const float* g, int64_t ld_g, const float* h, int64_t ld_h, int32_t B, int32_t N, float* g_out,
                       int64_t ld_o, float* g_bias, float* workspace, dctr_stream_t stream);

/* ---- dense optimizer over one flat parameter slab (torch.optim.SGD / Adagrad, basemodel.py:447-461) --------
 *   DCTR_UPD_SGD      p -= lr * g
 *   DCTR_UPD_ADAGRAD  state += g*g ; p -= lr * g / (sqrt(state) + eps)
 * One launch for every dense parameter of the model (the reference's optimizer issues ~8 foreach launches).  */
int dctr_dense_opt(float* p, const float* g, float* state, int64_t n, int32_t opt, float lr, float eps,
                   dctr_stream_t stream);
/* The same step on a list of contiguous fp32 tensors -- the parameters of a model whose train step runs through
 * autograd (xDeepFM's CIN weights, DCN's cross kernels, ...), each with the gradient autograd left in `.grad` and its
 * Adagrad `sum` -- in one launch per 48 tensors (torch.optim.Adagrad / SGD step, basemodel.py:262: 5 foreach launches).
 * items: HOST array.  state: ignored for DCTR_UPD_SGD.                                                              */
typedef struct dctr_dense_item {
  float* p;
  const float* g;
  float* state;
  int64_t n;
  float l2;   /* lambda of an L2 term lambda * sum(p^2) on this tensor (basemodel.py:412-428), 0: none.  The step then
               * uses g + 2*lambda*p -- what autograd adds to .grad for the term (rounded like autograd: product, sum) */
  float pad_;
} dctr_dense_item_t;
size_t dctr_sizeof_dense_item(void);
int dctr_dense_opt_multi(const dctr_dense_item_t* items, int32_t n_items, int32_t opt, float lr, float eps,
                         dctr_stream_t stream);
/* out[0] = sum_i l2_i * sum(p_i^2): the value of those terms for the logged loss; one workgroup, fixed summation order.
 * (g / state of the items are not read.)                                                                            */
int dctr_l2_value_multi(const dctr_dense_item_t* items, int32_t n_items, float* out, dctr_stream_t stream);
/* ABI 35 -- the multi-tensor step for every kind of dctr_lazy_opt_t (SGD, Adagrad, Adam, RMSprop) with a DEVICE-side step
 * count: optimizer step number *step + 1 (read, NOT advanced) on a list of contiguous fp32 tensors, one launch per 48
 * tensors; every launch of a longer list reads the same *step, and the caller advances the counter ONCE afterwards with
 * dctr_lazy_step_inc.  torch.optim.Adam computes its bias corrections on the host, so its step cannot be replayed from a
 * hipGraph; this one can.  g + 2*l2*p enters the step where l2 != 0 (rounded like autograd: product, then sum).  The
 * arithmetic per element is that of dctr_dense_opt_reg / the lazy table update (csrc/lazy_opt.hpp), IEEE division and
 * square root.  opt->adam_ss / adam_bc (optional, as for the tables): Adam's scalars by step number.
 *   s1: Adagrad sum | Adam exp_avg | RMSprop square_avg      s2: Adam exp_avg_sq      (ignored where the kind has none)
 * items: HOST array.  DCTR_EINVAL -- before anything is launched -- on a NULL opt or step, an unknown kind, n < 0, or a
 * tensor with n > 0 that lacks p, g or a state its kind needs; n_items == 0 or all n == 0: DCTR_OK, nothing launched. */
typedef struct dctr_dense_item2 {
  float* p;
  const float* g;
  float* s1;
  float* s2;
  int64_t n;
  float l2;
  float pad_;
} dctr_dense_item2_t;
size_t dctr_sizeof_dense_item2(void);
int dctr_dense_opt_multi_reg(const dctr_dense_item2_t* items, int32_t n_items, const dctr_lazy_opt_t* opt,
                             const int32_t* step, dctr_stream_t stream);

/* ---- table-sharded multi-GPU exchange: the two "assemble" kernels (csrc/shard.hip, deepctr_torch/parallel.py) ---
 * Rank q of N owns units q, q+N, q+2N, ... (a unit = one id column with its deep and/or wide table).  Owners gather
 * with dctr_embed_fwd over the N*B global samples and update with dctr_embed_update; what travels between ranks
 * are chunks [B, ld_chunk] whose row b is [ slot 0 | slot 1 | ... (slot j = unit q + j*N, D floats each) | pad |
 * wide partial sum at column wide_col | pad ].
 * dctr_shard_assemble_fwd: recv [N][B][ld_chunk] (chunk q from owner q) -> the single-GPU outputs of
 *   dctr_embed_fwd: out [B, ld_out] = [ e_0 | ... | e_{F-1} | dense block at dense_off ], wide [B] (sum of the owners'
 *   partials in rank order + X[:, wdense_cols] . wdense_w), fm [B], fm_s [B, ld_s]  (wide / fm / fm_s nullable).
 * dctr_shard_assemble_bwd: the adjoint; send [N][B][ld_chunk] with G[b, f] = g_out[b, f] + g_fm[b] * (S[b] - e[b, f])
 *   in unit f's slot and g_wide[b] at wide_col; g_wdense [n_wdense] (nullable) = X[:, wdense_cols]^T g_wide.
 * owner_slot [F] (device, nullable): unit f is owned by rank (owner_slot[f] & 0xffff) and sits in slot
 *   (owner_slot[f] >> 16) of that owner's chunk; NULL: owner f % N, slot f / N.
 * send_chunks [N] (device, nullable): chunk q is written at (float*)send_chunks[q] ([B][ld_chunk]) instead of
 *   send + q * B * ld_chunk -- owner q's receive buffer, peer memory: the push-style exchange, no copy node; columns
 *   [carry_col, carry_col + carry_n) of the LOCAL send rows (dctr_shard_stage's next-batch ids) are copied along.
 * Deterministic (no atomics).  D <= 64.                                                                          */
int dctr_shard_assemble_fwd(const float* recv, int64_t ld_chunk, int32_t n_ranks, int32_t B, int32_t F, int32_t D,
                            const int32_t* owner_slot, int32_t wide_col, const float* X, int64_t ld_x, const int32_t* dense_cols,
                            int32_t n_dense, int32_t dense_off, const int32_t* wdense_cols, const float* wdense_w,
                            int32_t n_wdense, float* out, int64_t ld_out, float* wide, float* fm, float* fm_s,
                            int64_t ld_s, dctr_stream_t stream);
int dctr_shard_assemble_bwd(float* send, const uint64_t* send_chunks, int32_t carry_col, int32_t carry_n, int64_t ld_chunk, int32_t n_ranks, int32_t B, int32_t F, int32_t D,
                            const int32_t* owner_slot, int32_t wide_col, const float* g_out, int64_t ld_g, const float* g_wide, const float* g_fm,
                            const float* out, int64_t ld_out, const float* fm_s, int64_t ld_s, const float* X,
                            int64_t ld_x, const int32_t* wdense_cols, int32_t n_wdense, float* g_wdense,
                            dctr_stream_t stream);
/* The same with the carried columns taken straight from the NEXT batch's input matrix (round 6: the staging launch in front
 * of every step of a captured group is gone): carried value (q, j) of sample b = x_next[b, carry_cols[q * carry_n + j]]
 * (carry_cols [n_ranks * carry_n], device); x_next == NULL: dctr_shard_assemble_bwd.                                    */
int dctr_shard_assemble_bwd_next(float* send, const uint64_t* send_chunks, int32_t carry_col, int32_t carry_n, int64_t ld_chunk,
                                 int32_t n_ranks, int32_t B, int32_t F, int32_t D, const int32_t* owner_slot, int32_t wide_col,
                                 const float* g_out, int64_t ld_g, const float* g_wide, const float* g_fm, const float* out,
                                 int64_t ld_out, const float* fm_s, int64_t ld_s, const float* X, int64_t ld_x,
                                 const int32_t* wdense_cols, int32_t n_wdense, float* g_wdense, const float* x_next,
                                 int64_t ld_xn, const int32_t* carry_cols, dctr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DCTR_H */
