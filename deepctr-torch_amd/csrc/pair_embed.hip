// pair_embed.hip -- ONN / NFFM's second-order lookup for gfx950 (MI355X): every ordered pair (i < j) of sparse features
// owns two tables, emb1 indexed by feature i's id and emb2 by feature j's; the DNN input is the concatenation of the
// P = F (F - 1) / 2 elementwise products followed by the dense values (reference models/onn.py:14-34, :98-120, :139-148:
// 2 P aten::embedding calls, P multiplies and a cat; backward 2 P dense [V, D] gradients).
//
// One launch per direction.  What bounds it is the memory system's random-line request rate (rows are 16-64 bytes), not
// bytes, so the kernel is shaped around keeping row requests in flight:
//   * the workgroup geometry is the gather's (csrc/embed_tile.hpp): 4 waves share SPB = 64 / LPR samples, whose X rows
//     (the F ids, each used F - 1 times) and the 2 P + n_wide descriptors are staged in LDS once;
//   * the first-order logit is the gather's own device code, on the gather's lane mapping: `wide` equals
//     dctr_embed_fwd's bit for bit;
//   * then the 256 / LPR lane groups of the workgroup walk the SPB * P (sample, pair) items: a lane group of LPR = D / VEC
//     lanes owns one item, both rows move as dwordx4 / dwordx2, neighbouring lane groups take neighbouring pairs of the
//     same sample -- their stores form contiguous runs of `out` (`g_rows`) -- and every lane group issues the 2 * CH row
//     loads of CH items before the first multiply;
//   * the backward re-reads the rows (L2 / MALL hits when the step is short) instead of saving a [B, 2 P D] copy.
// No atomics, no scratch: every output element is one fp32 multiply, written once.
#include "embed_tile.hpp"

using namespace dctr;

namespace {

constexpr int kPairCH = 8;  // (sample, pair) items in flight per lane group: 16 row loads per lane
constexpr int kPairRed = 1; // cross-wave scratch per thread: the wide partial

// item -> (sample s of the tile, pair p), both rows' addresses; out-of-range ids read row 0 and raise `bad`
struct PairItem {
  int s, p;
  const float* r1;
  const float* r2;
};

__device__ __forceinline__ PairItem pair_item(const Tile& T, int n_xcols, int n_pairs, int item, int eoff, int& bad) {
  PairItem it;
  it.s = item / n_pairs;
  it.p = item - it.s * n_pairs;
  const float* xr = T.xs + it.s * n_xcols;
  const dctr_field_t& f1 = T.deep[2 * it.p];
  const dctr_field_t& f2 = T.deep[2 * it.p + 1];
  it.r1 = f1.table + checked(raw_id(xr, f1.col), f1.vocab, bad) * row_ld(f1) + eoff;
  it.r2 = f2.table + checked(raw_id(xr, f2.col), f2.vocab, bad) * row_ld(f2) + eoff;
  return it;
}

template <int VEC, int LPR>
__global__ __launch_bounds__(kThreads) void k_pair_fwd(dctr_plan_t P, const float* __restrict__ X, int64_t ldx, int B,
                                                       float* __restrict__ out, int64_t ldo, float* __restrict__ wide,
                                                       int64_t ldw, int32_t* err, uint8_t* __restrict__ amax,
                                                       int64_t ld_am, const int32_t* __restrict__ am_wide_off) {
  step_priority();
  constexpr int SPB = kWave / LPR;
  constexpr int NG = kThreads / LPR;   // lane groups per workgroup
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wv_id = tid >> 6, lane = tid & 63;
  const int b0 = blockIdx.x * SPB;
  const int nrows = min(SPB, B - b0);
  const Tile T = stage_tile(P, X, ldx, b0, nrows, SPB, smem);
  int bad = 0;

  // ---- first-order logit: the gather's lane mapping (lane group `grp` of every wave = sample b0 + grp) --------------
  if (wide) {
    const int grp = lane / LPR, gl = lane % LPR;
    const bool valid = grp < nrows;
    const int g = valid ? grp : 0;   // idle groups shadow group 0; their stores are masked
    const int b = b0 + g;
    const float* xr = T.xs + g * P.n_xcols;
    float* wrow = wide + static_cast<int64_t>(b) * ldw;
    float wval[kWideCH];
    wide_issue<LPR>(T, xr, wv_id, gl, P.n_wide_fixed, wval, bad);
    const float ws = wide_finish<LPR>(P, T, xr, wv_id, gl, P.n_wide_fixed, wval, valid, wrow,
                                      amax ? amax + static_cast<int64_t>(b) * ld_am : nullptr, am_wide_off, bad);
    T.red[wv_id * kWave + lane] = ws;
    __syncthreads();
    if (wv_id == 0) {
      const float wt = wide_total<LPR>(T.red, kPairRed, 0, lane);
      if (gl == 0 && valid) stg_f32(wrow, wt);
    }
  }

  // ---- the products: lane group gi takes items gi, gi + NG, ... of the tile's nrows * P ----------------------------
  const int D = P.emb_dim;
  const int n_pairs = P.n_deep >> 1;
  const int n_items = nrows * n_pairs;
  const int gi = tid / LPR, e0 = (tid % LPR) * VEC;
  const bool act = e0 < D;
  const int eoff = act ? e0 : 0;   // lanes past the row width re-read the row's first strip; their value is never used
  for (int base = 0; base < n_items; base += NG * kPairCH) {
    Strip<VEC> a[kPairCH], c[kPairCH];
    int so[kPairCH];
#pragma unroll
    for (int k = 0; k < kPairCH; ++k) {
      const int item = base + k * NG + gi;
      const PairItem it = pair_item(T, P.n_xcols, n_pairs, min(item, n_items - 1), eoff, bad);
      a[k] = strip_load<VEC>(it.r1);
      c[k] = strip_load<VEC>(it.r2);
      so[k] = (item < n_items && act) ? it.s * 65536 + it.p : -1;
    }
#pragma unroll
    for (int k = 0; k < kPairCH; ++k) {
      if (so[k] >= 0) {
        Strip<VEC> r;
#pragma unroll
        for (int i = 0; i < VEC; ++i) r.v[i] = a[k].v[i] * c[k].v[i];
        strip_store<VEC>(out + static_cast<int64_t>(b0 + (so[k] >> 16)) * ldo + (so[k] & 65535) * D + e0, r);
      }
    }
  }
  // dense block of combined_dnn_input (inputs.py:126-138), behind the products
  if (P.dense_off >= 0) {
    for (int k = tid; k < nrows * P.n_dense; k += kThreads) {
      const int s = k / P.n_dense, j = k - s * P.n_dense;
      stg_f32(out + static_cast<int64_t>(b0 + s) * ldo + P.dense_off + j, T.xs[s * P.n_xcols + ldg_i32(P.dense_cols + j)]);
    }
  }
  if (err && bad) atomicOr(err, 1);
}

template <int VEC, int LPR>
__global__ __launch_bounds__(kThreads) void k_pair_bwd(dctr_plan_t P, const float* __restrict__ X, int64_t ldx, int B,
                                                       const float* __restrict__ gout, int64_t ldg,
                                                       float* __restrict__ grows, int64_t ldr) {
  step_priority();
  constexpr int SPB = kWave / LPR;
  constexpr int NG = kThreads / LPR;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * SPB;
  const int nrows = min(SPB, B - b0);
  const Tile T = stage_tile(P, X, ldx, b0, nrows, SPB, smem);
  int bad = 0;   // ids were range-checked (and flagged) by the forward pass
  const int D = P.emb_dim;
  const int n_pairs = P.n_deep >> 1;
  const int n_items = nrows * n_pairs;
  const int gi = tid / LPR, e0 = (tid % LPR) * VEC;
  const bool act = e0 < D;
  const int eoff = act ? e0 : 0;
  for (int base = 0; base < n_items; base += NG * kPairCH) {
    Strip<VEC> a[kPairCH], c[kPairCH], g[kPairCH];
    int so[kPairCH];
#pragma unroll
    for (int k = 0; k < kPairCH; ++k) {
      const int item = base + k * NG + gi;
      const PairItem it = pair_item(T, P.n_xcols, n_pairs, min(item, n_items - 1), eoff, bad);
      a[k] = strip_load<VEC>(it.r1);
      c[k] = strip_load<VEC>(it.r2);
      g[k] = strip_load<VEC>(gout + static_cast<int64_t>(b0 + it.s) * ldg + it.p * D + eoff);
      so[k] = (item < n_items && act) ? it.s * 65536 + it.p : -1;
    }
#pragma unroll
    for (int k = 0; k < kPairCH; ++k) {
      if (so[k] >= 0) {
        const int p = so[k] & 65535;
        float* row = grows + static_cast<int64_t>(b0 + (so[k] >> 16)) * ldr + e0;
        Strip<VEC> g1, g2;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          g1.v[i] = g[k].v[i] * c[k].v[i];   // d / d emb1 row = g * emb2 row
          g2.v[i] = g[k].v[i] * a[k].v[i];
        }
        strip_store<VEC>(row + T.deep[2 * p].out_off, g1);
        strip_store<VEC>(row + T.deep[2 * p + 1].out_off, g2);
      }
    }
  }
}

// what both entry points refuse (DCTR_ENOSUP) or reject; *lpr / *lds on success
int check_pair_plan(const dctr_plan_t* p, const float* X, int64_t ldx, int32_t B, int* lpr, size_t* lds) {
  if (int rc = check_plan(p, X, ldx, B)) return rc;
  if (p->out_chunks || (p->flags & DCTR_PLAN_WIDE_PER_FIELD)) return DCTR_ENOSUP;
  if (p->n_deep & 1) return DCTR_ENOSUP;
  if (p->n_deep_fixed != p->n_deep) return DCTR_ENOSUP;            // pooled / VarLen deep fields
  if (p->n_deep > 0 && (p->emb_dim <= 0 || p->max_dim != p->emb_dim)) return DCTR_ENOSUP;   // mixed dims
  if ((p->n_deep >> 1) > 65535) return DCTR_ENOSUP;
  *lpr = lanes_per_row(p, p->vec);
  *lds = tile_bytes_red(p, *lpr, kPairRed);
  if (*lds > kMaxTile) return DCTR_ENOSUP;
  return DCTR_OK;
}

bool misaligned(const void* ptr, int64_t ld, int vec) {
  return vec > 1 && (ld % vec != 0 || reinterpret_cast<uintptr_t>(ptr) % (4 * vec) != 0);
}

}  // namespace

extern "C" int dctr_pair_embed_fwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B, float* out,
                                   int64_t ld_out, float* wide, int64_t ld_wide, int32_t* err, dctr_stream_t stream) {
  int lpr = 1;
  size_t lds = 0;
  if (int rc = check_pair_plan(plan, X, ldx, B, &lpr, &lds)) return rc;
  if (B == 0) return DCTR_OK;
  const int n_pairs = plan->n_deep >> 1;
  const int64_t width = static_cast<int64_t>(n_pairs) * plan->emb_dim + (plan->dense_off >= 0 ? plan->n_dense : 0);
  if (!out && width > 0) return DCTR_EINVAL;
  if (out && ld_out < width) return DCTR_EINVAL;
  if (plan->dense_off >= 0 && plan->dense_off != static_cast<int64_t>(n_pairs) * plan->emb_dim) return DCTR_EINVAL;
  if (wide && ld_wide < 1) return DCTR_EINVAL;
  if (out && misaligned(out, ld_out, plan->vec)) return DCTR_EALIGN;
  const dctr_plan_ext_t* x = plan->ext;
  if (x && x->amax && (x->ld_amax <= 0 || !x->am_wide_off)) return DCTR_EINVAL;
  const int spb = kWave / lpr;
  const dim3 grid((B + spb - 1) / spb), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DCTR_DISPATCH(plan->vec, lpr, DCTR_LAUNCH((k_pair_fwd<VEC, LPR>), grid, block, lds, s, *plan, X, ldx, B, out, ld_out,
                                            wide, ld_wide, err, x ? x->amax : nullptr, x ? x->ld_amax : 0,
                                            x ? x->am_wide_off : nullptr));
  return launch_status();
}

extern "C" int dctr_pair_embed_bwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B, const float* g_out,
                                   int64_t ld_g, float* g_rows, int64_t ld_rows, dctr_stream_t stream) {
  int lpr = 1;
  size_t lds = 0;
  if (int rc = check_pair_plan(plan, X, ldx, B, &lpr, &lds)) return rc;
  const int n_pairs = plan->n_deep >> 1;
  if (n_pairs == 0 || B == 0) return DCTR_OK;
  if (!g_out || !g_rows) return DCTR_EINVAL;
  if (ld_g < static_cast<int64_t>(n_pairs) * plan->emb_dim || ld_rows < static_cast<int64_t>(plan->n_deep) * plan->emb_dim)
    return DCTR_EINVAL;
  if (misaligned(g_out, ld_g, plan->vec) || misaligned(g_rows, ld_rows, plan->vec)) return DCTR_EALIGN;
  const int spb = kWave / lpr;
  const dim3 grid((B + spb - 1) / spb), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DCTR_DISPATCH(plan->vec, lpr, DCTR_LAUNCH((k_pair_bwd<VEC, LPR>), grid, block, lds, s, *plan, X, ldx, B, g_out, ld_g,
                                            g_rows, ld_rows));
  return launch_status();
}
