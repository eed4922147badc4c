// mlr.hip -- MLR / LS-PLM (reference models/mlr.py:78-100) for gfx950 (MI355X): R region Linear modules are a softmax gate
// and, read again, the learners; an optional bias Linear scales the mixture.  The reference runs 2 R + 1 Linear calls (each
// its own lookups, cat and sum), then cat / softmax / sigmoid / mul / sum; here one launch forward and one (plus a small
// fixed-order reduce) backward, over a wide-only per-field plan whose fields carry the head they belong to.
//
// The model is nothing but 4-byte row reads, so what bounds the forward is the memory system's random-line request rate,
// as in csrc/pair_embed.hip, and the kernel is shaped the same way:
//   * the workgroup geometry is the gather's (csrc/embed_tile.hpp) at LPR = 4: 4 waves share 16 samples, thread t is sample
//     b0 + t % 16 and field slot t / 16, the 16 slots split the fields; the tile's X rows and the field descriptors are
//     staged in LDS once.  16 samples, not 64: at batch 4096 that is 256 workgroups instead of 64 (one per CU), and the
//     104 fields of the Criteo shape are 7 per thread -- every row request of a sample leaves in ONE batch;
//   * a lane issues the loads of kMlrCH fields before it parks the first weight; the weights of a tile go to LDS
//     ([field][sample]: conflict-free both ways), never to HBM;
//   * VarLen fields are pooled by the gather's own pool_field (sum / mean / max; a max pool's arg-max byte goes where the
//     gather puts it);
//   * then (sample, head) sums in field order + dense . weight through a pointer table (the R + 1 weights are separate
//     parameters), and one lane per sample does softmax, learners, bias factor and stores y.
// Every sum has a fixed order that depends neither on B nor on the sample's place in the batch.  No atomics on data (the
// out-of-range flag is the gather's idempotent OR).
#include "embed_tile.hpp"

using namespace dctr;

namespace {

constexpr int kMlrCH = 8;          // weight loads in flight per lane
constexpr int kMlrFwdSPB = 16;     // samples per workgroup of the forward (the gather's geometry at LPR = 4)
constexpr int kMlrSlots = kThreads / kMlrFwdSPB;   // field slots of the forward's workgroup
constexpr int kMlrBwdSPB = kWave;  // samples per workgroup of the backward (one tile = one partial of g_dense)

struct MlrDev {
  const int32_t* head_of;
  const int32_t* dense_cols;
  const int32_t* dense_off;
  const float* const* dense_w;
  int R, H, task, n_dense;
};

MlrDev mlr_dev(const dctr_mlr_t* m) {
  MlrDev d;
  d.head_of = m->head_of;
  d.dense_cols = m->dense_cols;
  d.dense_off = m->dense_off;
  d.dense_w = m->dense_w;
  d.R = m->n_regions;
  d.H = m->n_regions + (m->has_bias ? 1 : 0);
  d.task = m->task;
  d.n_dense = m->n_dense;
  return d;
}

// LDS of a workgroup: the tile (descriptors + spb rows of X), then the tile's weights [n_wide][spb] (forward only), its
// logits / logit gradients [spb][H], head_of [n_wide]
inline size_t mlr_lds(const dctr_plan_t* p, int H, int spb, bool fwd) {
  const size_t extra = (fwd ? static_cast<size_t>(spb) * p->n_wide : 0) + static_cast<size_t>(spb) * H + p->n_wide;
  return tile_bytes_red(p, kWave / spb, 0) + extra * sizeof(float);
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// softmax over z[0 .. R) (max-subtracted): the maximum and 1 / sum of the exponentials
__device__ __forceinline__ void softmax_stats(const float* z, int R, float& mx, float& rden) {
  mx = z[0];
  for (int r = 1; r < R; ++r) mx = fmaxf(mx, z[r]);
  float den = 0.f;
  for (int r = 0; r < R; ++r) den += expf(z[r] - mx);
  rden = 1.f / den;
}

__global__ __launch_bounds__(kThreads) void k_mlr_fwd(dctr_plan_t P, MlrDev M, const float* __restrict__ X, int64_t ldx,
                                                      int B, float* __restrict__ y, float* __restrict__ z, int64_t ld_z,
                                                      int32_t* err, const int32_t* __restrict__ units, int n_units,
                                                      int32_t* __restrict__ ids_t, uint16_t* __restrict__ parts_t,
                                                      int n_parts, uint8_t* __restrict__ amax, int64_t ld_am,
                                                      const int32_t* __restrict__ am_wide_off) {
#pragma clang fp contract(off)
  step_priority();
  extern __shared__ __align__(16) unsigned char smem[];
  constexpr int SPB = kMlrFwdSPB;
  const int tid = threadIdx.x, smp = tid % SPB, slot = tid / SPB;
  const int b0 = blockIdx.x * SPB;
  const int nrows = min(SPB, B - b0);
  const Tile T = stage_tile(P, X, ldx, b0, nrows, SPB, smem);
  const int nw = P.n_wide, nwf = P.n_wide_fixed, H = M.H;
  float* wvs = T.red;                                  // [nw][SPB]
  float* zs = wvs + SPB * nw;                          // [SPB][H]
  int32_t* hof = reinterpret_cast<int32_t*>(zs + SPB * H);
  for (int f = tid; f < nw; f += kThreads) hof[f] = ldg_i32(M.head_of + f);
  const bool valid = smp < nrows;
  const int g = valid ? smp : 0;   // idle threads shadow sample 0; nothing of theirs is stored
  const int b = b0 + g;
  const float* xr = T.xs + g * P.n_xcols;
  int bad = 0;

  // side output for dctr_embed_update, as dctr_embed_fwd writes it: the tile's ids transposed to [unit][b], and each entry's
  // partition tag
  if (ids_t) {
    for (int k = tid; k < n_units * nrows; k += kThreads) {
      const int u = k / nrows, r = k - u * nrows;
      const int32_t id = static_cast<int32_t>(T.xs[r * P.n_xcols + ldg_i32(units + 4 * u + 2)]);
      ids_t[static_cast<int64_t>(u) * B + b0 + r] = id;
      if (parts_t) {
        const int wi = ldg_i32(units + 4 * u + 1);   // (a wide-only plan: every unit is a wide table)
        const int64_t vocab = T.wide[min(max(wi, 0), nw - 1)].vocab;
        const uint32_t cid = (static_cast<uint64_t>(static_cast<int64_t>(id)) >= static_cast<uint64_t>(vocab))
                                 ? 0u : static_cast<uint32_t>(id);
        parts_t[static_cast<int64_t>(u) * B + b0 + r] = static_cast<uint16_t>(cid % static_cast<uint32_t>(n_parts));
      }
    }
  }

  // ---- fixed-length fields: slot q takes fields q, q + 16, ...; kMlrCH loads leave before the first weight is parked ----
  for (int f0 = slot; f0 < nwf; f0 += kMlrSlots * kMlrCH) {
    float val[kMlrCH];
#pragma unroll
    for (int k = 0; k < kMlrCH; ++k) {
      const dctr_field_t& fd = T.wide[min(f0 + k * kMlrSlots, nwf - 1)];   // slots past the last field re-read it
      val[k] = ldg_f32(fd.table + checked(raw_id(xr, fd.col), fd.vocab, bad) * row_ld(fd));
    }
#pragma unroll
    for (int k = 0; k < kMlrCH; ++k) {
      const int f = f0 + k * kMlrSlots;
      if (f < nwf) wvs[f * SPB + smp] = val[k];
    }
  }
  // ---- pooled VarLen fields: the gather's device code ----
  for (int f = nwf + slot; f < nw; f += kMlrSlots) {
    const dctr_field_t& fd = T.wide[f];
    uint8_t* am = nullptr;
    if (amax && valid && fd.pool == DCTR_POOL_MAX) {
      const int off = ldg_i32(am_wide_off + f);
      if (off >= 0) am = amax + static_cast<int64_t>(b) * ld_am + off;
    }
    wvs[f * SPB + smp] = pool_field<1>(fd, xr, 0, true, bad, am).v[0];
  }
  __syncthreads();

  // ---- (sample, head) logits: slot q takes heads q, q + 16, ...; fields in plan order, then the dense half ----
  for (int h = slot; h < H; h += kMlrSlots) {
    float acc = 0.f;
    for (int f = 0; f < nw; ++f)
      if (hof[f] == h) acc += wvs[f * SPB + smp];
    const int j0 = ldg_i32(M.dense_off + h), j1 = ldg_i32(M.dense_off + h + 1);
    if (j1 > j0) {
      const float* w = M.dense_w[h];
      for (int j = j0; j < j1; ++j) acc += xr[ldg_i32(M.dense_cols + j)] * ldg_f32(w + (j - j0));
    }
    zs[smp * H + h] = acc;
    if (valid) stg_f32(z + static_cast<int64_t>(b) * ld_z + h, acc);
  }
  __syncthreads();

  // ---- gate, learners, bias factor: one lane per sample ----
  if (slot == 0 && valid) {
    const float* zr = zs + smp * H;
    float mx, rden;
    softmax_stats(zr, M.R, mx, rden);
    float p0 = 0.f;
    for (int r = 0; r < M.R; ++r) {
      const float s = expf(zr[r] - mx) * rden;
      const float l = (M.task == DCTR_MLR_BINARY) ? sigmoidf_(zr[r]) : zr[r];
      p0 += s * l;
    }
    if (H > M.R) p0 = p0 * sigmoidf_(zr[M.R]);
    stg_f32(y + b, p0);
  }
  if (err && bad) atomicOr(err, 1);
}

// backward, one workgroup per tile of 64 samples: logit gradients from the saved z, the per-field rows of g_wide, and the
// tile's partial of every dense-weight gradient (samples in order)
__global__ __launch_bounds__(kThreads) void k_mlr_bwd(dctr_plan_t P, MlrDev M, const float* __restrict__ X, int64_t ldx,
                                                      int B, const float* __restrict__ g_y, const float* __restrict__ z,
                                                      int64_t ld_z, float* __restrict__ g_wide, int64_t ld_gw,
                                                      float* __restrict__ part) {
#pragma clang fp contract(off)
  step_priority();
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wv_id = tid >> 6, lane = tid & 63;
  const int b0 = blockIdx.x * kMlrBwdSPB;
  const int nrows = min(kMlrBwdSPB, B - b0);
  const Tile T = stage_tile(P, X, ldx, b0, nrows, kMlrBwdSPB, smem);
  const int nw = P.n_wide, H = M.H, R = M.R;
  float* gzs = T.red;                                  // [64][H]
  int32_t* hof = reinterpret_cast<int32_t*>(gzs + kMlrBwdSPB * H);
  for (int f = tid; f < nw; f += kThreads) hof[f] = ldg_i32(M.head_of + f);
  if (tid < nrows) {
    const int b = b0 + tid;
    float* zr = gzs + tid * H;
    for (int h = 0; h < H; ++h) zr[h] = ldg_f32(z + static_cast<int64_t>(b) * ld_z + h);
    float mx, rden;
    softmax_stats(zr, R, mx, rden);
    float p0 = 0.f;
    for (int r = 0; r < R; ++r) {
      const float l = (M.task == DCTR_MLR_BINARY) ? sigmoidf_(zr[r]) : zr[r];
      p0 += expf(zr[r] - mx) * rden * l;
    }
    const float g = ldg_f32(g_y + b);
    const float c = (H > R) ? sigmoidf_(zr[R]) : 1.f;
    const float gc = g * c;
    for (int r = 0; r < R; ++r) {
      const float s = expf(zr[r] - mx) * rden;
      const float l = (M.task == DCTR_MLR_BINARY) ? sigmoidf_(zr[r]) : zr[r];
      const float dl = (M.task == DCTR_MLR_BINARY) ? l * (1.f - l) : 1.f;
      zr[r] = gc * (s * (l - p0) + s * dl);
    }
    if (H > R) zr[R] = g * p0 * (c * (1.f - c));
  }
  __syncthreads();
  // g_wide: wave w writes rows w, w + 4, ... of the tile, a lane per field (+ the zero dense column)
  if (g_wide) {
    for (int s = wv_id; s < nrows; s += kNW) {
      float* row = g_wide + static_cast<int64_t>(b0 + s) * ld_gw;
      for (int f = lane; f <= nw; f += kWave) stg_f32(row + f, f < nw ? gzs[s * H + hof[f]] : 0.f);
    }
  }
  // dense-weight partials of this tile
  if (part) {
    for (int j = tid; j < M.n_dense; j += kThreads) {
      int h = 0;
      while (h + 1 < H && ldg_i32(M.dense_off + h + 1) <= j) ++h;
      const int col = ldg_i32(M.dense_cols + j);
      float acc = 0.f;
      for (int s = 0; s < nrows; ++s) acc += gzs[s * H + h] * T.xs[s * P.n_xcols + col];
      stg_f32(part + static_cast<int64_t>(blockIdx.x) * M.n_dense + j, acc);
    }
  }
}

// g_dense[j] = the tiles' partials in tile order
__global__ __launch_bounds__(kWave) void k_mlr_dense_reduce(const float* __restrict__ part, int n_tiles, int n_dense,
                                                            float* __restrict__ g_dense) {
#pragma clang fp contract(off)
  const int j = blockIdx.x * kWave + threadIdx.x;
  if (j >= n_dense) return;
  float acc = 0.f;
  for (int t = 0; t < n_tiles; ++t) acc += ldg_f32(part + static_cast<int64_t>(t) * n_dense + j);
  stg_f32(g_dense + j, acc);
}

// what the entry points reject (DCTR_EINVAL) or refuse (DCTR_ENOSUP); the forward's and the backward's LDS on success
int check_mlr(const dctr_plan_t* p, const dctr_mlr_t* m, size_t* lds_fwd, size_t* lds_bwd) {
  if (!p || !m) return DCTR_EINVAL;
  if (p->n_xcols <= 0 || p->n_wide < 0 || p->n_wide_fixed < 0 || p->n_wide_fixed > p->n_wide || (p->n_wide && !p->wide))
    return DCTR_EINVAL;
  if (m->n_dense < 0 || (m->task != DCTR_MLR_BINARY && m->task != DCTR_MLR_REGRESSION)) return DCTR_EINVAL;
  if (p->n_deep != 0 || p->n_dense != 0 || p->dense_off >= 0 || p->wdense_w || p->out_chunks) return DCTR_ENOSUP;
  if (!(p->flags & DCTR_PLAN_WIDE_PER_FIELD)) return DCTR_ENOSUP;
  if (m->n_regions < 2 || m->n_regions > DCTR_MLR_MAX_REGIONS) return DCTR_ENOSUP;
  if ((p->n_wide && !m->head_of) || !m->dense_off || (m->n_dense && (!m->dense_cols || !m->dense_w))) return DCTR_EINVAL;
  const int H = m->n_regions + (m->has_bias ? 1 : 0);
  *lds_fwd = mlr_lds(p, H, kMlrFwdSPB, true);
  *lds_bwd = mlr_lds(p, H, kMlrBwdSPB, false);
  if (*lds_fwd > kMaxTile || *lds_bwd > kMaxTile) return DCTR_ENOSUP;
  return DCTR_OK;
}

}  // namespace

extern "C" int dctr_mlr_supported(const dctr_plan_t* plan, const dctr_mlr_t* mlr) {
  size_t lf = 0, lb = 0;
  return check_mlr(plan, mlr, &lf, &lb) == DCTR_OK ? 1 : 0;
}

extern "C" int dctr_mlr_fwd(const dctr_plan_t* plan, const dctr_mlr_t* mlr, const float* X, int64_t ldx, int32_t B, float* y,
                            float* z, int64_t ld_z, int32_t* err, int32_t* ids_t, uint16_t* parts_t, const int32_t* units,
                            int32_t n_units, dctr_stream_t stream) {
  size_t lds = 0, lds_bwd = 0;
  if (int rc = check_mlr(plan, mlr, &lds, &lds_bwd)) return rc;
  if (!X || B < 0 || ldx < plan->n_xcols) return DCTR_EINVAL;
  if (B == 0) return DCTR_OK;
  const int H = mlr->n_regions + (mlr->has_bias ? 1 : 0);
  if (!y || !z || ld_z < H) return DCTR_EINVAL;
  if (ids_t && (!units || n_units <= 0 || n_units > plan->n_wide)) return DCTR_EINVAL;
  if (parts_t && !ids_t) return DCTR_EINVAL;
  const dctr_plan_ext_t* x = plan->ext;
  if (x && ids_t) return DCTR_EINVAL;   // (a general unit spans several X columns: dctr_embed_ids)
  if (x && x->amax && (x->ld_amax <= 0 || !x->am_wide_off)) return DCTR_EINVAL;
  const int n_parts = parts_t ? dctr_embed_update_partitions(plan, B) : 0;
  if (parts_t && (n_parts <= 0 || n_parts > 65535)) return DCTR_ENOSUP;
  const dim3 grid((B + kMlrFwdSPB - 1) / kMlrFwdSPB), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DCTR_LAUNCH(k_mlr_fwd, grid, block, lds, s, *plan, mlr_dev(mlr), X, ldx, B, y, z, ld_z, err, units, n_units, ids_t,
              parts_t, n_parts, x ? x->amax : nullptr, x ? x->ld_amax : 0, x ? x->am_wide_off : nullptr);
  return launch_status();
}

extern "C" size_t dctr_mlr_bwd_workspace_floats(const dctr_mlr_t* mlr, int32_t B) {
  if (!mlr || B <= 0 || mlr->n_dense <= 0) return 0;
  return static_cast<size_t>((B + kMlrBwdSPB - 1) / kMlrBwdSPB) * mlr->n_dense;
}

extern "C" int dctr_mlr_bwd(const dctr_plan_t* plan, const dctr_mlr_t* mlr, const float* X, int64_t ldx, int32_t B,
                            const float* g_y, const float* z, int64_t ld_z, float* g_wide, int64_t ld_gw, float* g_dense,
                            float* ws, dctr_stream_t stream) {
  size_t lds_fwd = 0, lds = 0;
  if (int rc = check_mlr(plan, mlr, &lds_fwd, &lds)) return rc;
  if (!X || B < 0 || ldx < plan->n_xcols) return DCTR_EINVAL;
  if (B == 0) return DCTR_OK;
  const int H = mlr->n_regions + (mlr->has_bias ? 1 : 0);
  if (!g_y || !z || ld_z < H) return DCTR_EINVAL;
  if (plan->n_wide > 0 && (!g_wide || ld_gw < plan->n_wide + 1)) return DCTR_EINVAL;
  if (mlr->n_dense > 0 && (!g_dense || !ws)) return DCTR_EINVAL;
  const int n_tiles = (B + kMlrBwdSPB - 1) / kMlrBwdSPB;
  const dim3 grid(n_tiles), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DCTR_LAUNCH(k_mlr_bwd, grid, block, lds, s, *plan, mlr_dev(mlr), X, ldx, B, g_y, z, ld_z,
              plan->n_wide > 0 ? g_wide : nullptr, ld_gw, mlr->n_dense > 0 ? ws : nullptr);
  if (int rc = launch_status()) return rc;
  if (mlr->n_dense > 0) {
    k_mlr_dense_reduce<<<dim3((mlr->n_dense + kWave - 1) / kWave), dim3(kWave), 0, s>>>(ws, n_tiles, mlr->n_dense, g_dense);
    return launch_status();
  }
  return DCTR_OK;
}
