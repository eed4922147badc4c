// embed.hip -- fused multi-table embedding lookup / scatter for gfx950 (MI355X).
//
// What the reference does with 2 x n_fields aten::embedding calls, n cat/sum/pow/mul launches and a
// dense [V, D] embedding_dense_backward per table (inputs.py:141-227, basemodel.py:63-92,354-380,
// interaction.py:26-34, sequence.py:49-77) is one gather kernel and one scatter kernel here.
//
// Mapping (HBM-bound, latency-critical at batch 4096):
//   * a workgroup is 4 waves (one per SIMD of a CU) that share SPB = 64 / LPR consecutive samples;
//   * LPR lanes of a wave form a "sample group"; lane g of the group owns floats [g*VEC, g*VEC+VEC)
//     of every embedding row, so a D=16 row is 4 lanes x dwordx4 = one 64-byte HBM burst;
//   * the 4 waves split the FIELDS (wave w takes fields w, w+4, ...): the per-wave dependent chain
//     (descriptor -> id -> address -> load) is 4x shorter and all 4 SIMDs issue loads;
//   * the workgroup first copies its X tile (ids + dense values, contiguous in memory) and the field
//     descriptors into LDS with coalesced loads -> one HBM round trip for all ids;
//   * every lane then issues ALL its row loads (branch-free, CH fields) before consuming any, so the
//     gather costs about one more HBM round trip;
//   * FM / wide-logit partials of the 4 waves meet in LDS; the final reduction inside a sample group
//     uses DPP shuffles.
#include "embed_tile.hpp"

using namespace dctr;

namespace {

// -------------------------------------------------------------------------------------------------
// forward
// -------------------------------------------------------------------------------------------------
template <int VEC, int LPR>
__global__ __launch_bounds__(kThreads) void k_embed_fwd(dctr_plan_t P, const float* __restrict__ X,
                                                        int64_t ldx, int B, float* __restrict__ out,
                                                        int64_t ldo, float* __restrict__ wide,
                                                        int64_t ldw, float* __restrict__ fm, int32_t* err,
                                                        const int32_t* __restrict__ units, int n_units,
                                                        int32_t* __restrict__ ids_t,
                                                        uint16_t* __restrict__ parts_t, int n_parts,
                                                        float* __restrict__ fm_s, int64_t lds_,
                                                        uint8_t* __restrict__ amax, int64_t ld_am,
                                                        const int32_t* __restrict__ am_deep_off,
                                                        const int32_t* __restrict__ am_wide_off) {
  // No fused multiply-adds in this body: the fused train launch (csrc/mlp.hip, dctr_embed_tower_train_step) computes the
  // same linear logit / FM term / sum_f e inside the tower kernel and must land on the same bits -- with contraction left
  // to the compiler the two bodies were contracted differently (round 4: losses equal for 30 steps, then off by one ulp).
#pragma clang fp contract(off)
  step_priority();
  constexpr int SPB = kWave / LPR;
  constexpr int CH = 8;   // row loads in flight per lane and per pass (x4 waves = 32 fields)
  constexpr int RED = 2 * VEC + 1;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wv_id = tid >> 6, lane = tid & 63;
  const int grp = lane / LPR, gl = lane % LPR;
  const int b0 = blockIdx.x * SPB;
  const int nrows = min(SPB, B - b0);
  const Tile T = stage_tile(P, X, ldx, b0, nrows, SPB, smem);
  const bool valid = grp < nrows;
  const int g = valid ? grp : 0;  // idle groups shadow group 0; their stores are masked
  const int b = b0 + g;
  const float* xr = T.xs + g * P.n_xcols;
  const int e0 = gl * VEC;
  int bad = 0;
  // P.out_chunks: output rows go to per-rank buffers (peer memory: the sharded step's push-style rows exchange)
  const auto row_of = [&](int row) -> float* {
    if (!P.out_chunks) return out + static_cast<int64_t>(row) * ldo;
    const int r = row / P.chunk_rows;
    return reinterpret_cast<float*>(P.out_chunks[r]) + static_cast<int64_t>(row - r * P.chunk_rows) * ldo;
  };
  float* orow = out ? row_of(b) : nullptr;
  // DCTR_PLAN_WIDE_PER_FIELD: the first-order weights go out per field (wrow[f]), only the dense half is summed (wrow[n_wide])
  const bool wpf = (P.flags & DCTR_PLAN_WIDE_PER_FIELD) != 0;
  float* wrow = wide ? wide + static_cast<int64_t>(b) * ldw : nullptr;

  // side output for dctr_embed_update: the ids of this tile, transposed to [unit][b] (64-byte runs)
  // (+ parts_t: the partition of dctr_embed_update each entry belongs to, so that its workgroups compare 16-bit tags
  // instead of dividing every id of the unit again)
  if (ids_t) {
    for (int k = tid; k < n_units * nrows; k += kThreads) {
      const int u = k / nrows, r = k - u * nrows;
      const int32_t id = static_cast<int32_t>(T.xs[r * P.n_xcols + ldg_i32(units + 4 * u + 2)]);
      ids_t[static_cast<int64_t>(u) * B + b0 + r] = id;
      if (parts_t) {
        const int di = ldg_i32(units + 4 * u), wi = ldg_i32(units + 4 * u + 1);
        const int64_t vocab = (di >= 0) ? T.deep[di].vocab : T.wide[wi].vocab;
        const uint32_t cid = (static_cast<uint64_t>(static_cast<int64_t>(id)) >= static_cast<uint64_t>(vocab))
                                 ? 0u : static_cast<uint32_t>(id);
        parts_t[static_cast<int64_t>(u) * B + b0 + r] = static_cast<uint16_t>(cid % static_cast<uint32_t>(n_parts));
      }
    }
  }

  // ---- wide (1-dim) tables: (wave, lane-in-group) pairs split the fields; loads issued first (embed_tile.hpp) ----
  float ws = 0.f;
  const int nwf = wide ? P.n_wide_fixed : 0;
  float wval[kWideCH];
  wide_issue<LPR>(T, xr, wv_id, gl, nwf, wval, bad);

  // ---- deep fixed-length fields: issue every row load of a pass, then consume -------------------
  Strip<VEC> S = strip_zero<VEC>(), Q = strip_zero<VEC>();
  const int nfix = out ? P.n_deep_fixed : 0;
  for (int f0 = wv_id; f0 < nfix; f0 += kNW * CH) {
    Strip<VEC> r[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const dctr_field_t& fd = T.deep[min(f0 + k * kNW, nfix - 1)];
      const int64_t id = checked(raw_id(xr, fd.col), fd.vocab, bad);
      // lanes past the row width re-read the row's first strip; their value is never used
      r[k] = strip_load<VEC>(fd.table + id * row_ld(fd) + ((e0 < fd.dim) ? e0 : 0));
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const dctr_field_t& fd = T.deep[min(f0 + k * kNW, nfix - 1)];
      const bool live = (f0 + k * kNW < nfix) && (e0 < fd.dim);
      if (live && valid) strip_store<VEC>(orow + fd.out_off + e0, r[k]);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float v = live ? r[k].v[i] : 0.f;
        S.v[i] += v;
        Q.v[i] += v * v;
      }
    }
  }

  // ---- deep VarLen fields ----------------------------------------------------------------------
  if (out) {
    for (int f = P.n_deep_fixed + wv_id; f < P.n_deep; f += kNW) {
      const dctr_field_t& fd = T.deep[f];
      const bool act = e0 < fd.dim;
      uint8_t* am = nullptr;
      if (amax && valid && fd.pool == DCTR_POOL_MAX) {
        const int off = ldg_i32(am_deep_off + f);
        if (off >= 0) am = amax + static_cast<int64_t>(b) * ld_am + off + e0;
      }
      const Strip<VEC> p = pool_field<VEC>(fd, xr, e0, act, bad, am);
      if (act) {
        if (valid) strip_store<VEC>(orow + fd.out_off + e0, p);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          S.v[i] += p.v[i];
          Q.v[i] += p.v[i] * p.v[i];
        }
      }
    }
    // dense block of combined_dnn_input (inputs.py:126-138)
    if (P.dense_off >= 0 && valid) {
      for (int j = wv_id * LPR + gl; j < P.n_dense; j += kNW * LPR) {
        stg_f32(orow + P.dense_off + j, xr[ldg_i32(P.dense_cols + j)]);
      }
    }
  }

  if (wide)
    ws = wide_finish<LPR>(P, T, xr, wv_id, gl, nwf, wval, valid, wrow,
                          (amax && valid) ? amax + static_cast<int64_t>(b) * ld_am : nullptr, am_wide_off, bad);

  // ---- the 4 waves' partials meet in LDS; wave 0 finishes --------------------------------------
  if (fm || wide || fm_s) {
    float* mine = T.red + (wv_id * kWave + lane) * RED;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      mine[i] = S.v[i];
      mine[VEC + i] = Q.v[i];
    }
    mine[2 * VEC] = ws;
    __syncthreads();
    if (wv_id == 0) {
      float st[VEC], qt[VEC], wt = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) st[i] = qt[i] = 0.f;
#pragma unroll
      for (int w = 0; w < kNW; ++w) {
        const float* o = T.red + (w * kWave + lane) * RED;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          st[i] += o[i];
          qt[i] += o[VEC + i];
        }
        wt += o[2 * VEC];
      }
      if (fm_s && valid && e0 < P.emb_dim) {
        Strip<VEC> sv;
#pragma unroll
        for (int i = 0; i < VEC; ++i) sv.v[i] = st[i];
        strip_store<VEC>(fm_s + static_cast<int64_t>(b) * lds_ + e0, sv);
      }
      if (fm) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < VEC; ++i) t += st[i] * st[i] - qt[i];
        t = group_sum<LPR>(t);
        if (gl == 0 && valid) stg_f32(fm + b, 0.5f * t);
      }
      if (wide) {
        wt = group_sum<LPR>(wt);
        if (gl == 0 && valid)
          stg_f32(P.out_chunks ? orow + (wide - out) : wide + static_cast<int64_t>(b) * ldw + (wpf ? P.n_wide : 0), wt);
      }
    }
  }
  if (err && bad) atomicOr(err, 1);
}

// -------------------------------------------------------------------------------------------------
// backward: scatter-add of the row gradients (+ FM backward folded in)
// -------------------------------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void scatter_strip(float* dst, const Strip<VEC>& g, float scale) {
#pragma unroll
  for (int i = 0; i < VEC; ++i) atomic_add_f32(dst + i, scale * g.v[i]);
}

// gradient of one pooled VarLen field routed back to its rows (sequence.py:49-77 under autograd)
template <int VEC, bool SGD>
__device__ __forceinline__ void unpool_field(const dctr_field_t& fd, const float* xr, int e0, bool act,
                                             const Strip<VEC>& gp, float scale) {
  if (!act) return;
  int bad = 0;  // ids were range-checked (and flagged) by the forward pass
  float* base = SGD ? fd.table : fd.gacc;
  const int64_t bld = SGD ? row_ld(fd) : fd.dim;   // gacc is contiguous
  const bool by_len = fd.len_col >= 0;
  const int64_t len_i = by_len ? raw_id(xr, fd.len_col) : 0;
  if (fd.pool == DCTR_POOL_MAX) {
    // arg-max per element, first maximum wins (torch.max on CPU); ties happen when every position
    // is masked -- then the gradient lands on position 0's row.
    float best[VEC];
    int64_t bid[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      best[i] = -INFINITY;
      bid[i] = 0;
    }
    for (int t = 0; t < fd.len; ++t) {
      const int64_t rid = raw_id(xr, fd.col + t);
      const bool m = by_len ? (static_cast<int64_t>(t) < len_i) : (rid != 0);
      const int64_t id = checked(rid, fd.vocab, bad);
      const Strip<VEC> row = strip_load<VEC>(fd.table + id * row_ld(fd) + e0);
      const float pen = m ? 0.f : 1e9f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float v = row.v[i] - pen;
        if (v > best[i]) {
          best[i] = v;
          bid[i] = id;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < VEC; ++i) atomic_add_f32(base + bid[i] * bld + e0 + i, scale * gp.v[i]);
    return;
  }
  float cnt = 0.f;
  if (fd.pool == DCTR_POOL_MEAN && !by_len)
    for (int t = 0; t < fd.len; ++t) cnt += (raw_id(xr, fd.col + t) != 0) ? 1.f : 0.f;
  Strip<VEC> gs = gp;
  if (fd.pool == DCTR_POOL_MEAN) {
    const float den = (by_len ? static_cast<float>(len_i) : cnt) + 1e-8f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) gs.v[i] = gp.v[i] / den;  // same rounding as autograd's div backward
  }
  for (int t = 0; t < fd.len; ++t) {
    const int64_t rid = raw_id(xr, fd.col + t);
    const bool m = by_len ? (static_cast<int64_t>(t) < len_i) : (rid != 0);
    if (!m) continue;
    const int64_t id = checked(rid, fd.vocab, bad);
    scatter_strip<VEC>(base + id * bld + e0, gs, scale);
  }
}

template <int VEC, int LPR, bool SGD>
__global__ __launch_bounds__(kThreads) void k_embed_bwd(dctr_plan_t P, const float* __restrict__ X,
                                                        int64_t ldx, int B,
                                                        const float* __restrict__ gout, int64_t ldg,
                                                        const float* __restrict__ out, int64_t ldo,
                                                        const float* __restrict__ gfm,
                                                        const float* __restrict__ gwide, float lr) {
  constexpr int SPB = kWave / LPR;
  constexpr int CH = 8;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wv_id = tid >> 6, lane = tid & 63;
  const int grp = lane / LPR, gl = lane % LPR;
  const int b0 = blockIdx.x * SPB;
  const int nrows = min(SPB, B - b0);
  const Tile T = stage_tile(P, X, ldx, b0, nrows, SPB, smem);
  if (grp >= nrows) return;  // no barrier below: whole groups may leave
  const int b = b0 + grp;
  const float* xr = T.xs + grp * P.n_xcols;
  const int e0 = gl * VEC;
  const float scale = SGD ? -lr : 1.f;
  int bad = 0;  // ids were range-checked (and flagged) by the forward pass

  // ---- wide tables: d wide[b] / d w_f[id] = 1 --------------------------------------------------
  if (gwide) {
    // DCTR_PLAN_WIDE_PER_FIELD: g_wide is [B, n_wide + 1], field f's gradient in column f
    const bool wpf = (P.flags & DCTR_PLAN_WIDE_PER_FIELD) != 0;
    const float* gwrow = wpf ? gwide + static_cast<int64_t>(b) * (P.n_wide + 1) : gwide + b;
    const float gw0 = wpf ? 0.f : ldg_f32(gwrow);
    for (int f = wv_id * LPR + gl; f < P.n_wide_fixed; f += kNW * LPR) {
      const dctr_field_t& fd = T.wide[f];
      const int64_t id = checked(raw_id(xr, fd.col), fd.vocab, bad);
      const float gw = wpf ? ldg_f32(gwrow + f) : gw0;
      atomic_add_f32((SGD ? fd.table + id * row_ld(fd) : fd.gacc + id), scale * gw);
    }
    for (int f = P.n_wide_fixed + wv_id * LPR + gl; f < P.n_wide; f += kNW * LPR) {
      const dctr_field_t& fd = T.wide[f];
      Strip<1> g1;
      g1.v[0] = wpf ? ldg_f32(gwrow + f) : gw0;
      unpool_field<1, SGD>(fd, xr, 0, true, g1, scale);
    }
  }
  if (!gout && !gfm) return;
  if (P.n_deep <= 0) return;

  // ---- FM backward needs S[d] = sum_f e[f][d]; e comes from the saved forward output (every wave
  //      rebuilds S from the L2-resident row rather than synchronising with its siblings) --------
  const float gf = gfm ? ldg_f32(gfm + b) : 0.f;
  const float* orow = out ? out + static_cast<int64_t>(b) * ldo : nullptr;
  const float* grow = gout ? gout + static_cast<int64_t>(b) * ldg : nullptr;
  Strip<VEC> S = strip_zero<VEC>();
  if (gfm) {
    for (int f0 = 0; f0 < P.n_deep; f0 += CH) {
      Strip<VEC> r[CH];
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const dctr_field_t& fd = T.deep[min(f0 + k, P.n_deep - 1)];
        r[k] = strip_load<VEC>(orow + fd.out_off + ((e0 < fd.dim) ? e0 : 0));
      }
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const dctr_field_t& fd = T.deep[min(f0 + k, P.n_deep - 1)];
        const bool live = (f0 + k < P.n_deep) && (e0 < fd.dim);
#pragma unroll
        for (int i = 0; i < VEC; ++i) S.v[i] += live ? r[k].v[i] : 0.f;
      }
    }
  }

  for (int f0 = wv_id; f0 < P.n_deep; f0 += kNW * CH) {
    Strip<VEC> g[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const dctr_field_t& fd = T.deep[min(f0 + k * kNW, P.n_deep - 1)];
      const int eo = fd.out_off + ((e0 < fd.dim) ? e0 : 0);
      g[k] = grow ? strip_load<VEC>(grow + eo) : strip_zero<VEC>();
      if (gfm) {
        const Strip<VEC> e = strip_load<VEC>(orow + eo);
#pragma unroll
        for (int i = 0; i < VEC; ++i) g[k].v[i] += gf * (S.v[i] - e.v[i]);
      }
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) {
      const int f = f0 + k * kNW;
      if (f < P.n_deep) {
        const dctr_field_t& fd = T.deep[f];
        const bool act = e0 < fd.dim;
        if (f < P.n_deep_fixed) {
          if (act) {
            const int64_t id = checked(raw_id(xr, fd.col), fd.vocab, bad);
            scatter_strip<VEC>((SGD ? fd.table + id * row_ld(fd) : fd.gacc + id * fd.dim) + e0, g[k], scale);
          }
        } else {
          unpool_field<VEC, SGD>(fd, xr, e0, act, g[k], scale);
        }
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------
// pass 2: consume gacc rows of this batch, apply the optimizer, leave gacc zero
// -------------------------------------------------------------------------------------------------
template <int OPT>
__device__ __forceinline__ void apply_elem(const dctr_field_t& fd, int64_t row, int e, float lr, float eps) {
  const float G = atomic_xchg_f32(fd.gacc + row * fd.dim + e, 0.f);
  if (G == 0.f) return;  // untouched, already consumed by a duplicate, or a genuinely zero gradient
  float* w = fd.table + row * row_ld(fd) + e;
  if (OPT == DCTR_OPT_ADAGRAD) {
    float* st = fd.state + row * state_ld(fd) + e;
    const float s = ldg_f32(st) + G * G;
    stg_f32(st, s);
    stg_f32(w, ldg_f32(w) - lr * (G / (sqrtf(s) + eps)));
  } else {
    stg_f32(w, ldg_f32(w) - lr * G);
  }
}

template <int VEC, int LPR, int OPT>
__global__ __launch_bounds__(kThreads) void k_embed_apply(dctr_plan_t P, const float* __restrict__ X,
                                                          int64_t ldx, int B, float lr, float eps) {
  constexpr int SPB = kWave / LPR;
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, wv_id = tid >> 6, lane = tid & 63;
  const int grp = lane / LPR, gl = lane % LPR;
  const int b0 = blockIdx.x * SPB;
  const int nrows = min(SPB, B - b0);
  const Tile T = stage_tile(P, X, ldx, b0, nrows, SPB, smem);
  if (grp >= nrows) return;
  const float* xr = T.xs + grp * P.n_xcols;
  const int e0 = gl * VEC;
  int bad = 0;
  for (int f = wv_id; f < P.n_deep; f += kNW) {
    const dctr_field_t& fd = T.deep[f];
    if (e0 >= fd.dim) continue;
    for (int t = 0; t < fd.len; ++t) {
      const int64_t id = checked(raw_id(xr, fd.col + t), fd.vocab, bad);
#pragma unroll
      for (int i = 0; i < VEC; ++i) apply_elem<OPT>(fd, id, e0 + i, lr, eps);
    }
  }
  for (int f = wv_id * LPR + gl; f < P.n_wide; f += kNW * LPR) {
    const dctr_field_t& fd = T.wide[f];
    for (int t = 0; t < fd.len; ++t)
      apply_elem<OPT>(fd, checked(raw_id(xr, fd.col + t), fd.vocab, bad), 0, lr, eps);
  }
}

// -------------------------------------------------------------------------------------------------
// host side
// -------------------------------------------------------------------------------------------------
size_t tile_bytes(const dctr_plan_t* p, int lpr, int vec) { return tile_bytes_red(p, lpr, 2 * vec + 1); }

}  // namespace

extern "C" int dctr_embed_fwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B,
                              float* out, int64_t ld_out, float* wide, int64_t ld_wide, float* fm,
                              int32_t* err, const int32_t* units, int32_t n_units, int32_t* ids_t,
                              uint16_t* parts_t, float* fm_s, int64_t ld_s, dctr_stream_t stream) {
  if (int rc = check_plan(plan, X, ldx, B)) return rc;
  if (wide && ld_wide < 1) return DCTR_EINVAL;
  if (plan->flags & DCTR_PLAN_WIDE_PER_FIELD) {
    if (wide && ld_wide < plan->n_wide + 1) return DCTR_EINVAL;
    if (plan->out_chunks) return DCTR_ENOSUP;   // (the sharded exchange carries one wide column per row)
  }
  if (B == 0) return DCTR_OK;
  if (fm && (plan->emb_dim <= 0 || !out)) return DCTR_EINVAL;  // FM needs the deep rows
  if (fm_s && (plan->emb_dim <= 0 || !out || ld_s < plan->emb_dim)) return DCTR_EINVAL;
  if (ids_t && (!units || n_units <= 0)) return DCTR_EINVAL;
  if (parts_t && !ids_t) return DCTR_EINVAL;
  if (plan->out_chunks && (plan->chunk_rows <= 0 || !out || (wide && (ld_wide != ld_out || wide < out || wide - out >= ld_out))))
    return DCTR_EINVAL;
  const int n_parts = parts_t ? dctr_embed_update_partitions(plan, B) : 0;
  if (parts_t && (n_parts <= 0 || n_parts > 65535)) return DCTR_ENOSUP;
  if (fm_s && plan->vec > 1 &&
      (ld_s % plan->vec != 0 || reinterpret_cast<uintptr_t>(fm_s) % (4 * plan->vec) != 0))
    return DCTR_EALIGN;
  const int vec = plan->vec;
  if (out && vec > 1 && (ld_out % vec != 0 || reinterpret_cast<uintptr_t>(out) % (4 * vec) != 0))
    return DCTR_EALIGN;
  const int lpr = lanes_per_row(plan, vec);
  const size_t lds = tile_bytes(plan, lpr, vec);
  if (lds > kMaxTile) return DCTR_ENOSUP;
  const int spb = kWave / lpr;
  const dim3 grid((B + spb - 1) / spb), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // general update units (dctr_plan_ext_t): the ids / tags side outputs come from dctr_embed_ids (a unit spans several X
  // columns); what the forward contributes is the arg-max side output of max-pooled fields
  const dctr_plan_ext_t* x = plan->ext;
  if (x && ids_t) return DCTR_EINVAL;
  if (x && x->amax && (x->ld_amax <= 0 || !x->am_deep_off || !x->am_wide_off)) return DCTR_EINVAL;
  DCTR_DISPATCH(vec, lpr, DCTR_LAUNCH((k_embed_fwd<VEC, LPR>), grid, block, lds, s, *plan, X, ldx, B, out, ld_out,
                                      wide, ld_wide, fm, err, units, n_units, ids_t, parts_t, n_parts, fm_s, ld_s,
                                      x ? x->amax : nullptr, x ? x->ld_amax : 0,
                                      x ? x->am_deep_off : nullptr, x ? x->am_wide_off : nullptr));
  return launch_status();
}

extern "C" int dctr_embed_bwd(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B,
                              const float* g_out, int64_t ld_g, const float* out, int64_t ld_out,
                              const float* g_fm, const float* g_wide, int32_t mode, float lr,
                              dctr_stream_t stream) {
  if (int rc = check_plan(plan, X, ldx, B)) return rc;
  if (B == 0) return DCTR_OK;
  if (mode != DCTR_BWD_ACCUM && mode != DCTR_BWD_SGD) return DCTR_EINVAL;
  if (mode == DCTR_BWD_ACCUM && !(plan->flags & DCTR_PLAN_HAS_GACC)) return DCTR_EINVAL;
  if (mode == DCTR_BWD_SGD && (plan->flags & DCTR_PLAN_HAS_MAXPOOL)) return DCTR_ENOSUP;
  if (g_fm && (!out || plan->emb_dim <= 0)) return DCTR_EINVAL;
  const int vec = plan->vec;
  if (vec > 1) {
    if (g_out && (ld_g % vec != 0 || reinterpret_cast<uintptr_t>(g_out) % (4 * vec) != 0))
      return DCTR_EALIGN;
    if (g_fm && (ld_out % vec != 0 || reinterpret_cast<uintptr_t>(out) % (4 * vec) != 0))
      return DCTR_EALIGN;
  }
  const int lpr = lanes_per_row(plan, vec);
  const size_t lds = tile_bytes(plan, lpr, vec);
  if (lds > kMaxTile) return DCTR_ENOSUP;
  const int spb = kWave / lpr;
  const dim3 grid((B + spb - 1) / spb), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mode == DCTR_BWD_SGD) {
    DCTR_DISPATCH(vec, lpr, DCTR_LAUNCH((k_embed_bwd<VEC, LPR, true>), grid, block, lds, s,
                                        *plan, X, ldx, B, g_out, ld_g, out, ld_out, g_fm, g_wide, lr));
  } else {
    DCTR_DISPATCH(vec, lpr, DCTR_LAUNCH((k_embed_bwd<VEC, LPR, false>), grid, block, lds, s,
                                        *plan, X, ldx, B, g_out, ld_g, out, ld_out, g_fm, g_wide, lr));
  }
  return launch_status();
}

extern "C" int dctr_embed_apply(const dctr_plan_t* plan, const float* X, int64_t ldx, int32_t B,
                                int32_t opt, float lr, float eps, dctr_stream_t stream) {
  if (int rc = check_plan(plan, X, ldx, B)) return rc;
  if (B == 0) return DCTR_OK;
  if (!(plan->flags & DCTR_PLAN_HAS_GACC)) return DCTR_EINVAL;
  if (opt != DCTR_OPT_SGD && opt != DCTR_OPT_ADAGRAD) return DCTR_EINVAL;
  if (opt == DCTR_OPT_ADAGRAD && !(plan->flags & DCTR_PLAN_HAS_STATE)) return DCTR_EINVAL;
  const int vec = plan->vec;
  const int lpr = lanes_per_row(plan, vec);
  const size_t lds = tile_bytes(plan, lpr, vec);
  if (lds > kMaxTile) return DCTR_ENOSUP;
  const int spb = kWave / lpr;
  const dim3 grid((B + spb - 1) / spb), block(kThreads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (opt == DCTR_OPT_ADAGRAD) {
    DCTR_DISPATCH(vec, lpr, DCTR_LAUNCH((k_embed_apply<VEC, LPR, DCTR_OPT_ADAGRAD>), grid, block, lds, s,
                                        *plan, X, ldx, B, lr, eps));
  } else {
    DCTR_DISPATCH(vec, lpr, DCTR_LAUNCH((k_embed_apply<VEC, LPR, DCTR_OPT_SGD>), grid, block, lds, s,
                                        *plan, X, ldx, B, lr, eps));
  }
  return launch_status();
}
