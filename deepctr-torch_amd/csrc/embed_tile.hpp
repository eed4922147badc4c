// embed_tile.hpp -- what the lookup kernels share (csrc/embed.hip: dctr_embed_fwd / _bwd / _apply; csrc/pair_embed.hip:
// dctr_pair_embed_fwd / _bwd): the workgroup geometry, the LDS tile of descriptors + X rows, the id helpers, VarLen
// pooling and the first-order ("wide") logit.  ONE definition of the wide logit: both forwards split the wide fields over
// (wave, lane in group) the same way and add the partials in the same order, so their `wide` agree bit for bit.
//
// Geometry: a workgroup is kNW waves that share SPB = 64 / LPR consecutive samples; LPR lanes of a wave form a sample
// group (lane g of the group owns floats [g * VEC, g * VEC + VEC) of a row); lane group `grp` of EVERY wave belongs to
// sample b0 + grp, the waves split the fields.
#pragma once

#include "common.hpp"

namespace dctr {
namespace {

constexpr int kNW = 4;  // waves per workgroup
constexpr int kThreads = kNW * kWave;
constexpr int kFieldWords = sizeof(dctr_field_t) / 4;
static_assert(sizeof(dctr_field_t) == 64, "dctr_field_t must be 64 bytes");
static_assert(sizeof(dctr_plan_t) == 112, "dctr_plan_t layout changed: update the Python binding");

struct Tile {
  const dctr_field_t* deep;
  const dctr_field_t* wide;
  const float* xs;  // [SPB][n_xcols]
  float* red;       // [kNW][kWave][RED] cross-wave reduction scratch
};

// Copy descriptors and the X tile of samples [b0, b0+nrows) into LDS (whole workgroup).
__device__ __forceinline__ Tile stage_tile(const dctr_plan_t& P, const float* __restrict__ X,
                                           int64_t ldx, int b0, int nrows, int spb,
                                           unsigned char* smem) {
  const int tid = threadIdx.x;
  uint32_t* w = reinterpret_cast<uint32_t*>(smem);
  const int nd = P.n_deep * kFieldWords, nw = P.n_wide * kFieldWords;
  const uint32_t* gd = reinterpret_cast<const uint32_t*>(P.deep);
  const uint32_t* gw = reinterpret_cast<const uint32_t*>(P.wide);
  for (int i = tid; i < nd; i += kThreads) w[i] = gd[i];
  for (int i = tid; i < nw; i += kThreads) w[nd + i] = gw[i];
  float* xs = reinterpret_cast<float*>(w + nd + nw);
  const int nc = P.n_xcols;
  const int n = nrows * nc;
  if (ldx == nc) {
    const float* src = X + static_cast<int64_t>(b0) * ldx;
    for (int i = tid; i < n; i += kThreads) xs[i] = src[i];
  } else {
    for (int i = tid; i < n; i += kThreads) {
      const int r = i / nc, c = i - r * nc;
      xs[i] = X[static_cast<int64_t>(b0 + r) * ldx + c];
    }
  }
  __syncthreads();
  Tile t;
  t.deep = reinterpret_cast<const dctr_field_t*>(w);
  t.wide = reinterpret_cast<const dctr_field_t*>(w + nd);
  t.xs = xs;
  t.red = xs + ((spb * nc + 3) & ~3);
  return t;
}

// LDS bytes of the tile: descriptors, SPB rows of X, `red` floats per thread of cross-wave scratch
inline size_t tile_bytes_red(const dctr_plan_t* p, int lpr, int red) {
  const size_t spb = kWave / lpr;
  return static_cast<size_t>(p->n_deep + p->n_wide) * sizeof(dctr_field_t) +
         ((spb * p->n_xcols + 3) & ~size_t(3)) * sizeof(float) +
         static_cast<size_t>(kNW) * kWave * red * sizeof(float);
}

// id = Tensor.long() of the float in X: truncation toward zero (basemodel.py:369).  float32 holds
// integers exactly only below 2^24, so a 32-bit convert (one v_cvt_i32_f32) is exact
// for every id the reference can represent.
__device__ __forceinline__ int64_t raw_id(const float* xr, int col) {
  return static_cast<int64_t>(static_cast<int32_t>(xr[col]));
}

// Out-of-range ids read row 0 and raise `bad`; the caller ORs it into the error word once.
__device__ __forceinline__ int64_t checked(int64_t id, int64_t vocab, int& bad) {
  const bool oob = static_cast<uint64_t>(id) >= static_cast<uint64_t>(vocab);
  bad |= oob ? 1 : 0;
  return oob ? 0 : id;
}

// Pool one VarLen field for this lane's strip of the row.  Mirrors SequencePoolingLayer.forward
// (sequence.py:49-77) as called from get_varlen_pooling_list (inputs.py:141-155):
//   mask mode   (len_col < 0): m_t = (id_t != 0); length = sum_t m_t
//   length mode (len_col >= 0): m_t = (t < length)
//   sum : sum_t m_t e_t        mean: that / (length + 1e-8)        max: max_t (e_t - (1 - m_t) * 1e9)
//   am (nullable; max pooling): this sample's arg-max bytes of the field at e0 -- the position of the FIRST maximum per
//   element (torch.max's backward routes the gradient there), the side output dctr_embed_update reads
template <int VEC>
__device__ __forceinline__ Strip<VEC> pool_field(const dctr_field_t& fd, const float* xr, int e0,
                                                 bool act, int& bad, uint8_t* am = nullptr) {
  const bool by_len = fd.len_col >= 0;
  const int64_t len_i = by_len ? raw_id(xr, fd.len_col) : 0;
  Strip<VEC> acc;
  int arg[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    acc.v[i] = (fd.pool == DCTR_POOL_MAX) ? -INFINITY : 0.f;
    arg[i] = 0;
  }
  float cnt = 0.f;
  for (int t = 0; t < fd.len; ++t) {
    const int64_t rid = raw_id(xr, fd.col + t);
    const bool m = by_len ? (static_cast<int64_t>(t) < len_i) : (rid != 0);
    const int64_t id = checked(rid, fd.vocab, bad);
    Strip<VEC> row = act ? strip_load<VEC>(fd.table + id * row_ld(fd) + e0) : strip_zero<VEC>();
    if (fd.pool == DCTR_POOL_MAX) {
      const float pen = m ? 0.f : 1e9f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float v = row.v[i] - pen;
        arg[i] = (v > acc.v[i]) ? t : arg[i];
        acc.v[i] = (v > acc.v[i]) ? v : acc.v[i];
      }
    } else if (m) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) acc.v[i] += row.v[i];
    }
    cnt += m ? 1.f : 0.f;
  }
  if (fd.pool == DCTR_POOL_MEAN) {
    const float den = (by_len ? static_cast<float>(len_i) : cnt) + 1e-8f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc.v[i] = acc.v[i] / den;
  }
  if (am && act && fd.pool == DCTR_POOL_MAX) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) *(DCTR_GLOBAL uint8_t*)(am + i) = static_cast<uint8_t>(arg[i]);
  }
  return acc;
}

// ---- the first-order logit: sum_f w_f[id] (+ pooled VarLen) + dense . Linear.weight (basemodel.py:63-92) --------------
// (wave, lane-in-group) pairs split the fixed-length wide fields: slot k of a lane is field (k * kNW + wave) * LPR + gl.
// wide_issue puts the first kWideCH loads of a lane in flight (the caller issues its row loads behind them);
// wide_finish consumes them, walks the remaining fields and returns the lane's partial sum -- or, for a
// DCTR_PLAN_WIDE_PER_FIELD plan, stores the weights per field at wrow[f] and returns the dense half only.
// Branch-free: slots past the last field re-read the last field and are masked when summed.
// wide_total adds the kNW waves' partials (parked in LDS `stride` floats apart at offset `off`) in wave order, then the
// LPR lanes of the sample group.  No fused multiply-adds: dctr_embed_tower_train_step computes the same logit inside the
// tower kernel and must land on the same bits.
constexpr int kWideCH = 2;  // wide loads in flight per lane ahead of the row loads

template <int LPR>
__device__ __forceinline__ void wide_issue(const Tile& T, const float* xr, int wv_id, int gl, int nwf,
                                           float (&wval)[kWideCH], int& bad) {
#pragma unroll
  for (int k = 0; k < kWideCH; ++k) wval[k] = 0.f;
  if (nwf > 0) {
#pragma unroll
    for (int k = 0; k < kWideCH; ++k) {
      const int f = (k * kNW + wv_id) * LPR + gl;
      const dctr_field_t& fd = T.wide[min(f, nwf - 1)];
      wval[k] = ldg_f32(fd.table + checked(raw_id(xr, fd.col), fd.vocab, bad) * row_ld(fd));
    }
  }
}

template <int LPR>
__device__ __forceinline__ float wide_finish(const dctr_plan_t& P, const Tile& T, const float* xr, int wv_id, int gl,
                                             int nwf, const float (&wval)[kWideCH], bool valid, float* wrow,
                                             uint8_t* am_row, const int32_t* __restrict__ am_wide_off, int& bad) {
#pragma clang fp contract(off)
  const bool wpf = (P.flags & DCTR_PLAN_WIDE_PER_FIELD) != 0;
  float ws = 0.f;
  if (wpf) {
#pragma unroll
    for (int k = 0; k < kWideCH; ++k) {
      const int f = (k * kNW + wv_id) * LPR + gl;
      if (f < nwf && valid) stg_f32(wrow + f, wval[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < kWideCH; ++k) ws += ((k * kNW + wv_id) * LPR + gl < nwf) ? wval[k] : 0.f;
  }
  for (int f = (kWideCH * kNW + wv_id) * LPR + gl; f < nwf; f += kNW * LPR) {  // > 8*LPR wide fields
    const dctr_field_t& fd = T.wide[f];
    const float wv = ldg_f32(fd.table + checked(raw_id(xr, fd.col), fd.vocab, bad) * row_ld(fd));
    if (!wpf) ws += wv;
    else if (valid) stg_f32(wrow + f, wv);
  }
  for (int f = P.n_wide_fixed + wv_id * LPR + gl; f < P.n_wide; f += kNW * LPR) {  // pooled VarLen
    const dctr_field_t& fd = T.wide[f];
    uint8_t* am = nullptr;
    if (am_row && valid && fd.pool == DCTR_POOL_MAX) {
      const int off = ldg_i32(am_wide_off + f);
      if (off >= 0) am = am_row + off;
    }
    const float wv = pool_field<1>(fd, xr, 0, true, bad, am).v[0];
    if (!wpf) ws += wv;
    else if (valid) stg_f32(wrow + f, wv);
  }
  if (P.wdense_w)
    for (int j = wv_id * LPR + gl; j < P.n_wdense; j += kNW * LPR)
      ws += xr[ldg_i32(P.wdense_cols + j)] * ldg_f32(P.wdense_w + j);
  return ws;
}

template <int LPR>
__device__ __forceinline__ float wide_total(const float* red, int stride, int off, int lane) {
#pragma clang fp contract(off)
  float wt = 0.f;
#pragma unroll
  for (int w = 0; w < kNW; ++w) wt += red[(w * kWave + lane) * stride + off];
  return group_sum<LPR>(wt);
}

// lanes per sample group: the smallest power of two that covers max_dim / vec
inline int lanes_per_row(const dctr_plan_t* p, int vec) {
  int need = (p->max_dim + vec - 1) / vec;
  int lpr = 1;
  while (lpr < need) lpr <<= 1;
  return lpr;
}

inline int check_plan(const dctr_plan_t* p, const float* X, int64_t ldx, int32_t B) {
  if (!p || !X || B < 0 || p->n_xcols <= 0 || ldx < p->n_xcols) return DCTR_EINVAL;
  if (p->n_deep < 0 || p->n_wide < 0 || p->n_deep_fixed > p->n_deep || p->n_wide_fixed > p->n_wide)
    return DCTR_EINVAL;
  if ((p->n_deep && !p->deep) || (p->n_wide && !p->wide)) return DCTR_EINVAL;
  if (p->vec != 1 && p->vec != 2 && p->vec != 4) return DCTR_EINVAL;
  if (p->max_dim > 64 * p->vec) return DCTR_ENOSUP;
  return DCTR_OK;
}

#define DCTR_DISPATCH_LPR(VEC_, lpr, ...)                                \
  switch (lpr) {                                                         \
    case 1: { constexpr int VEC = VEC_, LPR = 1; __VA_ARGS__; } break;   \
    case 2: { constexpr int VEC = VEC_, LPR = 2; __VA_ARGS__; } break;   \
    case 4: { constexpr int VEC = VEC_, LPR = 4; __VA_ARGS__; } break;   \
    case 8: { constexpr int VEC = VEC_, LPR = 8; __VA_ARGS__; } break;   \
    case 16: { constexpr int VEC = VEC_, LPR = 16; __VA_ARGS__; } break; \
    case 32: { constexpr int VEC = VEC_, LPR = 32; __VA_ARGS__; } break; \
    default: { constexpr int VEC = VEC_, LPR = 64; __VA_ARGS__; } break; \
  }

// Dynamic LDS above the 64 KB default needs the kernel's attribute raised first (gfx950: 160 KB per workgroup).  The
// tile of a plan with very many input columns (hundreds of VarLen positions, thousands of fields) goes up to kMaxTile.
constexpr size_t kMaxTile = 156 * 1024;
#define DCTR_LAUNCH(kernel, grid, block, lds, stream, ...)                                                       \
  do {                                                                                                           \
    auto kfn_ = kernel;                                                                                          \
    if ((lds) > 64 * 1024)                                                                                       \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kfn_), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                static_cast<int>(lds));                                                          \
    kfn_<<<grid, block, lds, stream>>>(__VA_ARGS__);                                                             \
  } while (0)

#define DCTR_DISPATCH(vec, lpr, ...)                              \
  if ((vec) == 4) { DCTR_DISPATCH_LPR(4, lpr, __VA_ARGS__) }      \
  else if ((vec) == 2) { DCTR_DISPATCH_LPR(2, lpr, __VA_ARGS__) } \
  else { DCTR_DISPATCH_LPR(1, lpr, __VA_ARGS__) }

}  // namespace
}  // namespace dctr
