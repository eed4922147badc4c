// iafm.hip -- the input-aware FM of IFM / DIFM (ifm.py:74-83, difm.py:96-102, basemodel.py:80-91), forward and backward.
//
//   m      = F * softmax_f(Z1)   |   Z1 + Z2
//   y_lin  = sum_f m_f * wl_f + wl_dense
//   y_fm   = 0.5 * sum_d ((sum_f m_f e_fd)^2 - sum_f (m_f e_fd)^2)
//
// What the reference spells as a softmax, two broadcasts, a concat, FM's five launches and the refined wide sum (and
// everything autograd adds behind them) is one streaming launch per direction here.
//
// Mapping (HBM-bound): LPR = DL * FL lanes form a sample group.  Lane (fl, dl) of the group owns the strip
// [dl*VEC, dl*VEC + VEC) of the fields fl, fl + FL, fl + 2 FL, ... -- at most kKF of them, all loaded before any is
// consumed and kept in registers for the second pass over f (the row is read ONCE).  Lane index = fl * DL + dl, so the
// lanes of a group read LPR * VEC consecutive floats per load (a D = 16 row is 4 lanes x dwordx4).  S_d = sum_f m_f e_fd
// meets across the FL lanes of a strip by xor shuffles over the fl bits, scalars across the whole group; the order of
// every sum is fixed by the lane layout: no atomics, identical bits from run to run.  E is the gather's buffer read in
// place, gE has its row layout, so it joins the tower's input gradient without a re-layout.
#include "common.hpp"

using namespace dctr;

namespace {

constexpr int kT = 256;  // threads per workgroup
constexpr int kKF = 8;   // fields a lane keeps in registers

struct Lanes {
  int vec, dl, fl, lpr;   // dl, fl, lpr powers of two, lpr = dl * fl <= 64
};

int pow2_ceil(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// the lane layout for (F, D) with strips of `vec` floats; false: the row does not fit kKF strips per lane of a wave
bool lanes_for(int F, int D, int vec, Lanes* L) {
  if (F < 1 || F > 64 || D < 1) return false;
  const int dl = pow2_ceil((D + vec - 1) / vec);
  const int fl = pow2_ceil((F + kKF - 1) / kKF);
  if (dl > 64 || dl * fl > 64) return false;
  L->vec = vec;
  L->dl = dl;
  L->fl = fl;
  L->lpr = dl * fl;
  return true;
}

int natural_vec(int D) { return D % 4 == 0 ? 4 : (D % 2 == 0 ? 2 : 1); }

bool rows_aligned(const void* p, int64_t ld, int vec) {
  return ld % vec == 0 && reinterpret_cast<uintptr_t>(p) % (4 * vec) == 0;
}

// sum / max over the lanes whose index differs in the bits [lo, hi) (powers of two): xor butterflies, so every lane of the
// set ends with the same value, added in the same order
__device__ __forceinline__ float bits_sum(float v, int lo, int hi) {
  for (int m = lo; m < hi; m <<= 1) v += __shfl_xor(v, m, kWave);
  return v;
}
// the same for N values at once: the N shuffles of a level are independent and overlap
template <int N>
__device__ __forceinline__ void bits_sum_n(float (&v)[N], int lo, int hi) {
  for (int m = lo; m < hi; m <<= 1) {
    float t[N];
#pragma unroll
    for (int i = 0; i < N; ++i) t[i] = __shfl_xor(v[i], m, kWave);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] += t[i];
  }
}
__device__ __forceinline__ float bits_max(float v, int lo, int hi) {
  for (int m = lo; m < hi; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
  return v;
}

struct Who {
  int b, fl, e0;
  bool valid, d_on, lead;   // lead: the lane of a strip column that speaks for its fields (dl == 0)
};
__device__ __forceinline__ Who who_am_i(int B, int D, int vec, int dl_n, int lpr) {
  const int tid = threadIdx.x;
  const int grp = tid / lpr, gl = tid - grp * lpr;
  const int dl = gl & (dl_n - 1);
  Who w;
  w.fl = gl / dl_n;
  w.b = blockIdx.x * (kT / lpr) + grp;
  w.valid = w.b < B;
  if (!w.valid) w.b = B - 1;   // idle groups shadow the last sample; their stores are masked
  w.e0 = dl * vec;
  w.d_on = w.e0 < D;
  w.lead = dl == 0;
  return w;
}

template <int VEC>
__global__ __launch_bounds__(kT) void k_iafm_fwd(const float* __restrict__ E, int64_t lde, const float* __restrict__ Wl,
                                                 int64_t ldw, int n_wl, const float* __restrict__ Z1, int64_t ldz1,
                                                 const float* __restrict__ Z2, int64_t ldz2, int mode, int B, int F, int D,
                                                 int dl_n, int lpr, float* __restrict__ m_out, int64_t ldm,
                                                 float* __restrict__ y_lin, float* __restrict__ y_fm) {
  // No fused multiply-adds here: (sum_f v)^2 - sum_f v^2 of a single field is exactly 0 in the reference (ifm.py:81-83 on
  // one field); contracted to fma(s, s, -q) it comes out as the rounding error of s * s.
#pragma clang fp contract(off)
  const Who w = who_am_i(B, D, VEC, dl_n, lpr);
  const int fl_n = lpr / dl_n;
  const int64_t b = w.b;
  const float* erow = E + b * lde + w.e0;

  // every load of the sample first: the row's strips, the fields' Z and first-order weights
  Strip<VEC> e[kKF];
  float z[kKF], wl[kKF];
#pragma unroll
  for (int k = 0; k < kKF; ++k) {
    const int f = k * fl_n + w.fl;
    const bool on = f < F;
    e[k] = (on && w.d_on) ? strip_load<VEC>(erow + f * D) : strip_zero<VEC>();
    z[k] = on ? ldg_f32(Z1 + b * ldz1 + f) : 0.f;
    if (mode == DCTR_IAFM_SUM && on) z[k] += ldg_f32(Z2 + b * ldz2 + f);
    wl[k] = (Wl && f < n_wl) ? ldg_f32(Wl + b * ldw + f) : 0.f;
  }
  const float wdense = Wl ? ldg_f32(Wl + b * ldw + n_wl) : 0.f;

  // m_f
  float m[kKF];
  if (mode == DCTR_IAFM_SOFTMAX) {
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < kKF; ++k) mx = (k * fl_n + w.fl < F) ? fmaxf(mx, z[k]) : mx;
    mx = bits_max(mx, dl_n, lpr);
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < kKF; ++k) {
      m[k] = (k * fl_n + w.fl < F) ? expf(z[k] - mx) : 0.f;
      den += m[k];
    }
    den = bits_sum(den, dl_n, lpr);
    const float Ff = static_cast<float>(F);
#pragma unroll
    for (int k = 0; k < kKF; ++k) m[k] = Ff * (m[k] / den);
  } else {
#pragma unroll
    for (int k = 0; k < kKF; ++k) m[k] = z[k];
  }

  // S_d, Q_d over this lane's fields, then over the FL lanes of the strip
  Strip<VEC> S = strip_zero<VEC>(), Q = strip_zero<VEC>();
  float lin = 0.f;
#pragma unroll
  for (int k = 0; k < kKF; ++k) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float v = m[k] * e[k].v[i];
      S.v[i] += v;
      Q.v[i] += v * v;
    }
    lin += m[k] * wl[k];
  }
  float sq[2 * VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    sq[i] = S.v[i];
    sq[VEC + i] = Q.v[i];
  }
  bits_sum_n<2 * VEC>(sq, dl_n, lpr);
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) t += sq[i] * sq[i] - sq[VEC + i];
  // one lane per strip (fl == 0) carries the strip's term, one lane per field column (dl == 0) its wide products
  t = bits_sum((w.fl == 0 && w.d_on) ? t : 0.f, 1, dl_n);
  lin = bits_sum(w.lead ? lin : 0.f, dl_n, lpr);
  if (!w.valid) return;
  if (w.lead) {
#pragma unroll
    for (int k = 0; k < kKF; ++k) {
      const int f = k * fl_n + w.fl;
      if (f < F) stg_f32(m_out + b * ldm + f, m[k]);
    }
    if (w.fl == 0) {
      stg_f32(y_fm + b, 0.5f * t);
      stg_f32(y_lin + b, lin + wdense);
    }
  }
}

template <int VEC>
__global__ __launch_bounds__(kT) void k_iafm_bwd(const float* __restrict__ E, int64_t lde, const float* __restrict__ Wl,
                                                 int64_t ldw, int n_wl, const float* __restrict__ M, int64_t ldm, int mode,
                                                 int B, int F, int D, int dl_n, int lpr, const float* __restrict__ g_lin,
                                                 const float* __restrict__ g_fm, float* __restrict__ gE, int64_t ldge,
                                                 float* __restrict__ gWl, int64_t ldgw, float* __restrict__ gZ,
                                                 int64_t ldgz) {
  const Who w = who_am_i(B, D, VEC, dl_n, lpr);
  const int fl_n = lpr / dl_n;
  const int64_t b = w.b;
  const float* erow = E + b * lde + w.e0;

  Strip<VEC> e[kKF];
  float m[kKF], wl[kKF];
#pragma unroll
  for (int k = 0; k < kKF; ++k) {
    const int f = k * fl_n + w.fl;
    const bool on = f < F;
    e[k] = (on && w.d_on) ? strip_load<VEC>(erow + f * D) : strip_zero<VEC>();
    m[k] = on ? ldg_f32(M + b * ldm + f) : 0.f;
    wl[k] = (Wl && f < n_wl) ? ldg_f32(Wl + b * ldw + f) : 0.f;
  }
  const float gl = g_lin ? ldg_f32(g_lin + b) : 0.f;
  const float gf = g_fm ? ldg_f32(g_fm + b) : 0.f;

  Strip<VEC> S = strip_zero<VEC>();
#pragma unroll
  for (int k = 0; k < kKF; ++k) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) S.v[i] += m[k] * e[k].v[i];
  }
  bits_sum_n<VEC>(S.v, dl_n, lpr);

  // gE_fd = g_fm m_f (S_d - v_fd);  gm_f = g_lin wl_f + g_fm sum_d e_fd (S_d - v_fd)
  float gm[kKF];
#pragma unroll
  for (int k = 0; k < kKF; ++k) {
    const int f = k * fl_n + w.fl;
    Strip<VEC> g;
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
      const float r = S.v[i] - m[k] * e[k].v[i];
      g.v[i] = gf * m[k] * r;
      a += e[k].v[i] * r;
    }
    if (w.valid && w.d_on && f < F) strip_store<VEC>(gE + b * ldge + w.e0 + f * D, g);
    gm[k] = a;
  }
  bits_sum_n<kKF>(gm, 1, dl_n);      // sum_d over the DL lanes of each field
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < kKF; ++k) {
    gm[k] = gl * wl[k] + gf * gm[k];
    dot += gm[k] * m[k];
  }
  if (mode == DCTR_IAFM_SOFTMAX) {
    dot = bits_sum(w.lead ? dot : 0.f, dl_n, lpr) / static_cast<float>(F);
#pragma unroll
    for (int k = 0; k < kKF; ++k) gm[k] = m[k] * (gm[k] - dot);
  }
  if (!w.valid || !w.lead) return;
#pragma unroll
  for (int k = 0; k < kKF; ++k) {
    const int f = k * fl_n + w.fl;
    if (f < F) {
      stg_f32(gZ + b * ldgz + f, gm[k]);
      if (gWl && f < n_wl) stg_f32(gWl + b * ldgw + f, gl * m[k]);
    }
  }
  if (gWl && w.fl == 0) stg_f32(gWl + b * ldgw + n_wl, gl);
}

}  // namespace

extern "C" int dctr_iafm_supported(int32_t F, int32_t D) {
  Lanes L;
  return lanes_for(F, D, D >= 1 ? natural_vec(D) : 1, &L) ? 1 : 0;
}

extern "C" int dctr_iafm_fwd(const float* E, int64_t ld_e, const float* Wl, int64_t ld_w, int32_t n_wl, const float* Z1,
                             int64_t ld_z1, const float* Z2, int64_t ld_z2, int32_t mode, int32_t B, int32_t F, int32_t D,
                             float* m, int64_t ld_m, float* y_lin, float* y_fm, dctr_stream_t stream) {
  if (!E || !Z1 || !m || !y_lin || !y_fm || B < 0 || F < 1 || D < 1) return DCTR_EINVAL;
  if (mode != DCTR_IAFM_SOFTMAX && mode != DCTR_IAFM_SUM) return DCTR_EINVAL;
  if (ld_e < static_cast<int64_t>(F) * D || ld_z1 < F || ld_m < F) return DCTR_EINVAL;
  if (mode == DCTR_IAFM_SUM && (!Z2 || ld_z2 < F)) return DCTR_EINVAL;
  if (Wl && ((n_wl != 0 && n_wl != F) || ld_w < n_wl + 1)) return DCTR_EINVAL;
  int vec = natural_vec(D);
  while (vec > 1 && !rows_aligned(E, ld_e, vec)) vec >>= 1;
  Lanes L;
  if (!lanes_for(F, D, vec, &L)) return DCTR_ENOSUP;
  if (B == 0) return DCTR_OK;
  const int spb = kT / L.lpr;
  const dim3 grid((B + spb - 1) / spb), block(kT);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define IAFM_FWD(V) k_iafm_fwd<V><<<grid, block, 0, s>>>(E, ld_e, Wl, ld_w, Wl ? n_wl : 0, Z1, ld_z1, Z2, ld_z2, mode, B, F, \
                                                        D, L.dl, L.lpr, m, ld_m, y_lin, y_fm)
  if (vec == 4) IAFM_FWD(4);
  else if (vec == 2) IAFM_FWD(2);
  else IAFM_FWD(1);
#undef IAFM_FWD
  return launch_status();
}

extern "C" int dctr_iafm_bwd(const float* E, int64_t ld_e, const float* Wl, int64_t ld_w, int32_t n_wl, const float* m,
                             int64_t ld_m, int32_t mode, int32_t B, int32_t F, int32_t D, const float* g_lin,
                             const float* g_fm, float* gE, int64_t ld_ge, float* gWl, int64_t ld_gw, float* gZ, int64_t ld_gz,
                             dctr_stream_t stream) {
  if (!E || !m || !gE || !gZ || B < 0 || F < 1 || D < 1) return DCTR_EINVAL;
  if (mode != DCTR_IAFM_SOFTMAX && mode != DCTR_IAFM_SUM) return DCTR_EINVAL;
  if (ld_e < static_cast<int64_t>(F) * D || ld_ge < static_cast<int64_t>(F) * D || ld_m < F || ld_gz < F) return DCTR_EINVAL;
  if (Wl && ((n_wl != 0 && n_wl != F) || ld_w < n_wl + 1)) return DCTR_EINVAL;
  if (gWl && (!Wl || ld_gw < n_wl + 1)) return DCTR_EINVAL;
  int vec = natural_vec(D);
  while (vec > 1 && !(rows_aligned(E, ld_e, vec) && rows_aligned(gE, ld_ge, vec))) vec >>= 1;
  Lanes L;
  if (!lanes_for(F, D, vec, &L)) return DCTR_ENOSUP;
  if (B == 0) return DCTR_OK;
  const int spb = kT / L.lpr;
  const dim3 grid((B + spb - 1) / spb), block(kT);
  hipStream_t s = static_cast<hipStream_t>(stream);
#define IAFM_BWD(V) k_iafm_bwd<V><<<grid, block, 0, s>>>(E, ld_e, Wl, ld_w, Wl ? n_wl : 0, m, ld_m, mode, B, F, D, L.dl, \
                                                        L.lpr, g_lin, g_fm, gE, ld_ge, gWl, ld_gw, gZ, ld_gz)
  if (vec == 4) IAFM_BWD(4);
  else if (vec == 2) IAFM_BWD(2);
  else IAFM_BWD(1);
#undef IAFM_BWD
  return launch_status();
}
