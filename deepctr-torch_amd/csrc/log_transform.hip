// log_transform.hip -- LogTransformLayer of AFN (reference interaction.py:720-757) on gfx950.
//
//   a[b,e,f] = log(max(|X[b,f,e]|, 1e-7))      n = BN0_e(a) over (b, f)
//   z[b,e,h] = sum_f n[b,e,f] W[f,h] + bias[h]  y = exp(z)      out[b, e*H + h] = BN1_e(y) over (b, h)
//
// The reference makes the [B, E, H] tensor four times on the way forward and again on the way back.  Here nothing of
// that size exists but `out` (and the gradient the tower hands back): every pass that needs y RECOMPUTES it from X,
// which stays in L2, with the [32 (b) x F] x [F x 128 (h)] product of a workgroup on the fp32 MFMA (32x32x2, one 32x32
// block per wave, F padded to even with zeros in LDS).  A workgroup owns one channel e, one 128-wide slice of H and
// tiles of 32 samples, so its BN1 partial belongs to one channel.
//
//   train forward   k_lt_bn0 (partials of BN0)  ->  k_lt_fwd<false> (BN1 partials, y is not written)  ->  k_lt_fwd<true>
//   eval forward    k_lt_fwd<true> on the running statistics
//   backward        k_lt_bwd_sums (sum g, sum g*yhat per e)  ->  k_lt_bwd_main (gn partials per H slice, per-workgroup
//                   gW / gbias, sums of BN0's backward)  ->  k_lt_bwd_finish (reductions, BN0 backward, gX = gn' / X)
//
// log and exp run in double (see log_abs / exp_of).  Batch statistics are per-workgroup (count, mean, M2), each from a two-pass sum over values it holds, merged by Chan's
// formula in double in a fixed order by whoever needs them.  Every other cross-workgroup sum is a fixed-order sum of
// per-workgroup partials: no atomics, no workgroup waits on another.  Limits and LDS: see dctr.h.
#include "common.hpp"

using namespace dctr;

namespace {

constexpr int kT = 256;          // threads: 4 waves, wave w owns columns [32 w, 32 w + 32) of the slice
constexpr int kRows = 32;        // samples per tile
constexpr int kHT = 128;         // columns of H per workgroup
constexpr int kFMax = 64;
constexpr int kLdN = kFMax + 1;  // row stride of the n tile (odd: the MFMA's A read walks rows)
constexpr int kLdG = kHT + 1;
constexpr int kGxFwd = 32;       // workgroups along B of the passes that keep nothing across channels
constexpr int kGxMain = 128;     // ... of k_lt_bwd_main, which loops over the channels itself
constexpr int kNb0 = 64;         // workgroups of k_lt_bn0
constexpr int kGxFin = 512;
constexpr float kClamp = 1e-7f;
constexpr double kEps = 1e-5;

struct LtArgs {
  const float* X;        // [B, ldx]: X[b, f*E + e]
  int64_t ldx;
  int B, F, E, H;
  const float *W, *bias, *g0, *b0, *g1, *b1;
  const float *rmean0, *rvar0, *rmean1, *rvar1;   // eval: the running statistics
  const double *mean0, *var0, *mean1, *var1;      // backward: the forward's batch statistics; both null: merge the partials
  const double *part0, *part1;                // [P][E][3] (count, mean, M2)
  int P0, P1;
  double* part1_w;       // fwd<false>: [gridDim.x * gridDim.z][E][3]
  float* out;            // fwd<true>: [B, ldo]
  int64_t ldo;
  double* stats;         // fwd<true>, train: [4][E] mean0, var0, mean1, var1 (biased)
  const float* gout;     // bwd: [B, ldg]
  int64_t ldg;
  double *sums1, *sums0; // bwd: [P][E][2]
  float* gn;             // bwd: [HZ][B][E][F]
  double* gwp;           // bwd: [gx][(F + 1)][H]
  float* gX;
  int64_t ldgx;
  float *gW, *gbias, *gg0, *gb0, *gg1, *gb1;
  int Pm;                // partials of sums0 (k_lt_bwd_main's workgroups)
};

struct Moments {
  double n, mean, m2;
};

__device__ __forceinline__ Moments chan(Moments a, Moments b) {
  const double n = a.n + b.n;
  if (n <= 0.0) return a;
  const double d = b.mean - a.mean;
  Moments r;
  r.n = n;
  r.mean = a.mean + d * (b.n / n);
  r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / n);
  return r;
}

// wave 0 merges the P partials of channel e in a fixed order; every thread gets (mean, biased variance).  Two barriers.
__device__ __forceinline__ void merged_stats(const double* part, int P, int E, int e, double* sh, double& mean, double& var) {
  if (threadIdx.x < kWave) {
    Moments m = {0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < P; p += kWave) {
      const double* q = part + (static_cast<int64_t>(p) * E + e) * 3;
      Moments o = {q[0], q[1], q[2]};
      m = chan(m, o);
    }
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {   // lane l takes lane l + s: lane 0 ends with lanes 0..63 in tree order
      Moments o;
      o.n = __shfl_down(m.n, s, kWave);
      o.mean = __shfl_down(m.mean, s, kWave);
      o.m2 = __shfl_down(m.m2, s, kWave);
      m = chan(m, o);
    }
    if (threadIdx.x == 0) {
      sh[0] = m.mean;
      sh[1] = m.n > 0.0 ? m.m2 / m.n : 0.0;
    }
  }
  __syncthreads();
  mean = sh[0];
  var = sh[1];
  __syncthreads();
}

// fixed-order sum of one value per thread over the workgroup; every thread gets it.  Two barriers.
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double t = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return t;
}

// The statistics stay in double from the sums to the normalised value: what a BatchNorm's backward leaves after its
// projection is eps / (var + eps) of the terms, and a float rstd moves that by 1e-7 / (eps / (var + eps)).
__device__ __forceinline__ double rstd_of(double var) { return 1.0 / sqrt(var + kEps); }
__device__ __forceinline__ float normalised(double v, double mean, double rstd) {
  return static_cast<float>((v - mean) * rstd);
}

// log and exp in double, from float arguments.  With few samples per channel the gradients are sums that cancel to a
// hundredth of their terms and less, and a 1-ulp float difference in y = exp(z) then shows as 1e-5 of a gradient (measured
// at B 33, F 1, H 1: logf / expf 1.4e-5, these 1e-6).  The log runs over the [B, F, E] input only.  The exp is the layer's
// bulk: argument reduction by ln 2 and the degree-11 Taylor polynomial on |r| <= 0.347 (remainder 6e-15), 13 double FMAs.
__device__ __forceinline__ double log_abs(float x) { return log(static_cast<double>(fmaxf(fabsf(x), kClamp))); }
__device__ __forceinline__ double exp_of(float z) {
  const double zd = static_cast<double>(fminf(fmaxf(z, -700.f), 700.f));
  const double k = rint(zd * 1.4426950408889634);
  const double r = fma(-k, 1.9082149292705877e-10, fma(-k, 0.6931471803691238, zd));   // ln 2 = hi + lo
  double p = 1.0 / 39916800.0;
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(p, static_cast<int>(k));
}

// W[:, h0 : h0 + 128] and the bias slice into LDS, zero outside F x H
__device__ __forceinline__ void stage_w(const LtArgs& a, int h0, int Fs, float* Ws, float* bs) {
  for (int i = threadIdx.x; i < Fs * kHT; i += kT) {
    const int f = i / kHT, c = i - f * kHT;
    const bool ok = f < a.F && h0 + c < a.H;
    Ws[i] = ok ? ldg_f32(a.W + static_cast<int64_t>(f) * a.H + h0 + c) : 0.f;
  }
  if (threadIdx.x < kHT) bs[threadIdx.x] = h0 + threadIdx.x < a.H ? ldg_f32(a.bias + h0 + threadIdx.x) : 0.f;
}

// the normalised logs of samples [r0, r0 + 32) of channel e into LDS (nT; nh: before gamma / beta), zero outside B x F
template <bool HAT>
__device__ __forceinline__ void load_n(const LtArgs& a, int e, int r0, int Fs, double m0, double r0s, float gam, float bet,
                                       float* nT, float* nh) {
  for (int i = threadIdx.x; i < kRows * Fs; i += kT) {
    const int row = i / Fs, f = i - row * Fs;
    const int b = r0 + row;
    float hat = 0.f, v = 0.f;
    if (b < a.B && f < a.F) {
      hat = normalised(log_abs(ldg_f32(a.X + static_cast<int64_t>(b) * a.ldx + f * a.E + e)), m0, r0s);
      v = __builtin_fmaf(hat, gam, bet);
    }
    nT[row * kLdN + f] = v;
    if (HAT) nh[row * kLdN + f] = hat;
  }
}

// this wave's 32 x 32 block of n W: lane holds column (lane & 31), rows acc_row32(r, lane >> 5)
__device__ __forceinline__ f32x16 tile_product(const float* nT, const float* Ws, int Fs) {
  const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const float* ap = nT + l32 * kLdN + half;
  const float* bp = Ws + half * kHT + wv * 32 + l32;
  for (int k = 0; k < Fs; k += 2) acc = mfma32(ap[k], bp[k * kHT], acc);
  return acc;
}

__device__ __forceinline__ void channel_stats0(const LtArgs& a, int e, double* sh, double& m0, double& v0) {
  if (a.rmean0) {
    m0 = static_cast<double>(ldg_f32(a.rmean0 + e));
    v0 = static_cast<double>(ldg_f32(a.rvar0 + e));
  } else {
    merged_stats(a.part0, a.P0, a.E, e, sh, m0, v0);
  }
}

// ---- BN0 partials: workgroup g owns samples [g rp, (g + 1) rp); thread (e, slot) walks the (b, f) pairs of its channel ----
__global__ __launch_bounds__(kT) void k_lt_bn0(LtArgs a, int rp, double* part) {
  __shared__ double red[kT];
  __shared__ double mean_s[kFMax];
  const int E = a.E, F = a.F;
  const int e = threadIdx.x % E, slot = threadIdx.x / E, nslots = kT / E;
  const int b_lo = blockIdx.x * rp, b_hi = min(a.B, b_lo + rp);
  const int pairs = b_hi > b_lo ? (b_hi - b_lo) * F : 0;
  double s = 0.0;
  if (slot < nslots)
    for (int p = slot; p < pairs; p += nslots) {
      const int b = b_lo + p / F, f = p % F;
      s += log_abs(ldg_f32(a.X + static_cast<int64_t>(b) * a.ldx + f * E + e));
    }
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x < E) {
    double t = 0.0;
    for (int k = 0; k < nslots; ++k) t += red[k * E + threadIdx.x];
    mean_s[threadIdx.x] = pairs > 0 ? t / static_cast<double>(pairs) : 0.0;
  }
  __syncthreads();
  const double mean = mean_s[e];
  double q = 0.0;
  if (slot < nslots)
    for (int p = slot; p < pairs; p += nslots) {
      const int b = b_lo + p / F, f = p % F;
      const double d = log_abs(ldg_f32(a.X + static_cast<int64_t>(b) * a.ldx + f * E + e)) - mean;
      q += d * d;
    }
  red[threadIdx.x] = q;
  __syncthreads();
  if (threadIdx.x < E) {
    double t = 0.0;
    for (int k = 0; k < nslots; ++k) t += red[k * E + threadIdx.x];
    double* o = part + (static_cast<int64_t>(blockIdx.x) * E + threadIdx.x) * 3;
    o[0] = static_cast<double>(pairs);
    o[1] = mean_s[threadIdx.x];
    o[2] = t;
  }
}

// ---- forward: WRITE = false reduces the BN1 partial of (blockIdx.x, e, slice); WRITE = true writes out ----
template <bool WRITE>
__global__ __launch_bounds__(kT) void k_lt_fwd(LtArgs a) {
  __shared__ __align__(16) float Ws[kFMax * kHT];
  __shared__ float nT[kRows * kLdN];
  __shared__ float bs[kHT];
  __shared__ double red[4];
  const int e = blockIdx.y, hz = blockIdx.z, h0 = hz * kHT;
  const int Fs = (a.F + 1) & ~1;
  const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  double m0, v0, m1 = 0.0, v1 = 1.0;
  channel_stats0(a, e, red, m0, v0);
  if (WRITE) {
    if (a.rmean1) {
      m1 = static_cast<double>(ldg_f32(a.rmean1 + e));
      v1 = static_cast<double>(ldg_f32(a.rvar1 + e));
    } else {
      merged_stats(a.part1, a.P1, a.E, e, red, m1, v1);
    }
    if (a.stats && blockIdx.x == 0 && hz == 0 && threadIdx.x == 0) {
      a.stats[e] = m0;
      a.stats[a.E + e] = v0;
      a.stats[2 * a.E + e] = m1;
      a.stats[3 * a.E + e] = v1;
    }
  }
  const double r0s = rstd_of(v0), r1s = rstd_of(v1);
  const float gam0 = ldg_f32(a.g0 + e), bet0 = ldg_f32(a.b0 + e);
  const float gam1 = WRITE ? ldg_f32(a.g1 + e) : 0.f, bet1 = WRITE ? ldg_f32(a.b1 + e) : 0.f;
  stage_w(a, h0, Fs, Ws, bs);
  const int col = wv * 32 + l32, h = h0 + col;
  const bool colok = h < a.H;
  const int cols_valid = min(kHT, a.H - h0);
  const int tiles = (a.B + kRows - 1) / kRows;
  Moments run = {0.0, 0.0, 0.0};
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r0 = t * kRows;
    __syncthreads();
    load_n<false>(a, e, r0, Fs, m0, r0s, gam0, bet0, nT, nullptr);
    __syncthreads();
    const f32x16 acc = tile_product(nT, Ws, Fs);
    const float bv = bs[col];
    double y[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] = exp_of(acc[r] + bv);
    if (WRITE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = r0 + acc_row32(r, half);
        if (colok && b < a.B)
          stg_f32(a.out + static_cast<int64_t>(b) * a.ldo + static_cast<int64_t>(e) * a.H + h, __builtin_fmaf(normalised(y[r], m1, r1s), gam1, bet1));
      }
    } else {
      // (double: a gradient downstream can hang on var1 to more digits than a float sum keeps -- few samples, H = 1)
      const double cnt = static_cast<double>(min(kRows, a.B - r0)) * static_cast<double>(cols_valid);
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += (colok && r0 + acc_row32(r, half) < a.B) ? y[r] : 0.0;
      const double mt = block_sum(s, red) / cnt;
      double q = 0.0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const double d = (colok && r0 + acc_row32(r, half) < a.B) ? y[r] - mt : 0.0;
        q += d * d;
      }
      const double m2 = block_sum(q, red);
      Moments o = {cnt, mt, m2};
      run = chan(run, o);
    }
  }
  if (!WRITE && threadIdx.x == 0) {
    double* o = a.part1_w + ((static_cast<int64_t>(blockIdx.x) * gridDim.z + hz) * a.E + e) * 3;
    o[0] = run.n;
    o[1] = run.mean;
    o[2] = run.m2;
  }
}

// ---- backward 1: sum g and sum g * yhat of (blockIdx.x, e, slice) ----
__global__ __launch_bounds__(kT) void k_lt_bwd_sums(LtArgs a) {
  __shared__ __align__(16) float Ws[kFMax * kHT];
  __shared__ float nT[kRows * kLdN];
  __shared__ float bs[kHT];
  __shared__ double red[4];
  const int e = blockIdx.y, hz = blockIdx.z, h0 = hz * kHT;
  const int Fs = (a.F + 1) & ~1;
  const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  const double m0 = a.mean0[e], r0s = rstd_of(a.var0[e]);
  const double m1 = a.mean1[e], r1s = rstd_of(a.var1[e]);
  const float gam0 = ldg_f32(a.g0 + e), bet0 = ldg_f32(a.b0 + e);
  stage_w(a, h0, Fs, Ws, bs);
  const int col = wv * 32 + l32, h = h0 + col;
  const bool colok = h < a.H;
  const int tiles = (a.B + kRows - 1) / kRows;
  double sg = 0.0, sgy = 0.0;
  for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int r0 = t * kRows;
    __syncthreads();
    load_n<false>(a, e, r0, Fs, m0, r0s, gam0, bet0, nT, nullptr);
    __syncthreads();
    const f32x16 acc = tile_product(nT, Ws, Fs);
    const float bv = bs[col];
    float g[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int b = r0 + acc_row32(r, half);
      const bool ok = colok && b < a.B;
      g[r] = ldg_f32(a.gout + (ok ? static_cast<int64_t>(b) * a.ldg + static_cast<int64_t>(e) * a.H + h : 0));
      if (!ok) g[r] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const double yh = (exp_of(acc[r] + bv) - m1) * r1s;
      sg += static_cast<double>(g[r]);
      sgy += static_cast<double>(g[r]) * yh;
    }
  }
  sg = block_sum(sg, red);
  sgy = block_sum(sgy, red);
  if (threadIdx.x == 0) {
    double* o = a.sums1 + ((static_cast<int64_t>(blockIdx.x) * gridDim.z + hz) * a.E + e) * 2;
    o[0] = sg;
    o[1] = sgy;
  }
}

// wave 0: fixed-order sums of the P two-value partials of channel e -> sh[0], sh[1] (no barrier).  These are the
// projection coefficients of a BatchNorm's backward: kept in double up to the subtraction they feed, because what is
// left after it can be a small fraction of the terms (var close to eps).
__device__ __forceinline__ void merged_sums(const double* part, int P, int E, int e, double* sh) {
  if (threadIdx.x < kWave) {
    double s0 = 0.0, s1 = 0.0;
    for (int p = threadIdx.x; p < P; p += kWave) {
      const double* q = part + (static_cast<int64_t>(p) * E + e) * 2;
      s0 += q[0];
      s1 += q[1];
    }
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
      s0 += __shfl_down(s0, s, kWave);
      s1 += __shfl_down(s1, s, kWave);
    }
    if (threadIdx.x == 0) {
      sh[0] = s0;
      sh[1] = s1;
    }
  }
}

// ---- backward 2: workgroup (x, slice) walks every channel: gz, its three products, BN0's sums ----
__global__ __launch_bounds__(kT) void k_lt_bwd_main(LtArgs a, int P1) {
  __shared__ __align__(16) float Ws[kFMax * kHT];
  __shared__ float nT[kRows * kLdN];
  __shared__ float nh[kRows * kLdN];
  __shared__ float gz[kRows * kLdG];
  __shared__ float bs[kHT];
  __shared__ double red[4];
  const int hz = blockIdx.y, h0 = hz * kHT;
  const int F = a.F, Fs = (F + 1) & ~1;
  const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5, wv = threadIdx.x >> 6;
  stage_w(a, h0, Fs, Ws, bs);
  const int col = wv * 32 + l32, h = h0 + col;
  const bool colok = h < a.H;
  const int tiles = (a.B + kRows - 1) / kRows;
  const double inv_n1 = 1.0 / (static_cast<double>(a.B) * static_cast<double>(a.H));
  const int wc = threadIdx.x & (kHT - 1), wf = threadIdx.x >> 7;     // gW: column wc, fields wf, wf + 2, ...
  const int nrow = threadIdx.x & 31, nf = threadIdx.x >> 5;          // gn: row nrow, fields nf, nf + 8, ...
  // (double: with few samples and a small variance these sums cancel to a hundredth of their terms and less)
  double accw[kFMax / 2];
#pragma unroll
  for (int j = 0; j < kFMax / 2; ++j) accw[j] = 0.0;
  double accb = 0.0;
  for (int e = 0; e < a.E; ++e) {
    __syncthreads();
    merged_sums(a.sums1, P1, a.E, e, red);
    __syncthreads();
    const double c1 = red[0] * inv_n1, c2 = red[1] * inv_n1;
    __syncthreads();
    const double m0 = a.mean0[e], r0s = rstd_of(a.var0[e]);
    const double m1 = a.mean1[e], r1s = rstd_of(a.var1[e]);
    const float gam0 = ldg_f32(a.g0 + e), bet0 = ldg_f32(a.b0 + e);
    const double k1 = static_cast<double>(ldg_f32(a.g1 + e)) * r1s;
    double s1 = 0.0, s2 = 0.0;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
      const int r0 = t * kRows;
      __syncthreads();
      load_n<true>(a, e, r0, Fs, m0, r0s, gam0, bet0, nT, nh);
      __syncthreads();
      const f32x16 acc = tile_product(nT, Ws, Fs);
      const float bv = bs[col];
      float g[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int b = r0 + acc_row32(r, half);
        const bool ok = colok && b < a.B;
        g[r] = ldg_f32(a.gout + (ok ? static_cast<int64_t>(b) * a.ldg + static_cast<int64_t>(e) * a.H + h : 0));
        if (!ok) g[r] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = acc_row32(r, half);
        const bool ok = colok && r0 + row < a.B;
        const double y = exp_of(acc[r] + bv);
        const double yh = (y - m1) * r1s;
        gz[row * kLdG + col] = ok ? static_cast<float>(k1 * (static_cast<double>(g[r]) - c1 - yh * c2) * y) : 0.f;
      }
      __syncthreads();
      if (threadIdx.x < kHT) {
        double s = 0.0;
        for (int row = 0; row < kRows; ++row) s += static_cast<double>(gz[row * kLdG + threadIdx.x]);
        accb += s;
      }
      {
        const int nj = (F - wf + 1) >> 1;   // fields wf + 2 j < F
        for (int row = 0; row < kRows; ++row) {
          const double gv = static_cast<double>(gz[row * kLdG + wc]);
          const float* nr = nT + row * kLdN + wf;
#pragma unroll
          for (int j = 0; j < kFMax / 2; ++j)
            if (j < nj) accw[j] += static_cast<double>(nr[2 * j]) * gv;
        }
      }
      for (int f = nf; f < F; f += 8) {
        const float* gr = gz + nrow * kLdG;
        const float* wr = Ws + f * kHT;
        float v = 0.f;
        for (int c = 0; c < kHT; ++c) v = __builtin_fmaf(gr[c], wr[c], v);
        const int b = r0 + nrow;
        if (b < a.B) {
          stg_f32(a.gn + ((static_cast<int64_t>(hz) * a.B + b) * a.E + e) * F + f, v);
          s1 += static_cast<double>(v);
          s2 += static_cast<double>(v) * static_cast<double>(nh[nrow * kLdN + f]);
        }
      }
    }
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
      double* o = a.sums0 + ((static_cast<int64_t>(blockIdx.x) * gridDim.y + hz) * a.E + e) * 2;
      o[0] = s1;
      o[1] = s2;
    }
  }
  double* mine = a.gwp + static_cast<int64_t>(blockIdx.x) * (F + 1) * a.H;
  if (h0 + wc < a.H) {
#pragma unroll
    for (int j = 0; j < kFMax / 2; ++j)
      if (wf + 2 * j < F) mine[static_cast<int64_t>(wf + 2 * j) * a.H + h0 + wc] = accw[j];
    if (threadIdx.x < kHT) mine[static_cast<int64_t>(F) * a.H + h0 + wc] = accb;
  }
}

// ---- backward 3: blocks [0, n_el): BN0 backward and gX (block 0 also the BatchNorm gradients); the rest: gW, gbias ----
__global__ __launch_bounds__(kT) void k_lt_bwd_finish(LtArgs a, int n_el, int P1, int HZ, int gx_main) {
  __shared__ double s1s[kFMax], s2s[kFMax];
  __shared__ double red[4];
  const int E = a.E, F = a.F;
  if (static_cast<int>(blockIdx.x) >= n_el) {
    const int i = (blockIdx.x - n_el) * kT + threadIdx.x;
    const int n = (F + 1) * a.H;
    if (i >= n) return;
    double s = 0.0;
    for (int p = 0; p < gx_main; ++p) s += a.gwp[static_cast<int64_t>(p) * n + i];
    if (i < F * a.H) stg_f32(a.gW + i, static_cast<float>(s));
    else stg_f32(a.gbias + (i - F * a.H), static_cast<float>(s));
    return;
  }
  for (int e = 0; e < E; ++e) {
    merged_sums(a.sums0, a.Pm, E, e, red);
    __syncthreads();
    if (threadIdx.x == 0) {
      s1s[e] = red[0];
      s2s[e] = red[1];
      if (blockIdx.x == 0) {
        stg_f32(a.gb0 + e, static_cast<float>(red[0]));
        stg_f32(a.gg0 + e, static_cast<float>(red[1]));
      }
    }
    __syncthreads();
    if (blockIdx.x == 0) {
      merged_sums(a.sums1, P1, E, e, red);
      __syncthreads();
      if (threadIdx.x == 0) {
        stg_f32(a.gb1 + e, static_cast<float>(red[0]));
        stg_f32(a.gg1 + e, static_cast<float>(red[1]));
      }
      __syncthreads();
    }
  }
  const double inv_n0 = 1.0 / (static_cast<double>(a.B) * static_cast<double>(F));
  const int64_t per = static_cast<int64_t>(E) * F, total = per * a.B;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * kT + threadIdx.x; i < total; i += static_cast<int64_t>(n_el) * kT) {
    const int64_t b = i / per;
    const int rem = static_cast<int>(i - b * per), e = rem / F, f = rem - e * F;
    float gn = 0.f;
    for (int z = 0; z < HZ; ++z) gn += ldg_f32(a.gn + static_cast<int64_t>(z) * total + i);
    const float x = ldg_f32(a.X + b * a.ldx + f * E + e);
    const double r0s = rstd_of(a.var0[e]);
    const double hat = (log_abs(x) - a.mean0[e]) * r0s;
    const float ga = static_cast<float>(static_cast<double>(ldg_f32(a.g0 + e)) * r0s *
                                        (static_cast<double>(gn) - s1s[e] * inv_n0 - hat * (s2s[e] * inv_n0)));
    stg_f32(a.gX + b * a.ldgx + f * E + e, fabsf(x) >= kClamp ? ga / x : 0.f);
  }
}

int tiles_of(int B) { return (B + kRows - 1) / kRows; }
int gx_fwd(int B) { return tiles_of(B) < kGxFwd ? tiles_of(B) : kGxFwd; }
int gx_main(int B) { return tiles_of(B) < kGxMain ? tiles_of(B) : kGxMain; }
int slices(int H) { return (H + kHT - 1) / kHT; }
int nb0(int B) { return B < kNb0 ? B : kNb0; }

int envelope(int B, int F, int E, int H) {
  if (B < 0 || F <= 0 || E <= 0 || H <= 0) return DCTR_EINVAL;
  if (F > kFMax || E > 64 || H > 1024) return DCTR_ENOSUP;
  return DCTR_OK;
}

// (the statistics' partials and the backward's sums are doubles: two floats each, at the head of the workspace)
size_t fwd_floats(int B, int E, int H) {
  return 2 * 3 * static_cast<size_t>(E) * (static_cast<size_t>(nb0(B)) + static_cast<size_t>(gx_fwd(B)) * slices(H));
}
// sums1 | sums0 | gwp (doubles) | gn
size_t bwd_sums1(int B, int E, int H) { return 2 * 2 * static_cast<size_t>(E) * gx_fwd(B) * slices(H); }
size_t bwd_sums0(int B, int E, int H) { return 2 * 2 * static_cast<size_t>(E) * gx_main(B) * slices(H); }
size_t bwd_gn(int B, int F, int E, int H) { return static_cast<size_t>(slices(H)) * B * E * F; }
size_t bwd_gwp(int B, int F, int H) { return 2 * static_cast<size_t>(gx_main(B)) * (F + 1) * H; }

void fill(LtArgs& a, const float* X, int64_t ld_e, int B, int F, int E, int H, const float* W, const float* bias,
          const float* g0, const float* b0, const float* g1, const float* b1) {
  a.X = X; a.ldx = ld_e; a.B = B; a.F = F; a.E = E; a.H = H;
  a.W = W; a.bias = bias; a.g0 = g0; a.b0 = b0; a.g1 = g1; a.b1 = b1;
}

}  // namespace

extern "C" size_t dctr_log_transform_workspace_floats(int32_t B, int32_t F, int32_t E, int32_t H) {
  if (B <= 0 || envelope(B, F, E, H) != DCTR_OK) return 0;
  const size_t f = fwd_floats(B, E, H);
  const size_t b = bwd_sums1(B, E, H) + bwd_sums0(B, E, H) + bwd_gn(B, F, E, H) + bwd_gwp(B, F, H);
  return f > b ? f : b;
}

extern "C" int dctr_log_transform_fwd_train(const float* X, int64_t ld_e, int32_t B, int32_t F, int32_t E, int32_t H,
                                            const float* W, const float* bias, const float* bn0_w, const float* bn0_b,
                                            const float* bn1_w, const float* bn1_b, float* out, int64_t ld_out,
                                            double* stats, float* workspace, dctr_stream_t stream) {
  const int rc = envelope(B, F, E, H);
  if (rc != DCTR_OK) return rc;
  if (B == 0) return DCTR_OK;
  if (!X || !W || !bias || !bn0_w || !bn0_b || !bn1_w || !bn1_b || !out || !stats || !workspace ||
      ld_e < static_cast<int64_t>(F) * E || ld_out < static_cast<int64_t>(E) * H)
    return DCTR_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 8) return DCTR_EALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  LtArgs a = {};
  fill(a, X, ld_e, B, F, E, H, W, bias, bn0_w, bn0_b, bn1_w, bn1_b);
  const int n0 = nb0(B), gx = gx_fwd(B), hz = slices(H);
  double* part0 = reinterpret_cast<double*>(workspace);
  double* part1 = part0 + 3 * static_cast<size_t>(E) * n0;
  k_lt_bn0<<<dim3(n0), dim3(kT), 0, s>>>(a, (B + n0 - 1) / n0, part0);
  int st = launch_status();
  if (st != DCTR_OK) return st;
  a.part0 = part0; a.P0 = n0; a.part1_w = part1;
  k_lt_fwd<false><<<dim3(gx, E, hz), dim3(kT), 0, s>>>(a);
  st = launch_status();
  if (st != DCTR_OK) return st;
  a.part1 = part1; a.P1 = gx * hz; a.out = out; a.ldo = ld_out; a.stats = stats;
  k_lt_fwd<true><<<dim3(gx, E, hz), dim3(kT), 0, s>>>(a);
  return launch_status();
}

extern "C" int dctr_log_transform_fwd_eval(const float* X, int64_t ld_e, int32_t B, int32_t F, int32_t E, int32_t H,
                                           const float* W, const float* bias, const float* bn0_w, const float* bn0_b,
                                           const float* bn0_mean, const float* bn0_var, const float* bn1_w,
                                           const float* bn1_b, const float* bn1_mean, const float* bn1_var, float* out,
                                           int64_t ld_out, dctr_stream_t stream) {
  const int rc = envelope(B, F, E, H);
  if (rc != DCTR_OK) return rc;
  if (B == 0) return DCTR_OK;
  if (!X || !W || !bias || !bn0_w || !bn0_b || !bn0_mean || !bn0_var || !bn1_w || !bn1_b || !bn1_mean || !bn1_var ||
      !out || ld_e < static_cast<int64_t>(F) * E || ld_out < static_cast<int64_t>(E) * H)
    return DCTR_EINVAL;
  LtArgs a = {};
  fill(a, X, ld_e, B, F, E, H, W, bias, bn0_w, bn0_b, bn1_w, bn1_b);
  a.rmean0 = bn0_mean; a.rvar0 = bn0_var; a.rmean1 = bn1_mean; a.rvar1 = bn1_var; a.out = out; a.ldo = ld_out;
  k_lt_fwd<true><<<dim3(gx_fwd(B), E, slices(H)), dim3(kT), 0, static_cast<hipStream_t>(stream)>>>(a);
  return launch_status();
}

extern "C" int dctr_log_transform_bwd(const float* X, int64_t ld_e, int32_t B, int32_t F, int32_t E, int32_t H,
                                      const float* W, const float* bias, const float* bn0_w, const float* bn0_b,
                                      const float* bn1_w, const double* stats, const float* g_out, int64_t ld_g, float* gX,
                                      int64_t ld_gx, float* gW, float* gbias, float* g_bn0_w, float* g_bn0_b,
                                      float* g_bn1_w, float* g_bn1_b, float* workspace, dctr_stream_t stream) {
  const int rc = envelope(B, F, E, H);
  if (rc != DCTR_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (B == 0) {
    if (gW) (void)hipMemsetAsync(gW, 0, sizeof(float) * F * H, s);
    if (gbias) (void)hipMemsetAsync(gbias, 0, sizeof(float) * H, s);
    float* v[4] = {g_bn0_w, g_bn0_b, g_bn1_w, g_bn1_b};
    for (float* p : v)
      if (p) (void)hipMemsetAsync(p, 0, sizeof(float) * E, s);
    return DCTR_OK;
  }
  if (!X || !W || !bias || !bn0_w || !bn0_b || !bn1_w || !stats || !g_out || !gX || !gW || !gbias || !g_bn0_w ||
      !g_bn0_b || !g_bn1_w || !g_bn1_b || !workspace || ld_e < static_cast<int64_t>(F) * E ||
      ld_g < static_cast<int64_t>(E) * H || ld_gx < static_cast<int64_t>(F) * E)
    return DCTR_EINVAL;
  if (reinterpret_cast<uintptr_t>(workspace) % 8) return DCTR_EALIGN;
  LtArgs a = {};
  fill(a, X, ld_e, B, F, E, H, W, bias, bn0_w, bn0_b, bn1_w, nullptr);
  a.mean0 = stats; a.var0 = stats + E; a.mean1 = stats + 2 * E; a.var1 = stats + 3 * E;
  a.gout = g_out; a.ldg = ld_g; a.gX = gX; a.ldgx = ld_gx;
  a.gW = gW; a.gbias = gbias; a.gg0 = g_bn0_w; a.gb0 = g_bn0_b; a.gg1 = g_bn1_w; a.gb1 = g_bn1_b;
  const int gx = gx_fwd(B), gm = gx_main(B), hz = slices(H);
  a.sums1 = reinterpret_cast<double*>(workspace);
  a.sums0 = reinterpret_cast<double*>(workspace + bwd_sums1(B, E, H));
  a.gwp = reinterpret_cast<double*>(workspace + bwd_sums1(B, E, H) + bwd_sums0(B, E, H));
  a.gn = workspace + bwd_sums1(B, E, H) + bwd_sums0(B, E, H) + bwd_gwp(B, F, H);
  a.Pm = gm * hz;
  k_lt_bwd_sums<<<dim3(gx, E, hz), dim3(kT), 0, s>>>(a);
  int st = launch_status();
  if (st != DCTR_OK) return st;
  k_lt_bwd_main<<<dim3(gm, hz), dim3(kT), 0, s>>>(a, gx * hz);
  st = launch_status();
  if (st != DCTR_OK) return st;
  const int64_t elems = static_cast<int64_t>(B) * E * F;
  const int n_el = static_cast<int>(elems / kT + 1 < kGxFin ? elems / kT + 1 : kGxFin);
  const int n_red = ((F + 1) * H + kT - 1) / kT;
  k_lt_bwd_finish<<<dim3(n_el + n_red), dim3(kT), 0, s>>>(a, n_el, gx * hz, hz, gm);
  return launch_status();
}
