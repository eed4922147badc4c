// ccpm.hip -- ConvLayer of CCPM (reference interaction.py:675-717: Conv2dSame / Tanh / KMaxPooling per layer) on gfx950.
//
//   layer i = 1..L on the image x [C_{i-1}][n_{i-1}][D] of one sample (C_0 = 1, n_0 = F, n_i = k_i):
//     a[co, f, d] = bias[co] + sum_ci sum_t W[co, ci, t] x[ci, f + t - top, d]     top = (w - 1) / 2, rows outside are 0
//     y = tanh(a);  per column (co, d) the k_i largest y over f, in descending order, ties to the lower f first
// The reference runs F.pad, a library convolution with a (w, 1) filter, tanh and torch.topk per layer, and autograd's
// gather / scatter through the sort on the way back.  Here ONE wave owns a sample: the taps, the current image and the
// activations live in LDS, nothing but E, out and the selection bytes touches HBM.  Selection is by rank (the number
// of rows of the column that beat this one), which needs no sort and IS the tie rule.  The backward reads the
// selection the forward wrote, recomputes only the selected activations, is free of atomics and sums the parameter
// gradients in a fixed order: per-workgroup partials in LDS summed in sample order -> one partial row per workgroup
// -> k_ccpm_reduce adds the rows in workgroup order.  Limits: see dctr.h.
#include "common.hpp"

using namespace dctr;

namespace {

constexpr int kW = 64;        // one wave per workgroup
constexpr int kMaxL = 4;
constexpr size_t kMaxLds = 64u * 1024u;   // per workgroup: two or more workgroups per CU (160 KB)

struct CcpmArgs {
  const float* E;        // [B, lde]: fields first
  int64_t lde;
  const float* params;   // layer 1 weight [C_1, C_0, w_1] | bias [C_1] | layer 2 weight | ...
  int B, F, D, L;
  int width[kMaxL], C[kMaxL + 1], n[kMaxL + 1];   // C[0] = 1, n[0] = F, n[i] = k_i
  int n_params, sel_stride, max_img, max_act;
  float* out;            // fwd: [B, ldo]
  int64_t ldo;
  uint8_t* sel_w;        // fwd: [B, sel_stride] or null
  const uint8_t* sel;    // bwd
  const float* gout;     // bwd: [B, ldgo]
  int64_t ldgo;
  float* gE;             // bwd: [B, ldge]
  int64_t ldge;
  float* part;           // bwd: [n_wg][n_params]
};

// pre-activation of (co, f, d) of a layer: x [Cin][n][D], Wl [Cout][Cin][w], in the one order both directions use
__device__ __forceinline__ float conv_at(const float* x, const float* Wl, float bias, int co, int f, int d, int Cin,
                                         int n, int D, int w) {
  const int top = (w - 1) >> 1;
  const int t0 = top - f > 0 ? top - f : 0, t1 = n + top - f < w ? n + top - f : w;
  float acc = bias;
  for (int ci = 0; ci < Cin; ++ci) {
    const float* wr = Wl + (co * Cin + ci) * w;
    const float* xr = x + (ci * n + f - top) * D + d;
    for (int t = t0; t < t1; ++t) acc = __builtin_fmaf(wr[t], xr[t * D], acc);
  }
  return acc;
}

__device__ __forceinline__ void load_row(float* dst, const float* src, int n, int lane) {
  for (int e0 = lane; e0 < n; e0 += 8 * kW) {   // unconditional loads, 8 in flight
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = ldg_f32(src + (e0 + u * kW < n ? e0 + u * kW : 0));
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (e0 + u * kW < n) dst[e0 + u * kW] = v[u];
  }
}

// LDS (floats): Ws [n_params] | x [max_img] | act [max_act]
__global__ __launch_bounds__(kW) void k_ccpm_fwd(CcpmArgs a) {
  extern __shared__ __align__(16) float smem[];
  const int D = a.D, lane = threadIdx.x;
  float* Ws = smem;
  float* x = Ws + a.n_params;
  float* act = x + a.max_img;
  for (int e = lane; e < a.n_params; e += kW) Ws[e] = ldg_f32(a.params + e);

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();
    load_row(x, a.E + static_cast<int64_t>(b) * a.lde, a.F * D, lane);
    __syncthreads();
    int poff = 0, soff = 0;
    for (int i = 1; i <= a.L; ++i) {
      const int Cin = a.C[i - 1], Cout = a.C[i], n = a.n[i - 1], k = a.n[i], w = a.width[i - 1];
      const float* Wl = Ws + poff;
      const float* bl = Wl + Cout * Cin * w;
      const int items = Cout * n * D;
      for (int e = lane; e < items; e += kW) {
        const int d = e % D, cf = e / D, f = cf % n, co = cf / n;
        act[e] = tanhf(conv_at(x, Wl, bl[co], co, f, d, Cin, n, D, w));
      }
      __syncthreads();
      // rank of row f in its column = rows that beat it (larger, or equal with a lower index); the first k are kept
      const bool last = i == a.L;
      for (int e = lane; e < items; e += kW) {
        const int d = e % D, cf = e / D, f = cf % n, co = cf / n;
        const float v = act[e];
        const float* col = act + co * n * D + d;
        int rank = 0;
        for (int g = 0; g < n; ++g) {
          const float u = col[g * D];
          rank += (u > v || (u == v && g < f)) ? 1 : 0;
        }
        if (rank < k) {
          const int o = (co * k + rank) * D + d;
          x[o] = v;
          if (last) stg_f32(a.out + static_cast<int64_t>(b) * a.ldo + o, v);
          if (a.sel_w) a.sel_w[static_cast<int64_t>(b) * a.sel_stride + soff + o] = static_cast<uint8_t>(f);
        }
      }
      __syncthreads();
      poff += Cout * Cin * w + Cout;
      soff += Cout * k * D;
    }
  }
}

// LDS (floats): Ws [n_params] | gp [n_params] | img [sum_i C_i n_i D] | g0 [max_img] | g1 [max_img] | sel (bytes)
__global__ __launch_bounds__(kW) void k_ccpm_bwd(CcpmArgs a, int img_total) {
  extern __shared__ __align__(16) float smem[];
  const int D = a.D, L = a.L, lane = threadIdx.x;
  float* Ws = smem;
  float* gp = Ws + a.n_params;
  float* img = gp + a.n_params;
  float* g0 = img + img_total;
  float* g1 = g0 + a.max_img;
  uint8_t* sl = reinterpret_cast<uint8_t*>(g1 + a.max_img);
  for (int e = lane; e < a.n_params; e += kW) {
    Ws[e] = ldg_f32(a.params + e);
    gp[e] = 0.f;
  }

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();
    load_row(img, a.E + static_cast<int64_t>(b) * a.lde, a.F * D, lane);
    {
      const uint8_t* src = a.sel + static_cast<int64_t>(b) * a.sel_stride;
      for (int e = lane; e < a.sel_stride; e += kW) sl[e] = src[e];
    }
    load_row(g0, a.gout + static_cast<int64_t>(b) * a.ldgo, a.C[L] * a.n[L] * D, lane);
    __syncthreads();
    // the pooled images of every layer, recomputed at the selected rows only
    int poff = 0, soff = 0, ioff = 0;
    for (int i = 1; i <= L; ++i) {
      const int Cin = a.C[i - 1], Cout = a.C[i], n = a.n[i - 1], k = a.n[i], w = a.width[i - 1];
      const float* Wl = Ws + poff;
      const float* bl = Wl + Cout * Cin * w;
      const float* x = img + ioff;
      float* y = img + ioff + Cin * n * D;
      const int items = Cout * k * D;
      for (int e = lane; e < items; e += kW) {
        const int d = e % D, co = e / (k * D);
        int f = sl[soff + e];
        f = f < n ? f : n - 1;
        y[e] = tanhf(conv_at(x, Wl, bl[co], co, f, d, Cin, n, D, w));
      }
      __syncthreads();
      poff += Cout * Cin * w + Cout;
      soff += items;
      ioff += Cin * n * D;
    }
    float* gy = g0;
    float* gx = g1;
    for (int i = L; i >= 1; --i) {
      const int Cin = a.C[i - 1], Cout = a.C[i], n = a.n[i - 1], k = a.n[i], w = a.width[i - 1];
      const int top = (w - 1) >> 1, nw = Cout * Cin * w, items = Cout * k * D;
      poff -= nw + Cout;
      soff -= items;
      ioff -= Cin * n * D;
      const float* Wl = Ws + poff;
      const float* x = img + ioff;
      const float* y = img + ioff + Cin * n * D;
      const uint8_t* s = sl + soff;
      for (int e = lane; e < items; e += kW) gy[e] *= 1.f - y[e] * y[e];     // through tanh
      __syncthreads();
      // weight and bias gradients: lane owns elements idx = lane + 64 * m of the layer's [nw + Cout] block
      for (int idx = lane; idx < nw + Cout; idx += kW) {
        float sum = 0.f;
        if (idx < nw) {
          const int t = idx % w, cc = idx / w, ci = cc % Cin, co = cc / Cin;
          const float* gr = gy + co * k * D;
          const uint8_t* sr = s + co * k * D;
          const float* xr = x + ci * n * D;
          for (int r = 0; r < k; ++r)
            for (int d = 0; d < D; ++d) {
              const int row = sr[r * D + d] + t - top;
              if (row >= 0 && row < n) sum = __builtin_fmaf(gr[r * D + d], xr[row * D + d], sum);
            }
        } else {
          const float* gr = gy + (idx - nw) * k * D;
          for (int e = 0; e < k * D; ++e) sum += gr[e];
        }
        gp[poff + idx] += sum;
      }
      // input gradient: element (ci, f, d) collects every pooled element whose window covers row f
      float* dst = i == 1 ? a.gE + static_cast<int64_t>(b) * a.ldge : gx;
      for (int e = lane; e < Cin * n * D; e += kW) {
        const int d = e % D, cf = e / D, f = cf % n, ci = cf / n;
        float sum = 0.f;
        for (int co = 0; co < Cout; ++co) {
          const float* wr = Wl + (co * Cin + ci) * w;
          for (int r = 0; r < k; ++r) {
            const int o = (co * k + r) * D + d;
            const int t = f - s[o] + top;
            if (t >= 0 && t < w) sum = __builtin_fmaf(gy[o], wr[t], sum);
          }
        }
        if (i == 1) stg_f32(dst + e, sum);
        else dst[e] = sum;
      }
      __syncthreads();
      float* tmp = gy;
      gy = gx;
      gx = tmp;
    }
  }
  __syncthreads();
  float* mine = a.part + static_cast<int64_t>(blockIdx.x) * a.n_params;
  for (int e = lane; e < a.n_params; e += kW) stg_f32(mine + e, gp[e]);
}

// out[i] = sum_g part[g][i] in workgroup order; thread (o, sl) adds the groups sl, sl + 16, ..., slices added in order
__global__ __launch_bounds__(256) void k_ccpm_reduce(const float* __restrict__ part, int stride, int groups,
                                                     float* __restrict__ out) {
  __shared__ float red[16][17];
  const int o = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + o;
  const int ic = i < stride ? i : 0;
  float s = 0.f;
  for (int g0 = sl; g0 < groups; g0 += 16 * 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int g = g0 + 16 * u;
      v[u] = ldg_f32(part + static_cast<int64_t>(g < groups ? g : 0) * stride + ic);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (g0 + 16 * u < groups) s += v[u];
  }
  red[sl][o] = s;
  __syncthreads();
  if (sl == 0 && i < stride) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][o];
    out[i] = t;
  }
}

int ccpm_groups(int B) { return B < 4096 ? B : 4096; }   // one wave each: about one round of the chip

// fills the shape part of the arguments; DCTR_EINVAL / DCTR_ENOSUP / DCTR_OK.  img_total = every layer's image.
int shape(CcpmArgs& a, int B, int F, int D, int L, const int32_t* width, const int32_t* filters, const int32_t* k,
          int* img_total) {
  if (B < 0 || F <= 0 || D <= 0 || L <= 0 || !width || !filters || !k) return DCTR_EINVAL;
  if (L > kMaxL || F > 64 || D > 64) return DCTR_ENOSUP;
  a.B = B; a.F = F; a.D = D; a.L = L;
  a.C[0] = 1;
  a.n[0] = F;
  a.n_params = a.sel_stride = a.max_act = 0;
  a.max_img = *img_total = F * D;
  for (int i = 1; i <= L; ++i) {
    const int w = width[i - 1], c = filters[i - 1], kk = k[i - 1];
    if (w <= 0 || c <= 0 || kk <= 0 || kk > a.n[i - 1]) return DCTR_EINVAL;
    if (w > 16 || c > 16) return DCTR_ENOSUP;
    a.width[i - 1] = w; a.C[i] = c; a.n[i] = kk;
    a.n_params += c * a.C[i - 1] * w + c;
    a.sel_stride += c * kk * D;
    const int act = c * a.n[i - 1] * D, im = c * kk * D;
    a.max_act = act > a.max_act ? act : a.max_act;
    a.max_img = im > a.max_img ? im : a.max_img;
    *img_total += im;
  }
  return DCTR_OK;
}

size_t fwd_lds(const CcpmArgs& a) { return sizeof(float) * (static_cast<size_t>(a.n_params) + a.max_img + a.max_act); }
size_t bwd_lds(const CcpmArgs& a, int img_total) {
  return sizeof(float) * (2 * static_cast<size_t>(a.n_params) + img_total + 2 * static_cast<size_t>(a.max_img)) +
         (static_cast<size_t>(a.sel_stride) + 3) / 4 * 4;
}

}  // namespace

extern "C" size_t dctr_ccpm_bwd_workspace_floats(int32_t B, int32_t n_params) {
  if (B <= 0 || n_params <= 0) return 0;
  return static_cast<size_t>(ccpm_groups(B)) * static_cast<size_t>(n_params);
}

extern "C" int dctr_ccpm_fwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t n_layers,
                             const int32_t* width, const int32_t* filters, const int32_t* k, const float* params,
                             float* out, int64_t ld_out, uint8_t* sel, dctr_stream_t stream) {
  if (B == 0) return DCTR_OK;
  CcpmArgs a = {};
  int img_total = 0;
  const int rc = shape(a, B, F, D, n_layers, width, filters, k, &img_total);
  if (rc != DCTR_OK) return rc;
  if (fwd_lds(a) > kMaxLds || bwd_lds(a, img_total) > kMaxLds) return DCTR_ENOSUP;
  if (!E || !params || !out || ld_e < static_cast<int64_t>(F) * D ||
      ld_out < static_cast<int64_t>(a.C[a.L]) * a.n[a.L] * D)
    return DCTR_EINVAL;
  a.E = E; a.lde = ld_e; a.params = params; a.out = out; a.ldo = ld_out; a.sel_w = sel;
  k_ccpm_fwd<<<dim3(ccpm_groups(B)), dim3(kW), fwd_lds(a), static_cast<hipStream_t>(stream)>>>(a);
  return launch_status();
}

extern "C" int dctr_ccpm_bwd(const float* E, int64_t ld_e, int32_t B, int32_t F, int32_t D, int32_t n_layers,
                             const int32_t* width, const int32_t* filters, const int32_t* k, const float* params,
                             const uint8_t* sel, const float* g_out, int64_t ld_gout, float* gE, int64_t ld_ge,
                             float* g_params, float* workspace, dctr_stream_t stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  CcpmArgs a = {};
  int img_total = 0;
  if (B == 0) {   // no sample: zero parameter gradients, when the shape says how many there are
    if (g_params && shape(a, B, F, D, n_layers, width, filters, k, &img_total) == DCTR_OK)
      (void)hipMemsetAsync(g_params, 0, sizeof(float) * a.n_params, s);
    return DCTR_OK;
  }
  const int rc = shape(a, B, F, D, n_layers, width, filters, k, &img_total);
  if (rc != DCTR_OK) return rc;
  if (fwd_lds(a) > kMaxLds || bwd_lds(a, img_total) > kMaxLds) return DCTR_ENOSUP;
  const int64_t n_out = static_cast<int64_t>(a.C[a.L]) * a.n[a.L] * D;
  if (!E || !params || !sel || !g_out || !gE || !g_params || !workspace || ld_e < static_cast<int64_t>(F) * D ||
      ld_gout < n_out || ld_ge < static_cast<int64_t>(F) * D)
    return DCTR_EINVAL;
  const int groups = ccpm_groups(B);
  a.E = E; a.lde = ld_e; a.params = params; a.sel = sel; a.gout = g_out; a.ldgo = ld_gout; a.gE = gE; a.ldge = ld_ge;
  a.part = workspace;
  k_ccpm_bwd<<<dim3(groups), dim3(kW), bwd_lds(a, img_total), s>>>(a, img_total);
  const int st = launch_status();
  if (st != DCTR_OK) return st;
  k_ccpm_reduce<<<dim3((a.n_params + 15) / 16), dim3(256), 0, s>>>(workspace, a.n_params, groups, g_params);
  return launch_status();
}
