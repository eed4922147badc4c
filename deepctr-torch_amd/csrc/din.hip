// din.hip -- AttentionSequencePoolingLayer of DIN / DIEN (reference layers/sequence.py:80-154 over
// layers/core.py:10-64) on gfx950: the local activation unit on [q, k, q-k, q*k], the mask, the optional softmax and
// the weighted sum of the keys, ONE launch per direction.
//
//   x(t)   = [q, k_t, q - k_t, q * k_t]                         (4E wide, never materialised: built from q and k_t)
//   a_0    = x;  a_l = act(W_l a_{l-1} + b_l)  l = 1..L;  s_t = dense.w . a_L + dense.b
//   w_t    = s_t on valid positions, 0 elsewhere                                  (no weight normalisation)
//          = softmax over the valid positions; 1/T everywhere when none is valid  (weight normalisation)
//   out    = sum_t w_t k_t
//
// A workgroup of 256 threads grid-strides over samples.  Only a sample's VALID positions are evaluated (every position is
// independent under an element-wise activation), kRowsF / kRowsB of them at a time: their keys and every layer's
// activations live in LDS, the weights are read through L1 / L2 (they are the same ~40 KB for every workgroup), and
// nothing of size B*T*4E or B*T*H touches HBM.  A thread owns (row, 4 consecutive units) of a layer: lanes run over the
// rows, so the weight reads of a wave fall on a handful of addresses and the LDS reads are conflict free (odd row stride).
//
// The backward recomputes the activations from Q, K and the parameters, reads the [B, T] weights the forward saved, is
// free of atomics and sums the parameter gradients in a fixed order: a thread owns an element of a layer's block and adds
// row chunk after row chunk, sample after sample into ITS slot of the workgroup's partial row; k_din_reduce adds the rows
// in workgroup order.  Limits and the packed parameter layout: see dctr.h.
#include "common.hpp"

using namespace dctr;

namespace {

constexpr int kT = 256;
constexpr int kMaxL = 3, kMaxSeg = 4, kMaxE = 64, kMaxT = 128, kMaxH = 128;
constexpr int kRowsF = 32, kRowsB = 16;     // valid positions per pass: forward / backward
constexpr int kGroupsF = 2048, kGroupsB = 512;
enum { ACT_LINEAR = 0, ACT_RELU = 1, ACT_SIGMOID = 2, ACT_PRELU = 3, ACT_DICE = 4 };

struct DinArgs {
  const float* Q;
  const float* K;
  int64_t ldq, ldk;
  int B, T, E, L, act, softmax, nseg;
  int dim[kMaxSeg];
  int64_t qoff[kMaxSeg], koff[kMaxSeg], kstep[kMaxSeg];
  int H[kMaxL], poff[kMaxL];      // units and offset of W_l in the packed vector (b_l, then the activation's own, follow)
  int pdense, n_params, sumH, maxH;
  const int32_t* len;
  const uint8_t* mask;
  const float* params;
  float* out;                     // fwd
  int64_t ldo;
  float* wts_w;                   // fwd: [B, T] or null
  const float* wts;               // bwd
  const float* gout;
  int64_t ldgo;
  float* gQ;
  int64_t ldgq;
  float* gK;
  int64_t ldgk;
  float* part;                    // bwd: [groups][n_params]
};

// (constant indices only: a runtime index into an array of the by-value arguments would put the array into scratch)
template <typename V>
__device__ __forceinline__ V pick3(const V (&v)[3], int l) { return l == 0 ? v[0] : l == 1 ? v[1] : v[2]; }
template <typename V>
__device__ __forceinline__ V pick4(const V (&v)[4], int g) { return g == 0 ? v[0] : g == 1 ? v[1] : g == 2 ? v[2] : v[3]; }

// ap = the activation's own parameters of the layer (prelu: slope; dice: alpha [H] | s [H] | t [H])
__device__ __forceinline__ float act_fwd(int act, float z, const float* ap, int h, int H) {
  switch (act) {
    case ACT_RELU: return z > 0.f ? z : 0.f;
    case ACT_SIGMOID: return 1.f / (1.f + expf(-z));
    case ACT_PRELU: return z > 0.f ? z : ldg_f32(ap) * z;
    case ACT_DICE: {
      const float al = ldg_f32(ap + h), p = 1.f / (1.f + expf(-(ldg_f32(ap + H + h) * z + ldg_f32(ap + 2 * H + h))));
      return z * (al + (1.f - al) * p);
    }
    default: return z;
  }
}
// d act / d z from the stored value v (the activation itself; z under prelu)
__device__ __forceinline__ float act_grad(int act, float v, float slope) {
  switch (act) {
    case ACT_RELU: return v > 0.f ? 1.f : 0.f;
    case ACT_SIGMOID: return v * (1.f - v);
    case ACT_PRELU: return v > 0.f ? 1.f : slope;
    default: return 1.f;
  }
}

// LDS carve-up shared by both kernels (the host mirrors it in base_floats)
struct Lds {
  long long* qaddr;   // [E] offset of element j inside a query row
  long long* kaddr;   // [E] offset of element j of position 0 inside a key row
  long long* kstp;    // [E] floats between two positions of element j
  float* q;           // [E]
  float* wbuf;        // [T] weights
  float* sc;          // [T] scores (fwd) / g . k_t (bwd)
  int* idx;           // [T] the valid positions, ascending
  int* n;             // [1]
  float* kb;          // [R][E + 1]
  float* a[kMaxL];    // [R][H_l + 1]
  float* rest;
};

__device__ __forceinline__ Lds carve(float* smem, const DinArgs& a, int R) {
  Lds s;
  s.qaddr = reinterpret_cast<long long*>(smem);
  s.kaddr = s.qaddr + a.E;
  s.kstp = s.kaddr + a.E;
  float* p = reinterpret_cast<float*>(s.kstp + a.E);
  s.q = p; p += a.E;
  s.wbuf = p; p += a.T;
  s.sc = p; p += a.T;
  s.idx = reinterpret_cast<int*>(p); p += a.T;
  s.n = reinterpret_cast<int*>(p); p += 1;
  s.kb = p; p += R * (a.E + 1);
#pragma unroll
  for (int l = 0; l < kMaxL; ++l) {
    s.a[l] = p;
    if (l < a.L) p += R * (a.H[l] + 1);
  }
  s.rest = p;
  return s;
}

__device__ __forceinline__ void fill_tables(const Lds& s, const DinArgs& a) {
  for (int j = threadIdx.x; j < a.E; j += kT) {
    int g = 0, o = j;
#pragma unroll
    for (int u = 0; u < kMaxSeg - 1; ++u)
      if (g == u && u < a.nseg - 1 && o >= a.dim[u]) {
        o -= a.dim[u];
        g = u + 1;
      }
    s.qaddr[j] = pick4(a.qoff, g) + o;
    s.kaddr[j] = pick4(a.koff, g) + o;
    s.kstp[j] = pick4(a.kstep, g);
  }
}

// the sample's valid positions (ascending) and the query; ends with a barrier
__device__ __forceinline__ void begin_sample(const Lds& s, const DinArgs& a, int b) {
  const int tid = threadIdx.x;
  if (a.len) {            // the first n positions: the list is the identity, every thread writes its share
    const int v = ldg_i32(a.len + b);
    const int n = v < 0 ? 0 : (v > a.T ? a.T : v);
    for (int t = tid; t < n; t += kT) s.idx[t] = t;
    if (tid == 0) *s.n = n;
  } else if (tid < kWave) {   // wave 0 compacts the mask, 64 positions per ballot
    const uint8_t* m = a.mask + static_cast<int64_t>(b) * a.T;
    int n = 0;
    for (int t0 = 0; t0 < a.T; t0 += kWave) {
      const int t = t0 + tid;
      const bool on = t < a.T && m[t] != 0;
      const unsigned long long bits = __ballot(on);
      if (on) s.idx[n + __popcll(bits & ((1ull << tid) - 1ull))] = t;
      n += __popcll(bits);
    }
    if (tid == 0) *s.n = n;
  }
  for (int j = tid; j < a.E; j += kT) s.q[j] = ldg_f32(a.Q + static_cast<int64_t>(b) * a.ldq + s.qaddr[j]);
  __syncthreads();
}

__device__ __forceinline__ void load_keys(const Lds& s, const DinArgs& a, int b, int c0, int nr) {
  const float* Kb = a.K + static_cast<int64_t>(b) * a.ldk;
  const int E = a.E;
  for (int e = threadIdx.x; e < nr * E; e += kT) {
    const int r = e / E, j = e - r * E;
    s.kb[r * (E + 1) + j] = ldg_f32(Kb + s.kaddr[j] + s.idx[c0 + r] * s.kstp[j]);
  }
}

// layer 1 on [q, k, q - k, q * k]: thread = (row, 4 units); ZMODE stores the pre-activation (prelu in the backward)
template <bool ZMODE>
__device__ __forceinline__ void layer_first(const Lds& s, const DinArgs& a, int nr) {
  const int E = a.E, H = a.H[0], IN = 4 * E, HB = (H + 3) >> 2;
  const float* W = a.params + a.poff[0];
  const float* bias = W + H * IN;
  const float* ap = bias + H;
  for (int e = threadIdx.x; e < nr * HB; e += kT) {
    const int hb = e / nr, r = e - hb * nr, h0 = hb * 4;
    const float* kr = s.kb + r * (E + 1);
    const float* w[4];
    float acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w[u] = W + (h0 + u < H ? h0 + u : H - 1) * IN;
      acc[u] = 0.f;
    }
    for (int j = 0; j < E; ++j) {
      const float qj = s.q[j], kj = kr[j], d = qj - kj, p = qj * kj;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = __builtin_fmaf(qj, ldg_f32(w[u] + j), acc[u]);
        acc[u] = __builtin_fmaf(kj, ldg_f32(w[u] + E + j), acc[u]);
        acc[u] = __builtin_fmaf(d, ldg_f32(w[u] + 2 * E + j), acc[u]);
        acc[u] = __builtin_fmaf(p, ldg_f32(w[u] + 3 * E + j), acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (h0 + u < H) {
        const float z = acc[u] + ldg_f32(bias + h0 + u);
        s.a[0][r * (H + 1) + h0 + u] = ZMODE ? z : act_fwd(a.act, z, ap, h0 + u, H);
      }
  }
}

// layer l + 1 (l >= 1) on the rows of a[l - 1]
template <bool ZMODE>
__device__ __forceinline__ void layer_next(const Lds& s, const DinArgs& a, int l, int nr) {
  const int IN = pick3(a.H, l - 1), H = pick3(a.H, l), HB = (H + 3) >> 2;
  const float* W = a.params + pick3(a.poff, l);
  const float* bias = W + H * IN;
  const float* ap = bias + H;
  const float slope_in = ZMODE ? ldg_f32(a.params + pick3(a.poff, l) - 1) : 0.f;     // (prelu: the last float of the block before)
  const float* x = pick3(s.a, l - 1);
  for (int e = threadIdx.x; e < nr * HB; e += kT) {
    const int hb = e / nr, r = e - hb * nr, h0 = hb * 4;
    const float* xr = x + r * (IN + 1);
    const float* w[4];
    float acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w[u] = W + (h0 + u < H ? h0 + u : H - 1) * IN;
      acc[u] = 0.f;
    }
    for (int i = 0; i < IN; ++i) {
      float xi = xr[i];
      if (ZMODE) xi = xi > 0.f ? xi : slope_in * xi;
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_fmaf(xi, ldg_f32(w[u] + i), acc[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (h0 + u < H) {
        const float z = acc[u] + ldg_f32(bias + h0 + u);
        pick3(s.a, l)[r * (H + 1) + h0 + u] = ZMODE ? z : act_fwd(a.act, z, ap, h0 + u, H);
      }
  }
}

template <bool ZMODE>
__device__ __forceinline__ void layers(const Lds& s, const DinArgs& a, int nr) {
  layer_first<ZMODE>(s, a, nr);
  __syncthreads();
  for (int l = 1; l < a.L; ++l) {
    layer_next<ZMODE>(s, a, l, nr);
    __syncthreads();
  }
}

// LDS: carve(kRowsF) | red [4][E]
__global__ __launch_bounds__(kT) void k_din_fwd(DinArgs a) {
  extern __shared__ __align__(16) float smem[];
  const Lds s = carve(smem, a, kRowsF);
  float* red = s.rest;
  const int tid = threadIdx.x, E = a.E, T = a.T, L = a.L;
  fill_tables(s, a);
  const int HL = pick3(a.H, L - 1);
  const float* wd = a.params + a.pdense;

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();
    begin_sample(s, a, b);
    const int n = *s.n;
    for (int c0 = 0; c0 < n; c0 += kRowsF) {
      const int nr = n - c0 < kRowsF ? n - c0 : kRowsF;
      load_keys(s, a, b, c0, nr);
      __syncthreads();
      layers<false>(s, a, nr);
      if (tid < nr) {
        const float* ar = pick3(s.a, L - 1) + tid * (HL + 1);
        float acc = 0.f;
        for (int h = 0; h < HL; ++h) acc = __builtin_fmaf(ar[h], ldg_f32(wd + h), acc);
        s.sc[c0 + tid] = acc + ldg_f32(wd + HL);     // (by rank among the valid positions)
      }
      __syncthreads();
    }
    // weights of every position
    // (softmax: wave 0 finds the max and the sum of the exponentials -- n <= 128: two per lane, then a butterfly, so every
    // lane holds the same bits -- and leaves them in LDS for everyone)
    if (a.softmax && n > 0 && tid < kWave) {
      float m = -3.0e38f;
      for (int i = tid; i < n; i += kWave) m = s.sc[i] > m ? s.sc[i] : m;
#pragma unroll
      for (int o = kWave / 2; o >= 1; o >>= 1) {
        const float u = __shfl_xor(m, o, kWave);
        m = u > m ? u : m;
      }
      float d = 0.f;
      for (int i = tid; i < n; i += kWave) d += expf(s.sc[i] - m);
      d = wave_sum(d);
      if (tid == 0) {
        red[0] = m;
        red[1] = d;
      }
    }
    for (int t = tid; t < T; t += kT) s.wbuf[t] = (a.softmax && n == 0) ? 1.f / static_cast<float>(T) : 0.f;
    __syncthreads();
    const float mx = red[0], den = red[1];     // (read only under softmax with n > 0)
    for (int i = tid; i < n; i += kT) s.wbuf[s.idx[i]] = a.softmax ? expf(s.sc[i] - mx) / den : s.sc[i];
    __syncthreads();
    if (a.wts_w)
      for (int t = tid; t < T; t += kT) stg_f32(a.wts_w + static_cast<int64_t>(b) * T + t, s.wbuf[t]);
    // out = sum_t w_t k_t: thread (j, quarter of the positions), the quarters added in order
    {
      const int j = tid & 63, part = tid >> 6;
      const bool all = a.softmax && n == 0;
      const int cnt = all ? T : n;
      float acc = 0.f;
      if (j < E) {
        const float* Kb = a.K + static_cast<int64_t>(b) * a.ldk + s.kaddr[j];
        const int64_t st = s.kstp[j];
        for (int i = part; i < cnt; i += 4) {
          const int t = all ? i : s.idx[i];
          acc = __builtin_fmaf(s.wbuf[t], ldg_f32(Kb + t * st), acc);
        }
        red[part * E + j] = acc;
      }
      __syncthreads();
      if (tid < E)
        stg_f32(a.out + static_cast<int64_t>(b) * a.ldo + tid,
                ((red[tid] + red[E + tid]) + red[2 * E + tid]) + red[3 * E + tid]);
    }
  }
}

// LDS: carve(kRowsB) | g [E] | gq [E] | dsc [T] | vld [T] | d0, d1, shr [R][maxH + 1] each | gqp [R][E] | tmp [maxH]
__global__ __launch_bounds__(kT) void k_din_bwd(DinArgs a) {
  extern __shared__ __align__(16) float smem[];
  constexpr int R = kRowsB;
  const Lds s = carve(smem, a, R);
  const int tid = threadIdx.x, E = a.E, T = a.T, L = a.L, act = a.act;
  float* g = s.rest;
  float* gq = g + E;
  float* dsc = gq + E;
  int* vld = reinterpret_cast<int*>(dsc + T);
  float* d0 = dsc + 2 * T;
  float* d1 = d0 + R * (a.maxH + 1);
  float* shr = d1 + R * (a.maxH + 1);     // prelu: every element's share of d loss / d slope
  float* gqp = shr + R * (a.maxH + 1);
  float* tmp = gqp + R * E;
  fill_tables(s, a);
  float* mine = a.part + static_cast<int64_t>(blockIdx.x) * a.n_params;
  for (int e = tid; e < a.n_params; e += kT) mine[e] = 0.f;
  const int HL = pick3(a.H, L - 1);
  const float* wd = a.params + a.pdense;

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    __syncthreads();
    begin_sample(s, a, b);
    const int n = *s.n;
    for (int j = tid; j < E; j += kT) {
      g[j] = ldg_f32(a.gout + static_cast<int64_t>(b) * a.ldgo + j);
      gq[j] = 0.f;
    }
    for (int t = tid; t < T; t += kT) {
      s.wbuf[t] = ldg_f32(a.wts + static_cast<int64_t>(b) * T + t);
      vld[t] = 0;
    }
    __syncthreads();
    const float* Kb = a.K + static_cast<int64_t>(b) * a.ldk;
    float* gKb = a.gK + static_cast<int64_t>(b) * a.ldgk;
    for (int i = tid; i < n; i += kT) {      // g . k_t of the valid positions, by rank
      const int t = s.idx[i];
      float acc = 0.f;
      for (int j = 0; j < E; ++j) acc = __builtin_fmaf(g[j], ldg_f32(Kb + s.kaddr[j] + t * s.kstp[j]), acc);
      s.sc[i] = acc;
    }
    __syncthreads();
    float c = 0.f;
    if (a.softmax)
      for (int i = 0; i < n; ++i) c = __builtin_fmaf(s.wbuf[s.idx[i]], s.sc[i], c);
    for (int i = tid; i < n; i += kT) {      // d loss / d score, by position
      const int t = s.idx[i];
      dsc[t] = a.softmax ? s.wbuf[t] * (s.sc[i] - c) : s.sc[i];
      vld[t] = 1;
    }
    __syncthreads();
    // positions that are not valid: no path through the unit, only w_t g (0, or g / T in a softmax row without any)
    if (n < T)
      for (int e = tid; e < T * E; e += kT) {
        const int t = e / E, j = e - t * E;
        if (!vld[t]) stg_f32(gKb + s.kaddr[j] + t * s.kstp[j], s.wbuf[t] * g[j]);
      }

    for (int c0 = 0; c0 < n; c0 += R) {
      const int nr = n - c0 < R ? n - c0 : R;
      load_keys(s, a, b, c0, nr);
      __syncthreads();
      if (act == ACT_PRELU) layers<true>(s, a, nr);
      else layers<false>(s, a, nr);
      // ---- dense: score = wd . a_L + bd
      {
        const float slope = act == ACT_PRELU ? ldg_f32(a.params + a.pdense - 1) : 0.f;
        const float* aL = pick3(s.a, L - 1);
        for (int idx = tid; idx < HL + 1; idx += kT) {
          float sum = 0.f;
          for (int r = 0; r < nr; ++r) {
            float v = idx < HL ? aL[r * (HL + 1) + idx] : 1.f;
            if (act == ACT_PRELU && idx < HL) v = v > 0.f ? v : slope * v;
            sum = __builtin_fmaf(dsc[s.idx[c0 + r]], v, sum);
          }
          mine[a.pdense + idx] += sum;
        }
        for (int e = tid; e < nr * HL; e += kT) {
          const int h = e / nr, r = e - h * nr;
          const float v = aL[r * (HL + 1) + h];
          const float dA = dsc[s.idx[c0 + r]] * ldg_f32(wd + h);
          d0[r * (a.maxH + 1) + h] = dA * act_grad(act, v, slope);
          if (act == ACT_PRELU) shr[r * (a.maxH + 1) + h] = v > 0.f ? 0.f : dA * v;
        }
      }
      __syncthreads();
      float* dz = d0;
      float* dn = d1;
      for (int l = L - 1; l >= 0; --l) {
        const int H = pick3(a.H, l), IN = l == 0 ? 4 * E : pick3(a.H, l - 1), ldd = a.maxH + 1;
        const float* W = a.params + pick3(a.poff, l);
        if (act == ACT_PRELU) {      // slope of layer l: rows summed per unit, then the units in order
          for (int h = tid; h < H; h += kT) {
            float sum = 0.f;
            for (int r = 0; r < nr; ++r) sum += shr[r * ldd + h];
            tmp[h] = sum;
          }
          __syncthreads();
          if (tid == 0) {
            float sum = 0.f;
            for (int h = 0; h < H; ++h) sum += tmp[h];
            mine[pick3(a.poff, l) + H * IN + H] += sum;
          }
          __syncthreads();
        }
        // weight and bias gradients of layer l: thread owns elements idx = tid + 256 m of the [H * IN + H] block
        if (l > 0) {
          const float* x = pick3(s.a, l - 1);
          const float slope_in = act == ACT_PRELU ? ldg_f32(a.params + pick3(a.poff, l) - 1) : 0.f;
          for (int idx = tid; idx < H * IN + H; idx += kT) {
            float sum = 0.f;
            if (idx < H * IN) {
              const int h = idx / IN, i = idx - h * IN;
              for (int r = 0; r < nr; ++r) {
                float v = x[r * (IN + 1) + i];
                if (act == ACT_PRELU) v = v > 0.f ? v : slope_in * v;
                sum = __builtin_fmaf(dz[r * ldd + h], v, sum);
              }
            } else {
              for (int r = 0; r < nr; ++r) sum += dz[r * ldd + idx - H * IN];
            }
            mine[pick3(a.poff, l) + idx] += sum;
          }
          // d loss / d z of layer l - 1: thread = (row, unit of layer l - 1)
          for (int e = tid; e < nr * IN; e += kT) {
            const int i = e / nr, r = e - i * nr;
            float sum = 0.f;
            for (int h = 0; h < H; ++h) sum = __builtin_fmaf(dz[r * ldd + h], ldg_f32(W + h * IN + i), sum);
            const float v = x[r * (IN + 1) + i];
            dn[r * ldd + i] = sum * act_grad(act, v, slope_in);
            if (act == ACT_PRELU) shr[r * ldd + i] = v > 0.f ? 0.f : sum * v;
          }
          __syncthreads();
          float* sw = dz;
          dz = dn;
          dn = sw;
        } else {
          for (int idx = tid; idx < H * IN + H; idx += kT) {
            float sum = 0.f;
            if (idx < H * IN) {
              const int h = idx / IN, cidx = idx - h * IN, sg = cidx / E, j = cidx - sg * E;
              const float qj = s.q[j];
              for (int r = 0; r < nr; ++r) {
                const float kj = s.kb[r * (E + 1) + j];
                const float v = sg == 0 ? qj : sg == 1 ? kj : sg == 2 ? qj - kj : qj * kj;
                sum = __builtin_fmaf(dz[r * ldd + h], v, sum);
              }
            } else {
              for (int r = 0; r < nr; ++r) sum += dz[r * ldd + idx - H * IN];
            }
            mine[a.poff[0] + idx] += sum;
          }
          // through x = [q, k, q - k, q * k]: thread = (row, element j)
          for (int e = tid; e < nr * E; e += kT) {
            const int j = e / nr, r = e - j * nr;
            float x0 = 0.f, x1 = 0.f, x2 = 0.f, x3 = 0.f;
            for (int h = 0; h < H; ++h) {
              const float d = dz[r * ldd + h];
              const float* wr = W + h * IN + j;
              x0 = __builtin_fmaf(d, ldg_f32(wr), x0);
              x1 = __builtin_fmaf(d, ldg_f32(wr + E), x1);
              x2 = __builtin_fmaf(d, ldg_f32(wr + 2 * E), x2);
              x3 = __builtin_fmaf(d, ldg_f32(wr + 3 * E), x3);
            }
            const float qj = s.q[j], kj = s.kb[r * (E + 1) + j];
            const int t = s.idx[c0 + r];
            gqp[r * E + j] = (x0 + x2) + x3 * kj;
            stg_f32(gKb + s.kaddr[j] + t * s.kstp[j], ((x1 - x2) + x3 * qj) + s.wbuf[t] * g[j]);
          }
          __syncthreads();
          for (int j = tid; j < E; j += kT) {
            float sum = gq[j];
            for (int r = 0; r < nr; ++r) sum += gqp[r * E + j];
            gq[j] = sum;
          }
        }
      }
      __syncthreads();
    }
    for (int j = tid; j < E; j += kT) stg_f32(a.gQ + static_cast<int64_t>(b) * a.ldgq + s.qaddr[j], gq[j]);
  }
}

// out[i] = sum_g part[g][i] in workgroup order; thread (o, sl) adds the groups sl, sl + 16, ..., slices added in order
__global__ __launch_bounds__(256) void k_din_reduce(const float* __restrict__ part, int stride, int groups,
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

int host_extra(int act, int H) { return act == ACT_PRELU ? 1 : act == ACT_DICE ? 3 * H : 0; }

// the shape part of the arguments; DCTR_EINVAL / DCTR_ENOSUP / DCTR_OK
int shape(DinArgs& a, int T, int n_seg, const int32_t* dim, int n_layers, const int32_t* hidden, int act, int softmax) {
  if (T <= 0 || n_seg <= 0 || !dim || n_layers <= 0 || !hidden || act < 0 || act > ACT_DICE) return DCTR_EINVAL;
  if (T > kMaxT || n_seg > kMaxSeg || n_layers > kMaxL) return DCTR_ENOSUP;
  a.T = T; a.nseg = n_seg; a.L = n_layers; a.act = act; a.softmax = softmax ? 1 : 0;
  a.E = 0;
  for (int g = 0; g < n_seg; ++g) {
    if (dim[g] <= 0) return DCTR_EINVAL;
    a.dim[g] = dim[g];
    a.E += dim[g];
    if (a.E > kMaxE) return DCTR_ENOSUP;
  }
  int off = 0, in = 4 * a.E;
  a.sumH = a.maxH = 0;
  for (int l = 0; l < n_layers; ++l) {
    const int H = hidden[l];
    if (H <= 0) return DCTR_EINVAL;
    if (H > kMaxH) return DCTR_ENOSUP;
    a.H[l] = H;
    a.poff[l] = off;
    off += H * in + H + host_extra(act, H);
    in = H;
    a.sumH += H;
    a.maxH = H > a.maxH ? H : a.maxH;
  }
  a.pdense = off;
  a.n_params = off + in + 1;
  return DCTR_OK;
}

size_t base_floats(const DinArgs& a, int R) {
  return 6 * static_cast<size_t>(a.E) + a.E + 3 * static_cast<size_t>(a.T) + 1 + static_cast<size_t>(R) * (a.E + 1) +
         static_cast<size_t>(R) * (a.sumH + a.L);
}
size_t fwd_lds(const DinArgs& a) { return sizeof(float) * (base_floats(a, kRowsF) + 4 * static_cast<size_t>(a.E)); }
size_t bwd_lds(const DinArgs& a) {
  return sizeof(float) * (base_floats(a, kRowsB) + 2 * static_cast<size_t>(a.E) + 2 * static_cast<size_t>(a.T) +
                          3 * static_cast<size_t>(kRowsB) * (a.maxH + 1) + static_cast<size_t>(kRowsB) * a.E + a.maxH);
}

int fill(DinArgs& a, const float* Q, int64_t ld_q, const float* K, int64_t ld_k, int B, const int64_t* q_off,
         const int64_t* k_off, const int64_t* k_step, const int32_t* len, const uint8_t* mask, const float* params) {
  if (!Q || !K || !q_off || !k_off || !k_step || !params || (len == nullptr) == (mask == nullptr)) return DCTR_EINVAL;
  for (int g = 0; g < a.nseg; ++g) {
    if (q_off[g] < 0 || k_off[g] < 0 || k_step[g] < a.dim[g] || q_off[g] + a.dim[g] > ld_q ||
        k_off[g] + (a.T - 1) * k_step[g] + a.dim[g] > ld_k)
      return DCTR_EINVAL;
    a.qoff[g] = q_off[g]; a.koff[g] = k_off[g]; a.kstep[g] = k_step[g];
  }
  a.Q = Q; a.ldq = ld_q; a.K = K; a.ldk = ld_k; a.B = B; a.len = len; a.mask = mask; a.params = params;
  return DCTR_OK;
}

}  // namespace

extern "C" int dctr_din_attn_supported(int32_t T, int32_t n_seg, const int32_t* dim, int32_t n_layers,
                                       const int32_t* hidden, int32_t act) {
  DinArgs a = {};
  return shape(a, T, n_seg, dim, n_layers, hidden, act, 0) == DCTR_OK ? 1 : 0;
}

extern "C" size_t dctr_din_attn_bwd_workspace_floats(int32_t B, int32_t n_params) {
  if (B <= 0 || n_params <= 0) return 0;
  return static_cast<size_t>(B < kGroupsB ? B : kGroupsB) * static_cast<size_t>(n_params);
}

extern "C" int dctr_din_attn_fwd(const float* Q, int64_t ld_q, const float* K, int64_t ld_k, int32_t B, int32_t T,
                                 int32_t n_seg, const int32_t* dim, const int64_t* q_off, const int64_t* k_off,
                                 const int64_t* k_step, const int32_t* len, const uint8_t* mask, int32_t n_layers,
                                 const int32_t* hidden, int32_t act, int32_t softmax, const float* params, float* out,
                                 int64_t ld_out, float* weights, dctr_stream_t stream) {
  if (B == 0) return DCTR_OK;
  if (B < 0) return DCTR_EINVAL;
  DinArgs a = {};
  int rc = shape(a, T, n_seg, dim, n_layers, hidden, act, softmax);
  if (rc != DCTR_OK) return rc;
  rc = fill(a, Q, ld_q, K, ld_k, B, q_off, k_off, k_step, len, mask, params);
  if (rc != DCTR_OK) return rc;
  if (!out || ld_out < a.E) return DCTR_EINVAL;
  a.out = out; a.ldo = ld_out; a.wts_w = weights;
  k_din_fwd<<<dim3(B < kGroupsF ? B : kGroupsF), dim3(kT), fwd_lds(a), static_cast<hipStream_t>(stream)>>>(a);
  return launch_status();
}

extern "C" int dctr_din_attn_bwd(const float* Q, int64_t ld_q, const float* K, int64_t ld_k, int32_t B, int32_t T,
                                 int32_t n_seg, const int32_t* dim, const int64_t* q_off, const int64_t* k_off,
                                 const int64_t* k_step, const int32_t* len, const uint8_t* mask, int32_t n_layers,
                                 const int32_t* hidden, int32_t act, int32_t softmax, const float* params,
                                 const float* weights, const float* g_out, int64_t ld_gout, float* gQ, int64_t ld_gq,
                                 float* gK, int64_t ld_gk, float* g_params, float* workspace, dctr_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  DinArgs a = {};
  if (B < 0) return DCTR_EINVAL;
  if (B == 0) {   // no sample: zero parameter gradients, when the shape says how many there are
    if (g_params && shape(a, T, n_seg, dim, n_layers, hidden, act, softmax) == DCTR_OK)
      (void)hipMemsetAsync(g_params, 0, sizeof(float) * a.n_params, st);
    return DCTR_OK;
  }
  int rc = shape(a, T, n_seg, dim, n_layers, hidden, act, softmax);
  if (rc != DCTR_OK) return rc;
  if (act == ACT_DICE) return DCTR_ENOSUP;      // frozen Dice is a forward-only activation here
  rc = fill(a, Q, ld_q, K, ld_k, B, q_off, k_off, k_step, len, mask, params);
  if (rc != DCTR_OK) return rc;
  if (!weights || !g_out || !gQ || !gK || !g_params || !workspace || ld_gout < a.E) return DCTR_EINVAL;
  for (int g = 0; g < a.nseg; ++g)
    if (q_off[g] + a.dim[g] > ld_gq || k_off[g] + (a.T - 1) * k_step[g] + a.dim[g] > ld_gk) return DCTR_EINVAL;
  a.wts = weights; a.gout = g_out; a.ldgo = ld_gout; a.gQ = gQ; a.ldgq = ld_gq; a.gK = gK; a.ldgk = ld_gk;
  a.part = workspace;
  const int groups = B < kGroupsB ? B : kGroupsB;
  k_din_bwd<<<dim3(groups), dim3(kT), bwd_lds(a), st>>>(a);
  rc = launch_status();
  if (rc != DCTR_OK) return rc;
  k_din_reduce<<<dim3((a.n_params + 15) / 16), dim3(256), 0, st>>>(workspace, a.n_params, groups, g_params);
  return launch_status();
}
