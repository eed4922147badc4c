// gate_mix.hip -- the gates of the multi-task models (MMOE, one CGC level of PLE) on gfx950.
//
//   per sample b and gate g:   z = h_g[b] . W_g^T   w = softmax(z)   out_g[b, :] = sum_j w[j] x_{member_g[j]}[b, :]
// The reference runs Linear -> softmax -> unsqueeze -> torch.stack(experts) -> matmul -> squeeze per gate: ~6 launches
// forward, twice that backward, each with a [B, n, dim] copy of the expert outputs.  Here ONE launch per direction serves
// every gate that draws on one pool of experts.  A wave owns a sample: its lanes split the H columns of the logits (and
// the dim columns of the mix), the n <= 16 logits live in registers, the softmax is computed redundantly by every lane.
// The weight every gate gives pool member e is parked in lane e (one register per gate) and read back with
// v_readlane: the mix then walks the pool ONCE per sample, each expert row is loaded once for all the gates that use it.
//
// Backward, per workgroup (4 waves) over a contiguous run of samples:
//   1. wave per sample: s[j] = g_out_g[b] . x_{m[j]}[b], dz = w * (s - w.s), g_h = dz W, g_x[e] = sum_g coef_g[e] g_out_g;
//      dz [B, sum n] goes to the workspace (each wave reads back what it wrote);
//   2. gW_g = dz^T h_g: per 64-column tile of H a lane owns one column, 16 accumulators in registers over all the
//      workgroup's samples, the four waves' sums added through LDS in wave order, ONE write of the tile to the workgroup's
//      partial row;
//   k_gate_mix_reduce adds the partial rows in workgroup order (no atomics anywhere: identical bits from run to run).
// Limits: see dctr.h.
#include "common.hpp"

using namespace dctr;

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = kWaves * kWave;
constexpr int kMaxG = DCTR_GATE_MAX_GATES, kMaxN = DCTR_GATE_MAX_MEMBERS, kMaxP = DCTR_GATE_MAX_POOL;
constexpr int kFwdGroups = 1024;                  // 4096 waves: about one round of the chip
constexpr int kBwdGroups = 1024;
constexpr size_t kPartBudget = size_t(4) << 20;   // floats of partial rows (16 MB): fewer workgroups for huge gates

struct GateDev {
  const float* h;
  const float* W;
  float* out;
  float* w;
  const float* gout;
  float* gh;
  float* gW;
  int64_t ldh, ldo, ldgo, ldgh;
  int ldw, H, n;
  int noff;          // of this gate's dz in a sample's row of the workspace
  int woff;          // of this gate's gW in a partial row
  uint32_t mask;     // pool members it mixes
  uint8_t member[kMaxN];
};

struct MixArgs {
  const float* x[kMaxP];
  int64_t ldx[kMaxP];
  float* gx[kMaxP];
  int64_t ldgx[kMaxP];
  GateDev g[kMaxG];
  int B, P, G, dim;
  int sum_n, total;  // floats per dz row / per partial row
  int per_wg;        // bwd: samples per workgroup
  float* dz;         // bwd: [B, sum_n]
  float* part;       // bwd: [groups, total]
};

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

// z[j] = h[b] . W[j] for j < n, complete in every lane
__device__ __forceinline__ void gate_logits(const GateDev& q, int64_t b, int lane, float (&z)[kMaxN]) {
#pragma unroll
  for (int j = 0; j < kMaxN; ++j) z[j] = 0.f;
  const float* hr = q.h + b * q.ldh;
  for (int k = lane; k < q.H; k += kWave) {
    const float hv = ldg_f32(hr + k);
#pragma unroll
    for (int j = 0; j < kMaxN; ++j)
      if (j < q.n) z[j] = __builtin_fmaf(hv, ldg_f32(q.W + static_cast<int64_t>(j) * q.ldw + k), z[j]);
  }
#pragma unroll
  for (int j = 0; j < kMaxN; ++j)
    if (j < q.n) z[j] = wave_sum(z[j]);
}

// lane e: the weight the gate gives pool member e (a member listed twice gets both shares)
__device__ __forceinline__ float member_share(const GateDev& q, const float (&w)[kMaxN], int lane) {
  float c = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxN; ++j)
    if (j < q.n && q.member[j] == lane) c += w[j];
  return c;
}

// slot[g] = v with g a run-time index: a chain of selects, so that the array stays in registers
__device__ __forceinline__ void set_slot(float (&slot)[kMaxG], int g, float v) {
#pragma unroll
  for (int i = 0; i < kMaxG; ++i) slot[i] = i == g ? v : slot[i];
}

__global__ __launch_bounds__(kThreads) void k_gate_mix_fwd(MixArgs a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  for (int64_t b = blockIdx.x * kWaves + wave; b < a.B; b += static_cast<int64_t>(gridDim.x) * kWaves) {
    float coef[kMaxG];
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) coef[g] = 0.f;
#pragma nounroll
    for (int g = 0; g < a.G; ++g) {
      {
        const GateDev& q = a.g[g];
        float z[kMaxN];
        gate_logits(q, b, lane, z);
        float m = z[0];
#pragma unroll
        for (int j = 1; j < kMaxN; ++j)
          if (j < q.n) m = fmaxf(m, z[j]);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxN; ++j)
          if (j < q.n) {
            z[j] = expf(z[j] - m);
            sum += z[j];
          }
        const float inv = 1.f / sum;
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < kMaxN; ++j)
          if (j < q.n) {
            z[j] *= inv;
            if (lane == j) mine = z[j];
          }
        if (q.w && lane < q.n) stg_f32(q.w + b * q.n + lane, mine);
        set_slot(coef, g, member_share(q, z, lane));
      }
    }
    for (int d = lane; d < a.dim; d += kWave) {
      float acc[kMaxG];
#pragma unroll
      for (int g = 0; g < kMaxG; ++g) acc[g] = 0.f;
      for (int e = 0; e < a.P; ++e) {
        const float xv = ldg_f32(a.x[e] + b * a.ldx[e] + d);
#pragma unroll
        for (int g = 0; g < kMaxG; ++g)
          if (g < a.G && ((a.g[g].mask >> e) & 1u)) acc[g] = __builtin_fmaf(lane_value(coef[g], e), xv, acc[g]);
      }
#pragma unroll
      for (int g = 0; g < kMaxG; ++g)
        if (g < a.G) stg_f32(a.g[g].out + b * a.g[g].ldo + d, acc[g]);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_gate_mix_bwd(MixArgs a) {
  __shared__ float red[kWaves][kMaxN * kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * a.per_wg;
  const int64_t hi = lo + a.per_wg < a.B ? lo + a.per_wg : a.B;

  // 1. per sample: dz, g_h, g_x
  for (int64_t b = lo + wave; b < hi; b += kWaves) {
    float coef[kMaxG];
#pragma unroll
    for (int g = 0; g < kMaxG; ++g) coef[g] = 0.f;
#pragma nounroll
    for (int g = 0; g < a.G; ++g) {
      {
        const GateDev& q = a.g[g];
        float* dzr = a.dz + b * a.sum_n + q.noff;
        float* ghr = q.gh + b * q.ldgh;
        if (!q.gout) {       // nothing downstream used this gate's output
          if (lane < q.n) stg_f32(dzr + lane, 0.f);
          for (int k = lane; k < q.H; k += kWave) stg_f32(ghr + k, 0.f);
        } else {
          float w[kMaxN], s[kMaxN];
          const float* xr[kMaxN];
#pragma unroll
          for (int j = 0; j < kMaxN; ++j) {
            s[j] = 0.f;
            w[j] = 0.f;
            xr[j] = nullptr;
            if (j < q.n) {
              w[j] = ldg_f32(q.w + b * q.n + j);
              xr[j] = a.x[q.member[j]] + b * a.ldx[q.member[j]];
            }
          }
          const float* gor = q.gout + b * q.ldgo;
          for (int d = lane; d < a.dim; d += kWave) {
            const float gv = ldg_f32(gor + d);
#pragma unroll
            for (int j = 0; j < kMaxN; ++j)
              if (j < q.n) s[j] = __builtin_fmaf(gv, ldg_f32(xr[j] + d), s[j]);
          }
          float t = 0.f;
#pragma unroll
          for (int j = 0; j < kMaxN; ++j)
            if (j < q.n) {
              s[j] = wave_sum(s[j]);
              t = __builtin_fmaf(w[j], s[j], t);
            }
          float mine = 0.f;
#pragma unroll
          for (int j = 0; j < kMaxN; ++j)
            if (j < q.n) {
              s[j] = w[j] * (s[j] - t);        // dz
              if (lane == j) mine = s[j];
            }
          if (lane < q.n) stg_f32(dzr + lane, mine);
          for (int k = lane; k < q.H; k += kWave) {
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < kMaxN; ++j)
              if (j < q.n) acc = __builtin_fmaf(s[j], ldg_f32(q.W + static_cast<int64_t>(j) * q.ldw + k), acc);
            stg_f32(ghr + k, acc);
          }
          set_slot(coef, g, member_share(q, w, lane));
        }
      }
    }
    for (int d = lane; d < a.dim; d += kWave) {
      float gv[kMaxG];
#pragma unroll
      for (int g = 0; g < kMaxG; ++g)
        gv[g] = (g < a.G && a.g[g].gout) ? ldg_f32(a.g[g].gout + b * a.g[g].ldgo + d) : 0.f;
      for (int e = 0; e < a.P; ++e) {
        float acc = 0.f;
#pragma unroll
        for (int g = 0; g < kMaxG; ++g)
          if (g < a.G && a.g[g].gout && ((a.g[g].mask >> e) & 1u))
            acc = __builtin_fmaf(lane_value(coef[g], e), gv[g], acc);
        stg_f32(a.gx[e] + b * a.ldgx[e] + d, acc);
      }
    }
  }
  __syncthreads();

  // 2. this workgroup's share of every gW, one 64-column tile at a time
  float* mine = a.part + static_cast<int64_t>(blockIdx.x) * a.total;
  for (int g = 0; g < a.G; ++g) {
    const GateDev& q = a.g[g];
    if (!q.gout) continue;
    for (int k0 = 0; k0 < q.H; k0 += kWave) {
      const int kc = k0 + lane < q.H ? k0 + lane : q.H - 1;
      float acc[kMaxN];
#pragma unroll
      for (int j = 0; j < kMaxN; ++j) acc[j] = 0.f;
      for (int64_t b = lo + wave; b < hi; b += kWaves) {
        const float hv = ldg_f32(q.h + b * q.ldh + kc);
        const float* dzr = a.dz + b * a.sum_n + q.noff;
#pragma unroll
        for (int j = 0; j < kMaxN; ++j)
          if (j < q.n) acc[j] = __builtin_fmaf(ldg_f32(dzr + j), hv, acc[j]);
      }
#pragma unroll
      for (int j = 0; j < kMaxN; ++j)
        if (j < q.n) red[wave][j * kWave + lane] = acc[j];
      __syncthreads();
      for (int e = threadIdx.x; e < q.n * kWave; e += kThreads) {
        const int j = e >> 6, k = k0 + (e & (kWave - 1));
        if (k < q.H) stg_f32(mine + q.woff + j * q.ldw + k, ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e]);
      }
      __syncthreads();
    }
  }
}

// gW_g[i] = sum over the workgroups' partial rows, in workgroup order; blockIdx.y = gate.  Thread (o, sl) adds the rows
// sl, sl + 16, ..., the 16 slices are added in order.  Padding columns and the gates without a gradient get zeros.
__global__ __launch_bounds__(256) void k_gate_mix_reduce(MixArgs a, int groups) {
  __shared__ float red[16][17];
  const GateDev& q = a.g[blockIdx.y];
  const int o = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int elems = q.n * q.ldw;
  const int i = blockIdx.x * 16 + o;
  const int ic = i < elems ? i : 0;
  const bool live = q.gout != nullptr && (ic % q.ldw) < q.H;
  float s = 0.f;
  if (live) {
    const float* col = a.part + q.woff + ic;
    for (int g0 = sl; g0 < groups; g0 += 16 * 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int g = g0 + 16 * u;
        v[u] = ldg_f32(col + static_cast<int64_t>(g < groups ? g : 0) * a.total);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (g0 + 16 * u < groups) s += v[u];
    }
  }
  red[sl][o] = s;
  __syncthreads();
  if (sl == 0 && i < elems) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += red[k][o];
    stg_f32(q.gW + i, live ? t : 0.f);
  }
}

int envelope(int P, int dim, int G, const int32_t* n, const int32_t* H) {
  if (P <= 0 || dim <= 0 || G <= 0 || !n || !H) return DCTR_EINVAL;
  for (int g = 0; g < G && g < kMaxG; ++g)
    if (n[g] <= 0 || H[g] <= 0) return DCTR_EINVAL;
  if (P > kMaxP || G > kMaxG || dim > DCTR_GATE_MAX_WIDTH) return DCTR_ENOSUP;
  for (int g = 0; g < G; ++g)
    if (n[g] > kMaxN || H[g] > DCTR_GATE_MAX_WIDTH) return DCTR_ENOSUP;
  return DCTR_OK;
}

// workgroups of the backward and the samples each takes
void bwd_split(int B, int64_t total, int* groups, int* per_wg) {
  int64_t cap = static_cast<int64_t>(kPartBudget) / (total > 0 ? total : 1);
  cap = cap < 1 ? 1 : (cap > kBwdGroups ? kBwdGroups : cap);
  int64_t want = (static_cast<int64_t>(B) + kWaves - 1) / kWaves;
  want = want < 1 ? 1 : (want > cap ? cap : want);
  *per_wg = static_cast<int>((B + want - 1) / want);
  *groups = (B + *per_wg - 1) / *per_wg;
}

// the shape part of the arguments, shared by both directions; DCTR_EINVAL / DCTR_ENOSUP / DCTR_OK
int fill(MixArgs& a, const float* const* x, const int64_t* ld_x, int P, int dim, int B, const dctr_gate_t* gates, int G) {
  if (B < 0 || !gates || !x || !ld_x || P <= 0 || G <= 0 || dim <= 0) return DCTR_EINVAL;
  if (P > kMaxP || G > kMaxG || dim > DCTR_GATE_MAX_WIDTH) return DCTR_ENOSUP;
  int32_t n[kMaxG], H[kMaxG];
  for (int g = 0; g < G; ++g) {
    n[g] = gates[g].n;
    H[g] = gates[g].H;
  }
  const int rc = envelope(P, dim, G, n, H);
  if (rc != DCTR_OK) return rc;
  a.B = B; a.P = P; a.G = G; a.dim = dim;
  for (int e = 0; e < P; ++e) {
    if (!x[e] || ld_x[e] < dim) return DCTR_EINVAL;
    a.x[e] = x[e];
    a.ldx[e] = ld_x[e];
  }
  int noff = 0;
  int64_t woff = 0;
  for (int g = 0; g < G; ++g) {
    const dctr_gate_t& s = gates[g];
    GateDev& q = a.g[g];
    if (!s.h || !s.W || s.ld_h < s.H || s.ld_w < s.H || s.ld_w > (1 << 24)) return DCTR_EINVAL;
    q.h = s.h; q.W = s.W; q.ldh = s.ld_h; q.ldw = static_cast<int>(s.ld_w); q.H = s.H; q.n = s.n;
    q.mask = 0;
    for (int j = 0; j < s.n; ++j) {
      if (s.member[j] < 0 || s.member[j] >= P) return DCTR_EINVAL;
      q.member[j] = static_cast<uint8_t>(s.member[j]);
      q.mask |= 1u << s.member[j];
    }
    q.noff = noff;
    q.woff = static_cast<int>(woff);
    noff += s.n;
    woff += static_cast<int64_t>(s.n) * s.ld_w;
  }
  if (woff > (int64_t(1) << 30)) return DCTR_EINVAL;
  a.sum_n = noff;
  a.total = static_cast<int>(woff);
  return DCTR_OK;
}

}  // namespace

extern "C" int dctr_gate_mix_supported(int32_t P, int32_t dim, int32_t G, const int32_t* n, const int32_t* H) {
  return envelope(P, dim, G, n, H) == DCTR_OK ? 1 : 0;
}

extern "C" size_t dctr_gate_mix_bwd_workspace_floats(int32_t B, int32_t G, const int32_t* n, const int32_t* ld_w) {
  if (B <= 0 || G <= 0 || G > kMaxG || !n || !ld_w) return 0;
  int64_t sum_n = 0, total = 0;
  for (int g = 0; g < G; ++g) {
    if (n[g] <= 0 || ld_w[g] <= 0) return 0;
    sum_n += n[g];
    total += static_cast<int64_t>(n[g]) * ld_w[g];
  }
  int groups = 0, per_wg = 0;
  bwd_split(B, total, &groups, &per_wg);
  return static_cast<size_t>(B) * static_cast<size_t>(sum_n) + static_cast<size_t>(groups) * static_cast<size_t>(total);
}

extern "C" int dctr_gate_mix_fwd(const float* const* x, const int64_t* ld_x, int32_t P, int32_t dim, int32_t B,
                                 const dctr_gate_t* gates, int32_t G, dctr_stream_t stream) {
  if (B == 0) return DCTR_OK;
  MixArgs a = {};
  const int rc = fill(a, x, ld_x, P, dim, B, gates, G);
  if (rc != DCTR_OK) return rc;
  for (int g = 0; g < G; ++g) {
    if (!gates[g].out || gates[g].ld_out < dim) return DCTR_EINVAL;
    a.g[g].out = gates[g].out;
    a.g[g].ldo = gates[g].ld_out;
    a.g[g].w = gates[g].w;
  }
  const int want = (B + kWaves - 1) / kWaves;
  k_gate_mix_fwd<<<dim3(want < kFwdGroups ? want : kFwdGroups), dim3(kThreads), 0, static_cast<hipStream_t>(stream)>>>(a);
  return launch_status();
}

extern "C" int dctr_gate_mix_bwd(const float* const* x, const int64_t* ld_x, int32_t P, int32_t dim, int32_t B,
                                 const dctr_gate_t* gates, int32_t G, float* const* g_x, const int64_t* ld_gx,
                                 float* workspace, dctr_stream_t stream) {
  if (B == 0) return DCTR_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  MixArgs a = {};
  const int rc = fill(a, x, ld_x, P, dim, B, gates, G);
  if (rc != DCTR_OK) return rc;
  if (!g_x || !ld_gx || !workspace) return DCTR_EINVAL;
  for (int e = 0; e < P; ++e) {
    if (!g_x[e] || ld_gx[e] < dim) return DCTR_EINVAL;
    a.gx[e] = g_x[e];
    a.ldgx[e] = ld_gx[e];
  }
  int max_elems = 0;
  for (int g = 0; g < G; ++g) {
    const dctr_gate_t& q = gates[g];
    if (!q.w || !q.g_h || !q.gW || q.ld_gh < q.H || (q.g_out && q.ld_gout < dim)) return DCTR_EINVAL;
    a.g[g].w = q.w; a.g[g].gout = q.g_out; a.g[g].ldgo = q.ld_gout; a.g[g].gh = q.g_h; a.g[g].ldgh = q.ld_gh;
    a.g[g].gW = q.gW;
    const int elems = q.n * static_cast<int>(q.ld_w);
    max_elems = elems > max_elems ? elems : max_elems;
  }
  int groups = 0;
  bwd_split(B, a.total, &groups, &a.per_wg);
  a.dz = workspace;
  a.part = workspace + static_cast<size_t>(B) * static_cast<size_t>(a.sum_n);
  k_gate_mix_bwd<<<dim3(groups), dim3(kThreads), 0, s>>>(a);
  const int st = launch_status();
  if (st != DCTR_OK) return st;
  k_gate_mix_reduce<<<dim3((max_elems + 15) / 16, G), dim3(256), 0, s>>>(a, groups);
  return launch_status();
}
