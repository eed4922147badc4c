// tower_tiles.hpp -- what the tower-shaped kernels share (mlp.hip, cross_tower.hip): the 16-sample row tile's constants,
// the kernel argument block, the general forward / backward-data bodies, the host-side checks, and the declaration of the
// weight-gradient launch that every backward ends with.
#pragma once

#include "common.hpp"

using namespace dctr;

// diagnostics (tools/mlp_trace.py): 16 wall_clock64 stamps per workgroup, or NULL -- only in the DCTR_DIAG build
// (libdctr_hip_diag.so); the shipped library keeps no mutable global state
#ifdef DCTR_DIAG
namespace dctr {
extern __attribute__((visibility("hidden"))) unsigned long long* g_mlp_trace;   // (defined in mlp.hip)
}
#define MLP_TRACE(T, slot)                                                                   \
  do {                                                                                       \
    if ((T) && threadIdx.x == 0) (T)[blockIdx.x * 16ull + (slot)] = wall_clock64();          \
  } while (0)
#else
static unsigned long long* const g_mlp_trace = nullptr;
#define MLP_TRACE(T, slot) do { } while (0)
#endif

namespace {

constexpr int kTM = 16;        // samples per workgroup (forward / backward-data)
constexpr int kT = 512;        // threads per workgroup (forward / backward-data)
constexpr int kWaves = kT / 64;
constexpr int kKC = 512;       // columns of the tower input staged in LDS at a time
constexpr int kNTMax = 4;      // output tiles a wave carries at once (forward)
constexpr int kTW = 256;       // threads per workgroup (wgrad)
constexpr int kMaxL = DCTR_MLP_MAX_LAYERS;
// Padding floats behind every LDS tile row (row strides are a multiple of 16 plus this).  The A operand of
// v_mfma_f32_16x16x4 is read as one ds_read_b128 per lane -- lane (g = lane / 16, c = lane % 16) takes the 16 bytes at
// row c, column 4 g of the K block -- and that instruction is served in four FIXED 16-lane groups
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...: MI355X_MICROARCH.md, LDS) over 16 slots of 16 bytes.  With a row pitch of
// s slots the lane's slot is (c s + g) mod 16: for odd s (the +4 padding of rounds 1-3: s = 13 and 1) every group has two
// lanes on one slot -- SQ_LDS_BANK_CONFLICT was 40 % of the tower's LDS cycles; for s = 2 mod 4 the eight rows of a group
// that share g land on eight distinct even (g = 0, 2) or odd (g = 1, 3) slots: conflict-free.  s = 2 mod 4 <=> pitch = 8 mod 16.
constexpr int kPad = 8;

__host__ __device__ __forceinline__ int round_up(int x, int m) { return (x + m - 1) / m * m; }

struct LayerDev {
  const float* W;
  const float* bias;
  float* h;
  float* dh;
  int K, N, ldw, ldh, relu;
};

struct MlpArgs {
  LayerDev L[kMaxL];
  int n_layers;
  int B;
  const float* x;
  int64_t ldx;
  const float* w_out;
  float* logit;      // forward: [B] (with w_out)
  const float* g;    // backward: [B] (with w_out) or [B, ldg]
  int64_t ldg;
  float* gx;         // backward: [B, ldgx] nullable
  int64_t ldgx;
  int rsx, rsh;      // LDS row strides (floats) of the forward
  int kc;            // columns of the tower input staged in LDS at a time (<= kKC; smaller for wide towers)
  int rsd;           // LDS row stride of the backward-data pass
  int fast;          // 1: the tower fits the fast bodies (mlp_fwd_fast / mlp_bwd_fast)
  uint32_t wmask;    // diagnostics: AND mask on the weight byte offsets (0xffffffff normally; DCTR_MLP_WMASK in the diag build
                     // folds the weight stream onto a few KB that stay in L1 -- timing experiment, wrong results)
  unsigned long long* trace;
};

__device__ __forceinline__ f32x4 ldg_f4(const float* p) { return *(const DCTR_GLOBAL f32x4*)p; }

// ------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------
// NT output tiles (16 columns each) of one layer over the K range [kg0, kg0 + klen) whose A rows sit in LDS.
//  * No load in the loop is predicated (a predicated load becomes a branch and serialises the loop on memory
//    latency): columns past N re-read row N-1 (their results are dropped by the epilogue) and a dwordx4 that
//    would leave the row is pulled back inside it (its A elements are zero, and weights are finite).
//  * The weight stream runs kPD-1 iterations ahead of the matrix pipe in a register ring (one iteration is
//    4*NT MFMAs = 128*NT cycles, so fewer tiles => deeper ring to cover the L2 latency).
//  * Addresses are a uniform base + one 32-bit lane offset per tile (+ a per-iteration byte offset shared by the
//    tiles): ~NT+2 vector ALU instructions per iteration next to 4*NT MFMAs.
//  * A tile's k-steps alternate between KS accumulators so that at least four independent MFMA chains are in
//    flight per wave (a dependent 16x16x4 chain leaves the matrix pipe idle between issues).
//  * `between()` runs after the ring prologue has been issued: the kernel stages the A chunk there, so the
//    first weight loads overlap the staging's own memory latency.
template <int NT, typename Between>
__device__ __forceinline__ void fwd_tiles(const float* As, int rs, int kg0, int klen, const LayerDev& Ld,
                                          int tile0, f32x4* acc, int g, int c, Between between) {
  constexpr int kPD = NT == 1 ? 12 : (NT == 2 ? 8 : (NT == 3 ? 6 : 4));
  constexpr int KS = NT >= 4 ? 1 : (NT >= 2 ? 2 : 4);
  const DCTR_GLOBAL char* wbase = (const DCTR_GLOBAL char*)Ld.W;
  // first column this lane reads, pulled back inside the row when the (16-wide, zero-padded in LDS) K range is wider
  // than the weight row itself (K < 12: the lane's A elements are zero there).  Was computed unsigned: for tiny K the
  // offset wrapped and the last row's loads left the allocation (round 2, tools/uninit_probe.py).
  const int col0 = (kg0 + 4 * g) < (Ld.ldw - 4) ? (kg0 + 4 * g) : (Ld.ldw - 4);
  uint32_t voff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int n = (tile0 + t * kWaves) * 16 + c;
    n = n < Ld.N ? n : Ld.N - 1;
    voff[t] = (static_cast<uint32_t>(n) * static_cast<uint32_t>(Ld.ldw) + static_cast<uint32_t>(col0)) * 4u;
  }
  const float* ap = As + c * rs + 4 * g;
  const int n_it = klen >> 4;
  const uint32_t omax = static_cast<uint32_t>(Ld.ldw - 4 - col0) * 4u;  // largest in-row byte offset (>= 0)
  auto woff = [&](int it) -> uint32_t {
    it = it < n_it ? it : n_it - 1;                       // scalar: `it` is wave-uniform
    const uint32_t o = static_cast<uint32_t>(it) << 6;
    return o < omax ? o : omax;
  };
  f32x4 ring[kPD][NT];
#pragma unroll
  for (int d = 0; d < kPD - 1; ++d) {
    const uint32_t o = woff(d);
#pragma unroll
    for (int t = 0; t < NT; ++t) ring[d][t] = *(const DCTR_GLOBAL f32x4*)(wbase + (voff[t] + o));
  }
  between();
  f32x4 accs[NT][KS];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    accs[t][0] = acc[t];
#pragma unroll
    for (int k = 1; k < KS; ++k) accs[t][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const int n_grp = n_it / kPD, rem = n_it - n_grp * kPD;
  f32x4 a_nxt = *reinterpret_cast<const f32x4*>(ap);
  for (int gi = 0; gi < n_grp; ++gi) {
#pragma unroll
    for (int d = 0; d < kPD; ++d) {
      const int it = gi * kPD + d;
      const uint32_t o = woff(it + kPD - 1);
#pragma unroll
      for (int t = 0; t < NT; ++t) ring[(d + kPD - 1) % kPD][t] = *(const DCTR_GLOBAL f32x4*)(wbase + (voff[t] + o));
      const f32x4 a4 = a_nxt;
      const int itn = it + 1 < n_it ? it + 1 : it;
      a_nxt = *reinterpret_cast<const f32x4*>(ap + (itn << 4));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) accs[t][j % KS] = mfma16(a4[j], ring[d][t][j], accs[t][j % KS]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < kPD - 1; ++d) {
    if (d < rem) {
      const int it = n_grp * kPD + d;
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(ap + (it << 4));
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) accs[t][j % KS] = mfma16(a4[j], ring[d][t][j], accs[t][j % KS]);
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4 r = accs[t][0];
#pragma unroll
    for (int k = 1; k < KS; ++k) r += accs[t][k];
    acc[t] = r;
  }
}

template <typename Between>
__device__ __forceinline__ void fwd_dispatch(int nt, const float* As, int rs, int kg0, int klen, const LayerDev& Ld,
                                             int tile0, f32x4* acc, int g, int c, Between between) {
  switch (nt) {
    case 1: fwd_tiles<1>(As, rs, kg0, klen, Ld, tile0, acc, g, c, between); break;
    case 2: fwd_tiles<2>(As, rs, kg0, klen, Ld, tile0, acc, g, c, between); break;
    case 3: fwd_tiles<3>(As, rs, kg0, klen, Ld, tile0, acc, g, c, between); break;
    case 4: fwd_tiles<4>(As, rs, kg0, klen, Ld, tile0, acc, g, c, between); break;
    default: between(); break;   // a wave without tiles still takes part in the staging barriers
  }
}

// the forward of one 16-sample row tile; `logit_lds` (nullable): [16] LDS floats that receive the projection.
// CROSS: the layers are the matrix form of CrossNet (interaction.py:448-451) instead of Linear + activation:
//     u_l = x_l W_l^T + b_l ;  x_{l+1} = x_0 (.) u_l + x_l          (every layer W x W, x_0 = the staged input tile)
// u_l is parked in the layer's `dh` buffer (the backward needs it and overwrites it with its own d loss / d u_l).
// Returns the LDS tile [16][rsh] that holds the top layer's output when the body ends.
template <bool CROSS = false>
__device__ __forceinline__ const float* mlp_fwd_body(const MlpArgs& A, float* smem, float* logit_lds) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int b0 = blockIdx.x * kTM;
  const int rsx = A.rsx, rsh = A.rsh;
  float* xs = smem;               // [16][rsx]  chunk of the tower input
  float* hb0 = xs + kTM * rsx;    // [16][rsh]  ping
  float* hb1 = hb0 + kTM * rsh;   // [16][rsh]  pong
  const int K0 = A.L[0].K, K0p = round_up(K0, 16);
  const int kcw = K0p < A.kc ? K0p : A.kc;
  MLP_TRACE(A.trace, 0);
  // the projection's weights, requested now and used after the last layer (it used to wait for them there)
  float wo_pre[4] = {0.f, 0.f, 0.f, 0.f};
  if (A.w_out && (A.logit || logit_lds)) {
    const int ntop = A.L[A.n_layers - 1].N;
#pragma unroll
    for (int i = 0; i < 4; ++i) wo_pre[i] = ldg_f32(A.w_out + ((lane + 64 * i) < ntop ? (lane + 64 * i) : ntop - 1));
  }

  const float* in = nullptr;
  for (int l = 0; l < A.n_layers; ++l) {
    const LayerDev& Ld = A.L[l];
    const int ntile = (Ld.N + 15) >> 4;
    float* outb = (l & 1) ? hb1 : hb0;
    for (int tbase = 0; tbase < ntile; tbase += kWaves * kNTMax) {
      const int tile0 = tbase + wv;
      int nt = 0;
#pragma unroll
      for (int t = 0; t < kNTMax; ++t) nt += (tile0 + t * kWaves < ntile) ? 1 : 0;
      f32x4 acc[kNTMax];
#pragma unroll
      for (int t = 0; t < kNTMax; ++t) {
        const int n = (tile0 + t * kWaves) * 16 + c;
        const float bv = (t < nt && n < Ld.N && Ld.bias) ? ldg_f32(Ld.bias + n) : 0.f;
        acc[t] = f32x4{bv, bv, bv, bv};
      }
      if (l == 0) {
        for (int kc = 0; kc < K0p; kc += kcw) {
          const int klen = (K0p - kc) < kcw ? (K0p - kc) : kcw;
          auto stage = [&]() {
            __syncthreads();  // the previous chunk (or pass) is consumed
            // No load here is predicated (a predicated load is a branch around the load with its own vmcnt(0): the
            // loop used to be one memory round trip per iteration, 4.9 us for the 27 KB tile of the DeepFM tower --
            // round 3): rows past B re-read row B-1, a dwordx4 that would leave the row is pulled back inside it
            // (ld_x % 4 == 0), and what lies past K0 or B is zeroed by a select on the way to LDS.
            const int q4 = klen >> 2, n_e = kTM * q4;
            const int64_t blast = A.B - 1;
            for (int e0 = 0; e0 < n_e; e0 += 4 * kT) {
              f32x4 v[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                int e = e0 + i * kT + tid;
                e = e < n_e ? e : n_e - 1;
                const int r = e / q4, q = e - r * q4;
                const int k = kc + 4 * q;
                const int64_t b = (b0 + r) < blast ? (b0 + r) : blast;
                const int64_t kk = k < A.ldx - 4 ? k : A.ldx - 4;
                v[i] = ldg_f4(A.x + b * A.ldx + kk);
              }
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int e = e0 + i * kT + tid;
                if (e < n_e) {
                  const int r = e / q4, q = e - r * q4;
                  const int k = kc + 4 * q;
                  const bool rv = b0 + r < A.B && k <= A.ldx - 4;
                  f32x4 w;
                  w.x = (rv && k < K0) ? v[i].x : 0.f;
                  w.y = (rv && k + 1 < K0) ? v[i].y : 0.f;
                  w.z = (rv && k + 2 < K0) ? v[i].z : 0.f;
                  w.w = (rv && k + 3 < K0) ? v[i].w : 0.f;
                  *reinterpret_cast<f32x4*>(xs + r * rsx + 4 * q) = w;
                }
              }
            }
            __syncthreads();
            if (kc == 0 && tbase == 0) MLP_TRACE(A.trace, 1);
          };
          fwd_dispatch(nt, xs, rsx, kc, klen, Ld, tile0, acc, g, c, stage);
        }
      } else {
        fwd_dispatch(nt, in, rsh, 0, round_up(Ld.K, 16), Ld, tile0, acc, g, c, []() {});
      }
      if (tbase == 0) MLP_TRACE(A.trace, 2 + 3 * l);
      // epilogue: activation; keep the tile in LDS for the next layer, save it for the backward
#pragma unroll
      for (int t = 0; t < kNTMax; ++t) {
        if (t < nt) {
          const int n = (tile0 + t * kWaves) * 16 + c;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * g + r;
            float v = acc[t][r];
            if (CROSS) {
              const float x0v = xs[row * rsx + n];                  // (K0 <= kKC: the whole input tile is staged)
              const float xlv = (l == 0) ? x0v : in[row * rsh + n];
              if (Ld.dh && n < Ld.N && b0 + row < A.B) stg_f32(Ld.dh + static_cast<int64_t>(b0 + row) * Ld.ldh + n, v);
              v = x0v * v + xlv;
            } else if (Ld.relu) {
              v = v > 0.f ? v : 0.f;
            }
            if (n >= Ld.N) v = 0.f;
            outb[row * rsh + n] = v;
            if (Ld.h && n < Ld.N && b0 + row < A.B) stg_f32(Ld.h + static_cast<int64_t>(b0 + row) * Ld.ldh + n, v);
          }
        }
      }
    }
    MLP_TRACE(A.trace, 3 + 3 * l);
    __syncthreads();
    MLP_TRACE(A.trace, 4 + 3 * l);
    in = outb;
  }
  if (A.w_out && (A.logit || logit_lds)) {  // dnn_linear: logit[b] = h_last[b, :] . w_out
    const LayerDev& Lt = A.L[A.n_layers - 1];
    for (int row = wv; row < kTM; row += kWaves) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (lane + 64 * i < Lt.N) s += in[row * rsh + lane + 64 * i] * wo_pre[i];
      for (int n = lane + 256; n < Lt.N; n += 64) s += in[row * rsh + n] * ldg_f32(A.w_out + n);
      s = wave_sum(s);
      if (lane == 0) {
        if (A.logit && b0 + row < A.B) stg_f32(A.logit + b0 + row, s);
        if (logit_lds) logit_lds[row] = s;
      }
    }
  }
  MLP_TRACE(A.trace, 15);
  return in;
}

// ------------------------------------------------------------------------------------------------------------
// backward, data path: dH_l (gradient w.r.t. the pre-activation of layer l) for every layer, then d/d input
// ------------------------------------------------------------------------------------------------------------
// Q consecutive output columns per lane (a group of 16 Q columns per wave pass) of d loss / d input of layer l:
//     out[16 rows][16 Q cols] = din[16][Np] . W_l[Np][cols]          (reduction over the layer's N outputs)
// then the epilogue: relu mask of the layer below, into LDS (`dout`) for the next pass and into its `dh`; at l = 0 into gx.
//  * Q = 4: 64-column groups, dwordx4 weight loads; Q = 2: 32-column groups, dwordx2 -- chosen when the 64-column groups
//    would leave waves without work (a 256-wide layer has 4 of them for 8 waves: round 3).
//  * ldw % 4 == 0: a load at col0 < ldw stays inside the row.  Columns past it re-read column 0 and rows past N re-read
//    row N-1 (the A operand is zero there): no predicated loads in the loop.
//  * The relu mask of the layer below (its saved output h) is requested BEFORE the weight ring and the MFMA loop and
//    consumed in the epilogue (it used to be loaded there: one exposed round trip per pass).
template <int Q>
__device__ __forceinline__ void bwd_cols(const MlpArgs& A, int l, const float* din, float* dout, int rs, int gb, int b0,
                                         int g, int c) {
  typedef float vecq __attribute__((ext_vector_type(Q)));
  const LayerDev& Ld = A.L[l];
  const int Np = round_up(Ld.N, 16);      // reduction length
  const int Kp = round_up(Ld.K, 16);      // output columns kept in LDS for the next (lower) layer
  const int col0 = 16 * Q * gb + Q * c;
  const int colc = col0 < Ld.ldw ? col0 : 0;
  const int lp = l > 0 ? l - 1 : 0;
  const LayerDev& Lp = A.L[lp];           // (l == 0: only its buffer is borrowed as a valid address)
  vecq hpre[4];
  {
    const int cc = col0 < Lp.ldh - Q ? col0 : Lp.ldh - Q;
    const int64_t blast = A.B - 1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t b = (b0 + 4 * g + r) < blast ? (b0 + 4 * g + r) : blast;
      hpre[r] = *(const DCTR_GLOBAL vecq*)(Lp.h + b * Lp.ldh + cc);
    }
  }
  f32x4 acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* ap = din + c * rs + 4 * g;
  const int n_it = Np >> 4;
  // uniform base + 32-bit lane offsets: row n = 16 it + 4 g + j of W starts at byte (n * ldw + colc) * 4
  const DCTR_GLOBAL char* wbase = (const DCTR_GLOBAL char*)Ld.W;
  const uint32_t ldw4 = static_cast<uint32_t>(Ld.ldw) * 4u;
  const uint32_t vlast = static_cast<uint32_t>(Ld.N - 1) * ldw4 + static_cast<uint32_t>(colc) * 4u;
  uint32_t vrow[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) vrow[j] = static_cast<uint32_t>(4 * g + j) * ldw4 + static_cast<uint32_t>(colc) * 4u;
  auto wld = [&](int it, vecq* dst) {
    it = it < n_it ? it : n_it - 1;                               // scalar
    const uint32_t so = static_cast<uint32_t>(it) * 16u * ldw4;  // scalar
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t o = vrow[j] + so;
      o = o < vlast ? o : vlast;                                  // rows past N re-read row N-1 (A is 0 there)
      dst[j] = *(const DCTR_GLOBAL vecq*)(wbase + o);
    }
  };
  constexpr int PD = Q == 4 ? 5 : 8;      // an iteration is 4 Q MFMAs: fewer columns => deeper ring to cover the L2 latency
  vecq ring[PD][4];
#pragma unroll
  for (int d = 0; d < PD - 1; ++d) wld(d, ring[d]);
  const int n_grp = n_it / PD, rem = n_it - n_grp * PD;
  f32x4 a_nxt = *reinterpret_cast<const f32x4*>(ap);
  for (int gi = 0; gi < n_grp; ++gi) {
#pragma unroll
    for (int d = 0; d < PD; ++d) {
      const int it = gi * PD + d;
      wld(it + PD - 1, ring[(d + PD - 1) % PD]);
      const f32x4 a4 = a_nxt;
      const int itn = it + 1 < n_it ? it + 1 : it;
      a_nxt = *reinterpret_cast<const f32x4*>(ap + (itn << 4));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = mfma16(a4[j], ring[d][j][q], acc[q]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int d = 0; d < PD - 1; ++d) {
    if (d < rem) {
      const int it = n_grp * PD + d;
      const f32x4 a4 = *reinterpret_cast<const f32x4*>(ap + (it << 4));
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = mfma16(a4[j], ring[d][j][q], acc[q]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * g + r;
    const int64_t b = b0 + row;
    vecq v;
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = acc[q][r];
    if (l > 0) {
      if (col0 < Kp) {    // Lp.N == Ld.K
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          float o = v[q];
          if (Lp.relu && !(hpre[r][q] > 0.f)) o = 0.f;
          if (col0 + q >= Lp.N || b >= A.B) o = 0.f;
          v[q] = o;
        }
        *reinterpret_cast<vecq*>(dout + row * rs + col0) = v;
        if (Lp.dh && b < A.B) {
          if (col0 + Q - 1 < Lp.N) *(DCTR_GLOBAL vecq*)(Lp.dh + b * Lp.ldh + col0) = v;
          else
            for (int q = 0; q < Q; ++q)
              if (col0 + q < Lp.N) stg_f32(Lp.dh + b * Lp.ldh + col0 + q, v[q]);
        }
      }
    } else if (b < A.B) {
      // columns [K, ldgx) of gx are padding: written as zeros so that no garbage is ever handed on
      if (col0 + Q - 1 < A.ldgx) {
#pragma unroll
        for (int q = 0; q < Q; ++q)
          if (col0 + q >= Ld.K) v[q] = 0.f;
        *(DCTR_GLOBAL vecq*)(A.gx + b * A.ldgx + col0) = v;
      } else {
        for (int q = 0; q < Q; ++q)
          if (col0 + q < A.ldgx) stg_f32(A.gx + b * A.ldgx + col0 + q, col0 + q < Ld.K ? v[q] : 0.f);
      }
    }
  }
}

// the backward-data pass of one row tile; `g_lds` (nullable): [16] LDS floats holding d loss / d logit of the tile's
// rows (the fused train kernel) instead of A.g; `htop` (nullable): the top layer's output tile still in LDS
// ([16][rs_h], the fused train kernel) instead of its saved copy in global memory
__device__ __forceinline__ void mlp_bwd_body(const MlpArgs& A, float* smem, const float* g_lds, const float* htop,
                                             int rs_h, unsigned long long* tr) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int b0 = blockIdx.x * kTM;
  const int rs = A.rsd;
  float* d0 = smem;
  float* d1 = d0 + kTM * rs;
  const int top = A.n_layers - 1;
  MLP_TRACE(tr, 0);
  {
    // d loss / d pre-activation of the top layer.  Four elements per thread and round trip, every load unconditional
    // from a clamped address (this loop was one round trip per element: 3.5 us for 16 x 128 -- round 3)
    const LayerDev& Lt = A.L[top];
    const int Np = round_up(Lt.N, 16);
    const int n_e = kTM * Np;
    const int64_t blast = A.B - 1;
    for (int e0 = 0; e0 < n_e; e0 += 4 * kT) {
      float gv[4], hv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        int e = e0 + i * kT + tid;
        e = e < n_e ? e : n_e - 1;
        const int r = e / Np, n = e - r * Np;
        const int nn = n < Lt.N ? n : Lt.N - 1;
        const int64_t b = (b0 + r) < blast ? (b0 + r) : blast;
        if (A.w_out) gv[i] = (g_lds ? g_lds[r] : ldg_f32(A.g + b)) * ldg_f32(A.w_out + nn);
        else gv[i] = ldg_f32(A.g + b * A.ldg + nn);
        hv[i] = htop ? htop[r * rs_h + nn] : ldg_f32(Lt.h + b * Lt.ldh + nn);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int e = e0 + i * kT + tid;
        if (e < n_e) {
          const int r = e / Np, n = e - r * Np;
          const int64_t b = b0 + r;
          float v = 0.f;
          if (b < A.B && n < Lt.N) {
            v = gv[i];
            if (Lt.relu) v = hv[i] > 0.f ? v : 0.f;
            if (Lt.dh) stg_f32(Lt.dh + b * Lt.ldh + n, v);
          }
          d0[r * rs + n] = v;
        }
      }
    }
  }
  __syncthreads();
  MLP_TRACE(tr, 1);
  float* din = d0;
  float* dout = d1;
  for (int l = top; l >= 0; --l) {
    const LayerDev& Ld = A.L[l];
    if (l > 0 || A.gx) {
      if (Ld.K <= 32 * kWaves) {
        const int ngroups = (Ld.K + 31) >> 5;
        for (int gb = wv; gb < ngroups; gb += kWaves) bwd_cols<2>(A, l, din, dout, rs, gb, b0, g, c);
      } else {
        const int ngroups = (Ld.K + 63) >> 6;
        for (int gb = wv; gb < ngroups; gb += kWaves) bwd_cols<4>(A, l, din, dout, rs, gb, b0, g, c);
      }
    }
    MLP_TRACE(tr, 2 + 2 * (top - l));
    __syncthreads();
    MLP_TRACE(tr, 3 + 2 * (top - l));
    float* t = din;
    din = dout;
    dout = t;
  }
  MLP_TRACE(tr, 15);
}

// ---- host helpers ---------------------------------------------------------------------------------------------
int check_mlp(const dctr_mlp_t* m, int32_t B) {
  if (!m || B < 0 || m->n_layers <= 0 || m->n_layers > kMaxL) return DCTR_EINVAL;
  for (int l = 0; l < m->n_layers; ++l) {
    const dctr_mlp_layer_t& L = m->layer[l];
    if (!L.W || L.K <= 0 || L.N <= 0 || L.ld_w < L.K) return DCTR_EINVAL;
    if (L.ld_w % 4 != 0 || reinterpret_cast<uintptr_t>(L.W) % 16 != 0) return DCTR_EALIGN;
    if (l > 0 && L.K != m->layer[l - 1].N) return DCTR_EINVAL;
    if (L.N > 2048) return DCTR_ENOSUP;
    if (static_cast<int64_t>(L.N) * L.ld_w * 4 >= (int64_t(1) << 31)) return DCTR_ENOSUP;  // 32-bit weight offsets
  }
  return DCTR_OK;
}

void fill_layers(const dctr_mlp_t* m, LayerDev* L) {
  for (int l = 0; l < m->n_layers; ++l) {
    const dctr_mlp_layer_t& s = m->layer[l];
    L[l].W = s.W; L[l].bias = s.bias; L[l].h = s.h; L[l].dh = s.dh;
    L[l].K = s.K; L[l].N = s.N; L[l].ldw = s.ld_w; L[l].ldh = s.ld_h; L[l].relu = s.relu;
  }
}

int max_width(const dctr_mlp_t* m) {
  int w = 0;
  for (int l = 0; l < m->n_layers; ++l) w = m->layer[l].N > w ? m->layer[l].N : w;
  return w;
}

int check_bwd(const dctr_mlp_t* m, const float* x, int64_t ld_x, int32_t B, const float* gx, int64_t ld_gx) {
  if (!x || ld_x < m->layer[0].K) return DCTR_EINVAL;
  if (gx && (ld_gx < m->layer[0].K)) return DCTR_EINVAL;
  if (gx && (ld_gx % 4 != 0 || reinterpret_cast<uintptr_t>(gx) % 16 != 0)) return DCTR_EALIGN;
  for (int l = 0; l < m->n_layers; ++l) {
    const dctr_mlp_layer_t& L = m->layer[l];
    if (!L.h || !L.dh || L.ld_h < L.N) return DCTR_EINVAL;
    if (L.ld_h % 4 != 0 || reinterpret_cast<uintptr_t>(L.h) % 16 != 0 || reinterpret_cast<uintptr_t>(L.dh) % 16 != 0)
      return DCTR_EALIGN;
    // k_mlp_wgrad addresses its operands with 32-bit byte offsets
    if (static_cast<int64_t>(B) * L.ld_h * 4 >= (int64_t(1) << 32)) return DCTR_ENOSUP;
  }
  if (static_cast<int64_t>(B) * ld_x * 4 >= (int64_t(1) << 32)) return DCTR_ENOSUP;
  return DCTR_OK;
}

// The argument block a launcher starts from: the layers filled, no weight mask, every other field zero or null.  A launcher
// then sets what its kernel reads.
MlpArgs mlp_args(const dctr_mlp_t* m, int32_t B, const float* x, int64_t ld_x) {
  MlpArgs a{};
  fill_layers(m, a.L);
  a.n_layers = m->n_layers; a.B = B; a.x = x; a.ldx = ld_x;
  a.wmask = 0xffffffffu;
  return a;
}

}  // namespace

// ---- the weight gradients (mlp.hip), as every backward entry point launches them ----------------------------------------
namespace dctr {

struct WgradPlan {
  int S, bs, P, pbs;
  int blk0[kMaxL + 2];
  int64_t off_w[kMaxL], off_b[kMaxL], off_o, slab;
};

__attribute__((visibility("hidden"))) WgradPlan plan_wgrad(const dctr_mlp_t* m, int32_t B);

__attribute__((visibility("hidden"))) int launch_wgrad_reduce(const dctr_mlp_t* m, const float* x, int64_t ld_x, int32_t B,
                                                              const float* g, float* workspace, const float* head_loss,
                                                              const float* head_gbias, int n_head, float* loss,
                                                              float* g_bias, const dctr_dense_step_t* step, hipStream_t s);

}  // namespace dctr
