// gru_seq.hip -- the variable-length recurrences of DIEN (reference models/dien.py:181-381 over layers/sequence.py's
// AGRUCell / AUGRUCell / DynamicGRU and torch.nn.GRU on packed sequences) on gfx950: GRU, AIGRU, AGRU and AUGRU over
// [B, T, H] with per-sample lengths read on the device, ONE launch per direction (plus the fixed-order reduction of the
// parameter gradients).  Formulas, addressing and the packed parameter layout: see dctr.h.
//
// A workgroup advances a TILE of samples together, step by step, up to the longest length in the tile.  The weights are
// read from HBM once per workgroup and then live in REGISTERS for the whole sequence:
//   forward   256 threads; thread (unit j, role) holds one row of W_ih and one of W_hh (role r: W_ir | W_hr, z: W_iz | W_hz,
//             n_i: W_in | 0, n_h: 0 | W_hn: the same 2 HP multiply-adds for every role, no divergence) -- 2 HP VGPRs.
//             x_t and h of the tile's samples sit in LDS and are read as broadcasts (every lane of a role the same address).
//   backward  512 threads; thread (column k, slice jq of 8) holds W_ih[g][j][k] and W_hh[g][j][k] for the HP / 8 units j of
//             its slice and the three gates -- 6 HP / 8 VGPRs -- and the gradient of exactly these elements, which it
//             accumulates over every step of every sample it sees, in a fixed order.  The same broadcast LDS read of a
//             pre-activation gradient feeds W^T d (-> dx, dh) and d (x) x (-> dW).
// HP is H rounded up to 16, 32 or 64 (template); padded units carry zero weights and stay exactly 0.
// Between the steps the element-wise work (gates, h', their derivatives) runs one (sample, unit) per thread.
// The forward saves r, z, c and W_hn h + b_hn ([B, T, 4, H]); the backward recomputes nothing.
#include "common.hpp"

using namespace dctr;

namespace {

constexpr int kMaxSeg = 4, kMaxH = 64, kMaxT = 128;
constexpr int kTF = 256, kTB = 512;
constexpr int kGroupsB = 512;          // workgroups of the backward (each leaves kTB / (8 HP) partial rows)
enum { M_GRU = 0, M_AIGRU = 1, M_AGRU = 2, M_AUGRU = 3 };

struct GruArgs {
  const float* X;
  int64_t ldx;
  int B, T, H, mode, nseg;
  int dim[kMaxSeg];
  int64_t xoff[kMaxSeg], xstep[kMaxSeg];
  const int32_t* len;
  const float* att;
  const float* params;
  float* states;                  // fwd
  int64_t lds;
  float* last;
  int64_t ldl;
  float* gates_w;
  const float* states_r;          // bwd (lds is its row stride)
  const float* gates;
  const float* gstates;
  int64_t ldgs;
  const float* glast;
  int64_t ldgl;
  float* gX;
  int64_t ldgx;
  float* gatt;
  float* part;
  int n_params, ntiles;
};

// (constant indices only: a runtime index into an array of the by-value arguments would put the array into scratch)
template <typename V>
__device__ __forceinline__ V pick4(const V (&v)[4], int g) { return g == 0 ? v[0] : g == 1 ? v[1] : g == 2 ? v[2] : v[3]; }

// where element j of position 0 lies inside a row of X, and how far apart two positions are
__device__ __forceinline__ void element_addr(const GruArgs& a, int j, int64_t& addr, int64_t& step) {
  int g = 0, o = j;
#pragma unroll
  for (int u = 0; u < kMaxSeg - 1; ++u)
    if (g == u && u < a.nseg - 1 && o >= a.dim[u]) {
      o -= a.dim[u];
      g = u + 1;
    }
  addr = pick4(a.xoff, g) + o;
  step = pick4(a.xstep, g);
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

__device__ __forceinline__ int clamp_len(const GruArgs& a, int b) {
  if (b >= a.B) return 0;
  const int v = ldg_i32(a.len + b);
  return v < 0 ? 0 : (v > a.T ? a.T : v);
}

template <int HP>
__global__ __launch_bounds__(kTF) void k_gru_fwd(GruArgs a) {
  constexpr int G = kTF / (4 * HP), S = 4, TB = G * S;      // TB == kTF / HP: one (sample, unit) per thread in between
  __shared__ __align__(16) float xs[TB * HP];
  __shared__ __align__(16) float hs[TB * HP];
  __shared__ float gs[TB * 4 * HP];
  __shared__ int nl[TB];
  const int tid = threadIdx.x, H = a.H, T = a.T, mode = a.mode;
  const int j = tid % HP, role = (tid / HP) & 3, grp = tid / (4 * HP), es = tid / HP;

  // this thread's two weight rows and its bias
  float wa[HP], wb[HP], bias = 0.f;
  {
    const float* Wih = a.params;
    const float* Whh = Wih + 3 * H * H;
    const float* bih = Whh + 3 * H * H;
    const float* bhh = bih + 3 * H;
    const bool ua = role < 3 && j < H, ub = role != 2 && j < H;
    const float* ra = Wih + static_cast<int64_t>((role < 3 ? role : 0) * H + (j < H ? j : 0)) * H;
    const float* rb = Whh + static_cast<int64_t>((role == 3 ? 2 : role == 2 ? 0 : role) * H + (j < H ? j : 0)) * H;
#pragma unroll
    for (int k = 0; k < HP; ++k) {
      wa[k] = (ua && k < H) ? ldg_f32(ra + k) : 0.f;
      wb[k] = (ub && k < H) ? ldg_f32(rb + k) : 0.f;
    }
    if (j < H)
      bias = role == 0 ? ldg_f32(bih + j) + ldg_f32(bhh + j)
           : role == 1 ? ldg_f32(bih + H + j) + ldg_f32(bhh + H + j)
           : role == 2 ? ldg_f32(bih + 2 * H + j) : ldg_f32(bhh + 2 * H + j);
  }
  int64_t xaddr, xstp;
  element_addr(a, j < H ? j : 0, xaddr, xstp);

  const int b = blockIdx.x * TB + es;
  const bool live = b < a.B && j < H;
  const int n = clamp_len(a, b);
  if (j == 0) nl[es] = n;
  hs[es * HP + j] = 0.f;
  __syncthreads();
  int nmax = 0;
#pragma unroll
  for (int s = 0; s < TB; ++s) nmax = nl[s] > nmax ? nl[s] : nmax;

  const float* Xb = a.X + static_cast<int64_t>(b < a.B ? b : 0) * a.ldx + xaddr;
  float h = 0.f;
  for (int t = 0; t < nmax; ++t) {
    const bool active = t < n;
    float at = 1.f;
    if (mode != M_GRU && active) at = ldg_f32(a.att + static_cast<int64_t>(b) * T + t);
    float xv = (active && j < H) ? ldg_f32(Xb + t * xstp) : 0.f;
    if (mode == M_AIGRU) xv *= at;
    xs[es * HP + j] = xv;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const f32x4* xr = reinterpret_cast<const f32x4*>(xs + (grp * S + s) * HP);
      const f32x4* hr = reinterpret_cast<const f32x4*>(hs + (grp * S + s) * HP);
      float ax = bias, ah = 0.f;
#pragma unroll
      for (int k4 = 0; k4 < HP / 4; ++k4) {
        const f32x4 x4 = xr[k4], h4 = hr[k4];
        ax = __builtin_fmaf(wa[4 * k4 + 0], x4.x, ax);
        ah = __builtin_fmaf(wb[4 * k4 + 0], h4.x, ah);
        ax = __builtin_fmaf(wa[4 * k4 + 1], x4.y, ax);
        ah = __builtin_fmaf(wb[4 * k4 + 1], h4.y, ah);
        ax = __builtin_fmaf(wa[4 * k4 + 2], x4.z, ax);
        ah = __builtin_fmaf(wb[4 * k4 + 2], h4.z, ah);
        ax = __builtin_fmaf(wa[4 * k4 + 3], x4.w, ax);
        ah = __builtin_fmaf(wb[4 * k4 + 3], h4.w, ah);
      }
      gs[((grp * S + s) * 4 + role) * HP + j] = ax + ah;
    }
    __syncthreads();
    float out = 0.f;
    if (active && j < H) {
      const float* gr = gs + es * 4 * HP + j;
      const float r = sigmoidf_(gr[0]), z = sigmoidf_(gr[HP]), hn = gr[3 * HP];
      const float c = tanhf(gr[2 * HP] + r * hn);
      if (mode == M_GRU || mode == M_AIGRU) {
        h = (1.f - z) * c + z * h;
      } else {
        const float u = mode == M_AGRU ? at : at * z;
        h = (1.f - u) * h + u * c;
      }
      hs[es * HP + j] = h;
      out = h;
      if (a.gates_w) {
        float* gw = a.gates_w + (static_cast<int64_t>(b) * T + t) * 4 * H + j;
        stg_f32(gw, r);
        stg_f32(gw + H, z);
        stg_f32(gw + 2 * H, c);
        stg_f32(gw + 3 * H, hn);
      }
    }
    if (a.states && live) stg_f32(a.states + static_cast<int64_t>(b) * a.lds + static_cast<int64_t>(t) * H + j, out);
  }
  if (live) {
    if (a.states)      // pad_packed_sequence's padding, beyond the tile's longest sample
      for (int t = nmax; t < T; ++t) stg_f32(a.states + static_cast<int64_t>(b) * a.lds + static_cast<int64_t>(t) * H + j, 0.f);
    if (a.last) stg_f32(a.last + static_cast<int64_t>(b) * a.ldl + j, h);
  }
}

// partial rows: part[(workgroup * G + group)][n_params]
template <int HP>
__global__ __launch_bounds__(kTB) void k_gru_bwd(GruArgs a) {
  constexpr int NQ = 8, JR = HP / NQ, G = kTB / (NQ * HP), S = 8, TB = G * S;      // TB == kTB / HP
  __shared__ __align__(16) float dl[TB * 4 * HP];      // d loss / d pre-activation: r, z, n (input side), n (hidden side)
  __shared__ float xs[TB * HP];
  __shared__ float hps[TB * HP];
  __shared__ float prt[TB * NQ * 2 * HP];
  __shared__ int nl[TB];
  const int tid = threadIdx.x, H = a.H, T = a.T, mode = a.mode;
  const int k = tid % HP, jq = (tid / HP) % NQ, grp = tid / (NQ * HP), es = tid / HP, ej = k;

  float wih[3][JR], whh[3][JR], dwih[3][JR], dwhh[3][JR];
  {
    const float* Wih = a.params;
    const float* Whh = Wih + 3 * H * H;
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int jj = 0; jj < JR; ++jj) {
        const int j = jq * JR + jj;
        const bool on = j < H && k < H;
        const int64_t e = static_cast<int64_t>(g * H + (j < H ? j : 0)) * H + (k < H ? k : 0);
        wih[g][jj] = on ? ldg_f32(Wih + e) : 0.f;
        whh[g][jj] = on ? ldg_f32(Whh + e) : 0.f;
        dwih[g][jj] = 0.f;
        dwhh[g][jj] = 0.f;
      }
  }
  int64_t xaddr, xstp;
  element_addr(a, ej < H ? ej : 0, xaddr, xstp);
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int b = tile * TB + es;
    const bool live = b < a.B && ej < H;
    const int n = clamp_len(a, b);
    __syncthreads();
    if (ej == 0) nl[es] = n;
    __syncthreads();
    int nmax = 0;
#pragma unroll
    for (int s = 0; s < TB; ++s) nmax = nl[s] > nmax ? nl[s] : nmax;
    const int64_t bb = b < a.B ? b : 0;
    const float* Xb = a.X + bb * a.ldx + xaddr;
    float* gXb = a.gX + bb * a.ldgx + xaddr;
    const float* Sb = a.states_r + bb * a.lds + ej;
    const float* Gb = a.gates + bb * T * 4 * H + ej;

    // positions beyond the tile's longest sample: zero gradients
    if (live)
      for (int t = nmax; t < T; ++t) stg_f32(gXb + t * xstp, 0.f);
    if (b < a.B && ej == 0 && a.gatt)
      for (int t = nmax; t < T; ++t) stg_f32(a.gatt + bb * T + t, 0.f);

    float dh = 0.f;      // d loss / d h_t arriving from the steps after t
    for (int t = nmax - 1; t >= 0; --t) {
      const bool active = t < n && ej < H;
      float dr = 0.f, dz = 0.f, dni = 0.f, dnh = 0.f, dhd = 0.f, da = 0.f, at = 1.f, xraw = 0.f, xe = 0.f, hp = 0.f;
      if (active) {
        float d = dh;
        if (a.gstates) d += ldg_f32(a.gstates + bb * a.ldgs + static_cast<int64_t>(t) * H + ej);
        if (a.glast && t == n - 1) d += ldg_f32(a.glast + bb * a.ldgl + ej);
        const float* gr = Gb + static_cast<int64_t>(t) * 4 * H;
        const float r = ldg_f32(gr), z = ldg_f32(gr + H), c = ldg_f32(gr + 2 * H), hn = ldg_f32(gr + 3 * H);
        hp = t > 0 ? ldg_f32(Sb + static_cast<int64_t>(t - 1) * H) : 0.f;
        if (mode != M_GRU) at = ldg_f32(a.att + bb * T + t);
        xraw = ldg_f32(Xb + t * xstp);
        xe = mode == M_AIGRU ? at * xraw : xraw;
        float dc, dzz;
        if (mode == M_GRU || mode == M_AIGRU) {      // h' = (1 - z) c + z h
          dc = d * (1.f - z);
          dzz = d * (hp - c);
          dhd = d * z;
        } else if (mode == M_AGRU) {                 // h' = (1 - a) h + a c
          dc = d * at;
          dzz = 0.f;
          da = d * (c - hp);
          dhd = d * (1.f - at);
        } else {                                     // u = a z; h' = (1 - u) h + u c
          const float u = at * z, du = d * (c - hp);
          dc = d * u;
          dzz = du * at;
          da = du * z;
          dhd = d * (1.f - u);
        }
        const float dpc = dc * (1.f - c * c);
        dni = dpc;
        dnh = dpc * r;
        dr = (dpc * hn) * (r * (1.f - r));
        dz = dzz * (z * (1.f - z));
        bsum[0] += dr;
        bsum[1] += dz;
        bsum[2] += dni;
        bsum[3] += dnh;
      }
      float* dle = dl + es * 4 * HP + ej;
      dle[0] = dr;
      dle[HP] = dz;
      dle[2 * HP] = dni;
      dle[3 * HP] = dnh;
      xs[es * HP + ej] = xe;
      hps[es * HP + ej] = hp;
      if (mode == M_AGRU || mode == M_AUGRU) {
        const float tot = group_sum<HP>(da);
        if (ej == 0 && b < a.B) stg_f32(a.gatt + bb * T + t, tot);      // (0 for a sample that ended before t)
      }
      __syncthreads();
#pragma unroll 1      // (unrolled, the scheduler hoists every sample's LDS reads and the registers run out)
      for (int s = 0; s < S; ++s) {
        const int ss = grp * S + s;
        const float xk = xs[ss * HP + k], hk = hps[ss * HP + k];
        const float* dp = dl + ss * 4 * HP + jq * JR;
        float px = 0.f, ph = 0.f;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
          for (int jj = 0; jj < JR; ++jj) {
            const float di = dp[(g < 2 ? g : 2) * HP + jj], dg = g < 2 ? di : dp[3 * HP + jj];
            px = __builtin_fmaf(wih[g][jj], di, px);
            dwih[g][jj] = __builtin_fmaf(di, xk, dwih[g][jj]);
            ph = __builtin_fmaf(whh[g][jj], dg, ph);
            dwhh[g][jj] = __builtin_fmaf(dg, hk, dwhh[g][jj]);
          }
        prt[((ss * NQ + jq) * 2 + 0) * HP + k] = px;
        prt[((ss * NQ + jq) * 2 + 1) * HP + k] = ph;
      }
      __syncthreads();
      {
        float dx = 0.f, dhp = 0.f;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          dx += prt[((es * NQ + q) * 2 + 0) * HP + ej];
          dhp += prt[((es * NQ + q) * 2 + 1) * HP + ej];
        }
        if (active) dh = dhd + dhp;
        if (live) stg_f32(gXb + t * xstp, active ? (mode == M_AIGRU ? at * dx : dx) : 0.f);
        if (mode == M_AIGRU) {
          const float tot = group_sum<HP>(active ? dx * xraw : 0.f);
          if (ej == 0 && b < a.B) stg_f32(a.gatt + bb * T + t, tot);
        }
      }
    }
  }

  // this group's partial row: the weights from their owners, the biases summed over the group's sample slots in order
  float* mine = a.part + static_cast<int64_t>(blockIdx.x * G + grp) * a.n_params;
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int jj = 0; jj < JR; ++jj) {
      const int j = jq * JR + jj;
      if (j < H && k < H) {
        mine[(g * H + j) * H + k] = dwih[g][jj];
        mine[3 * H * H + (g * H + j) * H + k] = dwhh[g][jj];
      }
    }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) dl[(es * 4 + q) * HP + ej] = bsum[q];
  __syncthreads();
  if (jq == 0 && k < H) {
    float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) s4[q] += dl[((grp * S + s) * 4 + q) * HP + k];
    float* bi = mine + 6 * H * H;
    bi[k] = s4[0];
    bi[H + k] = s4[1];
    bi[2 * H + k] = s4[2];
    bi[3 * H + k] = s4[0];
    bi[4 * H + k] = s4[1];
    bi[5 * H + k] = s4[3];
  }
}

// out[i] = sum_g part[g][i] in row order; thread (o, sl) adds the rows sl, sl + 16, ..., slices added in order
__global__ __launch_bounds__(256) void k_gru_reduce(const float* __restrict__ part, int stride, int rows,
                                                    float* __restrict__ out) {
  __shared__ float red[16][17];
  const int o = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + o;
  const int ic = i < stride ? i : 0;
  float s = 0.f;
  for (int g = sl; g < rows; g += 16) s += ldg_f32(part + static_cast<int64_t>(g) * stride + ic);
  red[sl][o] = s;
  __syncthreads();
  if (sl == 0 && i < stride) {
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) t += red[u][o];
    out[i] = t;
  }
}

int hp_of(int H) { return H <= 16 ? 16 : H <= 32 ? 32 : 64; }

// the shape part of the arguments; DCTR_EINVAL / DCTR_ENOSUP / DCTR_OK
int shape(GruArgs& a, int T, int n_seg, const int32_t* dim, int mode) {
  if (T <= 0 || n_seg <= 0 || !dim || mode < 0 || mode > M_AUGRU) return DCTR_EINVAL;
  if (T > kMaxT || n_seg > kMaxSeg) return DCTR_ENOSUP;
  a.T = T; a.nseg = n_seg; a.mode = mode; a.H = 0;
  for (int g = 0; g < n_seg; ++g) {
    if (dim[g] <= 0) return DCTR_EINVAL;
    a.dim[g] = dim[g];
    a.H += dim[g];
    if (a.H > kMaxH) return DCTR_ENOSUP;
  }
  a.n_params = 6 * a.H * a.H + 6 * a.H;
  return DCTR_OK;
}

int fill(GruArgs& a, const float* X, int64_t ld_x, int B, const int64_t* x_off, const int64_t* x_step, const int32_t* len,
         const float* att, const float* params) {
  if (!X || !x_off || !x_step || !len || !params || (a.mode != M_GRU && !att)) return DCTR_EINVAL;
  for (int g = 0; g < a.nseg; ++g) {
    if (x_off[g] < 0 || x_step[g] < a.dim[g] || x_off[g] + (a.T - 1) * x_step[g] + a.dim[g] > ld_x) return DCTR_EINVAL;
    a.xoff[g] = x_off[g]; a.xstep[g] = x_step[g];
  }
  a.X = X; a.ldx = ld_x; a.B = B; a.len = len; a.att = a.mode == M_GRU ? nullptr : att; a.params = params;
  return DCTR_OK;
}

int bwd_groups(int B, int H) {
  const int tb = kTB / hp_of(H), tiles = (B + tb - 1) / tb;
  return tiles < kGroupsB ? tiles : kGroupsB;
}

}  // namespace

extern "C" int dctr_gru_seq_supported(int32_t T, int32_t n_seg, const int32_t* dim, int32_t mode) {
  GruArgs a = {};
  return shape(a, T, n_seg, dim, mode) == DCTR_OK ? 1 : 0;
}

extern "C" size_t dctr_gru_seq_bwd_workspace_floats(int32_t B, int32_t H) {
  if (B <= 0 || H <= 0 || H > kMaxH) return 0;
  return static_cast<size_t>(bwd_groups(B, H)) * (kTB / (8 * hp_of(H))) * (6 * static_cast<size_t>(H) * H + 6 * H);
}

extern "C" int dctr_gru_seq_fwd(const float* X, int64_t ld_x, int32_t B, int32_t T, int32_t n_seg, const int32_t* dim,
                                const int64_t* x_off, const int64_t* x_step, const int32_t* len, const float* att,
                                int32_t mode, const float* params, float* states, int64_t ld_states, float* last,
                                int64_t ld_last, float* gates, dctr_stream_t stream) {
  if (B == 0) return DCTR_OK;
  if (B < 0) return DCTR_EINVAL;
  GruArgs a = {};
  int rc = shape(a, T, n_seg, dim, mode);
  if (rc != DCTR_OK) return rc;
  rc = fill(a, X, ld_x, B, x_off, x_step, len, att, params);
  if (rc != DCTR_OK) return rc;
  if ((!states && !last) || (states && ld_states < static_cast<int64_t>(T) * a.H) || (last && ld_last < a.H))
    return DCTR_EINVAL;
  a.states = states; a.lds = ld_states; a.last = last; a.ldl = ld_last; a.gates_w = gates;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int hp = hp_of(a.H), tb = kTF / hp;
  const dim3 grid((B + tb - 1) / tb), block(kTF);
  if (hp == 16) k_gru_fwd<16><<<grid, block, 0, st>>>(a);
  else if (hp == 32) k_gru_fwd<32><<<grid, block, 0, st>>>(a);
  else k_gru_fwd<64><<<grid, block, 0, st>>>(a);
  return launch_status();
}

extern "C" int dctr_gru_seq_bwd(const float* X, int64_t ld_x, int32_t B, int32_t T, int32_t n_seg, const int32_t* dim,
                                const int64_t* x_off, const int64_t* x_step, const int32_t* len, const float* att,
                                int32_t mode, const float* params, const float* states, int64_t ld_states,
                                const float* gates, const float* g_states, int64_t ld_gstates, const float* g_last,
                                int64_t ld_glast, float* gX, int64_t ld_gx, float* g_att, float* g_params,
                                float* workspace, dctr_stream_t stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  GruArgs a = {};
  if (B < 0) return DCTR_EINVAL;
  if (B == 0) {   // no sample: zero parameter gradients, when the shape says how many there are
    if (g_params && shape(a, T, n_seg, dim, mode) == DCTR_OK)
      (void)hipMemsetAsync(g_params, 0, sizeof(float) * a.n_params, st);
    return DCTR_OK;
  }
  int rc = shape(a, T, n_seg, dim, mode);
  if (rc != DCTR_OK) return rc;
  rc = fill(a, X, ld_x, B, x_off, x_step, len, att, params);
  if (rc != DCTR_OK) return rc;
  if (!states || ld_states < static_cast<int64_t>(T) * a.H || !gates || (!g_states && !g_last) ||
      (g_states && ld_gstates < static_cast<int64_t>(T) * a.H) || (g_last && ld_glast < a.H) || !gX || !g_params ||
      !workspace || (mode != M_GRU && !g_att))
    return DCTR_EINVAL;
  for (int g = 0; g < a.nseg; ++g)
    if (x_off[g] + (a.T - 1) * x_step[g] + a.dim[g] > ld_gx) return DCTR_EINVAL;
  a.states_r = states; a.lds = ld_states; a.gates = gates; a.gstates = g_states; a.ldgs = ld_gstates; a.glast = g_last;
  a.ldgl = ld_glast; a.gX = gX; a.ldgx = ld_gx; a.gatt = mode == M_GRU ? nullptr : g_att; a.part = workspace;
  const int hp = hp_of(a.H), tb = kTB / hp;
  a.ntiles = (B + tb - 1) / tb;
  const int groups = bwd_groups(B, a.H);
  const dim3 grid(groups), block(kTB);
  if (hp == 16) k_gru_bwd<16><<<grid, block, 0, st>>>(a);
  else if (hp == 32) k_gru_bwd<32><<<grid, block, 0, st>>>(a);
  else k_gru_bwd<64><<<grid, block, 0, st>>>(a);
  rc = launch_status();
  if (rc != DCTR_OK) return rc;
  k_gru_reduce<<<dim3((a.n_params + 15) / 16), dim3(256), 0, st>>>(workspace, a.n_params, groups * (kTB / (8 * hp)),
                                                                  g_params);
  return launch_status();
}
