// Light ranker of TwoTowerPlusLightRanker (ref:src/two_tower_plus_light_ranker.py):
//
//   per row / candidate:  s_n = <R_n, v>  (n < NU)   p = softmax(s)   t = sum_n p_n R_n   m = <u, v>
//                         z = [v | t | s | m]  (Z = 2 DI + NU + 1)      logits = W z + b  (T tasks)
//
// Training head (ref :300-340, upstream's torch.cat(dim=2) read as the last axis):
//   loss = mean over B*T of BCE_with_logits(logits, labels), forward and backward, v = the impressed item.
//   Forward: rows kernel (one wavefront per row, lane = one float4 column chunk) keeps z and the logits in the
//   workspace and one double partial of the BCE sum per workgroup; a one-workgroup kernel sums the partials in order.
//   Backward: ONE launch with two kinds of workgroup -- rows (dR, du, dv from dz = W^T dlogit and the softmax's
//   backward) and column blocks of dW | db (fixed row chunks of z^T dlogit, z extended by a column of ones for db) --
//   then one launch that sums the row-chunk partials in order.  No float atomics: two runs give the same bits.
//
// Rerank (ref :155-233): from the MIPS candidates to the top K by  val = (W z + b) . uvw.  Folded once per query:
//   w = W^T uvw, c = <uvw, b>, a_n = <w[DI:2DI], R_n>  so  val = <w_v, row> + sum_n p_n a_n + <w_s, s> + w_m score + c:
//   (NU + 1) dot products of length DI per candidate.  The candidate row is read straight from the corpus by index
//   (fp32, or bf16 widened exactly) or, for a caller's own mips_module, from its dense [B, NI, DI] rows.  Order:
//   value descending, then candidate position (the MIPS rank) ascending; every value maps to a distinct 64-bit key
//   (orderable value bits | inverted position), so the ranks are a permutation and every output slot is written once.
#include <algorithm>

#include "common.hpp"

namespace tt {

constexpr int LR_NU_MAX = 32, LR_T_MAX = 16, LR_DI_MAX = 256, LR_NI_MAX = 4096;
constexpr int LR_ROW_BLOCKS_MAX = 512;  // forward / backward row workgroups (4 rows each per pass)
constexpr int LR_ROW_CHUNK = 256;       // rows per dW partial

static bool lr_sizes_ok(int64_t NU, int64_t DI, int64_t T) {
  return NU >= 1 && NU <= LR_NU_MAX && T >= 1 && T <= LR_T_MAX && DI >= 4 && DI <= LR_DI_MAX && DI % 4 == 0;
}
static inline int64_t lr_Z(int64_t NU, int64_t DI) { return 2 * DI + NU + 1; }
static inline int64_t lr_ldz(int64_t NU, int64_t DI) { return round_up(lr_Z(NU, DI) + 1, 4); }  // + the ones column
static inline int64_t lr_row_blocks(int64_t B) { return std::min<int64_t>(ceil_div(B, 4), LR_ROW_BLOCKS_MAX); }

struct LrWs {  // the head's workspace: forward writes z, logits, loss partials; backward writes the dW partials
  float* z;
  float* logits;
  double* loss_part;
  float* dw_part;
};
static LrWs lr_carve(void* ws, int64_t B, int64_t NU, int64_t DI, int64_t T) {
  Carver cv(ws);
  LrWs w;
  w.z = cv.take<float>(B * lr_ldz(NU, DI));
  w.logits = cv.take<float>(B * T);
  w.loss_part = cv.take<double>(LR_ROW_BLOCKS_MAX);
  w.dw_part = cv.take<float>(ceil_div(B, LR_ROW_CHUNK) * T * (lr_Z(NU, DI) + 1));
  return w;
}
static int64_t lr_ws_bytes(int64_t B, int64_t NU, int64_t DI, int64_t T) {
  return round_up(B * lr_ldz(NU, DI) * 4, 256) + round_up(B * T * 4, 256) + round_up(LR_ROW_BLOCKS_MAX * 8, 256) +
         round_up(ceil_div(B, LR_ROW_CHUNK) * T * (lr_Z(NU, DI) + 1) * 4, 256);
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 fma4(float a, float4 x, float4 y) {
  return make_float4(fmaf(a, x.x, y.x), fmaf(a, x.y, y.y), fmaf(a, x.z, y.z), fmaf(a, x.w, y.w));
}

// p = softmax(s) over the first NU entries (torch's form: shift by the max, divide by the sum)
__device__ __forceinline__ void lr_softmax(const float (&s)[LR_NU_MAX], float (&p)[LR_NU_MAX], int NU) {
  float mx = s[0];
#pragma unroll
  for (int n = 1; n < LR_NU_MAX; ++n)
    if (n < NU) mx = fmaxf(mx, s[n]);
  float sum = 0.f;
#pragma unroll
  for (int n = 0; n < LR_NU_MAX; ++n)
    if (n < NU) { p[n] = expf(s[n] - mx); sum += p[n]; }
  const float inv = 1.f / sum;
#pragma unroll
  for (int n = 0; n < LR_NU_MAX; ++n)
    if (n < NU) p[n] *= inv;
}

// d loss / d logit for one (row, task): the forward's logits, the labels and the incoming scalar gradient
__device__ __forceinline__ float lr_dlogit(float x, float y, float gscale) {
  return gscale * (1.f / (1.f + expf(-x)) - y);
}

// stage W [T, Z] into LDS with row stride ldw (multiple of 4)
__device__ __forceinline__ void lr_stage_w(float* Ws, const float* __restrict__ W, int T, int Z, int ldw) {
  for (int e = threadIdx.x; e < T * ldw; e += blockDim.x) {
    const int t = e / ldw, j = e - t * ldw;
    Ws[e] = j < Z ? W[(int64_t)t * Z + j] : 0.f;
  }
}

// ------------------------------------------------------------------ training head, forward
__global__ __launch_bounds__(256) void lr_head_fwd_kernel(const float* __restrict__ R, int64_t ldR,
                                                          const float* __restrict__ U, int64_t ldu,
                                                          const float* __restrict__ V, int64_t ldv,
                                                          const float* __restrict__ labels, int64_t B, int NU, int DI,
                                                          int T, const float* __restrict__ W,
                                                          const float* __restrict__ bias, float* __restrict__ z,
                                                          int64_t ldz, float* __restrict__ logits,
                                                          double* __restrict__ loss_part) {
  extern __shared__ float lr_smem[];
  const int Z = 2 * DI + NU + 1, ldw = (Z + 3) & ~3;
  float* Ws = lr_smem;                                 // [T, ldw]
  double* wsum = reinterpret_cast<double*>(Ws + T * ldw);  // [4] (ldw % 4 == 0: 16-B aligned)
  lr_stage_w(Ws, W, T, Z, ldw);
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nc = DI >> 2;
  const bool on = lane < nc;
  const int c4 = on ? lane * 4 : 0;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 4 + wv; i < B; i += (int64_t)gridDim.x * 4) {
    const float* Ri = R + i * ldR;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 v = on ? ld4(V + i * ldv + c4) : zero;
    const float4 u = on ? ld4(U + i * ldu + c4) : zero;
    const float m = wave_sum(dot4(u, v));
    float s[LR_NU_MAX], p[LR_NU_MAX];
#pragma unroll
    for (int n = 0; n < LR_NU_MAX; ++n)
      if (n < NU) s[n] = wave_sum(on ? dot4(ld4(Ri + (int64_t)n * DI + c4), v) : 0.f);
    lr_softmax(s, p, NU);
    float4 t4 = zero;
#pragma unroll
    for (int n = 0; n < LR_NU_MAX; ++n)
      if (n < NU && on) t4 = fma4(p[n], ld4(Ri + (int64_t)n * DI + c4), t4);
    float* zi = z + i * ldz;
    if (on) {
      st4(zi + c4, v);
      st4(zi + DI + c4, t4);
    }
    if (lane == 0) {
#pragma unroll
      for (int n = 0; n < LR_NU_MAX; ++n)
        if (n < NU) zi[2 * DI + n] = s[n];
      zi[Z - 1] = m;
      zi[Z] = 1.f;  // the ones column: db is the dW column Z
    }
    float row_loss = 0.f;
    for (int t = 0; t < T; ++t) {
      const float* wt = Ws + t * ldw;
      float part = on ? dot4(ld4(wt + c4), v) + dot4(ld4(wt + DI + c4), t4) : 0.f;
      float x = wave_sum(part);
      float tail = 0.f;
#pragma unroll
      for (int n = 0; n < LR_NU_MAX; ++n)
        if (n < NU) tail = fmaf(wt[2 * DI + n], s[n], tail);
      x += tail + wt[Z - 1] * m + bias[t];
      if (lane == 0) logits[i * T + t] = x;
      const float y = labels[i * T + t];
      row_loss += fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
    }
    acc += (double)row_loss;
  }
  if (lane == 0) wsum[wv] = acc;
  __syncthreads();
  if (threadIdx.x == 0) loss_part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

__global__ __launch_bounds__(64) void lr_loss_reduce_kernel(const double* __restrict__ part, int n, double inv_bt,
                                                            float* __restrict__ loss) {
  if (threadIdx.x != 0) return;
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += part[k];
  *loss = (float)(s * inv_bt);
}

// ------------------------------------------------------------------ training head, backward
// blocks [0, n_row_blocks): rows;  the rest: (column block of 64 of z | 1) x (chunk of LR_ROW_CHUNK rows) dW partials
__global__ __launch_bounds__(256) void lr_head_bwd_kernel(const float* __restrict__ gloss, const float* __restrict__ R,
                                                          int64_t ldR, const float* __restrict__ U, int64_t ldu,
                                                          const float* __restrict__ labels, int64_t B, int NU, int DI,
                                                          int T, const float* __restrict__ W,
                                                          const float* __restrict__ z, int64_t ldz,
                                                          const float* __restrict__ logits, float* __restrict__ dR,
                                                          int64_t lddR, float* __restrict__ dU, int64_t lddu,
                                                          float* __restrict__ dV, int64_t lddv,
                                                          float* __restrict__ dw_part, int n_row_blocks) {
  extern __shared__ float lr_smem[];
  const int Z = 2 * DI + NU + 1;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float gscale = gloss[0] / (float)((double)B * (double)T);
  if ((int)blockIdx.x >= n_row_blocks) {
    // ---- dW | db partial: column j of the extended z, rows [r0, r1), T accumulators per lane
    const int ncb = (Z + 1 + 63) / 64;
    const int q = blockIdx.x - n_row_blocks;
    const int cb = q % ncb, chunk = q / ncb;
    const int j = cb * 64 + lane;
    const int64_t r0 = (int64_t)chunk * LR_ROW_CHUNK, r1 = std::min<int64_t>(r0 + LR_ROW_CHUNK, B);
    float acc[LR_T_MAX];
#pragma unroll
    for (int t = 0; t < LR_T_MAX; ++t) acc[t] = 0.f;
    for (int64_t i = r0 + wv; i < r1; i += 4) {
      const float zj = j <= Z ? z[i * ldz + j] : 0.f;
#pragma unroll
      for (int t = 0; t < LR_T_MAX; ++t)
        if (t < T) acc[t] = fmaf(lr_dlogit(logits[i * T + t], labels[i * T + t], gscale), zj, acc[t]);
    }
    float* red = lr_smem;  // [4][T_MAX][64]
#pragma unroll
    for (int t = 0; t < LR_T_MAX; ++t)
      if (t < T) red[(wv * LR_T_MAX + t) * 64 + lane] = acc[t];
    __syncthreads();
    for (int e = threadIdx.x; e < T * 64; e += blockDim.x) {
      const int t = e >> 6, l = e & 63, jj = cb * 64 + l;
      const float s = ((red[(0 * LR_T_MAX + t) * 64 + l] + red[(1 * LR_T_MAX + t) * 64 + l]) +
                       red[(2 * LR_T_MAX + t) * 64 + l]) + red[(3 * LR_T_MAX + t) * 64 + l];
      if (jj <= Z) dw_part[((int64_t)chunk * T + t) * (Z + 1) + jj] = s;
    }
    return;
  }
  // ---- rows
  const int ldw = (Z + 3) & ~3;
  float* Ws = lr_smem;
  lr_stage_w(Ws, W, T, Z, ldw);
  __syncthreads();
  const int nc = DI >> 2;
  const bool on = lane < nc;
  const int c4 = on ? lane * 4 : 0;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = (int64_t)blockIdx.x * 4 + wv; i < B; i += (int64_t)n_row_blocks * 4) {
    const float* Ri = R + i * ldR;
    const float* zi = z + i * ldz;
    const float4 v = on ? ld4(zi + c4) : zero;  // z[:, :DI] is v
    const float4 u = on ? ld4(U + i * ldu + c4) : zero;
    float s[LR_NU_MAX], p[LR_NU_MAX], ds[LR_NU_MAX];
#pragma unroll
    for (int n = 0; n < LR_NU_MAX; ++n)
      if (n < NU) { s[n] = zi[2 * DI + n]; ds[n] = 0.f; }
    lr_softmax(s, p, NU);
    // dz = W^T dlogit
    float4 dzv = zero, dt = zero;
    float dm = 0.f;
    for (int t = 0; t < T; ++t) {
      const float g = lr_dlogit(logits[i * T + t], labels[i * T + t], gscale);
      const float* wt = Ws + t * ldw;
      if (on) {
        dzv = fma4(g, ld4(wt + c4), dzv);
        dt = fma4(g, ld4(wt + DI + c4), dt);
      }
#pragma unroll
      for (int n = 0; n < LR_NU_MAX; ++n)
        if (n < NU) ds[n] = fmaf(g, wt[2 * DI + n], ds[n]);
      dm = fmaf(g, wt[Z - 1], dm);
    }
    // t = sum p_n R_n:  dp_n = <R_n, dt>;  softmax backward: ds_n += p_n (dp_n - sum_k p_k dp_k)
    float dp[LR_NU_MAX];
    float pdp = 0.f;
#pragma unroll
    for (int n = 0; n < LR_NU_MAX; ++n)
      if (n < NU) {
        dp[n] = wave_sum(on ? dot4(ld4(Ri + (int64_t)n * DI + c4), dt) : 0.f);
        pdp = fmaf(p[n], dp[n], pdp);
      }
#pragma unroll
    for (int n = 0; n < LR_NU_MAX; ++n)
      if (n < NU) ds[n] = fmaf(p[n], dp[n] - pdp, ds[n]);
    // s_n = <R_n, v>: dR_n = p_n dt + ds_n v, dv += ds_n R_n;  m = <u, v>: du = dm v, dv += dm u
    float4 dv = fma4(dm, u, dzv);
    if (on) {
#pragma unroll
      for (int n = 0; n < LR_NU_MAX; ++n)
        if (n < NU) {
          const float4 r = ld4(Ri + (int64_t)n * DI + c4);
          float4 d = make_float4(p[n] * dt.x, p[n] * dt.y, p[n] * dt.z, p[n] * dt.w);
          st4(dR + i * lddR + (int64_t)n * DI + c4, fma4(ds[n], v, d));
          dv = fma4(ds[n], r, dv);
        }
      st4(dV + i * lddv + c4, dv);
      st4(dU + i * lddu + c4, make_float4(dm * v.x, dm * v.y, dm * v.z, dm * v.w));
    }
  }
}

__global__ __launch_bounds__(256) void lr_dw_reduce_kernel(const float* __restrict__ part, int n_chunks, int T, int Z,
                                                           float* __restrict__ dW, float* __restrict__ db) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= T * (Z + 1)) return;
  const int t = e / (Z + 1), j = e - t * (Z + 1);
  double s = 0.0;
  for (int k = 0; k < n_chunks; ++k) s += (double)part[((int64_t)k * T + t) * (Z + 1) + j];
  if (j < Z) dW[(int64_t)t * Z + j] = (float)s;
  else db[t] = (float)s;
}

// ------------------------------------------------------------------ rerank
__device__ __forceinline__ float4 lr_load_row4(const void* corpus, int dtype, int64_t row, int DI, int c4) {
  if (dtype == TT_BF16) {
    const uint2 w = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(corpus) + row * DI + c4);
    return make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                       __uint_as_float(w.y & 0xffff0000u));
  }
  return ld4(reinterpret_cast<const float*>(corpus) + row * DI + c4);
}

__device__ __forceinline__ uint64_t lr_key(float val, int j) {
  uint32_t b = __float_as_uint(val + 0.f);  // -0 -> +0: equal values, equal keys
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | (uint32_t)(0xffffffffu - (uint32_t)j);
}

// one workgroup per query; 16-lane groups score one candidate each
__global__ __launch_bounds__(256) void lr_rerank_kernel(const void* __restrict__ corpus, int dtype, int64_t C,
                                                        const int64_t* __restrict__ idx,
                                                        const float* __restrict__ rows,
                                                        const float* __restrict__ scores, int NI, int K,
                                                        const float* __restrict__ R, int64_t ldR, int NU, int DI,
                                                        const float* __restrict__ W, const float* __restrict__ bias,
                                                        const float* __restrict__ uvw, int T,
                                                        int64_t* __restrict__ out_ids, float* __restrict__ out_vals,
                                                        int32_t* __restrict__ oob_flag) {
  extern __shared__ float lr_smem[];
  const int Z = 2 * DI + NU + 1;
  const int64_t b = blockIdx.x;
  uint64_t* keys = reinterpret_cast<uint64_t*>(lr_smem);  // [NI]
  float* Rs = lr_smem + ((2 * NI + 3) & ~3);               // [NU, DI], 16-B aligned
  float* wf = Rs + NU * DI;                                // [Z] = W^T uvw
  float* an = wf + ((Z + 3) & ~3);                         // [NU] then c at an[LR_NU_MAX]
  const float* Rb = R + b * ldR;
  for (int e = threadIdx.x; e < NU * DI; e += blockDim.x) Rs[e] = Rb[e];
  for (int j = threadIdx.x; j < Z; j += blockDim.x) {
    float s = 0.f;
    for (int t = 0; t < T; ++t) s = fmaf(uvw[t], W[(int64_t)t * Z + j], s);
    wf[j] = s;
  }
  if (threadIdx.x == 0) {
    float c = 0.f;
    for (int t = 0; t < T; ++t) c = fmaf(uvw[t], bias[t], c);
    an[LR_NU_MAX] = c;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int n = wv; n < NU; n += 4) {
    float s = 0.f;
    for (int k = lane; k < DI; k += 64) s = fmaf(wf[DI + k], Rs[n * DI + k], s);
    s = wave_sum(s);
    if (lane == 0) an[n] = s;
  }
  __syncthreads();
  const float cst = an[LR_NU_MAX], wm = wf[Z - 1];
  const int gl = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int nc = DI >> 2;
  bool bad = false;
  for (int j = grp; j < NI; j += 16) {
    const int64_t cand = b * NI + j;
    float s[LR_NU_MAX];
#pragma unroll
    for (int n = 0; n < LR_NU_MAX; ++n) s[n] = 0.f;
    float dv = 0.f;
    int64_t row = idx[cand];
    const bool valid = rows != nullptr || (row >= 0 && row < C);
    bad |= !valid;
    if (valid) {
      for (int c = gl; c < nc; c += 16) {
        const float4 x = rows != nullptr ? ld4(rows + cand * DI + c * 4) : lr_load_row4(corpus, dtype, row, DI, c * 4);
        dv += dot4(ld4(wf + c * 4), x);
#pragma unroll
        for (int n = 0; n < LR_NU_MAX; ++n)
          if (n < NU) s[n] += dot4(ld4(Rs + n * DI + c * 4), x);
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      dv += __shfl_xor(dv, o, 64);
#pragma unroll
      for (int n = 0; n < LR_NU_MAX; ++n)
        if (n < NU) s[n] += __shfl_xor(s[n], o, 64);
    }
    float p[LR_NU_MAX];
    lr_softmax(s, p, NU);
    float val = dv;
#pragma unroll
    for (int n = 0; n < LR_NU_MAX; ++n)
      if (n < NU) val += p[n] * an[n] + wf[2 * DI + n] * s[n];
    val += wm * scores[cand] + cst;
    if (gl == 0) {
      keys[j] = lr_key(val, j);
      if (out_vals != nullptr) out_vals[cand] = val;
    }
  }
  if (bad) *oob_flag = 1;
  __syncthreads();
  // rank = number of larger keys (keys are distinct): the ranks are a permutation of [0, NI)
  for (int j = threadIdx.x; j < NI; j += blockDim.x) {
    const uint64_t kj = keys[j];
    int rank = 0;
    for (int i = 0; i < NI; ++i) rank += keys[i] > kj;
    if (rank < K) out_ids[b * K + rank] = idx[b * NI + j];
  }
}

static size_t lr_rerank_lds(int64_t NI, int64_t NU, int64_t DI) {
  return (size_t)(round_up(2 * NI, 4) + NU * DI + round_up(lr_Z(NU, DI), 4) + LR_NU_MAX + 4) * 4;
}

}  // namespace tt

using namespace tt;

extern "C" int tt_light_ranker_supported(int64_t NU, int64_t DI, int64_t T) { return lr_sizes_ok(NU, DI, T) ? 1 : 0; }

extern "C" int64_t tt_light_ranker_head_workspace_bytes(int64_t B, int64_t NU, int64_t DI, int64_t T) {
  if (B < 1 || !lr_sizes_ok(NU, DI, T)) return 0;
  return lr_ws_bytes(B, NU, DI, T);
}

static int lr_check_vec(const float* p, int64_t ld, int64_t need, const char* what) {
  if (p == nullptr) return fail_arg(what);
  if (ld < need || ld % 4 != 0 || (reinterpret_cast<uintptr_t>(p) & 15) != 0) {
    set_error("bad argument: %s must be 16-byte aligned with a row stride >= %lld and a multiple of 4", what,
              (long long)need);
    return TT_E_BADARG;
  }
  return 0;
}

static int lr_head_args(const float* R, int64_t ldR, const float* u, int64_t ldu, const float* v, int64_t ldv,
                        const float* labels, int64_t B, int64_t NU, int64_t DI, int64_t T, const float* W,
                        const void* ws, int64_t ws_bytes) {
  if (B < 1) return fail_arg("B < 1");
  if (!lr_sizes_ok(NU, DI, T)) return fail_arg("light ranker sizes: need 1 <= NU <= 32, 1 <= T <= 16, DI % 4 == 0, 4 <= DI <= 256");
  if (labels == nullptr || W == nullptr || ws == nullptr) return fail_arg("null pointer");
  int rc;
  if ((rc = lr_check_vec(R, ldR, NU * DI, "R")) || (rc = lr_check_vec(u, ldu, DI, "u")) ||
      (rc = lr_check_vec(v, ldv, DI, "v")))
    return rc;
  if (ws_bytes < lr_ws_bytes(B, NU, DI, T)) {
    set_error("light ranker head: workspace %lld < %lld bytes", (long long)ws_bytes, (long long)lr_ws_bytes(B, NU, DI, T));
    return TT_E_WORKSPACE;
  }
  return 0;
}

extern "C" int tt_light_ranker_head_fwd(const float* R, int64_t ldR, const float* u, int64_t ldu, const float* v,
                                        int64_t ldv, const float* labels, int64_t B, int64_t NU, int64_t DI, int64_t T,
                                        const float* W, const float* bias, float* loss, void* ws, int64_t ws_bytes,
                                        tt_stream_t stream) {
  if (bias == nullptr || loss == nullptr) return fail_arg("null pointer");
  if (int rc = lr_head_args(R, ldR, u, ldu, v, ldv, labels, B, NU, DI, T, W, ws, ws_bytes)) return rc;
  LrWs w = lr_carve(ws, B, NU, DI, T);
  const int64_t Z = lr_Z(NU, DI), ldw = round_up(Z, 4);
  const int G = (int)lr_row_blocks(B);
  const size_t lds = (size_t)T * ldw * 4 + 4 * 8;
  {
    ProfScope ps("lr_head_fwd_kernel", S(stream));
    hipLaunchKernelGGL(lr_head_fwd_kernel, dim3(G), dim3(256), lds, S(stream), R, ldR, u, ldu, v, ldv, labels, B,
                       (int)NU, (int)DI, (int)T, W, bias, w.z, lr_ldz(NU, DI), w.logits, w.loss_part);
  }
  if (int rc = check_launch("lr_head_fwd_kernel")) return rc;
  hipLaunchKernelGGL(lr_loss_reduce_kernel, dim3(1), dim3(64), 0, S(stream), w.loss_part, G, 1.0 / ((double)B * T), loss);
  return check_launch("lr_loss_reduce_kernel");
}

extern "C" int tt_light_ranker_head_bwd(const float* grad_loss, const float* R, int64_t ldR, const float* u,
                                        int64_t ldu, const float* v, int64_t ldv, const float* labels, int64_t B,
                                        int64_t NU, int64_t DI, int64_t T, const float* W, void* ws, int64_t ws_bytes,
                                        float* dR, int64_t lddR, float* du, int64_t lddu, float* dv, int64_t lddv,
                                        float* dW, float* db, tt_stream_t stream) {
  if (grad_loss == nullptr || dW == nullptr || db == nullptr) return fail_arg("null pointer");
  if (int rc = lr_head_args(R, ldR, u, ldu, v, ldv, labels, B, NU, DI, T, W, ws, ws_bytes)) return rc;
  int rc;
  if ((rc = lr_check_vec(dR, lddR, NU * DI, "dR")) || (rc = lr_check_vec(du, lddu, DI, "du")) ||
      (rc = lr_check_vec(dv, lddv, DI, "dv")))
    return rc;
  LrWs w = lr_carve(ws, B, NU, DI, T);
  const int64_t Z = lr_Z(NU, DI), ldw = round_up(Z, 4);
  const int G = (int)lr_row_blocks(B);
  const int64_t n_chunks = ceil_div(B, LR_ROW_CHUNK), ncb = ceil_div(Z + 1, 64);
  const size_t lds = std::max<size_t>((size_t)T * ldw * 4, (size_t)4 * LR_T_MAX * 64 * 4);
  {
    ProfScope ps("lr_head_bwd_kernel", S(stream));
    hipLaunchKernelGGL(lr_head_bwd_kernel, dim3((unsigned)(G + n_chunks * ncb)), dim3(256), lds, S(stream), grad_loss,
                       R, ldR, u, ldu, labels, B, (int)NU, (int)DI, (int)T, W, w.z, lr_ldz(NU, DI), w.logits, dR,
                       lddR, du, lddu, dv, lddv, w.dw_part, G);
  }
  if (int rc2 = check_launch("lr_head_bwd_kernel")) return rc2;
  const int n = (int)(T * (Z + 1));
  hipLaunchKernelGGL(lr_dw_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, S(stream), w.dw_part, (int)n_chunks,
                     (int)T, (int)Z, dW, db);
  return check_launch("lr_dw_reduce_kernel");
}

extern "C" int tt_light_ranker_rerank(const void* corpus, int dtype, int64_t C, const int64_t* idx, const float* rows,
                                      const float* scores, int64_t B, int64_t NI, int64_t K, const float* R, int64_t ldR,
                                      int64_t NU, int64_t DI, const float* W, const float* bias, const float* uvw,
                                      int64_t T, int64_t* out_ids, float* out_vals, int32_t* oob_flag,
                                      tt_stream_t stream) {
  if (B < 1) return fail_arg("B < 1");
  if (!lr_sizes_ok(NU, DI, T)) return fail_arg("light ranker sizes: need 1 <= NU <= 32, 1 <= T <= 16, DI % 4 == 0, 4 <= DI <= 256");
  if (NI < 1 || NI > LR_NI_MAX) return fail_arg("num_mips_items must be in [1, 4096]");
  if (K < 1 || K > NI) return fail_arg("K must be in [1, num_mips_items]");
  if (idx == nullptr || scores == nullptr || W == nullptr || bias == nullptr || uvw == nullptr || out_ids == nullptr ||
      oob_flag == nullptr)
    return fail_arg("null pointer");
  if ((corpus == nullptr) == (rows == nullptr)) return fail_arg("exactly one of corpus / rows must be given");
  if (corpus != nullptr) {
    if (dtype != TT_F32 && dtype != TT_BF16) return fail_arg("corpus dtype must be TT_F32 or TT_BF16");
    if (C < 1) return fail_arg("C < 1");
    if ((reinterpret_cast<uintptr_t>(corpus) & (dtype == TT_BF16 ? 7 : 15)) != 0) return fail_arg("corpus alignment");
  } else if ((reinterpret_cast<uintptr_t>(rows) & 15) != 0) {
    return fail_arg("rows alignment");
  }
  if (R == nullptr || ldR < NU * DI) return fail_arg("R");
  const size_t lds = lr_rerank_lds(NI, NU, DI);
  {
    ProfScope ps("lr_rerank_kernel", S(stream));
    hipLaunchKernelGGL(lr_rerank_kernel, dim3((unsigned)B), dim3(256), lds, S(stream), corpus, dtype, C, idx, rows,
                       scores, (int)NI, (int)K, R, ldR, (int)NU, (int)DI, W, bias, uvw, (int)T, out_ids, out_vals,
                       oob_flag);
  }
  return check_launch("lr_rerank_kernel");
}
