// Row L2-normalisation with an optional learned scale: the op between the towers and the in-batch softmax CE that turns
// its dot-product logits into cos(u, v) / tau without touching a logits kernel (DESIGN.md "Cosine logits").
//
//   forward    inv[r] = 1 / max(||x_r||, eps);  y_r = (s * inv[r]) * x_r,  s = exp(*log_scale) (device word; NULL: s = 1)
//   backward   n = x_r * inv[r];  t = <n, dy_r>
//              ||x_r|| >  eps:  dx_r = (s * inv[r]) * (dy_r - n * t)
//              ||x_r|| <= eps:  dx_r = (s / eps) * dy_r                       (y is linear in x there)
//              d_log_scale = sum_r <dy_r, y_r> = sum_r s * t                 (y_r = s * n on both branches)
//
//   one wave per row, L2N_ROWS_PER_WG rows per 256-thread workgroup; one launch covers one or two operands ("sides": the
//   user rows, scaled, and the item rows, unscaled), a workgroup finds its side from its index;
//   vector form (16-byte aligned bases, ld % 4 == 0, D % 4 == 0; chosen per side): one float4 per lane and 256 columns per
//   trip -- for D <= 256 the row stays in that float4 between the reduction and the scaling, so x is read once;
//   scalar form for everything else (any D >= 1, any alignment);
//   the row reduction is the __shfl_xor butterfly (common.hpp wave_sum): every lane ends with the same sum, formed in the
//   same order, so no broadcast follows it;
//   d_log_scale: every workgroup stores the sum of its rows' s * t (wave order) to partials[workgroup]; a second launch of
//   ONE workgroup per side sums the side's partials -- thread j takes partials j, j + 256, ... in that order, then a fixed
//   tree over the 256 threads -- and WRITES the result.  No atomics of any kind, no counter to reset: the value is the same
//   bits run to run and under graph replay.  d_log_scale == NULL on every side: no partial is stored and the second launch
//   is not made.
#include <cmath>

#include "common.hpp"

namespace tt {

constexpr int L2N_THREADS = 256;
constexpr int L2N_ROWS_PER_WG = L2N_THREADS / WAVE;  // 4
constexpr int L2N_FINISH_THREADS = 256;              // partials one pass of the finishing workgroup takes

struct L2nFwdArgs {
  tt_l2norm_fwd_side s[2];
  int64_t wg0;  // workgroups of side 0 (side 1's follow)
  int vec[2];
};
struct L2nBwdArgs {
  tt_l2norm_bwd_side s[2];
  int64_t wg0;
  int vec[2];
  float* partials[2];  // NULL: the side has no d_log_scale
  int64_t n_partials[2];
};

__device__ __forceinline__ float l2n_scale(const float* log_scale) { return log_scale ? expf(*log_scale) : 1.0f; }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__global__ __launch_bounds__(L2N_THREADS) void l2norm_fwd_kernel(L2nFwdArgs a, int64_t D, float eps, float inv_eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t wg = blockIdx.x;
  const int sd = wg >= a.wg0 ? 1 : 0;
  if (sd) wg -= a.wg0;
  const tt_l2norm_fwd_side sp = a.s[sd];
  const int64_t r = wg * L2N_ROWS_PER_WG + wave;
  if (r >= sp.rows) return;  // (wave-uniform; nothing below crosses waves)
  const float* x = sp.x + r * sp.ldx;
  float* y = sp.y + r * sp.ldy;
  const float s = l2n_scale(sp.log_scale);
  if (a.vec[sd]) {
    const int64_t c0 = (int64_t)lane * 4;
    if (D <= 4 * WAVE) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c0 < D) v = ld4(x + c0);
      const float norm = sqrtf(wave_sum(dot4(v, v)));
      const float inv = norm > eps ? 1.0f / norm : inv_eps;
      const float c = s * inv;
      if (c0 < D) st4(y + c0, make_float4(c * v.x, c * v.y, c * v.z, c * v.w));
      if (lane == 0) sp.inv[r] = inv;
      return;
    }
    float ss = 0.f;
    for (int64_t c4 = c0; c4 < D; c4 += 4 * WAVE) {
      const float4 v = ld4(x + c4);
      ss += dot4(v, v);
    }
    const float norm = sqrtf(wave_sum(ss));
    const float inv = norm > eps ? 1.0f / norm : inv_eps;
    const float c = s * inv;
    for (int64_t c4 = c0; c4 < D; c4 += 4 * WAVE) {
      const float4 v = ld4(x + c4);
      st4(y + c4, make_float4(c * v.x, c * v.y, c * v.z, c * v.w));
    }
    if (lane == 0) sp.inv[r] = inv;
    return;
  }
  float ss = 0.f;
  for (int64_t j = lane; j < D; j += WAVE) ss += x[j] * x[j];
  const float norm = sqrtf(wave_sum(ss));
  const float inv = norm > eps ? 1.0f / norm : inv_eps;
  const float c = s * inv;
  for (int64_t j = lane; j < D; j += WAVE) y[j] = c * x[j];
  if (lane == 0) sp.inv[r] = inv;
}

__global__ __launch_bounds__(L2N_THREADS) void l2norm_bwd_kernel(L2nBwdArgs a, int64_t D, float inv_eps) {
  __shared__ float wave_part[L2N_ROWS_PER_WG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t wg = blockIdx.x;
  const int sd = wg >= a.wg0 ? 1 : 0;
  if (sd) wg -= a.wg0;
  const tt_l2norm_bwd_side sp = a.s[sd];
  float* partials = a.partials[sd];
  const int64_t r = wg * L2N_ROWS_PER_WG + wave;
  float mine = 0.f;  // this row's s * <n, dy>
  if (r < sp.rows) {
    const float* x = sp.x + r * sp.ldx;
    const float* dy = sp.dy + r * sp.lddy;
    float* dx = sp.dx + r * sp.lddx;
    const float s = l2n_scale(sp.log_scale);
    const float inv = sp.inv[r];
    const float c = s * inv;
    const bool clamped = !(inv < inv_eps);  // the forward stored exactly 1 / eps for ||x|| <= eps
    if (a.vec[sd]) {
      const int64_t c0 = (int64_t)lane * 4;
      if (D <= 4 * WAVE) {
        float4 n = make_float4(0.f, 0.f, 0.f, 0.f), g = n;
        if (c0 < D) {
          const float4 v = ld4(x + c0);
          n = make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
          g = ld4(dy + c0);
        }
        const float t = wave_sum(dot4(n, g));
        const float p = clamped ? 0.f : t;
        if (c0 < D) st4(dx + c0, make_float4(c * (g.x - n.x * p), c * (g.y - n.y * p), c * (g.z - n.z * p), c * (g.w - n.w * p)));
        mine = s * t;
      } else {
        float acc = 0.f;
        for (int64_t c4 = c0; c4 < D; c4 += 4 * WAVE) {
          const float4 v = ld4(x + c4), g = ld4(dy + c4);
          acc += dot4(make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv), g);
        }
        const float t = wave_sum(acc);
        const float p = clamped ? 0.f : t;
        for (int64_t c4 = c0; c4 < D; c4 += 4 * WAVE) {
          const float4 v = ld4(x + c4), g = ld4(dy + c4);
          st4(dx + c4, make_float4(c * (g.x - (v.x * inv) * p), c * (g.y - (v.y * inv) * p), c * (g.z - (v.z * inv) * p),
                                   c * (g.w - (v.w * inv) * p)));
        }
        mine = s * t;
      }
    } else {
      float acc = 0.f;
      for (int64_t j = lane; j < D; j += WAVE) acc += (x[j] * inv) * dy[j];
      const float t = wave_sum(acc);
      const float p = clamped ? 0.f : t;
      for (int64_t j = lane; j < D; j += WAVE) dx[j] = c * (dy[j] - (x[j] * inv) * p);
      mine = s * t;
    }
  }
  if (partials == nullptr) return;  // (uniform over the workgroup)
  if (lane == 0) wave_part[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    float sum = wave_part[0];
#pragma unroll
    for (int w = 1; w < L2N_ROWS_PER_WG; ++w) sum += wave_part[w];
    partials[wg] = sum;
  }
}

// one workgroup per side with a d_log_scale: out = sum of the side's partials in a fixed order, written (not accumulated)
__global__ __launch_bounds__(L2N_FINISH_THREADS) void l2norm_finish_kernel(L2nBwdArgs a) {
  __shared__ float red[L2N_FINISH_THREADS];
  int sd = blockIdx.x;
  if (a.partials[0] == nullptr) sd = 1;  // (the launch has one workgroup per side that asked)
  const float* partials = a.partials[sd];
  const int64_t n = a.n_partials[sd];
  float acc = 0.f;
  for (int64_t j = threadIdx.x; j < n; j += L2N_FINISH_THREADS) acc += partials[j];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int h = L2N_FINISH_THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *a.s[sd].d_log_scale = red[0];
}

inline bool l2n_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int64_t l2n_workgroups(int64_t rows) { return ceil_div(rows, L2N_ROWS_PER_WG); }

inline const char* l2n_check_common(const void* sides, int32_t n_sides, int64_t D, float eps) {
  if (!sides) return "null side array";
  if (n_sides < 1 || n_sides > 2) return "n_sides must be 1 or 2";
  if (D < 1) return "D < 1";
  if (!(eps > 0.f) || !std::isfinite(eps) || !std::isfinite(1.0f / eps)) return "eps must be positive and finite, with a finite reciprocal";
  return nullptr;
}

}  // namespace tt

using namespace tt;

extern "C" int64_t tt_l2norm_bwd_workspace_bytes(int64_t rows) {
  if (rows <= 0) return 0;
  return round_up(l2n_workgroups(rows) * (int64_t)sizeof(float), 256);
}

extern "C" int tt_l2norm_fwd(const tt_l2norm_fwd_side* sides, int32_t n_sides, int64_t D, float eps, tt_stream_t stream) {
  if (const char* why = l2n_check_common(sides, n_sides, D, eps)) {
    set_error("bad argument: tt_l2norm_fwd: %s", why);
    return TT_E_BADARG;
  }
  L2nFwdArgs a = {};
  int64_t total = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_l2norm_fwd_side& s = sides[i];
    if (s.rows < 0) return fail_arg("tt_l2norm_fwd: rows < 0");
    if (s.ldx < D || s.ldy < D) return fail_arg("tt_l2norm_fwd: ld < D");
    if (s.rows > 0 && (!s.x || !s.y || !s.inv)) return fail_arg("tt_l2norm_fwd: null x / y / inv");
    a.s[i] = s;
    a.vec[i] = D % 4 == 0 && s.ldx % 4 == 0 && s.ldy % 4 == 0 && l2n_aligned16(s.x) && l2n_aligned16(s.y);
    if (i == 0) a.wg0 = l2n_workgroups(s.rows);
    total += l2n_workgroups(s.rows);
  }
  if (total >= (1ll << 31)) return fail_arg("tt_l2norm_fwd: rows (at most 2^33 over both sides)");
  if (total == 0) return 0;
  hipStream_t st = S(stream);
  ProfScope prof("l2norm_fwd_kernel", st);
  l2norm_fwd_kernel<<<(unsigned)total, L2N_THREADS, 0, st>>>(a, D, eps, 1.0f / eps);
  return check_launch("l2norm_fwd_kernel");
}

extern "C" int tt_l2norm_bwd(const tt_l2norm_bwd_side* sides, int32_t n_sides, int64_t D, float eps, void* ws, int64_t ws_bytes,
                             tt_stream_t stream) {
  if (const char* why = l2n_check_common(sides, n_sides, D, eps)) {
    set_error("bad argument: tt_l2norm_bwd: %s", why);
    return TT_E_BADARG;
  }
  L2nBwdArgs a = {};
  int64_t total = 0, need = 0;
  int n_finish = 0;
  for (int i = 0; i < n_sides; ++i) {
    const tt_l2norm_bwd_side& s = sides[i];
    if (s.rows < 0) return fail_arg("tt_l2norm_bwd: rows < 0");
    if (s.ldx < D || s.lddy < D || s.lddx < D) return fail_arg("tt_l2norm_bwd: ld < D");
    if (s.rows > 0 && (!s.x || !s.dy || !s.inv || !s.dx)) return fail_arg("tt_l2norm_bwd: null x / dy / inv / dx");
    if (s.d_log_scale) {
      need += tt_l2norm_bwd_workspace_bytes(s.rows);
      ++n_finish;
    }
    total += l2n_workgroups(s.rows);
  }
  if (total >= (1ll << 31)) return fail_arg("tt_l2norm_bwd: rows (at most 2^33 over both sides)");
  if (need > 0 && (!ws || ws_bytes < need)) {
    set_error("bad argument: tt_l2norm_bwd: workspace of %lld bytes, needs %lld (tt_l2norm_bwd_workspace_bytes per side with a "
              "d_log_scale)", (long long)(ws ? ws_bytes : 0), (long long)need);
    return TT_E_BADARG;
  }
  Carver carve(ws);
  for (int i = 0; i < n_sides; ++i) {
    const tt_l2norm_bwd_side& s = sides[i];
    a.s[i] = s;
    a.vec[i] = D % 4 == 0 && s.ldx % 4 == 0 && s.lddy % 4 == 0 && s.lddx % 4 == 0 && l2n_aligned16(s.x) && l2n_aligned16(s.dy) &&
               l2n_aligned16(s.dx);
    if (i == 0) a.wg0 = l2n_workgroups(s.rows);
    if (s.d_log_scale) {
      a.n_partials[i] = l2n_workgroups(s.rows);
      // (a side without rows still gets its zero written: a non-null marker, never dereferenced with n_partials = 0)
      a.partials[i] = s.rows > 0 ? carve.take<float>(a.n_partials[i]) : reinterpret_cast<float*>(s.d_log_scale);
    }
  }
  if (total == 0 && n_finish == 0) return 0;
  hipStream_t st = S(stream);
  if (total > 0) {
    ProfScope prof("l2norm_bwd_kernel", st);
    l2norm_bwd_kernel<<<(unsigned)total, L2N_THREADS, 0, st>>>(a, D, 1.0f / eps);
    if (int rc = check_launch("l2norm_bwd_kernel")) return rc;
  }
  if (n_finish > 0) {
    ProfScope prof("l2norm_finish_kernel", st);
    l2norm_finish_kernel<<<(unsigned)n_finish, L2N_FINISH_THREADS, 0, st>>>(a);
    return check_launch("l2norm_finish_kernel");
  }
  return 0;
}
