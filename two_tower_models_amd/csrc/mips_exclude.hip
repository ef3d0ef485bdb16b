// MIPS exclusion filter: drop each query's already-seen items from its candidate list, keeping the order.
//
// The search itself (mips.hip) is untouched.  Under the (score desc, index asc) order the top-K of `corpus \ S` is the
// first K members of the top-(K + E) list of the whole corpus that are not in S, |S| <= E (DESIGN.md "Exclusion"): removing
// at most E elements from a sorted list cannot push a survivor of the first K past position K + E.  So the caller searches
// at K + E and this kernel filters: per query, the first K candidates in INPUT ORDER whose key is not in the query's
// exclusion set, indices and scores copied bit for bit, the tail (fewer than K survivors) filled with -1 / -inf and reported.
//
//   one workgroup (4 waves) per query;
//   the exclusion set in LDS: E <= 64 as a plain key list that every candidate compares against (broadcast reads),
//   larger E as an open-addressing hash set of full int64 keys (>= 2 E slots, linear probing; duplicates collapse);
//   the waves take consecutive 64-candidate tiles: a survivor's output position is the number of survivors before it,
//   i.e. a wave ballot + popcount and a 4-entry cross-wave prefix in LDS on top of the running count (route.hip's form).
// Integer compares and copies only: no float arithmetic, no float atomics, positions by list order -- deterministic.
#include "common.hpp"

namespace tt {

constexpr int XT = 256;           // threads per workgroup
constexpr int XW = XT / WAVE;     // waves per workgroup
constexpr int X_DIRECT = 64;      // E up to here: compare against the staged list itself
constexpr int64_t X_MAX_E = 4096;
constexpr int64_t X_EMPTY = -1;   // (keys of the set are >= 0)

__device__ __forceinline__ uint32_t x_slot(int64_t key, int shift) {
  return (uint32_t)(((uint64_t)key * 0x9E3779B97F4A7C15ull) >> shift);  // Fibonacci hashing: the top log2(slots) bits
}

// HASH = false: set[0:E] the exclusion list as given; HASH = true: set[0:slots] the hash set, slots = 1 << (64 - shift)
template <bool HASH>
__global__ __launch_bounds__(XT) void mips_exclude_kernel(const int64_t* __restrict__ idx, const float* __restrict__ scores,
                                                          int64_t n_cand, int64_t K, const int64_t* __restrict__ exclude,
                                                          int32_t E, const int64_t* __restrict__ row_key, int64_t C,
                                                          int32_t slots, int shift, int64_t* __restrict__ idx_out,
                                                          float* __restrict__ score_out, int32_t* __restrict__ short_flag) {
  extern __shared__ int64_t set[];  // [HASH ? slots : E] keys, then XW wave counts
  int32_t* wcnt = reinterpret_cast<int32_t*>(set + (HASH ? slots : E));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  const int64_t* ex = exclude + b * E;
  if (HASH) {
    for (int s = tid; s < slots; s += XT) set[s] = X_EMPTY;
    __syncthreads();
    for (int j = tid; j < E; j += XT) {
      const int64_t key = ex[j];
      if (key < 0) continue;  // padding
      uint32_t h = x_slot(key, shift);
      for (;;) {  // (at most E of >= 2 E slots are ever taken: an empty one is always found)
        const int64_t was = (int64_t)atomicCAS(reinterpret_cast<unsigned long long*>(&set[h]),
                                               (unsigned long long)X_EMPTY, (unsigned long long)key);
        if (was == X_EMPTY || was == key) break;
        h = (h + 1) & (uint32_t)(slots - 1);
      }
    }
  } else {
    for (int j = tid; j < E; j += XT) set[j] = ex[j];
  }
  __syncthreads();

  const int64_t* qi = idx + b * n_cand;
  const float* qs = scores + b * n_cand;
  int64_t* oi = idx_out + b * K;
  float* os = score_out + b * K;
  int64_t done = 0;  // survivors placed so far: the same value in every thread
  for (int64_t t0 = 0; t0 < n_cand && done < K; t0 += XT) {
    const int64_t j = t0 + tid;
    bool keep = false;
    int64_t id = -1;
    if (j < n_cand) {
      id = qi[j];
      if (id >= 0 && id < C) {  // anything else is dropped, and never reaches row_key
        const int64_t key = row_key ? row_key[id] : id;
        bool hit = false;
        if (key >= 0) {  // (the set holds no negative key: those are padding)
          if (HASH) {
            uint32_t h = x_slot(key, shift);
            for (;;) {
              const int64_t was = set[h];
              if (was == key) { hit = true; break; }
              if (was == X_EMPTY) break;
              h = (h + 1) & (uint32_t)(slots - 1);
            }
          } else {
            for (int e = 0; e < E; ++e) hit |= set[e] == key;
          }
        }
        keep = !hit;
      }
    }
    const uint64_t mine = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(mine);
    __syncthreads();
    int64_t pos = done + __popcll(mine & ((1ull << lane) - 1ull));
    int32_t tile = 0;
#pragma unroll
    for (int w = 0; w < XW; ++w) {
      const int32_t c = wcnt[w];
      if (w < wave) pos += c;
      tile += c;
    }
    if (keep && pos < K) {
      oi[pos] = id;
      os[pos] = qs[j];
    }
    done += tile;
    __syncthreads();  // wcnt is rewritten by the next tile
  }
  if (done < K) {
    for (int64_t p = done + tid; p < K; p += XT) {
      oi[p] = -1;
      os[p] = __uint_as_float(0xff800000u);  // -inf
    }
    if (tid == 0) *short_flag = 1;
  }
}

}  // namespace tt

using namespace tt;

extern "C" int tt_mips_exclude(const int64_t* idx, const float* scores, int64_t B, int64_t n_cand, int64_t K,
                               const int64_t* exclude, int64_t E, const int64_t* row_key, int64_t C, int64_t* idx_out,
                               float* score_out, int32_t* short_flag, tt_stream_t stream) {
  if (!idx || !scores || !exclude || !idx_out || !score_out || !short_flag) return fail_arg("tt_mips_exclude: null pointer");
  if (B < 1 || B >= (1ll << 31) || n_cand < 1 || n_cand >= (1ll << 31) || K < 1 || K > n_cand || E < 1 || E > X_MAX_E || C < 1)
    return fail_arg("tt_mips_exclude: sizes (1 <= K <= n_cand < 2^31, 1 <= E <= 4096, 1 <= B < 2^31, C >= 1)");
  hipStream_t st = S(stream);
  ProfScope prof("mips_exclude_kernel", st);
  if (E <= X_DIRECT) {
    const size_t lds = (size_t)E * sizeof(int64_t) + XW * sizeof(int32_t);
    mips_exclude_kernel<false><<<(unsigned)B, XT, lds, st>>>(idx, scores, n_cand, K, exclude, (int32_t)E, row_key, C, 0, 0,
                                                            idx_out, score_out, short_flag);
    return check_launch("mips_exclude_kernel");
  }
  int log2_slots = 8;
  while ((1ll << log2_slots) < 2 * E) ++log2_slots;  // 256 .. 8192 slots
  const int32_t slots = 1 << log2_slots;
  const size_t lds = (size_t)slots * sizeof(int64_t) + XW * sizeof(int32_t);
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(mips_exclude_kernel<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { set_error("mips_exclude_kernel: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
  }
  mips_exclude_kernel<true><<<(unsigned)B, XT, lds, st>>>(idx, scores, n_cand, K, exclude, (int32_t)E, row_key, C, slots,
                                                         64 - log2_slots, idx_out, score_out, short_flag);
  return check_launch("mips_exclude_kernel");
}
