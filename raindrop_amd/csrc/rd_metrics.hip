// rd_metrics.hip -- validation metrics on the device (include/raindrop_hip.h "validation metrics").
//
// code/Raindrop.py:348-370 copies the validation logits to the host every epoch and runs sklearn's roc_auc_score /
// average_precision_score there (two sorts), because the scheduler and the best-checkpoint test need them.  Here the ranking
// statistics are computed where the logits are:
//
//   keys    one 64-bit key per sample and column: (order-preserving bits of the float32 score) << 32 | (y == column)
//   sort    bitonic, descending.  N <= 16384 keys (128 KB) are sorted in ONE workgroup's LDS; larger N in 16384-key chunks in LDS
//           with the strides >= 16384 of the later stages as plain global compare-exchange launches in between
//   scan    tp (positives so far) as a workgroup scan over the sorted keys, written into the keys' low words in place
//   groups  tied scores form one threshold (sklearn: thresholds are the DISTINCT scores): the last key of a tie group finds
//           the group's first key by binary search in the sorted array -> (tp, fp) at this threshold and at the previous one
//   sums    AUROC numerator sum (fp - fp_prev)(tp + tp_prev): exact int64; AP sum (tp - tp_prev) / P * tp / (tp + fp): float64,
//           per thread in index order over its contiguous run of ceil(N / 1024) keys, then per wave, then over the 16 waves in
//           order -- a function of N alone, the same bits on every run, for every workspace address
//
// One workgroup of 1024 threads per column does the scan and the sums in both forms; nothing waits on another workgroup, there
// are no floating-point atomics and no cooperative launches.  No kernel here uses scratch.
#include "rd_common.h"

namespace rd {
namespace {

constexpr int RM_NT = 1024;          // threads of the sort / statistics workgroups
constexpr int RM_CH = 16384;         // keys one workgroup sorts in LDS (128 KB)
constexpr long RM_NMAX = 1L << 22;   // tp / fp live in 32-bit words of the keys

// float32 -> uint32 whose unsigned order is the float order; -0.0 and +0.0 compare equal as floats and get one key.
// NaNs are not refused (that would need a host sync): a positive NaN sorts above +inf, a negative one below -inf, by payload.
__device__ __forceinline__ uint64_t make_key(float s, bool pos) {
  uint32_t u = __float_as_uint(s);
  if ((u << 1) == 0u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)u << 32) | (pos ? 1ull : 0ull);
}

struct SortArgs {
  const float* scores; long ld; const int64_t* y;
  uint64_t* ws;                      // [C][n2] keys (chunked form)
  int N, n2, CH;                     // samples, padded power of two, keys per workgroup (min(n2, RM_CH))
  int k_lo, k_hi;                    // bitonic stages this launch runs (strides < CH of each)
  int from_scores;                   // build the keys from scores / y (first launch) or read them from ws
};
struct StatOut { double* auroc; double* auprc; int64_t* num; };

// Statistics of one column from its `N` sorted keys (LDS or global memory), by the whole workgroup (RM_NT threads).
__device__ __forceinline__ void rank_stats(uint64_t* keys, int N, int c, const StatOut& o) {
  __shared__ int s_cnt[RM_NT / 64];
  __shared__ long long s_num[RM_NT / 64];
  __shared__ double s_ap[RM_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ipt = (N + RM_NT - 1) / RM_NT;
  const int lo = min(N, tid * ipt), hi = min(N, lo + ipt);
  // positives in front of this thread's run: wave scan + the 16 wave totals
  int cnt = 0;
  for (int i = lo; i < hi; ++i) cnt += (int)(keys[i] & 1ull);
  int inc = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d);
    if (lane >= d) inc += v;
  }
  if (lane == 63) s_cnt[wave] = inc;
  __syncthreads();
  int before = inc - cnt, P = 0;
#pragma unroll
  for (int w = 0; w < RM_NT / 64; ++w) {
    const int t = s_cnt[w];
    if (w < wave) before += t;
    P += t;
  }
  // low word <- tp at (and including) this key; the label bit stays recoverable as a difference
  int run = before;
  for (int i = lo; i < hi; ++i) {
    const uint64_t k = keys[i];
    run += (int)(k & 1ull);
    keys[i] = (k & 0xFFFFFFFF00000000ull) | (uint32_t)run;
  }
  __syncthreads();
  long long num = 0;
  double ap = 0.0;
  for (int i = lo; i < hi; ++i) {
    const uint64_t k = keys[i];
    const uint32_t ord = (uint32_t)(k >> 32);
    const bool last = (i == N - 1) || ((uint32_t)(keys[i + 1] >> 32) != ord);
    if (!last) continue;
    int a = 0, b = i;                                     // first key of this tie group: descending order, so the first ord <= ours
    while (a < b) {
      const int m = (a + b) >> 1;
      if ((uint32_t)(keys[m] >> 32) > ord) a = m + 1; else b = m;
    }
    const long long tp = (uint32_t)k, tpp = a > 0 ? (long long)(uint32_t)keys[a - 1] : 0;
    const long long fp = (long long)(i + 1) - tp, fpp = (long long)a - tpp;
    num += (fp - fpp) * (tp + tpp);
    if (P > 0) ap += (double)(tp - tpp) / (double)P * (double)tp / (double)(tp + fp);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    num += __shfl_xor(num, d);
    ap += __shfl_xor(ap, d);                               // both partners add the same two values: one result per wave
  }
  if (lane == 0) { s_num[wave] = num; s_ap[wave] = ap; }
  __syncthreads();
  if (tid == 0) {
    long long tn = 0;
    double ta = 0.0;
    for (int w = 0; w < RM_NT / 64; ++w) { tn += s_num[w]; ta += s_ap[w]; }
    const long long Q = (long long)N - P;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    o.num[c] = tn;
    o.auroc[c] = (P > 0 && Q > 0) ? (double)tn / (2.0 * (double)P * (double)Q) : nan;
    o.auprc[c] = P > 0 ? ta : 0.0;                         // sklearn without positives: recall is defined as 1, precision is 0
  }
}

// Bitonic stages [k_lo, k_hi] on CH keys in LDS (the strides < CH of each stage; larger ones are k_rank_merge_global's).
// FUSED: the whole column is this one chunk -- build the keys, sort, statistics, nothing goes through global memory.
template <bool FUSED>
__global__ __launch_bounds__(RM_NT) void k_rank_sort(SortArgs a, StatOut o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rm_sm[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(rm_sm);
  const int tid = threadIdx.x, c = blockIdx.y, CH = a.CH;
  const int base = blockIdx.x * CH;
  uint64_t* col = FUSED ? nullptr : a.ws + (size_t)c * a.n2;
  for (int i = tid; i < CH; i += RM_NT) {
    const int g = base + i;
    uint64_t k = 0;                                        // padding: below every real key (or equal to one, bit for bit)
    if (FUSED || a.from_scores) {
      if (g < a.N) k = make_key(a.scores[(long)g * a.ld + c], a.y[g] == (int64_t)c);
    } else {
      k = col[g];
    }
    keys[i] = k;
  }
  __syncthreads();
  for (int k = a.k_lo; k <= a.k_hi; k <<= 1) {
    for (int j = min(k >> 1, CH >> 1); j > 0; j >>= 1) {
      for (int idx = tid; idx < (CH >> 1); idx += RM_NT) {
        const int l = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), r = l | j;
        const bool desc = ((base + l) & k) == 0;
        const uint64_t x = keys[l], y = keys[r];
        if ((x < y) == desc) { keys[l] = y; keys[r] = x; }
      }
      __syncthreads();
    }
  }
  if (FUSED) {
    rank_stats(keys, a.N, c, o);
  } else {
    for (int i = tid; i < CH; i += RM_NT) col[base + i] = keys[i];
  }
}

// one compare-exchange pass of stride j >= RM_CH of stage k over a column's n2 keys in global memory
__global__ __launch_bounds__(256) void k_rank_merge_global(uint64_t* ws, int n2, int j, int k) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= (n2 >> 1)) return;
  uint64_t* col = ws + (size_t)blockIdx.y * n2;
  const int l = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), r = l | j;
  const bool desc = (l & k) == 0;
  const uint64_t x = col[l], y = col[r];
  if ((x < y) == desc) { col[l] = y; col[r] = x; }
}

__global__ __launch_bounds__(RM_NT) void k_rank_stats(uint64_t* ws, int N, int n2, StatOut o) {
  rank_stats(ws + (size_t)blockIdx.y * n2, N, blockIdx.y, o);
}

// plain means over the columns, in column order (NaN where a column's value is NaN)
__global__ void k_rank_means(int C, const double* auroc, const double* auprc, double* mean) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double a = 0.0, p = 0.0;
  for (int c = 0; c < C; ++c) { a += auroc[c]; p += auprc[c]; }
  mean[0] = a / (double)C;
  mean[1] = p / (double)C;
}

// counts[t][p] += 1 for every row with label t in [0, C) and prediction p = first maximum of the row (np.argmax: a NaN is a maximum)
__global__ __launch_bounds__(256) void k_confusion(long N, int C, const float* logits, long ld, const int64_t* y,
                                                   unsigned long long* counts) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int64_t t = y[n];
  if (t < 0 || t >= C) return;
  const float* row = logits + n * ld;
  float best = row[0];
  int p = 0;
  for (int c = 1; c < C; ++c) {
    const float v = row[c];
    if (best == best && (v > best || v != v)) { best = v; p = c; }
  }
  atomicAdd(counts + (size_t)t * C + p, 1ull);
}

int pow2_at_least(long n) {
  int p = 2;
  while ((long)p < n) p <<= 1;
  return p;
}

}  // namespace
}  // namespace rd

using namespace rd;

extern "C" size_t rd_rank_metrics_workspace_bytes(int64_t N, int32_t C) {
  if (N < 1 || N > RM_NMAX || C < 1) return 0;
  const int n2 = pow2_at_least(N);
  return n2 <= RM_CH ? 0 : (size_t)C * n2 * sizeof(uint64_t);
}

extern "C" int rd_rank_metrics(int64_t N, int32_t C, const float* scores, int64_t ld, const int64_t* y, double* auroc,
                               double* auprc, double* mean, int64_t* auroc_num, void* workspace, size_t workspace_bytes,
                               void* stream) {
  RD_REQUIRE(N >= 1 && N <= RM_NMAX && C >= 1 && C <= 65535 && ld >= C, "bad dims N=%ld C=%d ld=%ld (1 <= N <= %ld, 1 <= C <= 65535 <= ld)",
             (long)N, C, (long)ld, RM_NMAX);
  RD_REQUIRE(scores && y && auroc && auprc && mean && auroc_num, "NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  SortArgs a{};
  a.scores = scores; a.ld = ld; a.y = y; a.N = (int)N; a.n2 = pow2_at_least(N); a.CH = a.n2 < RM_CH ? a.n2 : RM_CH;
  StatOut o{auroc, auprc, auroc_num};
  RD_LDS_ATTR(k_rank_sort<true>, RM_CH * sizeof(uint64_t));
  RD_LDS_ATTR(k_rank_sort<false>, RM_CH * sizeof(uint64_t));
  const size_t lds = (size_t)a.CH * sizeof(uint64_t);
  if (a.n2 <= RM_CH) {
    a.k_lo = 2; a.k_hi = a.n2;
    hipLaunchKernelGGL(k_rank_sort<true>, dim3(1, C), dim3(RM_NT), lds, st, a, o);
    if (int rc = check_launch("k_rank_sort<fused>")) return rc;
  } else {
    const size_t need = rd_rank_metrics_workspace_bytes(N, C);
    RD_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
               "workspace: %zu bytes, 8-byte aligned, needed (got %zu)", need, workspace_bytes);
    a.ws = static_cast<uint64_t*>(workspace);
    const dim3 chunks(a.n2 / RM_CH, C), pairs(cdiv(a.n2 >> 1, 256), C);
    a.from_scores = 1; a.k_lo = 2; a.k_hi = RM_CH;
    hipLaunchKernelGGL(k_rank_sort<false>, chunks, dim3(RM_NT), lds, st, a, o);
    if (int rc = check_launch("k_rank_sort<chunks>")) return rc;
    a.from_scores = 0;
    for (int k = 2 * RM_CH; k <= a.n2; k <<= 1) {
      for (int j = k >> 1; j >= RM_CH; j >>= 1) {
        hipLaunchKernelGGL(k_rank_merge_global, pairs, dim3(256), 0, st, a.ws, a.n2, j, k);
        if (int rc = check_launch("k_rank_merge_global")) return rc;
      }
      a.k_lo = a.k_hi = k;
      hipLaunchKernelGGL(k_rank_sort<false>, chunks, dim3(RM_NT), lds, st, a, o);
      if (int rc = check_launch("k_rank_sort<merge>")) return rc;
    }
    hipLaunchKernelGGL(k_rank_stats, dim3(1, C), dim3(RM_NT), 0, st, a.ws, a.N, a.n2, o);
    if (int rc = check_launch("k_rank_stats")) return rc;
  }
  hipLaunchKernelGGL(k_rank_means, dim3(1), dim3(64), 0, st, (int)C, auroc, auprc, mean);
  return check_launch("k_rank_means");
}

extern "C" int rd_confusion(int64_t N, int32_t C, const float* logits, int64_t ld, const int64_t* y, int64_t* counts,
                            void* stream) {
  RD_REQUIRE(N >= 0 && C >= 1 && C <= 4096 && ld >= C, "bad dims N=%ld C=%d ld=%ld", (long)N, C, (long)ld);
  RD_REQUIRE(counts && (N == 0 || (logits && y)), "NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  RD_HIP(hipMemsetAsync(counts, 0, (size_t)C * C * sizeof(int64_t), st));
  if (N == 0) return RD_OK;
  hipLaunchKernelGGL(k_confusion, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (long)N, (int)C, logits, (long)ld, y,
                     reinterpret_cast<unsigned long long*>(counts));
  return check_launch("k_confusion");
}
