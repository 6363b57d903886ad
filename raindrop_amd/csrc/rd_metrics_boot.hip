// rd_metrics_boot.hip -- bootstrap confidence intervals of the validation metrics (include/raindrop_hip.h "validation metrics":
// rd_rank_bootstrap, _summary, _counts).  The resample rule and the statistics are stated there; this is how they are computed.
//
// A resample changes how often a sample counts, never where its score ranks, so nothing is sorted per resample:
//
//   sort     k_boot_sort, one workgroup per column: rd_metrics.hip's LDS bitonic sort on keys that carry the row,
//            (order-preserving score bits) << 32 | row << 1 | (y == column).  What leaves the kernel is one 16-bit code per sorted
//            position, last-of-its-tie-group << 15 | row << 1 | label: 2 N bytes per column, read back through L2 by every resample
//   counts   boot_counts: the workgroup of resample r forms m_r [N] u32 in LDS with integer LDS atomics, one Threefry call per two
//            draws (64 KB at N = 16384)
//   stats    k_boot_stats, grid (R, column groups): thread t owns the contiguous run of ceil(N / 1024) sorted positions rd_metrics.hip's
//            rank_stats gives it.  Pass 1 sums the run's weights m_r[row] and weighted positives; one workgroup scan turns them into
//            the cumulative (weight, tp) in front of every run and, by a running maximum over "this run closes a tie group", tells
//            every thread whose run holds the last group end in front of its own.  Pass 2 walks the run again: at every group end
//            (tp, fp) are the running sums and (tp_prev, fp_prev) those of the previous end -- of this run, or the published ones of
//            that thread.  Sums as in rank_stats: the numerator exact int64, the AP terms float64 per thread in index order, then
//            per wave, then over the 16 waves in order: a function of N alone.  A group of weight 0 adds (0)(..) to the numerator
//            and no AP term (tp == tp_prev), so multiplicity 0 needs no other case
//   means    k_boot_means: per resample the plain means over the columns, in column order (k_rank_means)
//   summary  k_boot_summary, one workgroup per (column or macro mean, metric): the R values into LDS (NaN -> +inf behind the valid
//            ones), bitonic sort ascending, two-pass mean / deviation with fixed-order sums, the two percentiles by linear interpolation
//
// Nothing waits on another workgroup; no floating-point atomics, no cooperative launch, no scratch.  N <= 16384 only: the chunked
// sort of rd_rank_metrics (N up to 2^22) has no row-carrying form, and the 16-bit codes and the LDS counts end there too.
#include "rd_common.h"
#include "rd_rng.h"

namespace rd {
namespace {

constexpr int RB_NT = 1024;          // threads of the sort / statistics workgroups (rd_metrics.hip RM_NT: the same runs, the same sums)
constexpr int RB_NMAX = 16384;       // samples: one LDS sort per column, 14 bits of row in a 16-bit code
constexpr int RB_RMAX = 4096;        // resamples: the summary sorts them in LDS (32 KB)
constexpr int RB_SNT = 256;          // threads of the summary workgroups
constexpr int RB_WG_WANT = 1024;     // workgroups k_boot_stats aims for when R alone gives fewer: columns are split over blockIdx.y

// rd_metrics.hip make_key's score part: float32 -> uint32 whose unsigned order is the float order, -0.0 == +0.0 one key, a positive
// NaN above +inf, a negative one below -inf
__device__ __forceinline__ uint32_t order_bits(float s) {
  uint32_t u = __float_as_uint(s);
  if ((u << 1) == 0u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// m[0 .. N) <- multiplicities of resample r (the header's resample rule), by the whole workgroup; ends with a barrier
__device__ __forceinline__ void boot_counts(uint32_t* m, int N, int r, uint64_t seed) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < N; i += nt) m[i] = 0u;
  __syncthreads();
  const uint64_t call0 = (uint64_t)r * (2ull * (uint64_t)((N + 3) >> 2));     // two calls per quad of four draws
  const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
  for (int h = tid; 2 * h < N; h += nt) {
    const uint64_t call = call0 + (uint64_t)h;
    const uint2 w = threefry2x32_13(make_uint2((uint32_t)call, (uint32_t)(call >> 32) | ((uint32_t)SITE_BOOTSTRAP << 16)), key);
    atomicAdd(&m[__umulhi(w.x, (uint32_t)N)], 1u);                             // draw 2h;  floor(word * N / 2^32) < N
    if (2 * h + 1 < N) atomicAdd(&m[__umulhi(w.y, (uint32_t)N)], 1u);          // draw 2h + 1
  }
  __syncthreads();
}

// one column: keys with the row, sorted descending in LDS, out as 16-bit codes (file comment)
__global__ __launch_bounds__(RB_NT) void k_boot_sort(const float* scores, long ld, const int64_t* y, int N, int n2, uint16_t* ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rb_sm[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(rb_sm);
  const int tid = threadIdx.x, c = blockIdx.y;
  for (int i = tid; i < n2; i += RB_NT) {
    uint64_t k = 0;                                        // padding: not above any real key
    if (i < N) k = ((uint64_t)order_bits(scores[(long)i * ld + c]) << 32) | ((uint64_t)i << 1) | (y[i] == (int64_t)c ? 1ull : 0ull);
    keys[i] = k;
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = tid; idx < (n2 >> 1); idx += RB_NT) {
        const int l = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), r = l | j;
        const bool desc = (l & k) == 0;
        const uint64_t x = keys[l], z = keys[r];
        if ((x < z) == desc) { keys[l] = z; keys[r] = x; }
      }
      __syncthreads();
    }
  }
  uint16_t* col = ws + (size_t)c * N;
  for (int i = tid; i < N; i += RB_NT) {
    const uint64_t k = keys[i];
    const bool last = (i == N - 1) || ((uint32_t)(keys[i + 1] >> 32) != (uint32_t)(k >> 32));      // (i + 1 <= N - 1 < n2)
    col[i] = (uint16_t)((last ? 0x8000u : 0u) | ((uint32_t)k & 0x7FFFu));
  }
}

struct BootOut { double* auroc; double* auprc; int64_t* num; int64_t* pos; };

__global__ __launch_bounds__(RB_NT) void k_boot_stats(const uint16_t* ws, int N, int C, uint64_t seed, BootOut o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rb_sm[];
  uint32_t* m = reinterpret_cast<uint32_t*>(rb_sm);
  __shared__ int s_sum[RB_NT / 64], s_end[RB_NT / 64];
  __shared__ int s_pub[RB_NT];                             // cumulative weight << 16 | tp at the last group end of each thread's run
  __shared__ long long s_num[RB_NT / 64];
  __shared__ double s_ap[RB_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
  boot_counts(m, N, r, seed);
  const int ipt = (N + RB_NT - 1) / RB_NT;
  const int lo = min(N, tid * ipt), hi = min(N, lo + ipt);
  for (int c = blockIdx.y; c < C; c += gridDim.y) {
    const uint16_t* col = ws + (size_t)c * N;
    // pass 1: weight and weighted positives of this run, packed weight << 16 | tp (both <= N <= 2^14: no carry between the halves,
    // and the workgroup total N << 16 | P fits an int); whether the run closes a tie group
    int sum = 0, ends = 0;
    for (int i = lo; i < hi; ++i) {
      const uint32_t e = col[i];
      const int w = (int)m[(e >> 1) & 0x3FFFu];
      sum += (w << 16) + ((e & 1u) ? w : 0);
      if (e & 0x8000u) ends = tid + 1;
    }
    int inc = sum, emax = ends;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d), q = __shfl_up(emax, d);
      if (lane >= d) { inc += v; emax = max(emax, q); }
    }
    if (lane == 63) { s_sum[wave] = inc; s_end[wave] = emax; }
    __syncthreads();
    int before = inc - sum, total = 0;
    int eprev = __shfl_up(emax, 1);                        // last thread in front of this one whose run closes a group, + 1 (0: none)
    if (lane == 0) eprev = 0;
#pragma unroll
    for (int w = 0; w < RB_NT / 64; ++w) {
      const int t = s_sum[w];
      if (w < wave) { before += t; eprev = max(eprev, s_end[w]); }
      total += t;
    }
    const int P = total & 0xFFFF;
    // pass 2a: publish the cumulative sums at this run's last group end
    if (ends) {
      int run = before, at = 0;
      for (int i = lo; i < hi; ++i) {
        const uint32_t e = col[i];
        const int w = (int)m[(e >> 1) & 0x3FFFu];
        run += (w << 16) + ((e & 1u) ? w : 0);
        if (e & 0x8000u) at = run;
      }
      s_pub[tid] = at;
    }
    __syncthreads();
    // pass 2b: the group ends of this run
    int prev = eprev > 0 ? s_pub[eprev - 1] : 0;
    int run = before;
    long long num = 0;
    double ap = 0.0;
    for (int i = lo; i < hi; ++i) {
      const uint32_t e = col[i];
      const int w = (int)m[(e >> 1) & 0x3FFFu];
      run += (w << 16) + ((e & 1u) ? w : 0);
      if (!(e & 0x8000u)) continue;
      const long long tp = run & 0xFFFF, tpp = prev & 0xFFFF;
      const long long fp = (long long)(run >> 16) - tp, fpp = (long long)(prev >> 16) - tpp;
      num += (fp - fpp) * (tp + tpp);
      if (tp > tpp) ap += (double)(tp - tpp) / (double)P * (double)tp / (double)(tp + fp);      // (tp > tpp >= 0: P > 0, tp + fp > 0)
      prev = run;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      num += __shfl_xor(num, d);
      ap += __shfl_xor(ap, d);                             // both partners add the same two values: one result per wave
    }
    if (lane == 0) { s_num[wave] = num; s_ap[wave] = ap; }
    __syncthreads();
    if (tid == 0) {
      long long tn = 0;
      double ta = 0.0;
      for (int w = 0; w < RB_NT / 64; ++w) { tn += s_num[w]; ta += s_ap[w]; }
      const long long Q = (long long)N - P;
      const double nan = __longlong_as_double(0x7FF8000000000000ll);
      const size_t at = (size_t)r * C + c;
      o.num[at] = tn;
      o.pos[at] = P;
      o.auroc[at] = (P > 0 && Q > 0) ? (double)tn / (2.0 * (double)P * (double)Q) : nan;
      o.auprc[at] = P > 0 ? ta : 0.0;
    }
    __syncthreads();                                       // the next column rewrites s_sum .. s_ap
  }
}

// per resample the plain means over the columns, in column order (rd_metrics.hip k_rank_means)
__global__ __launch_bounds__(256) void k_boot_means(int R, int C, const double* auroc, const double* auprc, double* mean) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  double a = 0.0, p = 0.0;
  for (int c = 0; c < C; ++c) { a += auroc[(size_t)r * C + c]; p += auprc[(size_t)r * C + c]; }
  mean[2 * r] = a / (double)C;
  mean[2 * r + 1] = p / (double)C;
}

__global__ __launch_bounds__(RB_NT) void k_boot_counts(int N, uint64_t seed, int r0, uint32_t* counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rb_sm[];
  uint32_t* m = reinterpret_cast<uint32_t*>(rb_sm);
  boot_counts(m, N, r0 + (int)blockIdx.x, seed);
  uint32_t* row = counts + (size_t)blockIdx.x * N;
  for (int i = threadIdx.x; i < N; i += RB_NT) row[i] = m[i];
}

// sum of v over the workgroup (RB_SNT threads) in a fixed order, the same value in every thread
__device__ __forceinline__ double summary_sum(double v, double* s_part) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();                                         // s_part may still be read from the previous sum
  if ((tid & 63) == 0) s_part[tid >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < RB_SNT / 64; ++w) t += s_part[w];
  return t;
}

// the q-quantile of the n ascending values v, numpy.percentile's default (linear) rule
__device__ __forceinline__ double quantile_linear(const double* v, int n, double q) {
  const double h = (double)(n - 1) * q;
  int i = (int)floor(h);
  i = max(0, min(i, n - 1));
  const int j = min(i + 1, n - 1);
  const double a = v[i], b = v[j], t = h - (double)i;
  return t >= 0.5 ? b - (b - a) * (1.0 - t) : a + (b - a) * t;
}

// blockIdx.x: column 0 .. C - 1 or C = the macro mean; blockIdx.y: 0 AUROC, 1 AUPRC
__global__ __launch_bounds__(RB_SNT) void k_boot_summary(int R, int R2, int C, const double* auroc_b, const double* auprc_b,
                                                         const double* mean_b, double alpha, double* summary) {
  __shared__ double v[RB_RMAX];
  __shared__ double s_part[RB_SNT / 64];
  __shared__ int s_cnt[RB_SNT / 64];
  const int tid = threadIdx.x, col = blockIdx.x, metric = blockIdx.y;
  const double* src = col < C ? (metric ? auprc_b : auroc_b) + col : mean_b + metric;
  const size_t stride = col < C ? (size_t)C : 2;
  const double inf = __longlong_as_double(0x7FF0000000000000ll), nan = __longlong_as_double(0x7FF8000000000000ll);
  int cnt = 0;
  for (int i = tid; i < R2; i += RB_SNT) {
    double x = inf;                                        // padding and NaN: behind every valid value
    if (i < R) {
      const double s = src[(size_t)i * stride];
      if (s == s) { x = s; ++cnt; }
    }
    v[i] = x;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int w = 0; w < RB_SNT / 64; ++w) n += s_cnt[w];
  for (int k = 2; k <= R2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = tid; idx < (R2 >> 1); idx += RB_SNT) {
        const int l = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), r = l | j;
        const bool asc = (l & k) == 0;
        const double x = v[l], z = v[r];
        if ((x > z) == asc) { v[l] = z; v[r] = x; }
      }
      __syncthreads();
    }
  }
  // the n valid values are v[0 .. n), ascending; every thread sums its contiguous run in index order
  const int ipt = R2 / RB_SNT > 0 ? R2 / RB_SNT : 1;
  const int lo = min(n, tid * ipt), hi = min(n, lo + ipt);
  double s = 0.0;
  for (int i = lo; i < hi; ++i) s += v[i];
  const double mean = summary_sum(s, s_part) / (double)n;               // n == 0: NaN
  double ss = 0.0;
  for (int i = lo; i < hi; ++i) { const double d = v[i] - mean; ss += d * d; }
  const double var = summary_sum(ss, s_part) / (double)(n - 1);
  if (tid == 0) {
    double* out = summary + ((size_t)metric * (C + 1) + col) * 5;
    out[0] = (double)n;
    out[1] = n > 0 ? mean : nan;
    out[2] = n > 1 ? sqrt(var) : nan;
    out[3] = n > 1 ? quantile_linear(v, n, 0.5 * alpha) : nan;
    out[4] = n > 1 ? quantile_linear(v, n, 1.0 - 0.5 * alpha) : nan;
  }
}

int pow2_at_least(long n) {
  int p = 2;
  while ((long)p < n) p <<= 1;
  return p;
}

bool in_envelope(int64_t N, int32_t C, int32_t R) { return N >= 1 && N <= RB_NMAX && C >= 1 && C <= 65535 && R >= 1 && R <= RB_RMAX; }

}  // namespace
}  // namespace rd

using namespace rd;

extern "C" size_t rd_rank_bootstrap_workspace_bytes(int64_t N, int32_t C, int32_t R) {
  return in_envelope(N, C, R) ? (size_t)C * (size_t)N * sizeof(uint16_t) : 0;
}

extern "C" int rd_rank_bootstrap(int64_t N, int32_t C, const float* scores, int64_t ld, const int64_t* y, int32_t R, uint64_t seed,
                                 double* auroc_b, double* auprc_b, int64_t* auroc_num_b, int64_t* pos_b, double* mean_b,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!in_envelope(N, C, R))
    return fail(RD_EUNSUPPORTED, "rd_rank_bootstrap: N=%ld C=%d R=%d outside 1 <= N <= %d (one LDS sort per column), 1 <= C <= 65535, 1 <= R <= %d",
                (long)N, C, R, RB_NMAX, RB_RMAX);
  RD_REQUIRE(ld >= C, "bad dims C=%d ld=%ld (C <= ld)", C, (long)ld);
  RD_REQUIRE(scores && y && auroc_b && auprc_b && auroc_num_b && pos_b && mean_b, "NULL tensor");
  const size_t need = rd_rank_bootstrap_workspace_bytes(N, C, R);
  RD_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 1) == 0,
             "workspace: %zu bytes, 2-byte aligned, needed (got %zu)", need, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  uint16_t* ws = static_cast<uint16_t*>(workspace);
  const int n = (int)N, n2 = pow2_at_least(N);
  RD_LDS_ATTR(k_boot_sort, RB_NMAX * sizeof(uint64_t));
  RD_LDS_ATTR(k_boot_stats, RB_NMAX * sizeof(uint32_t));
  hipLaunchKernelGGL(k_boot_sort, dim3(1, C), dim3(RB_NT), (size_t)n2 * sizeof(uint64_t), st, scores, (long)ld, y, n, n2, ws);
  if (int rc = check_launch("k_boot_sort")) return rc;
  const int groups = C < cdiv(RB_WG_WANT, R) ? C : cdiv(RB_WG_WANT, R);      // >= 1; every (r, c) is one workgroup's, whatever the split
  BootOut o{auroc_b, auprc_b, auroc_num_b, pos_b};
  hipLaunchKernelGGL(k_boot_stats, dim3(R, groups), dim3(RB_NT), (size_t)n * sizeof(uint32_t), st, ws, n, (int)C, seed, o);
  if (int rc = check_launch("k_boot_stats")) return rc;
  hipLaunchKernelGGL(k_boot_means, dim3(cdiv(R, 256)), dim3(256), 0, st, (int)R, (int)C, auroc_b, auprc_b, mean_b);
  return check_launch("k_boot_means");
}

extern "C" int rd_rank_bootstrap_summary(int32_t R, int32_t C, const double* auroc_b, const double* auprc_b, const double* mean_b,
                                         double alpha, double* summary, void* stream) {
  if (!in_envelope(1, C, R))
    return fail(RD_EUNSUPPORTED, "rd_rank_bootstrap_summary: C=%d R=%d outside 1 <= C <= 65535, 1 <= R <= %d", C, R, RB_RMAX);
  RD_REQUIRE(alpha > 0.0 && alpha < 1.0, "alpha = %g, need 0 < alpha < 1", alpha);
  RD_REQUIRE(auroc_b && auprc_b && mean_b && summary, "NULL tensor");
  hipLaunchKernelGGL(k_boot_summary, dim3(C + 1, 2), dim3(RB_SNT), 0, (hipStream_t)stream, (int)R, pow2_at_least(R), (int)C, auroc_b,
                     auprc_b, mean_b, alpha, summary);
  return check_launch("k_boot_summary");
}

extern "C" int rd_rank_bootstrap_counts(int64_t N, int32_t R, uint64_t seed, int32_t r0, int32_t nr, uint32_t* counts, void* stream) {
  if (!in_envelope(N, 1, R))
    return fail(RD_EUNSUPPORTED, "rd_rank_bootstrap_counts: N=%ld R=%d outside 1 <= N <= %d, 1 <= R <= %d", (long)N, R, RB_NMAX, RB_RMAX);
  RD_REQUIRE(r0 >= 0 && nr >= 0 && (int64_t)r0 + nr <= R, "bad rows r0=%d nr=%d (0 <= r0, r0 + nr <= R = %d)", r0, nr, R);
  if (nr == 0) return RD_OK;
  RD_REQUIRE(counts, "NULL tensor");
  RD_LDS_ATTR(k_boot_counts, RB_NMAX * sizeof(uint32_t));
  hipLaunchKernelGGL(k_boot_counts, dim3(nr), dim3(RB_NT), (size_t)N * sizeof(uint32_t), (hipStream_t)stream, (int)N, seed, r0, counts);
  return check_launch("k_boot_counts");
}
