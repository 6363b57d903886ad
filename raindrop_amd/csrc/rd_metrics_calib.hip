// rd_metrics_calib.hip -- calibration of the validation probabilities (include/raindrop_hip.h "calibration": rd_calibration,
// rd_fit_temperature).  The bin rule, the statistics and the result cells are stated there; this is how they are computed.
//
//   rows     k_calib_rows, G = calib_plan(N).G workgroups of 256 threads: workgroup g owns the contiguous rows [g per, (g + 1) per),
//            per a multiple of 256, and walks them 256 at a time.  Thread t forms row (chunk base + t): softmax(logits / T) in
//            float64, max-subtracted; confidence, hit, bin; its NLL and Brier terms.  The (bin, hit) codes and the confidences of the
//            256 rows go to LDS and thread b sums bin b's over the 256 in row order -- counts exact, the confidence sum float64 in an
//            order fixed by N -- accumulating over the chunks in order.  NLL / Brier: per thread over its chunks in order, then per
//            wave, then over the 4 waves in order.  Partials: cnt int64 [G][M][2], sc f64 [G][M], scal f64 [G][2]
//   finish   k_calib_finish, one workgroup: thread b sums bin b's partials over g in order and writes its counts / table row; NLL and
//            Brier over g by contiguous runs per thread, per wave, over the waves; thread 0 then walks the M bins in order for ECE,
//            MCE, the hit rate and the mean confidence
//   fit      k_fit_temperature<STAGE>, ONE workgroup of 1024 threads that runs the whole safeguarded Newton iteration: every
//            evaluation of (g, h, NLL) at a beta is a pass over the rows -- thread t owns rows t, t + 1024, .. in that order -- and one
//            fixed-order block reduction (per wave by shuffles, the 16 wave sums in order from LDS, double-buffered: one barrier per
//            evaluation), after which every thread holds the same three numbers and takes the same branch.  STAGE: the logits are
//            copied once into LDS ([N][C] float32) and read from there; otherwise every pass re-reads them from global memory (they
//            stay in L2).  The arithmetic is the same instruction stream on the same values: the two forms give the same bits.
//            fit_route decides the form from (N, C) alone; the launch and rd_debug_calibration_route both call it.
//
// Nothing waits on another workgroup; no floating-point atomics (no atomics at all), no cooperative launch, no scratch.
#include "rd_common.h"

namespace rd {
namespace {

constexpr int CB_NT = 256;                       // threads of both calibration kernels = rows per chunk = the most bins
constexpr int CB_GMAX = 1024;                    // the most workgroups of k_calib_rows (partials: at most 1024 x 256 x 24 bytes)
constexpr long CB_NLIM = 1l << 24;               // N < 2^24
constexpr int CB_CMAX = 64, CB_MMAX = 256;
constexpr int FT_NT = 1024;                      // threads of the fit's one workgroup
constexpr int FT_NMAX = 16384;                   // the bootstrap's envelope
constexpr size_t FT_LDS_STAGE = 159 * 1024;      // dynamic LDS the staged form may use: the CU's 160 KiB less 1 KiB for the reduction scratch
constexpr double FT_BETA_LO = 1e-2, FT_BETA_HI = 1e2, FT_TOL = 1e-12;
constexpr int FT_ITMAX = 100;

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7FF8000000000000ll); }

struct CalibPlan { int G; long per; };           // G workgroups of `per` rows each (the last one fewer)
CalibPlan calib_plan(int64_t N) {
  const long chunks = (long)((N + CB_NT - 1) / CB_NT);
  const long per = ((chunks + CB_GMAX - 1) / CB_GMAX) * CB_NT;
  return CalibPlan{(int)((N + per - 1) / per), per};
}
bool calib_envelope(int64_t N, int32_t C, int32_t M) { return N >= 1 && N < CB_NLIM && C >= 2 && C <= CB_CMAX && M >= 1 && M <= CB_MMAX; }

struct CalibPart { int64_t* cnt; double* sc; double* scal; };
CalibPart calib_part(void* ws, int G, int M) {
  CalibPart p;
  p.cnt = static_cast<int64_t*>(ws);
  p.sc = reinterpret_cast<double*>(p.cnt + (size_t)G * M * 2);
  p.scal = p.sc + (size_t)G * M;
  return p;
}

// the bin of a confidence in [0, 1]: i with i / M < conf <= (i + 1) / M, 0 for conf == 0; -1 for a NaN.  The guess from the product
// is corrected against the edges themselves, (double)i / (double)M, so the rule is exact
__device__ __forceinline__ int calib_bin(double conf, int M) {
  if (!(conf == conf)) return -1;
  const double dm = (double)M;
  int k = (int)ceil(conf * dm) - 1;
  k = max(0, min(k, M - 1));
  while (k > 0 && conf <= (double)k / dm) --k;
  while (k < M - 1 && conf > (double)(k + 1) / dm) ++k;
  return k;
}

__global__ __launch_bounds__(CB_NT) void k_calib_rows(long N, int C, const float* logits, long ld, const int64_t* y, const double* temperature,
                                                     int column, int M, long per, CalibPart part) {
  __shared__ int s_code[CB_NT];                  // bin << 1 | hit of the chunk's rows; -1: no row, or a NaN confidence
  __shared__ double s_conf[CB_NT];
  __shared__ double s_red[CB_NT / 64][2];
  const int tid = threadIdx.x, g = blockIdx.x;
  const double T = temperature ? temperature[0] : 1.0;
  const long lo = (long)g * per, hi = min(N, lo + per);
  long bn = 0, bh = 0;                           // bin `tid`: rows, hits, confidence sum
  double bs = 0.0, nll = 0.0, brier = 0.0;
  for (long base = lo; base < hi; base += CB_NT) {
    const long n = base + tid;
    int code = -1;
    double conf = 0.0;
    if (n < hi) {
      const float* row = logits + n * ld;
      const int64_t t = y[n];
      float best = row[0];
      int am = 0;                                // first maximum of the logits (T > 0 keeps their order)
      for (int c = 1; c < C; ++c) {
        const float v = row[c];
        if (v > best) { best = v; am = c; }
      }
      const double m = (double)best / T;
      double sum = 0.0;
      for (int c = 0; c < C; ++c) sum += exp((double)row[c] / T - m);
      const bool labelled = t >= 0 && t < (int64_t)C;
      double b = 0.0, zy = 0.0, pcol = 0.0;
      for (int c = 0; c < C; ++c) {
        const double z = (double)row[c] / T - m;
        const double p = exp(z) / sum;
        const double d = p - ((int64_t)c == t ? 1.0 : 0.0);
        if (column < 0) b += d * d;
        else if (c == column) { b = d * d; pcol = p; }
        if ((int64_t)c == t) zy = z;
      }
      int hit;
      if (column < 0) { conf = 1.0 / sum; hit = labelled && t == (int64_t)am; }      // max_c p = exp(0) / sum
      else { conf = pcol; hit = t == (int64_t)column; }
      nll += labelled ? log(sum) - zy : qnan();
      brier += labelled ? b : qnan();
      const int k = calib_bin(conf, M);
      code = k < 0 ? -1 : (k << 1) | hit;
    }
    s_code[tid] = code;
    s_conf[tid] = conf;
    __syncthreads();
    if (tid < M) {
      for (int j = 0; j < CB_NT; ++j) {
        const int e = s_code[j];
        if (e >= 0 && (e >> 1) == tid) { ++bn; bh += e & 1; bs += s_conf[j]; }
      }
    }
    __syncthreads();                             // the next chunk rewrites s_code, s_conf
  }
  if (tid < M) {
    part.cnt[((size_t)g * M + tid) * 2] = bn;
    part.cnt[((size_t)g * M + tid) * 2 + 1] = bh;
    part.sc[(size_t)g * M + tid] = bs;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    nll += __shfl_xor(nll, d);
    brier += __shfl_xor(brier, d);
  }
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = nll; s_red[tid >> 6][1] = brier; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < CB_NT / 64; ++w) { a += s_red[w][0]; b += s_red[w][1]; }
    part.scal[2 * g] = a;
    part.scal[2 * g + 1] = b;
  }
}

__global__ __launch_bounds__(CB_NT) void k_calib_finish(long N, int M, int G, CalibPart part, int64_t* counts, double* table, double* summary) {
  __shared__ long long s_n[CB_NT], s_h[CB_NT];
  __shared__ double s_c[CB_NT];
  __shared__ double s_red[CB_NT / 64][2];
  const int tid = threadIdx.x;
  if (tid < M) {
    long long n = 0, h = 0;
    double s = 0.0;
    for (int g = 0; g < G; ++g) {
      n += part.cnt[((size_t)g * M + tid) * 2];
      h += part.cnt[((size_t)g * M + tid) * 2 + 1];
      s += part.sc[(size_t)g * M + tid];
    }
    s_n[tid] = n; s_h[tid] = h; s_c[tid] = s;
    counts[2 * tid] = n;
    counts[2 * tid + 1] = h;
    table[3 * tid] = (double)n;
    table[3 * tid + 1] = n > 0 ? s / (double)n : qnan();
    table[3 * tid + 2] = n > 0 ? (double)h / (double)n : qnan();
  }
  const int ipt = (G + CB_NT - 1) / CB_NT;
  const int lo = min(G, tid * ipt), hi = min(G, lo + ipt);
  double nll = 0.0, brier = 0.0;
  for (int g = lo; g < hi; ++g) { nll += part.scal[2 * g]; brier += part.scal[2 * g + 1]; }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    nll += __shfl_xor(nll, d);
    brier += __shfl_xor(brier, d);
  }
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = nll; s_red[tid >> 6][1] = brier; }
  __syncthreads();
  if (tid == 0) {
    double a = 0.0, b = 0.0;
    for (int w = 0; w < CB_NT / 64; ++w) { a += s_red[w][0]; b += s_red[w][1]; }
    const double dn = (double)N;
    double ece = 0.0, mce = 0.0, conf = 0.0;
    long long hits = 0;
    for (int i = 0; i < M; ++i) {
      const long long n = s_n[i];
      if (n == 0) continue;                      // an empty bin: weight 0 in the ECE, no part in the MCE
      const double gap = fabs((double)s_h[i] / (double)n - s_c[i] / (double)n);
      ece += (double)n / dn * gap;
      mce = gap > mce || gap != gap ? gap : mce;
      conf += s_c[i];
      hits += s_h[i];
    }
    summary[0] = ece;
    summary[1] = mce;
    summary[2] = b / dn;
    summary[3] = a / dn;
    summary[4] = (double)hits / dn;
    summary[5] = conf / dn;
  }
}

// ---- the fit ----
struct FitEval { double g, h, nll; };

// (g, h, NLL) at beta as MEANS over the N rows; the same three values in every thread.  `buf`: the parity of the evaluation
template <bool STAGE>
__device__ __forceinline__ FitEval fit_eval(double beta, int buf, int N, int C, const float* logits, long ld, const float* stage,
                                            const int64_t* y, double (*s_part)[FT_NT / 64][3]) {
  const int tid = threadIdx.x;
  double sg = 0.0, sh = 0.0, sn = 0.0;
  for (int i = tid; i < N; i += FT_NT) {
    const float* row = STAGE ? stage + (size_t)i * C : logits + (long)i * ld;
    const int64_t t = y[i];
    float mx = row[0];
    for (int c = 1; c < C; ++c) {
      const float v = row[c];
      mx = v > mx ? v : mx;
    }
    double S0 = 0.0, S1 = 0.0, S2 = 0.0, dy = qnan();        // a label outside [0, C): a non-finite gradient
    for (int c = 0; c < C; ++c) {
      const double d = (double)row[c] - (double)mx;          // <= 0: the row's own maximum taken out, which moves neither g nor h
      const double w = exp(beta * d);
      S0 += w;
      S1 += w * d;
      S2 += w * d * d;
      if ((int64_t)c == t) dy = d;
    }
    const double E = S1 / S0;
    sg += E - dy;
    sh += S2 / S0 - E * E;
    sn += log(S0) - beta * dy;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    sg += __shfl_xor(sg, d);
    sh += __shfl_xor(sh, d);
    sn += __shfl_xor(sn, d);
  }
  if ((tid & 63) == 0) { s_part[buf][tid >> 6][0] = sg; s_part[buf][tid >> 6][1] = sh; s_part[buf][tid >> 6][2] = sn; }
  __syncthreads();                               // the other buffer is free: every thread read it before this barrier
  double g = 0.0, h = 0.0, n = 0.0;
#pragma unroll
  for (int w = 0; w < FT_NT / 64; ++w) { g += s_part[buf][w][0]; h += s_part[buf][w][1]; n += s_part[buf][w][2]; }
  const double dn = (double)N;
  return FitEval{g / dn, h / dn, n / dn};
}

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }

template <bool STAGE>
__global__ __launch_bounds__(FT_NT) void k_fit_temperature(int N, int C, const float* logits, long ld, const int64_t* y, double* result) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ft_sm[];
  __shared__ double s_part[2][FT_NT / 64][3];
  float* stage = reinterpret_cast<float*>(ft_sm);
  const int tid = threadIdx.x;
  if (STAGE) {
    for (int i = tid; i < N * C; i += FT_NT) stage[i] = logits[(long)(i / C) * ld + (i % C)];      // (N C <= 159 KiB / 4)
    __syncthreads();
  }
  // One evaluation site, three phases.  0: beta = 1 -- the NLL before, and which side the minimum lies on (g rises with beta: g' = h
  // >= 0).  1: the bracket's end on that side -- no sign change there means the minimum is outside.  2: g(lo) < 0 < g(hi); Newton from
  // beta = 1, where a step that leaves the bracket, has no usable h or does not halve the previous step is replaced by the bracket's
  // midpoint, and every evaluation moves one end of the bracket to its beta by the sign of g
  int evals = 0, phase = 0;
  double beta = 1.0, status = 3.0, nll1 = 0.0, lo = FT_BETA_LO, hi = FT_BETA_HI, step = 0.0;
  FitEval e, at1{0.0, 0.0, 0.0};
  for (;;) {
    e = fit_eval<STAGE>(beta, evals & 1, N, C, logits, ld, stage, y, s_part);
    ++evals;
    if (phase == 0) nll1 = e.nll;
    if (!finite_d(e.g)) { status = 4.0; break; }
    if (e.g == 0.0) { status = 0.0; break; }
    if (phase == 0) {
      at1 = e;
      if (e.g < 0.0) { lo = 1.0; beta = FT_BETA_HI; } else { hi = 1.0; beta = FT_BETA_LO; }
      phase = 1;
      continue;
    }
    if (phase == 1) {
      if (lo == 1.0 ? e.g < 0.0 : e.g > 0.0) { status = lo == 1.0 ? 1.0 : 2.0; break; }
      step = hi - lo;
      beta = 1.0;
      e = at1;
      phase = 2;
    } else {
      if (e.g < 0.0) lo = beta; else hi = beta;
      if (fabs(step) <= FT_TOL * beta || hi - lo <= FT_TOL * beta) { status = 0.0; break; }
    }
    if (evals >= FT_ITMAX) break;                // status 3
    double next = beta - e.g / e.h;
    const bool usable = e.h > 0.0 && finite_d(next);
    if (usable && fabs(next - beta) <= FT_TOL * beta) { status = 0.0; break; }      // the step Newton asks for is below the tolerance: beta stands
    if (!(usable && next > lo && next < hi && fabs(next - beta) <= 0.5 * fabs(step))) next = 0.5 * (lo + hi);
    step = next - beta;
    beta = next;
  }
  if (tid == 0) {
    const bool bad = status == 4.0;
    result[0] = bad ? 1.0 : status == 1.0 ? FT_BETA_LO : status == 2.0 ? FT_BETA_HI : 1.0 / beta;      // (T = 1 / beta: the ends exchanged)
    result[1] = bad ? 1.0 : beta;
    result[2] = nll1;
    result[3] = bad ? nll1 : e.nll;
    result[4] = (double)evals;
    result[5] = status;
    result[6] = e.g;
    result[7] = 0.0;
  }
}

// the form of a fit of [N, C] logits, decided here and nowhere else: staged in LDS when N C 4 bytes fit the budget (and
// rd_debug_set_calibration_stage has not switched staging off: the tests' way to run both forms on the same logits)
int g_fit_stage_on = 1;
struct FitRoute { bool stage; size_t lds; };
bool fit_route(int64_t N, int32_t C, FitRoute* r) {
  if (N < 1 || N > FT_NMAX || C < 2 || C > CB_CMAX) return false;
  const size_t bytes = (size_t)N * (size_t)C * sizeof(float);
  r->stage = g_fit_stage_on && bytes <= FT_LDS_STAGE;
  r->lds = r->stage ? bytes : 0;
  return true;
}

}  // namespace
}  // namespace rd

using namespace rd;

extern "C" size_t rd_calibration_workspace_bytes(int64_t N, int32_t C, int32_t M) {
  if (!calib_envelope(N, C, M)) return 0;
  return (size_t)calib_plan(N).G * ((size_t)M * 24 + 16);
}

extern "C" int rd_calibration(int64_t N, int32_t C, const float* logits, int64_t ld, const int64_t* y, const double* temperature,
                              int32_t column, int32_t M, int64_t* counts, double* table, double* summary, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!calib_envelope(N, C, M))
    return fail(RD_EUNSUPPORTED, "rd_calibration: N=%ld C=%d M=%d outside 1 <= N < 2^24, 2 <= C <= %d, 1 <= M <= %d", (long)N, C, M, CB_CMAX,
                CB_MMAX);
  RD_REQUIRE(ld >= C && column >= -1 && column < C, "bad dims C=%d ld=%ld column=%d (C <= ld, -1 <= column < C)", C, (long)ld, column);
  RD_REQUIRE(logits && y && counts && table && summary, "NULL tensor");
  const size_t need = rd_calibration_workspace_bytes(N, C, M);
  RD_REQUIRE(workspace && workspace_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
             "workspace: %zu bytes, 8-byte aligned, needed (got %zu)", need, workspace_bytes);
  hipStream_t st = (hipStream_t)stream;
  const CalibPlan plan = calib_plan(N);
  const CalibPart part = calib_part(workspace, plan.G, M);
  hipLaunchKernelGGL(k_calib_rows, dim3(plan.G), dim3(CB_NT), 0, st, (long)N, (int)C, logits, (long)ld, y, temperature, (int)column, (int)M,
                     plan.per, part);
  if (int rc = check_launch("k_calib_rows")) return rc;
  hipLaunchKernelGGL(k_calib_finish, dim3(1), dim3(CB_NT), 0, st, (long)N, (int)M, plan.G, part, counts, table, summary);
  return check_launch("k_calib_finish");
}

extern "C" int rd_fit_temperature(int64_t N, int32_t C, const float* logits, int64_t ld, const int64_t* y, double* result, void* stream) {
  FitRoute r;
  if (!fit_route(N, C, &r))
    return fail(RD_EUNSUPPORTED, "rd_fit_temperature: N=%ld C=%d outside 1 <= N <= %d (one workgroup), 2 <= C <= %d", (long)N, C, FT_NMAX, CB_CMAX);
  RD_REQUIRE(ld >= C, "bad dims C=%d ld=%ld (C <= ld)", C, (long)ld);
  RD_REQUIRE(logits && y && result, "NULL tensor");
  hipStream_t st = (hipStream_t)stream;
  if (r.stage) {
    RD_LDS_ATTR(k_fit_temperature<true>, FT_LDS_STAGE);
    hipLaunchKernelGGL(k_fit_temperature<true>, dim3(1), dim3(FT_NT), r.lds, st, (int)N, (int)C, logits, (long)ld, y, result);
    return check_launch("k_fit_temperature<lds>");
  }
  hipLaunchKernelGGL(k_fit_temperature<false>, dim3(1), dim3(FT_NT), 0, st, (int)N, (int)C, logits, (long)ld, y, result);
  return check_launch("k_fit_temperature<global>");
}

// not part of the ABI (include/raindrop_hip_debug.h): 0: no fit stages its logits in LDS; 1, the default: fit_route's budget decides
extern "C" void rd_debug_set_calibration_stage(int on) { g_fit_stage_on = on ? 1 : 0; }

// not part of the ABI (include/raindrop_hip_debug.h): the form fit_route gives a fit of [N, C] logits; needs no device
extern "C" int rd_debug_calibration_route(int64_t N, int32_t C, uint32_t* bits) {
  RD_REQUIRE(bits, "NULL bits");
  *bits = 0;
  FitRoute r;
  if (!fit_route(N, C, &r))
    return fail(RD_EUNSUPPORTED, "rd_debug_calibration_route: N=%ld C=%d outside 1 <= N <= %d, 2 <= C <= %d", (long)N, C, FT_NMAX, CB_CMAX);
  *bits = (r.stage ? 1u : 0u) | ((uint32_t)r.lds << 8);
  return RD_OK;
}
