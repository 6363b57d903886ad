// rd_head.hip -- the classifier head of Raindrop_v2 with its loss, forward AND backward, in two launches.
//
//   agg[b]   = sum_t r[t,b,:] (1 - mask[b,t]) / (lengths[b] + 1)                 code/models_rd.py:366-367,379
//   feat[b]  = [agg[b] | emb(static[b])]                                          code/models_rd.py:381-384 (static model)
//   logits   = mlp_static(feat) = W2 relu(W0 feat + b0) + b2                      code/models_rd.py:385 (mlp_static: :263-267)
//   loss     = mean_b CrossEntropy(logits[b], y[b])                               code/Raindrop.py:255,322
// and every gradient of `loss`: dW0, db0, dW2, db2, d emb.weight, d emb.bias and dr [T,B,D] (the masked mean's backward,
// the entry gradient of the encoder stack).
//
// Why: the head is 256 rows x 186 features -- about 50 MFLOP -- but as separate operators it was 15 launches of
// latency-bound kernels (three forward products, the loss, two input-gradient and three weight-gradient products
// with their split-K reduces, the masked mean and its backward): ~114 us of a 0.85 ms step at ~4.5 us of fixed cost per
// launch.  Here a workgroup owns one sample (RB = 1; the template keeps the count) end to end:
//   k_head_rows   masked mean -> emb -> W0 (+ReLU) -> W2 -> softmax/loss -> dlogits -> dhid -> dfeat -> dr.
//                 W0 is read ONCE per workgroup, coalesced, into registers: wave w holds rows j = w, w+16, ... with lane l
//                 owning columns l, l+64, ...; the forward product reduces over lanes (one wave sum per output), the
//                 input gradient reuses the same registers and reduces over the 16 waves through LDS.  fp32 FMA
//                 arithmetic (at these sizes the matrix cores would idle behind the launch latency anyway).
//   k_head_wgrad  the three weight/bias gradients as 16 x 16 output tiles over the B rows (operands staged in LDS), and
//                 the mean of the per-sample losses -- all fixed-order sums, no atomics.
#include "rd_common.h"
#include "rd_plan.h"
#include "rd_trailing.h"

namespace rd {
namespace {

constexpr int HR_THR = 1024, HR_WAVES = 16;
constexpr int HR_RJ = 16, HR_KI = 4;               // most W0 rows per wave / 64-column slots per lane (dh <= 256); k_head_rows<RB, NRJ, NKI> fetches what dh needs
constexpr int HR_LD = 256;                         // row stride of the per-sample vectors in LDS
constexpr int HR_EMBW = 1024, HR_DS = 64;         // static embedding held in LDS when Fe * d_static <= 1024 and d_static <= 64 (else read in place)

struct HeadArgs {
  const float* r; const uint8_t* mask; const int64_t* lengths; const float* stat;
  const float *emb_w, *emb_b, *w0, *b0, *w2, *b2;
  const int64_t* y;
  float *logits, *dr;
  float *feat, *hid, *dhid, *demb, *dlog, *lossr;   // workspace: [B,dh] x3, [B,Fe], [B,C], [B]
  int T, B, D, ds, Fe, dh, C;
  const float* dlog_in;            // mode 2: d loss / d logits [B,C] from the caller (an autograd backward) instead of the cross entropy
  int mode;                        // 0: forward + loss + backward (rd_head_train); 1: forward only, logits out (rd_head_forward);
                                   // 2: forward recomputed + backward from dlog_in (rd_head_backward)
  const int32_t* plan;             // token plan (rd_plan.h) or null: r / dr hold the live rows only, sample b at rows off[rank[b]] + t
  unsigned long long* stamps;      // debug (tools/head_timing.py): clock64 per phase, thread 0 of workgroup 0
  int touch_bytes;                 // > 0: bytes of this kernel's own code requested into L2 at its start (rd_common.h touch_own_code)
  const float* crit;               // CRIT instantiations (rd_head_train_crit): [eps, w_0 .. w_{C-1}], the criterion's smoothing and class weights;
                                   // FOCAL instantiations (rd_head_train_focal): [gamma, w_0 .. w_{C-1}] -- the same size, the same load
};
static unsigned long long* g_head_stamps = nullptr;
#define HSTAMP(i)                                                                           \
  do {                                                                                      \
    if (a.stamps && blockIdx.x == 0 && threadIdx.x == 0) a.stamps[(i)] = clock64();         \
  } while (0)

// first row and row step of sample b's time steps in r / dr, and how many of them are live
struct HeadRows { long row0, rstep; int Tv; };
__device__ __forceinline__ HeadRows head_rows(const HeadArgs& a, int b) {
  HeadRows h;
  if (a.plan) {
    h.row0 = a.plan[plan::brow_base(a.B, a.T) + b]; h.rstep = 1; h.Tv = a.plan[plan::blen_base(a.B, a.T) + b];
  } else { h.row0 = b; h.rstep = a.B; h.Tv = a.T; }
  return h;
}

// the same for a workgroup-uniform sample, through the scalar cache, from the plan's by-sample arrays (brow / blen: ONE round trip;
// off[rank[b]] was two dependent ones)
__device__ __forceinline__ HeadRows head_rows_uniform(const HeadArgs& a, int b) {
  HeadRows h;
  if (a.plan) {
    int row0, tv;
    load_uniform_2xi32(a.plan + plan::brow_base(a.B, a.T) + b, a.plan + plan::blen_base(a.B, a.T) + b, row0, tv);
    h.row0 = row0; h.rstep = 1; h.Tv = tv;
  } else { h.row0 = b; h.rstep = a.B; h.Tv = a.T; }
  return h;
}

__device__ __forceinline__ float wsum64(float v) { return wave_sum64_dpp(v); }

// NRJ / NKI: W0 rows per wave and 64-column slots per lane that are actually FETCHED (16 NRJ >= dh, 64 NKI >= dh).  The generic
// <16, 4> form requests 256 x 256 clamped elements whatever dh is -- at P19 (dh = 186) 262 KB of address-unit traffic for a 138-KB
// matrix, and that request phase was the first 5.7 k of the kernel's 30 k cycles (tools/head_timing.py); <12, 3> requests 192 x 192.
// CRIT: torch's CrossEntropyLoss(weight = w, label_smoothing = eps), mean reduction, in place of the plain mean cross entropy
// (rd_head_train_crit; mode 0 only).  An instantiation, not a branch in front of the loss block (DESIGN rule 40): the CRIT = false
// kernels are the kernels as they were.  A workgroup owns one sample but the mean's denominator W = sum_b w[y_b] belongs to the
// batch: EVERY workgroup counts the labels per class (wave ballots -- integers, no order to fix) and forms
// W = sum over c ascending of n_c w_c, so all workgroups and any two launches get the same bits with no atomics and no ticket.
// FORM (the kernels below instantiate this body): HEAD_PLAIN, HEAD_CRIT, or HEAD_FOCAL -- the focal loss
//   loss = sum_b w[y_b] q_b^gamma (-log p[b,y_b]) / W,   q_b = sum over c != y_b ascending of p[b,c]      (rd_common.h focal_factors)
// on CRIT's label count and W (crs[0] carries gamma in place of eps): a third instantiation with a loss block of its own.  At
// gamma = 0 both focal factors are an exact 1.0f and every output is the CRIT form's at eps = 0.
constexpr int HEAD_PLAIN = 0, HEAD_CRIT = 1, HEAD_FOCAL = 2;
template <int RB, int NRJ, int NKI, int FORM>
__device__ __forceinline__ void head_rows_body(const HeadArgs& a) {
  constexpr bool CRIT = FORM != HEAD_PLAIN;          // the batch-wide label count and n_c w_c: both criterion forms
  __shared__ __attribute__((aligned(16))) float feat[RB][HR_LD], hid[RB][HR_LD], dhid[RB][HR_LD], dfeat[RB][HR_LD];
  __shared__ __attribute__((aligned(16))) float red[HR_WAVES * RB * HR_LD];     // mean-phase and wave partials
  __shared__ float lg[RB][16], dl[RB][16], invl[RB], b0s[HR_LD];
  // every small operand of the later phases, fetched ONCE at the top beside W0: as global loads inside their phases (static
  // embedding: d_static dependent steps of two loads; logits: three; the label; W2 again in the gradient) they were ~17 dependent
  // round trips during which the workgroup's other waves sat at the next barrier (SQ counters: 80 % of the wave cycles waiting)
  __shared__ float w2s[16 * HR_LD], embb[HR_LD], b2s[16], embws[HR_EMBW], stats[RB][HR_DS];
  __shared__ long long ys[RB];
  __shared__ int cntw[CRIT ? HR_WAVES : 1][16];      // CRIT: labels per (wave, class) of the whole batch
  __shared__ float crs[CRIT ? 17 : 1], nws[CRIT ? 16 : 1];   // CRIT: [eps, w_0 ..]; n_c w_c
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b0 = blockIdx.x * RB;
  const int T = a.T, B = a.B, D = a.D, dh = a.dh, C = a.C, D4 = D >> 2;

  HSTAMP(0);
  RD_TOUCH_CODE(a.touch_bytes);
  // Request order = the order the data is NEEDED (vector memory returns in order): small operands (they go out while the plan
  // look-up is on its way through the scalar cache), the sample's rows for the masked mean, then W0, which nothing reads before
  // the mean is reduced.  Round 3 had W0 first: the mean then waited for all of W0 (10.4 k cycles into the kernel).
  // ---- small operands: ALL requests first (unconditional, clamped indices), stored to LDS below.  Written as `if (tid < n) lds[tid] =
  // g[tid];` per array each was its own load -> wait -> store block: seven dependent round trips at the top of the kernel.
  const bool emb_lds = a.Fe > 0 && a.Fe * a.ds <= HR_EMBW && a.ds <= HR_DS;
  const int nw2 = C * dh;
  const float pb0 = a.b0[min(tid, dh - 1)], pw2 = a.w2[min(tid, nw2 - 1)], pb2 = a.b2[min(tid, C - 1)];
  const long long py = a.mode == 0 ? a.y[min(b0 + min(tid, RB - 1), B - 1)] : 0;   // uniform
  long long pyl = 0; float pcr = 0.f;
  if constexpr (CRIT) { pyl = a.y[min(tid, B - 1)]; pcr = a.crit[min(tid, C)]; }   // the batch's labels (first 1024), the criterion
  float pew = 0.f, peb = 0.f, pst = 0.f;
  if (emb_lds) {                                     // uniform
    const int ne = a.Fe * a.ds, ns = RB * a.ds, ts = min(tid, ns - 1), rs = ts / a.ds;
    pew = a.emb_w[min(tid, ne - 1)]; peb = a.emb_b[min(tid, a.Fe - 1)];
    pst = a.stat[(long)min(b0 + rs, B - 1) * a.ds + (ts - rs * a.ds)];
  }
  // ---- masked mean: thread = (sample r, column quad c4, time group tg); four steps per pass requested together (clamped rows, the
  // step's validity applied to the value).  Threads beyond the ntg groups request a duplicate and add nothing.
  const int P = RB * D4;
  const int ntg = min(HR_THR / P, 16);
  const int pair = tid % P, tg = tid / P;
  const int mr = pair / D4, mc4 = pair - mr * D4, mb = b0 + mr;
  const bool mlive = tg < ntg && mb < B;
  // the sample's length (for 1 / (len + 1)) and its rows.  One sample per workgroup: three scalar loads behind ONE wait -- as a
  // vector load of a uniform address the compiler read the length back with v_readfirstlane at once, i.e. behind `vmcnt(0)`.
  long long plen; HeadRows hr;
  if (RB == 1) {
    const int bu = __builtin_amdgcn_readfirstlane(b0);                 // b0 < B: the grid is B workgroups
    uint64_t lv; int row0 = bu, tv = T;
    if (a.plan) load_uniform_u64_2xi32(reinterpret_cast<const uint64_t*>(a.lengths) + bu, a.plan + plan::brow_base(B, T) + bu,
                                       a.plan + plan::blen_base(B, T) + bu, lv, row0, tv);
    else lv = load_uniform_u64(reinterpret_cast<const uint64_t*>(a.lengths) + bu);
    plen = (long long)lv;
    hr.row0 = row0; hr.rstep = a.plan ? 1 : B; hr.Tv = tv;
  } else {
    plen = a.lengths[min(b0 + min(tid, RB - 1), B - 1)];
    hr = head_rows(a, min(mb, B - 1));
  }
  float4 mv[4]; bool mok[4]; unsigned char mk[4] = {0, 0, 0, 0};
  auto request_rows = [&](int t0) {
    if (!a.plan) {                                                     // uniform: the padded layout's per-step mask bytes
#pragma unroll
      for (int u = 0; u < 4; ++u) mk[u] = a.mask[(long)min(mb, B - 1) * T + min(t0 + u * ntg, T - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u * ntg, tc = max(min(t, hr.Tv - 1), 0);
      mok[u] = mlive && t < hr.Tv;
      const long row = mok[u] ? hr.row0 + (long)tc * hr.rstep : 0;     // row 0 of r always exists
      mv[u] = *reinterpret_cast<const float4*>(a.r + row * D + 4 * mc4);
    }
  };
  request_rows(min(tg, ntg - 1));
  __builtin_amdgcn_sched_barrier(0);                       // the rows' requests stay IN FRONT of W0's (the fourth was moved behind them)
  // ---- W0 rows of this wave -> registers.  UNCONDITIONAL loads from clamped addresses: rows j >= dh are never used and columns
  // k >= dh only meet zeros (hid) or reach accumulator slots nobody reads (dfeat).  As conditional loads (a phi of {0, value} each)
  // the compiler waited for them one group at a time -- two dozen dependent round trips at the head of a kernel whose 256
  // workgroups all run at once, so its duration IS one workgroup's latency chain.
  float w[NRJ][NKI];
#pragma unroll
  for (int jj = 0; jj < NRJ; ++jj) {
    const int jc = min(wave + HR_WAVES * jj, dh - 1);
#pragma unroll
    for (int i = 0; i < NKI; ++i) w[jj][i] = a.w0[(long)jc * dh + min(lane + 64 * i, dh - 1)];
  }
  HSTAMP(1);
  // ---- small operands -> LDS ----
  {
    if (tid < HR_LD) b0s[tid] = pb0;
    if (tid < nw2) w2s[tid] = pw2;
    if (tid < C) b2s[tid] = pb2;
    if (tid < RB) ys[tid] = py;
    if (emb_lds) {
      const int ne = a.Fe * a.ds;
      if (tid < ne) embws[tid] = pew;
      if (tid < a.Fe) embb[tid] = peb;
      if (tid < RB * a.ds) stats[tid / a.ds][tid % a.ds] = pst;
      for (int i = tid + HR_THR; i < ne; i += HR_THR) embws[i] = a.emb_w[i];          // HR_EMBW <= HR_THR: never runs; kept for safety
    }
    for (int i = tid + HR_THR; i < nw2; i += HR_THR) w2s[i] = a.w2[i];                // C * dh > 1024 only
    if (tid < RB) invl[tid] = (b0 + tid < B) ? 1.0f / (float)(plen + 1) : 0.f;
    if constexpr (CRIT) {
      if (tid <= C) crs[tid] = pcr;
      // lane c of every wave counts the wave's labels equal to c (labels outside [0, C) are counted nowhere)
      // The first 1024 labels (in flight since the top) are NOT an iteration of the loop behind them: a loop with a load inside
      // waits for everything outstanding -- all of W0 -- before its first use, whatever its trip count (as for the rows below).
      int cn = 0;
      for (int c = 0; c < C; ++c) {
        const int n = __popcll(__ballot(tid < B && pyl == c));
        if (lane == c) cn += n;
      }
      for (int bb = HR_THR; bb < B; bb += HR_THR) {        // uniform; B > 1024 only
        const long long yv = a.y[min(bb + tid, B - 1)];
        for (int c = 0; c < C; ++c) {
          const int n = __popcll(__ballot(bb + tid < B && yv == c));
          if (lane == c) cn += n;
        }
      }
      if (lane < 16) cntw[wave][lane] = cn;
    }
  }
  // ---- the rows: first pass (in flight since the top), further passes for T > 4 ntg steps ----
  {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    // the first pass is NOT a loop iteration: inside one loop the waits are computed for the back edge (only that pass's four
    // requests outstanding = vmcnt(0) at the last use), which on entry would also wait for all of W0
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (mok[u] && !mk[u]) { s.x += mv[u].x; s.y += mv[u].y; s.z += mv[u].z; s.w += mv[u].w; }
    for (int pass = 1; pass * 4 * ntg < T; ++pass) {       // T > 4 ntg steps only (uniform trip count; the flags drop steps past the sample's length)
      request_rows(min(tg, ntg - 1) + pass * 4 * ntg);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (mok[u] && !mk[u]) { s.x += mv[u].x; s.y += mv[u].y; s.z += mv[u].z; s.w += mv[u].w; }
    }
    if (tg < ntg) *reinterpret_cast<float4*>(red + ((size_t)tg * P + pair) * 4) = s;
  }
  HSTAMP(2);
  lds_barrier();                                           // LDS only: W0 stays in flight (no thread reads global memory another wrote)
  HSTAMP(3);
  if constexpr (CRIT) {                                    // the last wave (idle in the mean's second half): n_c w_c per class
    if (tid >= HR_THR - 64 && lane < C) {
      int n = 0;
#pragma unroll
      for (int q = 0; q < HR_WAVES; ++q) n += cntw[q][lane];
      nws[lane] = (float)n * crs[1 + lane];
    }
  }
  if (tid < P) {
    const int r = tid / D4, c4 = tid - r * D4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g = 0; g < ntg; ++g) {
      const float4 v = *reinterpret_cast<const float4*>(red + ((size_t)g * P + tid) * 4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float il = invl[r];
    *reinterpret_cast<float4*>(&feat[r][4 * c4]) = make_float4(s.x * il, s.y * il, s.z * il, s.w * il);
  }
  // ---- static embedding into the right block (code/models_rd.py:381): thread = (r, j) ----
  for (int e = tid; e < RB * a.Fe; e += HR_THR) {         // (the prefetched operands were stored before the barrier above)
    const int r = e / a.Fe, j = e - r * a.Fe, b = b0 + r;
    float s;
    if (emb_lds) {
      s = embb[j];
      if (b < B)
        for (int q = 0; q < a.ds; ++q) s += stats[r][q] * embws[j * a.ds + q];
    } else {
      s = a.emb_b[j];
      if (b < B)
        for (int q = 0; q < a.ds; ++q) s += a.stat[(long)b * a.ds + q] * a.emb_w[(long)j * a.ds + q];
    }
    feat[r][D + j] = s;
  }
  lds_barrier();
  HSTAMP(4);
  // ---- hid = relu(W0 feat + b0): wave w owns outputs j = w, w+16, ...; lanes split the reduction.  Branch-free over the wave's
  // rows: behind `if (j < dh)` every row was its own basic block and the NRJ wave sums (six dependent DPP steps each) ran one after
  // the other -- 7.3 k cycles for 16 rows; as straight-line code the scheduler interleaves the independent chains. ----
  {
    float fv[RB][NKI];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int i = 0; i < NKI; ++i) {
        const int k = lane + 64 * i;
        const float f = feat[r][k];                        // k < HR_LD always; columns >= dh hold nothing
        fv[r][i] = k < dh ? f : 0.f;
      }
    float ps[NRJ][RB];
#pragma unroll
    for (int jj = 0; jj < NRJ; ++jj)
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        float p = 0.f;
#pragma unroll
        for (int i = 0; i < NKI; ++i) p += fv[r][i] * w[jj][i];
        ps[jj][r] = p;
      }
    // the wave sums step by step ACROSS the rows (rd_common.h wave_sum64_dpp, same order of additions per row): as NRJ calls in a
    // row the chains were emitted one after the other on one register
#define HR_DPP_STEP(ctrl, rmask)                                                                                              \
  _Pragma("unroll") for (int jj = 0; jj < NRJ; ++jj) _Pragma("unroll") for (int r = 0; r < RB; ++r)                           \
    ps[jj][r] += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, ps[jj][r]), ctrl, rmask, 0xf, false))
    HR_DPP_STEP(0x111, 0xf); HR_DPP_STEP(0x112, 0xf); HR_DPP_STEP(0x114, 0xf); HR_DPP_STEP(0x118, 0xf);
    HR_DPP_STEP(0x142, 0xa); HR_DPP_STEP(0x143, 0xc);
#undef HR_DPP_STEP
#pragma unroll
    for (int jj = 0; jj < NRJ; ++jj)
#pragma unroll
      for (int r = 0; r < RB; ++r) ps[jj][r] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ps[jj][r]), 63));
#pragma unroll
    for (int jj = 0; jj < NRJ; ++jj) {
      const int j = wave + HR_WAVES * jj;
      if (lane == 0 && j < dh) {
#pragma unroll
        for (int r = 0; r < RB; ++r) hid[r][j] = fmaxf(ps[jj][r] + b0s[j], 0.f);
      }
    }
  }
  lds_barrier();
  HSTAMP(5);
  // ---- logits: wave = (r, c) ----
  for (int o = wave; o < RB * C; o += HR_WAVES) {
    const int r = o / C, c = o - r * C;
    float p = 0.f;
    for (int k = lane; k < dh; k += 64) p += hid[r][k] * w2s[c * dh + k];
    p = wsum64(p);
    if (lane == 0) lg[r][c] = p + b2s[c];
  }
  lds_barrier();
  HSTAMP(6);
  if (a.mode == 1) {                                   // rd_head_forward: the logits are the result
    if (tid < RB * C && b0 + tid / C < B) a.logits[(long)(b0 + tid / C) * C + tid % C] = lg[tid / C][tid % C];
    return;
  }
  // ---- softmax cross entropy per sample, dlogits = (softmax - onehot) / B ----
  if (a.mode == 2) {                                   // rd_head_backward: d loss / d logits comes from the caller
    if (tid < RB * C) {
      const int r = tid / C, c = tid - r * C, b = b0 + r;
      const float d = b < B ? a.dlog_in[(long)b * C + c] : 0.f;
      dl[r][c] = d;
      if (b < B) a.dlog[(long)b * C + c] = d;
    }
  } else if (tid < RB && b0 + tid < B) {
    const int r = tid, b = b0 + r;
    float m = lg[r][0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, lg[r][c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(lg[r][c] - m);
    const float lse = m + logf(se);
    // a label outside [0, C) has no logit to index (torch raises): the sample's loss becomes NaN -- loud, and no out-of-bounds read
    const long yb = (long)ys[r];
    const bool yok = yb >= 0 && yb < C;
    const int t = yok ? (int)yb : 0;
    if constexpr (FORM == HEAD_FOCAL) {
      // loss = sum_b w[y_b] m_b nll_b / W, dlogits = (p - onehot) g_b w[y_b] / W with the factors m_b, g_b of focal_factors.  The
      // factor order is the CRIT block's below: m_b multiplies w[y_b] nll_b where (1 - eps) does, g_b multiplies (p - onehot)
      // where (1 - eps) does, w[y_b] (1 / W) stays the last factor -- at gamma = 0 (m_b = g_b = 1.0f) the CRIT form's bits at
      // eps = 0, whose smoothing terms are exact zeros.
      const float gamma = crs[0];
      float Wn = 0.f;
      for (int c = 0; c < C; ++c) Wn += nws[c];
      const float invW = 1.0f / Wn, wy = crs[1 + t], fy = wy * invW;
      const float nll = lse - lg[r][t];
      float q = 0.f, py = 0.f;
      for (int c = 0; c < C; ++c) {
        const float p = expf(lg[r][c] - lse);
        if (c == t) py = p; else q += p;
      }
      float mf, gf;
      focal_factors(gamma, q, py, nll, mf, gf);
      const float term = mf * (wy * nll);
      a.lossr[b] = yok ? term * ((float)B / Wn) : __builtin_nanf("");
      for (int c = 0; c < C; ++c) {
        const float p = expf(lg[r][c] - lse);
        const float d = ((p - (c == t ? 1.f : 0.f)) * gf) * fy;
        dl[r][c] = d;
        a.dlog[(long)b * C + c] = d;
        a.logits[(long)b * C + c] = lg[r][c];
      }
    } else if constexpr (CRIT) {
      // loss = (1 - eps) sum_b w[y_b] nll_b / W + (eps / C) sum_b sum_c w_c (-log p[b,c]) / W,  W = sum_b w[y_b] = sum_c n_c w_c.
      // w[y_b] (1 / W) is the LAST factor of the plain term: at eps = 0, w = 1 it is 1.0f / B and the smoothing term an exact zero,
      // i.e. dlogits are the plain kernel's bits.  The per-sample term leaves scaled by B / W (exactly 1 there): the trailing
      // launch's sum / B (head_wgrad_body, unchanged) is then the weighted mean.
      const float eps = crs[0];
      float Wn = 0.f, sw = 0.f, sm = 0.f;
      for (int c = 0; c < C; ++c) { Wn += nws[c]; sw += crs[1 + c]; sm += crs[1 + c] * (lse - lg[r][c]); }
      const float invW = 1.0f / Wn, wy = crs[1 + t], fy = wy * invW;
      const float ome = 1.0f - eps, ec = eps / (float)C, es = ec * invW;
      const float term = ome * (wy * (lse - lg[r][t])) + ec * sm;
      a.lossr[b] = yok ? term * ((float)B / Wn) : __builtin_nanf("");
      for (int c = 0; c < C; ++c) {
        const float p = expf(lg[r][c] - lse);
        const float d = (ome * (p - (c == t ? 1.f : 0.f))) * fy + es * (p * sw - crs[1 + c]);
        dl[r][c] = d;
        a.dlog[(long)b * C + c] = d;
        a.logits[(long)b * C + c] = lg[r][c];
      }
    } else {
    a.lossr[b] = yok ? lse - lg[r][t] : __builtin_nanf("");
    const float invB = 1.0f / (float)B;
    for (int c = 0; c < C; ++c) {
      const float d = (expf(lg[r][c] - lse) - (c == t ? 1.f : 0.f)) * invB;
      dl[r][c] = d;
      a.dlog[(long)b * C + c] = d;
      a.logits[(long)b * C + c] = lg[r][c];
    }
    }
  } else if (tid < RB) {
    for (int c = 0; c < C; ++c) dl[tid][c] = 0.f;
  }
  lds_barrier();
  HSTAMP(7);
  // ---- dhid = (dlogits W2) gated by hid > 0: thread = (r, j); rows out to the workspace for the weight gradients ----
  for (int e = tid; e < RB * dh; e += HR_THR) {
    const int r = e / dh, j = e - r * dh, b = b0 + r;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += dl[r][c] * w2s[c * dh + j];
    const float h = hid[r][j];
    s = h > 0.f ? s : 0.f;
    dhid[r][j] = s;
    if (b < B) {
      a.dhid[(long)b * dh + j] = s;
      a.hid[(long)b * dh + j] = h;
      a.feat[(long)b * dh + j] = feat[r][j];
    }
  }
  lds_barrier();
  HSTAMP(8);
  // ---- dfeat = dhid W0: the same registers; this wave's rows give a partial for every column, waves combined in order ----
  {
    float acc[RB][NKI];
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int i = 0; i < NKI; ++i) acc[r][i] = 0.f;
#pragma unroll
    for (int jj = 0; jj < NRJ; ++jj) {
      const int j = wave + HR_WAVES * jj;                  // < HR_LD; rows >= dh contribute zero (their W0 registers hold a clamped duplicate)
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const float dv = dhid[r][j];
        const float d = j < dh ? dv : 0.f;
#pragma unroll
        for (int i = 0; i < NKI; ++i) acc[r][i] += d * w[jj][i];
      }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
      for (int i = 0; i < NKI; ++i) red[((size_t)wave * RB + r) * HR_LD + lane + 64 * i] = acc[r][i];
  }
  lds_barrier();
  HSTAMP(9);
  for (int e = tid; e < RB * HR_LD; e += HR_THR) {
    const int r = e / HR_LD, k = e - r * HR_LD;
    float s = 0.f;
    if (k < 64 * NKI) {                                    // columns beyond the fetched slots were never written (and are >= dh)
#pragma unroll
      for (int q = 0; q < HR_WAVES; ++q) s += red[((size_t)q * RB + r) * HR_LD + k];
    }
    dfeat[r][k] = s;
    const int b = b0 + r;
    if (k >= D && k < dh && b < B) a.demb[(long)b * a.Fe + (k - D)] = s;   // gradient of the static embedding's output
  }
  lds_barrier();
  HSTAMP(10);
  // ---- masked mean backward: dr[t,b,:] = valid ? dfeat[b,:D] / (len + 1) : 0   (code/models_rd.py:379, autograd) ----
  for (int e = tid; e < RB * T * D4; e += HR_THR) {
    const int c4 = e % D4, rt = e / D4;
    const int t = rt % T, r = rt / T, b = b0 + r;
    if (b >= B) continue;
    const HeadRows hq = RB == 1 ? hr : head_rows(a, b);                  // RB == 1: the look-up of the top of the kernel
    if (t >= hq.Tv) continue;                                           // token plan: padded steps have no row
    const float il = (!a.plan && a.mask[(long)b * T + t]) ? 0.f : invl[r];
    const float4 v = *reinterpret_cast<const float4*>(&dfeat[r][4 * c4]);
    *reinterpret_cast<float4*>(a.dr + (hq.row0 + (long)t * hq.rstep) * D + 4 * c4) = make_float4(v.x * il, v.y * il, v.z * il, v.w * il);
  }
  HSTAMP(11);
}

// the kernels: plain / CRIT as they were (the template flag the launch sites and the build's touch sites name), FOCAL beside them
template <int RB, int NRJ, int NKI, bool CRIT>
__global__ __launch_bounds__(HR_THR) void k_head_rows(HeadArgs a) {
  head_rows_body<RB, NRJ, NKI, CRIT ? HEAD_CRIT : HEAD_PLAIN>(a);
}
template <int RB, int NRJ, int NKI>
__global__ __launch_bounds__(HR_THR) void k_head_rows_focal(HeadArgs a) {
  head_rows_body<RB, NRJ, NKI, HEAD_FOCAL>(a);
}

// dW[n,k] = sum_b u[b,n] v[b,k], db[n] = sum_b u[b,n]: 16 x 16 output tile per workgroup, thread = one output (rd_trailing.h)
__global__ __launch_bounds__(256) void k_head_wgrad(HwArgs a) {
  __shared__ float us[256][16], vs[256][17];
  head_wgrad_body(a, (int)blockIdx.x, (int)threadIdx.x, us, vs);
}

}  // namespace
}  // namespace rd

using namespace rd;

namespace rd {
int launch_head_wgrad_standalone(const HwArgs& h, hipStream_t st) {
  hipLaunchKernelGGL(k_head_wgrad, dim3(h.ntiles), dim3(256), 0, st, h);
  return check_launch("k_head_wgrad");
}
}  // namespace rd

extern "C" void rd_debug_set_head_stamps(void* p) { g_head_stamps = (unsigned long long*)p; }   // not part of the ABI

extern "C" size_t rd_head_train_workspace_bytes(int32_t B, int32_t dh, int32_t C) {
  if (B < 0 || dh <= 0 || C <= 0) return 0;
  return align_up(((size_t)4 * B * dh + (size_t)B * C + B) * sizeof(float), 256);
}

extern "C" int rd_head_train_supported(int32_t D, int32_t Fe, int32_t C) {
  const char* e = getenv("RD_HEAD_FUSED");
  if (e && atoi(e) == 0) return 0;
  return (D % 4) == 0 && D > 0 && Fe >= 0 && D + Fe <= 256 && C >= 1 && C <= 16 && 2 * (D / 4) <= HR_THR;
}

static int head_launch(int mode, const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                       const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w, const float* emb_b,
                       const float* w0, const float* b0, const float* w2, const float* b2, const int64_t* y, const float* crit,
                       int form, const float* dlog_in, float* loss, float* logits, float* g_emb_w, float* g_emb_b, float* g_w0, float* g_b0, float* g_w2,
                       float* g_b2, float* dr, void* workspace, size_t workspace_bytes, void* stream);

// ---- the route: every decision of one head call, taken ONCE, from the sizes alone (head_launch runs it; rd_debug_head_route,
// include/raindrop_hip_debug.h, reports it) ----
struct HeadRoute {
  bool narrow;                     // k_head_rows<1, 12, 3, .>: W0 fetched as 192 x 192; else <1, 16, 4, .>: 256 x 256
  bool crit;                       // the CRIT instantiations
  bool focal;                      // the FOCAL instantiations (never with crit)
  bool emb_lds;                    // the static embedding's operands are staged in LDS (else read in place)
  int touch_bytes;                 // own-code touch of the instantiation (0: RD_CODE_TOUCH=0)
  int grid;                        // workgroups of k_head_rows: one sample each
  int njobs;                       // trailing launch: weight-gradient jobs (0: rd_head_forward has none) -- d mlp_static[0], [2], d emb
  struct { int N, K, tiles_n, tiles_k, blk0; } job[3];
  int ntiles;                      // workgroups of k_head_wgrad: 16 x 16 output tiles over all jobs
  int rider_blocks;                // 1024-thread blocks of the deferred form (rd_trailing.h: four tiles per block)
  const char* name;                // what the launch reports to the error check and the launch log
};

// one name per instantiation: the launch log tells the six k_head_rows apart
static const char* head_name(const HeadRoute& r) {
  if (r.focal) return r.narrow ? "k_head_rows<12,3,focal>" : "k_head_rows<16,4,focal>";
  if (r.crit) return r.narrow ? "k_head_rows<12,3,crit>" : "k_head_rows<16,4,crit>";
  return r.narrow ? "k_head_rows<12,3>" : "k_head_rows<16,4>";
}

static HeadRoute head_route(int mode, int B, int D, int d_static, int Fe, int C, int form) {
  // own-code touch: 14.5 KB of the 15.4 KB <1, 12, 3> kernel, 16 KB of the 16.9 KB generic one (tests/test_kernel_resources.py keeps the
  // constants below the code lengths); RD_CODE_TOUCH=0 switches it off (A/B)
  static const int touch = [] { const char* e = getenv("RD_CODE_TOUCH"); return e ? atoi(e) : 1; }();
  // one sample per workgroup (B workgroups: every CU busy at B = 256); two samples per workgroup measured inside the noise twice
  // (rounds 2 and 4) and is no longer built (its hid phase spilled at 128 registers).
  // W0 fetched as 192 x 192 where that covers it (P19: dh = 186), else 256 x 256 (RD_HEAD_NARROW=0: always the latter)
  static const int narrow = [] { const char* e = getenv("RD_HEAD_NARROW"); return e ? atoi(e) : 1; }();
  const int dh = D + Fe;
  HeadRoute r{};
  r.narrow = narrow && dh <= 192;
  const bool crit = form == HEAD_CRIT, focal = form == HEAD_FOCAL;
  r.crit = crit; r.focal = focal;                                      // the criterion / focal instantiations: touch lengths of their own
  // the kernel's own predicate (k_head_rows: `const bool emb_lds = ...`), restated: the kernel bodies are not touched by the route
  r.emb_lds = Fe > 0 && Fe * d_static <= HR_EMBW && d_static <= HR_DS;
  r.touch_bytes = !touch ? 0 : focal ? (r.narrow ? RD_TL_HEAD_P19_F : RD_TL_HEAD_F) : crit ? (r.narrow ? RD_TL_HEAD_P19_C : RD_TL_HEAD_C) : (r.narrow ? RD_TL_HEAD_P19 : RD_TL_HEAD);
  r.grid = B;
  r.name = head_name(r);
  if (mode == 1) return r;                                             // rd_head_forward: the logits are the result
  int blk = 0;
  auto add = [&](int N, int K) {
    auto& J = r.job[r.njobs++];
    J.N = N; J.K = K; J.tiles_n = cdiv(N, 16); J.tiles_k = cdiv(K, 16); J.blk0 = blk; blk += J.tiles_n * J.tiles_k;
  };
  add(dh, dh);                                                         // d mlp_static[0]
  add(C, dh);                                                          // d mlp_static[2]
  if (Fe) add(Fe, d_static);                                           // d emb
  r.ntiles = blk; r.rider_blocks = cdiv(blk, 4);
  return r;
}

extern "C" int rd_head_train(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                             const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                             const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                             const int64_t* y, float* loss, float* logits, float* g_emb_w, float* g_emb_b, float* g_w0,
                             float* g_b0, float* g_w2, float* g_b2, float* dr, void* workspace, size_t workspace_bytes,
                             void* stream) {
  RD_REQUIRE(y && loss && logits && g_w0 && g_b0 && g_w2 && g_b2 && dr, "NULL tensor");
  return head_launch(0, s, D, d_static, Fe, C, r, mask, lengths, stat, emb_w, emb_b, w0, b0, w2, b2, y, nullptr, HEAD_PLAIN, nullptr, loss, logits,
                     g_emb_w, g_emb_b, g_w0, g_b0, g_w2, g_b2, dr, workspace, workspace_bytes, stream);
}

// rd_head_train with torch's CrossEntropyLoss(weight = w, label_smoothing = eps), mean reduction, as the loss: crit = [eps, w_0 ..
// w_{C-1}] on the device, read when the kernel RUNS (a captured step changes its criterion by a copy into that buffer).
extern "C" int rd_head_train_crit(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                                  const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                                  const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                                  const int64_t* y, const float* crit, float* loss, float* logits, float* g_emb_w, float* g_emb_b,
                                  float* g_w0, float* g_b0, float* g_w2, float* g_b2, float* dr, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  RD_REQUIRE(y && crit && loss && logits && g_w0 && g_b0 && g_w2 && g_b2 && dr, "NULL tensor");
  RD_REQUIRE(s && s->B < (1 << 24), "head_train_crit: B must be below 2^24 (per-class label counts are carried as floats)");
  return head_launch(0, s, D, d_static, Fe, C, r, mask, lengths, stat, emb_w, emb_b, w0, b0, w2, b2, y, crit, HEAD_CRIT, nullptr, loss, logits,
                     g_emb_w, g_emb_b, g_w0, g_b0, g_w2, g_b2, dr, workspace, workspace_bytes, stream);
}

// rd_head_train with the focal loss (rd_softmax_xent_focal's formulas) as the loss: crit = [gamma, w_0 .. w_{C-1}] on the device,
// read when the kernel RUNS.  gamma = 0: every output is rd_head_train_crit's at eps = 0.
extern "C" int rd_head_train_focal(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                                   const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                                   const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                                   const int64_t* y, const float* crit, float* loss, float* logits, float* g_emb_w, float* g_emb_b,
                                   float* g_w0, float* g_b0, float* g_w2, float* g_b2, float* dr, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  RD_REQUIRE(y && crit && loss && logits && g_w0 && g_b0 && g_w2 && g_b2 && dr, "NULL tensor");
  RD_REQUIRE(s && s->B < (1 << 24), "head_train_focal: B must be below 2^24 (per-class label counts are carried as floats)");
  return head_launch(0, s, D, d_static, Fe, C, r, mask, lengths, stat, emb_w, emb_b, w0, b0, w2, b2, y, crit, HEAD_FOCAL, nullptr, loss,
                     logits, g_emb_w, g_emb_b, g_w0, g_b0, g_w2, g_b2, dr, workspace, workspace_bytes, stream);
}

// The same head as two calls around a loss the CALLER evaluates (the reference's training loop: `criterion(outputs, y)` in
// code/Raindrop.py:319-322, then loss.backward()): rd_head_forward stops at the logits; rd_head_backward recomputes the forward
// phases (a masked mean and two small products: cheaper than saving and re-reading them) and continues from the caller's
// d loss / d logits.  Same kernel, same arithmetic, same workspace as rd_head_train.
extern "C" int rd_head_forward(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                               const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                               const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                               float* logits, void* workspace, size_t workspace_bytes, void* stream) {
  RD_REQUIRE(logits, "NULL tensor");
  return head_launch(1, s, D, d_static, Fe, C, r, mask, lengths, stat, emb_w, emb_b, w0, b0, w2, b2, nullptr, nullptr, HEAD_PLAIN, nullptr, nullptr, logits,
                     nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}
extern "C" int rd_head_backward(const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                                const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w,
                                const float* emb_b, const float* w0, const float* b0, const float* w2, const float* b2,
                                const float* dlogits, float* g_emb_w, float* g_emb_b, float* g_w0, float* g_b0, float* g_w2,
                                float* g_b2, float* dr, void* workspace, size_t workspace_bytes, void* stream) {
  RD_REQUIRE(dlogits && g_w0 && g_b0 && g_w2 && g_b2 && dr, "NULL tensor");
  return head_launch(2, s, D, d_static, Fe, C, r, mask, lengths, stat, emb_w, emb_b, w0, b0, w2, b2, nullptr, nullptr, HEAD_PLAIN, dlogits, nullptr, nullptr,
                     g_emb_w, g_emb_b, g_w0, g_b0, g_w2, g_b2, dr, workspace, workspace_bytes, stream);
}

static int head_launch(int mode, const rd_shape* s, int32_t D, int32_t d_static, int32_t Fe, int32_t C, const float* r,
                       const uint8_t* mask, const int64_t* lengths, const float* stat, const float* emb_w, const float* emb_b,
                       const float* w0, const float* b0, const float* w2, const float* b2, const int64_t* y, const float* crit,
                       int form, const float* dlog_in, float* loss, float* logits, float* g_emb_w, float* g_emb_b, float* g_w0, float* g_b0, float* g_w2,
                       float* g_b2, float* dr, void* workspace, size_t workspace_bytes, void* stream) {
  RD_REQUIRE(s && s->T > 0 && s->B > 0, "bad shape");
  RD_REQUIRE(rd_head_train_supported(D, Fe, C), "head_train: unsupported sizes D=%d Fe=%d C=%d", D, Fe, C);
  RD_REQUIRE(r && mask && lengths && w0 && b0 && w2 && b2 && workspace, "NULL tensor");
  RD_REQUIRE(Fe == 0 || (stat && emb_w && emb_b && d_static > 0 && (mode == 1 || (g_emb_w && g_emb_b))), "static embedding tensors missing");
  const int B = s->B, dh = D + Fe;
  RD_REQUIRE(workspace_bytes >= rd_head_train_workspace_bytes(B, dh, C), "workspace too small");
  RD_REQUIRE((reinterpret_cast<uintptr_t>(r) & 15) == 0 && (reinterpret_cast<uintptr_t>(dr) & 15) == 0, "r / dr must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  HeadArgs a{};
  a.r = r; a.mask = mask; a.lengths = lengths; a.stat = stat; a.emb_w = emb_w; a.emb_b = emb_b; a.w0 = w0; a.b0 = b0; a.w2 = w2;
  a.b2 = b2; a.y = y; a.crit = crit; a.logits = logits; a.dr = dr; a.mode = mode; a.dlog_in = dlog_in;
  float* ws = (float*)workspace;
  a.feat = ws; a.hid = a.feat + (size_t)B * dh; a.dhid = a.hid + (size_t)B * dh; a.demb = a.dhid + (size_t)B * dh;
  a.dlog = a.demb + (size_t)B * dh; a.lossr = a.dlog + (size_t)B * C;
  a.T = s->T; a.B = B; a.D = D; a.ds = d_static; a.Fe = Fe; a.dh = dh; a.C = C;
  a.plan = token_plan(); a.stamps = g_head_stamps;
  const HeadRoute rt = head_route(mode, B, D, d_static, Fe, C, form);
  a.touch_bytes = rt.touch_bytes;
  if (rt.focal) {
    if (rt.narrow) hipLaunchKernelGGL((k_head_rows_focal<1, 12, 3>), dim3(rt.grid), dim3(HR_THR), 0, st, a);
    else hipLaunchKernelGGL((k_head_rows_focal<1, HR_RJ, HR_KI>), dim3(rt.grid), dim3(HR_THR), 0, st, a);
  } else if (rt.crit) {
    if (rt.narrow) hipLaunchKernelGGL((k_head_rows<1, 12, 3, true>), dim3(rt.grid), dim3(HR_THR), 0, st, a);
    else hipLaunchKernelGGL((k_head_rows<1, HR_RJ, HR_KI, true>), dim3(rt.grid), dim3(HR_THR), 0, st, a);
  } else if (rt.narrow) hipLaunchKernelGGL((k_head_rows<1, 12, 3, false>), dim3(rt.grid), dim3(HR_THR), 0, st, a);
  else hipLaunchKernelGGL((k_head_rows<1, HR_RJ, HR_KI, false>), dim3(rt.grid), dim3(HR_THR), 0, st, a);
  int rc = check_launch(rt.name);
  if (rc || mode == 1) return rc;
  HwArgs h{};
  h.B = B; h.lossr = a.lossr; h.loss = loss;             // loss == null (rd_head_backward): no loss mean
  int n = 0;
  auto add = [&](const float* u, int ldu, const float* v, int ldv, float* dW, float* db) {     // job n of the route: its operands
    HwJob& J = h.j[n];
    J.u = u; J.ldu = ldu; J.N = rt.job[n].N; J.v = v; J.ldv = ldv; J.K = rt.job[n].K; J.dW = dW; J.db = db;
    J.tiles_k = rt.job[n].tiles_k; J.blk0 = rt.job[n].blk0;
    ++n;
  };
  add(a.dhid, dh, a.feat, dh, g_w0, g_b0);                               // d mlp_static[0]
  add(a.dlog, C, a.hid, dh, g_w2, g_b2);                                 // d mlp_static[2]
  if (Fe) add(a.demb, Fe, stat, d_static, g_emb_w, g_emb_b);             // d emb
  h.n = rt.njobs; h.ntiles = rt.ntiles;
  // weight gradients + the loss mean: nothing in the backward chain reads them.  Deferred mode: parked for the next backward chain
  // launch's idle workgroups (rd_trailing.h: four tiles per 1024-thread block); else side branch if registered, else here.
  if (trailing_deferred()) {
    RiderArgs r{};
    r.kind = RIDER_HEAD; r.nblocks = rt.rider_blocks; r.hw = h;
    return trailing_park(r, st);
  }
  hipLaunchKernelGGL(k_head_wgrad, dim3(rt.ntiles), dim3(256), 0, side_fork(st), h);
  return check_launch("k_head_wgrad");
}

// include/raindrop_hip_debug.h: the route above by value; needs no device
extern "C" int rd_debug_head_route(int32_t mode, int32_t B, int32_t D, int32_t d_static, int32_t Fe, int32_t C, int32_t with_crit,
                                   uint32_t* words, char* name, size_t cap) {
  RD_REQUIRE(words && name && cap > 0, "NULL output");
  for (int i = 0; i < 11; ++i) words[i] = 0;
  name[0] = 0;
  RD_REQUIRE(mode >= 0 && mode <= 2 && B > 0 && with_crit >= 0 && with_crit <= 2 && (!with_crit || mode == 0), "bad mode / shape");
  RD_REQUIRE(rd_head_train_supported(D, Fe, C), "head_train: unsupported sizes D=%d Fe=%d C=%d", D, Fe, C);
  RD_REQUIRE(Fe == 0 || d_static > 0, "static embedding tensors missing");
  const HeadRoute r = head_route(mode, B, D, d_static, Fe, C, with_crit == 2 ? HEAD_FOCAL : with_crit ? HEAD_CRIT : HEAD_PLAIN);
  words[0] = (r.narrow ? 1u : 0u) | (r.crit ? 2u : 0u) | (r.emb_lds ? 4u : 0u) | (r.focal ? 8u : 0u) | ((unsigned)r.njobs << 8);
  words[1] = (uint32_t)r.touch_bytes; words[2] = (uint32_t)r.grid; words[3] = (uint32_t)r.ntiles; words[4] = (uint32_t)r.rider_blocks;
  for (int i = 0; i < r.njobs; ++i) {
    words[5 + i] = (uint32_t)r.job[i].blk0;
    words[8 + i] = ((uint32_t)r.job[i].tiles_n << 16) | (uint32_t)r.job[i].tiles_k;
  }
  snprintf(name, cap, "%s", r.name);
  return RD_OK;
}
