// rd_optim.hip -- Adam update over one flat parameter buffer (the optimizer of code/Raindrop.py:256,
// torch.optim.Adam(lr=1e-4) with default betas / eps, no amsgrad).  With the live parameters and
// their gradients held in flat buffers (raindrop_amd/dp.py) the whole update is one elementwise pass.
// One body, four kernel shells, sixteen instantiations: the update is written ONCE (adam_element / adam_thread, templates on
// <CLIP, EMA, GROUPS>); k_adam<EMA>, k_adam_dev<EMA>, k_adam_clip<DEV, EMA> and k_adam_grp<DEV, CLIP, EMA> only fetch their scalars
// and call it; the sixteen extern "C" entry points fill one AdamCall and share one launcher (adam_launch<DEV, CLIP, EMA, GROUPS>).
// A flag that is off does not exist in the instruction stream (rule 40): profiles/adam_refactor_isa.txt holds the eight ungrouped
// instantiations against the six hand-kept copies, profiles/param_groups_isa.txt the same eight with and without the GROUPS flag.
#include "rd_common.h"

namespace rd {
namespace {

// (the device step state: the comment in front of k_adam_dev)
struct AdamState { double t, p1, p2, lr, base_lr, wd, sched_n, pad2; };        // (base_lr, sched_n and the table behind the eight: the advance's alone)
// ---- exponential moving average of the weights (DESIGN.md "Weight averaging") ------------------------------------------------------
// ema[i] += c_t (p_new[i] - ema[i]) in the thread that holds p_new in a register: one more flat buffer read and written by the update's
// own launch, no launch of its own.  A template flag of the four update kernels (rule 40): the EMA = false instantiations are the
// kernels as they were, instruction for instruction -- three unused trailing arguments move the kernarg offset of the hidden
// block-size word, one immediate (profiles/ema_isa_diff.txt).  (No own-code touch in the EMA = true ones: the table has no site.)
// The EMA cell, eight doubles {d, warm-up, k[0], k[1], 0, 0, 0, 0}: slots 0 and 1 are read by every workgroup and written by the host
// only (a new decay is an 8-byte copy, not a new capture).  k, the number of EMA updates so far, lives in TWO slots selected by the
// parity of the step number s (host forms: the `step` argument; _dev forms: t of the step state, which an EARLIER launch advanced):
// every workgroup reads k from slot s & 1, thread 0 of workgroup 0 writes k + 1 -- or k, when the non-finite guard skips the step --
// to slot (s + 1) & 1, where the next step reads it.  No workgroup reads a word another workgroup of the same launch writes (the
// rule of k_adam_dev's step state), whether the update happens is decided in THIS launch, and there is no atomic.
struct EmaCell { double decay, warmup, k[2], pad0, pad1, pad2, pad3; };

// c_t = 1 - d_t as a float, d_t = d or min(d, (1 + k) / (10 + k)) formed in double: the same bits in every workgroup
__device__ __forceinline__ float ema_coef(const EmaCell* cell, long step, double& k) {
  const double d = cell->decay;
  k = cell->k[step & 1];
  const double w = (1.0 + k) / (10.0 + k);
  const double dt = (cell->warmup != 0.0 && w < d) ? w : d;
  return (float)(1.0 - dt);
}
__device__ __forceinline__ void ema_count(EmaCell* cell, long step, double k_next) {
  if (blockIdx.x == 0 && threadIdx.x == 0) cell->k[(step + 1) & 1] = k_next;
}

// ---- parameter groups and decoupled weight decay (DESIGN.md "Parameter groups") ------------------------------------------------------
// dp.FlatGradAllReduce starts every tensor on a 64-element boundary, so elements [64c, 64c + 64) -- and with them the four elements of
// every thread -- belong to ONE tensor (or to the zero padding behind it): the group of a thread is one byte of `chunk_group`, its
// scalars one 32-byte row of the group cell.  Sixteen rows {lr_scale, wd_coupled, wd_decoupled, 0}; the byte is masked to 0..15, so
// no map can index outside the cell.  The launches only read both; the host writes a row with one 32-byte copy (not a new capture).
// What stays global: the clip scale (the norm over ALL groups), the step count and the bias corrections, the EMA coefficient.
struct GroupRow { double lr_scale, wd_coupled, wd_decoupled, pad; };
constexpr int kGroupRows = 16;

// a * b rounded on its own: never the multiply of a fused multiply-add (the compiler contracts a plain `a * b + c`, __fmul_rn included)
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// ---- the update, once ----------------------------------------------------------------------------------------------------------------
// Adam on one element.  CLIP: the gradient is scaled first, by its own rounded multiply -- at scale == 1 `g * scale` IS g and everything
// behind it is the expression without the flag: the same bits.  Weight decay is added AFTER the scale (torch clips the raw gradient;
// Adam adds wd * p inside its step).  EMA: the average follows the new parameter in the same thread.  Without a flag its operand is
// not in the expression at all (not `* 1.0f`: that is another instruction stream).
// GROUPS: torch.optim.AdamW's p *= 1 - lr * weight_decay stands in front of everything (`shrink`; 1 where the group's decay is coupled).
struct AdamCoef { float b1, b2, eps, wd, bc2_sqrt, step_size, scale, ce, shrink; };

// (Buffers and index, not references: element i of the flat buffers in the tail, of the thread's four registers in the float4 path;
// each access is then formed where the expression uses it, which keeps the tail's loads and stores in the order they always had.)
template <bool CLIP, bool EMA, bool GROUPS, typename I>
__device__ __forceinline__ void adam_element(float* p, const float* g, float* m, float* v, float* e, I i, const AdamCoef& c) {
  // (GROUPS: the decayed parameter is held in a value of its own.  Without the flag p[i] is named where it always was: reading it
  // once into a value moved the tail's loads and with them the products the FMA contraction takes -- other bits, see adam_thread.)
  const float pd = GROUPS ? mul_rounded(p[i], c.shrink) : 0.f;
  const float gr = (CLIP ? mul_rounded(g[i], c.scale) : g[i]) + c.wd * (GROUPS ? pd : p[i]);
  m[i] = c.b1 * m[i] + (1.f - c.b1) * gr;
  v[i] = c.b2 * v[i] + (1.f - c.b2) * gr * gr;
  const float step = c.step_size * m[i] / (sqrtf(v[i]) / c.bc2_sqrt + c.eps);
  if (GROUPS) p[i] = pd - step;
  else p[i] -= step;
  if (EMA) e[i] += c.ce * (p[i] - e[i]);
}

// One thread's four elements: 16-byte loads and stores, or -- the last thread of the buffer -- a scalar tail.  (The buffers are the
// kernels' __restrict__ arguments; the qualifier is not repeated here.)
// GROUPS: lr and wd are the thread's group's -- lr times the row's scale (formed in double, rounded once), the row's coupled decay;
// the `wd` argument is not read.
template <bool CLIP, bool EMA, bool GROUPS = false>
__device__ __forceinline__ void adam_thread(float* p, const float* g, float* m, float* v, float* ema, long n, float lr, float b1,
                                            float b2, float eps, float wd, float bc1, float bc2_sqrt, float scale, float ce,
                                            const uint8_t* chunk_group = nullptr, const GroupRow* rows = nullptr) {
  const long i4 = (blockIdx.x * (long)blockDim.x + threadIdx.x) * 4;
  if (i4 >= n) return;
  float shrink = 1.f;
  if (GROUPS) {
    const GroupRow r = rows[chunk_group[i4 >> 6] & (kGroupRows - 1)];
    lr = (float)((double)lr * r.lr_scale);
    wd = (float)r.wd_coupled;
    shrink = (float)(1.0 - (double)lr * r.wd_decoupled);
  }
  const AdamCoef c = {b1, b2, eps, wd, bc2_sqrt, lr / bc1, scale, ce, shrink};
  if (i4 + 3 < n) {
    // p is loaded LAST.  Which of two products a sum fuses into its FMA follows the order of the sum's operands, and the optimiser
    // orders them by where their loads stand (it sees this function unrolled before it sees the kernel): with p first,
    // `b1 * m + (1 - b1) * gr` came out as fma(1 - b1, gr, b1 * m) instead of fma(b1, m, (1 - b1) * gr) -- other bits than the kernels
    // have always given.  profiles/adam_refactor_isa.txt records the streams, tests/test_adam_bits_gpu.py pins the bits.
    float4 gg = *reinterpret_cast<const float4*>(g + i4), mm = *reinterpret_cast<float4*>(m + i4);
    float4 vv = *reinterpret_cast<float4*>(v + i4), pp = *reinterpret_cast<float4*>(p + i4);
    float4 ee;
    if (EMA) ee = *reinterpret_cast<float4*>(ema + i4);
#pragma unroll
    for (int k = 0; k < 4; ++k) adam_element<CLIP, EMA, GROUPS>(&pp.x, &gg.x, &mm.x, &vv.x, &ee.x, k, c);
    *reinterpret_cast<float4*>(p + i4) = pp; *reinterpret_cast<float4*>(m + i4) = mm;
    *reinterpret_cast<float4*>(v + i4) = vv;
    if (EMA) *reinterpret_cast<float4*>(ema + i4) = ee;
  } else {
    for (long i = i4; i < n; ++i) adam_element<CLIP, EMA, GROUPS>(p, g, m, v, ema, i, c);
  }
}

// ---- the three shells: where lr / wd / bc1 / bc2_sqrt, the scale and the EMA coefficient come from ----------------------------------
template <bool EMA>
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v, long n, float lr,
                                              float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                              float* __restrict__ ema, EmaCell* cell, long step) {
  float ce = 0.f;
  if (EMA) {
    double k;
    ce = ema_coef(cell, step, k);
    ema_count(cell, step, k + 1.0);
  }
  if (!EMA) RD_TOUCH_CODE_FIRST(RD_TL_ADAM, blockIdx.x, 64);            // own code -> L2 by the first workgroups (rd_common.h; 3 012-byte kernel)
  adam_thread<false, EMA>(p, g, m, v, ema, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, 1.f, ce);
}

// The same update with the optimizer's step state on the DEVICE: a captured launch cannot carry the host's bias corrections (they
// change every step).  The state is eight doubles {t, beta1^t, beta2^t, lr, base lr, weight_decay, n, -} holding the values OF THE STEP
// BEING APPLIED; this kernel only READS it (t, beta^t, lr, weight_decay).  The state is advanced -- t += 1, beta^t *= beta -- by an earlier launch of the same
// step: the step's first launch where there is one (rd_set_adam_state registers the cell, rd_step_begin's plan workgroup does it
// next to the dropout seed bump), else rd_adam_state_advance (one thread).  Rounds 5's form advanced a second slot from workgroup 0
// of THIS launch: workgroups dispatched after that store became visible applied step t + 2's corrections (a race wherever the grid
// does not fit the device in one round).  Round 6's first fix -- an arrival ticket, the last workgroup advances -- was
// race-free and cost 4.5 us per step (profiles/r06_adam_ticket_vs_begin.txt: 9.85 against 5.4 us: every workgroup waits for the
// return of a device-scope atomic on ONE line, the last one for a fence and a second atomic on top).
// lr and weight_decay live in the cell too: a new rate is an 8-byte copy, not a new capture.  A PER-STEP schedule needs no copy at
// all: with n = slot 6 > 0 the cell goes on behind the eight doubles with a table of n factors, and the advancing thread -- the one
// that forms t -- also writes lr = base lr (slot 4) * f[min(t - 1, n - 1)] into slot 3 (adam_state_advance, rd_common.h): the
// sixteen update kernels read state->lr as before, no launch and no argument is added.  n == 0: slot 3 is the caller's.
// (beta^t by repeated multiplication differs from pow() by ~t 2^-53 relative: far below the float the correction is rounded to.)
template <bool EMA>
__global__ __launch_bounds__(256) void k_adam_dev(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, long n, float b1, float b2, float eps,
                                                  const AdamState* __restrict__ state, float* __restrict__ ema, EmaCell* cell) {
  float ce = 0.f;
  if (EMA) {                                                     // the step number: t of the step being applied
    const long step = (long)state->t;
    double k;
    ce = ema_coef(cell, step, k);
    ema_count(cell, step, k + 1.0);
  }
  if (!EMA) RD_TOUCH_CODE_FIRST(RD_TL_ADAM_DEV, blockIdx.x, 64);
  const float lr = (float)state->lr, wd = (float)state->wd;
  const float bc1 = (float)(1.0 - state->p1), bc2_sqrt = (float)sqrt(1.0 - state->p2);
  adam_thread<false, EMA>(p, g, m, v, ema, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, 1.f, ce);
}
__global__ void k_adam_advance(double* state, float b1, float b2) { adam_state_advance(state, b1, b2); }

// ---- global-norm gradient clipping and the non-finite guard (DESIGN.md "Gradient clipping") -------------------------------------
// Two launches behind the last all-reduce wait, both capturable: k_sumsq_partial leaves kClipGrid partial sums of squares of the flat
// gradient, k_adam_clip adds them up -- every workgroup the same kClipGrid doubles in index order, ~1 KB from L2: no float atomics,
// no arrival ticket (rules 15, 37), the same bits on every workgroup, every launch and every rank -- and applies Adam to
// g * min(1, max_norm / (norm + 1e-6)), or nothing at all when the sum is not finite.  New kernels, not a flag in k_adam / k_adam_dev:
// with the feature off the step enqueues exactly what it did (rule 40).  (No own-code touch: the table has no site for them.)
constexpr int kClipGrid = 128;

// sum over the 64 lanes on the DPP path (rd_common.h wave_sum64_dpp) for a double: the two halves travel as two dwords
__device__ __forceinline__ double wave_sum64_dpp_f64(double v) {
#define RD_DPP_ADD64(ctrl, rmask)                                                                            \
  {                                                                                                          \
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, rmask, 0xf, false);               \
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, rmask, 0xf, false);               \
    v += __hiloint2double(hi, lo);                                                                           \
  }
  RD_DPP_ADD64(0x111, 0xf);   // row_shr:1
  RD_DPP_ADD64(0x112, 0xf);   // row_shr:2
  RD_DPP_ADD64(0x114, 0xf);   // row_shr:4
  RD_DPP_ADD64(0x118, 0xf);   // row_shr:8
  RD_DPP_ADD64(0x142, 0xa);   // row_bcast:15 -> rows 1, 3
  RD_DPP_ADD64(0x143, 0xc);   // row_bcast:31 -> rows 2, 3
#undef RD_DPP_ADD64
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// partial[w] = sum of g[i]^2 over workgroup w's contiguous run of float4 slots, squared and accumulated in double (the square of a
// float is exact in a double).  Fixed order: thread t takes slots t, t + 256, ..; lanes by DPP, the four waves through LDS.
// Every workgroup writes its partial (0 for an empty run: n smaller than the grid's reach).
__global__ __launch_bounds__(256) void k_sumsq_partial(const float* __restrict__ g, long n, double* __restrict__ partial) {
  __shared__ double wsum[4];
  const long n4 = (n + 3) >> 2;                                  // float4 slots, the last one possibly short
  const long per = (n4 + kClipGrid - 1) / kClipGrid;            // the grid IS kClipGrid (rd_grad_sumsq): a shift, not a 64-bit division
  const long q0 = blockIdx.x * per, q1 = q0 + per < n4 ? q0 + per : n4;
  double acc = 0.0;
#pragma unroll 4
  for (long q = q0 + threadIdx.x; q < q1; q += 256) {
    const long i = q * 4;
    if (i + 3 < n) {
      const float4 x = *reinterpret_cast<const float4*>(g + i);
      acc += (double)x.x * (double)x.x; acc += (double)x.y * (double)x.y;
      acc += (double)x.z * (double)x.z; acc += (double)x.w * (double)x.w;
    } else {
      for (long j = i; j < n; ++j) acc += (double)g[j] * (double)g[j];
    }
  }
  const double s = wave_sum64_dpp_f64(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// The clip cell: slot 0 is read by every workgroup and written only by the host (an 8-byte copy, like lr); slots 1-4 are written by
// thread 0 of workgroup 0 alone and read by no workgroup of any launch (the counters by that one thread, to add 1).
struct ClipCell { double max_norm, last_norm, last_scale, skipped, clipped, pad0, pad1, pad2; };

// k_adam_dev (DEV: step state in the device cell) / k_adam (host-computed corrections) on the clipped gradient: the prologue forms the
// scale and decides whether the step happens at all, the update is adam_thread<CLIP = true>.
template <bool DEV, bool EMA>
__global__ __launch_bounds__(256) void k_adam_clip(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, float b1, float b2, float eps,
                                                   const AdamState* __restrict__ state, float lr_h, float wd_h, float bc1_h,
                                                   float bc2_sqrt_h, const double* __restrict__ partial, double* clip,
                                                   float* __restrict__ ema, EmaCell* cell, long step_h) {
  double sum = 0.0;
  for (int k = 0; k < kClipGrid; ++k) sum += partial[k];
  const double max_norm = clip[0];
  const bool finite = fabs(sum) <= 1.7976931348623157e308;       // false for inf and NaN
  const double norm = sqrt(sum);
  const double sc = norm > max_norm ? max_norm / (norm + 1e-6) : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    clip[1] = norm;
    clip[2] = finite ? sc : 0.0;
    if (!finite) clip[3] += 1.0;
    else if (sc < 1.0) clip[4] += 1.0;
  }
  float ce = 0.f;
  if (EMA) {                                                     // a skipped step is no update of the average: k moves on unchanged
    const long step = DEV ? (long)state->t : step_h;
    double k;
    ce = ema_coef(cell, step, k);
    ema_count(cell, step, finite ? k + 1.0 : k);
  }
  if (!finite) return;                                           // uniform over the launch: p, m, v (and ema) keep their bits
  const float scale = (float)sc;
  float lr, wd, bc1, bc2_sqrt;
  if (DEV) {
    lr = (float)state->lr; wd = (float)state->wd;
    bc1 = (float)(1.0 - state->p1); bc2_sqrt = (float)sqrt(1.0 - state->p2);
  } else {
    lr = lr_h; wd = wd_h; bc1 = bc1_h; bc2_sqrt = bc2_sqrt_h;
  }
  adam_thread<true, EMA>(p, g, m, v, ema, n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, scale, ce);
}

// The grouped update, all eight forms behind one shell (the three shells above keep their parameter lists and with them their
// instruction streams): k_adam / k_adam_dev / k_adam_clip's prologues as they stand there, selected by the flags, then
// adam_thread<CLIP, EMA, GROUPS = true>.  The step cell's wd slot and a host weight decay are not read: every group's decay is in its row.
template <bool DEV, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_adam_grp(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, long n, float b1, float b2, float eps,
                                                  const AdamState* __restrict__ state, float lr_h, float bc1_h, float bc2_sqrt_h,
                                                  const double* __restrict__ partial, double* clip, float* __restrict__ ema,
                                                  EmaCell* cell, long step_h, const uint8_t* __restrict__ chunk_group,
                                                  const GroupRow* __restrict__ rows) {
  bool finite = true;
  float scale = 1.f;
  if (CLIP) {                                                    // (k_adam_clip's prologue: the same sum in the same order)
    double sum = 0.0;
    for (int k = 0; k < kClipGrid; ++k) sum += partial[k];
    const double max_norm = clip[0];
    finite = fabs(sum) <= 1.7976931348623157e308;
    const double norm = sqrt(sum);
    const double sc = norm > max_norm ? max_norm / (norm + 1e-6) : 1.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      clip[1] = norm;
      clip[2] = finite ? sc : 0.0;
      if (!finite) clip[3] += 1.0;
      else if (sc < 1.0) clip[4] += 1.0;
    }
    scale = (float)sc;
  }
  float ce = 0.f;
  if (EMA) {
    const long step = DEV ? (long)state->t : step_h;
    double k;
    ce = ema_coef(cell, step, k);
    ema_count(cell, step, finite ? k + 1.0 : k);
  }
  if (!finite) return;                                           // uniform over the launch: no group stores anything
  float lr = lr_h, bc1 = bc1_h, bc2_sqrt = bc2_sqrt_h;
  if (DEV) {
    lr = (float)state->lr;
    bc1 = (float)(1.0 - state->p1); bc2_sqrt = (float)sqrt(1.0 - state->p2);
  }
  adam_thread<CLIP, EMA, true>(p, g, m, v, ema, n, lr, b1, b2, eps, 0.f, bc1, bc2_sqrt, scale, ce, chunk_group, rows);
}

// a <-> b over n floats, 16 bytes per thread and a scalar tail behind the last whole float4 (FlatAdam.swap_ema: the flat parameters and
// their average change places IN PLACE, so every holder of a parameter address -- EvalStep, feed.validate -- reads the other one)
__global__ __launch_bounds__(256) void k_swap_f32(float* __restrict__ a, float* __restrict__ b, long n) {
  const long i4 = (blockIdx.x * (long)blockDim.x + threadIdx.x) * 4;
  if (i4 >= n) return;
  if (i4 + 3 < n) {
    const float4 x = *reinterpret_cast<float4*>(a + i4), y = *reinterpret_cast<float4*>(b + i4);
    *reinterpret_cast<float4*>(a + i4) = y; *reinterpret_cast<float4*>(b + i4) = x;
  } else {
    for (long i = i4; i < n; ++i) { const float x = a[i]; a[i] = b[i]; b[i] = x; }
  }
}

// ---- gradient accumulation over a window of micro-batches --------------------------------------------------------------
// Two element-wise passes over the flat gradient buffer `g` and an accumulator `acc` of the same size: the micro-batches of a window
// but the last run k_grad_accumulate (acc += g), the last one k_grad_accumulate_close (g = (acc + g) * s, acc = 0), which leaves the
// window's mean where the all-reduce and the update read it and the accumulator clean for the next window -- whatever it held: an inf
// or NaN goes into g (the update's non-finite guard sees it) and not into the next window.  One add and one multiply per element, each
// rounded on its own (torch's `(acc + g) * s`, bit for bit); no atomics, element i depends on element i alone.  `s` is read from a
// device cell when the kernel RUNS, like the optimizer's other cells: a shorter last window is a 4-byte copy, not a new capture.
// Grid: one float4 per thread and pass, at most kAccumGridMax workgroups (8 per CU: every one resident at once) striding over the rest;
// the P19 buffer (0.5 M floats, 2 MB) is about 500 workgroups, one pass each.  The tail behind the last whole float4 is workgroup 0's.
constexpr int kAccumGridMax = 2048;

__device__ __forceinline__ float add_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

template <bool CLOSE>
__global__ __launch_bounds__(256) void k_grad_accumulate(float* __restrict__ g, float* __restrict__ acc, long n,
                                                         const float* __restrict__ scale_cell) {
  const float s = CLOSE ? *scale_cell : 1.f;
  const long n4 = n >> 2, stride = (long)gridDim.x * 256;
  for (long q = blockIdx.x * 256L + threadIdx.x; q < n4; q += stride) {
    const float4 x = *reinterpret_cast<const float4*>(g + 4 * q), a = *reinterpret_cast<const float4*>(acc + 4 * q);
    float4 r = {add_rounded(a.x, x.x), add_rounded(a.y, x.y), add_rounded(a.z, x.z), add_rounded(a.w, x.w)};
    if (CLOSE) {
      r.x = mul_rounded(r.x, s); r.y = mul_rounded(r.y, s); r.z = mul_rounded(r.z, s); r.w = mul_rounded(r.w, s);
      *reinterpret_cast<float4*>(g + 4 * q) = r;
      *reinterpret_cast<float4*>(acc + 4 * q) = float4{0.f, 0.f, 0.f, 0.f};
    } else {
      *reinterpret_cast<float4*>(acc + 4 * q) = r;
    }
  }
  const long i = (n4 << 2) + threadIdx.x;                        // n % 4 elements behind the last whole float4
  if (blockIdx.x == 0 && i < n) {
    const float r = add_rounded(acc[i], g[i]);
    if (CLOSE) { g[i] = mul_rounded(r, s); acc[i] = 0.f; }
    else acc[i] = r;
  }
}

template <bool CLOSE>
int accumulate_launch(int64_t n, float* g, float* acc, const float* scale_cell, void* stream) {
  RD_REQUIRE(n >= 0, "bad n");
  RD_REQUIRE(g && acc && (!CLOSE || scale_cell), "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(acc)) & 15) == 0, "buffers must be 16-byte aligned");
  RD_REQUIRE((reinterpret_cast<uintptr_t>(scale_cell) & 3) == 0, "scale_cell must be 4-byte aligned");
  if (n == 0) return RD_OK;
  const long blocks = ((n >> 2) + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 1 ? 1 : blocks > kAccumGridMax ? kAccumGridMax : blocks);
  hipLaunchKernelGGL(k_grad_accumulate<CLOSE>, dim3(grid), dim3(256), 0, (hipStream_t)stream, g, acc, (long)n, scale_cell);
  return check_launch(CLOSE ? "k_grad_accumulate_close" : "k_grad_accumulate");
}

// What kind of box is this?  (DESIGN.md "Box variance")  32 KB of straight-line code -- 4096 dependent 8-byte v_fma_f32, nothing the
// compiler can fold --, one wave, clock64 around it: cold (its code in no cache) about 80 ticks per 64-byte line where the hardware
// fetches instructions ahead, 400-450 where it does not; warm 45-55 / 75-95.  tools/probe_clocks.hip is the standalone form.
__global__ __launch_bounds__(64) void k_ifetch_probe(float* out, unsigned long long* t, float a, float b) {
  float x = (float)threadIdx.x;
  const unsigned long long c0 = clock64();
  asm volatile(".rept 4096\n\tv_fma_f32 %0, %0, %1, %2\n\t.endr" : "+v"(x) : "v"(a), "v"(b));
  const unsigned long long c1 = clock64();
  out[threadIdx.x] = x;
  if (threadIdx.x == 0) t[0] = c1 - c0;
}

// ---- one launch path behind the sixteen rd_adam_step* entry points -------------------------------------------------------------------
// What an entry point was given; the fields its form does not have stay zero.
struct AdamCall {
  int64_t n; float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
  float beta1, beta2, eps;
  void* stream;
  float lr = 0.f, weight_decay = 0.f; int64_t step = 0;                         // host forms: the scalars of this step
  const void* state = nullptr;                                                  // _dev forms: the device step state
  const void* partial = nullptr; size_t partial_bytes = 0; void* clip = nullptr;   // _clip forms
  float* ema = nullptr; void* ema_cell = nullptr;                               // _ema forms
  const uint8_t* chunk_group = nullptr; const void* group_cell = nullptr;       // _grp forms
};

inline bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

// the names the launch log knows the sixteen instantiations by, indexed [GROUPS][CLIP][EMA][DEV]
constexpr const char* kAdamLaunch[2][2][2][2] = {
    {{{"k_adam", "k_adam_dev"}, {"k_adam_ema", "k_adam_dev_ema"}},
     {{"k_adam_clip", "k_adam_clip_dev"}, {"k_adam_clip_ema", "k_adam_clip_ema_dev"}}},
    {{{"k_adam_grp", "k_adam_grp_dev"}, {"k_adam_ema_grp", "k_adam_ema_grp_dev"}},
     {{"k_adam_clip_grp", "k_adam_clip_grp_dev"}, {"k_adam_clip_ema_grp", "k_adam_clip_ema_grp_dev"}}}};

// Validation, the host's bias corrections, the grid and the <DEV, CLIP, EMA, GROUPS> dispatch, once.  Everything refused is RD_EINVAL
// before any launch.  n == 0 is an empty update ONLY for plain rd_adam_step (RD_OK, no launch: its callers may hold an empty buffer);
// every other form refuses it, as rd_grad_sumsq does (the ABI as it grew; the host tests pin both answers).
template <bool DEV, bool CLIP, bool EMA, bool GROUPS = false>
int adam_launch(const AdamCall& c) {
  RD_REQUIRE(DEV || c.step >= 1, "bad step");
  RD_REQUIRE(!DEV || (c.state != nullptr && aligned16(c.state)), "NULL / misaligned optimizer state");
  RD_REQUIRE(c.n > 0 || (c.n == 0 && !DEV && !CLIP && !EMA && !GROUPS), "bad n");
  RD_REQUIRE(c.param && c.grad && c.exp_avg && c.exp_avg_sq && (!CLIP || (c.partial && c.clip)), "NULL tensor");
  RD_REQUIRE(!EMA || (c.ema && c.ema_cell), "NULL ema / ema_cell");
  RD_REQUIRE(!GROUPS || (c.chunk_group && c.group_cell), "NULL chunk_group / group_cell");
  RD_REQUIRE(aligned16(c.group_cell), "group_cell must be 16-byte aligned");
  RD_REQUIRE(aligned16(c.param, c.grad, c.exp_avg, c.exp_avg_sq) && aligned16(c.partial, c.clip, c.ema, c.ema_cell),
             "buffers must be 16-byte aligned");
  RD_REQUIRE(!CLIP || c.partial_bytes >= (size_t)kClipGrid * sizeof(double), "partial buffer too small (rd_grad_sumsq_bytes)");
  if (c.n == 0) return RD_OK;
  float bc1 = 0.f, bc2_sqrt = 0.f;                                // the _dev forms form them on the device, from the state
  if (!DEV) {
    bc1 = (float)(1.0 - pow((double)c.beta1, (double)c.step));
    bc2_sqrt = (float)sqrt(1.0 - pow((double)c.beta2, (double)c.step));
  }
  const long threads = (c.n + 3) / 4;
  const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
  const hipStream_t stream = (hipStream_t)c.stream;
  const AdamState* state = (const AdamState*)c.state;
  EmaCell* cell = (EmaCell*)c.ema_cell;
  const long step = EMA && !DEV ? (long)c.step : 0L;             // only the EMA count's slot needs the step number on the device
  if constexpr (GROUPS)
    hipLaunchKernelGGL((k_adam_grp<DEV, CLIP, EMA>), grid, block, 0, stream, c.param, c.grad, c.exp_avg, c.exp_avg_sq, (long)c.n, c.beta1,
                       c.beta2, c.eps, state, c.lr, bc1, bc2_sqrt, (const double*)c.partial, (double*)c.clip, c.ema, cell, step,
                       c.chunk_group, (const GroupRow*)c.group_cell);
  else if constexpr (CLIP)
    hipLaunchKernelGGL((k_adam_clip<DEV, EMA>), grid, block, 0, stream, c.param, c.grad, c.exp_avg, c.exp_avg_sq, (long)c.n, c.beta1,
                       c.beta2, c.eps, state, c.lr, c.weight_decay, bc1, bc2_sqrt, (const double*)c.partial, (double*)c.clip, c.ema,
                       cell, step);
  else if constexpr (DEV)
    hipLaunchKernelGGL(k_adam_dev<EMA>, grid, block, 0, stream, c.param, c.grad, c.exp_avg, c.exp_avg_sq, (long)c.n, c.beta1, c.beta2,
                       c.eps, state, c.ema, cell);
  else
    hipLaunchKernelGGL(k_adam<EMA>, grid, block, 0, stream, c.param, c.grad, c.exp_avg, c.exp_avg_sq, (long)c.n, c.lr, c.beta1,
                       c.beta2, c.eps, c.weight_decay, bc1, bc2_sqrt, c.ema, cell, step);
  return check_launch(kAdamLaunch[GROUPS][CLIP][EMA][DEV]);
}

}  // namespace
}  // namespace rd

using namespace rd;

// not part of the ABI (include/raindrop_hip_debug.h): ticks of the probe block -> ticks_dev[0]; scratch_dev: 64 floats
extern "C" void rd_debug_ifetch_probe(void* ticks_dev, void* scratch_dev, void* stream) {
  hipLaunchKernelGGL(k_ifetch_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, (float*)scratch_dev, (unsigned long long*)ticks_dev,
                     1.0000001f, 0.5f);
}

// ---- the sixteen forms of the update (include/raindrop_hip.h): rd_adam_step [_clip] [_ema] [_grp] [_dev] -----------------------------
extern "C" int rd_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                            void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.weight_decay = weight_decay; c.step = step;
  return adam_launch<false, false, false>(c);
}

extern "C" int rd_adam_step_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                float beta1, float beta2, float eps, const void* state, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state;
  return adam_launch<true, false, false>(c);
}

extern "C" int rd_adam_state_advance(void* state, float beta1, float beta2, void* stream) {
  RD_REQUIRE(state != nullptr && (reinterpret_cast<uintptr_t>(state) & 15) == 0, "NULL / misaligned optimizer state");
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, (double*)state, beta1, beta2);
  return check_launch("k_adam_advance");
}

extern "C" int32_t rd_grad_sumsq_grid(void) { return kClipGrid; }
extern "C" size_t rd_grad_sumsq_bytes(void) { return (size_t)kClipGrid * sizeof(double); }

extern "C" int rd_grad_sumsq(int64_t n, const float* grad, void* partial, size_t partial_bytes, void* stream) {
  RD_REQUIRE(n > 0, "bad n");
  RD_REQUIRE(grad && partial, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(partial)) & 15) == 0, "buffers must be 16-byte aligned");
  RD_REQUIRE(partial_bytes >= rd_grad_sumsq_bytes(), "partial buffer too small (rd_grad_sumsq_bytes)");
  hipLaunchKernelGGL(k_sumsq_partial, dim3(kClipGrid), dim3(256), 0, (hipStream_t)stream, grad, (long)n, (double*)partial);
  return check_launch("k_sumsq_partial");
}

extern "C" int rd_adam_step_clip(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* partial,
                                 size_t partial_bytes, void* clip, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.weight_decay = weight_decay; c.step = step;
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  return adam_launch<false, true, false>(c);
}

extern "C" int rd_adam_step_clip_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                     float beta2, float eps, const void* state, const void* partial, size_t partial_bytes,
                                     void* clip, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state;
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  return adam_launch<true, true, false>(c);
}

extern "C" int rd_adam_step_ema(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int64_t step, float* ema, void* ema_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.weight_decay = weight_decay; c.step = step;
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<false, false, true>(c);
}

extern "C" int rd_adam_step_ema_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                    float beta2, float eps, const void* state, float* ema, void* ema_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state;
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<true, false, true>(c);
}

extern "C" int rd_adam_step_clip_ema(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* partial,
                                     size_t partial_bytes, void* clip, float* ema, void* ema_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.weight_decay = weight_decay; c.step = step;
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<false, true, true>(c);
}

extern "C" int rd_adam_step_clip_ema_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                         float beta2, float eps, const void* state, const void* partial, size_t partial_bytes,
                                         void* clip, float* ema, void* ema_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state;
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<true, true, true>(c);
}

// The grouped twins: the arguments of the form without _grp, then `chunk_group` and `group_cell` in front of the stream
// (`weight_decay` of the host forms is accepted and not read: every group's decay is in its row of the cell).
#define RD_GRP(c) (c).chunk_group = chunk_group, (c).group_cell = group_cell
extern "C" int rd_adam_step_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int64_t step, const uint8_t* chunk_group,
                                const void* group_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.step = step; RD_GRP(c);
  return adam_launch<false, false, false, true>(c);
}

extern "C" int rd_adam_step_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                    float beta2, float eps, const void* state, const uint8_t* chunk_group, const void* group_cell,
                                    void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state; RD_GRP(c);
  return adam_launch<true, false, false, true>(c);
}

extern "C" int rd_adam_step_clip_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* partial,
                                     size_t partial_bytes, void* clip, const uint8_t* chunk_group, const void* group_cell,
                                     void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.step = step; RD_GRP(c);
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  return adam_launch<false, true, false, true>(c);
}

extern "C" int rd_adam_step_clip_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                         float beta2, float eps, const void* state, const void* partial, size_t partial_bytes,
                                         void* clip, const uint8_t* chunk_group, const void* group_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state; RD_GRP(c);
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  return adam_launch<true, true, false, true>(c);
}

extern "C" int rd_adam_step_ema_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                    float beta1, float beta2, float eps, float weight_decay, int64_t step, float* ema,
                                    void* ema_cell, const uint8_t* chunk_group, const void* group_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.step = step; RD_GRP(c);
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<false, false, true, true>(c);
}

extern "C" int rd_adam_step_ema_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                        float beta2, float eps, const void* state, float* ema, void* ema_cell,
                                        const uint8_t* chunk_group, const void* group_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state; RD_GRP(c);
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<true, false, true, true>(c);
}

extern "C" int rd_adam_step_clip_ema_grp(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                         float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* partial,
                                         size_t partial_bytes, void* clip, float* ema, void* ema_cell, const uint8_t* chunk_group,
                                         const void* group_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.lr = lr; c.step = step; RD_GRP(c);
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<false, true, true, true>(c);
}

extern "C" int rd_adam_step_clip_ema_grp_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                             float beta1, float beta2, float eps, const void* state, const void* partial,
                                             size_t partial_bytes, void* clip, float* ema, void* ema_cell,
                                             const uint8_t* chunk_group, const void* group_cell, void* stream) {
  AdamCall c{n, param, grad, exp_avg, exp_avg_sq, beta1, beta2, eps, stream};
  c.state = state; RD_GRP(c);
  c.partial = partial; c.partial_bytes = partial_bytes; c.clip = clip;
  c.ema = ema; c.ema_cell = ema_cell;
  return adam_launch<true, true, true, true>(c);
}
#undef RD_GRP

extern "C" int rd_grad_accumulate(int64_t n, const float* g, float* acc, void* stream) {
  return accumulate_launch<false>(n, const_cast<float*>(g), acc, nullptr, stream);
}

extern "C" int rd_grad_accumulate_close(int64_t n, float* g, float* acc, const float* scale_cell, void* stream) {
  return accumulate_launch<true>(n, g, acc, scale_cell, stream);
}

extern "C" int rd_swap_f32(int64_t n, float* a, float* b, void* stream) {
  RD_REQUIRE(n > 0, "bad n");
  RD_REQUIRE(a && b, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0, "buffers must be 16-byte aligned");
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_swap_f32, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, (long)n);
  return check_launch("k_swap_f32");
}
