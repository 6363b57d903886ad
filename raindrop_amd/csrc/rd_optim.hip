// rd_optim.hip -- Adam update over one flat parameter buffer (the optimizer of code/Raindrop.py:256,
// torch.optim.Adam(lr=1e-4) with default betas / eps, no amsgrad).  With the live parameters and
// their gradients held in flat buffers (raindrop_amd/dp.py) the whole update is one elementwise pass.
#include "rd_common.h"

namespace rd {
namespace {

// (the device step state: the comment in front of k_adam_dev)
struct AdamState { double t, p1, p2, lr, pad0, wd, pad1, pad2; };
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
  const long i4 = (blockIdx.x * (long)blockDim.x + threadIdx.x) * 4;
  if (i4 >= n) return;
  const float step_size = lr / bc1;
  if (i4 + 3 < n) {
    float4 pp = *reinterpret_cast<float4*>(p + i4), gg = *reinterpret_cast<const float4*>(g + i4);
    float4 mm = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
    float4 ee;
    if (EMA) ee = *reinterpret_cast<float4*>(ema + i4);
    float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x; float* E = &ee.x;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float gr = G[c] + wd * P[c];
      M[c] = b1 * M[c] + (1.f - b1) * gr;
      V[c] = b2 * V[c] + (1.f - b2) * gr * gr;
      P[c] -= step_size * M[c] / (sqrtf(V[c]) / bc2_sqrt + eps);
      if (EMA) E[c] += ce * (P[c] - E[c]);
    }
    *reinterpret_cast<float4*>(p + i4) = pp; *reinterpret_cast<float4*>(m + i4) = mm;
    *reinterpret_cast<float4*>(v + i4) = vv;
    if (EMA) *reinterpret_cast<float4*>(ema + i4) = ee;
  } else {
    for (long i = i4; i < n; ++i) {
      const float gr = g[i] + wd * p[i];
      m[i] = b1 * m[i] + (1.f - b1) * gr;
      v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
      p[i] -= step_size * m[i] / (sqrtf(v[i]) / bc2_sqrt + eps);
      if (EMA) ema[i] += ce * (p[i] - ema[i]);
    }
  }
}

// What kind of box is this?  (DESIGN.md "Box variance")  32 KB of straight-line code -- 4096 dependent 8-byte v_fma_f32, nothing the
// compiler can fold --, one wave, clock64 around it: cold (its code in no cache) about 80 ticks per 64-byte line where the hardware
// fetches instructions ahead, 400-450 where it does not; warm 45-55 / 75-95.  tools/probe_clocks.hip is the standalone form.
// The same update with the optimizer's step state on the DEVICE: a captured launch cannot carry the host's bias corrections (they
// change every step).  The state is eight doubles {t, beta1^t, beta2^t, lr, -, weight_decay, -, -} holding the values OF THE STEP
// BEING APPLIED; this kernel only READS it.  The state is advanced -- t += 1, beta^t *= beta -- by an earlier launch of the same
// step: the step's first launch where there is one (rd_set_adam_state registers the cell, rd_step_begin's plan workgroup does it
// next to the dropout seed bump), else rd_adam_state_advance (one thread).  Rounds 5's form advanced a second slot from workgroup 0
// of THIS launch: workgroups dispatched after that store became visible applied step t + 2's corrections (a race wherever the grid
// does not fit the device in one round).  Round 6's first fix -- an arrival ticket, the last workgroup advances -- was
// race-free and cost 4.5 us per step (profiles/r06_adam_ticket_vs_begin.txt: 9.85 against 5.4 us: every workgroup waits for the
// return of a device-scope atomic on ONE line, the last one for a fence and a second atomic on top).
// lr and weight_decay live in the cell too: a learning-rate schedule is an 8-byte copy, not a new capture.
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
  const long i4 = (blockIdx.x * (long)blockDim.x + threadIdx.x) * 4;
  if (i4 >= n) return;
  const float step_size = lr / bc1;
  if (i4 + 3 < n) {
    float4 pp = *reinterpret_cast<float4*>(p + i4), gg = *reinterpret_cast<const float4*>(g + i4);
    float4 mm = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
    float4 ee;
    if (EMA) ee = *reinterpret_cast<float4*>(ema + i4);
    float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x; float* E = &ee.x;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      const float gr = G[c4] + wd * P[c4];
      M[c4] = b1 * M[c4] + (1.f - b1) * gr;
      V[c4] = b2 * V[c4] + (1.f - b2) * gr * gr;
      P[c4] -= step_size * M[c4] / (sqrtf(V[c4]) / bc2_sqrt + eps);
      if (EMA) E[c4] += ce * (P[c4] - E[c4]);
    }
    *reinterpret_cast<float4*>(p + i4) = pp; *reinterpret_cast<float4*>(m + i4) = mm;
    *reinterpret_cast<float4*>(v + i4) = vv;
    if (EMA) *reinterpret_cast<float4*>(ema + i4) = ee;
  } else {
    for (long i = i4; i < n; ++i) {
      const float gr = g[i] + wd * p[i];
      m[i] = b1 * m[i] + (1.f - b1) * gr;
      v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
      p[i] -= step_size * m[i] / (sqrtf(v[i]) / bc2_sqrt + eps);
      if (EMA) ema[i] += ce * (p[i] - ema[i]);
    }
  }
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

// a * b rounded on its own: never the multiply of a fused multiply-add (the compiler contracts a plain `a * b + c`, __fmul_rn included)
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// The clip cell: slot 0 is read by every workgroup and written only by the host (an 8-byte copy, like lr); slots 1-4 are written by
// thread 0 of workgroup 0 alone and read by no workgroup of any launch (the counters by that one thread, to add 1).
struct ClipCell { double max_norm, last_norm, last_scale, skipped, clipped, pad0, pad1, pad2; };

// k_adam_dev (DEV: step state in the device cell) / k_adam (host-computed corrections) on the clipped gradient.  The scale is its own
// rounded multiply: at scale == 1 `gs` IS g and everything behind it is the expression of k_adam / k_adam_dev -- the same bits.
// Weight decay is added AFTER the scale (torch clips the raw gradient; Adam adds wd * p inside its step).
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
  const long i4 = (blockIdx.x * (long)blockDim.x + threadIdx.x) * 4;
  if (i4 >= n) return;
  const float step_size = lr / bc1;
  if (i4 + 3 < n) {
    float4 pp = *reinterpret_cast<float4*>(p + i4), gg = *reinterpret_cast<const float4*>(g + i4);
    float4 mm = *reinterpret_cast<float4*>(m + i4), vv = *reinterpret_cast<float4*>(v + i4);
    float4 ee;
    if (EMA) ee = *reinterpret_cast<float4*>(ema + i4);
    float* P = &pp.x; float* G = &gg.x; float* M = &mm.x; float* V = &vv.x; float* E = &ee.x;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      const float gs = mul_rounded(G[c4], scale);
      const float gr = gs + wd * P[c4];
      M[c4] = b1 * M[c4] + (1.f - b1) * gr;
      V[c4] = b2 * V[c4] + (1.f - b2) * gr * gr;
      P[c4] -= step_size * M[c4] / (sqrtf(V[c4]) / bc2_sqrt + eps);
      if (EMA) E[c4] += ce * (P[c4] - E[c4]);
    }
    *reinterpret_cast<float4*>(p + i4) = pp; *reinterpret_cast<float4*>(m + i4) = mm;
    *reinterpret_cast<float4*>(v + i4) = vv;
    if (EMA) *reinterpret_cast<float4*>(ema + i4) = ee;
  } else {
    for (long i = i4; i < n; ++i) {
      const float gs = mul_rounded(g[i], scale);
      const float gr = gs + wd * p[i];
      m[i] = b1 * m[i] + (1.f - b1) * gr;
      v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
      p[i] -= step_size * m[i] / (sqrtf(v[i]) / bc2_sqrt + eps);
      if (EMA) ema[i] += ce * (p[i] - ema[i]);
    }
  }
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

__global__ __launch_bounds__(64) void k_ifetch_probe(float* out, unsigned long long* t, float a, float b) {
  float x = (float)threadIdx.x;
  const unsigned long long c0 = clock64();
  asm volatile(".rept 4096\n\tv_fma_f32 %0, %0, %1, %2\n\t.endr" : "+v"(x) : "v"(a), "v"(b));
  const unsigned long long c1 = clock64();
  out[threadIdx.x] = x;
  if (threadIdx.x == 0) t[0] = c1 - c0;
}

}  // namespace
}  // namespace rd

using namespace rd;

// not part of the ABI (include/raindrop_hip_debug.h): ticks of the probe block -> ticks_dev[0]; scratch_dev: 64 floats
extern "C" void rd_debug_ifetch_probe(void* ticks_dev, void* scratch_dev, void* stream) {
  hipLaunchKernelGGL(k_ifetch_probe, dim3(1), dim3(64), 0, (hipStream_t)stream, (float*)scratch_dev, (unsigned long long*)ticks_dev,
                     1.0000001f, 0.5f);
}

extern "C" int rd_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                            void* stream) {
  RD_REQUIRE(n >= 0 && step >= 1, "bad n / step");
  RD_REQUIRE(param && grad && exp_avg && exp_avg_sq, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
               reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) == 0,
             "buffers must be 16-byte aligned");
  if (n == 0) return RD_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_adam<false>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, (long)n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2),
                     (float*)nullptr, (EmaCell*)nullptr, 0L);
  return check_launch("k_adam");
}

// rd_adam_step with the step state on the device: `state` = 64 bytes {t, beta1^t, beta2^t, lr, -, weight_decay, -, -} (doubles) OF THE
// STEP BEING APPLIED (advanced beforehand: rd_adam_state_advance, or the step's first launch after rd_set_adam_state) -- ONE launch a
// hipGraph can replay, read-only on the state.
extern "C" int rd_adam_step_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                float beta1, float beta2, float eps, const void* state, void* stream) {
  RD_REQUIRE(n > 0 && state != nullptr, "bad n / NULL optimizer state");
  RD_REQUIRE(param && grad && exp_avg && exp_avg_sq, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
               reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(state)) & 15) == 0, "buffers must be 16-byte aligned");
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_adam_dev<false>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, (long)n, beta1, beta2, eps, (const AdamState*)state, (float*)nullptr, (EmaCell*)nullptr);
  return check_launch("k_adam_dev");
}

extern "C" int rd_adam_state_advance(void* state, float beta1, float beta2, void* stream) {
  RD_REQUIRE(state != nullptr && (reinterpret_cast<uintptr_t>(state) & 15) == 0, "NULL / misaligned optimizer state");
  hipLaunchKernelGGL(k_adam_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, (double*)state, beta1, beta2);
  return check_launch("k_adam_advance");
}

// ---- gradient clipping / non-finite guard -----------------------------------------------------------------------------------------
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

static int clip_args_ok(int64_t n, const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                        const void* partial, size_t partial_bytes, const void* clip) {
  RD_REQUIRE(n > 0, "bad n");
  RD_REQUIRE(param && grad && exp_avg && exp_avg_sq && partial && clip, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
               reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(clip)) & 15) == 0,
             "buffers must be 16-byte aligned");
  RD_REQUIRE(partial_bytes >= rd_grad_sumsq_bytes(), "partial buffer too small (rd_grad_sumsq_bytes)");
  return RD_OK;
}

extern "C" int rd_adam_step_clip(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* partial,
                                 size_t partial_bytes, void* clip, void* stream) {
  RD_REQUIRE(step >= 1, "bad step");
  if (int rc = clip_args_ok(n, param, grad, exp_avg, exp_avg_sq, partial, partial_bytes, clip)) return rc;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL((k_adam_clip<false, false>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, (long)n, beta1, beta2, eps, (const AdamState*)nullptr, lr, weight_decay, (float)bc1,
                     (float)sqrt(bc2), (const double*)partial, (double*)clip, (float*)nullptr, (EmaCell*)nullptr, 0L);
  return check_launch("k_adam_clip");
}

extern "C" int rd_adam_step_clip_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                     float beta2, float eps, const void* state, const void* partial, size_t partial_bytes,
                                     void* clip, void* stream) {
  RD_REQUIRE(state != nullptr && (reinterpret_cast<uintptr_t>(state) & 15) == 0, "NULL / misaligned optimizer state");
  if (int rc = clip_args_ok(n, param, grad, exp_avg, exp_avg_sq, partial, partial_bytes, clip)) return rc;
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL((k_adam_clip<true, false>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, (long)n, beta1, beta2, eps, (const AdamState*)state, 0.f, 0.f, 0.f, 0.f,
                     (const double*)partial, (double*)clip, (float*)nullptr, (EmaCell*)nullptr, 0L);
  return check_launch("k_adam_clip_dev");
}

// ---- exponential moving average of the weights: the EMA twins of the four updates, and the in-place exchange -------------------------
static int ema_args_ok(int64_t n, const float* ema, const void* ema_cell) {
  RD_REQUIRE(n > 0, "bad n");
  RD_REQUIRE(ema && ema_cell, "NULL ema / ema_cell");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(ema) | reinterpret_cast<uintptr_t>(ema_cell)) & 15) == 0, "ema / ema_cell must be 16-byte aligned");
  return RD_OK;
}

extern "C" int rd_adam_step_ema(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int64_t step, float* ema, void* ema_cell, void* stream) {
  RD_REQUIRE(n > 0 && step >= 1, "bad n / step");
  RD_REQUIRE(param && grad && exp_avg && exp_avg_sq, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
               reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) == 0,
             "buffers must be 16-byte aligned");
  if (int rc = ema_args_ok(n, ema, ema_cell)) return rc;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_adam<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, (long)n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), ema, (EmaCell*)ema_cell,
                     (long)step);
  return check_launch("k_adam_ema");
}

extern "C" int rd_adam_step_ema_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                    float beta2, float eps, const void* state, float* ema, void* ema_cell, void* stream) {
  RD_REQUIRE(n > 0 && state != nullptr, "bad n / NULL optimizer state");
  RD_REQUIRE(param && grad && exp_avg && exp_avg_sq, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
               reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(state)) & 15) == 0, "buffers must be 16-byte aligned");
  if (int rc = ema_args_ok(n, ema, ema_cell)) return rc;
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_adam_dev<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, (long)n, beta1, beta2, eps, (const AdamState*)state, ema, (EmaCell*)ema_cell);
  return check_launch("k_adam_dev_ema");
}

extern "C" int rd_adam_step_clip_ema(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int64_t step, const void* partial,
                                     size_t partial_bytes, void* clip, float* ema, void* ema_cell, void* stream) {
  RD_REQUIRE(step >= 1, "bad step");
  if (int rc = clip_args_ok(n, param, grad, exp_avg, exp_avg_sq, partial, partial_bytes, clip)) return rc;
  if (int rc = ema_args_ok(n, ema, ema_cell)) return rc;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL((k_adam_clip<false, true>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, (long)n, beta1, beta2, eps, (const AdamState*)nullptr, lr, weight_decay, (float)bc1,
                     (float)sqrt(bc2), (const double*)partial, (double*)clip, ema, (EmaCell*)ema_cell, (long)step);
  return check_launch("k_adam_clip_ema");
}

extern "C" int rd_adam_step_clip_ema_dev(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float beta1,
                                         float beta2, float eps, const void* state, const void* partial, size_t partial_bytes,
                                         void* clip, float* ema, void* ema_cell, void* stream) {
  RD_REQUIRE(state != nullptr && (reinterpret_cast<uintptr_t>(state) & 15) == 0, "NULL / misaligned optimizer state");
  if (int rc = clip_args_ok(n, param, grad, exp_avg, exp_avg_sq, partial, partial_bytes, clip)) return rc;
  if (int rc = ema_args_ok(n, ema, ema_cell)) return rc;
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL((k_adam_clip<true, true>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, (long)n, beta1, beta2, eps, (const AdamState*)state, 0.f, 0.f, 0.f, 0.f,
                     (const double*)partial, (double*)clip, ema, (EmaCell*)ema_cell, 0L);
  return check_launch("k_adam_clip_ema_dev");
}

extern "C" int rd_swap_f32(int64_t n, float* a, float* b, void* stream) {
  RD_REQUIRE(n > 0, "bad n");
  RD_REQUIRE(a && b, "NULL tensor");
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0, "buffers must be 16-byte aligned");
  const long threads = (n + 3) / 4;
  hipLaunchKernelGGL(k_swap_f32, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, (long)n);
  return check_launch("k_swap_f32");
}
