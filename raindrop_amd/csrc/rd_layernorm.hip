// rd_layernorm.hip -- residual add + dropout + LayerNorm of the temporal encoder (kernel family K3) as stand-alone launches: what
// the layer runs where the LayerNorm is not the epilogue / prologue of a row-block product or inside a fused chain.
#include <stdlib.h>

#include "rd_encoder.h"

namespace rd {
namespace {

__device__ __forceinline__ float wave_sum64(float v) { return wave_sum64_dpp(v); }   // rd_common.h: same order as the row-block kernels

// ------------------------------------------------------------------------------------------------
// s = x + dropout(r);  y = LayerNorm(s) * g + b.   One wavefront per row; three passes over the
// row (each lane re-reads only what it wrote), exact two-pass variance like torch.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_add_ln_fwd(const float* __restrict__ x, const float* __restrict__ r,
                                                    const float* __restrict__ g, const float* __restrict__ bta,
                                                    float* __restrict__ s_out, float* __restrict__ y,
                                                    float* __restrict__ stats, int M, int D, float p_drop,
                                                    uint64_t seed, uint32_t site, const uint64_t* cell) {
  seed = eff_seed(seed, cell);
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= M) return;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  const float* xr = x + row * D; const float* rr = r + row * D;
  float* sr = s_out + row * D; float* yr = y + row * D;
  float sum = 0.f;
  for (int c = lane; c < D; c += 64) {
    float rv = rr[c];
    if (p_drop > 0.f) rv *= dropout_scale(seed, site, (uint64_t)row * D + c, p_drop, inv_keep);
    const float s = xr[c] + rv;
    sr[c] = s;
    sum += s;
  }
  const float mean = wave_sum64(sum) / D;
  float var = 0.f;
  for (int c = lane; c < D; c += 64) { const float d = sr[c] - mean; var += d * d; }
  const float rstd = rsqrtf(wave_sum64(var) / D + 1e-5f);
  for (int c = lane; c < D; c += 64) yr[c] = (sr[c] - mean) * rstd * g[c] + bta[c];
  if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
}

// register form for D <= 64*NV: two rows per wavefront, every load of both rows issued before the first
// use (one memory round trip per wave instead of three dependent passes per row); the row lives in VGPRs
// between the passes.  Same per-lane summation order as the generic kernel above.
constexpr int LNF_RPW = 2;
template <int NV>
__global__ __launch_bounds__(256) void k_add_ln_fwd_r(const float* __restrict__ x, const float* __restrict__ r,
                                                      const float* __restrict__ g, const float* __restrict__ bta,
                                                      float* __restrict__ s_out, float* __restrict__ y,
                                                      float* __restrict__ stats, int M, int D, float p_drop,
                                                      uint64_t seed, uint32_t site, const uint64_t* cell) {
  seed = eff_seed(seed, cell);
  const int lane = threadIdx.x & 63;
  const long row0 = (blockIdx.x * 4L + (threadIdx.x >> 6)) * LNF_RPW;
  if (row0 >= M) return;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  float xv[LNF_RPW][NV], rv[LNF_RPW][NV], gg[NV], bb[NV];
#pragma unroll
  for (int q = 0; q < LNF_RPW; ++q)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      const bool ok = (row0 + q < M) && c < D;
      xv[q][i] = ok ? x[(row0 + q) * D + c] : 0.f;
      rv[q][i] = ok ? r[(row0 + q) * D + c] : 0.f;
    }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    gg[i] = c < D ? g[c] : 0.f; bb[i] = c < D ? bta[c] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < LNF_RPW; ++q) {
    const long row = row0 + q;
    if (row >= M) break;
    float sv[NV], sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      sv[i] = 0.f;
      if (c < D) {
        float t = rv[q][i];
        if (p_drop > 0.f) t *= dropout_scale(seed, site, (uint64_t)row * D + c, p_drop, inv_keep);
        sv[i] = xv[q][i] + t;
        s_out[row * D + c] = sv[i];
        sum += sv[i];
      }
    }
    const float mean = wave_sum64(sum) / D;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (lane + 64 * i < D) { const float d = sv[i] - mean; var += d * d; }
    const float rstd = rsqrtf(wave_sum64(var) / D + 1e-5f);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < D) y[row * D + c] = (sv[i] - mean) * rstd * gg[i] + bb[i];
    }
    if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
  }
}

// float4 form for D % 4 == 0, D <= 256: lane l owns columns 4l..4l+3 of a row, so the four keep decisions
// of an element quad come from ONE Philox evaluation (the scalar-column kernels evaluate it once per
// element, 4x redundantly, and are bound by those integer multiplies, not by memory); 16-byte accesses,
// LNV_RPW rows per wavefront with every load issued before the first use.  Same masks as the other forms.
constexpr int LNV_RPW = 4;
__global__ __launch_bounds__(256) void k_add_ln_fwd_v(const float* __restrict__ x, const float* __restrict__ r,
                                                      const float* __restrict__ g, const float* __restrict__ bta,
                                                      float* __restrict__ s_out, float* __restrict__ y,
                                                      float* __restrict__ stats, int M, int D, float p_drop,
                                                      uint64_t seed, uint32_t site, const uint64_t* cell) {
  RD_TOUCH_CODE_X(RD_TL_ADD_LN_FWD, blockIdx.x, 512);
  seed = eff_seed(seed, cell);
  const int lane = threadIdx.x & 63;
  const long row0 = (blockIdx.x * 4L + (threadIdx.x >> 6)) * LNV_RPW;
  if (row0 >= M) return;
  const int c = 4 * lane;
  const bool cok = c < D;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 xv[LNV_RPW], rv[LNV_RPW];
#pragma unroll
  for (int q = 0; q < LNV_RPW; ++q) {
    const bool ok = cok && (row0 + q < M);
    xv[q] = zero4; rv[q] = zero4;              // (`ok ? *p : zero4` compiles to a pointer select + flat load from scratch)
    if (ok) {
      xv[q] = *reinterpret_cast<const float4*>(x + (row0 + q) * D + c);
      rv[q] = *reinterpret_cast<const float4*>(r + (row0 + q) * D + c);
    }
  }
  float4 gg = zero4, bb = zero4;
  if (cok) { gg = *reinterpret_cast<const float4*>(g + c); bb = *reinterpret_cast<const float4*>(bta + c); }
#pragma unroll
  for (int q = 0; q < LNV_RPW; ++q) {
    const long row = row0 + q;
    if (row >= M) break;
    float4 t = rv[q];
    if (p_drop > 0.f) {
      const float4 u = uniform4(seed, site, ((uint64_t)row * D + c) >> 2);
      t.x *= u.x >= p_drop ? inv_keep : 0.f; t.y *= u.y >= p_drop ? inv_keep : 0.f;
      t.z *= u.z >= p_drop ? inv_keep : 0.f; t.w *= u.w >= p_drop ? inv_keep : 0.f;
    }
    const float4 sv = make_float4(xv[q].x + t.x, xv[q].y + t.y, xv[q].z + t.z, xv[q].w + t.w);   // 0 beyond D
    if (cok) *reinterpret_cast<float4*>(s_out + row * D + c) = sv;
    const float mean = wave_sum64((sv.x + sv.y) + (sv.z + sv.w)) / D;
    float4 d = make_float4(sv.x - mean, sv.y - mean, sv.z - mean, sv.w - mean);
    if (!cok) d = zero4;
    const float rstd = rsqrtf(wave_sum64((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w)) / D + 1e-5f);
    if (cok)
      *reinterpret_cast<float4*>(y + row * D + c) =
          make_float4(d.x * rstd * gg.x + bb.x, d.y * rstd * gg.y + bb.y, d.z * rstd * gg.z + bb.z, d.w * rstd * gg.w + bb.w);
    if (lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
  }
}

static bool ln_vec_ok(int D, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f) {
  static const bool on = [] { const char* v = getenv("RD_LN_VEC"); return !(v && atoi(v) == 0); }();
  const uintptr_t m = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
                      reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(e) | reinterpret_cast<uintptr_t>(f);
  return on && (D % 4) == 0 && D <= 256 && (m & 15) == 0;
}

}  // namespace

int launch_add_ln_fwd(const float* x, const float* r, const float* g, const float* bta, float* s_out, float* y,
                      float* stats, int M, int D, float p_drop, uint64_t seed, uint32_t site, hipStream_t st) {
  if (ln_vec_ok(D, x, r, g, bta, s_out, y)) {
    hipLaunchKernelGGL(k_add_ln_fwd_v, dim3(cdiv(M, 4 * LNV_RPW)), dim3(256), 0, st, x, r, g, bta, s_out, y, stats, M, D,
                       p_drop, seed, site, seed_cell());
    return check_launch("k_add_ln_fwd_v");
  }
  const int nv = cdiv(D, 64);
  const int nb = cdiv(M, 4 * LNF_RPW);
#define RD_LNF(NV) hipLaunchKernelGGL(k_add_ln_fwd_r<NV>, dim3(nb), dim3(256), 0, st, x, r, g, bta, s_out, y, stats, M, D, \
                                      p_drop, seed, site, seed_cell())
  if (nv == 1) RD_LNF(1); else if (nv == 2) RD_LNF(2); else if (nv == 3) RD_LNF(3); else if (nv == 4) RD_LNF(4);
  else hipLaunchKernelGGL(k_add_ln_fwd, dim3(cdiv(M, 4)), dim3(256), 0, st, x, r, g, bta, s_out, y, stats, M, D, p_drop,
                          seed, site, seed_cell());
#undef RD_LNF
  return check_launch(nv == 1 ? "k_add_ln_fwd_r1" : nv == 2 ? "k_add_ln_fwd_r2" : nv == 3 ? "k_add_ln_fwd_r3" : nv == 4 ? "k_add_ln_fwd_r4"
                                                                                                                   : "k_add_ln_fwd");
}

namespace {

// backward: ds = rstd * (dy*g - mean(dy*g) - xhat * mean(dy*g*xhat));  dr = ds o dropout mask;
// per-block partial sums of dgamma = sum dy*xhat and dbeta = sum dy (64 rows per block).
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ dy, const float* __restrict__ s,
                                                const float* __restrict__ stats, const float* __restrict__ g,
                                                float* __restrict__ ds_out, float* __restrict__ dr_out,
                                                float* __restrict__ part, int M, int D, float p_drop,
                                                uint64_t seed, uint32_t site, const uint64_t* cell) {
  seed = eff_seed(seed, cell);
  extern __shared__ float red[];             // [4][2*D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  for (int c = threadIdx.x; c < 8 * D; c += 256) red[c] = 0.f;
  __syncthreads();
  float* myg = red + wave * 2 * D;
  for (int i = 0; i < LN_RPB / 4; ++i) {
    const long row = (long)blockIdx.x * LN_RPB + wave * (LN_RPB / 4) + i;
    if (row >= M) break;
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    const float* dyr = dy + row * D; const float* sr = s + row * D;
    float c1 = 0.f, c2 = 0.f;
    for (int c = lane; c < D; c += 64) {
      const float xh = (sr[c] - mean) * rstd, dg = dyr[c] * g[c];
      c1 += dg; c2 += dg * xh;
    }
    c1 = wave_sum64(c1) / D; c2 = wave_sum64(c2) / D;
    for (int c = lane; c < D; c += 64) {
      const float xh = (sr[c] - mean) * rstd, d = dyr[c];
      const float v = rstd * (d * g[c] - c1 - xh * c2);
      ds_out[row * D + c] = v;
      float dv = v;
      if (p_drop > 0.f) dv *= dropout_scale(seed, site, (uint64_t)row * D + c, p_drop, inv_keep);
      dr_out[row * D + c] = dv;
      myg[c] += d * xh;          // each lane owns its columns: no race within the wave
      myg[D + c] += d;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += 256)
    part[(long)blockIdx.x * 2 * D + c] = (red[c] + red[2 * D + c]) + (red[4 * D + c] + red[6 * D + c]);
}

// register-accumulating form for D <= 64*NV: each lane keeps its columns' dgamma/dbeta partials in
// VGPRs across the wave's rows; the LDS is touched once per block for the 4-wave combine.
template <int NV>
__global__ __launch_bounds__(256) void k_ln_bwd_r(const float* __restrict__ dy, const float* __restrict__ s,
                                                  const float* __restrict__ stats, const float* __restrict__ g,
                                                  float* __restrict__ ds_out, float* __restrict__ dr_out,
                                                  float* __restrict__ part, int M, int D, float p_drop,
                                                  uint64_t seed, uint32_t site, const uint64_t* cell) {
  RD_TOUCH_CODE_X(RD_TL_LN_BWD_R, blockIdx.x, 512);
  seed = eff_seed(seed, cell);
  extern __shared__ float red[];             // [4][2*D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  float gg[NV], ag[NV], ab[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    gg[i] = c < D ? g[c] : 0.f; ag[i] = 0.f; ab[i] = 0.f;
  }
  // every load of the wave's rows is issued before the first use (one memory round trip per wave)
  constexpr int RPW = LN_RPB / 4;
  const long rbase = (long)blockIdx.x * LN_RPB + wave * RPW;
  float sraw[RPW][NV], dvr[RPW][NV], mean_r[RPW], rstd_r[RPW];
#pragma unroll
  for (int it = 0; it < RPW; ++it) {
    const long row = rbase + it;
    const bool rok = row < M;
    mean_r[it] = rok ? stats[2 * row] : 0.f; rstd_r[it] = rok ? stats[2 * row + 1] : 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      const bool ok = rok && c < D;
      sraw[it][i] = ok ? s[row * D + c] : 0.f;
      dvr[it][i] = ok ? dy[row * D + c] : 0.f;
    }
  }
#pragma unroll
  for (int it = 0; it < RPW; ++it) {
    const long row = rbase + it;
    if (row >= M) break;
    const float mean = mean_r[it], rstd = rstd_r[it];
    float xh[NV], dv[NV];
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      const bool ok = c < D;
      xh[i] = ok ? (sraw[it][i] - mean) * rstd : 0.f;
      dv[i] = dvr[it][i];
      const float dg = dv[i] * gg[i];
      c1 += dg; c2 += dg * xh[i];
    }
    c1 = wave_sum64(c1) / D; c2 = wave_sum64(c2) / D;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < D) {
        const float v = rstd * (dv[i] * gg[i] - c1 - xh[i] * c2);
        ds_out[row * D + c] = v;
        float dvv = v;
        if (p_drop > 0.f) dvv *= dropout_scale(seed, site, (uint64_t)row * D + c, p_drop, inv_keep);
        dr_out[row * D + c] = dvv;
        ag[i] += dv[i] * xh[i];
        ab[i] += dv[i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (c < D) { red[wave * 2 * D + c] = ag[i]; red[wave * 2 * D + D + c] = ab[i]; }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += 256)
    part[(long)blockIdx.x * 2 * D + c] = (red[c] + red[2 * D + c]) + (red[4 * D + c] + red[6 * D + c]);
}

// float4 form of the backward (see k_add_ln_fwd_v): one Philox evaluation per lane and row, 16-byte accesses
__global__ __launch_bounds__(256) void k_ln_bwd_v(const float* __restrict__ dy, const float* __restrict__ s,
                                                  const float* __restrict__ stats, const float* __restrict__ g,
                                                  float* __restrict__ ds_out, float* __restrict__ dr_out,
                                                  float* __restrict__ part, int M, int D, float p_drop,
                                                  uint64_t seed, uint32_t site, const uint64_t* cell) {
  RD_TOUCH_CODE_X(RD_TL_LN_BWD_V, blockIdx.x, 512);
  seed = eff_seed(seed, cell);
  extern __shared__ float red[];             // [4][2*D]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  constexpr int RPW = LN_RPB / 4;
  const int c = 4 * lane;
  const bool cok = c < D;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gg = zero4;
  if (cok) gg = *reinterpret_cast<const float4*>(g + c);
  float4 ag = zero4, ab = zero4;
  const long rbase = (long)blockIdx.x * LN_RPB + wave * RPW;
  float4 sraw[RPW], dvr[RPW]; float mean_r[RPW], rstd_r[RPW];
#pragma unroll
  for (int it = 0; it < RPW; ++it) {
    const long row = rbase + it;
    const bool rok = row < M;
    mean_r[it] = rok ? stats[2 * row] : 0.f; rstd_r[it] = rok ? stats[2 * row + 1] : 0.f;
    sraw[it] = zero4; dvr[it] = zero4;
    if (rok && cok) {
      sraw[it] = *reinterpret_cast<const float4*>(s + row * D + c);
      dvr[it] = *reinterpret_cast<const float4*>(dy + row * D + c);
    }
  }
#pragma unroll
  for (int it = 0; it < RPW; ++it) {
    const long row = rbase + it;
    if (row >= M) break;
    const float mean = mean_r[it], rstd = rstd_r[it];
    const float4 dv = dvr[it];
    float4 xh = make_float4((sraw[it].x - mean) * rstd, (sraw[it].y - mean) * rstd, (sraw[it].z - mean) * rstd,
                            (sraw[it].w - mean) * rstd);
    if (!cok) xh = zero4;
    const float4 dg = make_float4(dv.x * gg.x, dv.y * gg.y, dv.z * gg.z, dv.w * gg.w);
    const float c1 = wave_sum64((dg.x + dg.y) + (dg.z + dg.w)) / D;
    const float c2 = wave_sum64((dg.x * xh.x + dg.y * xh.y) + (dg.z * xh.z + dg.w * xh.w)) / D;
    if (cok) {
      const float4 v = make_float4(rstd * (dg.x - c1 - xh.x * c2), rstd * (dg.y - c1 - xh.y * c2),
                                   rstd * (dg.z - c1 - xh.z * c2), rstd * (dg.w - c1 - xh.w * c2));
      *reinterpret_cast<float4*>(ds_out + row * D + c) = v;
      float4 dr = v;
      if (p_drop > 0.f) {
        const float4 u = uniform4(seed, site, ((uint64_t)row * D + c) >> 2);
        dr.x *= u.x >= p_drop ? inv_keep : 0.f; dr.y *= u.y >= p_drop ? inv_keep : 0.f;
        dr.z *= u.z >= p_drop ? inv_keep : 0.f; dr.w *= u.w >= p_drop ? inv_keep : 0.f;
      }
      *reinterpret_cast<float4*>(dr_out + row * D + c) = dr;
      ag.x += dv.x * xh.x; ag.y += dv.y * xh.y; ag.z += dv.z * xh.z; ag.w += dv.w * xh.w;
      ab.x += dv.x; ab.y += dv.y; ab.z += dv.z; ab.w += dv.w;
    }
  }
  if (cok) {
    *reinterpret_cast<float4*>(red + wave * 2 * D + c) = ag;
    *reinterpret_cast<float4*>(red + wave * 2 * D + D + c) = ab;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * D; i += 256)
    part[(long)blockIdx.x * 2 * D + i] = (red[i] + red[2 * D + i]) + (red[4 * D + i] + red[6 * D + i]);
}

}  // namespace

int launch_ln_bwd(const float* dy, const float* s, const float* stats, const float* g, float* ds_out, float* dr_out,
                  float* part, int M, int D, float p_drop, uint64_t seed, uint32_t site, hipStream_t st) {
  const int lnb = cdiv(M, LN_RPB);
  const size_t lds = sizeof(float) * 8 * D;
  if (ln_vec_ok(D, dy, s, g, ds_out, dr_out, nullptr)) {
    hipLaunchKernelGGL(k_ln_bwd_v, dim3(lnb), dim3(256), lds, st, dy, s, stats, g, ds_out, dr_out, part, M, D, p_drop, seed,
                       site, seed_cell());
    return check_launch("k_ln_bwd_v");
  }
  const int nv = cdiv(D, 64);
#define RD_LN(NV) hipLaunchKernelGGL(k_ln_bwd_r<NV>, dim3(lnb), dim3(256), lds, st, dy, s, stats, g, ds_out, dr_out, \
                                     part, M, D, p_drop, seed, site, seed_cell())
  if (nv == 1) RD_LN(1); else if (nv == 2) RD_LN(2); else if (nv == 3) RD_LN(3); else if (nv == 4) RD_LN(4);
  else hipLaunchKernelGGL(k_ln_bwd, dim3(lnb), dim3(256), lds, st, dy, s, stats, g, ds_out, dr_out, part, M, D,
                          p_drop, seed, site, seed_cell());
#undef RD_LN
  return check_launch(nv == 1 ? "k_ln_bwd_r1" : nv == 2 ? "k_ln_bwd_r2" : nv == 3 ? "k_ln_bwd_r3" : nv == 4 ? "k_ln_bwd_r4" : "k_ln_bwd");
}
}  // namespace rd
