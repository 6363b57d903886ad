// rd_attention.hip -- the attention core of the temporal encoder (kernel family K2; semantics: rd_temporal.hip): masked multi-head
// attention forward / backward between in_proj and out_proj.  Exact-fp32 tiled kernels (v_mfma_f32_16x16x4_f32) and their split-
// bf16 forms, flash-style: sequence tiles are 64 steps; a P19 sample (T=60) is a single tile, P12 (215) / PAM (600) loop over key
// tiles with an online softmax, so the [T,T] score matrix only ever exists in LDS; the materialised-score path of wide heads;
// the route of a pass (attn_route: family, instantiation and launch geometry, decided once) behind attn_forward / attn_backward
// (rd_encoder.h), which the layer calls, and the stand-alone rd_attention_fwd / rd_attention_bwd.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "rd_encoder.h"
#include "rd_plan.h"

namespace rd {
namespace {

constexpr int LDP = TS + 4;     // row stride of the 64x64 score / probability tiles in LDS

// acc[j] (16x16 tiles, j < NT) += A[16 x KK] * B[KK x 16*NT]
// A(i,k) at a[i*a_si + k*a_sk], B(k,n) at b[k*b_sk + n*b_sn]; all LDS.  MFMA lane map: lane l
// supplies A(i = l&15, k = k0 + (l>>4)) and B(k = k0 + (l>>4), n = l&15).
template <int NT>
__device__ __forceinline__ void mma_f32(f32x4 (&acc)[NT], const float* a, int a_si, int a_sk,
                                        const float* b, int b_sk, int b_sn, int KK, int lane) {
  const float* ap = a + (lane & 15) * a_si + (lane >> 4) * a_sk;
  const float* bp = b + (lane >> 4) * b_sk + (lane & 15) * b_sn;
  for (int k0 = 0; k0 < KK; k0 += 4) {
    const float av = ap[k0 * a_sk];
#pragma unroll
    for (int j = 0; j < NT; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[k0 * b_sk + 16 * j * b_sn], acc[j], 0, 0, 0);
  }
}

__device__ __forceinline__ float wave_sum64(float v) { return wave_sum64_dpp(v); }   // rd_common.h: same order as the row-block kernels
__device__ __forceinline__ float wave_max64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
// max / sum over each 16-lane row of the wavefront, every lane of the row gets the result: four rotate-within-row DPP steps
// (row_ror:8, 4, 2, 1) instead of four ds_bpermute round trips
#define RD_ROW_ROR(v, n) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + (n), 0xf, 0xf, false))
__device__ __forceinline__ float group16_max(float v) {
  v = fmaxf(v, RD_ROW_ROR(v, 8)); v = fmaxf(v, RD_ROW_ROR(v, 4)); v = fmaxf(v, RD_ROW_ROR(v, 2)); v = fmaxf(v, RD_ROW_ROR(v, 1));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
  v += RD_ROW_ROR(v, 8); v += RD_ROW_ROR(v, 4); v += RD_ROW_ROR(v, 2); v += RD_ROW_ROR(v, 1);
  return v;
}


static unsigned long long* g_attn_stamps = nullptr;

// Where the rows of one sample live.  Padded layout: [T,B,*] tensors, row of step t = t*B + b, key validity from the mask.
// Token plan: workgroup index b is a RANK, its rows are the contiguous block off[b] .. off[b] + len[b]; steps >= len do
// not exist (as keys they are what the mask would have removed; as queries nothing reads them).
struct AttnRows { long row0, rstep; int Tv; };
__device__ __forceinline__ AttnRows attn_rows(const AttnArgs& a, int b) {
  AttnRows r;
  if (a.plan) {
    r.row0 = __builtin_amdgcn_readfirstlane(a.plan[plan::off_base() + b]); r.rstep = 1;
    r.Tv = __builtin_amdgcn_readfirstlane(a.plan[plan::len_base(a.B) + b]);
  } else { r.row0 = b; r.rstep = a.B; r.Tv = a.T; }
  return r;
}
#define ASTAMP(i)                                                                                         \
  do {                                                                                                    \
    if (a.stamps && blockIdx.x < 8 && threadIdx.x == 0) a.stamps[blockIdx.x * 16 + (i)] = clock64();      \
  } while (0)

// Dropout mask of the attention probabilities: element (bh, q, key) is component (q & 3) of the Philox
// quad (bh*T + key)*ceil(T/4) + (q >> 2): the four query rows a lane holds in an MFMA accumulator
// (q = q4*4 + r) come from ONE Philox evaluation.
__device__ __forceinline__ uint64_t attn_quad(int bh, int T, int q, int key) {
  return ((uint64_t)bh * T + key) * ((T + 3) >> 2) + (q >> 2);
}
__device__ __forceinline__ float attn_keep1(uint64_t seed, uint32_t site, int bh, int T, int q, int key, float p,
                                            float inv_keep) {
  const float4 u = uniform4(seed, site, attn_quad(bh, T, q, key));
  const int j = q & 3;
  const float v = j == 0 ? u.x : (j == 1 ? u.y : (j == 2 ? u.z : u.w));
  return v >= p ? inv_keep : 0.f;
}
// keep-scales of the 4 consecutive query rows q4*4 .. q4*4+3 for one key
__device__ __forceinline__ void attn_keep4(float (&k4)[4], uint64_t seed, uint32_t site, int bh, int T, int q0,
                                           int key, float p, float inv_keep) {
  const float4 u = uniform4(seed, site, attn_quad(bh, T, q0, key));
  k4[0] = u.x >= p ? inv_keep : 0.f; k4[1] = u.y >= p ? inv_keep : 0.f;
  k4[2] = u.z >= p ? inv_keep : 0.f; k4[3] = u.w >= p ? inv_keep : 0.f;
}

// rows [t0, t0+64) x cols [0, hd) of one head of q / k / v / out / dout: 4 threads per row, thread (r, q) holds
// the 16-byte chunks q, q+4, q+8, ... of row r (zero padded to 16*NTH columns).  Loading is split from the LDS
// store so that a kernel can request ALL of its tiles before it consumes the first one: the loop form
// (load, wait, store per chunk) cost one dependent memory round trip per chunk -- 20 to 40 per workgroup.
template <int NTH>
struct HeadRegs { float4 v[NTH]; unsigned ok; };     // ok: bit 4*i+j = component j of chunk i is inside the tile

// VEC: 16-byte loads (head_dim % 4 == 0, row strides % 4 == 0, 16-byte aligned bases -- decided once per kernel
// by the host, AttnRoute::vec, and compiled in as the kernels' VEC flag); otherwise four 4-byte loads per chunk.  Every load is UNCONDITIONAL
// from a clamped (always legal) address and the zero padding is applied later by head_mask: a conditional
// load is a phi of {0, loaded value}, which makes the compiler shuffle registers -- and therefore wait --
// right behind the request.
template <int NTH, bool VEC>
__device__ __forceinline__ void head_load_t(HeadRegs<NTH>& h, const float* base, long row_stride, int t0, int T, int hd,
                                            int tid) {
  const int t = t0 + (tid >> 2);
  const bool rok = t < T;
  const float* src = base + (long)(rok ? t : t0) * row_stride;
  unsigned ok = 0;
#pragma unroll
  for (int i = 0; i < NTH; ++i) {
    const int c = 4 * (tid & 3) + 16 * i;
    if (VEC) {
      const bool cok = c < hd;
      h.v[i] = *reinterpret_cast<const float4*>(src + (cok ? c : 0));
      if (rok && cok) ok |= 0xFu << (4 * i);
    } else {
      float e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool cok = c + j < hd;
        e[j] = src[cok ? c + j : 0];
        if (rok && cok) ok |= 1u << (4 * i + j);
      }
      h.v[i] = make_float4(e[0], e[1], e[2], e[3]);
    }
  }
  h.ok = ok;
}
// zero padding (rows >= T, columns >= head_dim); call below the point where the loads may complete
template <int NTH>
__device__ __forceinline__ void head_mask(HeadRegs<NTH>& h) {
#pragma unroll
  for (int i = 0; i < NTH; ++i) {
    if (!((h.ok >> (4 * i)) & 1u)) h.v[i].x = 0.f;
    if (!((h.ok >> (4 * i + 1)) & 1u)) h.v[i].y = 0.f;
    if (!((h.ok >> (4 * i + 2)) & 1u)) h.v[i].z = 0.f;
    if (!((h.ok >> (4 * i + 3)) & 1u)) h.v[i].w = 0.f;
  }
}
template <int NTH>
__device__ __forceinline__ void head_store(HeadRegs<NTH>& h, float* dst, int ldh, int tid) {
  head_mask<NTH>(h);
  float* d = dst + (tid >> 2) * ldh + 4 * (tid & 3);
#pragma unroll
  for (int i = 0; i < NTH; ++i) *reinterpret_cast<float4*>(d + 16 * i) = h.v[i];
}
// sum over the row of a[r,:] * b[r,:], combined over the row's 4 threads (every one of them gets the sum)
template <int NTH>
__device__ __forceinline__ float head_rowdot(const HeadRegs<NTH>& a, const HeadRegs<NTH>& b) {
  float d = 0.f;
#pragma unroll
  for (int i = 0; i < NTH; ++i)
    d += (a.v[i].x * b.v[i].x + a.v[i].y * b.v[i].y) + (a.v[i].z * b.v[i].z + a.v[i].w * b.v[i].w);
  d += __shfl_xor(d, 1);
  d += __shfl_xor(d, 2);
  return d;
}

// ------------------------------------------------------------------------------------------------
// forward: grid (q tiles, B*H).  Wave w owns query rows 16w..16w+15 of the tile.
// ------------------------------------------------------------------------------------------------
// dynamic LDS: Q, K, V [64][LDH] and P [64][LDP] -- no P where it overlays Q (one_tile below); the attribute takes the size with P
constexpr size_t attn_fwd_lds(int nth, int T) {
  return sizeof(float) * (3 * TS * (16 * nth + 4) + (T <= TS && 16 * nth + 4 >= LDP ? 0 : TS * LDP));
}
template <int NTH, bool VEC>
__global__ __launch_bounds__(256) void k_attn_fwd(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int HDP = 16 * NTH, LDH = HDP + 4;
  float* Qs = smem;
  float* Ks = Qs + TS * LDH;
  float* Vs = Ks + TS * LDH;
  // single key tile (T <= 64, the P19 shape): Q is dead once S is formed, and each wave writes P rows
  // 16w..16w+15 only after reading exactly those Q rows -> P overlays Q (same row stride) and two
  // workgroups fit one CU's LDS (64.5 KB each) instead of one
  const bool one_tile = a.T <= TS && LDH >= LDP;             // a P row (64 keys) must fit a Q row
  float* Ps = one_tile ? Qs : Vs + TS * LDH;
  const int ldp = one_tile ? LDH : LDP;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int q0 = blockIdx.x * TS;
  const long rs = (long)a.B * 3 * a.D;
  const float* qb = a.qkv + (long)b * 3 * a.D + h * a.hd;
  constexpr bool vec = VEC;
  HeadRegs<NTH> qv;
  if (vec) {
    head_load_t<NTH, true>(qv, qb, rs, q0, a.T, a.hd, tid);
  } else {
    head_load_t<NTH, false>(qv, qb, rs, q0, a.T, a.hd, tid);
  }
  // device seed cell on the scalar path (a vector load would queue behind the tile loads and be waited for
  // in the middle of the softmax)
  uint64_t seedv = a.seed;
  if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
  float m_i[4], l_i[4];
  f32x4 o[NTH];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m_i[r] = -INFINITY; l_i[r] = 0.f; }
#pragma unroll
  for (int j = 0; j < NTH; ++j) o[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float inv_keep = 1.0f / (1.0f - a.p_drop);

  for (int k0 = 0; k0 < a.T; k0 += TS) {
    // every load of this key tile (and, first time round, the query tile requested above) is in flight
    // before the first is consumed
    HeadRegs<NTH> kv, vv;
    if (vec) {
      head_load_t<NTH, true>(kv, qb + a.D, rs, k0, a.T, a.hd, tid);
      head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, k0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(kv, qb + a.D, rs, k0, a.T, a.hd, tid);
      head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, k0, a.T, a.hd, tid);
    }
    uint8_t mb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) mb[j] = a.mask[(long)b * a.T + min(k0 + 16 * j + (lane & 15), a.T - 1)];
    __syncthreads();
    if (k0 == 0) head_store<NTH>(qv, Qs, LDH, tid);
    head_store<NTH>(kv, Ks, LDH, tid);
    head_store<NTH>(vv, Vs, LDH, tid);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mma_f32<4>(s, Qs + wave * 16 * LDH, LDH, 1, Ks, 1, LDH, HDP, lane);   // S = Q K^T
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = k0 + 16 * j + (lane & 15);
      const bool dead = key >= a.T || mb[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = dead ? -INFINITY : s[j][r] * a.scale;
        mx[r] = fmaxf(mx[r], s[j][r]);
      }
    }
    float alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m_i[r], group16_max(mx[r]));
      alpha[r] = (m_i[r] == -INFINITY) ? 0.f : expf(m_i[r] - mn);
      m_i[r] = mn;
    }
    float rsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = k0 + 16 * j + (lane & 15);
      float k4[4] = {1.f, 1.f, 1.f, 1.f};
      if (a.p_drop > 0.f)     // F.dropout on the attention probabilities (after the softmax sum)
        attn_keep4(k4, seedv, a.site, bh, a.T, q0 + wave * 16 + 4 * (lane >> 4), min(key, a.T - 1), a.p_drop, inv_keep);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + 4 * (lane >> 4) + r;
        const float p = (s[j][r] == -INFINITY) ? 0.f : __expf(s[j][r] - m_i[r]);
        rsum[r] += p;
        Ps[row * ldp + 16 * j + (lane & 15)] = p * k4[r];
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) l_i[r] = l_i[r] * alpha[r] + group16_sum(rsum[r]);
#pragma unroll
    for (int j = 0; j < NTH; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[j][r] *= alpha[r];
    __syncthreads();
    mma_f32<NTH>(o, Ps + wave * 16 * ldp, ldp, 1, Vs, LDH, 1, TS, lane);  // O += P V
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + wave * 16 + 4 * (lane >> 4) + r;
    if (q >= a.T) continue;
    const float inv = 1.0f / l_i[r];
#pragma unroll
    for (int j = 0; j < NTH; ++j) {
      const int c = 16 * j + (lane & 15);
      if (c < a.hd) a.out[((long)q * a.B + b) * a.D + h * a.hd + c] = o[j][r] * inv;
    }
    if ((lane & 15) == 0) a.lse[(long)bh * a.T + q] = m_i[r] + logf(l_i[r]);
  }
}

// ------------------------------------------------------------------------------------------------
// backward, dQ: grid (q tiles, B*H); also writes delta = rowsum(dout * out).
// ------------------------------------------------------------------------------------------------
// dynamic LDS of the three backward kernels: Q, dO, K, V [64][LDH], lse and delta of the tile's rows, and np score tiles [64][LDP] --
// P here, (P o M)^T and dS^T in k_attn_bwd_dkv, P o M and dS in k_attn_bwd_one
constexpr size_t attn_bwd_lds(int nth, int np) { return sizeof(float) * (4 * TS * (16 * nth + 4) + np * TS * LDP + 2 * TS); }
template <int NTH, bool VEC>
__global__ __launch_bounds__(256) void k_attn_bwd_dq(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int HDP = 16 * NTH, LDH = HDP + 4;
  float* Qs = smem;
  float* dOs = Qs + TS * LDH;
  float* Ks = dOs + TS * LDH;
  float* Vs = Ks + TS * LDH;
  float* Ps = Vs + TS * LDH;
  float* lse_s = Ps + TS * LDP;
  float* dl_s = lse_s + TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int q0 = blockIdx.x * TS;
  const long rs = (long)a.B * 3 * a.D, ro = (long)a.B * a.D;
  const float* qb = a.qkv + (long)b * 3 * a.D + h * a.hd;
  const float* dob = a.dout + (long)b * a.D + h * a.hd;
  const float* ob = a.out + (long)b * a.D + h * a.hd;
  constexpr bool vec = VEC;
  {
    HeadRegs<NTH> qv, dov, ov;
    if (vec) {
      head_load_t<NTH, true>(qv, qb, rs, q0, a.T, a.hd, tid);
      head_load_t<NTH, true>(dov, dob, ro, q0, a.T, a.hd, tid);
      head_load_t<NTH, true>(ov, ob, ro, q0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(qv, qb, rs, q0, a.T, a.hd, tid);
      head_load_t<NTH, false>(dov, dob, ro, q0, a.T, a.hd, tid);
      head_load_t<NTH, false>(ov, ob, ro, q0, a.T, a.hd, tid);
    }
    const int r = tid >> 2, q = q0 + r;
    const float l = q < a.T ? a.lse[(long)bh * a.T + q] : 0.f;
    __builtin_amdgcn_sched_barrier(0);                  // every request above, every use below
    head_store<NTH>(qv, Qs, LDH, tid);
    head_store<NTH>(dov, dOs, LDH, tid);
    head_mask<NTH>(ov);
    const float d = head_rowdot<NTH>(dov, ov);          // delta = rowsum(dO * O); rows >= T are zero padded
    if ((tid & 3) == 0) {
      dl_s[r] = d; lse_s[r] = l;
      if (q < a.T) a.delta[(long)bh * a.T + q] = d;
    }
  }
  uint64_t seedv = a.seed;
  if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
  f32x4 dq[NTH];
#pragma unroll
  for (int j = 0; j < NTH; ++j) dq[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  for (int k0 = 0; k0 < a.T; k0 += TS) {
    HeadRegs<NTH> kv, vv;
    if (vec) {
      head_load_t<NTH, true>(kv, qb + a.D, rs, k0, a.T, a.hd, tid);
      head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, k0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(kv, qb + a.D, rs, k0, a.T, a.hd, tid);
      head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, k0, a.T, a.hd, tid);
    }
    __syncthreads();
    head_store<NTH>(kv, Ks, LDH, tid);
    head_store<NTH>(vv, Vs, LDH, tid);
    __syncthreads();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[j] = s[j]; }
    mma_f32<4>(s, Qs + wave * 16 * LDH, LDH, 1, Ks, 1, LDH, HDP, lane);     // S  = Q K^T
    mma_f32<4>(dp, dOs + wave * 16 * LDH, LDH, 1, Vs, 1, LDH, HDP, lane);   // dP = dO V^T
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = k0 + 16 * j + (lane & 15);
      const bool dead = key >= a.T || a.mask[(long)b * a.T + key];
      float k4[4] = {1.f, 1.f, 1.f, 1.f};
      if (a.p_drop > 0.f)
        attn_keep4(k4, seedv, a.site, bh, a.T, q0 + wave * 16 + 4 * (lane >> 4), min(key, a.T - 1), a.p_drop, inv_keep);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + 4 * (lane >> 4) + r;
        float ds = 0.f;
        if (!dead && q0 + row < a.T) {
          const float p = __expf(s[j][r] * a.scale - lse_s[row]);
          ds = p * (dp[j][r] * k4[r] - dl_s[row]) * a.scale;
        }
        Ps[row * LDP + 16 * j + (lane & 15)] = ds;
      }
    }
    __syncthreads();
    mma_f32<NTH>(dq, Ps + wave * 16 * LDP, LDP, 1, Ks, LDH, 1, TS, lane);   // dQ += dS K
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + wave * 16 + 4 * (lane >> 4) + r;
    if (q >= a.T) continue;
#pragma unroll
    for (int j = 0; j < NTH; ++j) {
      const int c = 16 * j + (lane & 15);
      if (c < a.hd) a.dqkv[((long)q * a.B + b) * 3 * a.D + h * a.hd + c] = dq[j][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward, dK / dV: grid (key tiles, B*H).  Wave w owns key rows 16w..16w+15; scores are formed
// directly transposed (S^T = K Q^T) so that both products below reduce over the query axis.
// ------------------------------------------------------------------------------------------------
template <int NTH, bool VEC>
__global__ __launch_bounds__(256) void k_attn_bwd_dkv(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int HDP = 16 * NTH, LDH = HDP + 4;
  float* Ks = smem;
  float* Vs = Ks + TS * LDH;
  float* Qs = Vs + TS * LDH;
  float* dOs = Qs + TS * LDH;
  float* PTs = dOs + TS * LDH;       // (P o M)^T  [key][q]
  float* DSTs = PTs + TS * LDP;      // dS^T       [key][q]
  float* lse_s = DSTs + TS * LDP;
  float* dl_s = lse_s + TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int k0 = blockIdx.x * TS;
  const long rs = (long)a.B * 3 * a.D, ro = (long)a.B * a.D;
  const float* qb = a.qkv + (long)b * 3 * a.D + h * a.hd;
  const float* dob = a.dout + (long)b * a.D + h * a.hd;
  constexpr bool vec = VEC;
  {
    HeadRegs<NTH> kv, vv;
    if (vec) {
      head_load_t<NTH, true>(kv, qb + a.D, rs, k0, a.T, a.hd, tid);
      head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, k0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(kv, qb + a.D, rs, k0, a.T, a.hd, tid);
      head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, k0, a.T, a.hd, tid);
    }
    head_store<NTH>(kv, Ks, LDH, tid);
    head_store<NTH>(vv, Vs, LDH, tid);
  }
  uint64_t seedv = a.seed;
  if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
  f32x4 dk[NTH], dv[NTH];
#pragma unroll
  for (int j = 0; j < NTH; ++j) { dk[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[j] = dk[j]; }
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  bool dead[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + wave * 16 + 4 * (lane >> 4) + r;
    dead[r] = key >= a.T || a.mask[(long)b * a.T + min(key, a.T - 1)];
  }
  for (int q0 = 0; q0 < a.T; q0 += TS) {
    HeadRegs<NTH> qv, dov;
    if (vec) {
      head_load_t<NTH, true>(qv, qb, rs, q0, a.T, a.hd, tid);
      head_load_t<NTH, true>(dov, dob, ro, q0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(qv, qb, rs, q0, a.T, a.hd, tid);
      head_load_t<NTH, false>(dov, dob, ro, q0, a.T, a.hd, tid);
    }
    __syncthreads();
    head_store<NTH>(qv, Qs, LDH, tid);
    head_store<NTH>(dov, dOs, LDH, tid);
    if (tid < TS) {
      const int q = q0 + tid;
      lse_s[tid] = q < a.T ? a.lse[(long)bh * a.T + q] : 0.f;
      dl_s[tid] = q < a.T ? a.delta[(long)bh * a.T + q] : 0.f;
    }
    __syncthreads();
    f32x4 st[4], dpt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { st[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dpt[j] = st[j]; }
    mma_f32<4>(st, Ks + wave * 16 * LDH, LDH, 1, Qs, 1, LDH, HDP, lane);     // S^T  = K Q^T
    mma_f32<4>(dpt, Vs + wave * 16 * LDH, LDH, 1, dOs, 1, LDH, HDP, lane);   // dP^T = V dO^T
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int qi = 16 * j + (lane & 15);
      const int q = q0 + qi;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int krow = wave * 16 + 4 * (lane >> 4) + r;
        float pm = 0.f, ds = 0.f;
        if (!dead[r] && q < a.T) {
          const float p = __expf(st[j][r] * a.scale - lse_s[qi]);
          float keep = 1.f;
          if (a.p_drop > 0.f) keep = attn_keep1(seedv, a.site, bh, a.T, q, k0 + krow, a.p_drop, inv_keep);
          pm = p * keep;
          ds = p * (dpt[j][r] * keep - dl_s[qi]) * a.scale;
        }
        PTs[krow * LDP + qi] = pm;
        DSTs[krow * LDP + qi] = ds;
      }
    }
    __syncthreads();
    mma_f32<NTH>(dv, PTs + wave * 16 * LDP, LDP, 1, dOs, LDH, 1, TS, lane);  // dV += (P o M)^T dO
    mma_f32<NTH>(dk, DSTs + wave * 16 * LDP, LDP, 1, Qs, LDH, 1, TS, lane);  // dK += dS^T Q
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + wave * 16 + 4 * (lane >> 4) + r;
    if (key >= a.T) continue;
#pragma unroll
    for (int j = 0; j < NTH; ++j) {
      const int c = 16 * j + (lane & 15);
      if (c < a.hd) {
        float* row = a.dqkv + ((long)key * a.B + b) * 3 * a.D + h * a.hd + c;
        row[a.D] = dk[j][r];
        row[2 * a.D] = dv[j][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward, single-tile form (T <= 64: the P19 shape): one workgroup per (sample, head) forms S, P,
// dP and dS ONCE and produces dQ, dK and dV from them (the two-kernel form above recomputes the
// scores in each kernel and is kept for longer sequences).  Wave w owns query rows 16w..16w+15 for
// S / dP / dQ and key rows 16w..16w+15 for dK / dV; dS and P o M are exchanged through LDS.
// ------------------------------------------------------------------------------------------------
template <int NTH, bool VEC>
__global__ __launch_bounds__(256) void k_attn_bwd_one(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int HDP = 16 * NTH, LDH = HDP + 4;
  float* Qs = smem;
  float* Ks = Qs + TS * LDH;
  float* Vs = Ks + TS * LDH;
  float* dOs = Vs + TS * LDH;
  float* PMs = dOs + TS * LDH;       // P o M   [q][key]
  float* DSs = PMs + TS * LDP;       // dS      [q][key]
  float* lse_s = DSs + TS * LDP;
  float* dl_s = lse_s + TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
  const long rs = (long)a.B * 3 * a.D, ro = (long)a.B * a.D;
  const float* qb = a.qkv + (long)b * 3 * a.D + h * a.hd;
  const float* dob = a.dout + (long)b * a.D + h * a.hd;
  const float* ob = a.out + (long)b * a.D + h * a.hd;
  // all five tiles (Q, K, V, dO, O), the LSE row and the key mask are requested in one burst
  constexpr bool vec = VEC;
  uint64_t seedv = a.seed;
  uint8_t mb[4];
  {
    HeadRegs<NTH> qv, kv, vv, dov, ov;
    if (vec) {
      head_load_t<NTH, true>(qv, qb, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(kv, qb + a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(dov, dob, ro, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(ov, ob, ro, 0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(qv, qb, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(kv, qb + a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(dov, dob, ro, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(ov, ob, ro, 0, a.T, a.hd, tid);
    }
    const int r = tid >> 2;
    const float l = r < a.T ? a.lse[(long)bh * a.T + r] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) mb[j] = a.mask[(long)b * a.T + min(16 * j + (lane & 15), a.T - 1)];
    if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);   // scalar path, under the tile loads
    __builtin_amdgcn_sched_barrier(0);                  // every request above, every use below
    head_store<NTH>(qv, Qs, LDH, tid);
    head_store<NTH>(kv, Ks, LDH, tid);
    head_store<NTH>(vv, Vs, LDH, tid);
    head_store<NTH>(dov, dOs, LDH, tid);
    head_mask<NTH>(ov);
    const float d = head_rowdot<NTH>(dov, ov);          // delta = rowsum(dO * O)
    if ((tid & 3) == 0) { dl_s[r] = d; lse_s[r] = l; }
  }
  __syncthreads();
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  f32x4 s[4], dp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { s[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[j] = s[j]; }
  mma_f32<4>(s, Qs + wave * 16 * LDH, LDH, 1, Ks, 1, LDH, HDP, lane);     // S  = Q K^T
  mma_f32<4>(dp, dOs + wave * 16 * LDH, LDH, 1, Vs, 1, LDH, HDP, lane);   // dP = dO V^T
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = 16 * j + (lane & 15);
    const bool dead = key >= a.T || mb[j];
    float k4[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.p_drop > 0.f)
      attn_keep4(k4, seedv, a.site, bh, a.T, wave * 16 + 4 * (lane >> 4), min(key, a.T - 1), a.p_drop, inv_keep);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wave * 16 + 4 * (lane >> 4) + r;
      float pm = 0.f, ds = 0.f;
      if (!dead && row < a.T) {
        const float p = __expf(s[j][r] * a.scale - lse_s[row]);
        pm = p * k4[r];
        ds = p * (dp[j][r] * k4[r] - dl_s[row]) * a.scale;
      }
      PMs[row * LDP + key] = pm;
      DSs[row * LDP + key] = ds;
    }
  }
  __syncthreads();
  f32x4 dq[NTH], dk[NTH], dv[NTH];
#pragma unroll
  for (int j = 0; j < NTH; ++j) { dq[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dk[j] = dq[j]; dv[j] = dq[j]; }
  mma_f32<NTH>(dq, DSs + wave * 16 * LDP, LDP, 1, Ks, LDH, 1, TS, lane);    // dQ = dS K
  mma_f32<NTH>(dk, DSs + wave * 16, 1, LDP, Qs, LDH, 1, TS, lane);          // dK = dS^T Q   (A(i,k) = dS[k][i])
  mma_f32<NTH>(dv, PMs + wave * 16, 1, LDP, dOs, LDH, 1, TS, lane);         // dV = (P o M)^T dO
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = wave * 16 + 4 * (lane >> 4) + r;
    if (t >= a.T) continue;
    float* row = a.dqkv + ((long)t * a.B + b) * 3 * a.D + h * a.hd;
#pragma unroll
    for (int j = 0; j < NTH; ++j) {
      const int c = 16 * j + (lane & 15);
      if (c < a.hd) { row[c] = dq[j][r]; row[a.D + c] = dk[j][r]; row[2 * a.D + c] = dv[j][r]; }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Single-tile attention (T <= 64: the P19 shape) on the split-bf16 matrix path.  The kernels above contract in exact
// fp32 (v_mfma_f32_16x16x4_f32: 1/16 of the bf16 rate, and one 4-byte LDS read per operand and MFMA); here the
// Q / K / V / dO tiles are split ONCE into bf16 hi/lo planes while they are stored to LDS, every contraction is
// hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 (fp32 accumulate, ~2^-16 per product like every dense product of
// the path), and an operand fragment is one 16-byte LDS read -- or, where the reduction index runs along the plane's
// ROWS (P V, dS K, dS^T Q, P^T dO), two transposing reads (ds_read_b64_tr_b16).  P o M and dS are stored TRANSPOSED
// ([key][query]): the four query rows a lane holds in an accumulator become one 8-byte store.
// Same masks, same dropout quads (attn_keep4), same saved LSE as the fp32 kernels; used in the bf16 modes only.
// ------------------------------------------------------------------------------------------------
typedef __bf16 abf8 __attribute__((ext_vector_type(8)));
typedef __bf16 abf4 __attribute__((ext_vector_type(4)));
typedef short as4 __attribute__((ext_vector_type(4)));
typedef short as8 __attribute__((ext_vector_type(8)));
constexpr int LDT = TS + 8;                     // row stride (bf16) of the transposed score planes [key][query]

// fragment with the reduction index along the plane's columns: lane -> row row0 + (lane & 15), columns k0 + 8 (lane >> 4) ..
__device__ __forceinline__ abf8 frag_n(const __bf16* P, int ld, int row0, int k0, int lane) {
  return *reinterpret_cast<const abf8*>(P + (row0 + (lane & 15)) * ld + k0 + 8 * (lane >> 4));
}
// fragment with the reduction index along the plane's rows: lane -> column col0 + (lane & 15), rows k0 + 8 (lane >> 4) ..
__device__ __forceinline__ abf8 frag_t(const __bf16* P, int ld, int k0, int col0, int lane) {
  const int i = lane & 15, G = lane >> 4;
  const __bf16* src = P + (k0 + 8 * G + (i >> 2)) * ld + col0 + 4 * (i & 3);
  const as4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((as4 __attribute__((address_space(3)))*)(src));
  const as4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((as4 __attribute__((address_space(3)))*)(src + 4 * ld));
  const as8 o = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(abf8, o);
}
// acc[j] += A(16 x KK) B(KK x 16 NT), split-bf16.  AT / BT: operand read transposed (reduction along plane rows).
// a0: first row (AT: first column) of A's 16-wide slice; B tile j starts at row (BT: column) 16 j.
template <int NT, bool AT, bool BT>
__device__ __forceinline__ void mma_b16(f32x4 (&acc)[NT], const __bf16* Ah, const __bf16* Al, int lda, int a0,
                                        const __bf16* Bh, const __bf16* Bl, int ldb, int KK, int lane, bool one) {
  // `one` (RD_PREC_BF16: hi*hi only) is decided outside the reduction loop: inside it every step became its own basic block and
  // the fragment reads of the next step could not move above this step's products
  if (!one) {
#pragma unroll
    for (int k0 = 0; k0 < KK; k0 += 32) {
      const abf8 ah = AT ? frag_t(Ah, lda, k0, a0, lane) : frag_n(Ah, lda, a0, k0, lane);
      const abf8 al = AT ? frag_t(Al, lda, k0, a0, lane) : frag_n(Al, lda, a0, k0, lane);
      abf8 bh[NT], bl[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        bh[j] = BT ? frag_t(Bh, ldb, k0, 16 * j, lane) : frag_n(Bh, ldb, 16 * j, k0, lane);
        bl[j] = BT ? frag_t(Bl, ldb, k0, 16 * j, lane) : frag_n(Bl, ldb, 16 * j, k0, lane);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[j], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[j], acc[j], 0, 0, 0);
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[j], acc[j], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int k0 = 0; k0 < KK; k0 += 32) {
      const abf8 ah = AT ? frag_t(Ah, lda, k0, a0, lane) : frag_n(Ah, lda, a0, k0, lane);
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const abf8 bh = BT ? frag_t(Bh, ldb, k0, 16 * j, lane) : frag_n(Bh, ldb, 16 * j, k0, lane);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc[j], 0, 0, 0);
      }
    }
  }
}
// head tile (fp32 registers) -> hi/lo planes [64][ldb], columns [16 NTH, hdp) zeroed
template <int NTH>
__device__ __forceinline__ void head_store_b16(HeadRegs<NTH>& h, __bf16* Ph, __bf16* Pl, int ldb, int hdp, int tid) {
  head_mask<NTH>(h);
  const int o = (tid >> 2) * ldb + 4 * (tid & 3);
#pragma unroll
  for (int i = 0; i < NTH; ++i) {
    const float x[4] = {h.v[i].x, h.v[i].y, h.v[i].z, h.v[i].w};
    abf4 hi, lo;
#pragma unroll
    for (int c = 0; c < 4; ++c) { hi[c] = (__bf16)x[c]; lo[c] = (__bf16)(x[c] - (float)hi[c]); }
    *reinterpret_cast<abf4*>(Ph + o + 16 * i) = hi;
    *reinterpret_cast<abf4*>(Pl + o + 16 * i) = lo;
  }
  if (16 * NTH < hdp) {                                   // at most 16 tail columns (hdp = round-up to 32)
    abf4 z;
#pragma unroll
    for (int c = 0; c < 4; ++c) z[c] = (__bf16)0.f;
    *reinterpret_cast<abf4*>(Ph + o + 16 * NTH) = z;
    *reinterpret_cast<abf4*>(Pl + o + 16 * NTH) = z;
  }
}
// the four accumulator rows of a lane (consecutive queries) -> transposed planes [key][query], one 8-byte store each
__device__ __forceinline__ void store_t4(__bf16* Ph, __bf16* Pl, int key, int q4, const float (&v)[4]) {
  abf4 hi, lo;
#pragma unroll
  for (int r = 0; r < 4; ++r) { hi[r] = (__bf16)v[r]; lo[r] = (__bf16)(v[r] - (float)hi[r]); }
  *reinterpret_cast<abf4*>(Ph + key * LDT + q4) = hi;
  *reinterpret_cast<abf4*>(Pl + key * LDT + q4) = lo;
}

// row stride (bf16) of the hi / lo head planes of every split-bf16 kernel below
constexpr int attn_ldb(int nth) { return 32 * ((16 * nth + 31) / 32) + 16; }
// dynamic LDS of the single-tile kernels, four-wave and eight-wave form.  Forward: Q, K, V hi / lo [64][LDB], P^T hi / lo [64][LDT]
// unless it overlays Q, and the eight-wave form's partial row maxima and sums; backward: Q, K, V, dO planes, (P o M)^T and dS^T
// planes, lse and delta
constexpr size_t attn_fwd_one_b16_lds(int nth, bool wide) {
  const int LDB = attn_ldb(nth);
  return (size_t)(6 * TS * LDB + (LDB >= LDT ? 0 : 2 * TS * LDT)) * sizeof(__bf16) + (wide ? 4 * TS * sizeof(float) : 0);
}
constexpr size_t attn_bwd_one_b16_lds(int nth) { return (size_t)(8 * TS * attn_ldb(nth) + 4 * TS * LDT) * sizeof(__bf16) + 2 * TS * sizeof(float); }
template <int NTH, bool VEC>
__global__ __launch_bounds__(256) void k_attn_fwd_one_b16(AttnArgs a, int one) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  constexpr int HDP = 32 * ((16 * NTH + 31) / 32), LDB = HDP + 16;
  __bf16* Qh = reinterpret_cast<__bf16*>(bsm);
  __bf16* Ql = Qh + TS * LDB;
  __bf16* Kh = Ql + TS * LDB;
  __bf16* Kl = Kh + TS * LDB;
  __bf16* Vh = Kl + TS * LDB;
  __bf16* Vl = Vh + TS * LDB;
  constexpr bool OVL = LDB >= LDT;                  // P^T overlays Q (dead once S is formed; barrier below) when it fits
  __bf16* Ph = OVL ? Qh : Vl + TS * LDB;
  __bf16* Pl = Ph + TS * LDT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
  const long rs = (long)a.B * 3 * a.D;
  const float* qb = a.qkv + (long)b * 3 * a.D + h * a.hd;
  constexpr bool vec = VEC;
  ASTAMP(0);
  uint64_t seedv = a.seed;
  uint8_t mb[4];
  {
    HeadRegs<NTH> qv, kv, vv;
    if (vec) {
      head_load_t<NTH, true>(qv, qb, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(kv, qb + a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, 0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(qv, qb, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(kv, qb + a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, 0, a.T, a.hd, tid);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) mb[j] = a.mask[(long)b * a.T + min(16 * j + (lane & 15), a.T - 1)];
    if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
    __builtin_amdgcn_sched_barrier(0);
    ASTAMP(1);
    head_store_b16<NTH>(qv, Qh, Ql, LDB, HDP, tid);
    head_store_b16<NTH>(kv, Kh, Kl, LDB, HDP, tid);
    head_store_b16<NTH>(vv, Vh, Vl, LDB, HDP, tid);
  }
  ASTAMP(2);
  __syncthreads();
  ASTAMP(3);
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  f32x4 s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  mma_b16<4, false, false>(s, Qh, Ql, LDB, wave * 16, Kh, Kl, LDB, HDP, lane, one);      // S = Q K^T
  ASTAMP(4);
  float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = 16 * j + (lane & 15);
    const bool dead = key >= a.T || mb[j];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[j][r] = dead ? -INFINITY : s[j][r] * a.scale;
      mx[r] = fmaxf(mx[r], s[j][r]);
    }
  }
  float m_i[4], l_i[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) m_i[r] = group16_max(mx[r]);
  __syncthreads();                                  // every wave is done with Q before P^T overwrites it
  float rsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = 16 * j + (lane & 15);
    float k4[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.p_drop > 0.f)
      attn_keep4(k4, seedv, a.site, bh, a.T, wave * 16 + 4 * (lane >> 4), min(key, a.T - 1), a.p_drop, inv_keep);
    float pv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = (s[j][r] == -INFINITY) ? 0.f : __expf(s[j][r] - m_i[r]);
      rsum[r] += p;
      pv[r] = p * k4[r];
    }
    store_t4(Ph, Pl, key, wave * 16 + 4 * (lane >> 4), pv);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) l_i[r] = group16_sum(rsum[r]);
  __syncthreads();
  ASTAMP(5);
  f32x4 o[NTH];
#pragma unroll
  for (int j = 0; j < NTH; ++j) o[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  mma_b16<NTH, true, true>(o, Ph, Pl, LDT, wave * 16, Vh, Vl, LDB, TS, lane, one);        // O = P V
  ASTAMP(6);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = wave * 16 + 4 * (lane >> 4) + r;
    if (q >= a.T) continue;
    const float inv = 1.0f / l_i[r];
#pragma unroll
    for (int j = 0; j < NTH; ++j) {
      const int c = 16 * j + (lane & 15);
      if (c < a.hd) a.out[((long)q * a.B + b) * a.D + h * a.hd + c] = o[j][r] * inv;
    }
    if ((lane & 15) == 0) a.lse[(long)bh * a.T + q] = m_i[r] + logf(l_i[r]);
  }
  ASTAMP(7);
}

template <int NTH, bool VEC>
__global__ __launch_bounds__(256) void k_attn_bwd_one_b16(AttnArgs a, int one) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  constexpr int HDP = 32 * ((16 * NTH + 31) / 32), LDB = HDP + 16;
  __bf16* Qh = reinterpret_cast<__bf16*>(bsm);
  __bf16* Ql = Qh + TS * LDB;
  __bf16* Kh = Ql + TS * LDB;
  __bf16* Kl = Kh + TS * LDB;
  __bf16* Vh = Kl + TS * LDB;
  __bf16* Vl = Vh + TS * LDB;
  __bf16* Oh = Vl + TS * LDB;                       // dO
  __bf16* Ol = Oh + TS * LDB;
  __bf16* Ph = Ol + TS * LDB;                       // (P o M)^T  [key][query]
  __bf16* Pl = Ph + TS * LDT;
  __bf16* Sh = Pl + TS * LDT;                       // dS^T       [key][query]
  __bf16* Sl = Sh + TS * LDT;
  float* lse_s = reinterpret_cast<float*>(Sl + TS * LDT);
  float* dl_s = lse_s + TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
  const long rs = (long)a.B * 3 * a.D, ro = (long)a.B * a.D;
  const float* qb = a.qkv + (long)b * 3 * a.D + h * a.hd;
  const float* dob = a.dout + (long)b * a.D + h * a.hd;
  const float* ob = a.out + (long)b * a.D + h * a.hd;
  constexpr bool vec = VEC;
  ASTAMP(0);
  uint64_t seedv = a.seed;
  uint8_t mb[4];
  {
    HeadRegs<NTH> qv, kv, vv, dov, ov;
    if (vec) {
      head_load_t<NTH, true>(qv, qb, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(kv, qb + a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(dov, dob, ro, 0, a.T, a.hd, tid);
      head_load_t<NTH, true>(ov, ob, ro, 0, a.T, a.hd, tid);
    } else {
      head_load_t<NTH, false>(qv, qb, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(kv, qb + a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(dov, dob, ro, 0, a.T, a.hd, tid);
      head_load_t<NTH, false>(ov, ob, ro, 0, a.T, a.hd, tid);
    }
    const int r = tid >> 2;
    const float l = r < a.T ? a.lse[(long)bh * a.T + r] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) mb[j] = a.mask[(long)b * a.T + min(16 * j + (lane & 15), a.T - 1)];
    if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
    __builtin_amdgcn_sched_barrier(0);
    ASTAMP(1);
    head_store_b16<NTH>(qv, Qh, Ql, LDB, HDP, tid);
    head_store_b16<NTH>(kv, Kh, Kl, LDB, HDP, tid);
    head_store_b16<NTH>(vv, Vh, Vl, LDB, HDP, tid);
    head_mask<NTH>(ov);
    head_mask<NTH>(dov);
    const float d = head_rowdot<NTH>(dov, ov);          // delta = rowsum(dO * O), in fp32
    head_store_b16<NTH>(dov, Oh, Ol, LDB, HDP, tid);
    if ((tid & 3) == 0) { dl_s[r] = d; lse_s[r] = l; }
  }
  ASTAMP(2);
  __syncthreads();
  ASTAMP(3);
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  f32x4 s[4], dp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { s[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[j] = s[j]; }
  mma_b16<4, false, false>(s, Qh, Ql, LDB, wave * 16, Kh, Kl, LDB, HDP, lane, one);      // S  = Q K^T
  mma_b16<4, false, false>(dp, Oh, Ol, LDB, wave * 16, Vh, Vl, LDB, HDP, lane, one);     // dP = dO V^T
  ASTAMP(4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int key = 16 * j + (lane & 15);
    const bool dead = key >= a.T || mb[j];
    float k4[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.p_drop > 0.f)
      attn_keep4(k4, seedv, a.site, bh, a.T, wave * 16 + 4 * (lane >> 4), min(key, a.T - 1), a.p_drop, inv_keep);
    float pm[4], ds[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wave * 16 + 4 * (lane >> 4) + r;
      pm[r] = 0.f; ds[r] = 0.f;
      if (!dead && row < a.T) {
        const float p = __expf(s[j][r] * a.scale - lse_s[row]);
        pm[r] = p * k4[r];
        ds[r] = p * (dp[j][r] * k4[r] - dl_s[row]) * a.scale;
      }
    }
    store_t4(Ph, Pl, key, wave * 16 + 4 * (lane >> 4), pm);
    store_t4(Sh, Sl, key, wave * 16 + 4 * (lane >> 4), ds);
  }
  ASTAMP(5);
  __syncthreads();
  f32x4 dq[NTH], dk[NTH], dv[NTH];
#pragma unroll
  for (int j = 0; j < NTH; ++j) { dq[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dk[j] = dq[j]; dv[j] = dq[j]; }
  mma_b16<NTH, true, true>(dq, Sh, Sl, LDT, wave * 16, Kh, Kl, LDB, TS, lane, one);      // dQ = dS K       (rows: queries)
  mma_b16<NTH, false, true>(dk, Sh, Sl, LDT, wave * 16, Qh, Ql, LDB, TS, lane, one);     // dK = dS^T Q     (rows: keys)
  mma_b16<NTH, false, true>(dv, Ph, Pl, LDT, wave * 16, Oh, Ol, LDB, TS, lane, one);     // dV = (P o M)^T dO
  ASTAMP(6);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = wave * 16 + 4 * (lane >> 4) + r;
    if (t >= a.T) continue;
    float* row = a.dqkv + ((long)t * a.B + b) * 3 * a.D + h * a.hd;
#pragma unroll
    for (int j = 0; j < NTH; ++j) {
      const int c = 16 * j + (lane & 15);
      if (c < a.hd) { row[c] = dq[j][r]; row[a.D + c] = dk[j][r]; row[2 * a.D + c] = dv[j][r]; }
    }
  }
  ASTAMP(7);
}

// Eight-wave form of k_attn_fwd_one_b16: wave = (query row tile wq, half wh).  S: two of the four key tiles per wave, the row
// maximum and the row sum are combined across the two halves through 1 KB of LDS; O = P V: the head-dim tiles split
// between the halves.  Loads: waves 0-3 fetch Q and K, waves 4-7 V.
template <int NTH, bool VEC>
__global__ __launch_bounds__(512) void k_attn_fwd_one_b16w(AttnArgs a, int one) {
  RD_TOUCH_CODE_X(RD_TL_ATTN_FWD_ONE, blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y, 512);
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  constexpr int HDP = 32 * ((16 * NTH + 31) / 32), LDB = HDP + 16, NA = (NTH + 1) / 2;
  __bf16* Qh = reinterpret_cast<__bf16*>(bsm);
  __bf16* Ql = Qh + TS * LDB;
  __bf16* Kh = Ql + TS * LDB;
  __bf16* Kl = Kh + TS * LDB;
  __bf16* Vh = Kl + TS * LDB;
  __bf16* Vl = Vh + TS * LDB;
  constexpr bool OVL = LDB >= LDT;
  __bf16* Ph = OVL ? Qh : Vl + TS * LDB;
  __bf16* Pl = Ph + TS * LDT;
  float* mxs = reinterpret_cast<float*>((OVL ? Vl + TS * LDB : Pl + TS * LDT));    // [2][64] partial row maxima
  float* sms = mxs + 2 * TS;                                                       // [2][64] partial row sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave & 3, wh = wave >> 2, lt = tid & 255;
  const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
  const AttnRows ar = attn_rows(a, b);
  const int Tv = ar.Tv;
  const long rs = ar.rstep * 3 * a.D, ro = ar.rstep * a.D;
  const float* qb = a.qkv + ar.row0 * 3 * a.D + h * a.hd;
  constexpr bool vec = VEC;
  uint64_t seedv = a.seed;
  uint8_t mb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = min(16 * (2 * wh + j) + (lane & 15), a.T - 1);
    mb[j] = a.plan ? (uint8_t)(key >= Tv) : a.mask[(long)b * a.T + key];
  }
  if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
  if (wh == 0) {
    HeadRegs<NTH> qv, kv;
    if (vec) {
      head_load_t<NTH, true>(qv, qb, rs, 0, Tv, a.hd, lt);
      head_load_t<NTH, true>(kv, qb + a.D, rs, 0, Tv, a.hd, lt);
    } else {
      head_load_t<NTH, false>(qv, qb, rs, 0, Tv, a.hd, lt);
      head_load_t<NTH, false>(kv, qb + a.D, rs, 0, Tv, a.hd, lt);
    }
    __builtin_amdgcn_sched_barrier(0);
    head_store_b16<NTH>(qv, Qh, Ql, LDB, HDP, lt);
    head_store_b16<NTH>(kv, Kh, Kl, LDB, HDP, lt);
  } else {
    HeadRegs<NTH> vv;
    if (vec) head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, 0, Tv, a.hd, lt);
    else head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, 0, Tv, a.hd, lt);
    __builtin_amdgcn_sched_barrier(0);
    head_store_b16<NTH>(vv, Vh, Vl, LDB, HDP, lt);
  }
  __syncthreads();
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  f32x4 s[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) s[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  mma_b16<2, false, false>(s, Qh, Ql, LDB, wq * 16, Kh + 32 * wh * LDB, Kl + 32 * wh * LDB, LDB, HDP, lane, one);    // S = Q K^T
  float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = 16 * (2 * wh + j) + (lane & 15);
    const bool dead = key >= a.T || mb[j];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[j][r] = dead ? -INFINITY : s[j][r] * a.scale;
      mx[r] = fmaxf(mx[r], s[j][r]);
    }
  }
  const int row0 = wq * 16 + 4 * (lane >> 4);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mx[r] = group16_max(mx[r]);
    if ((lane & 15) == 0) mxs[wh * TS + row0 + r] = mx[r];
  }
  __syncthreads();                                  // partial maxima visible; every wave is done with Q before P^T overwrites it
  float m_i[4], rsum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) m_i[r] = fmaxf(mxs[row0 + r], mxs[TS + row0 + r]);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = 16 * (2 * wh + j) + (lane & 15);
    float k4[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.p_drop > 0.f)
      attn_keep4(k4, seedv, a.site, bh, a.T, row0, min(key, a.T - 1), a.p_drop, inv_keep);
    float pv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = (s[j][r] == -INFINITY) ? 0.f : __expf(s[j][r] - m_i[r]);
      rsum[r] += p;
      pv[r] = p * k4[r];
    }
    store_t4(Ph, Pl, key, row0, pv);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    rsum[r] = group16_sum(rsum[r]);
    if ((lane & 15) == 0) sms[wh * TS + row0 + r] = rsum[r];
  }
  __syncthreads();
  float l_i[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) l_i[r] = sms[row0 + r] + sms[TS + row0 + r];
  const int t0 = wh * NA;
  f32x4 o[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) o[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  mma_b16<NA, true, true>(o, Ph, Pl, LDT, wq * 16, Vh + 16 * t0, Vl + 16 * t0, LDB, TS, lane, one);      // O = P V
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = row0 + r;
    if (q >= Tv) continue;
    const float inv = 1.0f / l_i[r];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int c = 16 * (t0 + j) + (lane & 15);
      if (t0 + j < NTH && c < a.hd) a.out[ar.row0 * a.D + (long)q * ro + h * a.hd + c] = o[j][r] * inv;
    }
    if (wh == 0 && (lane & 15) == 0) a.lse[(long)bh * a.T + q] = m_i[r] + logf(l_i[r]);
  }
}

// Eight-wave form of the kernel above: wave = (row tile wq, half wh).  S / dP: each wave takes two of the four key
// tiles of its query rows; dQ / dK / dV: the head-dim tiles are split between the two waves of a row tile.  Loads: waves
// 0-3 fetch Q, K, V, waves 4-7 dO, O (+ delta, LSE).  Same LDS planes, two waves per SIMD instead of one: the phases of a
// workgroup overlap a little instead of not at all (nothing needs a cross-wave reduction: the backward uses the saved LSE).
template <int NTH, bool VEC>
__global__ __launch_bounds__(512) void k_attn_bwd_one_b16w(AttnArgs a, int one) {
  RD_TOUCH_CODE_X(RD_TL_ATTN_BWD_ONE, blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y, 512);
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  constexpr int HDP = 32 * ((16 * NTH + 31) / 32), LDB = HDP + 16, NA = (NTH + 1) / 2;
  __bf16* Qh = reinterpret_cast<__bf16*>(bsm);
  __bf16* Ql = Qh + TS * LDB;
  __bf16* Kh = Ql + TS * LDB;
  __bf16* Kl = Kh + TS * LDB;
  __bf16* Vh = Kl + TS * LDB;
  __bf16* Vl = Vh + TS * LDB;
  __bf16* Oh = Vl + TS * LDB;
  __bf16* Ol = Oh + TS * LDB;
  __bf16* Ph = Ol + TS * LDB;
  __bf16* Pl = Ph + TS * LDT;
  __bf16* Sh = Pl + TS * LDT;
  __bf16* Sl = Sh + TS * LDT;
  float* lse_s = reinterpret_cast<float*>(Sl + TS * LDT);
  float* dl_s = lse_s + TS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wq = wave & 3, wh = wave >> 2, lt = tid & 255;
  const int bh = blockIdx.x, b = bh / a.H, h = bh - b * a.H;
  const AttnRows ar = attn_rows(a, b);
  const int Tv = ar.Tv;
  const long rs = ar.rstep * 3 * a.D, ro = ar.rstep * a.D;
  const float* qb = a.qkv + ar.row0 * 3 * a.D + h * a.hd;
  const float* dob = a.dout + ar.row0 * a.D + h * a.hd;
  const float* ob = a.out + ar.row0 * a.D + h * a.hd;
  constexpr bool vec = VEC;
  uint64_t seedv = a.seed;
  uint8_t mb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = min(16 * (2 * wh + j) + (lane & 15), a.T - 1);
    mb[j] = a.plan ? (uint8_t)(key >= Tv) : a.mask[(long)b * a.T + key];
  }
  if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
  if (wh == 0) {                                      // wave-uniform
    HeadRegs<NTH> qv, kv, vv;
    if (vec) {
      head_load_t<NTH, true>(qv, qb, rs, 0, Tv, a.hd, lt);
      head_load_t<NTH, true>(kv, qb + a.D, rs, 0, Tv, a.hd, lt);
      head_load_t<NTH, true>(vv, qb + 2 * a.D, rs, 0, Tv, a.hd, lt);
    } else {
      head_load_t<NTH, false>(qv, qb, rs, 0, Tv, a.hd, lt);
      head_load_t<NTH, false>(kv, qb + a.D, rs, 0, Tv, a.hd, lt);
      head_load_t<NTH, false>(vv, qb + 2 * a.D, rs, 0, Tv, a.hd, lt);
    }
    __builtin_amdgcn_sched_barrier(0);
    head_store_b16<NTH>(qv, Qh, Ql, LDB, HDP, lt);
    head_store_b16<NTH>(kv, Kh, Kl, LDB, HDP, lt);
    head_store_b16<NTH>(vv, Vh, Vl, LDB, HDP, lt);
  } else {
    HeadRegs<NTH> dov, ov;
    if (vec) {
      head_load_t<NTH, true>(dov, dob, ro, 0, Tv, a.hd, lt);
      head_load_t<NTH, true>(ov, ob, ro, 0, Tv, a.hd, lt);
    } else {
      head_load_t<NTH, false>(dov, dob, ro, 0, Tv, a.hd, lt);
      head_load_t<NTH, false>(ov, ob, ro, 0, Tv, a.hd, lt);
    }
    const int r = lt >> 2;
    const float l = r < Tv ? a.lse[(long)bh * a.T + r] : 0.f;
    __builtin_amdgcn_sched_barrier(0);
    head_mask<NTH>(ov);
    head_mask<NTH>(dov);
    const float d = head_rowdot<NTH>(dov, ov);
    head_store_b16<NTH>(dov, Oh, Ol, LDB, HDP, lt);
    if ((lt & 3) == 0) { dl_s[r] = d; lse_s[r] = l; }
  }
  __syncthreads();
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  f32x4 s[2], dp[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) { s[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[j] = s[j]; }
  mma_b16<2, false, false>(s, Qh, Ql, LDB, wq * 16, Kh + 32 * wh * LDB, Kl + 32 * wh * LDB, LDB, HDP, lane, one);    // S
  mma_b16<2, false, false>(dp, Oh, Ol, LDB, wq * 16, Vh + 32 * wh * LDB, Vl + 32 * wh * LDB, LDB, HDP, lane, one);   // dP
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = 16 * (2 * wh + j) + (lane & 15);
    const bool dead = key >= a.T || mb[j];
    float k4[4] = {1.f, 1.f, 1.f, 1.f};
    if (a.p_drop > 0.f)
      attn_keep4(k4, seedv, a.site, bh, a.T, wq * 16 + 4 * (lane >> 4), min(key, a.T - 1), a.p_drop, inv_keep);
    float pm[4], ds[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = wq * 16 + 4 * (lane >> 4) + r;
      pm[r] = 0.f; ds[r] = 0.f;
      if (!dead && row < Tv) {
        const float p = __expf(s[j][r] * a.scale - lse_s[row]);
        pm[r] = p * k4[r];
        ds[r] = p * (dp[j][r] * k4[r] - dl_s[row]) * a.scale;
      }
    }
    store_t4(Ph, Pl, key, wq * 16 + 4 * (lane >> 4), pm);
    store_t4(Sh, Sl, key, wq * 16 + 4 * (lane >> 4), ds);
  }
  __syncthreads();
  const int t0 = wh * NA;                             // first head-dim tile of this wave
  f32x4 dq[NA], dk[NA], dv[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) { dq[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dk[j] = dq[j]; dv[j] = dq[j]; }
  mma_b16<NA, true, true>(dq, Sh, Sl, LDT, wq * 16, Kh + 16 * t0, Kl + 16 * t0, LDB, TS, lane, one);     // dQ = dS K
  mma_b16<NA, false, true>(dk, Sh, Sl, LDT, wq * 16, Qh + 16 * t0, Ql + 16 * t0, LDB, TS, lane, one);    // dK = dS^T Q
  mma_b16<NA, false, true>(dv, Ph, Pl, LDT, wq * 16, Oh + 16 * t0, Ol + 16 * t0, LDB, TS, lane, one);    // dV = (P o M)^T dO
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int t = wq * 16 + 4 * (lane >> 4) + r;
    if (t >= Tv) continue;
    float* row = a.dqkv + ar.row0 * 3 * a.D + (long)t * rs + h * a.hd;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      const int c = 16 * (t0 + j) + (lane & 15);
      if (t0 + j < NTH && c < a.hd) { row[c] = dq[j][r]; row[a.D + c] = dk[j][r]; row[2 * a.D + c] = dv[j][r]; }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Multi-tile attention (T > 64: P12's 215 steps, PAM's 600) on the split-bf16 matrix path, scores chained in REGISTERS.
// The MFMA accumulator layout (lane l: column l & 15, rows 4 (l >> 4) + r) is, up to a permutation of the reduction index that
// the other operand can follow, the B-operand layout of the next product.  So the kernels form the scores with the OWNED
// dimension in the accumulator columns and feed them straight back:
//   forward / dQ (a wave owns 16 queries):  S^T = K Q^T, dP^T = V dO^T  ->  O^T += V^T (P o M)^T,  dQ^T += K^T dS^T
//   dK / dV      (a wave owns 16 keys):     S   = Q K^T, dP   = dO V^T  ->  dV^T += dO^T (P o M),  dK^T += Q^T dS
// The owned rows' own operand (Q, dO / K, V) lives in registers as B fragments read once from global memory; only the streamed
// 64-row tiles (K, V / Q, dO) go through LDS as hi/lo planes, whose transposed A fragments are two ds_read_b64_tr_b16 of FOUR
// rows each (frag_t2: rows 4G.. of two 16-row blocks -- the permutation the accumulators impose).  No P / dS planes, no
// transposing stores, one barrier less per tile, 53 KB of LDS instead of 98 - 143, 8 waves (128 owned rows) per workgroup, and the
// results leave as 16-byte stores (an accumulator holds 4 consecutive head columns of one row).
//  * a 64-key tile with no live key (padding: most P12 samples are far shorter than 215) contributes exactly nothing -- p = 0,
//    alpha = 1 -- and is skipped: one 64-bit "tile has a live key" word per sample, built from the key mask before the loop;
//  * the NEXT tile's rows are requested while the current tile is computed (register double buffer) and the loop's barriers
//    order LDS only (lds_barrier: no vmcnt drain).
// Same masks, same dropout quads (attn_quad), same saved LSE as the fp32 kernels; padded layout or token plan (AttnRows).
// ------------------------------------------------------------------------------------------------
constexpr int QW = 8;                   // waves per workgroup: 16-row blocks of the owned dimension
constexpr int QROWS = 16 * QW;
// dynamic LDS: the streamed tile's four planes [64][LDB] and the tile's key-mask bytes (forward, dQ) or its lse and delta (dK / dV)
constexpr size_t attn_mt_lds(int nth, bool dkv) {
  return (size_t)4 * TS * attn_ldb(nth) * sizeof(__bf16) + (dkv ? 2 * TS * sizeof(float) : TS);
}

// bit i: key tile i of sample b holds at least one live key (tiles >= 64 are never skipped)
__device__ __forceinline__ uint64_t live_key_tiles(const uint8_t* __restrict__ mrow, int T, int lane) {
  const int nt = (T + TS - 1) / TS;
  uint64_t live = 0ull;
  for (int i0 = 0; i0 < nt && i0 < 64; i0 += 4) {
    uint8_t mv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = (i0 + u) * TS + lane;
      const uint8_t m = mrow[min(key, T - 1)];
      mv[u] = key < T ? m : (uint8_t)1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (__ballot(mv[u] == 0) != 0ull && i0 + u < 64) live |= 1ull << (i0 + u);
  }
  return live;
}
// first live tile index >= i, or nt
__device__ __forceinline__ int next_live_tile(uint64_t live, int i, int nt) {
  while (i < nt && i < 64 && !((live >> i) & 1ull)) ++i;
  return i;
}

// The 8 consecutive head columns 32 ks + 8 G .. +7 of ONE row, per reduction step ks: a lane's share of a register-resident
// B operand (lane l: row l & 15 of the wave's 16, G = l >> 4).  Loads are unconditional from clamped addresses (raw_load);
// rows >= T and columns >= head_dim become zero in raw_split.
template <int NKS>
struct RawFrag { float4 v[NKS][2]; };
template <int NKS, bool VEC>
__device__ __forceinline__ void raw_load(RawFrag<NKS>& f, const float* __restrict__ row, int hd, int G) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int c = 32 * ks + 8 * G;
    if (VEC) {
      f.v[ks][0] = *reinterpret_cast<const float4*>(row + (c < hd ? c : 0));
      f.v[ks][1] = *reinterpret_cast<const float4*>(row + (c + 4 < hd ? c + 4 : 0));
    } else {
      float e[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) e[u] = row[c + u < hd ? c + u : 0];
      f.v[ks][0] = make_float4(e[0], e[1], e[2], e[3]);
      f.v[ks][1] = make_float4(e[4], e[5], e[6], e[7]);
    }
  }
}
template <int NKS>
__device__ __forceinline__ void raw_zero(RawFrag<NKS>& f, bool rok, int hd, int G) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    float* e = reinterpret_cast<float*>(&f.v[ks][0]);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (!(rok && 32 * ks + 8 * G + u < hd)) e[u] = 0.f;
  }
}
template <int NKS>
__device__ __forceinline__ void raw_split(const RawFrag<NKS>& f, abf8 (&fh)[NKS], abf8 (&fl)[NKS]) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const float* e = reinterpret_cast<const float*>(&f.v[ks][0]);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      fh[ks][u] = (__bf16)e[u];
      fl[ks][u] = (__bf16)(e[u] - (float)fh[ks][u]);
    }
  }
}
// two accumulator tiles (16-row blocks 2p and 2p+1 of the 64-row tile) -> the B operand of reduction step p:
// slots 0..3 = rows 32 p + 4 G + r, slots 4..7 = rows 32 p + 16 + 4 G + r (the order frag_t2 reads the other operand in)
__device__ __forceinline__ void pack_b(const float (&x0)[4], const float (&x1)[4], abf8& bh, abf8& bl) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    bh[r] = (__bf16)x0[r]; bl[r] = (__bf16)(x0[r] - (float)bh[r]);
    bh[4 + r] = (__bf16)x1[r]; bl[4 + r] = (__bf16)(x1[r] - (float)bh[4 + r]);
  }
}
// A fragment with the reduction index along the plane's rows, in the accumulator-imposed order: lane -> column col0 + (l & 15),
// rows ra + 4 G .. +3 then rb + 4 G .. +3
__device__ __forceinline__ abf8 frag_t2(const __bf16* P, int ld, int ra, int rb, int col0, int lane) {
  const int i = lane & 15, G = lane >> 4;
  const int o = (4 * G + (i >> 2)) * ld + col0 + 4 * (i & 3);
  const as4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((as4 __attribute__((address_space(3)))*)(P + ra * ld + o));
  const as4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((as4 __attribute__((address_space(3)))*)(P + rb * ld + o));
  const as8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(abf8, v);
}
template <bool ONE>
__device__ __forceinline__ void mfma3(f32x4& acc, const abf8& ah, const abf8& al, const abf8& bh, const abf8& bl) {
  if (!ONE) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
  }
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}
// acc[j] (rows = rows 16 j .. of the 64-row plane tile, columns = the wave's 16 owned rows) += plane(64 x HDP) . regs^T
template <int NKS, bool ONE>
__device__ __forceinline__ void mma_plane_regs(f32x4 (&acc)[4], const __bf16* Ph, const __bf16* Pl, int ld, const abf8 (&bh)[NKS],
                                               const abf8 (&bl)[NKS], int lane) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const abf8 ah = frag_n(Ph, ld, 16 * j, 32 * ks, lane);
      abf8 al = ah;
      if (!ONE) al = frag_n(Pl, ld, 16 * j, 32 * ks, lane);
      mfma3<ONE>(acc[j], ah, al, bh[ks], bl[ks]);
    }
}
// acc[ct] (rows = head columns 16 ct .., columns = the wave's 16 owned rows) += plane^T(HDP x 64) . x, x = the four accumulator
// tiles xs[j][r] of the 64 streamed rows
template <int NTH, bool ONE>
__device__ __forceinline__ void mma_planeT_acc(f32x4 (&acc)[NTH], const __bf16* Ph, const __bf16* Pl, int ld, const float (&xs)[4][4],
                                               int lane) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    abf8 bh, bl;
    pack_b(xs[2 * p], xs[2 * p + 1], bh, bl);
#pragma unroll
    for (int ct = 0; ct < NTH; ++ct) {
      const abf8 ah = frag_t2(Ph, ld, 32 * p, 32 * p + 16, 16 * ct, lane);
      abf8 al = ah;
      if (!ONE) al = frag_t2(Pl, ld, 32 * p, 32 * p + 16, 16 * ct, lane);
      mfma3<ONE>(acc[ct], ah, al, bh, bl);
    }
  }
}
// sum / max over the four 16-lane rows of the wavefront (lanes l, l^16, l^32, l^48): every lane gets the result
__device__ __forceinline__ float rows4_sum(float v) { v += __shfl_xor(v, 16); v += __shfl_xor(v, 32); return v; }
__device__ __forceinline__ float rows4_max(float v) { v = fmaxf(v, __shfl_xor(v, 16)); v = fmaxf(v, __shfl_xor(v, 32)); return v; }
// Dropout keep flags in the TRANSPOSED score layout (a lane: ONE query q, keys kb .. kb+3): the quad of (key, queries 4m .. 4m+3)
// is evaluated once, by the lane whose (l & 3) names the key, and the four lanes of a quad exchange their 4-bit results through
// DPP quad_perm -- the same number of generator calls as the query-major kernels.  Returns bit r = keep (q, kb + r).
__device__ __forceinline__ unsigned keep_bits_t(uint64_t seed, uint32_t site, int bh, int T, int q, int kb, int lane, float p) {
  const float4 u = uniform4(seed, site, attn_quad(bh, T, q, min(kb + (lane & 3), T - 1)));
  const int mine = (u.x >= p ? 1 : 0) | (u.y >= p ? 2 : 0) | (u.z >= p ? 4 : 0) | (u.w >= p ? 8 : 0);   // queries 4m .. 4m+3 of MY key
  const int sh = lane & 3;                                                                           // my query's component
  unsigned bits = 0;
  bits |= ((unsigned)__builtin_amdgcn_update_dpp(0, mine, 0x00, 0xf, 0xf, false) >> sh & 1u) << 0;
  bits |= ((unsigned)__builtin_amdgcn_update_dpp(0, mine, 0x55, 0xf, 0xf, false) >> sh & 1u) << 1;
  bits |= ((unsigned)__builtin_amdgcn_update_dpp(0, mine, 0xaa, 0xf, 0xf, false) >> sh & 1u) << 2;
  bits |= ((unsigned)__builtin_amdgcn_update_dpp(0, mine, 0xff, 0xf, 0xf, false) >> sh & 1u) << 3;
  return bits;
}
// a lane's 4 consecutive head columns 16 ct + 4 G .. of row `dst` (16-byte store when VEC)
template <bool VEC>
__device__ __forceinline__ void store_cols4(float* __restrict__ dst, int c, int hd, const f32x4& v, float s) {
  if (VEC) {
    if (c < hd) *reinterpret_cast<float4*>(dst + c) = make_float4(v[0] * s, v[1] * s, v[2] * s, v[3] * s);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (c + r < hd) dst[c + r] = v[r] * s;
  }
}

template <int NTH, bool VEC, bool ONE>
__global__ __launch_bounds__(64 * QW) void k_attn_fwd_b16(AttnArgs a) {
  RD_TOUCH_CODE_X(RD_TL_ATTN_FWD_B16, blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y, 512);
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  constexpr int HDP = 32 * ((16 * NTH + 31) / 32), LDB = HDP + 16, NKS = HDP / 32;
  __bf16* Kh = reinterpret_cast<__bf16*>(bsm);
  __bf16* Kl = Kh + TS * LDB;
  __bf16* Vh = Kl + TS * LDB;
  __bf16* Vl = Vh + TS * LDB;
  uint32_t* mk = reinterpret_cast<uint32_t*>(Vl + TS * LDB);   // key-mask bytes of the current tile (1 = dead)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = lane >> 4;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int qw0 = blockIdx.x * QROWS + wave * 16;             // the wave's first query
  const int q = qw0 + (lane & 15);
  // token plan (round 4): workgroup index b is a RANK, the sample's Tv = len rows sit at row0 .. (AttnRows); keys >= Tv are what
  // the mask would have removed, query / key super-tiles past Tv do not exist
  const AttnRows ar = attn_rows(a, b);
  const int Tv = ar.Tv;
  if ((int)blockIdx.x * QROWS >= Tv) return;                  // (padded layout: Tv == T, never)
  const long rs = ar.rstep * 3 * a.D;
  const float* qb = a.qkv + ar.row0 * 3 * a.D + h * a.hd;
  const uint8_t* mrow = a.mask + (long)b * a.T;
  const int nt = (Tv + TS - 1) / TS;
  // requests: my query row, key tile 0 (threads 0..255: K, 256..511: V; processed whether live or not -- a dead tile is an identity)
  RawFrag<NKS> qraw;
  raw_load<NKS, VEC>(qraw, qb + (long)min(q, Tv - 1) * rs, a.hd, G);
  const bool isv = tid >= 256;
  const int lt = tid & 255;
  const float* kvb = qb + (isv ? 2 : 1) * a.D;
  HeadRegs<NTH> kvr;
  head_load_t<NTH, VEC>(kvr, kvb, rs, 0, Tv, a.hd, lt);
  uint8_t mbyte = a.plan ? (uint8_t)0 : mrow[min(tid & 63, Tv - 1)];
  const uint64_t live = a.plan ? ~0ull : (live_key_tiles(mrow, Tv, lane) | 1ull);
  uint64_t seedv = a.seed;
  if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  abf8 qh[NKS], ql[NKS];
  raw_zero<NKS>(qraw, q < Tv, a.hd, G);
  raw_split<NKS>(qraw, qh, ql);
  float m_i = -INFINITY, l_i = 0.f;                            // l_i: this lane's keys only; combined over the 4 lane rows at the end
  f32x4 o[NTH];                                               // O^T: rows = head columns, column = my query
#pragma unroll
  for (int ct = 0; ct < NTH; ++ct) o[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int kt = 0;
  while (kt < nt) {
    const int k0 = kt * TS;
    lds_barrier();                                            // the previous tile's products have read the planes
    head_store_b16<NTH>(kvr, isv ? Vh : Kh, isv ? Vl : Kl, LDB, HDP, lt);
    if (tid < TS) reinterpret_cast<uint8_t*>(mk)[tid] = (k0 + tid < Tv) ? mbyte : (uint8_t)1;
    const int kn = next_live_tile(live, kt + 1, nt);
    if (kn < nt) {                                            // in flight during this tile's products
      head_load_t<NTH, VEC>(kvr, kvb, rs, kn * TS, Tv, a.hd, lt);
      if (!a.plan) mbyte = mrow[min(kn * TS + (tid & 63), Tv - 1)];
    }
    lds_barrier();
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    mma_plane_regs<NKS, ONE>(s, Kh, Kl, LDB, qh, ql, lane);    // S^T = K Q^T: rows = keys 16 j + 4 G + r, column = my query
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t dm = mk[4 * j + G];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[j][r] = ((dm >> (8 * r)) & 0xffu) ? -INFINITY : s[j][r] * a.scale;
        mx = fmaxf(mx, s[j][r]);
      }
    }
    const float mn = fmaxf(m_i, rows4_max(mx));
    const float alpha = (m_i == -INFINITY) ? 0.f : expf(m_i - mn);
    m_i = mn;
    float rsum = 0.f, pm[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned kb = 0xfu;
      if (a.p_drop > 0.f) kb = keep_bits_t(seedv, a.site, bh, a.T, q, k0 + 16 * j + 4 * G, lane, a.p_drop);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (s[j][r] == -INFINITY) ? 0.f : __expf(s[j][r] - m_i);
        rsum += p;
        pm[j][r] = ((kb >> r) & 1u) ? (a.p_drop > 0.f ? p * inv_keep : p) : 0.f;   // F.dropout on the probabilities (after the softmax sum)
      }
    }
    l_i = l_i * alpha + rsum;
#pragma unroll
    for (int ct = 0; ct < NTH; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[ct][r] *= alpha;
    mma_planeT_acc<NTH, ONE>(o, Vh, Vl, LDB, pm, lane);        // O^T += V^T (P o M)^T
    kt = kn;
  }
  const float l = rows4_sum(l_i);
  if (q < Tv) {
    const float inv = 1.0f / l;
    float* orow = a.out + (ar.row0 + (long)q * ar.rstep) * a.D + h * a.hd;
#pragma unroll
    for (int ct = 0; ct < NTH; ++ct) store_cols4<VEC>(orow, 16 * ct + 4 * G, a.hd, o[ct], inv);
    if (G == 0) a.lse[(long)bh * a.T + q] = m_i + logf(l);
  }
}

// dQ (and delta = rowsum(dO * O)): grid (query super-tiles, B*H); a wave owns 16 queries
template <int NTH, bool VEC, bool ONE>
__global__ __launch_bounds__(64 * QW) void k_attn_bwd_dq_b16(AttnArgs a) {
  RD_TOUCH_CODE_X(RD_TL_ATTN_BWD_DQ, blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y, 512);
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  constexpr int HDP = 32 * ((16 * NTH + 31) / 32), LDB = HDP + 16, NKS = HDP / 32;
  __bf16* Kh = reinterpret_cast<__bf16*>(bsm);
  __bf16* Kl = Kh + TS * LDB;
  __bf16* Vh = Kl + TS * LDB;
  __bf16* Vl = Vh + TS * LDB;
  uint32_t* mk = reinterpret_cast<uint32_t*>(Vl + TS * LDB);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = lane >> 4;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int qw0 = blockIdx.x * QROWS + wave * 16;
  const int q = qw0 + (lane & 15);
  const AttnRows ar = attn_rows(a, b);                        // token plan: see k_attn_fwd_b16
  const int Tv = ar.Tv;
  if ((int)blockIdx.x * QROWS >= Tv) return;
  const int qc = min(q, Tv - 1);
  const long rs = ar.rstep * 3 * a.D, ro = ar.rstep * a.D;
  const float* qb = a.qkv + ar.row0 * 3 * a.D + h * a.hd;
  const uint8_t* mrow = a.mask + (long)b * a.T;
  const int nt = (Tv + TS - 1) / TS;
  RawFrag<NKS> qraw, doraw, oraw;
  raw_load<NKS, VEC>(qraw, qb + (long)qc * rs, a.hd, G);
  raw_load<NKS, VEC>(doraw, a.dout + ar.row0 * a.D + h * a.hd + (long)qc * ro, a.hd, G);
  raw_load<NKS, VEC>(oraw, a.out + ar.row0 * a.D + h * a.hd + (long)qc * ro, a.hd, G);
  const float lse_q = a.lse[(long)bh * a.T + qc];
  const bool isv = tid >= 256;
  const int lt = tid & 255;
  const float* kvb = qb + (isv ? 2 : 1) * a.D;
  HeadRegs<NTH> kvr;
  head_load_t<NTH, VEC>(kvr, kvb, rs, 0, Tv, a.hd, lt);
  uint8_t mbyte = a.plan ? (uint8_t)0 : mrow[min(tid & 63, Tv - 1)];
  const uint64_t live = a.plan ? ~0ull : (live_key_tiles(mrow, Tv, lane) | 1ull);
  uint64_t seedv = a.seed;
  if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
  const float inv_keep = 1.0f / (1.0f - a.p_drop);
  abf8 qh[NKS], ql[NKS], gh[NKS], gl[NKS];                     // Q and dO rows of my query, as B operands
  const bool qok = q < Tv;
  raw_zero<NKS>(qraw, qok, a.hd, G);
  raw_zero<NKS>(doraw, qok, a.hd, G);
  raw_zero<NKS>(oraw, qok, a.hd, G);
  float dsum = 0.f;                                           // delta = rowsum(dO * O), in fp32
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const float* x = reinterpret_cast<const float*>(&doraw.v[ks][0]);
    const float* y = reinterpret_cast<const float*>(&oraw.v[ks][0]);
#pragma unroll
    for (int u = 0; u < 8; ++u) dsum += x[u] * y[u];
  }
  const float dl_q = rows4_sum(dsum);
  if (qok && G == 0) a.delta[(long)bh * a.T + q] = dl_q;
  raw_split<NKS>(qraw, qh, ql);
  raw_split<NKS>(doraw, gh, gl);
  f32x4 dq[NTH];                                              // dQ^T: rows = head columns, column = my query
#pragma unroll
  for (int ct = 0; ct < NTH; ++ct) dq[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int kt = 0;
  while (kt < nt) {
    const int k0 = kt * TS;
    lds_barrier();
    head_store_b16<NTH>(kvr, isv ? Vh : Kh, isv ? Vl : Kl, LDB, HDP, lt);
    if (tid < TS) reinterpret_cast<uint8_t*>(mk)[tid] = (k0 + tid < Tv) ? mbyte : (uint8_t)1;
    const int kn = next_live_tile(live, kt + 1, nt);
    if (kn < nt) {
      head_load_t<NTH, VEC>(kvr, kvb, rs, kn * TS, Tv, a.hd, lt);
      if (!a.plan) mbyte = mrow[min(kn * TS + (tid & 63), Tv - 1)];
    }
    lds_barrier();
    f32x4 s[4], dp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[j] = s[j]; }
    mma_plane_regs<NKS, ONE>(s, Kh, Kl, LDB, qh, ql, lane);    // S^T  = K Q^T
    mma_plane_regs<NKS, ONE>(dp, Vh, Vl, LDB, gh, gl, lane);   // dP^T = V dO^T
    float ds[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t dm = mk[4 * j + G];
      unsigned kb = 0xfu;
      if (a.p_drop > 0.f) kb = keep_bits_t(seedv, a.site, bh, a.T, q, k0 + 16 * j + 4 * G, lane, a.p_drop);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ds[j][r] = 0.f;
        if (!((dm >> (8 * r)) & 0xffu) && qok) {
          const float p = __expf(s[j][r] * a.scale - lse_q);
          const float k = ((kb >> r) & 1u) ? (a.p_drop > 0.f ? inv_keep : 1.f) : 0.f;
          ds[j][r] = p * (dp[j][r] * k - dl_q) * a.scale;
        }
      }
    }
    mma_planeT_acc<NTH, ONE>(dq, Kh, Kl, LDB, ds, lane);       // dQ^T += K^T dS^T
    kt = kn;
  }
  if (qok) {
    float* row = a.dqkv + (ar.row0 + (long)q * ar.rstep) * 3 * a.D + h * a.hd;
#pragma unroll
    for (int ct = 0; ct < NTH; ++ct) store_cols4<VEC>(row, 16 * ct + 4 * G, a.hd, dq[ct], 1.f);
  }
}

// dK / dV: grid (key super-tiles, B*H); a wave owns 16 keys, K and V rows in registers, the Q / dO tiles stream through LDS.
// A workgroup whose 128 keys are all dead writes zeros and leaves; a wave whose 16 keys are all dead only helps with the tiles.
template <int NTH, bool VEC, bool ONE>
__global__ __launch_bounds__(64 * QW) void k_attn_bwd_dkv_b16(AttnArgs a) {
  RD_TOUCH_CODE_X(RD_TL_ATTN_BWD_DKV, blockIdx.x + blockIdx.y * gridDim.x + blockIdx.z * gridDim.x * gridDim.y, 512);
  extern __shared__ __attribute__((aligned(16))) unsigned char bsm[];
  constexpr int HDP = 32 * ((16 * NTH + 31) / 32), LDB = HDP + 16, NKS = HDP / 32;
  __bf16* Qh = reinterpret_cast<__bf16*>(bsm);
  __bf16* Ql = Qh + TS * LDB;
  __bf16* Oh = Ql + TS * LDB;                       // dO
  __bf16* Ol = Oh + TS * LDB;
  float* lse_s = reinterpret_cast<float*>(Ol + TS * LDB);
  float* dl_s = lse_s + TS;
  __shared__ int any_live_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = lane >> 4;
  const int bh = blockIdx.y, b = bh / a.H, h = bh - b * a.H;
  const int key = blockIdx.x * QROWS + wave * 16 + (lane & 15);
  const AttnRows ar = attn_rows(a, b);                        // token plan: see k_attn_fwd_b16 (rows >= Tv do not exist: nothing to zero)
  const int Tv = ar.Tv;
  if ((int)blockIdx.x * QROWS >= Tv) return;
  const int kc = min(key, Tv - 1);
  const long rs = ar.rstep * 3 * a.D, ro = ar.rstep * a.D;
  const float* qb = a.qkv + ar.row0 * 3 * a.D + h * a.hd;
  const float* dob = a.dout + ar.row0 * a.D + h * a.hd;
  const uint8_t* mrow = a.mask + (long)b * a.T;
  RawFrag<NKS> kraw, vraw;
  raw_load<NKS, VEC>(kraw, qb + a.D + (long)kc * rs, a.hd, G);
  raw_load<NKS, VEC>(vraw, qb + 2 * a.D + (long)kc * rs, a.hd, G);
  const uint8_t mkey = a.plan ? (uint8_t)0 : mrow[kc];
  // first query tile (threads 0..255: Q, 256..511: dO), lse / delta of its rows (threads 0..63)
  const bool isg = tid >= 256;
  const int lt = tid & 255;
  const float* tb = isg ? dob : qb;
  const long ts = isg ? ro : rs;
  HeadRegs<NTH> tr;
  head_load_t<NTH, VEC>(tr, tb, ts, 0, Tv, a.hd, lt);
  float lq = a.lse[(long)bh * a.T + min(tid & 63, Tv - 1)], dlq = a.delta[(long)bh * a.T + min(tid & 63, Tv - 1)];
  const bool dead = key >= Tv || mkey;
  const bool wave_live = __ballot(!dead) != 0ull;
  if (tid == 0) any_live_s = 0;
  __syncthreads();
  if (wave_live && lane == 0) any_live_s = 1;
  __syncthreads();
  const bool any_live = any_live_s != 0;
  f32x4 dk[NTH], dv[NTH];                                     // dK^T, dV^T: rows = head columns, column = my key
#pragma unroll
  for (int ct = 0; ct < NTH; ++ct) { dk[ct] = (f32x4){0.f, 0.f, 0.f, 0.f}; dv[ct] = dk[ct]; }
  if (any_live) {
    abf8 kh[NKS], kl[NKS], vh[NKS], vl[NKS];
    raw_zero<NKS>(kraw, key < Tv, a.hd, G);
    raw_zero<NKS>(vraw, key < Tv, a.hd, G);
    raw_split<NKS>(kraw, kh, kl);
    raw_split<NKS>(vraw, vh, vl);
    uint64_t seedv = a.seed;
    if (a.p_drop > 0.f && a.seed_cell) seedv += load_uniform_u64(a.seed_cell);
    const float inv_keep = 1.0f / (1.0f - a.p_drop);
    for (int q0 = 0; q0 < Tv; q0 += TS) {
      lds_barrier();                                          // the previous query tile's products have read the planes
      head_store_b16<NTH>(tr, isg ? Oh : Qh, isg ? Ol : Ql, LDB, HDP, lt);
      if (tid < TS) { lse_s[tid] = lq; dl_s[tid] = dlq; }
      if (q0 + TS < Tv) {                                     // next query tile, in flight during this one's products
        head_load_t<NTH, VEC>(tr, tb, ts, q0 + TS, Tv, a.hd, lt);
        lq = a.lse[(long)bh * a.T + min(q0 + TS + (tid & 63), Tv - 1)];
        dlq = a.delta[(long)bh * a.T + min(q0 + TS + (tid & 63), Tv - 1)];
      }
      lds_barrier();
      if (!wave_live) continue;                               // uniform per wave; the barriers above are still met
      f32x4 s[4], dp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { s[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dp[j] = s[j]; }
      mma_plane_regs<NKS, ONE>(s, Qh, Ql, LDB, kh, kl, lane);  // S  = Q K^T: rows = queries 16 j + 4 G + r, column = my key
      mma_plane_regs<NKS, ONE>(dp, Oh, Ol, LDB, vh, vl, lane); // dP = dO V^T
      float pm[4][4], ds[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int qj = q0 + 16 * j + 4 * G;
        float k4[4] = {1.f, 1.f, 1.f, 1.f};
        if (a.p_drop > 0.f) attn_keep4(k4, seedv, a.site, bh, a.T, qj, kc, a.p_drop, inv_keep);
        const float4 l4 = *reinterpret_cast<const float4*>(lse_s + 16 * j + 4 * G);
        const float4 d4 = *reinterpret_cast<const float4*>(dl_s + 16 * j + 4 * G);
        const float lr[4] = {l4.x, l4.y, l4.z, l4.w}, dr[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pm[j][r] = 0.f; ds[j][r] = 0.f;
          if (!dead && qj + r < Tv) {
            const float p = __expf(s[j][r] * a.scale - lr[r]);
            pm[j][r] = p * k4[r];
            ds[j][r] = p * (dp[j][r] * k4[r] - dr[r]) * a.scale;
          }
        }
      }
      mma_planeT_acc<NTH, ONE>(dv, Oh, Ol, LDB, pm, lane);     // dV^T += dO^T (P o M)
      mma_planeT_acc<NTH, ONE>(dk, Qh, Ql, LDB, ds, lane);     // dK^T += Q^T dS
    }
  }
  if (key < Tv) {
    float* row = a.dqkv + (ar.row0 + (long)key * ar.rstep) * 3 * a.D + h * a.hd;
#pragma unroll
    for (int ct = 0; ct < NTH; ++ct) {
      store_cols4<VEC>(row + a.D, 16 * ct + 4 * G, a.hd, dk[ct], 1.f);
      store_cols4<VEC>(row + 2 * a.D, 16 * ct + 4 * G, a.hd, dv[ct], 1.f);
    }
  }
}

// ---- the route of an attention pass ----------------------------------------------------------------------------------------------
// Which kernels one forward or backward of the core runs, in the current arithmetic mode and switches, and the geometry of each
// launch.  Decided HERE and nowhere else, once per pass; no HIP call, so rd_debug_attention_route (include/raindrop_hip_debug.h)
// answers without a device from the very functions the launch runs.  aligned: qkv, out and dout all start on 16-byte boundaries.
enum AttnPass { ATTN_FWD = 0, ATTN_BWD = 1, ATTN_IS_BIG = 2 };      // ATTN_IS_BIG: `family == ATTN_BIG` or not alone (attn_big: the size queries)
enum AttnFamily { ATTN_FP32 = 0, ATTN_ONE_B16 = 1, ATTN_MT_B16 = 2, ATTN_BIG = 3 };   // exact fp32 tiled | single-tile, multi-tile split-bf16 | materialised scores
enum AttnKernel { AK_FWD, AK_BWD_DQ, AK_BWD_DKV, AK_BWD_ONE, AK_FWD_ONE_B16, AK_FWD_ONE_B16W, AK_BWD_ONE_B16, AK_BWD_ONE_B16W,
                  AK_FWD_B16, AK_BWD_DQ_B16, AK_BWD_DKV_B16 };      // attn_route: an eight-wave kernel is its four-wave form + 1
struct AttnLaunch {
  int kernel; dim3 grid; int block;      // kernel: AttnKernel
  size_t lds_attr, lds;                  // dynamic LDS bytes: the kernel's opt-in (its largest launch) and this launch's
  const char* name;                      // what the launch reports to the error check and the launch log
};
struct AttnRoute {
  int family;            // AttnFamily
  int nth;               // 16-column tiles of a head, ceil(head_dim / 16): 1..6
  bool vec;              // 16-byte head-tile loads: every row of every head starts on a 16-byte boundary.  Compiled into the kernels
                         // (template flag): as a runtime flag the compiler merged the two load forms into four 4-byte loads per chunk
  bool one_product;      // split-bf16 families in RD_PREC_BF16: hi*hi only
  bool wide;             // ATTN_ONE_B16: the eight-wave kernels
  int nlaunch;           // 0: ATTN_BIG (attn_big_fwd / attn_big_bwd run it); 2: a backward over several key tiles, dq (+ delta) then dk / dv
  AttnLaunch l[2];
};

// Whole literals, by AttnKernel: the launch log keeps the pointer, and the tests match on these names.  attn_route names each launch
// as it adds it: this is the name of the route's last one ("" before the first).
static const char* attn_name(const AttnRoute& r) {
  static const char* const names[11] = {"k_attn_fwd", "k_attn_bwd_dq", "k_attn_bwd_dkv", "k_attn_bwd_one", "k_attn_fwd_one_b16", "k_attn_fwd_one_b16w",
                                        "k_attn_bwd_one_b16", "k_attn_bwd_one_b16w", "k_attn_fwd_b16", "k_attn_bwd_dq_b16", "k_attn_bwd_dkv_b16"};
  return r.nlaunch > 0 ? names[r.l[r.nlaunch - 1].kernel] : "";
}

static AttnRoute attn_route(AttnPass pass, int T, int B, int D, int H, int hd, bool with_plan, bool aligned) {
  // read once per process
  static const bool fwd_w8 = [] { const char* e = getenv("RD_ATTN_FWD_W8"); return !(e && atoi(e) == 0); }();
  static const bool bwd_w8 = [] { const char* e = getenv("RD_ATTN_BWD_W8"); return !(e && atoi(e) == 0); }();
  // read per call (tests compare both paths in one process; the saved / workspace sizes follow RD_ATTN_BIG)
  auto on = [](const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; };
  AttnRoute r{};
  if (hd > ATTN_MAX_HD || on("RD_ATTN_BIG", false)) r.family = ATTN_BIG;
  if (r.family == ATTN_BIG || pass == ATTN_IS_BIG) return r;
  const bool fwd = pass == ATTN_FWD, b16 = precision() != RD_PREC_FP32;
  r.nth = cdiv(hd, 16);
  r.vec = (hd & 3) == 0 && (D & 3) == 0 && aligned;
  auto add = [&](int kernel, dim3 grid, int block, size_t lds) {
    r.l[r.nlaunch++] = AttnLaunch{kernel, grid, block, lds, lds, nullptr};
    r.l[r.nlaunch - 1].name = attn_name(r);
  };
  if (b16 && T <= TS && on("RD_ATTN_B16", true)) {                // one workgroup per (sample, head)
    r.family = ATTN_ONE_B16;
    r.wide = (fwd ? fwd_w8 : bwd_w8) || with_plan;                // of the two forms only the eight-wave one reads a plan
    add((fwd ? AK_FWD_ONE_B16 : AK_BWD_ONE_B16) + r.wide, dim3(B * H), r.wide ? 512 : 256,
        fwd ? attn_fwd_one_b16_lds(r.nth, r.wide) : attn_bwd_one_b16_lds(r.nth));
  } else if (b16 && T > TS && on("RD_ATTN_B16_MT", true)) {       // a workgroup owns 128 queries (dk / dv: keys)
    r.family = ATTN_MT_B16;
    const dim3 grid(cdiv(T, QROWS), B * H);
    add(fwd ? AK_FWD_B16 : AK_BWD_DQ_B16, grid, 64 * QW, attn_mt_lds(r.nth, false));
    if (!fwd) add(AK_BWD_DKV_B16, grid, 64 * QW, attn_mt_lds(r.nth, true));
  } else {
    r.family = ATTN_FP32;
    const dim3 grid(cdiv(T, TS), B * H);
    if (fwd) { add(AK_FWD, grid, 256, attn_fwd_lds(r.nth, TS + 1)); r.l[0].lds = attn_fwd_lds(r.nth, T); }     // less where P overlays Q
    else if (T <= TS) add(AK_BWD_ONE, dim3(B * H), 256, attn_bwd_lds(r.nth, 2));      // single tile: S, P, dP, dS formed once
    else { add(AK_BWD_DQ, grid, 256, attn_bwd_lds(r.nth, 1)); add(AK_BWD_DKV, grid, 256, attn_bwd_lds(r.nth, 2)); }
  }
  r.one_product = r.family != ATTN_FP32 && precision() == RD_PREC_BF16;
  return r;
}

// what a pass refuses: the calls that reach it have taken the materialised form elsewhere (the layer) or refused it (rd_attention_*)
static int attn_check(const AttnRoute& r, int hd, bool with_plan) {
  if (with_plan && r.family != ATTN_ONE_B16 && r.family != ATTN_MT_B16)
    return fail(RD_EUNSUPPORTED, "token plan: only the split-bf16 attention kernels (head_dim <= 96, bf16 modes) read it");
  if (r.family != ATTN_BIG) return RD_OK;
  return hd > ATTN_MAX_HD ? fail(RD_EUNSUPPORTED, "attention head_dim %d > 96 not built", hd)
                          : fail(RD_EUNSUPPORTED, "attention: RD_ATTN_BIG takes the materialised scores, which only the layer runs");
}

// ---- one launcher: (kernel, nth, vec, one_product) -> the instantiation ----------------------------------------------------------
template <auto KERNEL, class... One>
static int attn_run(const AttnLaunch& l, const AttnArgs& a, hipStream_t st, One... one) {
  // dynamic-LDS opt-in, once per process and kernel (RD_LDS_ATTR, under the route's name): lds_attr depends on the instantiation only
  static const hipError_t attr = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.lds_attr);
  if (attr != hipSuccess) return fail((int)attr, "hipFuncSetAttribute(%s): %s", l.name, hipGetErrorString(attr));
  hipLaunchKernelGGL(KERNEL, l.grid, dim3(l.block), l.lds, st, a, one...);
  return check_launch(l.name);
}
// f(NTH, VEC) with the head's tile count (1..6) and the load form as compile-time constants
template <int NTH = 1, class F>
static int by_head(const AttnRoute& r, F&& f) {
  if constexpr (NTH < 6)
    if (r.nth > NTH) return by_head<NTH + 1>(r, f);
  return r.vec ? f(std::integral_constant<int, NTH>{}, std::true_type{}) : f(std::integral_constant<int, NTH>{}, std::false_type{});
}
// launch i of the route.  The single-tile split-bf16 kernels take one_product as an argument, the multi-tile ones as a template flag
static int attn_launch(AttnArgs a, const AttnRoute& r, int i, hipStream_t st) {
  const AttnLaunch& l = r.l[i];
  a.stamps = g_attn_stamps;                      // k_attn_*_one_b16 alone write stamps
  const int one = r.one_product;
  return by_head(r, [&](auto nth, auto vec) {
    constexpr int N = decltype(nth)::value; constexpr bool V = decltype(vec)::value;
    switch (l.kernel) {
      case AK_FWD: return attn_run<k_attn_fwd<N, V>>(l, a, st);
      case AK_BWD_DQ: return attn_run<k_attn_bwd_dq<N, V>>(l, a, st);
      case AK_BWD_DKV: return attn_run<k_attn_bwd_dkv<N, V>>(l, a, st);
      case AK_BWD_ONE: return attn_run<k_attn_bwd_one<N, V>>(l, a, st);
      case AK_FWD_ONE_B16: return attn_run<k_attn_fwd_one_b16<N, V>>(l, a, st, one);
      case AK_FWD_ONE_B16W: return attn_run<k_attn_fwd_one_b16w<N, V>>(l, a, st, one);
      case AK_BWD_ONE_B16: return attn_run<k_attn_bwd_one_b16<N, V>>(l, a, st, one);
      case AK_BWD_ONE_B16W: return attn_run<k_attn_bwd_one_b16w<N, V>>(l, a, st, one);
      case AK_FWD_B16: return one ? attn_run<k_attn_fwd_b16<N, V, true>>(l, a, st) : attn_run<k_attn_fwd_b16<N, V, false>>(l, a, st);
      case AK_BWD_DQ_B16: return one ? attn_run<k_attn_bwd_dq_b16<N, V, true>>(l, a, st) : attn_run<k_attn_bwd_dq_b16<N, V, false>>(l, a, st);
      default: return one ? attn_run<k_attn_bwd_dkv_b16<N, V, true>>(l, a, st) : attn_run<k_attn_bwd_dkv_b16<N, V, false>>(l, a, st);
    }
  });
}

// ------------------------------------------------------------------------------------------------
// Wide heads (head_dim > 96: the 256-sensor stress shape, D = 1040, 2 heads of 520): the score matrix is MATERIALISED.
// At head_dim 520 and T = 512 the products are large square GEMMs (MFMA-bound), so the flash-style
// tiling above buys nothing: S = scale Q K^T, P = softmax(S + key mask), O = dropout(P) V run as batched tiled GEMMs
// (one problem per (sample, head), rd_gemm.hip) around a row-softmax kernel; P and dropout(P) are saved for the backward
// (2 B H T^2 floats).  Same masks and the same Philox quads (attn_quad) as the tiled kernels.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_softmax_rows(float* __restrict__ S, float* __restrict__ PD, const uint8_t* __restrict__ mask,
                                                      int T, int H, long rows, float p_drop, uint64_t seed, uint32_t site,
                                                      const uint64_t* cell) {
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= rows) return;
  seed = eff_seed(seed, cell);
  const int bh = (int)(row / T), q = (int)(row - (long)bh * T), b = bh / H;
  float* s = S + row * T;
  float m = -INFINITY;
  for (int k = lane; k < T; k += 64)
    if (!mask[(long)b * T + k]) m = fmaxf(m, s[k]);
  m = wave_max64(m);
  float sum = 0.f;
  for (int k = lane; k < T; k += 64)
    if (!mask[(long)b * T + k]) sum += __expf(s[k] - m);
  sum = wave_sum64(sum);
  const float inv = 1.0f / sum, inv_keep = 1.0f / (1.0f - p_drop);
  for (int k = lane; k < T; k += 64) {
    const float p = mask[(long)b * T + k] ? 0.f : __expf(s[k] - m) * inv;
    s[k] = p;
    PD[row * T + k] = p_drop > 0.f ? p * attn_keep1(seed, site, bh, T, q, k, p_drop, inv_keep) : p;
  }
}
// dS = P o (dP - rowsum(P o dP)) * scale with dP = dPD o keep, in place over dPD
__global__ __launch_bounds__(256) void k_softmax_bwd_rows(const float* __restrict__ P, float* __restrict__ dPD, int T, long rows,
                                                          float scale, float p_drop, uint64_t seed, uint32_t site,
                                                          const uint64_t* cell) {
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= rows) return;
  seed = eff_seed(seed, cell);
  const int bh = (int)(row / T), q = (int)(row - (long)bh * T);
  const float* p = P + row * T;
  float* d = dPD + row * T;
  const float inv_keep = 1.0f / (1.0f - p_drop);
  float delta = 0.f;
  for (int k = lane; k < T; k += 64) {
    float dp = d[k];
    if (p_drop > 0.f) dp *= attn_keep1(seed, site, bh, T, q, k, p_drop, inv_keep);
    d[k] = dp;
    delta += p[k] * dp;
  }
  delta = wave_sum64(delta);
  for (int k = lane; k < T; k += 64) d[k] = p[k] * (d[k] - delta) * scale;
}

static GemmArgs bh_gemm(const AttnArgs& a, int M, int N, int K) {
  GemmArgs g{};
  g.M = M; g.N = N; g.K = K; g.nsplit = 1; g.nbatch = a.B * a.H; g.batch_inner = a.H;
  return g;
}
}  // namespace

// P, PD: [B*H][T][T] each (saved)
int attn_big_fwd(const AttnArgs& a, float* P, float* PD, hipStream_t st) {
  const long rs = (long)a.B * 3 * a.D, TT = (long)a.T * a.T;
  int rc;
  GemmArgs g = bh_gemm(a, a.T, a.T, a.hd);                                  // S = scale Q K^T
  g.A = a.qkv; g.sa_m = rs; g.sa_k = 1; g.a_bo = 3 * a.D; g.a_bi = a.hd;
  g.B = a.qkv + a.D; g.sb_n = rs; g.sb_k = 1; g.b_bo = 3 * a.D; g.b_bi = a.hd;
  g.C = P; g.sc_m = a.T; g.c_bo = (long)a.H * TT; g.c_bi = TT; g.cscale = a.scale;
  if ((rc = launch_gemm(g, st))) return rc;
  const long rows = (long)a.B * a.H * a.T;
  hipLaunchKernelGGL(k_softmax_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, P, PD, a.mask, a.T, a.H, rows, a.p_drop,
                     a.seed, a.site, a.seed_cell);
  if ((rc = check_launch("k_softmax_rows"))) return rc;
  g = bh_gemm(a, a.T, a.hd, a.T);                                           // O = PD V
  g.A = PD; g.sa_m = a.T; g.sa_k = 1; g.a_bo = (long)a.H * TT; g.a_bi = TT;
  g.B = a.qkv + 2 * a.D; g.sb_n = 1; g.sb_k = rs; g.b_bo = 3 * a.D; g.b_bi = a.hd;
  g.C = a.out; g.sc_m = (long)a.B * a.D; g.c_bo = a.D; g.c_bi = a.hd;
  return launch_gemm(g, st);
}
// dS: [B*H][T][T] workspace
int attn_big_bwd(const AttnArgs& a, const float* P, const float* PD, float* dS, hipStream_t st) {
  const long rs = (long)a.B * 3 * a.D, ro = (long)a.B * a.D, TT = (long)a.T * a.T;
  int rc;
  GemmArgs g = bh_gemm(a, a.T, a.T, a.hd);                                  // dPD = dO V^T
  g.A = a.dout; g.sa_m = ro; g.sa_k = 1; g.a_bo = a.D; g.a_bi = a.hd;
  g.B = a.qkv + 2 * a.D; g.sb_n = rs; g.sb_k = 1; g.b_bo = 3 * a.D; g.b_bi = a.hd;
  g.C = dS; g.sc_m = a.T; g.c_bo = (long)a.H * TT; g.c_bi = TT;
  if ((rc = launch_gemm(g, st))) return rc;
  g = bh_gemm(a, a.T, a.hd, a.T);                                           // dV = PD^T dO
  g.A = PD; g.sa_m = 1; g.sa_k = a.T; g.a_bo = (long)a.H * TT; g.a_bi = TT;
  g.B = a.dout; g.sb_n = 1; g.sb_k = ro; g.b_bo = a.D; g.b_bi = a.hd;
  g.C = a.dqkv + 2 * a.D; g.sc_m = rs; g.c_bo = 3 * a.D; g.c_bi = a.hd;
  if ((rc = launch_gemm(g, st))) return rc;
  const long rows = (long)a.B * a.H * a.T;
  hipLaunchKernelGGL(k_softmax_bwd_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, P, dS, a.T, rows, a.scale, a.p_drop,
                     a.seed, a.site, a.seed_cell);
  if ((rc = check_launch("k_softmax_bwd_rows"))) return rc;
  g = bh_gemm(a, a.T, a.hd, a.T);                                           // dQ = dS K
  g.A = dS; g.sa_m = a.T; g.sa_k = 1; g.a_bo = (long)a.H * TT; g.a_bi = TT;
  g.B = a.qkv + a.D; g.sb_n = 1; g.sb_k = rs; g.b_bo = 3 * a.D; g.b_bi = a.hd;
  g.C = a.dqkv; g.sc_m = rs; g.c_bo = 3 * a.D; g.c_bi = a.hd;
  if ((rc = launch_gemm(g, st))) return rc;
  g = bh_gemm(a, a.T, a.hd, a.T);                                           // dK = dS^T Q
  g.A = dS; g.sa_m = 1; g.sa_k = a.T; g.a_bo = (long)a.H * TT; g.a_bi = TT;
  g.B = a.qkv; g.sb_n = 1; g.sb_k = rs; g.b_bo = 3 * a.D; g.b_bi = a.hd;
  g.C = a.dqkv + a.D; g.sc_m = rs; g.c_bo = 3 * a.D; g.c_bi = a.hd;
  return launch_gemm(g, st);
}

static int attn_pass(AttnPass pass, const AttnArgs& a, hipStream_t st) {
  auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const AttnRoute r = attn_route(pass, a.T, a.B, a.D, a.H, a.hd, a.plan != nullptr, al(a.qkv) && al(a.out) && al(a.dout));
  int rc = attn_check(r, a.hd, a.plan != nullptr);
  for (int i = 0; i < r.nlaunch && !rc; ++i) rc = attn_launch(a, r, i, st);
  return rc;
}
int attn_forward(const AttnArgs& a, hipStream_t st) { return attn_pass(ATTN_FWD, a, st); }
int attn_backward(const AttnArgs& a, hipStream_t st) { return attn_pass(ATTN_BWD, a, st); }
bool attn_big(const EncDims& e) { return attn_route(ATTN_IS_BIG, e.T, e.B, e.D, e.H, e.Hd, false, true).family == ATTN_BIG; }
}  // namespace rd

using namespace rd;

extern "C" void rd_debug_set_attn_stamps(void* p) { g_attn_stamps = (unsigned long long*)p; }   // not part of the ABI

// The attention core alone (torch F.multi_head_attention_forward between in_proj and out_proj, as used by the encoder layer of
// code/models_rd.py:235-237,358): qkv [T,B,3D] -> out [T,B,D], lse [B,H,T]; backward: dout -> dqkv.  Same kernels and dispatch as
// inside rd_encoder_layer_fwd/bwd; exposed so that this sub-graph (no ReLU gate in it) can be held to a tight bound against the
// oracle by itself (tests/test_gpu_parity.py::test_attention_core_vs_float64).
extern "C" int rd_attention_fwd(const rd_shape* s, int32_t layer, const float* qkv, const uint8_t* mask, float p_drop, uint64_t seed,
                                float* out, float* lse, void* stream) {
  int rc = check_enc(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(qkv && mask && out && lse, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  const EncDims e = enc_dims(s);
  RD_REQUIRE(!attn_big(e), "rd_attention_fwd: head_dim %d > 96 runs as materialised products inside the layer only", e.Hd);
  return attn_forward(attn_args(e, qkv, mask, out, lse, p_drop, seed, (uint32_t)layer, token_plan()), (hipStream_t)stream);
}
// delta_ws: [B,H,T] floats of scratch
extern "C" int rd_attention_bwd(const rd_shape* s, int32_t layer, const float* qkv, const uint8_t* mask, float p_drop, uint64_t seed,
                                const float* out, const float* lse, const float* dout, float* dqkv, float* delta_ws, void* stream) {
  int rc = check_enc(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(qkv && mask && out && lse && dout && dqkv && delta_ws, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  const EncDims e = enc_dims(s);
  RD_REQUIRE(!attn_big(e), "rd_attention_bwd: head_dim %d > 96 runs as materialised products inside the layer only", e.Hd);
  AttnArgs a = attn_args(e, qkv, mask, const_cast<float*>(out), const_cast<float*>(lse), p_drop, seed, (uint32_t)layer, token_plan());
  a.dout = dout; a.dqkv = dqkv; a.delta = delta_ws;
  return attn_backward(a, (hipStream_t)stream);
}

// not part of the ABI (include/raindrop_hip_debug.h): the route of one pass over this shape, from the pass's own functions
extern "C" int rd_debug_attention_route(const rd_shape* s, int32_t pass, int32_t with_plan, int32_t aligned, uint32_t* words, char* name,
                                        size_t cap) {
  int rc = check_enc(s);
  if (rc) return rc;
  RD_REQUIRE(words && name && cap > 0, "NULL tensor");
  RD_REQUIRE(pass == ATTN_FWD || pass == ATTN_BWD, "pass: 0 forward, 1 backward");
  const EncDims e = enc_dims(s);
  const AttnRoute r = attn_route((AttnPass)pass, e.T, e.B, e.D, e.H, e.Hd, with_plan != 0, aligned != 0);
  words[0] = (uint32_t)r.family | (uint32_t)r.vec << 2 | (uint32_t)r.one_product << 3 | (uint32_t)r.wide << 4 | (uint32_t)r.nth << 8 |
             (uint32_t)r.nlaunch << 12;
  for (int i = 0; i < 2; ++i) {
    const AttnLaunch l = i < r.nlaunch ? r.l[i] : AttnLaunch{0, dim3(0, 0), 0, 0, 0, ""};
    const uint32_t w[5] = {l.grid.x, l.grid.y, (uint32_t)l.block, (uint32_t)l.lds_attr, (uint32_t)l.lds};
    std::copy(w, w + 5, words + 1 + 5 * i);
  }
  snprintf(name, cap, "%s%s%s", r.nlaunch > 0 ? r.l[0].name : "", r.nlaunch > 1 ? "," : "", r.nlaunch > 1 ? r.l[1].name : "");
  return attn_check(r, e.Hd, with_plan != 0);
}
