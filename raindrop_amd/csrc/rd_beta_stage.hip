// rd_beta_stage.hip -- the sensor stage of Raindrop_v2(use_beta=True) as ONE C-ABI pair in the training step's layout
// (raindrop_amd/step_beta.py BetaTrainStep): what Raindrop_v2._sensor_stage_beta composes under autograd -- code/models_rd.py:313-346
// with the `use_beta` literal of :317 flipped -- enqueued by the library itself, every gradient written into a caller-given
// destination (the flat gradient buffer's views), z / dz in the padded [T,B,D] layout or in the token plan's live-row layout
// (rd_plan.h).
//
//   forward : rd_pe_mask | p_t | rd_obs_embed_fwd | V = relu(lin_value(X)) | H = increase_dim(X) (exact fp32: feeds the top-K) |
//             rd_graph_beta_fwd | y2 = relu(lin_value2(y1)) | k_beta_l2_tokens_fwd | (rd_structure_distance)
//   backward: k_beta_l2_tokens_bwd | dW2, db2, dy1 | (rd_structure_distance_bwd) | rd_graph_beta_bwd(_alpha) | d map_weights |
//             ReLU gate of V | dW1, db1, dWinc, dbinc | dX = dV W1 + dH Winc | rd_obs_embed_bwd
//
// The products, the graph operator, the observation embedding and the structure distance are the library's existing entry points,
// called in the order and with the arguments the autograd surface (raindrop_amd/ops.py) uses: same kernels, same bits.  New here:
//   k_beta_l2_tokens_fwd  replaces k_edge_softmax_list (batched) + k_rows_to_tokens and the ssum2 round trip through HBM: per sample
//                         the per-target softmax sum over that sample's kept edges is formed in LDS (one wave per target, the lane
//                         partition and reduction order of k_edge_softmax_list: bit-identical), layer 2's rows are multiplied by it
//                         and transposed [F, T cells] -> [T, F cells] through an LDS tile, 16-byte accesses along the contiguous
//                         axis on both sides; z rows follow the token plan when one is registered.
//   k_beta_l2_tokens_bwd  the reverse: dz rows (either layout) -> layer 2's row gradient, already multiplied by the coefficient and by
//                         the ReLU gate of the saved y2; steps a plan-layout dz has no row for are written as exact zeros.  In the
//                         stage it reads the [B,F] coefficient table the forward left in `saved` instead of repeating the softmax.
// No float atomics, every cross-workgroup sum in a fixed order (the reused entry points'), vector stores only.
#include "rd_common.h"
#include "rd_plan.h"

namespace rd {
namespace {

constexpr int BT_THR = 512;            // 8 waves: one wave per target node in the coefficient pass
constexpr int BT_STAGE_EDGES = 4096;   // kept edges (target id + score) staged in LDS up to this many: 32 KB

// the reductions of k_edge_softmax_list (rd_graph.hip), verbatim: the coefficient must come out bit-identical
__device__ __forceinline__ float bt_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float bt_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct BtArgs {
  const float* Y;            // y2 [B,F,T*4] (fwd: source; bwd: ReLU gate)
  const int64_t* tgt;        // kept edges' targets of sample 0, `tgt_bstride` int64 apart per sample
  const float* alpha;        // [B,Kk] their scores
  float* z;                  // fwd: destination rows; bwd: dz rows (read only)
  float* dY;                 // bwd: [B,F,T*4]
  float* coef_out;           // fwd, optional: the coefficients [B,F] for the backward (written by the sample's first workgroup)
  const float* coef_in;      // optional: coefficients [B,F] a forward wrote -- read instead of repeating the softmax
  long tgt_bstride, ldz;
  int B, T, F, Kk, TT, nchunk, stage;
  const int32_t *brow, *blen;   // token plan (rd_plan.h brow / blen) or null: padded layout, row = t * B + b
};

__host__ __device__ inline int bt_f4(int F) { return (F + 3) & ~3; }
inline size_t bt_lds_bytes(int F, int TT, int Kk, bool stage) {
  return (size_t)bt_f4(F) * 4 + (size_t)TT * (F + 1) * 16 + (stage ? (size_t)Kk * 8 : 0);
}
inline int bt_tile_steps(int F) { int tt = 3072 / (F + 1); return tt < 1 ? 1 : (tt > 16 ? 16 : tt); }

// coef[n] = sum over the sample's kept edges into n of softmax_n(alpha)  (rd_edge_softmax_list_batched(norm_row = 1)'s ssum row):
// one wave per target, lanes stride over the list, three passes (max, denominator, sum of the quotients)
template <bool STAGE>
__device__ __forceinline__ void bt_coef(const int64_t* __restrict__ tgt, const float* __restrict__ w, int Kk, int F, float* coef,
                                        const int* s_t, const float* s_w) {
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int n = threadIdx.x >> 6; n < F; n += nw) {
    float m = -INFINITY;
    for (int e = lane; e < Kk; e += 64)
      if ((STAGE ? s_t[e] : (int)tgt[e]) == n) m = fmaxf(m, STAGE ? s_w[e] : w[e]);
    m = bt_wave_max(m);
    float den = 0.f;
    for (int e = lane; e < Kk; e += 64)
      if ((STAGE ? s_t[e] : (int)tgt[e]) == n) den += expf((STAGE ? s_w[e] : w[e]) - m);
    den = bt_wave_sum(den) + 1e-16f;
    float tot = 0.f;
    for (int e = lane; e < Kk; e += 64)
      if ((STAGE ? s_t[e] : (int)tgt[e]) == n) tot += expf((STAGE ? s_w[e] : w[e]) - m) / den;
    tot = bt_wave_sum(tot);
    if (lane == 0) coef[n] = tot;
  }
}

// grid (B, nchunk): workgroup (b, c) owns the steps [c * per, (c + 1) * per) of sample b, per = ceil(T / nchunk) rounded to tiles
template <bool BWD>
__device__ __forceinline__ void bt_body(const BtArgs& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char bt_smem[];
  float* coef = reinterpret_cast<float*>(bt_smem);
  float4* tile = reinterpret_cast<float4*>(bt_smem + (size_t)bt_f4(a.F) * 4);
  int* s_t = reinterpret_cast<int*>(bt_smem + (size_t)bt_f4(a.F) * 4 + (size_t)a.TT * (a.F + 1) * 16);
  float* s_w = reinterpret_cast<float*>(s_t + a.Kk);
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int T = a.T, F = a.F, TT = a.TT, ldt = F + 1;
  const int64_t* tgt = a.tgt + (long)b * a.tgt_bstride;
  const float* w = a.alpha + (long)b * a.Kk;
  if (a.coef_in) {                                      // uniform: the forward's table (the same bits: it is what the forward multiplied by)
    for (int n = tid; n < F; n += nthr) coef[n] = a.coef_in[(long)b * F + n];
  } else if (a.stage) {
    for (int e = tid; e < a.Kk; e += nthr) { s_t[e] = (int)tgt[e]; s_w[e] = w[e]; }
    __syncthreads();
    bt_coef<true>(tgt, w, a.Kk, F, coef, s_t, s_w);
  } else {
    bt_coef<false>(tgt, w, a.Kk, F, coef, s_t, s_w);
  }
  __syncthreads();
  if (a.coef_out && blockIdx.y == 0)
    for (int n = tid; n < F; n += nthr) a.coef_out[(long)b * F + n] = coef[n];
  const int per = ((T + a.nchunk - 1) / a.nchunk + TT - 1) / TT * TT;
  const int t_begin = blockIdx.y * per;
  int t_end = t_begin + per; if (t_end > T) t_end = T;
  int live_end = t_end, row0 = 0;
  if (a.brow) {                                         // token plan: sample b's step t is row brow[b] + t, t < blen[b]
    row0 = a.brow[b];
    const int len = a.blen[b];
    if (live_end > len) live_end = len;
  }
  const float4* Y4 = reinterpret_cast<const float4*>(a.Y) + (long)b * F * T;
  for (int t0 = t_begin; t0 < t_end; t0 += TT) {
    if (!BWD) {
      if (t0 >= live_end) break;                        // uniform: nothing of this chunk is stored any more
      for (int i = tid; i < F * TT; i += nthr) {        // source order: 16-byte cells along t
        const int f = i / TT, tt = i - f * TT, t = t0 + tt;
        if (t < live_end) {
          float4 v = Y4[(long)f * T + t];
          const float r = coef[f];
          v.x = v.x * r; v.y = v.y * r; v.z = v.z * r; v.w = v.w * r;
          tile[tt * ldt + f] = v;
        }
      }
      __syncthreads();
      for (int i = tid; i < TT * F; i += nthr) {        // destination order: 16-byte cells along f
        const int tt = i / F, f = i - tt * F, t = t0 + tt;
        if (t < live_end) {
          const long row = a.brow ? (long)row0 + t : (long)t * a.B + b;
          *reinterpret_cast<float4*>(a.z + row * a.ldz + 4 * f) = tile[tt * ldt + f];
        }
      }
      __syncthreads();
    } else {
      for (int i = tid; i < TT * F; i += nthr) {        // dz rows: cells along f
        const int tt = i / F, f = i - tt * F, t = t0 + tt;
        if (t < live_end) {
          const long row = a.brow ? (long)row0 + t : (long)t * a.B + b;
          tile[tt * ldt + f] = *reinterpret_cast<const float4*>(a.z + row * a.ldz + 4 * f);
        }
      }
      __syncthreads();
      float4* dY4 = reinterpret_cast<float4*>(a.dY) + (long)b * F * T;
      for (int i = tid; i < F * TT; i += nthr) {        // row gradient: cells along t
        const int f = i / TT, tt = i - f * TT, t = t0 + tt;
        if (t >= t_end) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);     // a step without a row in the plan layout: exact zeros
        if (t < live_end) {
          const float4 g = tile[tt * ldt + f];
          const float4 y = Y4[(long)f * T + t];
          const float r = coef[f];
          o.x = (g.x * r) * (y.x > 0.f ? 1.f : 0.f); o.y = (g.y * r) * (y.y > 0.f ? 1.f : 0.f);
          o.z = (g.z * r) * (y.z > 0.f ? 1.f : 0.f); o.w = (g.w * r) * (y.w > 0.f ? 1.f : 0.f);
        }
        dY4[(long)f * T + t] = o;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(BT_THR) void k_beta_l2_tokens_fwd(const BtArgs a) { bt_body<false>(a); }
__global__ __launch_bounds__(BT_THR) void k_beta_l2_tokens_bwd(const BtArgs a) { bt_body<true>(a); }

// p_t [B,T,16] = the positional encoding of every (sample, step), padded steps included (the graph operator scores every step):
// the expression of k_pe_mask (rd_graph.hip), so these are the bits of z's PE columns.  Also the ones column of the d map_weights sum.
// ONES = false (the inference forward): `ones`, the backward's reduction operand, is not written
template <bool ONES = true>
__global__ __launch_bounds__(256) void k_beta_pt(const float* __restrict__ times, const float* __restrict__ ts, float* __restrict__ p_t,
                                                 float* __restrict__ ones, int T, int B, int H) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if constexpr (ONES) {
    if (i < B) ones[i] = 1.f;
  }
  if (i >= (long)T * B) return;
  const int t = (int)(i / B), b = (int)(i - (long)t * B);
  const float tm = times[i];
  float* row = p_t + ((long)b * T + t) * (2 * H);
  for (int k = 0; k < H; ++k) {
    const float a = tm / ts[k];
    float sn, cs;
    sincosf(a, &sn, &cs);
    row[k] = sn;
    row[H + k] = cs;
  }
}

// out [C,R] = in [R,C]^T (alpha [B,Kk] <-> the [Kk,B] layout of the structure distance); small: thread per element
__global__ __launch_bounds__(256) void k_beta_transpose(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)R * C) return;
  const int c = (int)(i / R), r = (int)(i - (long)c * R);
  out[i] = in[(long)r * C + c];
}

// dv *= (v > 0): the ReLU gate of layer 1's lin_value on the graph operator's dV;  a += b: the two input gradients of X
__global__ __launch_bounds__(256) void k_beta_gate(float* __restrict__ dv, const float* __restrict__ v, long n4) {
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
    float4 g = reinterpret_cast<float4*>(dv)[q];
    const float4 y = reinterpret_cast<const float4*>(v)[q];
    g.x = g.x * (y.x > 0.f ? 1.f : 0.f); g.y = g.y * (y.y > 0.f ? 1.f : 0.f);
    g.z = g.z * (y.z > 0.f ? 1.f : 0.f); g.w = g.w * (y.w > 0.f ? 1.f : 0.f);
    reinterpret_cast<float4*>(dv)[q] = g;
  }
}
__global__ __launch_bounds__(256) void k_beta_add(float* __restrict__ a, const float* __restrict__ b, long n4) {
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
    float4 x = reinterpret_cast<float4*>(a)[q];
    const float4 y = reinterpret_cast<const float4*>(b)[q];
    x.x += y.x; x.y += y.y; x.z += y.z; x.w += y.w;
    reinterpret_cast<float4*>(a)[q] = x;
  }
}

inline unsigned ew_blocks(long n4) { long b = (n4 + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b)); }

int check_stage_shape(const rd_shape* s, int E) {
  RD_REQUIRE(s != nullptr, "rd_shape is NULL");
  RD_REQUIRE(s->B >= 0 && s->T > 0 && s->F > 0 && s->F <= 1024, "bad rd_shape (B=%d T=%d F=%d)", s->B, s->T, s->F);
  RD_REQUIRE(s->d_ob == 4 && s->d_pe == 16, "the use_beta stage needs d_ob = 4 and d_pe = 16 (got %d, %d)", s->d_ob, s->d_pe);
  RD_REQUIRE(E >= 0, "bad edge count %d", E);
  RD_REQUIRE((long)s->B * s->F * s->T * 32 < (1L << 31), "B*F*T*32 exceeds 2^31");
  return RD_OK;
}

int launch_l2_tokens(const rd_shape* s, int Kk, const int64_t* ei2, const float* alpha, const float* y2, float* z, long ldz,
                     float* dY, float* coef_out, const float* coef_in, hipStream_t st) {
  const int B = s->B, T = s->T, F = s->F;
  RD_REQUIRE(Kk >= 0, "bad kept-edge count %d", Kk);
  RD_REQUIRE(((ei2 && alpha) || Kk == 0 || coef_in) && y2 && z, "NULL tensor");       // an empty list (E < 2) has no data to point at
  RD_REQUIRE(ldz >= 4 * F && (ldz & 3) == 0, "row stride %ld must be a multiple of 4 and >= F*d_ob", ldz);
  RD_REQUIRE(((reinterpret_cast<uintptr_t>(y2) | reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(dY)) & 15) == 0,
             "tensors must be 16-byte aligned");
  const int32_t* tp = token_plan();
  BtArgs a{};
  a.Y = y2; a.tgt = ei2 ? ei2 + Kk : nullptr; a.tgt_bstride = 2L * Kk; a.alpha = alpha; a.z = z; a.dY = dY; a.ldz = ldz;
  a.coef_out = coef_out; a.coef_in = coef_in;
  a.B = B; a.T = T; a.F = F; a.Kk = Kk; a.TT = bt_tile_steps(F);
  a.stage = Kk <= BT_STAGE_EDGES ? 1 : 0;
  int nchunk = (512 + B - 1) / B;                                   // a few hundred workgroups (without a table every one forms its sample's coefficients)
  const int ntile = (T + a.TT - 1) / a.TT;
  a.nchunk = nchunk < 1 ? 1 : (nchunk > ntile ? ntile : nchunk);
  a.brow = tp ? tp + plan::brow_base(B, T) : nullptr;
  a.blen = tp ? tp + plan::blen_base(B, T) : nullptr;
  const size_t lds = bt_lds_bytes(F, a.TT, Kk, a.stage != 0);       // <= 4 + 48 + 32 KB
  if (dY) {
    RD_LDS_ATTR(k_beta_l2_tokens_bwd, 96 * 1024);
    hipLaunchKernelGGL(k_beta_l2_tokens_bwd, dim3(B, a.nchunk), dim3(BT_THR), lds, st, a);
    return check_launch("k_beta_l2_tokens_bwd");
  }
  RD_LDS_ATTR(k_beta_l2_tokens_fwd, 96 * 1024);
  hipLaunchKernelGGL(k_beta_l2_tokens_fwd, dim3(B, a.nchunk), dim3(BT_THR), lds, st, a);
  return check_launch("k_beta_l2_tokens_fwd");
}

// ---- caller-owned memory of the pair -------------------------------------------------------------------------------------------
struct StageSaved {          // forward -> backward
  float *X, *V, *H, *y1, *y2, *beta, *p_t, *coef, *ones;
  int32_t* kept;
  size_t bytes;
};
struct StageWs {             // scratch of one call
  float *a, *b, *c, *h, *dmap_part, *wg, *alpha_t, *dalpha_t, *dalpha, *dist_rows;
  void *obs, *sd, *gb;
  size_t wg_bytes, obs_bytes, sd_bytes, gb_bytes, bytes;
};

struct Carver {
  char* base; size_t off;
  template <class P> P* take(size_t nbytes) { P* p = base ? reinterpret_cast<P*>(base + off) : nullptr; off += align_up(nbytes > 0 ? nbytes : 1, 256); return p; }
};

// infer: the buffer of the inference forward (rd_beta_stage_infer_bytes) holds the graph operator's small per-sample tensors only
// (beta, p_t, kept); X, V, H, y1, y2 live in the workspace's backward scratch (carve_infer_scratch), coef and ones do not exist
StageSaved carve_saved(const rd_shape* s, int E, void* base, bool infer = false) {
  const size_t B = s->B, F = s->F, T = s->T, M = B * F, K = T * 4, Kk = (size_t)rd_graph_beta_kept(E);
  Carver c{static_cast<char*>(base), 0};
  StageSaved v;
  if (infer) {
    v = StageSaved{};
    v.beta = c.take<float>(M * T * 4); v.p_t = c.take<float>(B * T * 16 * 4); v.kept = c.take<int32_t>(B * (Kk > 0 ? Kk : 1) * 4);
    v.bytes = c.off;
    return v;
  }
  v.X = c.take<float>(M * K * 4); v.V = c.take<float>(M * K * 4); v.H = c.take<float>(M * T * 32 * 4);
  v.y1 = c.take<float>(M * K * 4); v.y2 = c.take<float>(M * K * 4); v.beta = c.take<float>(M * T * 4);
  v.p_t = c.take<float>(B * T * 16 * 4); v.coef = c.take<float>(B * F * 4); v.ones = c.take<float>(B * 4);
  v.kept = c.take<int32_t>(B * (Kk > 0 ? Kk : 1) * 4);
  v.bytes = c.off;
  return v;
}

StageWs carve_ws(const rd_shape* s, int E, void* base) {
  const size_t B = s->B, F = s->F, T = s->T, M = B * F, K = T * 4, Kk = (size_t)rd_graph_beta_kept(E);
  Carver c{static_cast<char*>(base), 0};
  StageWs w;
  w.a = c.take<float>(M * K * 4); w.b = c.take<float>(M * K * 4); w.c = c.take<float>(M * K * 4); w.h = c.take<float>(M * T * 32 * 4);
  w.dmap_part = c.take<float>(M * 16 * 4);
  size_t wg = rd_linear_bwd_weight_workspace_bytes((int)M, (int)K, (int)K);
  const size_t wg2 = rd_linear_bwd_weight_workspace_bytes((int)M, (int)T * 32, (int)K);
  const size_t wg3 = rd_linear_bwd_weight_workspace_bytes((int)B, 1, (int)F * 16);
  wg = wg > wg2 ? wg : wg2; wg = wg > wg3 ? wg : wg3;
  w.wg_bytes = wg; w.wg = c.take<float>(wg);
  w.alpha_t = c.take<float>(Kk * B * 4); w.dalpha_t = c.take<float>(Kk * B * 4); w.dalpha = c.take<float>(Kk * B * 4); w.dist_rows = c.take<float>(B * 4);
  w.obs_bytes = rd_obs_embed_bwd_workspace_bytes(s); w.obs = c.take<char>(w.obs_bytes);
  w.sd_bytes = rd_structure_distance_bwd_workspace_bytes((int)Kk, (int)B); w.sd = c.take<char>(w.sd_bytes);
  w.gb_bytes = rd_graph_beta_workspace_bytes((int)B, (int)F, (int)K, (int)T, E); w.gb = c.take<char>(w.gb_bytes);
  w.bytes = c.off;
  return w;
}

}  // namespace
}  // namespace rd

using namespace rd;

extern "C" size_t rd_beta_stage_saved_bytes(const rd_shape* s, int32_t E) {
  if (check_stage_shape(s, E) || s->B == 0) return 256;
  return carve_saved(s, E, nullptr).bytes;
}
extern "C" size_t rd_beta_stage_workspace_bytes(const rd_shape* s, int32_t E) {
  if (check_stage_shape(s, E) || s->B == 0) return 256;
  return carve_ws(s, E, nullptr).bytes;
}

extern "C" int rd_beta_l2_tokens_fwd(const rd_shape* s, int32_t Kk, const int64_t* edge_index_kept, const float* alpha, const float* y2,
                                     float* z, int32_t ldz, float* coef_out, void* stream) {
  int rc = check_stage_shape(s, 0);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  return launch_l2_tokens(s, Kk, edge_index_kept, alpha, y2, z, ldz, nullptr, coef_out, nullptr, (hipStream_t)stream);
}
extern "C" int rd_beta_l2_tokens_bwd(const rd_shape* s, int32_t Kk, const int64_t* edge_index_kept, const float* alpha, const float* y2,
                                     const float* dz, int32_t lddz, const float* coef, float* dY, void* stream) {
  int rc = check_stage_shape(s, 0);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(dY != nullptr, "NULL gradient output");
  return launch_l2_tokens(s, Kk, edge_index_kept, alpha, y2, const_cast<float*>(dz), lddz, dY, nullptr, coef, (hipStream_t)stream);
}

static int beta_stage_fwd(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                          const float* timescales, const float* R_u, const float* W1, const float* b1, const float* Winc,
                          const float* binc, const float* map_weights, const float* W2, const float* b2,
                          const int64_t* edge_index, int64_t row_stride, const float* edge_weights, int32_t E, float p_drop,
                          float p_edge1, uint64_t seed, float* z, uint8_t* mask, int64_t* edge_index_out,
                          float* alpha_out, float* distance, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                          void* stream, bool infer = false) {
  int rc = check_stage_shape(s, E);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(src && times && lengths && timescales && R_u && W1 && b1 && Winc && binc && map_weights && W2 && b2 && edge_index &&
             edge_weights && z && mask && saved && workspace, "NULL tensor");
  RD_REQUIRE((edge_index_out && alpha_out) || rd_graph_beta_kept(E) == 0, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  RD_REQUIRE(p_edge1 >= 0.f && p_edge1 < 1.f, "edge dropout probability must be in [0,1)");
  StageSaved v = carve_saved(s, E, saved, infer);
  const StageWs w = carve_ws(s, E, workspace);
  RD_REQUIRE(saved_bytes >= v.bytes, "saved buffer too small: %zu < %zu", saved_bytes, v.bytes);
  RD_REQUIRE(workspace_bytes >= w.bytes, "workspace too small: %zu < %zu", workspace_bytes, w.bytes);
  // inference: the stage's large intermediates in the workspace's backward scratch (same sizes; no forward launch uses it), y2 over X,
  // which is dead once V and H are formed
  if (infer) { v.X = w.a; v.V = w.b; v.y1 = w.c; v.H = w.h; v.y2 = w.a; }
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, T = s->T, F = s->F, K = 4 * T, M = B * F, Kk = rd_graph_beta_kept(E), D = 4 * F + 16;
  if ((rc = rd_pe_mask(s, times, lengths, timescales, z, mask, stream))) return rc;          // PE columns (either layout) + mask
  if (infer) hipLaunchKernelGGL(k_beta_pt<false>, dim3((unsigned)(((long)T * B + 255) / 256)), dim3(256), 0, st, times, timescales, v.p_t, nullptr, T, B, 8);
  else hipLaunchKernelGGL(k_beta_pt<true>, dim3((unsigned)(((long)T * B + 255) / 256)), dim3(256), 0, st, times, timescales, v.p_t, v.ones, T, B, 8);
  if ((rc = check_launch("k_beta_pt"))) return rc;
  if ((rc = rd_obs_embed_fwd(s, src, R_u, p_drop, seed, v.X, stream))) return rc;
  if ((rc = rd_linear_fwd(M, K, K, v.X, K, W1, b1, v.V, K, 1, stream))) return rc;
  if ((rc = rd_linear_fwd_fp32(M, 32 * T, K, v.X, K, Winc, binc, v.H, 32 * T, 0, stream))) return rc;
  if (p_edge1 > 0.f) rc = rd_graph_beta_fwd_dropout(B, F, K, T, 4, E, v.V, v.H, map_weights, v.p_t, 16L * T, edge_index, row_stride,
                                                    edge_weights, 0, p_edge1, seed, v.y1, edge_index_out, alpha_out, v.beta, v.kept,
                                                    w.gb, w.gb_bytes, stream);
  else rc = rd_graph_beta_fwd(B, F, K, T, 4, E, v.V, v.H, map_weights, v.p_t, 16L * T, edge_index, row_stride, edge_weights, 0, v.y1,
                              edge_index_out, alpha_out, v.beta, v.kept, w.gb, w.gb_bytes, stream);
  if (rc) return rc;
  if ((rc = rd_linear_fwd(M, K, K, v.y1, K, W2, b2, v.y2, K, 1, stream))) return rc;
  if ((rc = launch_l2_tokens(s, Kk, edge_index_out, alpha_out, v.y2, z, D, nullptr, v.coef, nullptr, st))) return rc;     // + the coefficient table for the backward (inference: none)
  if (distance) {
    if (Kk > 0) {
      hipLaunchKernelGGL(k_beta_transpose, dim3((unsigned)(((long)B * Kk + 255) / 256)), dim3(256), 0, st, alpha_out, w.alpha_t, B, Kk);
      if ((rc = check_launch("k_beta_transpose"))) return rc;
    }
    if ((rc = rd_structure_distance(Kk, B, w.alpha_t, w.dist_rows, distance, stream))) return rc;
  }
  return RD_OK;
}

extern "C" int rd_beta_stage_fwd(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                 const float* timescales, const float* R_u, const float* W1, const float* b1, const float* Winc,
                                 const float* binc, const float* map_weights, const float* W2, const float* b2,
                                 const int64_t* edge_index, int64_t row_stride, const float* edge_weights, int32_t E, float p_drop,
                                 uint64_t seed, float* z, uint8_t* mask, int64_t* edge_index_out, float* alpha_out, float* distance,
                                 void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  return beta_stage_fwd(s, src, times, lengths, timescales, R_u, W1, b1, Winc, binc, map_weights, W2, b2, edge_index, row_stride,
                        edge_weights, E, p_drop, 0.f, seed, z, mask, edge_index_out, alpha_out, distance, saved, saved_bytes,
                        workspace, workspace_bytes, stream);
}
extern "C" int rd_beta_stage_fwd_dropout(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                         const float* timescales, const float* R_u, const float* W1, const float* b1,
                                         const float* Winc, const float* binc, const float* map_weights, const float* W2,
                                         const float* b2, const int64_t* edge_index, int64_t row_stride, const float* edge_weights,
                                         int32_t E, float p_drop, float p_edge1, uint64_t seed, float* z, uint8_t* mask,
                                         int64_t* edge_index_out, float* alpha_out, float* distance, void* saved, size_t saved_bytes,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return beta_stage_fwd(s, src, times, lengths, timescales, R_u, W1, b1, Winc, binc, map_weights, W2, b2, edge_index, row_stride,
                        edge_weights, E, p_drop, p_edge1, seed, z, mask, edge_index_out, alpha_out, distance, saved,
                        saved_bytes, workspace, workspace_bytes, stream);
}

// ---- inference forward (include/raindrop_hip.h "inference forward"): same z, mask, kept edges, alpha and distance ------------------
extern "C" size_t rd_beta_stage_infer_bytes(const rd_shape* s, int32_t E) {
  if (check_stage_shape(s, E) || s->B == 0) return 256;
  return carve_saved(s, E, nullptr, true).bytes;
}
extern "C" int rd_beta_stage_fwd_infer(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                       const float* timescales, const float* R_u, const float* W1, const float* b1, const float* Winc,
                                       const float* binc, const float* map_weights, const float* W2, const float* b2,
                                       const int64_t* edge_index, int64_t row_stride, const float* edge_weights, int32_t E, float* z,
                                       uint8_t* mask, int64_t* edge_index_out, float* alpha_out, float* distance, void* saved,
                                       size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
  return beta_stage_fwd(s, src, times, lengths, timescales, R_u, W1, b1, Winc, binc, map_weights, W2, b2, edge_index, row_stride,
                        edge_weights, E, 0.f, 0.f, 0, z, mask, edge_index_out, alpha_out, distance, saved, saved_bytes, workspace,
                        workspace_bytes, stream, true);
}

static int beta_stage_bwd(const rd_shape* s, const float* src, const float* R_u, const float* W1, const float* Winc,
                          const float* map_weights, const float* W2, const int64_t* edge_index, int64_t row_stride,
                          const float* edge_weights, int32_t E, float p_drop, float p_edge1, uint64_t seed,
                          const int64_t* edge_index_kept, const float* alpha,
                          const void* saved, size_t saved_bytes, const float* dz, int32_t lddz, const float* dist_grad,
                          float* dR_u, float* dW1, float* db1, float* dWinc, float* dbinc, float* dmap_weights, float* dW2,
                          float* db2, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_stage_shape(s, E);
  if (rc) return rc;
  RD_REQUIRE(dR_u && dW1 && db1 && dWinc && dbinc && dmap_weights && dW2 && db2, "NULL gradient output");
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, T = s->T, F = s->F, K = 4 * T, M = B * F, Kk = rd_graph_beta_kept(E);
  if (B == 0) {
    RD_HIP(hipMemsetAsync(dW1, 0, sizeof(float) * K * K, st)); RD_HIP(hipMemsetAsync(dW2, 0, sizeof(float) * K * K, st));
    RD_HIP(hipMemsetAsync(db1, 0, sizeof(float) * K, st)); RD_HIP(hipMemsetAsync(db2, 0, sizeof(float) * K, st));
    RD_HIP(hipMemsetAsync(dWinc, 0, sizeof(float) * 32 * T * K, st)); RD_HIP(hipMemsetAsync(dbinc, 0, sizeof(float) * 32 * T, st));
    RD_HIP(hipMemsetAsync(dmap_weights, 0, sizeof(float) * F * 16, st)); RD_HIP(hipMemsetAsync(dR_u, 0, sizeof(float) * F * 4, st));
    return RD_OK;
  }
  RD_REQUIRE(src && R_u && W1 && Winc && map_weights && W2 && edge_index && edge_weights && saved && dz && workspace, "NULL tensor");
  RD_REQUIRE((edge_index_kept && alpha) || rd_graph_beta_kept(E) == 0, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  const StageSaved v = carve_saved(s, E, const_cast<void*>(saved));
  const StageWs w = carve_ws(s, E, workspace);
  RD_REQUIRE(saved_bytes >= v.bytes, "saved buffer too small: %zu < %zu", saved_bytes, v.bytes);
  RD_REQUIRE(workspace_bytes >= w.bytes, "workspace too small: %zu < %zu", workspace_bytes, w.bytes);
  const long n4 = (long)M * K / 4;
  // layer 2: dz rows -> gated, scaled row gradient (w.a); its weight gradients; dy1 (w.b)
  if ((rc = launch_l2_tokens(s, Kk, edge_index_kept, alpha, v.y2, const_cast<float*>(dz), lddz, w.a, nullptr, v.coef, st))) return rc;
  if ((rc = rd_linear_bwd_input(M, K, K, w.a, K, W2, w.b, K, stream))) return rc;
  if ((rc = rd_linear_bwd_weight(M, K, K, w.a, K, v.y1, K, dW2, db2, w.wg, w.wg_bytes, stream))) return rc;
  // graph operator (with the structure distance's cotangent of alpha when the loss carries lambda * distance)
  const float* dalpha = nullptr;
  if (dist_grad && Kk > 0) {
    // alpha^T is formed here from the caller's alpha, not carried over from the forward: the backward does not depend on
    // whether the forward was asked for the distance
    hipLaunchKernelGGL(k_beta_transpose, dim3((unsigned)(((long)B * Kk + 255) / 256)), dim3(256), 0, st, alpha, w.alpha_t, B, Kk);
    if ((rc = check_launch("k_beta_transpose"))) return rc;
    if ((rc = rd_structure_distance_bwd(Kk, B, w.alpha_t, dist_grad, w.sd, w.sd_bytes, w.dalpha_t, stream))) return rc;
    hipLaunchKernelGGL(k_beta_transpose, dim3((unsigned)(((long)B * Kk + 255) / 256)), dim3(256), 0, st, w.dalpha_t, w.dalpha, Kk, B);
    if ((rc = check_launch("k_beta_transpose"))) return rc;
    dalpha = w.dalpha;
  }
  if (p_edge1 > 0.f) rc = rd_graph_beta_bwd_dropout(B, F, K, T, 4, E, v.V, v.H, map_weights, v.p_t, 16L * T, edge_index, row_stride,
                                                    edge_weights, 0, p_edge1, seed, v.beta, v.kept, w.b, dalpha, w.c, w.h, w.dmap_part,
                                                    nullptr, w.gb, w.gb_bytes, stream);
  else if (dalpha) rc = rd_graph_beta_bwd_alpha(B, F, K, T, 4, E, v.V, v.H, map_weights, v.p_t, 16L * T, edge_index, row_stride, edge_weights, 0,
                                           v.beta, v.kept, w.b, dalpha, w.c, w.h, w.dmap_part, nullptr, w.gb, w.gb_bytes, stream);
  else rc = rd_graph_beta_bwd(B, F, K, T, 4, E, v.V, v.H, map_weights, v.p_t, 16L * T, edge_index, row_stride, edge_weights, 0, v.beta,
                              v.kept, w.b, w.c, w.h, w.dmap_part, nullptr, w.gb, w.gb_bytes, stream);
  if (rc) return rc;
  // d map_weights = sum over the samples of the per-sample parts: the library's fixed-order split reduction (ones^T parts)
  if ((rc = rd_linear_bwd_weight(B, 1, 16 * F, v.ones, 1, w.dmap_part, 16 * F, dmap_weights, nullptr, w.wg, w.wg_bytes, stream))) return rc;
  // layer 1: ReLU gate of V, the two weight-gradient products over X, dX = dV W1 + dH Winc, the observation embedding
  hipLaunchKernelGGL(k_beta_gate, dim3(ew_blocks(n4)), dim3(256), 0, st, w.c, v.V, n4);
  if ((rc = check_launch("k_beta_gate"))) return rc;
  if ((rc = rd_linear_bwd_weight(M, 32 * T, K, w.h, 32 * T, v.X, K, dWinc, dbinc, w.wg, w.wg_bytes, stream))) return rc;
  if ((rc = rd_linear_bwd_weight(M, K, K, w.c, K, v.X, K, dW1, db1, w.wg, w.wg_bytes, stream))) return rc;
  if ((rc = rd_linear_bwd_input(M, K, K, w.c, K, W1, w.a, K, stream))) return rc;
  if ((rc = rd_linear_bwd_input(M, 32 * T, K, w.h, 32 * T, Winc, w.b, K, stream))) return rc;
  hipLaunchKernelGGL(k_beta_add, dim3(ew_blocks(n4)), dim3(256), 0, st, w.a, w.b, n4);
  if ((rc = check_launch("k_beta_add"))) return rc;
  return rd_obs_embed_bwd(s, src, v.X, w.a, p_drop, dR_u, w.obs, w.obs_bytes, stream);
}

extern "C" int rd_beta_stage_bwd(const rd_shape* s, const float* src, const float* R_u, const float* W1, const float* Winc,
                                 const float* map_weights, const float* W2, const int64_t* edge_index, int64_t row_stride,
                                 const float* edge_weights, int32_t E, float p_drop, const int64_t* edge_index_kept, const float* alpha,
                                 const void* saved, size_t saved_bytes, const float* dz, int32_t lddz, const float* dist_grad,
                                 float* dR_u, float* dW1, float* db1, float* dWinc, float* dbinc, float* dmap_weights, float* dW2,
                                 float* db2, void* workspace, size_t workspace_bytes, void* stream) {
  return beta_stage_bwd(s, src, R_u, W1, Winc, map_weights, W2, edge_index, row_stride, edge_weights, E, p_drop, 0.f, 0, edge_index_kept,
                        alpha, saved, saved_bytes, dz, lddz, dist_grad, dR_u, dW1, db1, dWinc, dbinc, dmap_weights, dW2, db2, workspace,
                        workspace_bytes, stream);
}
// the backward of rd_beta_stage_fwd_dropout: layer 1's mask is regenerated from (p_edge1, seed), the forward's
extern "C" int rd_beta_stage_bwd_dropout(const rd_shape* s, const float* src, const float* R_u, const float* W1, const float* Winc,
                                         const float* map_weights, const float* W2, const int64_t* edge_index, int64_t row_stride,
                                         const float* edge_weights, int32_t E, float p_drop, float p_edge1, uint64_t seed,
                                         const int64_t* edge_index_kept, const float* alpha, const void* saved, size_t saved_bytes,
                                         const float* dz, int32_t lddz, const float* dist_grad, float* dR_u, float* dW1, float* db1,
                                         float* dWinc, float* dbinc, float* dmap_weights, float* dW2, float* db2, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  RD_REQUIRE(p_edge1 >= 0.f && p_edge1 < 1.f, "edge dropout probability must be in [0,1)");
  return beta_stage_bwd(s, src, R_u, W1, Winc, map_weights, W2, edge_index, row_stride, edge_weights, E, p_drop, p_edge1, seed,
                        edge_index_kept, alpha, saved, saved_bytes, dz, lddz, dist_grad, dR_u, dW1, db1, dWinc, dbinc, dmap_weights, dW2,
                        db2, workspace, workspace_bytes, stream);
}
