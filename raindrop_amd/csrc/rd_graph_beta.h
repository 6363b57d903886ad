// rd_graph_beta.h -- argument block shared by the two forms of the use_beta graph operator (rd_graph_beta.hip: one workgroup per
// sample graph, graph staged in LDS; rd_graph_beta_large.hip: any graph size, state in a caller-provided workspace).
#pragma once
#include "rd_common.h"
#include "rd_rng.h"

namespace rd {

struct BetaArgs {
  const float *V, *H;                    // [B,N,K] relu(lin_value(x)),  [B,N,T*32] increase_dim(x)
  const float *map_w, *p_t;              // [N,16], [B or 1][T,16]
  const int64_t* ei; int64_t ei_stride;  // edge_index rows (source; target), shared by the batch
  const float* w; long w_bstride;        // [E] edge weights (per-sample stride, 0 = shared)
  long pt_bstride;
  float* out;                            // [B,N,K]
  int64_t* ei_out; float* alpha_out;     // [B][2,Kk] kept edges in pruning order, [B][Kk] mean kept score
  float* beta_save;                      // [B,N,T]
  int32_t* kept;                         // [B][Kk] original edge ids in pruning order (for backward)
  // backward
  const float* dout; float *dV, *dH, *dmap_part, *dw;   // dmap_part [B,N,16]; dw [B,E] or null
  const float* dalpha;                   // [B][Kk] cotangent of alpha_out (the structure distance's), or null: none
  int B, N, K, T, d, E, Kk;
  // coefficient dropout (code/Ob_propagation.py:195-196 on the use_beta branch); p_drop == 0: none, the fields below are unread
  float p_drop, inv_keep;                // p, 1 / (1 - p)
  uint64_t seed; const uint64_t* cell;   // by-value seed + the registered seed cell (rd_set_seed_cell) or null
};

// ---- coefficient dropout of the use_beta branch ------------------------------------------------------------------------------
// The reference repeats gamma to [E/2, T*d_ob] before the softmax and drops element-wise: the d_ob = 4 channels of one (edge, step)
// share the softmax weight and have four independent keep decisions.  ONE quad of the project's generator (rd_rng.h) per
// (sample b, edge e, step t), its four uniforms the four channels, keep iff u >= p:
//     quad = (b * E + e) * T + t,   e the edge's id in the INPUT list (not its position in the kept list), site SITE_EDGE_COEFF
// (< 2^48 at every supported size: B < 2^16, E <= 2^28 and N*T <= 2^31 bound it where T is large).  Both forms of the operator, both
// directions and rd_graph_beta_keep go through these functions, so they draw the same mask.
__device__ __forceinline__ uint64_t beta_drop_base(int b, int E, int e, int T) {          // + t = the quad
  return ((uint64_t)b * (uint64_t)E + (uint64_t)e) * (uint64_t)T;
}
// bit c set: channel c of the quad is kept
__device__ __forceinline__ unsigned beta_keep_code(uint64_t seed_eff, uint64_t quad, float p) {
  const float4 u = uniform4(seed_eff, SITE_EDGE_COEFF, quad);
  return (u.x >= p ? 1u : 0u) | (u.y >= p ? 2u : 0u) | (u.z >= p ? 4u : 0u) | (u.w >= p ? 8u : 0u);
}
__device__ __forceinline__ float4 beta_keep_scale(unsigned code, float inv_keep) {        // 0 or 1 / (1 - p) per channel
  return make_float4((code & 1u) ? inv_keep : 0.f, (code & 2u) ? inv_keep : 0.f, (code & 4u) ? inv_keep : 0.f, (code & 8u) ? inv_keep : 0.f);
}
// d loss / d weight[e][t] under the mask = sum_c keep_c / (1 - p) * dout[src][4t + c] * V[tgt][4t + c], channels in order
__device__ __forceinline__ float beta_dwgt_drop(const float4 o, const float4 v, const float4 ks) {
  float s = 0.f;
  s += (ks.x * o.x) * v.x; s += (ks.y * o.y) * v.y; s += (ks.z * o.z) * v.z; s += (ks.w * o.w) * v.w;
  return s;
}

// edge endpoint -> node index that is always legal (raindrop_amd.ops.graph_beta validates the range and raises like the
// reference's index_select; the kernels must not read out of range whatever they are handed)
__device__ __forceinline__ int node_of(int64_t v, int N) { return v < 0 ? 0 : (v >= N ? N - 1 : (int)v); }

__device__ __forceinline__ unsigned sortable_desc(float x) {          // larger float -> smaller key
  unsigned u = __float_as_uint(x);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                     // ascending order-preserving map
  return ~u;
}

inline int beta_next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// rd_graph_beta_large.hip
size_t beta_large_ws_bytes(int B, int N, int T, int E);
int beta_large_fwd(const BetaArgs& a, void* ws, size_t ws_bytes, hipStream_t st);
int beta_large_bwd(const BetaArgs& a, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace rd
