// rd_encoder.h -- what the translation units of the temporal encoder share (internal; the C ABI is include/raindrop_hip.h): the
// launch interface of every kernel file that rd_temporal.hip's layer drives.
#pragma once
#include <math.h>

#include "rd_common.h"
#include "rd_rng.h"

namespace rd {
// row-block dense layer on pre-split weight planes (rd_rowgemm.hip)
bool rowgemm_ok(int N, int K, long lda, long ldc);
size_t rowgemm_plane_elems(int rows, int cols);
int launch_wsplit(int njobs, const float* const* W, const int* N, const int* K, const int* transpose, __bf16* const* hi,
                  __bf16* const* lo, void* ones, hipStream_t st);
// weight gradients from exported row tiles (rd_tile_wgrad.hip)
// s32 / S: this job's own chunk count (device / bound) when its row tiles live in another chunk space than the launch's; hd != 0: the
// A tiles' columns are in the fused attention's head-padded layout ((which, head) blocks of hdp columns, hd of them real)
struct TileWgradJob { const void *tA, *tB; float* part; float *dW, *db; int N, K; const int32_t* s32; int S; int hd, hdp, H, D; };
size_t tile_elems(long M, int cols);
size_t tile_wgrad_ones_elems();
size_t tile_wgrad_part_floats(int N, int K);
bool tile_wgrad_ok(int N, int K);
struct TileColsumJob { const float* x; int M, N, n1; float *out1, *out2; };
int launch_rows_to_tiles(long M, int n, const float* const* x, const long* ld, const int* cols, void* const* tiles, hipStream_t st);   // rd_tiles_export.hip
int launch_tile_wgrad(long M, int njobs, const TileWgradJob* jobs, const void* ones, int ncs, const TileColsumJob* cs,
                      hipStream_t st, const int32_t* s32);
void rowgemm_export_next(void* tiles);
void rowgemm_set_mlive(const int32_t* p);
// row-local chains of the layer as one launch per direction (rd_encfuse.hip)
bool attnfuse_ok(int T, int D, int H, int hd);
size_t attnfuse_wf_elems(int H);
size_t attnfuse_wb_elems(int H);
int attnfuse_split_specs(const float* in_proj_w, int D, int H, int hd, void* wf, void* wb, WsplitSpec* out);
int attnfuse_padded_cols(int H);
int attnfuse_nth();
int launch_attn_fused_fwd(const float* x, const void* wf, const float* bias, const int32_t* plan, int T, int B, int D, int H, int hd,
                          float p_drop, uint64_t seed, uint32_t site, float* out, float* lse, hipStream_t st, bool save = true);
int launch_attn_fused_bwd(const float* x, const void* wf, const void* wb, const float* bias, const int32_t* plan, int T, int B, int D, int H,
                          int hd, float p_drop, uint64_t seed, uint32_t site, const float* out, const float* lse, const float* dout,
                          const float* ds1, float* dx, void* xt, void* dt, hipStream_t st);
int encfuse_level(int D, int H);
int launch_enc_post_fwd(long M, int D, int H, const float* attn, const float* x, const void* Wo, const void* W1, const void* W2,
                        const float* bo, const float* b1, const float* b2, const float* g1, const float* be1, const float* g2,
                        const float* be2, float* s1, float* x1, float* st1, float* h, float* s2, float* y, float* st2,
                        void* xt_attn, void* xt_x1, void* xt_h, float p, uint64_t seed, uint32_t site_ao, uint32_t site_fh,
                        uint32_t site_fo, const int32_t* mlive, void* hgate, hipStream_t st, bool save = true);
int encfuse_part_rows(long M);
int launch_enc_pre_bwd(long M, int D, int H, const float* dy, const float* s2, const float* st2, const float* g2, const float* h,
                       const float* s1, const float* st1, const float* g1, const void* W2t, const void* W1t, const void* Wot,
                       float* ds2, float* ds1, float* da, float* part2, float* part1, void* xt_df, void* xt_du, void* xt_dout, float p,
                       uint64_t seed, uint32_t site_fo, uint32_t site_ao, const int32_t* mlive, const void* hgate, hipStream_t st);
bool rowgemm_lnb_ok(int N, int K);
int rowgemm_lnb_part_rows(long M);
int launch_rowgemm_lnb(long M, int N, int K, const float* dy, const float* s, const float* stats, const float* g, float* ds_out,
                       float* part, float p_drop, uint64_t seed, uint32_t site, const void* Wh, float* C, long ldc,
                       const float* posmask, long pm_ld, float cscale, hipStream_t st);
bool rowgemm_ln_ok(int N, int K);
int launch_rowgemm_ln(long M, int N, int K, const float* A, const void* Wh, const float* bias, const float* residual,
                      const float* ln_g, const float* ln_b, float* s_out, float* y, float* stats, float drop_p,
                      uint64_t drop_seed, uint32_t drop_site, hipStream_t st);
int launch_rowgemm(long M, int N, int K, const float* A, long lda, const void* Wh, const void* Wl, float* C, long ldc,
                   const float* bias, int relu, const float* posmask, long pm_ld, float cscale, const float* residual,
                   long res_ld, float drop_p, uint64_t drop_seed, uint32_t drop_site, hipStream_t st);

// ---- the layer's shape (rd_temporal.hip) ------------------------------------------------------------------------------------
struct EncDims { long M; int D, Hd, nhid, H, T, B; };
EncDims enc_dims(const rd_shape* s);
int check_enc(const rd_shape* s);

// ---- attention core (rd_attention.hip) ---------------------------------------------------------------------------------------
constexpr int TS = 64;          // sequence tile (queries and keys)
constexpr int ATTN_MAX_HD = 96; // widest head of the tiled kernels (six 16-column tiles); wider heads take the materialised scores
// the attention route's family is the materialised one: wide heads, or RD_ATTN_BIG=1 (read per call: saved / workspace sizes follow it)
bool attn_big(const EncDims& e);

struct AttnArgs {
  const float* qkv;      // [T,B,3D]
  const uint8_t* mask;   // [B,T], 1 = padded key
  float* out;            // fwd: attention output [T,B,D]; bwd: same tensor (read)
  float* lse;            // [B,H,T] log-sum-exp of the scaled, masked scores
  const float* dout;     // bwd: grad of out [T,B,D]
  float* dqkv;           // bwd: [T,B,3D]
  float* delta;          // bwd: [B,H,T] rowsum(dout * out)
  int T, B, D, H, hd;
  float scale, p_drop; uint64_t seed; uint32_t site; const uint64_t* seed_cell;
  unsigned long long* stamps;   // debug only (tools/attn_timing.py)
  const int32_t* plan;          // token plan (rd_plan.h) or null; read by k_attn_*_one_b16w and k_attn_*_b16, refused on every other route
};
// the forward's arguments of layer `layer`; a backward adds dout, dqkv and delta
inline AttnArgs attn_args(const EncDims& e, const float* qkv, const uint8_t* mask, float* out, float* lse, float p_drop, uint64_t seed,
                          uint32_t layer, const int32_t* plan) {
  AttnArgs a{};
  a.qkv = qkv; a.mask = mask; a.out = out; a.lse = lse;
  a.T = e.T; a.B = e.B; a.D = e.D; a.H = e.H; a.hd = e.Hd;
  a.scale = 1.0f / sqrtf((float)e.Hd); a.p_drop = p_drop; a.seed = seed; a.site = SITE_ATTN_PROB + layer; a.seed_cell = seed_cell();
  a.plan = plan;
  return a;
}
// one pass of the tiled kernels: the launches of its route (the backward over several key tiles: dq + delta, then dk / dv)
int attn_forward(const AttnArgs& a, hipStream_t st);
int attn_backward(const AttnArgs& a, hipStream_t st);
// materialised scores (attn_big).  P, PD: [B*H][T][T] each (saved); dS: [B*H][T][T] workspace
int attn_big_fwd(const AttnArgs& a, float* P, float* PD, hipStream_t st);
int attn_big_bwd(const AttnArgs& a, const float* P, const float* PD, float* dS, hipStream_t st);

// ---- residual add + dropout + LayerNorm (rd_layernorm.hip) -------------------------------------------------------------------
constexpr int LN_RPB = 16;    // rows per block of the backward (4 per wavefront): ~1000 blocks at 15k tokens keep every CU busy
int launch_add_ln_fwd(const float* x, const float* r, const float* g, const float* bta, float* s_out, float* y,
                      float* stats, int M, int D, float p_drop, uint64_t seed, uint32_t site, hipStream_t st);
int launch_ln_bwd(const float* dy, const float* s, const float* stats, const float* g, float* ds_out, float* dr_out,
                  float* part, int M, int D, float p_drop, uint64_t seed, uint32_t site, hipStream_t st);
}  // namespace rd
