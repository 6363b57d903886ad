// rd_temporal.hip -- temporal self-attention stage, host side (kernel families K2/K3/K5):
//   * rd_encoder_layer_{fwd,fwd_infer,bwd}: one post-norm nn.TransformerEncoderLayer as a chain of launches, the route through
//     the kernel forms decided ONCE per call (enc_route), and the weight preparation of a layer / a whole step,
//   * masked mean over time forward/backward.
// The layer's kernels: rd_attention.hip, rd_layernorm.hip, rd_rowgemm.hip, rd_attnfuse.hip, rd_encfuse.hip, rd_tile_wgrad.hip,
// rd_gemm.hip (declared in rd_encoder.h).  Replaces nn.TransformerEncoder (code/models_rd.py:235-237,358; torch semantics in
// torch/nn/modules/transformer.py:799-983 and F.multi_head_attention_forward): post-norm, ReLU FFN, key-padding mask -> -inf,
// q.k scaled by 1/sqrt(head_dim), LayerNorm eps 1e-5, dropout on attention probabilities / attention output / FFN hidden / FFN
// output; and the masked mean of code/models_rd.py:366-367,379.
#include <stdlib.h>
#include <algorithm>

#include "rd_encoder.h"
#include "rd_k1_route.h"
#include "rd_plan.h"

namespace rd {
EncDims enc_dims(const rd_shape* s) {
  EncDims e;
  e.T = s->T; e.B = s->B; e.D = s->F * s->d_ob + s->d_pe; e.H = s->nhead; e.Hd = e.D / e.H;
  e.nhid = s->nhid; e.M = (long)s->T * s->B;
  return e;
}

int check_enc(const rd_shape* s) {
  RD_REQUIRE(s != nullptr, "rd_shape is NULL");
  RD_REQUIRE(s->B >= 0 && s->T > 0 && s->F > 0 && s->d_ob > 0 && s->d_pe >= 0 && s->nhead > 0 && s->nhid > 0,
             "bad rd_shape");
  const int D = s->F * s->d_ob + s->d_pe;
  RD_REQUIRE(D % s->nhead == 0, "D=%d not divisible by nhead=%d", D, s->nhead);
  RD_REQUIRE((long)s->B * s->nhead * s->T * s->T < (1L << 31) || D / s->nhead <= ATTN_MAX_HD, "score tensor exceeds 2^31 elements");
  RD_REQUIRE((long)s->T * s->B * (3L * D > s->nhid ? 3L * D : s->nhid) < (1L << 31), "tensor exceeds 2^31 elements");
  return RD_OK;
}

namespace {

// code/models_rd.py:366-367,379: agg[b,c] = sum_t r[t,b,c] * (1 - mask[b,t]) / (lengths[b] + 1)
__global__ __launch_bounds__(1024) void k_masked_mean_fwd(const float* __restrict__ r, const uint8_t* __restrict__ mask,
                                                          const int64_t* __restrict__ lengths, float* __restrict__ out,
                                                          int T, int B, int D, int ldo, const int32_t* __restrict__ tp) {
  // block = (sample, 64-column chunk); 16 time groups x 64 columns, fixed-order LDS combine
  // tp (token plan, rd_plan.h) or null: r holds the live rows only, sample b's step t at row brow[b] + t -- the same steps enter the
  // same partial sums in the same order as on the padded layout (mask[b,t] is set exactly for the steps that have no row)
  __shared__ float red[16][64];
  const int b = blockIdx.x, cl = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  const long row0 = tp ? (long)tp[plan::brow_base(B, T) + b] : (long)b, rstep = tp ? 1 : (long)B;
  const int Tv = tp ? tp[plan::blen_base(B, T) + b] : T;
  float s = 0.f;
  if (c < D)
    for (int t = tg; t < Tv; t += 16)
      if (!mask[(long)b * T + t]) s += r[(row0 + (long)t * rstep) * D + c];
  red[tg][cl] = s;
  __syncthreads();
  if (tg == 0 && c < D) {
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) v += red[q][cl];
    out[(long)b * ldo + c] = v / (float)(lengths[b] + 1);
  }
}

__global__ __launch_bounds__(256) void k_masked_mean_bwd(const float* __restrict__ dagg, const uint8_t* __restrict__ mask,
                                                         const int64_t* __restrict__ lengths, float* __restrict__ dr,
                                                         int T, int B, int D, int ldo) {
  const long n = (long)T * B * D;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % D);
    const long tb = i / D;
    const int b = (int)(tb % B), t = (int)(tb / B);
    dr[i] = mask[(long)b * T + t] ? 0.f : dagg[(long)b * ldo + c] / (float)(lengths[b] + 1);
  }
}

// ---- the route of a layer call -----------------------------------------------------------------------------------------------
// Which kernel forms one encoder layer of this shape runs through, in the current arithmetic mode and switches.  Decided HERE and
// nowhere else: prepare, the carves, the `covers` queries and the three layer entry points all read these fields, so the tiles one
// of them writes are the tiles another reads.  (include/raindrop_hip_debug.h rd_debug_encoder_route: the bit of each field.)
// A forward (prepare, the queries) does not evaluate the fields marked [bwd], a backward not those marked [fwd]: no environment read the caller cannot use
enum RouteUse { ROUTE_RG, ROUTE_FWD, ROUTE_BWD, ROUTE_ALL };      // ROUTE_RG: `rg` alone (rd_step_prepare_covers)
struct EncRoute {
  bool rg;           // all four forward products run on the row-block kernels (rd_rowgemm.hip); else the tiled family (rd_gemm.hip)
  bool dx_rowblock;  // rg and the in_proj input-gradient product (reduction 3D) too: 8 weight orientations are split, else 7
  bool tw;           // dx_rowblock and ONE streaming launch (rd_tile_wgrad.hip) over row tiles the products export ends the backward
  bool panel;        // tiled family on its panel form (bf16 modes): the forward splits the eight weight orientations into `saved`
  bool tw2;          // [bwd] panel, and the same stream fed by ONE conversion pass over the eight operands (rd_tiles_export.hip), not four split-K
                     // GEMMs (SYN256: 11.2 -> 7.65 ms; narrow layers keep the GEMMs, PAM: 2.96 vs 3.04 ms).  RD_TILE_WGRAD_GENERIC=0: GEMMs
  bool big;          // attention with materialised scores (attn_big: the attention route's family)
  bool lnf1, lnf2;   // out_proj / linear2 carry the residual add + LayerNorm in their epilogue (a workgroup owns complete rows)
  bool lnb;          // the LayerNorm backward is the PROLOGUE of the input-gradient product that consumes its output
  bool chain_fwd;    // [fwd] out_proj + LayerNorm1 + linear1 + linear2 + LayerNorm2 as ONE launch (rd_encfuse.hip): the rows stay in LDS
  bool chain_bwd;    // [bwd] the whole row-local chain (LayerNorm2' .. out_proj') as ONE launch
  bool attn_tiles;   // fused attention's envelope (rd_attnfuse.hip): prepare, which sees no token plan, splits its per-head in_proj tiles
  bool afuse_fwd;    // [fwd] in_proj + attention core as ONE launch: a workgroup owns a sample, qkv never reaches memory
  bool afuse_bwd;    // [bwd] attention backward + dx = dqkv W_in + ds1 + the row tiles of x and dqkv, one launch.  It also needs lnb (through
                     // chain_bwd), afuse_fwd does not: the two coincide wherever plan_ok holds, which every token-plan call requires
  bool lean;         // LEAN chains: token plan + tile stream (the training step, both directions known to take the fused chains): no fp32
                     // FFN hidden and x1 are written, the gate bytes live at the start of the unused h buffer.  RD_ENC_LEAN=0: A/B
  bool infer;        // [fwd] the layer has an inference forward: row-block + tile-stream path, LayerNorm epilogues, save-free chain (P19 widths)
  bool plan_ok;      // a token plan can run: what the three "token plan: ..." checks of forward and backward require together
};

EncRoute enc_route(const EncDims& e, bool with_plan, RouteUse use) {
  const bool fwd = use != ROUTE_BWD, bwd = use != ROUTE_FWD;
  // read once per process
  static const bool ln_fuse_env = [] { const char* v = getenv("RD_LN_FUSE"); return !(v && atoi(v) == 0); }();
  static const bool lnb_env = [] { const char* v = getenv("RD_LNB_FUSE"); return !(v && atoi(v) == 0); }();
  // read per call (tests compare both paths in one process), and only where the answer can matter
  auto off = [](const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; };
  auto wgrad4 = [&] { return tile_wgrad_ok(3 * e.D, e.D) && tile_wgrad_ok(e.D, e.D) && tile_wgrad_ok(e.nhid, e.D) && tile_wgrad_ok(e.D, e.nhid); };
  EncRoute r{};
  r.rg = rowgemm_ok(3 * e.D, e.D, e.D, 3 * e.D) && rowgemm_ok(e.D, e.D, e.D, e.D) && rowgemm_ok(e.nhid, e.D, e.D, e.nhid) &&
         rowgemm_ok(e.D, e.nhid, e.nhid, e.D);
  if (use == ROUTE_RG) return r;
  r.dx_rowblock = r.rg && rowgemm_ok(e.D, 3 * e.D, 3 * e.D, e.D);
  r.tw = r.dx_rowblock && wgrad4();
  r.panel = !r.rg && precision() != RD_PREC_FP32;
  r.tw2 = bwd && r.panel && e.M >= 1024 && e.D >= 256 && !off("RD_TILE_WGRAD_GENERIC") && wgrad4();
  r.big = attn_big(e);
  r.lnf1 = r.rg && ln_fuse_env && rowgemm_ln_ok(e.D, e.D);
  r.lnf2 = r.rg && ln_fuse_env && rowgemm_ln_ok(e.D, e.nhid);
  r.lnb = r.tw && lnb_env && rowgemm_lnb_ok(e.nhid, e.D) && rowgemm_lnb_ok(e.D, e.D);
  // >= 1: the fused chains exist at these widths, 2: the inference chain too; asked only where a field below can come out true
  const int ef = (fwd && r.lnf1 && r.lnf2) || (bwd && r.lnb) || (with_plan && r.tw) ? encfuse_level(e.D, e.nhid) : 0;
  r.chain_fwd = fwd && r.lnf1 && r.lnf2 && ef >= 1;
  r.chain_bwd = bwd && r.lnb && ef >= 1;
  r.attn_tiles = r.rg && attnfuse_ok(e.T, e.D, e.H, e.Hd);
  r.afuse_fwd = fwd && with_plan && r.tw && ef >= 1 && r.attn_tiles;
  r.afuse_bwd = with_plan && r.tw && r.chain_bwd && r.attn_tiles;
  r.lean = with_plan && r.tw && !off("RD_ENC_LEAN");
  r.infer = fwd && r.tw && r.lnf1 && r.lnf2 && !r.big && e.H <= 2 && ef == 2;
  r.plan_ok = r.tw && !r.big && r.lnf1 && r.lnf2 && r.lnb;
  return r;
}

// chunks of the per-sample group space (rd_plan.h: coff): every sample up to ceil(T / 16) groups of 16 rows, two groups per chunk
size_t attn_chunks(const EncDims& e) { return ((size_t)e.B * cdiv(e.T, 16) + 1) / 2; }

struct EncSaved { float *qkv, *attn, *lse, *s1, *st1, *x1, *h, *s2, *st2; __bf16* pl[8][2];
                  __bf16* xt[4]; __bf16* ones;        // row tiles of x, attn, x1, h (operands of the weight-gradient stream)
                  __bf16 *afw, *abw;                  // fused attention (rd_attnfuse.hip): per-head in_proj tiles, forward / input-gradient form
                  float *pbig, *pdbig;                // wide heads only: P and dropout(P), [B*H][T][T] each
                  size_t bytes; bool infer; };        // infer: this is the inference carve
// weight tiles kept from forward to backward: 0 in_proj, 1 out_proj, 2 lin1, 3 lin2, 4 out_proj^T, 5 lin2^T, 6 lin1^T, 7 in_proj^T
// infer: the buffer of the inference forward (rd_encoder_layer_infer_bytes) -- the four forward weight orientations, the fused
// attention's forward tiles and what one forward launch hands to the next (attn; qkv and lse on the layouts whose attention is not
// fused); everything else is null
EncSaved carve_saved(const EncDims& e, void* base, bool big, bool infer = false) {
  EncSaved v{}; size_t off = 0;
  auto take = [&](size_t n) { float* p = base ? (float*)((char*)base + off) : nullptr;
                              off += align_up(n * sizeof(float), 256); return p; };
  v.infer = infer;
  if (infer) {
    const int prow[4] = {3 * e.D, e.D, e.nhid, e.D}, pcol[4] = {e.D, e.D, e.D, e.nhid};
    for (int i = 0; i < 4; ++i)
      for (int h = 0; h < 2; ++h) v.pl[i][h] = (__bf16*)take((rowgemm_plane_elems(prow[i], pcol[i]) + 1) / 2);
    v.afw = (__bf16*)take((attnfuse_wf_elems(e.H) + 1) / 2);
    v.attn = take(e.M * e.D); v.qkv = take(e.M * 3 * e.D); v.lse = take((size_t)e.B * e.H * e.T);
    v.bytes = off;
    return v;
  }
  v.qkv = take(e.M * 3 * e.D); v.attn = take(e.M * e.D); v.lse = take((size_t)e.B * e.H * e.T);
  v.s1 = take(e.M * e.D); v.st1 = take(e.M * 2); v.x1 = take(e.M * e.D);
  v.h = take(e.M * e.nhid); v.s2 = take(e.M * e.D); v.st2 = take(e.M * 2);
  const int prow[8] = {3 * e.D, e.D, e.nhid, e.D, e.D, e.nhid, e.D, e.D};      // plane rows = output columns
  const int pcol[8] = {e.D, e.D, e.D, e.nhid, e.D, e.D, e.nhid, 3 * e.D};      // plane cols = reduction length
  for (int i = 0; i < 8; ++i)
    for (int h = 0; h < 2; ++h) v.pl[i][h] = (__bf16*)take((rowgemm_plane_elems(prow[i], pcol[i]) + 1) / 2);
  const int xcols[4] = {e.D, e.D, e.D, e.nhid};
  for (int i = 0; i < 4; ++i) {
    size_t n = tile_elems(e.M, xcols[i]);
    if (i == 0) n = std::max(n, attn_chunks(e) * (size_t)cdiv(e.D, 16) * 1024);     // x tiles in the per-sample chunk space (fused attention)
    v.xt[i] = (__bf16*)take((n + 1) / 2);
  }
  v.ones = (__bf16*)take((tile_wgrad_ones_elems() + 1) / 2);
  v.afw = (__bf16*)take((attnfuse_wf_elems(e.H) + 1) / 2);
  v.abw = (__bf16*)take((attnfuse_wb_elems(e.H) + 1) / 2);
  const size_t nbig = big ? (size_t)e.B * e.H * e.T * e.T : 0;
  v.pbig = take(nbig); v.pdbig = take(nbig);
  v.bytes = off;
  return v;
}
// The carve a buffer of `bytes` holds: the training carve when it is large enough for it, else the inference carve -- ONE rule for
// rd_encoder_layer_prepare / rd_step_prepare / rd_step_begin and rd_encoder_layer_fwd_infer, so the tile offsets cannot disagree.
EncSaved carve_for_bytes(const EncDims& e, const EncRoute& r, void* base, size_t bytes) {
  return carve_saved(e, base, r.big, r.infer && bytes < carve_saved(e, nullptr, r.big).bytes);
}

struct EncWs { float *o, *f, *ds2, *df, *du, *dx1, *ds1, *dout, *da, *dqkv, *delta, *lnpart, *lnpart1, *lnred, *splitk;
               float* dsbig;                      // wide heads only: dS [B*H][T][T]
               __bf16* dt[4]; float* twpart[4];   // row tiles of df, du, dout, dqkv; slice partials of lin2, lin1, out_proj, in_proj
               size_t bytes; };
EncWs carve_ws(const EncDims& e, void* base, bool big) {
  EncWs w; size_t off = 0;
  auto take = [&](size_t n) { float* p = base ? (float*)((char*)base + off) : nullptr;
                              off += align_up(n * sizeof(float), 256); return p; };
  w.o = take(e.M * e.D); w.f = take(e.M * e.D);
  w.ds2 = take(e.M * e.D); w.df = take(e.M * e.D); w.du = take(e.M * e.nhid); w.dx1 = take(e.M * e.D);
  w.ds1 = take(e.M * e.D); w.dout = take(e.M * e.D); w.da = take(e.M * e.D); w.dqkv = take(e.M * 3 * e.D);
  w.delta = take((size_t)e.B * e.H * e.T);
  w.lnpart = take((size_t)cdiv((int)e.M, LN_RPB) * 2 * e.D);
  w.lnpart1 = take((size_t)cdiv((int)e.M, LN_RPB) * 2 * e.D);
  w.lnred = take((size_t)2 * e.D + colsum_ws_floats(cdiv((int)e.M, LN_RPB), 2 * e.D));
  size_t sk = 0;
  const int shapes[4][2] = {{3 * e.D, e.D}, {e.D, e.D}, {e.nhid, e.D}, {e.D, e.nhid}};
  for (auto& sh : shapes) { size_t v = (size_t)wgrad_ws_floats(e.M, sh[0], sh[1]); if (v > sk) sk = v; }
  w.splitk = take(sk);
  take(colsum_ws_floats((int)e.M, 3 * e.D > e.nhid ? 3 * e.D : e.nhid));      // no launch uses it; it keeps its place in the layout
  const int dcols[4] = {e.D, e.nhid, e.D, 3 * e.D};
  const int padc = attnfuse_padded_cols(e.H);                       // head-padded dqkv columns of the fused attention's export
  for (int i = 0; i < 4; ++i) {
    size_t n = tile_elems(e.M, dcols[i]);
    if (i == 3) n = std::max(n, attn_chunks(e) * (size_t)(padc / 16) * 1024);
    w.dt[i] = (__bf16*)take((n + 1) / 2);
  }
  const int pn[4] = {e.D, e.nhid, e.D, std::max(3 * e.D, padc)}, pk[4] = {e.nhid, e.D, e.D, e.D};
  for (int i = 0; i < 4; ++i) w.twpart[i] = take(tile_wgrad_part_floats(pn[i], pk[i]));
  w.dsbig = take(big ? (size_t)e.B * e.H * e.T * e.T : 0);
  w.bytes = off;
  return w;
}

// the layer's dense products on the tiled family (rd_gemm.hip).  tiles: the weight also as native operand tiles (k_wsplit), or null:
// launch_gemm takes the panel form when it applies
int linear_fwd_t(long M, int N, int K, const float* x, const float* W, const void* tiles, const float* b, float* y, int relu,
                 float p, uint64_t seed, uint32_t site, hipStream_t st) {
  GemmArgs g{};
  g.M = (int)M; g.N = N; g.K = K; g.nsplit = 1;
  g.A = x; g.sa_m = K; g.sa_k = 1; g.B = W; g.sb_n = K; g.sb_k = 1; g.C = y; g.sc_m = N;
  g.Btiles = tiles; g.bt_ntile = cdiv(N, 16); g.bt_nkc = cdiv(K, 32);
  g.bias = b; g.relu = relu; g.drop_p = p; g.drop_seed = seed; g.drop_site = site;
  return launch_gemm(g, st);
}
// dx = dy W (+ residual), optionally gated by posmask > 0 and scaled
int linear_bwd_x_t(long M, int N, int K, const float* dy, const float* W, const void* tiles_t, float* dx, const float* posmask,
                   float cscale, const float* residual, hipStream_t st) {
  GemmArgs g{};
  g.M = (int)M; g.N = K; g.K = N; g.nsplit = 1;
  g.A = dy; g.sa_m = N; g.sa_k = 1; g.B = W; g.sb_n = 1; g.sb_k = K; g.C = dx; g.sc_m = K;
  g.Btiles = tiles_t; g.bt_ntile = cdiv(K, 16); g.bt_nkc = cdiv(N, 32);     // tiles of W^T: rows = K, reduction = N
  g.posmask = posmask; g.pm_m = K; g.cscale = cscale; g.residual = residual; g.res_m = K;
  return launch_gemm(g, st);
}

// the token plan's live-row count reaches the row-block launches of one layer call
struct MliveScope { MliveScope(const int32_t* p) { rowgemm_set_mlive(p); } ~MliveScope() { rowgemm_set_mlive(nullptr); } };

// weights of a layer -> native bf16 hi/lo operand tiles + the constant tiles of the weight-gradient stream.  The training carve
// takes both orientations (7 or 8 matrices) and the fused attention's per-head in_proj tiles in both forms (6 H more jobs of a few
// tiles each); the inference carve the four forward orientations and the forward form of each per-head pair
int enc_split_specs(const EncDims& e, const EncRoute& r, const rd_encoder_weights* w, const EncSaved& v, WsplitSpec* out) {
  const float* Ws[8] = {w->in_proj_w, w->out_proj_w, w->lin1_w, w->lin2_w, w->out_proj_w, w->lin2_w, w->lin1_w, w->in_proj_w};
  const int Ns[8] = {3 * e.D, e.D, e.nhid, e.D, e.D, e.D, e.nhid, 3 * e.D};
  const int Ks[8] = {e.D, e.D, e.D, e.nhid, e.D, e.nhid, e.D, e.D};
  const int Tr[8] = {0, 0, 0, 0, 1, 1, 1, 1};
  int njobs = v.infer ? 4 : (r.panel || r.dx_rowblock) ? 8 : 7;
  for (int i = 0; i < njobs; ++i) out[i] = WsplitSpec{Ws[i], Ns[i], Ks[i], Tr[i], v.pl[i][0]};
  if (r.attn_tiles && v.infer) {
    WsplitSpec both[12];
    const int nb = e.H <= 2 ? attnfuse_split_specs(w->in_proj_w, e.D, e.H, e.Hd, v.afw, v.afw, both) : 0;
    for (int i = 0; i < nb; i += 2) out[njobs++] = both[i];                // (forward form, input-gradient form) pairs: the first of each
  } else if (r.attn_tiles) njobs += attnfuse_split_specs(w->in_proj_w, e.D, e.H, e.Hd, v.afw, v.abw, out + njobs);
  return njobs;
}
constexpr int ENC_MAX_SPECS = 8 + 12;                  // per layer: 8 orientations + (fused attention, H = 2) 6 H
bool enc_wants_ones(const EncRoute& r, const EncSaved& v) { return (r.tw || r.panel) && !v.infer; }   // the backward streams weight gradients
int enc_prepare(const EncDims& e, const EncRoute& r, const rd_encoder_weights* w, const EncSaved& v, hipStream_t st) {
  WsplitSpec specs[ENC_MAX_SPECS];
  const int n = enc_split_specs(e, r, w, v, specs);
  void* on[1] = {v.ones};
  return launch_wsplit_specs(n, specs, enc_wants_ones(r, v) ? 1 : 0, on, st);
}

}  // namespace
}  // namespace rd

using namespace rd;

extern "C" size_t rd_encoder_layer_saved_bytes(const rd_shape* s) {
  if (check_enc(s)) return 0;
  return carve_saved(enc_dims(s), nullptr, attn_big(enc_dims(s))).bytes;
}
extern "C" size_t rd_encoder_layer_workspace_bytes(const rd_shape* s) {
  if (check_enc(s)) return 0;
  return carve_ws(enc_dims(s), nullptr, attn_big(enc_dims(s))).bytes;
}

// not part of the ABI (include/raindrop_hip_debug.h): bit i of *bits = field i of EncRoute, in declaration order
extern "C" int rd_debug_encoder_route(const rd_shape* s, int32_t with_plan, uint32_t* bits) {
  int rc = check_enc(s);
  if (rc) return rc;
  RD_REQUIRE(bits, "NULL tensor");
  const EncRoute r = enc_route(enc_dims(s), with_plan != 0, ROUTE_ALL);
  const bool f[17] = {r.rg, r.dx_rowblock, r.tw, r.panel, r.tw2, r.big, r.lnf1, r.lnf2, r.lnb, r.chain_fwd, r.chain_bwd, r.attn_tiles,
                      r.afuse_fwd, r.afuse_bwd, r.lean, r.infer, r.plan_ok};
  *bits = 0;
  for (int i = 0; i < 17; ++i) *bits |= (uint32_t)f[i] << i;
  return RD_OK;
}

extern "C" int rd_encoder_layer_prepare(const rd_shape* s, const rd_encoder_weights* w, void* saved, size_t saved_bytes,
                                        void* stream) {
  int rc = check_enc(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(w && saved, "NULL tensor");
  const EncDims e = enc_dims(s);
  const EncRoute r = enc_route(e, false, ROUTE_FWD);
  EncSaved v = carve_for_bytes(e, r, saved, saved_bytes);
  RD_REQUIRE(saved_bytes >= v.bytes, "saved buffer too small");
  if (!r.rg) return RD_OK;                           // the tiled path reads the fp32 weights directly
  return enc_prepare(e, r, w, v, (hipStream_t)stream);
}

// Every weight matrix of a training step -> matrix-core operand tiles in ONE launch: the encoder layers' (what
// rd_encoder_layer_prepare does per layer) and the message-passing stage's (what rd_sensor_stage_fwd does first).
static int step_prepare_impl(const rd_shape* s, int32_t nlayers, const rd_encoder_weights* const* w, void* const* enc_saved,
                             const size_t* enc_saved_bytes, const float* W1, const float* W2, void* k1_saved, size_t k1_saved_bytes,
                             const int64_t* lengths, int32_t* plan_out, uint64_t* seed_cell_dev, uint64_t delta, void* stream) {
  int rc = check_enc(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(nlayers >= 0 && nlayers <= 2 && (nlayers == 0 || (w && enc_saved && enc_saved_bytes)), "rd_step_prepare: 0..2 encoder layers");
  const EncDims e = enc_dims(s);
  const EncRoute r = enc_route(e, false, ROUTE_FWD);
  WsplitSpec specs[2 * ENC_MAX_SPECS + 8]; void* ones[4]; int n = 0, no = 0;
  if (r.rg)
    for (int l = 0; l < nlayers; ++l) {
      RD_REQUIRE(w[l] && enc_saved[l], "NULL tensor");
      EncSaved v = carve_for_bytes(e, r, enc_saved[l], enc_saved_bytes[l]);      // a buffer of the inference size: the forward's tiles only
      RD_REQUIRE(enc_saved_bytes[l] >= v.bytes, "saved buffer too small");
      n += enc_split_specs(e, r, w[l], v, specs + n);
      if (enc_wants_ones(r, v)) ones[no++] = v.ones;
    }
  if (W1 && W2 && k1_saved) n += k1_weight_split_specs(s, W1, W2, k1_saved, k1_saved_bytes, specs + n);
  if (n == 0) return plan_out ? rd_token_plan(s, lengths, plan_out, seed_cell_dev, delta, stream) : RD_OK;
  return launch_wsplit_plan(n, specs, no, ones, lengths, plan_out, s->B, s->T, seed_cell_dev, delta, (hipStream_t)stream);
}
extern "C" int rd_step_prepare(const rd_shape* s, int32_t nlayers, const rd_encoder_weights* const* w, void* const* enc_saved,
                               const size_t* enc_saved_bytes, const float* W1, const float* W2, void* k1_saved, size_t k1_saved_bytes,
                               void* stream) {
  return step_prepare_impl(s, nlayers, w, enc_saved, enc_saved_bytes, W1, W2, k1_saved, k1_saved_bytes, nullptr, nullptr, nullptr, 0, stream);
}
// rd_token_plan + rd_step_prepare as ONE launch: everything a training step needs before its first compute kernel (the plan is one
// workgroup of integer work, the splits ~1500 small tiles: two launches of 6-8 us each were mostly launch latency)
extern "C" int rd_step_begin(const rd_shape* s, const int64_t* lengths, int32_t* plan_out, uint64_t* seed_cell_dev, uint64_t delta,
                             int32_t nlayers, const rd_encoder_weights* const* w, void* const* enc_saved, const size_t* enc_saved_bytes,
                             const float* W1, const float* W2, void* k1_saved, size_t k1_saved_bytes, void* stream) {
  RD_REQUIRE(lengths && plan_out, "NULL tensor");
  return step_prepare_impl(s, nlayers, w, enc_saved, enc_saved_bytes, W1, W2, k1_saved, k1_saved_bytes, lengths, plan_out, seed_cell_dev,
                           delta, stream);
}
// 1 if rd_step_prepare covers the encoder layers / the message-passing stage of this shape in the current arithmetic mode (then
// pass RD_LAYER_WEIGHTS_PREPARED / call rd_sensor_stage_fwd_prepared), else the per-call splits must run
extern "C" int rd_step_prepare_covers(const rd_shape* s, int32_t* encoder, int32_t* sensor_stage) {
  if (check_enc(s)) return RD_EINVAL;
  if (encoder) *encoder = enc_route(enc_dims(s), false, ROUTE_RG).rg ? 1 : 0;
  if (sensor_stage) *sensor_stage = k1_route(s, K1_FUSED).fused ? 1 : 0;
  return RD_OK;
}

static int layer_fwd(const rd_shape* s, int32_t layer, const float* x, const uint8_t* mask, const rd_encoder_weights* w, float p_drop,
                     uint64_t seed, float* y, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream,
                     const EncRoute* route) {        // route: the caller's (the inference forward falls back to this one) or null
  int rc = check_enc(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;                       // empty batch
  RD_REQUIRE(x && mask && w && y && saved && workspace, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  const EncDims e = enc_dims(s);
  // token plan (rd_plan.h): x, y and every saved / scratch tensor hold the live rows only, in plan order
  const int32_t* tp = token_plan();
  const EncRoute r = route ? *route : enc_route(e, tp != nullptr, ROUTE_FWD);
  EncSaved v = carve_saved(e, saved, r.big);
  EncWs ws = carve_ws(e, workspace, r.big);
  RD_REQUIRE(saved_bytes >= v.bytes && workspace_bytes >= ws.bytes, "saved/workspace buffer too small");
  hipStream_t st = (hipStream_t)stream;
  const bool prepared = (layer & RD_LAYER_WEIGHTS_PREPARED) != 0;      // rd_encoder_layer_prepare already ran for these weights
  const uint32_t L = (uint32_t)(layer & 0xffff);
  RD_REQUIRE(!tp || (r.tw && !r.big), "token plan: this shape / mode does not run on the row-block + tile-stream path");
  RD_REQUIRE(!tp || (r.lnf1 && r.lnf2), "token plan: needs the LayerNorm-epilogue path (RD_LN_FUSE)");
  MliveScope mscope(tp);
  // ---- weights -> bf16 hi/lo planes, both orientations, one launch (the panel form, SYN256: D = 1040, has no prepare call)
  if ((r.panel || (r.rg && !prepared)) && (rc = enc_prepare(e, r, w, v, st))) return rc;
  // out = in W_i^T + b (+ ReLU, dropout) as its own launch: row-block (exporting `in` as the row tiles xt[i]) or tiled family
  auto dense = [&](int i, int N, int K, const float* in, const float* W, const float* b, float* out, int relu, float p, uint64_t sd,
                   uint32_t site) {
    if (!r.rg) return linear_fwd_t(e.M, N, K, in, W, r.panel ? v.pl[i][0] : nullptr, b, out, relu, p, sd, site, st);
    if (r.tw) rowgemm_export_next(v.xt[i]);
    return launch_rowgemm(e.M, N, K, in, K, v.pl[i][0], v.pl[i][1], out, N, b, relu, nullptr, 0, 0.f, nullptr, 0, p, sd, site, st);
  };
  // ---- in_proj ---------------------------------------------------------------------------------------------------------------
  if (!r.afuse_fwd && (rc = dense(0, 3 * e.D, e.D, x, w->in_proj_w, w->in_proj_b, v.qkv, 0, 0.f, 0, 0))) return rc;
  // ---- attention core (afuse_fwd: with in_proj inside) -------------------------------------------------------------------------
  const AttnArgs a = attn_args(e, v.qkv, mask, v.attn, v.lse, p_drop, seed, L, tp);
  if (r.afuse_fwd)
    rc = launch_attn_fused_fwd(x, v.afw, w->in_proj_b, tp, e.T, e.B, e.D, e.H, e.Hd, p_drop, seed, SITE_ATTN_PROB + L, v.attn, v.lse, st);
  else if (r.big) rc = attn_big_fwd(a, v.pbig, v.pdbig, st);
  else rc = attn_forward(a, st);
  if (rc) return rc;
  // ---- out_proj + LayerNorm1 + linear1 + linear2 + LayerNorm2 ------------------------------------------------------------------
  if (r.chain_fwd)
    return launch_enc_post_fwd(e.M, e.D, e.nhid, v.attn, x, v.pl[1][0], v.pl[2][0], v.pl[3][0], w->out_proj_b, w->lin1_b, w->lin2_b,
                               w->norm1_w, w->norm1_b, w->norm2_w, w->norm2_b, v.s1, v.x1, v.st1, v.h, v.s2, y, v.st2,
                               r.tw ? v.xt[1] : nullptr, r.tw ? v.xt[2] : nullptr, r.tw ? v.xt[3] : nullptr, p_drop, seed,
                               SITE_ATTN_OUT + L, SITE_FFN_HID + L, SITE_FFN_OUT + L, tp ? tp + plan::I_MLIVE : nullptr,
                               r.lean ? (void*)v.h : nullptr, st);
  if (r.lnf1) {
    if (r.tw) rowgemm_export_next(v.xt[1]);
    rc = launch_rowgemm_ln(e.M, e.D, e.D, v.attn, v.pl[1][0], w->out_proj_b, x, w->norm1_w, w->norm1_b, v.s1, v.x1, v.st1, p_drop, seed,
                           SITE_ATTN_OUT + L, st);
  } else if (!(rc = dense(1, e.D, e.D, v.attn, w->out_proj_w, w->out_proj_b, ws.o, 0, 0.f, 0, 0)))
    rc = launch_add_ln_fwd(x, ws.o, w->norm1_w, w->norm1_b, v.s1, v.x1, v.st1, (int)e.M, e.D, p_drop, seed, SITE_ATTN_OUT + L, st);
  if (rc) return rc;
  if ((rc = dense(2, e.nhid, e.D, v.x1, w->lin1_w, w->lin1_b, v.h, 1, p_drop, seed, SITE_FFN_HID + L))) return rc;
  if (r.lnf2) {
    if (r.tw) rowgemm_export_next(v.xt[3]);
    return launch_rowgemm_ln(e.M, e.D, e.nhid, v.h, v.pl[3][0], w->lin2_b, v.x1, w->norm2_w, w->norm2_b, v.s2, y, v.st2, p_drop, seed,
                             SITE_FFN_OUT + L, st);
  }
  if ((rc = dense(3, e.D, e.nhid, v.h, w->lin2_w, w->lin2_b, ws.f, 0, 0.f, 0, 0))) return rc;
  return launch_add_ln_fwd(v.x1, ws.f, w->norm2_w, w->norm2_b, v.s2, y, v.st2, (int)e.M, e.D, p_drop, seed, SITE_FFN_OUT + L, st);
}

extern "C" int rd_encoder_layer_fwd(const rd_shape* s, int32_t layer, const float* x, const uint8_t* mask, const rd_encoder_weights* w,
                                    float p_drop, uint64_t seed, float* y, void* saved, size_t saved_bytes, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return layer_fwd(s, layer, x, mask, w, p_drop, seed, y, saved, saved_bytes, workspace, workspace_bytes, stream, nullptr);
}

// ---- inference forward (include/raindrop_hip.h "inference forward") -----------------------------------------------------------
// Where the route has one (EncRoute::infer): the attention launch is the fused save-free one on a token plan, the saving kernels
// (into the inference buffer's qkv / lse) on the padded layout; then the save-free fused chain.  RD_LN_FUSE is part of that
// condition and, like everywhere in the route, is read once per process: flipping it later in the process changes nothing.
extern "C" int rd_infer_covers(const rd_shape* s, int32_t* sensor_stage, int32_t* encoder) {
  if (check_enc(s)) return RD_EINVAL;
  if (sensor_stage) *sensor_stage = k1_route(s, K1_SIZES).infer ? 1 : 0;
  if (encoder) *encoder = enc_route(enc_dims(s), false, ROUTE_FWD).infer ? 1 : 0;
  return RD_OK;
}

extern "C" size_t rd_encoder_layer_infer_bytes(const rd_shape* s) {
  if (check_enc(s)) return 0;
  const EncDims e = enc_dims(s);
  const EncRoute r = enc_route(e, false, ROUTE_FWD);
  return carve_saved(e, nullptr, r.big, r.infer).bytes;
}

extern "C" int rd_encoder_layer_fwd_infer(const rd_shape* s, int32_t layer, const float* x, const uint8_t* mask,
                                          const rd_encoder_weights* w, float* y, void* saved, size_t saved_bytes, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  int rc = check_enc(s);
  if (rc) return rc;
  const EncDims e = enc_dims(s);
  const int32_t* tp = token_plan();
  const EncRoute r = enc_route(e, tp != nullptr, ROUTE_FWD);
  if (!r.infer)                                       // no save-free instantiation: the saving forward into the buffer the query sized
    return layer_fwd(s, layer, x, mask, w, 0.f, 0, y, saved, saved_bytes, workspace, workspace_bytes, stream, &r);
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(x && mask && w && y && saved, "NULL tensor");
  EncSaved v = carve_for_bytes(e, r, saved, saved_bytes);
  RD_REQUIRE(saved_bytes >= v.bytes, "inference buffer too small: %zu < %zu", saved_bytes, v.bytes);
  hipStream_t st = (hipStream_t)stream;
  const bool prepared = (layer & RD_LAYER_WEIGHTS_PREPARED) != 0;
  const uint32_t L = (uint32_t)(layer & 0xffff);
  MliveScope mscope(tp);
  if (!prepared) {                                    // the forward's tiles only, whichever carve the buffer holds
    EncSaved vf = v; vf.infer = true;
    if ((rc = enc_prepare(e, r, w, vf, st))) return rc;
  }
  // ---- in_proj (without its row-tile export) + attention core ------------------------------------------------------------------
  if (r.afuse_fwd) {
    if ((rc = launch_attn_fused_fwd(x, v.afw, w->in_proj_b, tp, e.T, e.B, e.D, e.H, e.Hd, 0.f, 0, SITE_ATTN_PROB + L, v.attn, nullptr, st, false)))
      return rc;
  } else {
    if ((rc = launch_rowgemm(e.M, 3 * e.D, e.D, x, e.D, v.pl[0][0], v.pl[0][1], v.qkv, 3 * e.D, w->in_proj_b, 0, nullptr, 0,
                             0.f, nullptr, 0, 0.f, 0, 0, st))) return rc;
    if ((rc = attn_forward(attn_args(e, v.qkv, mask, v.attn, v.lse, 0.f, 0, L, tp), st))) return rc;
  }
  // ---- out_proj + LayerNorm1 + linear1 + linear2 + LayerNorm2: the save-free chain ---------------------------------------------
  return launch_enc_post_fwd(e.M, e.D, e.nhid, v.attn, x, v.pl[1][0], v.pl[2][0], v.pl[3][0], w->out_proj_b, w->lin1_b, w->lin2_b,
                             w->norm1_w, w->norm1_b, w->norm2_w, w->norm2_b, nullptr, nullptr, nullptr, nullptr, nullptr, y, nullptr,
                             nullptr, nullptr, nullptr, 0.f, 0, SITE_ATTN_OUT + L, SITE_FFN_HID + L, SITE_FFN_OUT + L,
                             tp ? tp + plan::I_MLIVE : nullptr, nullptr, st, false);
}

extern "C" int rd_encoder_layer_bwd(const rd_shape* s, int32_t layer, const float* x, const uint8_t* mask,
                                    const rd_encoder_weights* w, float p_drop, uint64_t seed, const void* saved,
                                    size_t saved_bytes, const float* dy, float* dx, const rd_encoder_grads* g,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_enc(s);
  if (rc) return rc;
  RD_REQUIRE(x && mask && w && saved && dy && dx && g && workspace, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  const EncDims e = enc_dims(s);
  const int32_t* tp = token_plan();
  const EncRoute r = enc_route(e, tp != nullptr, ROUTE_BWD);
  EncSaved v = carve_saved(e, const_cast<void*>(saved), r.big);
  EncWs ws = carve_ws(e, workspace, r.big);
  RD_REQUIRE(saved_bytes >= v.bytes && workspace_bytes >= ws.bytes, "saved/workspace buffer too small");
  hipStream_t st = (hipStream_t)stream;
  if (e.B == 0) return RD_OK;
  const uint32_t L = (uint32_t)layer;
  const float gate = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 0.f;      // scale of the h > 0 gate of linear2's input gradient
  RD_REQUIRE(!tp || (r.tw && !r.big), "token plan: this shape / mode does not run on the row-block + tile-stream path");
  RD_REQUIRE(!tp || r.lnb, "token plan: needs the LayerNorm-backward prologue path (RD_LNB_FUSE)");
  MliveScope mscope(tp);
  // no tile stream: each weight gradient is a split-K GEMM once its dy is complete, launch_colsum2 sums the LayerNorm partials
  const bool wg_gemm = !r.tw && !r.tw2;
  const int lnb_rows = cdiv((int)e.M, LN_RPB);
  // dx = dy W (+ residual; gated by posmask > 0 and scaled) as its own launch: row-block on the transposed planes pl[p] (exporting
  // dy as the row tiles dt[t]; in_proj': reduction 3D, was 70 us as a tiled GEMM) or tiled family
  auto dgrad = [&](bool rowblock, int p, int t, int N, int K, const float* dyv, const float* W, float* dxv, const float* posmask,
                   float cscale, const float* residual) {
    if (!rowblock) return linear_bwd_x_t(e.M, N, K, dyv, W, r.panel ? v.pl[p][0] : nullptr, dxv, posmask, cscale, residual, st);
    if (r.tw) rowgemm_export_next(ws.dt[t]);
    return launch_rowgemm(e.M, K, N, dyv, N, v.pl[p][0], v.pl[p][1], dxv, K, nullptr, 0, posmask, posmask ? K : 0, cscale, residual,
                          residual ? K : 0, 0.f, 0, 0, st);
  };
  // ---- LayerNorm2' + linear2' + linear1' + LayerNorm1' + out_proj': dy -> ds2, ds1, da ------------------------------------------
  if (r.chain_bwd) {
    if ((rc = launch_enc_pre_bwd(e.M, e.D, e.nhid, dy, v.s2, v.st2, w->norm2_w, v.h, v.s1, v.st1, w->norm1_w, v.pl[5][0], v.pl[6][0],
                                 v.pl[4][0], ws.ds2, ws.ds1, ws.da, ws.lnpart, ws.lnpart1, ws.dt[0], ws.dt[1], ws.dt[2], p_drop, seed,
                                 SITE_FFN_OUT + L, SITE_ATTN_OUT + L, tp ? tp + plan::I_MLIVE : nullptr,
                                 r.lean ? (const void*)v.h : nullptr, st))) return rc;
  } else if (r.lnb) {                                 // three row-block products, each LayerNorm' in the prologue of the next
    rowgemm_export_next(ws.dt[0]);                    // du = (df W2) gated by h>0, * keep
    if ((rc = launch_rowgemm_lnb(e.M, e.nhid, e.D, dy, v.s2, v.st2, w->norm2_w, ws.ds2, ws.lnpart, p_drop, seed, SITE_FFN_OUT + L,
                                 v.pl[5][0], ws.du, e.nhid, v.h, e.nhid, gate, st))) return rc;
    if ((rc = dgrad(true, 6, 1, e.nhid, e.D, ws.du, w->lin1_w, ws.dx1, nullptr, 0.f, ws.ds2))) return rc;
    rowgemm_export_next(ws.dt[2]);
    if ((rc = launch_rowgemm_lnb(e.M, e.D, e.D, ws.dx1, v.s1, v.st1, w->norm1_w, ws.ds1, ws.lnpart1, p_drop, seed,
                                 SITE_ATTN_OUT + L, v.pl[4][0], ws.da, e.D, nullptr, 0, 0.f, st))) return rc;
  } else {                                            // stand-alone LayerNorm' launches around row-block (rg) or tiled products
    // LayerNorm 2:  ds2 (residual path), df = ds2 o mask(ffn out)
    if ((rc = launch_ln_bwd(dy, v.s2, v.st2, w->norm2_w, ws.ds2, ws.df, ws.lnpart, (int)e.M, e.D, p_drop, seed, SITE_FFN_OUT + L, st))) return rc;
    if (!r.tw && (rc = launch_colsum2(ws.lnpart, lnb_rows, 2 * e.D, 2 * e.D, g->norm2_w, e.D, g->norm2_b, ws.lnred, st))) return rc;
    // FFN: du = (df W2) gated by h>0, * keep;  dx1 = du W1 + ds2
    if (wg_gemm && (rc = launch_wgrad(e.M, e.D, e.nhid, ws.df, e.D, v.h, e.nhid, g->lin2_w, g->lin2_b, ws.splitk, st))) return rc;
    if ((rc = dgrad(r.rg, 5, 0, e.D, e.nhid, ws.df, w->lin2_w, ws.du, v.h, gate, nullptr))) return rc;
    if (wg_gemm && (rc = launch_wgrad(e.M, e.nhid, e.D, ws.du, e.nhid, v.x1, e.D, g->lin1_w, g->lin1_b, ws.splitk, st))) return rc;
    if ((rc = dgrad(r.rg, 6, 1, e.nhid, e.D, ws.du, w->lin1_w, ws.dx1, nullptr, 0.f, ws.ds2))) return rc;
    // LayerNorm 1
    if ((rc = launch_ln_bwd(ws.dx1, v.s1, v.st1, w->norm1_w, ws.ds1, ws.dout, r.tw ? ws.lnpart1 : ws.lnpart, (int)e.M, e.D,
                            p_drop, seed, SITE_ATTN_OUT + L, st))) return rc;
    if (!r.tw && (rc = launch_colsum2(ws.lnpart, lnb_rows, 2 * e.D, 2 * e.D, g->norm1_w, e.D, g->norm1_b, ws.lnred, st))) return rc;
    // attention output projection
    if (wg_gemm && (rc = launch_wgrad(e.M, e.D, e.D, ws.dout, e.D, v.attn, e.D, g->out_proj_w, g->out_proj_b, ws.splitk, st))) return rc;
    if ((rc = dgrad(r.rg, 4, 2, e.D, e.D, ws.dout, w->out_proj_w, ws.da, nullptr, 0.f, nullptr))) return rc;
  }
  // ---- attention core (afuse_bwd: with in_proj' inside) -------------------------------------------------------------------------
  AttnArgs a = attn_args(e, v.qkv, mask, v.attn, v.lse, p_drop, seed, L, tp);
  a.dout = ws.da; a.dqkv = ws.dqkv; a.delta = ws.delta;
  if (r.afuse_bwd)
    rc = launch_attn_fused_bwd(x, v.afw, v.abw, w->in_proj_b, tp, e.T, e.B, e.D, e.H, e.Hd, p_drop, seed, SITE_ATTN_PROB + L, v.attn, v.lse,
                               ws.da, ws.ds1, dx, v.xt[0], ws.dt[3], st);
  else if (r.big) rc = attn_big_bwd(a, v.pbig, v.pdbig, ws.dsbig, st);
  else rc = attn_backward(a, st);
  if (rc) return rc;
  // ---- in_proj': dx = dqkv W_in + ds1 ----------------------------------------------------------------------------------------------
  if (wg_gemm && (rc = launch_wgrad(e.M, 3 * e.D, e.D, ws.dqkv, 3 * e.D, x, e.D, g->in_proj_w, g->in_proj_b, ws.splitk, st))) return rc;
  if (!r.afuse_bwd && (rc = dgrad(r.dx_rowblock, 7, 3, 3 * e.D, e.D, ws.dqkv, w->in_proj_w, dx, nullptr, 0.f, ws.ds1))) return rc;
  // ---- the four weight gradients as one tile stream ----------------------------------------------------------------------------
  if (wg_gemm) return RD_OK;
  TileWgradJob jobs[4] = {
      {ws.dt[3], v.xt[0], ws.twpart[3], g->in_proj_w, g->in_proj_b, 3 * e.D, e.D, nullptr, 0, 0, 0, 0, 0},      // dqkv^T x
      {ws.dt[1], v.xt[2], ws.twpart[1], g->lin1_w, g->lin1_b, e.nhid, e.D, nullptr, 0, 0, 0, 0, 0},             // du^T x1
      {ws.dt[0], v.xt[3], ws.twpart[0], g->lin2_w, g->lin2_b, e.D, e.nhid, nullptr, 0, 0, 0, 0, 0},             // df^T h
      {ws.dt[2], v.xt[1], ws.twpart[2], g->out_proj_w, g->out_proj_b, e.D, e.D, nullptr, 0, 0, 0, 0, 0}};       // dout^T attn
  if (r.afuse_bwd) {   // x and dqkv tiles come from the fused attention backward: per-sample chunk space, head-padded dqkv columns
    jobs[0].N = attnfuse_padded_cols(e.H); jobs[0].s32 = tp + plan::I_SCHUNK; jobs[0].S = (int)attn_chunks(e);
    jobs[0].hd = e.Hd; jobs[0].hdp = 16 * attnfuse_nth(); jobs[0].H = e.H; jobs[0].D = e.D;
  }
  if (r.tw2) {
    // no product exported tiles: every operand of the four is complete and still in place (ws.* are this call's, v.* the forward's),
    // one conversion launch makes them.  The LayerNorm column sums went their own way above (launch_colsum2).
    const float* src[8] = {ws.df, ws.du, ws.dout, ws.dqkv, x, v.attn, v.x1, v.h};
    const long ld[8] = {e.D, e.nhid, e.D, 3L * e.D, e.D, e.D, e.D, e.nhid};
    const int cols[8] = {e.D, e.nhid, e.D, 3 * e.D, e.D, e.D, e.D, e.nhid};
    void* dst[8] = {ws.dt[0], ws.dt[1], ws.dt[2], ws.dt[3], v.xt[0], v.xt[1], v.xt[2], v.xt[3]};
    if ((rc = launch_rows_to_tiles(e.M, 8, src, ld, cols, dst, st))) return rc;
    return launch_tile_wgrad(e.M, 4, jobs, v.ones, 0, nullptr, st, nullptr);
  }
  const int lnrows = r.chain_bwd ? encfuse_part_rows(e.M) : (r.lnb ? rowgemm_lnb_part_rows(e.M) : lnb_rows);
  const TileColsumJob cs[2] = {{ws.lnpart, lnrows, 2 * e.D, e.D, g->norm2_w, g->norm2_b},
                               {ws.lnpart1, lnrows, 2 * e.D, e.D, g->norm1_w, g->norm1_b}};
  return launch_tile_wgrad(e.M, 4, jobs, v.ones, 2, cs, st, tp ? tp + plan::I_S32 : nullptr);
}

extern "C" int rd_masked_mean_fwd(const rd_shape* s, int32_t D, const float* r, const uint8_t* mask,
                                  const int64_t* lengths, float* out, int32_t ldo, void* stream) {
  RD_REQUIRE(s && s->T > 0 && s->B >= 0 && D > 0 && ldo >= D, "bad arguments");
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(r && mask && lengths && out, "NULL tensor");
  hipLaunchKernelGGL(k_masked_mean_fwd, dim3(s->B, cdiv(D, 64)), dim3(1024), 0, (hipStream_t)stream, r, mask, lengths,
                     out, s->T, s->B, D, ldo, token_plan());
  return check_launch("k_masked_mean_fwd");
}

extern "C" int rd_masked_mean_bwd(const rd_shape* s, int32_t D, const float* dout, int32_t ldo,
                                  const uint8_t* mask, const int64_t* lengths, float* dr, void* stream) {
  RD_REQUIRE(s && s->T > 0 && s->B >= 0 && D > 0 && ldo >= D, "bad arguments");
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(dout && mask && lengths && dr, "NULL tensor");
  const long n = (long)s->T * s->B * D;
  int blocks = (int)((n + 255) / 256); if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_masked_mean_bwd, dim3(blocks), dim3(256), 0, (hipStream_t)stream, dout, mask, lengths, dr,
                     s->T, s->B, D, ldo);
  return check_launch("k_masked_mean_bwd");
}
