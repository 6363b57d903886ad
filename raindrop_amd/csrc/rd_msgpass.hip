// rd_msgpass.hip -- inter-sensor message passing (kernel family K1), general path.
//
// Replaces, for the whole batch at once, the reference's per-sample Python loop
//   code/models_rd.py:285-296   observation embedding  h = relu(repeat_interleave(src) * R_u)
//   code/models_rd.py:313-343   for unit in range(batch): reshape -> ob_propagation ->
//                               ob_propagation_layer2 -> reshape back -> output[:, unit, :] = ...
//   code/Ob_propagation.py:157-228  message(): edge softmax, relu(lin_value(x_i)) * gamma;
//                               aggregate(): scatter-add onto the target node
// On the shipped (default) branch the value multiplied by the softmax is the TARGET node's own
// relu(lin_value(x_i)), so summing the messages into target i gives V[i] * sum_j gamma[j,i]
// (SURVEY.md fact 2).  The per-target coefficient sum `ssum` comes from rd_edge_softmax (the
// graph kernel), and lin_value is evaluated once per NODE instead of once per EDGE.
//
// This file holds the shape-generic path (any T, F): the [B*F, K] x [K, K] products run on the
// tiled MFMA GEMM (rd_gemm.hip) with the ReLU / aggregate-scale / layout-scatter fused into its
// epilogue.  The LDS-resident fused kernel for small K lives in rd_msgpass_fused.hip.
#include <stdlib.h>
#include <algorithm>

#include "rd_k1_route.h"
#include "rd_plan.h"
#include "rd_rng.h"

namespace rd {
namespace {

// X[b,f,t*d+c] = relu(src[t,b,f] * R_u[f*d+c])   (code/models_rd.py:290-291 + the layout change
// of :326-327).  One workgroup per (sample, sensor-chunk); writes are contiguous in K.
__global__ __launch_bounds__(256) void k_obs_embed(const float* __restrict__ src,
                                                   const float* __restrict__ R_u,
                                                   float* __restrict__ X, int B, int T, int F, int d,
                                                   float p_drop, uint64_t seed, const uint64_t* cell) {
  seed = eff_seed(seed, cell);
  const int b = blockIdx.x;
  const int K = T * d;
  const long total = (long)F * K;
  for (long o = blockIdx.y * (long)blockDim.x + threadIdx.x; o < total;
       o += (long)gridDim.y * blockDim.x) {
    const int f = (int)(o / K);
    const int k = (int)(o - (long)f * K);
    const int t = k / d, c = k - t * d;
    float v = fmaxf(src[((long)t * B + b) * (2 * F) + f] * R_u[f * d + c], 0.f);
    // nn.Dropout on h (code/models_rd.py:296); the mask is indexed in h's own [T,B,F*d] order
    if (p_drop > 0.f && v > 0.f)
      v *= dropout_scale(seed, SITE_OBS_EMBED, ((uint64_t)t * B + b) * (F * d) + f * d + c, p_drop,
                         1.0f / (1.0f - p_drop));
    X[(long)b * total + o] = v;
  }
}

// dz2[b,f,t*d+c] = dz[t,b,f*d+c] * ssum[b*sstride + f] * (z[t,b,f*d+c] > 0)
// (backward of `out * gamma` + scatter-add + ReLU of layer 2, read through the [T,B,ldz] layout).  sstride = 0: the shared ssum[f];
// F: layer 2's rows of the coefficient-dropout table (rd_msgpass_bwd_coef).
__global__ __launch_bounds__(256) void k_msg_dz2(const float* __restrict__ dz,
                                                 const float* __restrict__ z,
                                                 const float* __restrict__ ssum,
                                                 float* __restrict__ dz2, int B, int T, int F, int d,
                                                 long ldz, const int32_t* __restrict__ sp_row0, const int32_t* __restrict__ sp_len,
                                                 int sstride) {
  const int b = blockIdx.x;
  const int Fd = F * d;
  ssum += (long)b * sstride;
  const long total = (long)T * Fd;
  // token plan: sample b's step t lives at row sp_row0[b] + t of z / dz; steps >= sp_len[b] have no row and a zero gradient
  const long row0 = sp_row0 ? sp_row0[b] : b;
  const long rstep = sp_row0 ? 1 : B;
  const int len = sp_row0 ? sp_len[b] : T;
  // iterate in the SOURCE order (t, f, c) so the strided global reads are coalesced
  for (long i = blockIdx.y * (long)blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.y * blockDim.x) {
    const int t = (int)(i / Fd);
    const int fc = (int)(i - (long)t * Fd);
    const int f = fc / d, c = fc - f * d;
    float g = 0.f;
    if (t < len) {
      const long zi = (row0 + (long)t * rstep) * ldz + fc;
      g = (z[zi] > 0.f) ? dz[zi] * ssum[f] : 0.f;
    }
    dz2[((long)b * F + f) * ((long)T * d) + t * d + c] = g;
  }
}

// per-sample partial of dR_u: part[b][f*d+c] = sum_t dx[b,f,t*d+c] * (x>0) * src[t,b,f].  One wavefront per (b, f) row of
// T*d contiguous floats, lanes along t (coalesced up to the stride d), fixed-order DPP sum over the 64 lanes.
__global__ __launch_bounds__(256) void k_obs_embed_bwd(const float* __restrict__ dx,
                                                       const float* __restrict__ X,
                                                       const float* __restrict__ src,
                                                       float* __restrict__ part, int B, int T, int F,
                                                       int d, float keep_scale) {
  const int lane = threadIdx.x & 63;
  const long row = blockIdx.x * 4L + (threadIdx.x >> 6);
  if (row >= (long)B * F) return;
  const int b = (int)(row / F), f = (int)(row - (long)b * F);
  const long base = row * ((long)T * d);
  for (int c = 0; c < d; ++c) {
    float s = 0.f;
    for (int t = lane; t < T; t += 64) {
      const long o = base + (long)t * d + c;
      if (X[o] > 0.f) s += dx[o] * src[((long)t * B + b) * (2 * F) + f];   // X>0 <=> relu open AND kept
    }
    s = wave_sum64_dpp(s);
    if (lane == 0) part[row * d + c] = s * keep_scale;
  }
}

// z[t,b,f*d+c] = Y[b,f,t*d+c] * rs[b,f]  -- the [F,T*d] -> [T,F*d] layout change of code/models_rd.py:338-342 with the
// aggregate coefficient of a per-sample graph folded in (rs == null: 1).  Iterates in the DESTINATION order (coalesced stores).
__global__ __launch_bounds__(256) void k_rows_to_tokens(const float* __restrict__ Y, const float* __restrict__ rs,
                                                        float* __restrict__ z, int B, int T, int F, int d, long ldz, int bwd) {
  const int b = blockIdx.x;
  const int Fd = F * d;
  const long total = (long)T * Fd;
  float* Yw = const_cast<float*>(Y);
  for (long i = blockIdx.y * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.y * blockDim.x) {
    const int t = (int)(i / Fd);
    const int fc = (int)(i - (long)t * Fd);
    const int f = fc / d, c = fc - f * d;
    const long zi = ((long)t * B + b) * ldz + fc;
    const long yi = ((long)b * F + f) * ((long)T * d) + t * d + c;
    const float r = rs ? rs[(long)b * F + f] : 1.f;
    if (bwd) Yw[yi] = z[zi] * r;                       // dY = dz * rs (z holds dz)
    else z[zi] = Y[yi] * r;
  }
}

struct MsgWs {
  float *dz2, *dz1, *dx, *splitk, *colsum, *rupart;
  void* tl[4]; float* part[2];      // wgrad_stream_shape: row tiles of dz2, y1, dz1, x; slice partials of dW2, dW1
  size_t bytes;
  int nsplit, kps;
};

// generic (tiled-GEMM) path
MsgWs carve(const rd_shape* s, void* base) {
  const long B = s->B, F = s->F, K = (long)s->T * s->d_ob;
  const long M = B * F;
  MsgWs w;
  // split the B*F reduction of the weight gradients so that ~256+ workgroups exist
  int kps;
  const int nsplit = splitk_plan(M, (int)K, (int)K, &kps);
  w.nsplit = nsplit; w.kps = kps;
  size_t off = 0;
  auto take = [&](size_t nfloats) { float* p = base ? (float*)((char*)base + off) : nullptr;
                                    off += align_up(nfloats * sizeof(float), 256); return p; };
  w.dz2 = take(M * K); w.dz1 = take(M * K); w.dx = take(M * K);
  w.splitk = take((size_t)2 * wgrad_ws_floats(M, (int)K, (int)K));
  w.colsum = take(colsum_ws_floats((int)M, (int)K));
  w.rupart = take(B * F * s->d_ob);
  for (int i = 0; i < 4; ++i) w.tl[i] = nullptr;
  w.part[0] = w.part[1] = nullptr;
  if (wgrad_stream_shape(M, K)) {
    for (int i = 0; i < 4; ++i) w.tl[i] = take((tile_elems(M, (int)K) + 1) / 2);
    for (int i = 0; i < 2; ++i) w.part[i] = take(tile_wgrad_part_floats((int)K, (int)K));
  }
  w.bytes = off;
  return w;
}

// wt: W1, W2, W2^T, W1^T as native operand tiles (k_wsplit; bf16 modes): the B operands of the two forward products and of the two
// input-gradient products (launch_gemm's panel form), written once by the forward and kept for the backward
struct MsgSaved { float *xsave, *y1save; void* wt[4]; void* ones; int ntile, nkc; size_t bytes; };
MsgSaved carve_saved(const rd_shape* s, void* base) {
  const size_t M = (size_t)s->B * s->F, K = (size_t)s->T * s->d_ob;
  MsgSaved v; size_t off = 0;
  auto take = [&](size_t bytes) { void* p = base ? (void*)((char*)base + off) : nullptr;
                                  off += align_up(bytes, 256); return p; };
  v.xsave = (float*)take(M * K * sizeof(float));
  v.y1save = (float*)take(M * K * sizeof(float));
  const size_t plane = ((K + 15) / 16 * 16) * ((K + 31) / 32 * 32);                    // elements of one plane (rd_rowgemm.hip: k_wsplit)
  for (int i = 0; i < 4; ++i) v.wt[i] = take(2 * plane * 2);                           // hi + lo, bf16
  v.ones = take(tile_wgrad_ones_elems() * 2);                                          // constant tile of the streamed weight gradients
  v.ntile = ((int)K + 15) / 16; v.nkc = ((int)K + 31) / 32;
  v.bytes = off;
  return v;
}

// fused path (rd_k1_layout.h): forward -> backward hand-over and backward scratch
struct FusedSaved { __bf16 *wt, *tpX, *tpY1; uint64_t* m1; uint8_t *m2, *mx; size_t bytes; };
// infer: the buffer of the save-free forward (rd_msgpass_infer_bytes) -- the weight tiles, at the same offset, and nothing else
FusedSaved carve_fused_saved(const k1::Layout& L, void* base, bool infer = false) {
  FusedSaved v{}; size_t off = 0;
  auto take = [&](size_t bytes) { void* p = base ? (void*)((char*)base + off) : nullptr;
                                  off += align_up(bytes, 256); return p; };
  v.wt = (__bf16*)take(L.wt_bytes);
  if (!infer) {
    v.tpX = (__bf16*)take(L.tp_bytes); v.tpY1 = (__bf16*)take(L.tp_bytes);
    v.m1 = (uint64_t*)take(L.g1_bytes); v.m2 = (uint8_t*)take(L.g2_bytes); v.mx = (uint8_t*)take(L.mx_bytes);
  }
  v.bytes = off;
  return v;
}
struct FusedWs { __bf16 *tpD1, *tpD2, *ones; float *part, *rupart; size_t bytes; };
FusedWs carve_fused_ws(const k1::Layout& L, const k1::DwPlan& P, void* base) {
  FusedWs w; size_t off = 0;
  auto take = [&](size_t bytes) { void* p = base ? (void*)((char*)base + off) : nullptr;
                                  off += align_up(bytes, 256); return p; };
  w.tpD1 = (__bf16*)take(L.tp_bytes); w.tpD2 = (__bf16*)take(L.tp_bytes);
  w.part = (float*)take(P.part_floats * sizeof(float));
  w.rupart = (float*)take((size_t)L.B * L.F * 4 * sizeof(float));
  w.ones = (__bf16*)take(3 * k1::TILE * 2);
  w.bytes = off;
  return w;
}

int check_shape(const rd_shape* s) {
  RD_REQUIRE(s != nullptr, "rd_shape is NULL");
  RD_REQUIRE(s->B >= 0 && s->T > 0 && s->F > 0 && s->d_ob > 0, "bad rd_shape (B=%d T=%d F=%d d_ob=%d)",
             s->B, s->T, s->F, s->d_ob);
  RD_REQUIRE((long)s->B * s->F * s->T * s->d_ob < (1L << 31), "B*F*T*d_ob exceeds 2^31");
  return RD_OK;
}
bool sizable(const rd_shape* s) { return s && s->T > 0 && s->F > 0 && s->d_ob > 0 && s->B >= 0; }   // the byte queries: else 0

// grid of the element-wise kernels: one row of workgroups per sample, up to 64 of 256 threads striding over its `per` elements
dim3 sample_grid(int B, long per) { return dim3(B, (unsigned)std::min(64L, (per + 255) / 256)); }

}  // namespace
}  // namespace rd

using namespace rd;

// Buffer sizes: the larger of the generic and (inside the envelope) the fused carve, whatever the mode and switches are
extern "C" size_t rd_msgpass_workspace_bytes(const rd_shape* s) {
  if (!sizable(s)) return 0;
  size_t n = carve(s, nullptr).bytes;
  if (k1_envelope(s)) {
    const k1::Layout L = k1::make_layout(s->B, s->T, s->F);
    n = std::max(n, carve_fused_ws(L, k1::make_dw_plan(L), nullptr).bytes);
  }
  return n;
}

extern "C" size_t rd_msgpass_saved_bytes(const rd_shape* s) {
  if (!sizable(s)) return 0;
  size_t n = carve_saved(s, nullptr).bytes;
  if (k1_envelope(s)) n = std::max(n, carve_fused_saved(k1::make_layout(s->B, s->T, s->F), nullptr).bytes);
  return n;
}

// not part of the ABI (include/raindrop_hip_debug.h): the route of a sensor-stage call, K1Route's flags in declaration order, rt in bits 8-9
extern "C" int rd_debug_sensor_route(const rd_shape* s, int32_t ldz, int32_t with_pe, int32_t with_coef, uint32_t* bits) {
  int rc = check_shape(s);
  if (rc) return rc;
  RD_REQUIRE(bits, "NULL tensor");
  const K1Route r = k1_route(s, K1_ALL, ldz, with_pe != 0, with_coef != 0);
  const bool f[6] = {r.fused, r.specialised, r.infer, r.coef, r.tiles, r.wgrad_stream};
  *bits = (uint32_t)r.rt << 8;
  for (int i = 0; i < 6; ++i) *bits |= (uint32_t)f[i] << i;
  return RD_OK;
}

// The forward behind every entry point: check, route, carve what the route needs, run the stages.
// pe (null: rd_msgpass_fwd, z gets no PE columns and there is no mask): PE + padding mask + message passing in one call -- on the
//   fused path ONE launch (plus the weight split unless `prepared`) produces the whole [T,B,D] input of the temporal encoder.
// coef (null: none): the per-(layer, sample, sensor) aggregate coefficients [2][B][F] of the coefficient dropout
//   (rd_msgpass_coef_table) in place of ssum[f] -- graph row b*F + f of layer l scales by coef[l*B*F + b*F + f]
// infer: write nothing that only a backward reads, where the route has such a forward; else the saving forward
struct PeArgs { const float *times, *tscale; const int64_t* lengths; uint8_t* mask; };
static int msgpass_fwd_impl(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                            const float* b1, const float* W2, const float* b2, const float* ssum, const float* coef,
                            float p_drop, uint64_t seed, float* z, int32_t ldz, void* saved,
                            size_t saved_bytes, void* stream, const PeArgs* pe = nullptr, bool prepared = false, bool infer = false) {
  int rc = check_shape(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;                       // empty batch
  if (pe) {
    RD_REQUIRE(pe->times && pe->lengths && pe->tscale && pe->mask, "NULL tensor");
    RD_REQUIRE(s->d_pe > 0 && (s->d_pe % 2) == 0, "d_pe must be even and positive");
    ldz = s->F * s->d_ob + s->d_pe;
  }
  RD_REQUIRE(src && R_u && W1 && b1 && W2 && b2 && ssum && z && saved, "NULL tensor");
  RD_REQUIRE(ldz >= s->F * s->d_ob, "ldz (%d) < F*d_ob", ldz);
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  const K1Route r = k1_route(s, K1_FWD, ldz, pe != nullptr, coef != nullptr);
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, T = s->T, F = s->F, d = s->d_ob, K = T * d, M = B * F;
  if (r.fused) {
    const bool save = !(infer && r.infer);
    const k1::Layout L = k1::make_layout(B, T, F);
    const FusedSaved fv = carve_fused_saved(L, saved, !save);
    if (save) RD_REQUIRE(saved_bytes >= fv.bytes, "saved buffer too small: %zu < %zu", saved_bytes, fv.bytes);
    else RD_REQUIRE(saved_bytes >= fv.bytes, "inference buffer too small: %zu < %zu", saved_bytes, fv.bytes);
    if (!prepared && (rc = fused_wprep(L, W1, W2, fv.wt, st))) return rc;
    FusedArgs a{};
    a.src = src; a.R_u = R_u; a.b1 = b1; a.b2 = b2; a.ssum = ssum; a.coef = coef; a.wt = fv.wt;
    a.tpX = fv.tpX; a.tpY1 = fv.tpY1; a.m1 = fv.m1; a.m2 = fv.m2; a.mx = fv.mx;
    if (pe) { a.times = pe->times; a.lengths = pe->lengths; a.tscale = pe->tscale; a.mask = pe->mask; a.d_pe = s->d_pe; }
    a.z = z; a.ldz = ldz; a.p_drop = p_drop; a.seed = seed;
    return fused_msgpass(a, L, r, false, save, st);
  }
  const MsgSaved v = carve_saved(s, saved);
  RD_REQUIRE(saved_bytes >= v.bytes, "saved buffer too small: %zu < %zu", saved_bytes, v.bytes);
  if (pe && (rc = rd_pe_mask(s, pe->times, pe->lengths, pe->tscale, z, pe->mask, stream))) return rc;
  // token plan on the unfused path (round 4): the products run on all B*F graph rows as before -- lin_value mixes ALL of a
  // sensor's time steps, observed ones past `lengths` included -- only the last product's scatter follows the plan: step t of
  // sample b goes to row brow[b] + t, steps >= blen[b] are not stored (nothing ever reads them)
  const int32_t* tp = token_plan();
  hipLaunchKernelGGL(k_obs_embed, sample_grid(B, (long)F * K), dim3(256), 0, st, src, R_u, v.xsave, B, T, F, d, p_drop, seed, seed_cell());
  if ((rc = check_launch("k_obs_embed"))) return rc;
  if (r.tiles) {                                       // the split weights feed the panel form of launch_gemm (bf16 modes)
    const WsplitSpec specs[4] = {{W1, K, K, 0, v.wt[0]}, {W2, K, K, 0, v.wt[1]}, {W2, K, K, 1, v.wt[2]}, {W1, K, K, 1, v.wt[3]}};
    void* on[1] = {v.ones};
    if ((rc = launch_wsplit_specs(4, specs, 1, on, st))) return rc;
  }
  GemmArgs g{};
  g.M = M; g.N = K; g.K = K; g.nsplit = 1;
  g.A = v.xsave; g.sa_m = K; g.sa_k = 1;
  g.B = W1; g.sb_n = K; g.sb_k = 1;
  if (r.tiles) { g.Btiles = v.wt[0]; g.bt_ntile = v.ntile; g.bt_nkc = v.nkc; }
  g.C = v.y1save; g.sc_m = K;
  g.bias = b1; g.relu = 1; g.rowscale = ssum; g.rs_period = F;
  if (coef) { g.rowscale = coef; g.rs_period = M; }       // row b*F + f of layer 1
  if ((rc = launch_gemm(g, st))) return rc;
  g.A = v.y1save; g.B = W2; g.bias = b2;
  if (coef) g.rowscale = coef + (size_t)M;                 // layer 2's rows
  if (r.tiles) g.Btiles = v.wt[1];
  g.C = z; g.scatter = 1; g.sB = B; g.sF = F; g.sd = d; g.ldz = ldz;
  if (tp) { g.sp_row0 = tp + plan::brow_base(B, T); g.sp_len = tp + plan::blen_base(B, T); }
  return launch_gemm(g, st);
}

extern "C" int rd_msgpass_fwd(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                              const float* b1, const float* W2, const float* b2, const float* ssum,
                              float p_drop, uint64_t seed, float* z, int32_t ldz, void* saved,
                              size_t saved_bytes, void* stream) {
  return msgpass_fwd_impl(s, src, R_u, W1, b1, W2, b2, ssum, nullptr, p_drop, seed, z, ldz, saved, saved_bytes, stream);
}
extern "C" int rd_msgpass_fwd_coef(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                                   const float* b1, const float* W2, const float* b2, const float* ssum, const float* coef,
                                   float p_drop, uint64_t seed, float* z, int32_t ldz, void* saved,
                                   size_t saved_bytes, void* stream) {
  RD_REQUIRE(!s || s->B == 0 || coef, "NULL coefficient table");
  return msgpass_fwd_impl(s, src, R_u, W1, b1, W2, b2, ssum, coef, p_drop, seed, z, ldz, saved, saved_bytes, stream);
}

// the sensor-stage forwards: the same with PE and the mask
static int sensor_stage_fwd_impl(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                 const float* timescales, const float* R_u, const float* W1, const float* b1,
                                 const float* W2, const float* b2, const float* ssum, float p_drop, uint64_t seed,
                                 float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream, bool prepared,
                                 const float* coef = nullptr, bool infer = false) {
  const PeArgs pe{times, timescales, lengths, mask};
  return msgpass_fwd_impl(s, src, R_u, W1, b1, W2, b2, ssum, coef, p_drop, seed, z, 0, saved, saved_bytes, stream, &pe, prepared, infer);
}

extern "C" int rd_sensor_stage_fwd(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                   const float* timescales, const float* R_u, const float* W1, const float* b1,
                                   const float* W2, const float* b2, const float* ssum, float p_drop, uint64_t seed,
                                   float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream) {
  return sensor_stage_fwd_impl(s, src, times, lengths, timescales, R_u, W1, b1, W2, b2, ssum, p_drop, seed, z, mask, saved, saved_bytes,
                               stream, false);
}
// the same after rd_step_prepare has written the operand tiles of W1, W2 into `saved` (this step's weights): no split launch here
extern "C" int rd_sensor_stage_fwd_prepared(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                            const float* timescales, const float* R_u, const float* W1, const float* b1,
                                            const float* W2, const float* b2, const float* ssum, float p_drop, uint64_t seed,
                                            float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream) {
  return sensor_stage_fwd_impl(s, src, times, lengths, timescales, R_u, W1, b1, W2, b2, ssum, p_drop, seed, z, mask, saved, saved_bytes,
                               stream, true);
}

// the two with the coefficient-dropout table coef [2][B][F] (rd_msgpass_coef_table; caller-owned, handed to rd_msgpass_bwd_coef too)
extern "C" int rd_sensor_stage_fwd_coef(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                        const float* timescales, const float* R_u, const float* W1, const float* b1,
                                        const float* W2, const float* b2, const float* ssum, const float* coef, float p_drop,
                                        uint64_t seed, float* z, uint8_t* mask, void* saved, size_t saved_bytes, void* stream) {
  RD_REQUIRE(!s || s->B == 0 || coef, "NULL coefficient table");
  return sensor_stage_fwd_impl(s, src, times, lengths, timescales, R_u, W1, b1, W2, b2, ssum, p_drop, seed, z, mask, saved, saved_bytes,
                               stream, false, coef);
}
extern "C" int rd_sensor_stage_fwd_prepared_coef(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                                 const float* timescales, const float* R_u, const float* W1, const float* b1,
                                                 const float* W2, const float* b2, const float* ssum, const float* coef,
                                                 float p_drop, uint64_t seed, float* z, uint8_t* mask, void* saved,
                                                 size_t saved_bytes, void* stream) {
  RD_REQUIRE(!s || s->B == 0 || coef, "NULL coefficient table");
  return sensor_stage_fwd_impl(s, src, times, lengths, timescales, R_u, W1, b1, W2, b2, ssum, p_drop, seed, z, mask, saved, saved_bytes,
                               stream, true, coef);
}

// ---- inference forward: nothing that only a backward reads is written (include/raindrop_hip.h "inference forward") -------------
extern "C" size_t rd_msgpass_infer_bytes(const rd_shape* s) {
  if (!sizable(s)) return 0;
  if (!k1_route(s, K1_SIZES).infer) return rd_msgpass_saved_bytes(s);
  return carve_fused_saved(k1::make_layout(s->B, s->T, s->F), nullptr, true).bytes;
}

// (no save-free instantiation for the shape: the saving forward into the buffer the query sized)
extern "C" int rd_sensor_stage_fwd_infer(const rd_shape* s, const float* src, const float* times, const int64_t* lengths,
                                         const float* timescales, const float* R_u, const float* W1, const float* b1,
                                         const float* W2, const float* b2, const float* ssum, float* z, uint8_t* mask,
                                         void* saved, size_t saved_bytes, int32_t prepared, void* stream) {
  return sensor_stage_fwd_impl(s, src, times, lengths, timescales, R_u, W1, b1, W2, b2, ssum, 0.f, 0, z, mask, saved, saved_bytes, stream,
                               prepared != 0, nullptr, true);
}

namespace rd {
// the operand-tile jobs of the fused message-passing stage (W1, W2: forward and transposed orientation) for rd_step_prepare;
// 0 when this shape / mode does not run the fused path (its weights are then read as fp32)
int k1_weight_split_specs(const rd_shape* s, const float* W1, const float* W2, void* saved, size_t saved_bytes, WsplitSpec* out) {
  if (!s || !k1_route(s, K1_FUSED).fused || !saved) return 0;
  const k1::Layout L = k1::make_layout(s->B, s->T, s->F);
  // the tiles come first in both carves: a buffer of the inference size (rd_msgpass_infer_bytes) holds them at the same offset
  FusedSaved fv = carve_fused_saved(L, saved, saved_bytes < carve_fused_saved(L, nullptr).bytes);
  if (saved_bytes < fv.bytes) return 0;
  const size_t per = (size_t)L.nct * k1::NKC * 2 * k1::TILE;           // bf16 elements of one (layer, orientation) tile set
  const int K = L.K;
  out[0] = WsplitSpec{W1, K, K, 0, fv.wt}; out[1] = WsplitSpec{W1, K, K, 1, fv.wt + per};
  out[2] = WsplitSpec{W2, K, K, 0, fv.wt + 2 * per}; out[3] = WsplitSpec{W2, K, K, 1, fv.wt + 3 * per};
  return 4;
}
}  // namespace rd

static int msgpass_bwd_impl(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                            const float* W2, const float* ssum, const float* coef, float p_drop, const void* saved_in,
                            size_t saved_bytes, const float* z, const float* dz, int32_t ldz,
                            float* dW1, float* db1, float* dW2, float* db2, float* dR_u,
                            void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_shape(s);
  if (rc) return rc;
  RD_REQUIRE(dW1 && db1 && dW2 && db2 && dR_u, "NULL gradient output");
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, T = s->T, F = s->F, d = s->d_ob, K = T * d, M = B * F;
  if (B == 0) {
    RD_HIP(hipMemsetAsync(dW1, 0, sizeof(float) * K * K, st)); RD_HIP(hipMemsetAsync(dW2, 0, sizeof(float) * K * K, st));
    RD_HIP(hipMemsetAsync(db1, 0, sizeof(float) * K, st)); RD_HIP(hipMemsetAsync(db2, 0, sizeof(float) * K, st));
    RD_HIP(hipMemsetAsync(dR_u, 0, sizeof(float) * F * d, st));
    return RD_OK;
  }
  RD_REQUIRE(src && R_u && W1 && W2 && ssum && saved_in && z && dz, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  RD_REQUIRE(ldz >= F * d, "ldz (%d) < F*d_ob", ldz);
  void* saved = const_cast<void*>(saved_in);           // the forward's buffer: read only
  const K1Route r = k1_route(s, K1_BWD, ldz, false, coef != nullptr);
  if (r.fused) {
    // chain kernel (dz -> dZ2 -> dZ1 -> dX -> dR_u partials; dZ as row tiles) + streamed weight-gradient product + reduce
    const k1::Layout L = k1::make_layout(B, T, F);
    const k1::DwPlan P = k1::make_dw_plan(L);
    const FusedSaved fv = carve_fused_saved(L, saved);
    RD_REQUIRE(saved_bytes >= fv.bytes, "saved buffer too small");
    const FusedWs fw = carve_fused_ws(L, P, workspace);
    RD_REQUIRE(workspace && workspace_bytes >= fw.bytes, "workspace too small: %zu < %zu", workspace_bytes, fw.bytes);
    FusedArgs a{};
    a.src = src; a.ssum = ssum; a.coef = coef; a.wt = fv.wt;
    a.tpX = fv.tpX; a.tpY1 = fv.tpY1; a.m1 = fv.m1; a.m2 = fv.m2; a.mx = fv.mx;
    a.dz = dz; a.ldz = ldz; a.tpD1 = fw.tpD1; a.tpD2 = fw.tpD2; a.ones = fw.ones; a.rupart = fw.rupart; a.p_drop = p_drop;
    if ((rc = fused_msgpass(a, L, r, true, true, st))) return rc;
    return fused_dw(L, P, fv.tpX, fv.tpY1, fw.tpD1, fw.tpD2, fw.ones, fw.part, fw.rupart, dW1, db1, dW2, db2, dR_u, st);
  }
  const MsgSaved sv = carve_saved(s, saved);
  RD_REQUIRE(saved_bytes >= sv.bytes, "saved buffer too small");
  const MsgWs w = carve(s, workspace);
  RD_REQUIRE(workspace && workspace_bytes >= w.bytes, "workspace too small: %zu < %zu", workspace_bytes, w.bytes);
  const int32_t* tp = token_plan();
  hipLaunchKernelGGL(k_msg_dz2, sample_grid(B, (long)F * K), dim3(256), 0, st, dz, z, coef ? coef + (size_t)M : ssum, w.dz2, B, T, F, d, (long)ldz,
                     tp ? tp + plan::brow_base(B, T) : nullptr, tp ? tp + plan::blen_base(B, T) : nullptr, coef ? F : 0);
  if ((rc = check_launch("k_msg_dz2"))) return rc;
  // dz1 = (dz2 W2) * ssum[f] * (y1 > 0)
  GemmArgs g{};
  g.M = M; g.N = K; g.K = K; g.nsplit = 1;
  g.A = w.dz2; g.sa_m = K; g.sa_k = 1;
  g.B = W2; g.sb_n = 1; g.sb_k = K;          // B(n=k_out, k=n_red) = W2[n_red*K + k_out]
  if (r.tiles) { g.Btiles = sv.wt[2]; g.bt_ntile = sv.ntile; g.bt_nkc = sv.nkc; }      // W2^T / W1^T tiles written by the forward
  g.C = w.dz1; g.sc_m = K;
  g.rowscale = ssum; g.rs_period = F; g.posmask = sv.y1save; g.pm_m = K;
  if (coef) { g.rowscale = coef; g.rs_period = M; }       // layer 1's rows of the table
  if ((rc = launch_gemm(g, st))) return rc;
  // dx = dz1 W1
  GemmArgs h{};
  h.M = M; h.N = K; h.K = K; h.nsplit = 1;
  h.A = w.dz1; h.sa_m = K; h.sa_k = 1;
  h.B = W1; h.sb_n = 1; h.sb_k = K;
  if (r.tiles) { h.Btiles = sv.wt[3]; h.bt_ntile = sv.ntile; h.bt_nkc = sv.nkc; }
  h.C = w.dx; h.sc_m = K;
  if ((rc = launch_gemm(h, st))) return rc;
  hipLaunchKernelGGL(k_obs_embed_bwd, dim3((unsigned)(((long)B * F + 3) / 4)), dim3(256), 0, st, w.dx, sv.xsave, src, w.rupart, B, T, F, d,
                     1.0f / (1.0f - p_drop));
  if ((rc = check_launch("k_obs_embed_bwd"))) return rc;
  if ((rc = launch_colsum(w.rupart, B, F * d, F * d, dR_u, w.colsum, st))) return rc;
  // weight gradients dW_l = dz_l^T in_l (+ bias gradients as row sums of dz_l^T), split over the B*F rows
  // Large shapes in the bf16 modes (round 4): one conversion pass over the four operands + the tile stream of rd_tile_wgrad.hip,
  // instead of the split-K GEMM pair that converts both fp32 operands once per 64 x 64 output tile (12.5 % of P12's step, 10 % of
  // SYN256's).  RD_K1_WGRAD_STREAM=0: the GEMMs (A/B; read per call).
  if (r.wgrad_stream) {
    const float* srcs[4] = {w.dz2, sv.y1save, w.dz1, sv.xsave};
    const long ld[4] = {K, K, K, K};
    const int cols[4] = {K, K, K, K};
    if ((rc = launch_rows_to_tiles(M, 4, srcs, ld, cols, w.tl, st))) return rc;
    TileWgradJob jobs[2] = {{w.tl[0], w.tl[1], w.part[0], dW2, db2, K, K, nullptr, 0, 0, 0, 0, 0},       // dz2^T y1
                            {w.tl[2], w.tl[3], w.part[1], dW1, db1, K, K, nullptr, 0, 0, 0, 0, 0}};      // dz1^T x
    return launch_tile_wgrad(M, 2, jobs, sv.ones, 0, nullptr, st, nullptr);
  }
  return launch_wgrad2(M, K, K, w.dz2, sv.y1save, dW2, db2, w.dz1, sv.xsave, dW1, db1, w.splitk, st);
}

extern "C" int rd_msgpass_bwd(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                              const float* W2, const float* ssum, float p_drop, const void* saved,
                              size_t saved_bytes, const float* z, const float* dz, int32_t ldz,
                              float* dW1, float* db1, float* dW2, float* db2, float* dR_u,
                              void* workspace, size_t workspace_bytes, void* stream) {
  return msgpass_bwd_impl(s, src, R_u, W1, W2, ssum, nullptr, p_drop, saved, saved_bytes, z, dz, ldz, dW1, db1, dW2, db2, dR_u, workspace,
                          workspace_bytes, stream);
}
// backward of the `_coef` forwards: `coef` is the table the forward was given (the gates multiply by the same numbers)
extern "C" int rd_msgpass_bwd_coef(const rd_shape* s, const float* src, const float* R_u, const float* W1,
                                   const float* W2, const float* ssum, const float* coef, float p_drop, const void* saved,
                                   size_t saved_bytes, const float* z, const float* dz, int32_t ldz,
                                   float* dW1, float* db1, float* dW2, float* db2, float* dR_u,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  RD_REQUIRE(!s || s->B == 0 || coef, "NULL coefficient table");
  return msgpass_bwd_impl(s, src, R_u, W1, W2, ssum, coef, p_drop, saved, saved_bytes, z, dz, ldz, dW1, db1, dW2, db2, dR_u, workspace,
                          workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
// Building blocks of the paper-faithful sensor stage (Raindrop_v2(use_beta=True): code/models_rd.py:317-343 with the literal
// at :317 flipped).  There the two graph layers cannot be folded into one fused launch (layer 1 prunes a different edge set per
// sample), so the model composes: observation embedding -> lin_value / increase_dim (rd_linear_fwd) -> rd_graph_beta_fwd ->
// rd_edge_softmax_list_batched -> lin_value of layer 2 (rd_linear_fwd) -> rd_rows_to_tokens_fwd.
// ------------------------------------------------------------------------------------------------
extern "C" int rd_obs_embed_fwd(const rd_shape* s, const float* src, const float* R_u, float p_drop, uint64_t seed, float* X,
                                void* stream) {
  int rc = check_shape(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(src && R_u && X, "NULL tensor");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  hipLaunchKernelGGL(k_obs_embed, sample_grid(s->B, (long)s->F * s->T * s->d_ob), dim3(256), 0, (hipStream_t)stream, src, R_u, X, s->B, s->T, s->F, s->d_ob, p_drop,
                     seed, seed_cell());
  return check_launch("k_obs_embed");
}

extern "C" size_t rd_obs_embed_bwd_workspace_bytes(const rd_shape* s) {
  if (!s || s->B <= 0) return 256;
  return ((size_t)s->B * s->F * s->d_ob + (size_t)colsum_ws_floats(s->B, s->F * s->d_ob)) * sizeof(float) + 512;
}

extern "C" int rd_obs_embed_bwd(const rd_shape* s, const float* src, const float* X, const float* dX, float p_drop, float* dR_u,
                                void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_shape(s);
  if (rc) return rc;
  RD_REQUIRE(dR_u, "NULL gradient output");
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, T = s->T, F = s->F, d = s->d_ob;
  if (B == 0) { RD_HIP(hipMemsetAsync(dR_u, 0, sizeof(float) * F * d, st)); return RD_OK; }
  RD_REQUIRE(src && X && dX && workspace, "NULL tensor");
  RD_REQUIRE(workspace_bytes >= rd_obs_embed_bwd_workspace_bytes(s), "workspace too small");
  RD_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop must be in [0,1)");
  float* rupart = (float*)workspace;
  float* cws = rupart + align_up((size_t)B * F * d * sizeof(float), 256) / sizeof(float);
  hipLaunchKernelGGL(k_obs_embed_bwd, dim3((unsigned)(((long)B * F + 3) / 4)), dim3(256), 0, st, dX, X, src, rupart, B, T, F, d, 1.0f / (1.0f - p_drop));
  if ((rc = check_launch("k_obs_embed_bwd"))) return rc;
  return launch_colsum(rupart, B, F * d, F * d, dR_u, cws, st);
}

static int rows_tokens(const rd_shape* s, const float* Y, const float* rowscale, float* z, int32_t ldz, void* stream, int bwd) {
  int rc = check_shape(s);
  if (rc) return rc;
  if (s->B == 0) return RD_OK;
  RD_REQUIRE(Y && z, "NULL tensor");
  RD_REQUIRE(ldz >= s->F * s->d_ob, "ldz (%d) < F*d_ob", ldz);
  hipLaunchKernelGGL(k_rows_to_tokens, sample_grid(s->B, (long)s->F * s->T * s->d_ob), dim3(256), 0, (hipStream_t)stream, Y, rowscale, z, s->B, s->T, s->F, s->d_ob,
                     (long)ldz, bwd);
  return check_launch("k_rows_to_tokens");
}
extern "C" int rd_rows_to_tokens_fwd(const rd_shape* s, const float* Y, const float* rowscale, float* z, int32_t ldz, void* stream) {
  return rows_tokens(s, Y, rowscale, z, ldz, stream, 0);
}
extern "C" int rd_rows_to_tokens_bwd(const rd_shape* s, const float* dz, int32_t ldz, const float* rowscale, float* dY, void* stream) {
  return rows_tokens(s, dY, rowscale, const_cast<float*>(dz), ldz, stream, 1);
}
