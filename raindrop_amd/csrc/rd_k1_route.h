// rd_k1_route.h -- what the host side of the sensor stage (kernel family K1) shares between rd_msgpass.hip, rd_msgpass_fused.hip and
// rd_temporal.hip: the route of a call, decided ONCE (k1_route), the argument block of the fused kernels and their launch interface.
#pragma once
#include <stdlib.h>

#include "rd_common.h"
#include "rd_encoder.h"
#include "rd_k1_layout.h"

namespace rd {

struct FusedArgs {
  const float *src, *R_u, *b1, *b2, *ssum;
  const float *times, *tscale; const int64_t* lengths; uint8_t* mask; int d_pe;   // optional PE / mask (fwd)
  const __bf16* wt;              // weight tiles [layer 2][orient 2][nct][NKC][hi/lo][64][8]
  __bf16* ones;                  // bwd writes the constant bias-gradient operand tile of rd_msgpass_dw.hip here
  __bf16 *tpX, *tpY1, *tpD1, *tpD2;   // row tiles of X, Y1 (fwd writes) and dZ1, dZ2 (bwd writes)
  // gates (rd_k1_layout.h): m1 = Y1 > 0 as 64-bit lane masks [slot][column tile][RT][4] of the epilogue that made them (the backward's
  // epilogue has the same lane -> element map and applies them as v_cndmask operands); m2 = Y2 > 0 and mx = X > 0 as one byte per
  // (slot, t, f) cell, bit c = channel c
  uint64_t* m1; uint8_t *m2, *mx;
  float* z;
  const float* dz;               // bwd
  float* rupart;
  int B, T, F, K, ldz, nct, q, rem, per;
  float p_drop; uint64_t seed; const uint64_t* seed_cell;
  unsigned long long* stamps;    // debug: per-phase clock64() of every wave of the first 4 workgroups
  const int32_t* plan;           // token plan (rd_plan.h) or null: which steps of a sample are live, and where its z rows are
  int* lin;                      // [B] per slot: 1 + last step with a non-zero observation (fwd writes, bwd reads)
  const float* coef;             // COEF instantiations: [2][B][F] per-(layer, sample, sensor) aggregate coefficients in place of ssum[f]
};

// ---- the route of a sensor-stage call ----------------------------------------------------------------------------------------
// The fused envelope (rd_k1_layout.h): the staging tile [F][244] fp32 must fit inside two bf16 planes [RT*16][256]; d_ob == 4 only.
// A function of the shape ALONE: the four byte queries size their buffers by it, so sizes must not depend on the precision mode or
// the environment (a caller may size under one mode and run under another).
inline bool k1_envelope(const rd_shape* s) {
  const int K = s->T * s->d_ob;
  return s->d_ob == 4 && s->F <= 48 && K <= 240 && (K % 16) == 0 && K >= 16;
}
// Shapes whose two weight gradients dW_l = dZ_l^T in_l ([K, K], reduction over the B*F graph rows) take the conversion pass + tile
// stream instead of the split-K GEMM pair: enough rows to amortise the conversion and a K the stream's 5 x 6-tile blocks fill
// and many more rows than columns (P12: 9216 x 860: 1.70 -> 1.64 ms/step, 1.45 -> 1.37 in the single-product mode; not SYN256's
// 4096 x 2048, where the pass + stream come out 1 % behind the GEMM pair, nor PAM's 1088 rows).  Part of the workspace LAYOUT, so it
// must not depend on the arithmetic mode or the environment.
inline bool wgrad_stream_shape(long M, long K) { return M >= 2048 && K >= 512 && (K % 4) == 0 && M >= 4 * K; }

// Which kernels one call of this shape runs, in the current arithmetic mode and switches.  Decided HERE and nowhere else: prepare,
// the `covers` queries, rd_msgpass_infer_bytes and the forward / inference / backward entry points read these fields.
// (include/raindrop_hip_debug.h rd_debug_sensor_route: the bit of each field.)  A use evaluates only what it consumes, so no
// entry point reads a switch it cannot use: K1_FUSED `fused` alone (rd_step_prepare_covers, the weight-split jobs), K1_SIZES `fused`
// and `infer` (rd_msgpass_infer_bytes, rd_infer_covers), K1_FWD all but `wgrad_stream`, K1_BWD all but `infer`.
enum K1Use { K1_FUSED, K1_SIZES, K1_FWD, K1_BWD, K1_ALL };
struct K1Route {
  bool fused;         // the LDS-resident kernels (rd_msgpass_fused.hip, rd_msgpass_dw.hip); else the tiled GEMM family (rd_msgpass.hip)
  int rt;             // fused: row tiles ceil(F / 16) = 1 .. 3, the runtime-shape instantiation <rt, 0, 0>
  bool specialised;   // fused, and the P19 instantiation <3, 34, 60> runs instead of <3, 0, 0>.  RD_K1_SPECIALIZE=0: A/B, parity test
  bool infer;         // a save-free forward exists (the specialised shape only): rd_sensor_stage_fwd_infer, rd_msgpass_infer_bytes
  bool coef;          // a coefficient-dropout table is given: the COEF instantiations
  bool tiles;         // generic side, bf16 modes: the forward splits the weights and the four products take launch_gemm's panel form
  bool wgrad_stream;  // generic side: weight gradients by one conversion pass + the tile stream.  RD_K1_WGRAD_STREAM=0: the split-K GEMMs
};
// ldz: row stride of z / dz; with_pe: the call writes PE and the mask (times != null)
inline K1Route k1_route(const rd_shape* s, K1Use use, int ldz = 0, bool with_pe = false, bool with_coef = false) {
  // read per call (tests flip them inside one process), and only where the answer can matter
  auto off = [](const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; };
  K1Route r{};
  r.coef = with_coef;
  // index arithmetic of the kernels is 32-bit with 24-bit multiplies: B*T rows < 2^22 (with ldz < 1024, checked at the launch).
  // RD_K1_FUSED=0 routes the envelope through the generic tiled path (the parity tests compare the two paths in one process)
  r.fused = precision() == RD_PREC_BF16X3 && k1_envelope(s) && (long)s->B * s->T < (1L << 22) && !off("RD_K1_FUSED");
  if (use == K1_FUSED) return r;
  if (r.fused) {
    r.rt = (s->F + 15) / 16;
    // The specialised instantiation fixes ldz = 4 F + 16 and d_pe = 16 (the model's layout).  Each entry point's test, as it was:
    //   rd_msgpass_fwd (writes no PE) and the backward: ldz == 4 F + 16, whatever d_pe is;
    //   the sensor-stage forwards (with_pe): d_pe == 16 too;
    //   the inference queries (no ldz): s->d_pe == 16 alone.
    const bool spec = use != K1_SIZES && ldz == 4 * s->F + 16 && (!with_pe || s->d_pe == 16), inf = use != K1_BWD && s->d_pe == 16;
    const bool on = s->F == 34 && s->T == 60 && (spec || inf) && !off("RD_K1_SPECIALIZE");
    r.specialised = on && spec; r.infer = on && inf;
    return r;
  }
  r.tiles = precision() != RD_PREC_FP32;
  const long M = (long)s->B * s->F, K = (long)s->T * s->d_ob;
  r.wgrad_stream = (use == K1_BWD || use == K1_ALL) && r.tiles && wgrad_stream_shape(M, K) && tile_wgrad_ok((int)K, (int)K) &&
                   !off("RD_K1_WGRAD_STREAM");
  return r;
}

// ---- launch interface of the fused kernels (rd_msgpass_fused.hip) and their weight gradients (rd_msgpass_dw.hip) ---------------
int fused_wprep(const k1::Layout& L, const float* W1, const float* W2, void* wt, hipStream_t st);
// `a`: the caller's tensors, the carved buffers and p_drop / seed by field; the layout numbers, token plan, `lin`, seed cell and debug
// stamps are filled in here.  save = false: the save-free forward (tpX .. mx are not touched and may be null)
int fused_msgpass(FusedArgs a, const k1::Layout& L, const K1Route& r, bool bwd, bool save, hipStream_t st);
int fused_dw(const k1::Layout& L, const k1::DwPlan& P, const void* tpX, const void* tpY1, const void* tpD1,
             const void* tpD2, const void* ones, float* part, const float* rupart, float* dW1, float* db1, float* dW2, float* db2,
             float* dRu, hipStream_t st);
// the operand-tile jobs of the fused stage for rd_step_prepare (rd_msgpass.hip)
int k1_weight_split_specs(const rd_shape* s, const float* W1, const float* W2, void* saved, size_t saved_bytes, WsplitSpec* out);
}  // namespace rd
