/*
 * raindrop_hip_debug.h -- profiling hooks of libraindrop_hip.so.  NOT part of the C-ABI (include/raindrop_hip.h): no host binding
 * in raindrop_amd/_lib.py (but the route queries, DEBUG_SIGNATURES there), no stability promise; used by tools/*_timing.py and the tests only.  Each stamp setter registers (process-wide) a device
 * buffer into which the named kernels write clock64() stamps per phase, or restores normal operation when passed NULL; the
 * pointer travels to the kernels as an argument of the launches enqueued while it is registered.
 */
#ifndef RAINDROP_HIP_DEBUG_H
#define RAINDROP_HIP_DEBUG_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

void rd_debug_set_stamps(void* device_u64);          /* k_msg_fwd_fused / k_msg_bwd_fused   (tools/fused_timing.py)   */
void rd_debug_set_rowgemm_stamps(void* device_u64);  /* k_rowgemm                            (tools/rowgemm_timing.py) */
void rd_debug_set_attn_stamps(void* device_u64);     /* k_attn_*_one_b16*                    (tools/attn_timing.py)    */
void rd_debug_set_gemm_stamps(void* device_u64);     /* k_gemm_bf16x3                        (tools/gemm_timing.py)    */
void rd_debug_set_encfuse_stamps(void* device_u64);  /* k_enc_post_fwd / k_enc_pre_bwd       (tools/encfuse_timing.py) */
void rd_debug_set_head_stamps(void* device_u64);     /* k_head_rows                          (tools/head_timing.py)    */
void rd_debug_set_attnfuse_stamps(void* device_u64); /* k_attn_fwd_fused / k_attn_bwd_fused  (tools/attnfuse_timing.py) */
void rd_debug_ifetch_probe(void* ticks_device_u64, void* scratch_64_floats, void* stream);   /* 32 KB of straight-line code, one wave: clock64 ticks (bench.py config.box; tools/probe_clocks.hip) */
void rd_debug_set_splitk_want(int workgroups);       /* target workgroup count of the split-K weight-gradient plan     */
/* Launch log (tests/switch_child.py): host memory only, no kernel sees it.  While it is on, every launch site records the name it
 * reports to the error check (the kernel, with the tile / prefetch / column-group variant where one name would cover two paths).
 * Switching it (either way) clears the set; off, the default, costs a launch one load and one branch.  The read copies the distinct
 * names so far, joined by '\n' and NUL-terminated, into out[cap] (whole names only) and returns the length all of them need.
 * The bootstrap of the validation metrics (rd_metrics_boot.hip) reports "k_boot_sort", "k_boot_stats", "k_boot_means"
 * (rd_rank_bootstrap), "k_boot_summary" (rd_rank_bootstrap_summary) and "k_boot_counts" (rd_rank_bootstrap_counts).
 * The calibration (rd_metrics_calib.hip) reports "k_calib_rows", "k_calib_finish" (rd_calibration) and "k_fit_temperature<lds>" or
 * "k_fit_temperature<global>" (rd_fit_temperature: the logits staged in LDS, or re-read from global memory). */
void rd_debug_launch_log(int on);
size_t rd_debug_launch_log_read(char* out, size_t cap);
/* The route one encoder layer of this shape takes (rd_temporal.hip enc_route) in the current arithmetic mode and switches, with or
 * without a token plan: which of its kernel forms run, nothing more.  Needs no device.  Bit i of *bits:
 *    0 rg           all four forward products on the row-block kernels       9 chain_fwd   out_proj .. LayerNorm2 as one launch
 *    1 dx_rowblock  rg and the in_proj input-gradient product too           10 chain_bwd   LayerNorm2' .. out_proj' as one launch
 *    2 tw           weight gradients as one tile stream fed by the products 11 attn_tiles  prepare splits the fused attention's tiles
 *    3 panel        tiled GEMM family on its panel form                     12 afuse_fwd   in_proj + attention as one launch
 *    4 tw2          panel: tile stream fed by a conversion pass             13 afuse_bwd   attention' + in_proj' as one launch
 *    5 big          attention with materialised scores                      14 lean        the chains skip the fp32 FFN hidden and x1
 *    6 lnf1         out_proj with the add + LayerNorm epilogue              15 infer       the layer has an inference forward
 *    7 lnf2         linear2 with the add + LayerNorm epilogue               16 plan_ok     a token plan can run
 *    8 lnb          LayerNorm backward as the prologue of the next product
 * Returns RD_OK or the error of a bad shape. */
int rd_debug_encoder_route(const struct rd_shape* s, int32_t with_plan, uint32_t* bits);
/* The route one pass of the attention core over this shape takes (rd_attention.hip attn_route + attn_check, the functions
 * attn_forward / attn_backward call) in the current arithmetic mode and switches.  pass: 0 forward, 1 backward; with_plan: a token
 * plan is set; aligned: qkv, out and dout all start on 16-byte boundaries.  Needs no device.  Returns RD_OK, the error of a bad
 * shape, or what the pass refuses (words and names are filled in either way): a token plan outside the split-bf16 families, and the
 * materialised family, which only the layer runs.  The launch-log names go to name[cap], joined by ',', and
 *    words[0]  bits 0-1 family (0 exact-fp32 tiled, 1 single-tile split-bf16, 2 multi-tile split-bf16, 3 materialised scores), 2 vec
 *              (16-byte head-tile loads), 3 one_product, 4 wide (eight-wave single-tile form), 8-11 nth = ceil(head_dim / 16),
 *              12-13 nlaunch (0 materialised; 2: dq then dk / dv)
 *    words[1 + 5 i ..], launch i:  grid x, grid y, block, dynamic LDS bytes of the kernel's attribute, of the launch (0 past nlaunch) */
int rd_debug_attention_route(const struct rd_shape* s, int32_t pass, int32_t with_plan, int32_t aligned, uint32_t* words, char* name,
                             size_t cap);
/* The route one sensor-stage call of this shape takes (rd_k1_route.h k1_route) in the current arithmetic mode and switches.  ldz: row
 * stride of z / dz; with_pe: the call writes PE and the mask (rd_sensor_stage_fwd*; 0: rd_msgpass_fwd, rd_msgpass_bwd); with_coef:
 * a coefficient-dropout table is given.  Needs no device.  Bit i of *bits:
 *    0 fused         the LDS-resident kernels, else the tiled GEMM family    3 coef          the COEF instantiations
 *    1 specialised   the <3, 34, 60> instantiation, not <3, 0, 0>            4 tiles         generic: split weights, panel products
 *    2 infer         the shape has a save-free forward                       5 wgrad_stream  generic: weight gradients by tile stream
 * and in bits 8-9 rt, the row tiles ceil(F / 16) of a fused call (0 otherwise).  Returns RD_OK or the error of a bad shape. */
int rd_debug_sensor_route(const struct rd_shape* s, int32_t ldz, int32_t with_pe, int32_t with_coef, uint32_t* bits);
/* The route one use_beta graph-operator call (rd_graph_beta_fwd* / _bwd*) of these dimensions takes (rd_graph_beta.hip beta_fwd_route /
 * beta_bwd_route, the functions the launch sites call) at d_ob = 4, K = 4 T, under the RD_BETA_V1 / RD_BETA_LARGE settings of the
 * moment; with_alpha: the backward gets an alpha cotangent; with_drop: p_drop > 0.  Needs no device.  Bit i of *bits:
 *    0 fwd_lds   forward on the LDS-staged form, else the workspace form      2 stage_v   k_graph_beta_fwd2<true, .>: V staged in LDS
 *    1 bwd_lds   backward on the LDS-staged form                              3 v1        the rounds 2-5 kernels
 * and in bits 8-23 Tc, the steps per pass of an LDS-form backward (0 on the workspace form).  Returns RD_OK or the error of bad dims. */
int rd_debug_graph_beta_route(int32_t B, int32_t N, int32_t T, int32_t E, int32_t with_alpha, int32_t with_drop, uint32_t* bits);
/* The route one launch_gemm call takes (rd_gemm.hip gemm_check + gemm_route, the functions the launch calls) in the current arithmetic
 * mode and switches, for a product C[M,N] = A[M,K] B[N,K]^T described by value: the four operand strides, the split-K plan, tile_hint
 * and flags -- bit 0 a second problem (A2), 1 row sums, 2 batched, 3 scatter, 4 weight tiles given (Btiles), 5 A on a 16-byte
 * boundary, 6 token plan for the scatter.  Needs no device.  Returns RD_OK or gemm_check's error.  The launch-log name goes to
 * name[cap] ("" and all words 0 where nothing is launched: M or N <= 0), and
 *    words[0]  bits 0-1 family (1 k_gemm, 2 k_gemm_bf16x3, 3 k_gemm_panel*), 2 akc, 3 bkc, 4 one_product, 5-6 map (0 XCD round-robin,
 *              1 row-major, 2 split-K slice per XCD, 3 z grid), 8-11 npre, 12-15 tile (bf16x3: index into 64x64, 128x64, 128x128,
 *              64x128, 64x160; panel: 0 small, 1 wide, 2 pc)
 *    words[1..3]  the grid          words[4]  dynamic LDS bytes
 * rd_debug_splitk_plan: the split of a weight-gradient product's reduction (splitk_plan): returns nsplit, *k_per_split the slice. */
int rd_debug_gemm_route(int32_t M, int32_t N, int32_t K, int64_t sa_m, int64_t sa_k, int64_t sb_n, int64_t sb_k, int32_t nsplit,
                        int32_t k_per_split, int32_t tile_hint, uint32_t flags, uint32_t* words, char* name, size_t cap);
int rd_debug_splitk_plan(int64_t red, int32_t rows, int32_t cols, int32_t* k_per_split);
/* The route one fused-head call takes (rd_head.hip head_route, the function the launch site calls) under the RD_HEAD_NARROW /
 * RD_CODE_TOUCH settings of the moment.  mode: 0 rd_head_train (with_crit: rd_head_train_crit), 1 rd_head_forward, 2 rd_head_backward.
 * Needs no device.  Returns RD_OK or the error of sizes the head refuses.  The launch-log name of the k_head_rows instantiation goes
 * to name[cap] -- "k_head_rows<12,3>", "k_head_rows<16,4>", each also as "...,crit>" and (with_crit == 2: rd_head_train_focal)
 * "...,focal>" -- and
 *    words[0]  bit 0 narrow (W0 fetched as 192 x 192: <1, 12, 3>, else <1, 16, 4>), 1 crit, 2 emb_lds (static embedding staged in LDS,
 *              else read in place), 3 focal, bits 8-9 the weight-gradient jobs of the trailing launch (0: mode 1 has none)
 *    words[1]  own-code touch bytes        words[2]  workgroups of k_head_rows        words[3]  workgroups (tiles) of k_head_wgrad
 *    words[4]  1024-thread blocks of the deferred form (rd_set_defer_trailing)
 *    words[5 + j]  first tile blk0 of job j (d mlp_static[0], d mlp_static[2], d emb)   words[8 + j]  its tiles: n << 16 | k */
int rd_debug_head_route(int32_t mode, int32_t B, int32_t D, int32_t d_static, int32_t Fe, int32_t C, int32_t with_crit, uint32_t* words,
                        char* name, size_t cap);
/* The form one rd_fit_temperature call of [N, C] logits takes (rd_metrics_calib.hip fit_route, the function the launch site calls).
 * Needs no device.  Bit 0 of *bits: stage, the logits are copied into LDS once (else every evaluation re-reads global memory); bits
 * 8-31: the launch's dynamic LDS bytes (N C 4 when staged, else 0).  Returns RD_OK, or RD_EUNSUPPORTED outside the fit's envelope. */
int rd_debug_calibration_route(int64_t N, int32_t C, uint32_t* bits);
void rd_debug_set_calibration_stage(int on);         /* 0: rd_fit_temperature never stages (the route query follows); 1, the default: by the budget */

#ifdef __cplusplus
}
#endif
#endif /* RAINDROP_HIP_DEBUG_H */
