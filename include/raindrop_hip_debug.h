/*
 * raindrop_hip_debug.h -- profiling hooks of libraindrop_hip.so.  NOT part of the C-ABI (include/raindrop_hip.h): no host binding
 * in raindrop_amd/_lib.py, no stability promise; used by tools/*_timing.py and the tests only.  Each stamp setter registers (process-wide) a device
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
 * names so far, joined by '\n' and NUL-terminated, into out[cap] (whole names only) and returns the length all of them need. */
void rd_debug_launch_log(int on);
size_t rd_debug_launch_log_read(char* out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* RAINDROP_HIP_DEBUG_H */
