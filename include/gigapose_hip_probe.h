/*
 * gigapose_hip_probe.h -- what libgigapose_hip_probe.so exports ON TOP of gigapose_hip.h: the same sources compiled with -DGP_PROBES
 * (gigapose_amd/csrc/Makefile).  Nothing here is part of the product: these are the A/B switches behind the bit-identity tests (a
 * variant on / off must give equal bits), time-stamped probe builds of the hot kernels (tools/probe_*.py), test-only epilogues and the
 * readers of the stream-K scratch's error word.  All switches are PROCESS-GLOBAL and not thread-safe: set, measure, reset.
 * Python: `with _lib.probe_library(): ...` (gigapose_amd/_lib.py) routes the calls of a block to this library.
 */
#ifndef GIGAPOSE_HIP_PROBE_H
#define GIGAPOSE_HIP_PROBE_H
#include "gigapose_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- matcher ---- */
/* probe build of gp_match_tiles_split_dir (two-plane bank, tar2src) writing 8 time stamps per tile, see gp_match.hip */
int gp_match_tiles_split_trace(const void* q_hi, const void* q_lo, const void* b_hi, const void* b_lo, const float* qmask,
                               const float* bmask, const int* labels, int B, int O, int N, int C, float sim_threshold,
                               float patch_threshold, uint8_t* idx_t2s, float* score_t2s, float* mask_all, float* sim_avg,
                               unsigned long long* trace, void* stream);
/* 1 (default) = tiles are built from the live (mask != 0) patches only, per-wave rectangles of 32 x 32 blocks; 0 = every patch counts
 * as live (the full 2 x 4 per wave).  Outputs are bit-identical. */
int gp_match_split_set_compact(int on);

/* ---- f32 (chain) GEMM ---- */
void gp_gemm_set_streamk(int mode); /* 0 = one workgroup per tile even with a scratch, 1 = by the built-in rule (default), 2 = split
                                       whenever the tile count allows (results identical) */
void gp_gemm_set_group(int g);      /* tiles are ordered in bands of g i-tiles (default 8; results identical) */
int gp_gemm_streamk_error(const float* scratch, void* stream);  /* synchronises; the scratch's error word (0 = every hand-off arrived) */

/* ---- split GEMMs ---- */
int gp_gemm_split_set_trace(unsigned long long* dev_buf);
int gp_gemm_split_timing(const float* act, int ld_act, const void* whi, const void* wlo, float* D, int ldd, int I, int J, int K,
                         unsigned long long* out20 /* 23 entries */, void* stream);
int gp_gemm_split256_error(const float* scratch, void* stream); /* scratch error word of gp_gemm_split256 / gp_gemm_planes256_scaled */
/* gemm_planes256_kernel: bit 0 (default 1): data-parallel rounds before the stream-K remainder; bit 1: TEST hook, head fragments are
 * never published (every waiter times out -> GP_STATUS_HANDOFF_SPLIT) */
int gp_gemm_planes256_set_dp(int mode);
/* default 1: shapes with 8 <= tiles < 256 (ViT-L below 64 crops) run with the slots of a tile splitting its K in parallel; 0: such
 * shapes are refused and the ViT falls back to the 128 x 128 kernels; n >= 2: at least n k-steps per slot of a split tile */
int gp_gemm_planes256_set_par(int on);
/* default 1: launches whose 256 x 256 tiles fill at most half of the 256 slots run on 256 x 128 tiles; 0: always 256 x 256 */
int gp_gemm_planes256_set_half_tiles(int on);
/* gp_gemm_planes256_scaled (epilogues 0, 3, 6, 7; plane scale 8) from a build with per-slot time stamps, see gp_split256.hip */
int gp_gemm_planes256_trace(const void* a_hi, const void* a_lo, const void* b_hi, const void* b_lo, float* D, int ldd, void* out_hi,
                            void* out_lo, int ldo, int I, int J, int J_valid, int K, int epilogue, const float* bias, const float* scale,
                            const float* residual, int ldr, float out_scale, float* scratch, unsigned long long* trace, void* stream);
int gp_gemm_planes256_timing(const void* a_hi, const void* a_lo, const void* b_hi, const void* b_lo, float* D, int ldd, int I, int J,
                             int K, float* scratch, unsigned long long* out8, void* stream);

/* ---- ViT ---- */
void gp_vit_set_ln_reg(int mode); /* plane path's LayerNorm: 1 (default) 32-token blocks, 16-token blocks when the launch has at most 128 of
                                     them; 2 always 32-token blocks; 0 the first-generation three-pass kernel (results identical) */
void gp_vit_set_ln_live(int tokens); /* gp_layernorm_planes: only rows < tokens carry tokens, as in the forward (B * 257 of Mpad): blocks of
                                        pure row padding do not run (those plane rows are zeroed), and 32-token blocks past a whole number of
                                        resident rounds are folded into first-round blocks; <= 0 (default): all Mpad rows */
void gp_vit_set_planes(int on);   /* split numerics: 1 (default; any value but 0) = activation planes + attention in split numerics where the
                                     shapes allow, 0 = f32 activations and the lock-step kernels */
/* Stage entries of the f32 kernels gp_vit_forward runs whenever the plane path is not taken (chain numerics, ViT-S, ViT-L below 8 crops,
 * the fall-back after a range trip); the feature epilogue runs on every forward.  Each launches through the launcher the forward uses
 * (tests/test_gpu_vit_f32_stages.py; the product library's kernels are tied to these by a bit-exact composition test).
 * Token b*257 + t is column (row of vt) b*257 + t; Mpad = round_up(257 B, 256) in the forward.
 *   gp_vit_attention_f32  softmax(q k^T / 8) v per (crop, head), HF modeling_dinov2.py:207-229.  qk [2 dim][Mpad]: Q in rows h*64 + d, K in
 *                         rows dim + h*64 + d; vt [Mpad][dim]; out [dim][Mpad].  Requires dim == 64 heads, Mpad % 256 == 0, Mpad >= 257 B.
 *                         Columns / rows from 257 B on are neither read nor written.
 *   gp_vit_layernorm_f32  LayerNorm over C of X [C][Mpad] -> Y [C][Mpad] (norm1 / norm2, :342-380).  Requires C % 16 == 0, Mpad % 64 == 0.
 *   gp_vit_features       X [C][Mpad] -> out (B, C, 256): the patch tokens (t >= 1) of every crop, divided by max(|x|_2, 1e-12) over C if
 *                         normalize != 0 (ae_net.py:64-69).  The class-token column and the pad columns are not read.  The finiteness guard
 *                         (GP_STATUS_SPLIT_RANGE on a token with a NaN / inf or sum x^2 > 3e38) belongs to the normalisation: with
 *                         normalize == 0 the values are copied as they are and no bit is raised. */
int gp_vit_attention_f32(const float* qk, const float* vt, float* out, int B, int heads, int dim, int Mpad, void* stream);
int gp_vit_layernorm_f32(const float* X, float* Y, const float* gamma, const float* beta, int C, int Mpad, float eps, void* stream);
int gp_vit_features(const float* X, float* out, int B, int C, int Mpad, int normalize, void* stream);

/* ---- IST convolutions ---- */
void gp_conv_set_direct(int on);                                  /* 0 = always the generic gather kernel (results identical) */
void gp_conv2d_planes_set_trace(unsigned long long* device_buf);  /* per slot segments / k-steps / ticks, NULL = off */
/* 1 (default) = 3 x 3 / stride 1 layers take conv_halo_kernel and its parallel split below 256 tiles; 0 = neither; 5 = halo without the
 * parallel split; 1 + 16 n: at least n channel blocks per slot of a split tile */
int gp_conv2d_planes_set_halo(int on);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_HIP_PROBE_H */
