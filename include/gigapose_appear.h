/*
 * gigapose_appear.h -- C-ABI of libgigapose_appear.so: the appearance score of a mask proposal on MI355X (gfx950), the patch-level
 * companion of the class-token score of libgigapose_label.so.  CNOS's successors (the instance segmentation stage of SAM-6D) take,
 * for every foreground patch of a proposal's crop, its best cosine match among the foreground patches of the object's best
 * template, and average the matches.  Three stages: the 256 patch tokens of a DINOv2 ViT after the final LayerNorm, L2-normalised,
 * quantised and split into three int8 limbs (gpp_patch_descriptors); which of the 16 x 16 patches of a crop lie on its mask
 * (gpp_patch_valid); and per (proposal, template) pair the 256 x 256 x C exact products on the int8 matrix cores, the masked
 * maximum over the template's patches and the sum over the proposal's (gpp_appearance).  Nothing of the reference is restated: it
 * holds no such stage, the definitions below ARE the contract.  This library links no object of the other libraries.
 *
 * Conventions (those of gigapose_label.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gpp_last_error() returns a thread-local message
 *     for the last failure.  An invalid argument is refused before anything is launched.
 *
 * THE ARITHMETIC IS THE CONTRACT (gigapose_testing/appear_ref.py restates it in numpy and Python integers and must agree bit for
 * bit).  Every DECISION -- which template patch a proposal's patch matches, which patches count -- is taken on integers, so no
 * result depends on how the work is spread over threads, waves and workgroups or on the order in which they finish.  The one
 * floating-point stage (gpp_patch_descriptors) is IEEE float64 in a summation order fixed below, one rounding per written
 * operation, no fused multiply-add (the library is built with -ffp-contract=off) except inside the correctly rounded square root
 * (gigapose_dist.h states its construction; numpy.sqrt returns the same bits); `/` is the correctly rounded float64 division.
 */
#ifndef GIGAPOSE_APPEAR_H
#define GIGAPOSE_APPEAR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gpp_abi_version(void);
const char* gpp_last_error(void);

#define GPP_PATCHES 256 /* a crop's 16 x 16 grid of patches, patch n = 16 * row + column */
#define GPP_CELL 14     /* a patch covers 14 x 14 pixels of the 224 x 224 crop */
#define GPP_Q_BITS 20   /* a component d in [-1, 1] is the integer q = rint(d * 2^20) (ties to even), in [-2^20, 2^20] */
#define GPP_MAX_C 2048  /* C is a multiple of 64, 64 <= C <= 2048 */
#define GPP_MAX_ROWS 1048576 /* crops or bank rows (templates) of one call */
#define GPP_MAX_PAIRS 65535

/* status bits of gpp_patch_descriptors (per token) */
#define GPP_NON_FINITE 1 /* a value of the token is NaN or infinite, or the squared norm is */
#define GPP_ZERO_NORM 2  /* the normalised token is all zeros (a constant token with beta = 0) */
/* status bits of gpp_appearance (per pair) */
#define GPP_BAD_INDEX 1         /* qi or ti lies outside its array */
#define GPP_NO_QUERY_PATCH 2    /* the query crop has no valid patch */
#define GPP_NO_TEMPLATE_PATCH 4 /* the template has no valid patch */

/* The limbs.  q is never stored: a component is written as its three balanced base-128 digits, one int8 plane each,
 *     a0 = ((q + 64) mod 128) - 64;   q1 = (q - a0) / 128;   a1 = ((q1 + 64) mod 128) - 64;   a2 = (q1 - a1) / 128
 * (mod with a result in [0, 127]; both divisions are exact), so that q = a0 + 128 * a1 + 16384 * a2 with a0, a1 in [-64, 63] and
 * a2 in [-64, 64] (q = 2^20 is 0, 0, 64).  Limb plane u of B crops is the int8 tensor (B, 256, C); the three planes follow each
 * other: (3, B, 256, C). */

/* The patch descriptors of B crops.
 *   x f32: value c of patch n of crop b is x[b * crop_stride + n * token_stride + c * channel_stride] (strides in ELEMENTS, all
 *   > 0).  The contiguous (B, 257, C) tensor, passed one token in (x + C), has strides (257 * C, C, 1); the ViT workspace's
 *   channel-major view (C, mpad), passed one element in (x + 1), has (257, 1, mpad): either way the class token is skipped, and
 *   nothing but these B * 256 * C values is read.  gamma, beta f32 (C): the final LayerNorm's weight and bias; eps its epsilon.
 *   ->  a (3, B, 256, C) int8, 16-byte aligned;  status (B, 256) int32.
 *   B >= 0 (B = 0 is a no-op after the checks), B <= 2^20, C a multiple of 64, 64 <= C <= 2048.
 * SUM(v) = (S0 + S1) + (S2 + S3), where S_j starts at +0.0 and adds v[c] for c = j, j + 4, j + 8, .. < C in that order.  Per
 * token, with every f32 widened to float64 first (the formulas are gpa_descriptors's, the summation order is this library's):
 *     mean = SUM(x) / C;   dev[c] = x[c] - mean;   var = SUM(dev * dev) / C;   r = 1 / root(var + eps)
 *     y[c] = (dev[c] * r) * gamma[c] + beta[c];     n2 = SUM(y * y);   norm = root(n2)
 *     q[c] = (int) rint((y[c] / norm) * 2^20)       and its limbs as above
 * status = GPP_NON_FINITE when an x[c] is not finite or n2 is not finite; else GPP_ZERO_NORM when n2 == 0; else 0.  The limbs of
 * a flagged token are all 0.
 * Shape: a workgroup of 256 threads takes 64 tokens; lane l of wave j keeps chain S_j of token l, the four chains meet in LDS in
 * the order written above; in the channel-major layout a wave's loads are 64 consecutive tokens. */
int gpp_patch_descriptors(const float* x, long long crop_stride, long long token_stride, long long channel_stride, const float* gamma,
                          const float* beta, double eps, int B, int C, signed char* a, int* status, void* stream);

/* Which patches of B crops lie on the crop's mask.
 *   mask f32 (B, 224, 224): pixel (y, x) is SET iff its value > 0.5f (a NaN is not set); it belongs to patch
 *   n = 16 * (y / 14) + (x / 14);  num / den: the occupancy a patch must EXCEED, 0 <= num <= den <= 2^16, den >= 1
 *   ->  valid (B, 256) u8: 1 iff  set * den > num * 196  (integers, STRICT; set = the patch's number of set pixels), else 0;
 *       count (B) int32: the number of valid patches;   set (B, 256) u8 or NULL: the counts themselves, 0 .. 196.
 *   0 <= B <= 2^20 (B = 0 is a no-op after the checks).  One workgroup per crop, a thread per patch. */
int gpp_patch_valid(const float* mask, int B, int num, int den, unsigned char* valid, int* count, unsigned char* set, void* stream);

/* The appearance sums of P (query crop, bank row) pairs.
 *   qa (3, Bq, 256, C) int8, q_valid (Bq, 256) u8: the limbs and valid patches of the query crops;
 *   ta (3, R, 256, C) int8, t_valid (R, 256) u8: those of the bank's rows (one row per template); both limb tensors 16-byte
 *   aligned, every limb within the ranges above (the caller's duty: see the bound below); a patch is valid iff its byte is not 0;
 *   qi, ti int32 (P): pair p is query crop qi[p] against bank row ti[p].
 * With q[., c] = a0 + 128 * a1 + 16384 * a2 of either side,
 *     dot[i, j] = sum over c of q_query[i, c] * q_bank[j, c]                 exact, |dot| <= C * 2^40 < 2^52
 * (for ANY limbs within their ranges |q| <= 64 + 64 * 128 + 64 * 16384 = 1056832, and |dot| <= 2048 * 1056832^2 < 2^52 still).
 * For every VALID query patch i:  best[i] = the largest dot[i, j] over the VALID template patches j, arg[i] = the FIRST j that
 * attains it.
 *   ->  sum (P) int64, 8-byte aligned: the sum of best[i] over the valid i;   n (P) int32: the number of valid i (the float score
 *       is sum / (n * 2^40), one correctly rounded division, taken on the host);
 *       best (P, 256) int64 (8-byte aligned) or NULL, arg (P, 256) int32 or NULL: an invalid i gets best = 0 and arg = -1;
 *       status (P) int32: GPP_BAD_INDEX when not (0 <= qi[p] < Bq and 0 <= ti[p] < R), and nothing is read for the pair; else
 *       GPP_NO_QUERY_PATCH when the crop has no valid patch, | GPP_NO_TEMPLATE_PATCH when the row has none.  A flagged pair gets
 *       sum = 0, n = 0, best = 0, arg = -1 and touches nothing of its neighbours.
 * Limits: 0 <= P <= 65535 (P = 0 is a no-op after the checks), 1 <= Bq, R <= 2^20, C a multiple of 64, 64 <= C <= 2048.
 *
 * How the sum stays exact on the matrix cores.  q_query * q_bank = sum over u, v of 128^(u + v) * a_u * b_v, so with
 *     s_w[i, j] = sum over c and over the limb pairs (u, v) with u + v = w of a_u[i, c] * b_v[j, c]          (w = 0 .. 4)
 *     dot = s0 + (s1 << 7) + (s2 << 14) + (s3 << 21) + (s4 << 28)                                             (int64)
 * Each s_w is an int32 accumulator of v_mfma_i32_16x16x64_i8: nine limb products per 64 channels, products of equal weight
 * sharing an accumulator.  A product of two limbs is at most 64 * 64 = 4096 in magnitude, an accumulator sums at most 3 limb pairs
 * (w = 2) over at most 2048 channels: |s_w| <= 3 * 4096 * 2048 = 3 * 2^23 < 2^31.  It cannot wrap, and integer addition being
 * associative, the order in which the matrix core adds the 64 products of a step cannot matter.
 * The maximum and the first-j rule are ONE unsigned 64-bit maximum of the key ((dot + 2^52) << 8) | (255 - j) of the valid j
 * (dot + 2^52 is in [1, 2^53), so a key is in [256, 2^61); 0 stands for "no valid j"): the reduction needs no tie handling and
 * its order cannot matter.  The sums of the four 64-patch strips of a pair meet in sum[p] by an integer atomic add, whose order
 * cannot matter either.
 * Shape: pair_kernel, one workgroup per pair, writes status, n and sum = 0; strip_kernel, grid (4 strips of 64 query patches, P),
 * four waves, wave w takes the template's patch tiles w, w + 4, w + 8, w + 12 against the strip's four query tiles: the bank is
 * operand A (rows j), the query operand B (columns i), so that a lane meets the j's of ONE i and keeps a running maximum. */
int gpp_appearance(const signed char* qa, const unsigned char* q_valid, int Bq, const signed char* ta, const unsigned char* t_valid, int R,
                   int C, const int* qi, const int* ti, int P, long long* sum, int* n, int* status, long long* best, int* arg,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_APPEAR_H */
