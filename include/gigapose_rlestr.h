/*
 * gigapose_rlestr.h -- C-ABI of libgigapose_rlestr.so: COCO COMPRESSED run-length strings decoded on MI355X (gfx950).
 * A `segmentation` whose `counts` is a string (every COCO-results json; pycocotools' mask.encode) goes to the GPU as its bytes;
 * one kernel turns it into the run list and the prefix sums that libgigapose_ingest.so (gigapose_ingest.h) crops and decodes
 * from.  Reference: rle_to_binary_mask per detection on the CPU (bop_toolkit's pycoco_utils, called at
 * src/dataloader/test.py:238).  This library is separate from the other four and links none of their objects.
 *
 * Conventions (those of gigapose_ingest.h)
 *   - every pointer is a DEVICE pointer; the caller owns all buffers, kernels never allocate; inputs are never modified
 *     (`counts` is in/out, see below);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous;
 *   - return value: 0 = ok, -1 = invalid argument, -2 = launch failure; gps_last_error() returns a thread-local message
 *     for the last failure;
 *   - err_flag: one int32 on the device, zeroed by the caller.  A bad detection d stores d + 1 there (if several are bad,
 *     one of them); the others are processed.
 *
 * Format.  A string codes the list of the uncompressed form (gigapose_ingest.h): lengths of alternating runs of 0 and 1 over
 * the mask flattened COLUMN-major, the first run is zeros and may be 0, the sum is H*W.
 *   - list position m carries x[m] = counts[m] for m <= 2 and x[m] = counts[m] - counts[m-2] for m >= 3 (x may be negative);
 *   - x is written as little-endian 5-bit groups, one per character: c = x & 0x1f; x >>= 5 (arithmetic); another group
 *     follows unless x == 0 and bit 0x10 of c is clear, or x == -1 and bit 0x10 of c is set; if one follows, c |= 0x20;
 *     the character is c + 48.  Valid characters are 48 .. 111; a value below 2^31 takes at most 7;
 *   - decoding: group k contributes (c & 0x1f) << 5k; the token ends at the first character whose 0x20 bit is clear; if
 *     that character has 0x10 set, the value is sign-extended from bit 5(k+1); then counts[m] = x[m] + counts[m-2], m >= 3.
 *     So counts[0] stands alone, the even positions >= 2 are a running sum of the even x, the odd positions of the odd x.
 *   Examples: [5, 3, 7, 1, 9, 40, 2] is "537N2W1I"; 15 is "?", 16 is "`0", -16 is "@", -17 is "_O", 2^31 - 1 is "oooooo1".
 * Limits: H*W < 2^31, total < 2^30, D <= 65535, n_bytes < 2^31.
 */
#ifndef GIGAPOSE_RLESTR_H
#define GIGAPOSE_RLESTR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gps_abi_version(void);
const char* gps_last_error(void);

/* Detection d owns the characters bytes[byte_offsets[d] .. byte_offsets[d+1]) and the list slots [offsets[d], offsets[d+1]) of
 * counts and cum (byte_offsets, offsets: i32[D+1]).  The caller sizes the slots: a string holds as many list entries as it has
 * characters with the 0x20 bit clear.
 *   - A detection WITH bytes: its slots of counts receive the decoded list, its slots of cum the inclusive prefix sums.
 *   - A detection with NO bytes (byte_offsets[d] == byte_offsets[d+1]) is an uncompressed one: its slots of counts already hold
 *     the list, which is only scanned.  One launch serves a mixed batch.
 * cum is bit for bit what gpi_rle_scan (gigapose_ingest.h) writes for the decoded list, the mark of a bad list (its last entry is
 * -1) and the flag included, so gpi_preprocess_detections_rle and gpi_rle_decode consume it unchanged.  One workgroup per
 * detection: any string length.
 * A detection is BAD when its slot slice is empty or leaves [0, total] (nothing is written), its byte slice leaves
 * [0, n_bytes], or, for a list, what gpi_rle_scan rejects; a string is bad when
 *   - a byte lies outside 48 .. 111, or the last byte has the 0x20 bit set (the string stops inside a token);
 *   - a token is longer than 7 characters;
 *   - it holds another number of tokens than offsets[d+1] - offsets[d];
 *   - a decoded count is negative or exceeds H*W, or the counts do not sum to H*W (all sums are 64-bit).
 * Of a bad string's slots only the mark cum[offsets[d+1] - 1] == -1 is specified.  Every index is bounded by the two slices,
 * never by what the bytes say. */
int gps_rle_string_scan(const uint8_t* bytes, const int* byte_offsets, int n_bytes, const int* offsets, int total, int D, int H, int W,
                        int* counts /* in/out */, int* cum, int* err_flag, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GIGAPOSE_RLESTR_H */
