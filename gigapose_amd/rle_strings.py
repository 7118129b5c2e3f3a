"""COCO COMPRESSED run-length masks in: a `segmentation` whose `counts` is a string -- what every COCO-results json holds, what
detectron2 / mmdet / ultralytics `save_json` and pycocotools' mask.encode write -- goes to the GPU as its bytes and is decoded there
(libgigapose_rlestr.so, C-ABI: include/gigapose_rlestr.h) into the run list and prefix sums the ingest kernels crop from.

The reference decodes such strings on the CPU, one detection at a time (bop_toolkit's pycoco_utils.rle_to_binary_mask, called at
src/dataloader/test.py:238).  `ingest.pack_rle` rejects them; this module is the route that takes them, next to ingest.py and
without changing it.

The coding: a string holds the list of the uncompressed form (ingest.py).  List position m carries x[m] = counts[m] for m <= 2 and
counts[m] - counts[m-2] for m >= 3; x is written as little-endian 5-bit groups, one per character c + 48, with bit 0x20 of c for
"another group follows" and bit 0x10 of the last group as the sign.  Valid characters are 48 .. 111; a value below 2^31 takes at
most 7.

  rle_string_from_counts(counts)      run lengths -> bytes            } the host codec, vectorised numpy
  rle_counts_from_string(s)           str / bytes -> int32 run lengths }
  mask_to_rle_string(mask)            (H,W) mask -> bytes
  pack_rle_any(segmentations, H, W)   list of {"counts": str | bytes | list, "size"} -> (bytes, byte_offsets, counts, offsets)
  StringRleDetectionPreprocessor      RleDetectionPreprocessor with (bytes, byte_offsets) next to (counts, offsets); same results
  CocoFrameIngest                     FrameIngest that accepts string, bytes and list counts, mixed within a batch
There is no CPU fallback: the kernel needs the GPU, a missing library is an error.
"""
import numpy as np
import torch

from . import _lib
from .ingest import FrameIngest, RleDetectionPreprocessor, host_batch, lay_pinned, mask_to_rle_counts
from .crop import CLIP_MEAN, CLIP_STD

MAX_TOKEN = 7                                         # characters of one value (35 bits)
_rlestr = _lib.SideLibrary("libgigapose_rlestr.so", "gps")
RLESTR_LIB_PATH, lib, _call = _rlestr.path, _rlestr.lib, _rlestr.call


# ------------------------------------------------------------------------------------------------ host side: the codec
def rle_string_from_counts(counts):
    """Run lengths -> the compressed string (bytes).  All values at once: the 7 possible groups of every x, then the length of
    every token, then the characters that exist, in order."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    if (c < 0).any() or (c >= 2 ** 31).any():
        raise ValueError("rle_string_from_counts: run lengths must lie in [0, 2^31)")
    x = c.copy()
    x[3:] -= c[1:-2]
    k = np.arange(MAX_TOKEN, dtype=np.int64)
    groups = (x[:, None] >> (5 * k)) & 0x1f                        # arithmetic shifts: numpy's >> on int64
    rest = x[:, None] >> (5 * (k + 1))
    more = np.where(groups & 0x10, rest != -1, rest != 0)
    length = more.argmin(axis=1) + 1                               # the first group after which nothing follows (|x| < 2^34: there is one)
    chars = (groups | np.where(more, 0x20, 0)) + 48
    return chars[k[None, :] < length[:, None]].astype(np.uint8).tobytes()


def _as_bytes(s, who):
    if isinstance(s, str):
        try:
            s = s.encode("ascii")
        except UnicodeEncodeError:
            raise ValueError(f"{who}: the string is not ASCII") from None
    b = np.frombuffer(bytes(s), np.uint8)
    if b.size == 0:
        raise ValueError(f"{who}: the string is empty")
    if (b > 127).any():
        raise ValueError(f"{who}: the string is not ASCII")
    return b


def rle_counts_from_string(s):
    """The compressed string (str or bytes) -> int32 run lengths.  Raises ValueError on a character outside 48 .. 111, a token of
    more than 7 characters, a string that stops inside a token and a run length outside [0, 2^31)."""
    b = _as_bytes(s, "rle_counts_from_string")
    if (b < 48).any() or (b > 111).any():
        raise ValueError("rle_counts_from_string: a character outside 48 .. 111")
    v = b.astype(np.int64) - 48
    last = (v & 0x20) == 0                                          # the characters that end a token
    if not last[-1]:
        raise ValueError("rle_counts_from_string: the string stops inside a token")
    ends = np.flatnonzero(last)
    starts = np.concatenate(([0], ends[:-1] + 1))
    token = np.cumsum(last) - last                                  # the token every character belongs to
    k = np.arange(b.size) - starts[token]                           # ... and its group number there
    if (k >= MAX_TOKEN).any():
        raise ValueError(f"rle_counts_from_string: a token of more than {MAX_TOKEN} characters")
    x = np.zeros(ends.size, np.int64)
    np.add.at(x, token, (v & 0x1f) << (5 * k))
    x -= np.where(v[ends] & 0x10, np.int64(1) << (5 * (k[ends] + 1)), 0)   # sign extension
    c = x.copy()
    c[1::2] = np.cumsum(x[1::2])                                    # odd positions: a running sum from m = 1
    c[2::2] = np.cumsum(x[2::2])                                    # even positions: one from m = 2; counts[0] stands alone
    if (c < 0).any() or (c >= 2 ** 31).any():
        raise ValueError("rle_counts_from_string: a decoded run length outside [0, 2^31)")
    return c.astype(np.int32)


def mask_to_rle_string(mask):
    """(H,W) array, non-zero = set -> the compressed string of its column-major run lengths (bytes)."""
    return rle_string_from_counts(mask_to_rle_counts(mask))


def pack_rle_any(segmentations, H, W):
    """List of {"counts", "size": [H, W]} whose counts are a str, bytes or an integer list (mixed within the batch) ->
    (bytes uint8[n_bytes], byte_offsets int32[D+1], counts int32[total], offsets int32[D+1]).  Detection d owns
    bytes[byte_offsets[d]:byte_offsets[d+1]] -- nothing when it came as a list -- and counts[offsets[d]:offsets[d+1]], filled for a
    list and zero for a string, whose slots the kernel fills: a string has one list entry per character with the 0x20 bit clear.
    Raises ValueError, naming the detection, on a size other than [H, W], an empty or non-ASCII string, a negative entry in a list or
    a list that does not sum to H*W (as pack_rle), and on the batch limits.  What a string holds is checked by the kernel."""
    H, W = int(H), int(W)
    if not (H > 0 and W > 0 and H * W < 2 ** 31):
        raise ValueError(f"pack_rle_any: frame size {H} x {W} is not supported (0 < H*W < 2^31)")
    strings, lists, is_string = [], [], []
    for d, seg in enumerate(segmentations):
        size, counts = list(seg["size"]), seg["counts"]
        if [int(s) for s in size] != [H, W]:
            raise ValueError(f"pack_rle_any: detection {d}: mask size {size} does not match the frame size [{H}, {W}]")
        if isinstance(counts, (str, bytes, bytearray)):
            strings.append(_as_bytes(counts, f"pack_rle_any: detection {d}"))
            is_string.append(True)
            continue
        c = np.asarray(counts, dtype=np.int64).reshape(-1)
        if (c < 0).any():
            raise ValueError(f"pack_rle_any: detection {d}: negative run length {int(c[c < 0][0])}")
        if int(c.sum()) != H * W:
            raise ValueError(f"pack_rle_any: detection {d}: the run lengths sum to {int(c.sum())}, not H*W = {H * W}")
        lists.append(c.astype(np.int32))
        is_string.append(False)
    is_string = np.asarray(is_string, bool)
    D = len(is_string)
    n_chars = np.zeros(D, np.int64)
    n_chars[is_string] = [len(s) for s in strings]
    byte_offsets = np.concatenate(([0], np.cumsum(n_chars)))
    if byte_offsets[-1] >= 2 ** 31:
        raise ValueError(f"pack_rle_any: {byte_offsets[-1]} string bytes in one batch (the limit is 2^31)")
    data = np.concatenate(strings) if strings else np.zeros(0, np.uint8)
    ends = np.concatenate(([0], np.cumsum(((data - 48) & 0x20) == 0)))     # one pass over all strings: the terminators before each byte
    n_slots = ends[byte_offsets[1:]] - ends[byte_offsets[:-1]]
    n_slots[~is_string] = [len(c) for c in lists]
    offsets = np.concatenate(([0], np.cumsum(n_slots)))
    if offsets[-1] >= 2 ** 30:
        raise ValueError(f"pack_rle_any: {offsets[-1]} runs in one batch (the limit is 2^30)")
    counts = np.zeros(int(offsets[-1]), np.int32)
    for d, c in zip(np.flatnonzero(~is_string), lists):
        counts[offsets[d]:offsets[d + 1]] = c
    return data, byte_offsets.astype(np.int32), counts, offsets.astype(np.int32)


# ------------------------------------------------------------------------------------------------ device side
class StringRleDetectionPreprocessor(RleDetectionPreprocessor):
    """frames uint8 (n_img,3,H,W) + what pack_rle_any returns + boxes / frame ids -> what RleDetectionPreprocessor returns for the
    decoded lists: {"tar_img", "tar_mask", "tar_M"}, bit for bit.  gps_rle_string_scan stands where gpi_rle_scan stood; the crop and
    the dense decoder are the ingest library's."""

    @torch.no_grad()
    def scan_strings(self, data, byte_offsets, counts, offsets, H, W, err):
        """bytes uint8[n_bytes], byte_offsets / offsets int32[D+1], counts int32[total] on the device -> cum int32[total]; the
        string detections' slots of `counts` receive their decoded lists (gps_rle_string_scan)."""
        cum = torch.empty_like(counts)
        _call("gps_rle_string_scan", data, byte_offsets, data.numel(), offsets, counts.numel(), offsets.numel() - 1, H, W, counts, cum, err, _lib.stream_ptr())
        return cum

    def _scan(self, lists, H, W, err):
        return self.scan_strings(*lists, H, W, err)

    def _inputs(self, data, byte_offsets, counts, offsets, dev, in_place=False):
        data = self._dev(data, dev, torch.uint8)
        byte_offsets = self._dev(byte_offsets, dev, torch.int32)
        own = self._dev(counts, dev, torch.int32)
        if own is counts and not in_place:                # the kernel writes the decoded lists there: not into the caller's tensor
            own = own.clone()
        offsets = self._dev(offsets, dev, torch.int32)
        assert data.dim() == 1 and own.dim() == 1 and offsets.dim() == 1 and byte_offsets.shape == offsets.shape
        return data, byte_offsets, own, offsets

    @torch.no_grad()
    def decode(self, data, byte_offsets, counts, offsets, H, W):
        """The dense masks (D,H,W) f32 the strings and lists encode (gps_rle_string_scan, then gpi_rle_decode)."""
        if not (isinstance(data, torch.Tensor) and data.is_cuda):
            raise _lib.GigaPoseHipError("StringRleDetectionPreprocessor.decode needs the strings on the GPU (no CPU fallback)")
        return self._decode((data, byte_offsets, counts, offsets), data.device, H, W)

    @torch.no_grad()
    def __call__(self, rgb_u8, data, byte_offsets, counts, offsets, xyxy_boxes, batch_im_id, in_place=False):
        """in_place: a `counts` tensor that already sits on the device receives the decoded lists instead of a copy of it."""
        return self._crop(rgb_u8, (data, byte_offsets, counts, offsets), xyxy_boxes, batch_im_id, in_place=in_place)


class CocoFrameIngest(FrameIngest):
    """FrameIngest whose detections' `segmentation["counts"]` may be a compressed string (str or bytes) or an integer list, mixed
    within a batch: same call, same PandasTensorCollection.  The string bytes travel in the same pinned staging buffer (one
    non-blocking copy); the list slots of the strings, which the kernel fills, do not travel at all.  The only host synchronisation
    is still the error-flag read."""

    def __init__(self, target_size=224, mean=CLIP_MEAN, std=CLIP_STD, device="cuda"):
        super().__init__(target_size, mean, std, device)
        self.preprocess = StringRleDetectionPreprocessor(target_size, mean, std)

    @staticmethod
    def stage(data, byte_offsets, counts, offsets, xyxy, im_id, K):
        """The pinned staging buffer [boxes i64 | offsets i32 | byte_offsets i32 | im_id i32 | K f32 | bytes u8 | pad | counts i32],
        the byte spans of its parts and the size of the DEVICE buffer it is copied to the front of.  Of `counts` only the head up
        to the end of the last list detection is staged; on the device the span runs on over all the slots, past the copy, where
        only strings own slots and the kernel writes them.  A batch of strings alone ships no list slot at all."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        byte_offsets = np.ascontiguousarray(byte_offsets, np.int32)
        counts = np.ascontiguousarray(counts, np.int32)
        is_list = np.flatnonzero(np.diff(byte_offsets) == 0)
        head = int(offsets[is_list[-1] + 1]) if is_list.size else 0
        data = np.ascontiguousarray(data, np.uint8)
        parts = [("boxes", np.ascontiguousarray(xyxy, np.int64)), ("offsets", offsets), ("byte_offsets", byte_offsets),
                 ("im_id", np.ascontiguousarray(im_id, np.int32)), ("K", np.ascontiguousarray(K, np.float32)), ("bytes", data),
                 ("pad", np.zeros(-data.size % 4, np.uint8)), ("counts", counts[:head])]
        buf, spans = lay_pinned(parts)
        a = spans["counts"][0]
        spans["counts"] = (a, a + counts.nbytes, counts.shape)
        return buf, spans, max(a + counts.nbytes, 1)

    def _preprocess(self, frames, part, boxes, im):
        return self.preprocess(frames, part("bytes", torch.uint8), part("byte_offsets", torch.int32), part("counts", torch.int32),
                               part("offsets", torch.int32), boxes, im, in_place=True)

    @torch.no_grad()
    def __call__(self, frames_u8, K, infos, detections, test_list=None, label_map=None):
        frames_u8, K, H, W = self._frames(frames_u8, K, detections)
        if len(infos) != len(detections):
            raise ValueError(f"CocoFrameIngest: {len(infos)} image infos for {len(detections)} detection lists")
        data, byte_offsets, counts, offsets = pack_rle_any([det["segmentation"] for dets in detections for det in dets], H, W)
        # boxes, frame ids and the infos rows are host_batch's; it gets a one-run list in place of every mask, which it only packs
        blank = dict(counts=[H * W], size=[H, W])
        _, _, xyxy, im_id, frame = host_batch(infos, [[dict(det, segmentation=blank) for det in dets] for dets in detections], H, W, label_map)
        if len(im_id) == 0:
            return self._empty(frame, test_list)
        buf, spans, device_bytes = self.stage(data, byte_offsets, counts, offsets, xyxy, im_id, K)
        dbuf = torch.empty(device_bytes, dtype=torch.uint8, device=self.device)
        dbuf[:buf.numel()].copy_(buf, non_blocking=True)
        return self._finish(dbuf, spans, frame, frames_u8.to(self.device, non_blocking=True), test_list)
