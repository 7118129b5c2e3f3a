"""GPU: COCO compressed run-length strings decoded on the device (libgigapose_rlestr.so, gigapose_amd/rle_strings.py).

gps_rle_string_scan against the sequential decoder (gigapose_testing/rle_string_ref.py) for the lists and, bit for bit, against
gpi_rle_scan of the decoded lists for the prefix sums; mixed string / list batches; every class of malformed string (flagged,
marked, its crop untouched, its neighbours right); the routes StringRleDetectionPreprocessor == RleDetectionPreprocessor == dense
and the reference golden; CocoFrameIngest -> GigaPose.test_step against FrameIngest on the equivalent lists."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dropin_flow as df
import test_gpu_ingest as tgi
from gigapose_testing import rle_string_ref as ref
from gigapose_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 46340                                        # 46340^2 < 2^31: [H*W] and [1, H*W - 1] are legal, no dense buffer is made


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def layout(items):
    """items: per detection bytes (a string), an integer array (a list) or (bytes, n_slots) to force another slot count than the
    string's terminators -> (bytes, byte_offsets, counts, offsets) as pack_rle_any lays them out, without its checks."""
    data, byte_offsets, counts, offsets = [], [0], [], [0]
    for it in items:
        n_slots = None
        if isinstance(it, tuple):
            it, n_slots = it
        if isinstance(it, bytes):
            b = np.frombuffer(it, np.uint8)
            data.append(b)
            byte_offsets.append(byte_offsets[-1] + len(b))
            n = int(((((b.astype(np.int64) - 48) & 0x20) == 0).sum())) if n_slots is None else n_slots
            counts.append(np.zeros(n, np.int32))
        else:
            byte_offsets.append(byte_offsets[-1])
            counts.append(np.asarray(it, np.int64).astype(np.int32))
        offsets.append(offsets[-1] + len(counts[-1]))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return cat(data, np.uint8), np.asarray(byte_offsets, np.int32), cat(counts, np.int32), np.asarray(offsets, np.int32)


def string_scan(data, byte_offsets, counts, offsets, H, W):
    """gps_rle_string_scan through the C-ABI -> (flag, counts after the call, cum); cum is pre-filled with -77."""
    from gigapose_amd import _lib
    from gigapose_amd import rle_strings as rs

    d_data, d_bo, d_counts, d_off = _t(data), _t(byte_offsets), _t(counts), _t(offsets)
    cum = torch.full_like(d_counts, -77)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = rs.lib().gps_rle_string_scan(_lib.ptr(d_data), _lib.ptr(d_bo), _lib.i(len(data)), _lib.ptr(d_off), _lib.i(len(counts)),
                                      _lib.i(len(offsets) - 1), _lib.i(H), _lib.i(W), _lib.ptr(d_counts), _lib.ptr(cum), _lib.ptr(err),
                                      _lib.stream_ptr())
    assert rc == 0, rs.lib().gps_last_error()
    return int(err.item()), d_counts.cpu().numpy(), cum


def list_scan(lists, H, W):
    """gpi_rle_scan of the uncompressed lists -> (flag, cum, offsets); cum is pre-filled with -77 as above."""
    from gigapose_amd import _lib, ingest

    offsets = np.concatenate(([0], np.cumsum([len(c) for c in lists]))).astype(np.int32)
    counts = np.concatenate([np.asarray(c, np.int64) for c in lists]).astype(np.int32)
    d_counts, d_off = _t(counts), _t(offsets)
    cum = torch.full_like(d_counts, -77)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rc = ingest.lib().gpi_rle_scan(_lib.ptr(d_counts), _lib.ptr(d_off), _lib.i(len(counts)), _lib.i(len(lists)), _lib.i(H), _lib.i(W),
                                   _lib.ptr(cum), _lib.ptr(err), _lib.stream_ptr())
    assert rc == 0
    return int(err.item()), cum.cpu().numpy(), offsets


def check_against_the_list_scan(lists, H, W, as_list=()):
    """The lists, coded as strings by the sequential encoder (those in `as_list` stay lists), in ONE launch: the decoded counts equal
    the sequential decoder's, cum equals gpi_rle_scan's of the all-list batch, bit for bit."""
    strings = [ref.encode_counts(c) for c in lists]
    for c, s in zip(lists, strings):
        assert int(np.sum(np.asarray(c, np.int64))) == H * W
        np.testing.assert_array_equal(ref.decode_counts(s), np.asarray(c, np.int64))
    items = [np.asarray(c) if d in as_list else s for d, (c, s) in enumerate(zip(lists, strings))]
    data, byte_offsets, counts, offsets = layout(items)
    flag, got_counts, got_cum = string_scan(data, byte_offsets, counts, offsets, H, W)
    ref_flag, ref_cum, ref_offsets = list_scan(lists, H, W)
    assert flag == 0 and ref_flag == 0
    np.testing.assert_array_equal(offsets, ref_offsets)
    for d, c in enumerate(lists):
        np.testing.assert_array_equal(got_counts[offsets[d]:offsets[d + 1]], np.asarray(c, np.int64), err_msg=f"detection {d}")
    got_cum = got_cum.cpu().numpy()
    assert got_cum.dtype == ref_cum.dtype == np.int32
    np.testing.assert_array_equal(got_cum, ref_cum)
    return strings


# ------------------------------------------------------------------------------------------------ decode against the list scan
def test_short_lists_zero_first_run_negative_deltas_and_every_token_length():
    HW = BIG * BIG
    ladder = [5, 100, 5000, 100100, 5005000, 300100100]             # deltas of 1 .. 6 characters; the rest takes 7
    ladder.append(HW - sum(ladder))
    lists = [[HW], [1, HW - 1], [7, HW - 10, 3], [7, 9, HW - 20, 4], [7, 9, 11, HW - 40, 13],    # 1 .. 5 tokens: the delta rule starts at the 4th
             [0, HW], [0, 3, HW - 3],                                                          # a zero first run
             [10, 2147000000, 20, 5, 30, HW - 2147000065],                                      # x[3] = 5 - 2147000000
             ladder, ladder[::-1]]
    strings = check_against_the_list_scan(lists, BIG, BIG)
    lengths = {(len(ref.encode_value(x)), x < 0) for s in strings for x in ref.decode_values(s)}
    assert {n for n, _ in lengths} == {1, 2, 3, 4, 5, 6, 7}
    assert {n for n, neg in lengths if neg} >= {3, 4, 5, 6, 7}      # the reversed ladder: negative tokens of every longer length
    assert min(x for s in strings for x in ref.decode_values(s)) < -2 ** 30


def test_random_mask_and_multi_byte_tokens_at_every_byte_alignment():
    from gigapose_amd import ingest

    H, W = 37, 53
    rng = np.random.RandomState(41)
    lists = [ingest.mask_to_rle_counts(rng.rand(H, W) < 0.5)]
    for k in range(8):                                               # k one-byte tokens, then tokens of 2 and 3 characters
        tail = [200, 300, 150 + k, 420, 17, 333]
        lists.append([1] * k + tail + [H * W - k - sum(tail)])
    strings = check_against_the_list_scan(lists, H, W)
    for k in range(8):
        s = strings[1 + k]
        assert [len(ref.encode_value(x)) for x in ref.decode_values(s)[:k + 1]] == [1] * k + [2]
        check_against_the_list_scan([lists[1 + k]], H, W)            # alone: its bytes start at the buffer's aligned base
    check_against_the_list_scan(lists[::-1], H, W)


def test_noise_mask_of_150k_tokens_straddles_every_chunk_of_both_passes():
    from gigapose_amd import ingest
    from gigapose_amd import rle_strings as rs

    H, W = 480, 640
    rng = np.random.RandomState(43)
    noise = ingest.mask_to_rle_counts(rng.rand(H, W) < 0.5)
    assert len(noise) > 140000                                       # > 2048 bytes and > 1024 tokens per chunk, many times over
    small = ingest.mask_to_rle_counts(syn.detection_case(seed=44, n_img=1, D=1, H=H, W=W)["masks"][0])
    strings = check_against_the_list_scan([small, noise, small], H, W)
    assert strings[1] == rs.mask_to_rle_string(np.random.RandomState(43).rand(H, W) < 0.5)      # the vectorised host encoder, same mask
    assert len(strings[1]) < 2 * len(noise)                         # about one character per run: a quarter of the int32 list


def test_uncompressed_lists_get_the_same_cum_and_flag_from_both_scans_at_the_chunk_and_thread_boundaries():
    """The same uncompressed lists through gpi_rle_scan and through gps_rle_string_scan with an empty byte slice for every
    detection, one launch per route: the shared scan (csrc/gp_rle_scan.h) at lengths that straddle its 1024-count chunk and its
    4-count thread, and a bad list (total H*W + 1) that both routes flag and mark."""
    H, W = 48, 64
    HW = H * W
    lengths = [1, 4, 1023, 1024, 1025, 2048, 2049]
    lists = [[1] * (L - 1) + [HW - (L - 1)] for L in lengths]
    lists.append([1] * 1024 + [HW + 1 - 1024])                       # 1025 counts that sum to H*W + 1
    bad = len(lists) - 1
    assert all(sum(c) == HW for c in lists[:bad]) and sum(lists[bad]) == HW + 1 and len(lists[bad]) == 1025
    data, byte_offsets, counts, offsets = layout([np.asarray(c) for c in lists])
    assert len(data) == 0 and not byte_offsets.any()
    flag, got_counts, got_cum = string_scan(data, byte_offsets, counts, offsets, H, W)
    ref_flag, ref_cum, ref_offsets = list_scan(lists, H, W)
    np.testing.assert_array_equal(offsets, ref_offsets)
    assert flag == ref_flag == bad + 1
    np.testing.assert_array_equal(got_counts, counts)                # a list's slots are read, not written
    got_cum = got_cum.cpu().numpy()
    assert got_cum.dtype == ref_cum.dtype == np.int32
    np.testing.assert_array_equal(got_cum, ref_cum)
    assert got_cum[offsets[bad + 1] - 1] == -1 and ref_cum[offsets[bad + 1] - 1] == -1
    for d, c in enumerate(lists[:bad]):                              # and the valid ones are the prefix sums
        np.testing.assert_array_equal(ref_cum[offsets[d]:offsets[d + 1]], np.cumsum(c), err_msg=f"detection {d}")


def test_mixed_batch_of_strings_and_lists_in_one_launch():
    from gigapose_amd import ingest

    H, W = 97, 131
    case = syn.detection_case(seed=45, n_img=1, D=5, H=H, W=W)
    rng = np.random.RandomState(46)
    masks = np.logical_xor(case["masks"] != 0, rng.rand(5, H, W) < 0.1)
    lists = [ingest.mask_to_rle_counts(m) for m in masks]
    check_against_the_list_scan(lists, H, W, as_list=(1, 4))         # string, list, string, string, list
    check_against_the_list_scan(lists, H, W, as_list=(0, 1, 2, 3, 4))


# ------------------------------------------------------------------------------------------------ malformed strings
def crop_after_scan(case, cum, offsets, total, H, W, T, sentinel):
    """gpi_preprocess_detections_rle on sentinel-filled outputs -> (crop flag, outputs)."""
    from gigapose_amd import _lib, ingest
    from gigapose_amd.crop import CLIP_MEAN, CLIP_STD

    D, n_img = len(offsets) - 1, case["rgb"].shape[0]
    out = dict(tar_img=torch.full((D, 3, T, T), sentinel, device=DEV), tar_mask=torch.full((D, T, T), sentinel, device=DEV),
               tar_M=torch.full((D, 3, 3), sentinel, device=DEV))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    mean, std = (ctypes.c_float * 3)(*CLIP_MEAN), (ctypes.c_float * 3)(*CLIP_STD)
    d_rgb, d_off, d_boxes, d_im = _t(case["rgb"]), _t(offsets), _t(case["boxes"]), _t(case["im_id"])
    rc = ingest.lib().gpi_preprocess_detections_rle(_lib.ptr(d_rgb), _lib.ptr(cum), _lib.ptr(d_off), _lib.i(total), _lib.ptr(d_boxes),
                                                    _lib.ptr(d_im), _lib.i(n_img), _lib.i(D), _lib.i(H), _lib.i(W), _lib.i(T), mean, std,
                                                    _lib.ptr(out["tar_img"]), _lib.ptr(out["tar_mask"]), _lib.ptr(out["tar_M"]),
                                                    _lib.ptr(err), _lib.stream_ptr())
    assert rc == 0
    return int(err.item()), out


def malformed(good, lst, HW):
    """Every class of bad string, made from a good string and its list: name -> bytes or (bytes, forced slot count)."""
    n = len(lst)
    assert n >= 3 and len(good) > 6
    with_negative = list(lst)
    with_negative[1] += with_negative[2] + 1
    with_negative[2] = -1                                            # a negative count, the total still H*W
    assert sum(with_negative) == HW
    short = list(lst)
    short[1] -= 1                                                    # total H*W - 1
    first = int(lst[0])
    groups = [(first >> (5 * k)) & 0x1f for k in range(8)]           # lst[0] in EIGHT characters: right value, one character too many
    long_token = bytes([g + 0x20 + 48 for g in groups[:7]] + [groups[7] + 48])
    assert first < 2 ** 34 and ref.encode_value(first) == good[:len(ref.encode_value(first))]
    rest = good[len(ref.encode_value(first)):]
    return {
        "byte below 48": good[:5] + b"/" + good[6:],
        "byte above 111": good[:5] + b"p" + good[6:],
        "unterminated": good[:-1] + bytes([((good[-1] - 48) | 0x20) + 48]),
        "token of 8 characters": long_token + rest,
        "one slot too few": (good, n - 1),
        "one slot too many": (good, n + 1),
        "negative count": ref.encode_counts(with_negative),
        "count above H*W": ref.encode_counts([0, HW + 1]),
        "sum H*W - 1": ref.encode_counts(short),
    }


def test_every_class_of_bad_string_is_flagged_marked_and_leaves_its_crop_untouched():
    """Malformed inputs the kernel bounds by its slices: nothing faults.  Detection `bad` of six is replaced by each class in turn."""
    from gigapose_amd import ingest

    H, W, T, sentinel = 120, 160, 224, -7.5
    case = syn.detection_case(seed=31, n_img=2, D=6, H=H, W=W)
    lists = [ingest.mask_to_rle_counts(m).astype(np.int64) for m in case["masks"]]
    strings = [ref.encode_counts(c) for c in lists]
    _, good_rle, _ = tgi.both_routes(case)
    _, good_cum, _ = list_scan(lists, H, W)
    for bad in (2, 5):
        classes = malformed(strings[bad], [int(v) for v in lists[bad]], H * W)
        assert ref.decode_values(classes["unterminated"][:-1] + b"0")          # only its last character is wrong
        with pytest.raises(ValueError, match="stops inside"):
            ref.decode_values(classes["unterminated"])
        with pytest.raises(ValueError, match="longer than 7"):
            ref.decode_values(classes["token of 8 characters"])
        for name, item in classes.items():
            items = list(strings)
            items[bad] = item
            data, byte_offsets, counts, offsets = layout(items)
            flag, got_counts, cum = string_scan(data, byte_offsets, counts, offsets, H, W)
            assert flag == bad + 1, name
            got_cum = cum.cpu().numpy()
            assert got_cum[offsets[bad + 1] - 1] == -1, name
            at = 0
            for d in range(6):                                          # the neighbours: decoded and summed as if alone
                n = len(lists[d])
                if d != bad:
                    np.testing.assert_array_equal(got_counts[offsets[d]:offsets[d + 1]], lists[d], err_msg=f"{name}: detection {d}")
                    np.testing.assert_array_equal(got_cum[offsets[d]:offsets[d + 1]], good_cum[at:at + n], err_msg=f"{name}: detection {d}")
                at += n
            crop_flag, out = crop_after_scan(case, cum, offsets, len(counts), H, W, T, sentinel)
            assert crop_flag == bad + 1, name
            keep = [d for d in range(6) if d != bad]
            for key in ("tar_img", "tar_mask", "tar_M"):
                assert bool((out[key][bad] == sentinel).all()), f"{name}: {key} of the bad detection was written"
                assert torch.equal(out[key][keep], good_rle[key][keep]), f"{name}: {key}"


def test_bad_slices_and_a_sum_that_would_wrap_32_bits():
    HW = BIG * BIG
    wrap = [1610590724] * 4                                          # every count <= H*W, the sum is H*W + 2^32
    assert sum(wrap) == HW + 2 ** 32 and max(wrap) <= HW
    items = [ref.encode_counts([HW]), ref.encode_counts(wrap), ref.encode_counts([1, HW - 1])]
    data, byte_offsets, counts, offsets = layout(items)
    flag, got_counts, cum = string_scan(data, byte_offsets, counts, offsets, BIG, BIG)
    cum = cum.cpu().numpy()
    assert flag == 2 and cum[4] == -1
    assert got_counts.tolist() == [HW] + wrap + [1, HW - 1]
    assert cum[0] == HW and cum[5:].tolist() == [1, HW]
    # the same sum as an uncompressed list: what gpi_rle_scan says
    lflag, lcum, _ = list_scan([[HW], wrap, [1, HW - 1]], BIG, BIG)
    assert lflag == 2
    np.testing.assert_array_equal(cum, lcum)
    # a slot slice that leaves the arrays, or is empty: flagged by its offsets alone, nothing written through it
    data, byte_offsets, counts, offsets = layout([items[0], items[2], items[0]])
    o = offsets.copy()
    o[-1] += 5
    flag, _, cum = string_scan(data, byte_offsets, counts, o, BIG, BIG)
    assert flag == 3 and cum.cpu().numpy().tolist() == [HW, 1, HW, -77]
    data, byte_offsets, counts, offsets = layout([items[0], (b"o", 0), items[2]])     # no terminator: no slot
    flag, _, cum = string_scan(data, byte_offsets, counts, offsets, BIG, BIG)
    assert flag == 2 and cum.cpu().numpy().tolist() == [HW, 1, HW]
    # a byte slice that leaves the array: marked without reading a byte
    data, byte_offsets, counts, offsets = layout([items[0], items[2]])
    b = byte_offsets.copy()
    b[-1] += 9
    flag, _, cum = string_scan(data, b, counts, offsets, BIG, BIG)
    assert flag == 2 and cum.cpu().numpy().tolist() == [HW, -77, -1]


# ------------------------------------------------------------------------------------------------ routes
def string_route(case, target=224, kinds=("str", "bytes")):
    from gigapose_amd import rle_strings as rs

    H, W = case["masks"].shape[1:]
    segs = []
    for d, m in enumerate(case["masks"]):
        s = rs.mask_to_rle_string(m)
        kind = kinds[d % len(kinds)]
        counts = s.decode("ascii") if kind == "str" else s if kind == "bytes" else rs.rle_counts_from_string(s).tolist()
        segs.append(dict(counts=counts, size=[H, W]))
    packed = rs.pack_rle_any(segs, H, W)
    out = rs.StringRleDetectionPreprocessor(target_size=target)(_t(case["rgb"]), *[_t(a) for a in packed], _t(case["boxes"]),
                                                                _t(case["im_id"]))
    return out, packed


def test_string_route_equals_list_route_equals_dense_route_and_the_reference_golden(golden_dir):
    from gigapose_amd import rle_strings as rs

    g = np.load(os.path.join(golden_dir, "crop.npz"))
    case = syn.detection_case(seed=int(g["seed"]))
    dense, rle, _ = tgi.both_routes(case)
    out, packed = string_route(case)
    tgi.assert_same_bits(out, rle)
    tgi.assert_same_bits(out, dense)
    np.testing.assert_array_equal(out["tar_mask"].cpu().numpy(), g["tar_mask"])
    np.testing.assert_array_equal(out["tar_img"].cpu().numpy().view(np.uint32), g["tar_img"].view(np.uint32))
    np.testing.assert_allclose(out["tar_M"].cpu().numpy(), g["M"], rtol=2e-7, atol=0)
    mixed, packed_mixed = string_route(case, kinds=("str", "list", "bytes"))
    assert len(packed_mixed[0]) < len(packed[0]) and packed_mixed[2].any()
    tgi.assert_same_bits(mixed, dense)
    H, W = case["masks"].shape[1:]
    pre = rs.StringRleDetectionPreprocessor()
    for p in (packed, packed_mixed):
        d_counts = _t(p[2])
        masks = pre.decode(_t(p[0]), _t(p[1]), d_counts, _t(p[3]), H, W)
        np.testing.assert_array_equal(masks.cpu().numpy(), (case["masks"] != 0).astype(np.float32))
        np.testing.assert_array_equal(d_counts.cpu().numpy(), p[2])           # the caller's tensor is not written


def test_bad_string_raises_like_the_list_route_and_empty_batch_and_cpu_tensors():
    from gigapose_amd import _lib
    from gigapose_amd import rle_strings as rs
    from gigapose_amd.ingest import RleDetectionPreprocessor

    H, W = 64, 80
    case = syn.detection_case(seed=33, n_img=1, D=4, H=H, W=W)
    lists = [rs.rle_counts_from_string(rs.mask_to_rle_string(m)).astype(np.int64) for m in case["masks"]]
    lists[2][1] -= 1                                                      # total H*W - 1
    rgb, boxes, im_id = _t(case["rgb"]), _t(case["boxes"]), _t(case["im_id"])
    packed = layout([ref.encode_counts(c) for c in lists])
    with pytest.raises(ValueError, match="detection 2 has a bad run-length list") as s_err:
        rs.StringRleDetectionPreprocessor()(rgb, *[_t(a) for a in packed], boxes, im_id)
    with pytest.raises(ValueError, match="detection 2 has a bad run-length list") as l_err:
        RleDetectionPreprocessor()(rgb, _t(np.concatenate(lists).astype(np.int32)), _t(packed[3]), boxes, im_id)
    assert str(s_err.value).split(": ", 1)[1] == str(l_err.value).split(": ", 1)[1]
    with pytest.raises(ValueError, match="decode: detection 2 has a bad run-length list"):
        rs.StringRleDetectionPreprocessor().decode(*[_t(a) for a in packed], H, W)
    lists[2][1] += 1
    case["boxes"][1] = (9, 9, 9, 12)                                      # empty box
    packed = layout([ref.encode_counts(c) for c in lists])
    with pytest.raises(ValueError, match="detection 1 has an empty / out-of-frame box"):
        rs.StringRleDetectionPreprocessor()(rgb, *[_t(a) for a in packed], _t(case["boxes"]), im_id)
    empty = rs.pack_rle_any([], H, W)
    out = rs.StringRleDetectionPreprocessor()(rgb, *[_t(a) for a in empty], torch.zeros(0, 4, dtype=torch.int64, device=DEV),
                                              torch.zeros(0, dtype=torch.int32, device=DEV))
    assert out["tar_img"].shape == (0, 3, 224, 224) and out["tar_mask"].shape == (0, 224, 224) and out["tar_M"].shape == (0, 3, 3)
    with pytest.raises(_lib.GigaPoseHipError):
        rs.StringRleDetectionPreprocessor()(torch.from_numpy(case["rgb"]), *packed, case["boxes"], case["im_id"])
    with pytest.raises(_lib.GigaPoseHipError):
        rs.StringRleDetectionPreprocessor().decode(torch.from_numpy(packed[0]), *packed[1:], H, W)


# ------------------------------------------------------------------------------------------------ through the model
def test_coco_frame_ingest_then_test_step_writes_what_frame_ingest_writes(tmp_path):
    """ViT-S, 2 objects x 12 templates, chain numerics, crops accumulated; three frames with 5 / 9 / 0 detections.  Route A:
    CocoFrameIngest on compressed strings (str and bytes, one detection per frame left as a list).  Route B: FrameIngest on the
    equivalent lists.  The batches are equal tensor for tensor, the prediction files in every field except `time`."""
    from gigapose_amd import rle_strings as rs
    from gigapose_amd.ingest import FrameIngest

    sizes = [5, 9, 0]
    frames, Ks, infos, dets, _ = tgi.cnos_frames(60, sizes, n_obj=2)
    coco = []
    for frame_dets in dets:
        out = []
        for d, det in enumerate(frame_dets):
            seg = det["segmentation"]
            s = rs.rle_string_from_counts(seg["counts"])
            counts = seg["counts"] if d == 3 else s if d % 2 else s.decode("ascii")
            out.append(dict(det, segmentation=dict(counts=counts, size=seg["size"])))
        coco.append(out)
    assert isinstance(coco[0][0]["segmentation"]["counts"], str) and isinstance(coco[0][1]["segmentation"]["counts"], bytes)
    with pytest.raises(ValueError, match="compressed string counts"):
        FrameIngest()(frames[:1], Ks[:1], infos[:1], coco[:1])            # the gap this route closes
    test_lists = [tgi.make_test_list([d["category_id"] for d in dets[i]], infos[i]["view_id"]) for i in range(3)]
    pinned = torch.from_numpy(frames).pin_memory()
    results = {}
    for name, ingest, source in (("coco", rs.CocoFrameIngest(target_size=224), coco), ("lists", FrameIngest(target_size=224), dets)):
        model = tgi.vits_model(tmp_path / name, 64)
        batches = [ingest(pinned[i:i + 1], Ks[i:i + 1], infos[i:i + 1], source[i:i + 1], test_list=test_lists[i]) for i in range(3)]
        assert [len(b) for b in batches] == sizes and batches[2].tar_img.shape == (0, 3, 224, 224)
        df.trainer_test(model, batches)
        results[name] = (batches, *tgi.read_predictions(tmp_path / name, 3))
    (a_batches, a_files, a_csv), (b_batches, b_files, b_csv) = results["coco"], results["lists"]
    for a, b in zip(a_batches, b_batches):
        for key in ("tar_img", "tar_mask", "tar_K", "tar_M"):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
        assert a.infos.equals(b.infos) and a.test_list is b.test_list
    for i, n in enumerate(sizes):
        assert sorted(a_files[i]) == sorted(b_files[i]) and a_files[i]["poses"].shape == (n, 5, 4, 4)
        for key in a_files[i]:
            assert a_files[i][key].dtype == b_files[i][key].dtype and a_files[i][key].shape == b_files[i][key].shape
            if key != "time":
                assert a_files[i][key].tobytes() == b_files[i][key].tobytes(), f"image {i}: {key}"
    assert list(a_csv) == list(b_csv) and len(a_csv) == 2
    for name in a_csv:
        ca, cb = a_csv[name], b_csv[name]
        assert list(ca.columns) == list(cb.columns) and len(ca) == len(cb) and len(ca) > 0
        for col in ca.columns:
            if col != "time":
                assert ca[col].tolist() == cb[col].tolist(), f"{name}: column {col}"
    # all three frames in ONE call: the per-frame batches, concatenated (strings and lists of several frames in one launch)
    allb = rs.CocoFrameIngest()(pinned, Ks, infos, coco)
    assert len(allb) == 14 and allb.infos.view_id.tolist() == [40] * 5 + [41] * 9
    for key in ("tar_img", "tar_mask", "tar_K", "tar_M"):
        assert torch.equal(getattr(allb, key), torch.cat([getattr(b, key) for b in a_batches]))
