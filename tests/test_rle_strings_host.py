"""CPU: COCO compressed run-length strings on the host -- the coding's fixed vectors, the vectorised codec of
gigapose_amd.rle_strings against the sequential restatement (gigapose_testing/rle_string_ref.py), pack_rle_any's layout and checks,
a numpy model of the kernel's two passes, and libgigapose_rlestr.so against include/gigapose_rlestr.h."""
import ctypes
import os
import re

import numpy as np
import pytest

from gigapose_amd import ingest
from gigapose_amd import rle_strings as rs
from gigapose_testing import rle_string_ref as ref
from gigapose_testing.symbols import exported_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIST_VECTORS = [
    ([0, 1], b"01"),
    ([12], b"<"),
    ([5, 3, 7], b"537"),
    ([5, 3, 7, 3], b"5370"),
    ([5, 3, 7, 1, 9, 40, 2], b"537N2W1I"),
    ([0, 15, 16, 17, 1, 1000000], b"0?`02A_a`n0"),
    ([100, 15, 16, 511, 512, 2147482493], b"T3?`0`?`?n[nooo1"),
]
VALUE_VECTORS = [
    (15, b"?"), (16, b"`0"), (-16, b"@"), (-17, b"_O"), (511, b"o?"), (512, b"P`0"), (-512, b"P@"), (-513, b"o_O"),
    (2 ** 30, b"PPPPPP1"), (2 ** 31 - 1, b"oooooo1"),
]


@pytest.mark.parametrize("counts,string", LIST_VECTORS)
def test_list_vectors_both_directions(counts, string):
    assert ref.encode_counts(counts) == string
    assert ref.decode_counts(string).tolist() == counts
    assert rs.rle_string_from_counts(counts) == string
    got = rs.rle_counts_from_string(string)
    assert got.dtype == np.int32 and got.tolist() == counts
    assert rs.rle_counts_from_string(string.decode("ascii")).tolist() == counts        # str as well as bytes


@pytest.mark.parametrize("value,token", VALUE_VECTORS)
def test_value_vectors_both_directions(value, token):
    assert ref.encode_value(value) == token
    assert ref.decode_values(token) == [value]
    # through the list codec: [a, b, c, d] with d - b = value puts the token at position 3
    b = max(0, -value)
    counts = [1, b, 2, b + value]
    s = rs.rle_string_from_counts(counts)
    assert s.endswith(token) and s == ref.encode_counts(counts)
    assert rs.rle_counts_from_string(s).tolist() == counts


def random_lists(seed, n):
    """Lists whose deltas are negative as often as positive and whose tokens take every length 1 .. 7."""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(n):
        length = int(rng.randint(1, 40))
        bits = rng.randint(0, 32, size=length)                       # magnitudes spread over all token lengths
        c = (rng.randint(0, 2 ** 31, size=length, dtype=np.int64) >> (31 - bits)).astype(np.int64)
        if i % 5 == 0:
            c[0] = 0
        out.append(c)
    return out


def test_round_trips_of_random_lists_cover_negative_deltas_and_all_token_lengths():
    lengths, negative = set(), 0
    for c in random_lists(11, 200):
        s = rs.rle_string_from_counts(c)
        assert s == ref.encode_counts(c)
        np.testing.assert_array_equal(rs.rle_counts_from_string(s), c)
        np.testing.assert_array_equal(ref.decode_counts(s), c)
        xs = ref.decode_values(s)
        negative += sum(x < 0 for x in xs)
        lengths |= {len(ref.encode_value(x)) for x in xs}
    assert lengths == {1, 2, 3, 4, 5, 6, 7} and negative > 100


def test_mask_to_rle_string_decodes_to_the_uncompressed_counts():
    rng = np.random.RandomState(5)
    masks = [(rng.rand(37, 53) < p).astype(np.uint8) for p in (0.5, 0.05, 0.95)]
    masks += [np.zeros((9, 4), np.uint8), np.ones((9, 4), np.float32)]
    yy, xx = np.mgrid[0:60, 0:80]
    masks.append((((xx - 40) / 25.0) ** 2 + ((yy - 30) / 17.0) ** 2 <= 1.0).astype(np.uint8))
    for m in masks:
        s = rs.mask_to_rle_string(m)
        assert isinstance(s, bytes)
        np.testing.assert_array_equal(ref.decode_counts(s), ingest.mask_to_rle_counts(m))
    assert rs.mask_to_rle_string(masks[3]) == ref.encode_counts([36]) and rs.mask_to_rle_string(masks[4]) == ref.encode_counts([0, 36])


def test_host_decoder_rejections():
    for bad, what in ((b"53/7", "outside 48"), (b"53p7", "outside 48"), (b"53o", "stops inside a token"), (b"5ooooooo1", "more than 7"),
                      (b"", "empty"), ("53é", "not ASCII"), (b"53\xe9", "not ASCII"), (b"5_O", "outside \\[0, 2\\^31\\)")):
        with pytest.raises(ValueError, match=what):
            rs.rle_counts_from_string(bad)
    for bad in (b"53/7", b"53o", b"5ooooooo1"):
        with pytest.raises(ValueError):
            ref.decode_values(bad)
    with pytest.raises(ValueError, match="run lengths must lie"):
        rs.rle_string_from_counts([3, -1])


def seg_list(mask):
    return {"counts": ingest.mask_to_rle_counts(mask).tolist(), "size": list(mask.shape)}


def test_pack_rle_any_offsets_dtypes_and_mixed_batches():
    rng = np.random.RandomState(3)
    H, W = 12, 17
    masks = [(rng.rand(H, W) < p).astype(np.uint8) for p in (0.5, 0.0, 1.0, 0.2, 0.7)]
    kinds = ["str", "list", "bytes", "str", "list"]
    segs = []
    for m, kind in zip(masks, kinds):
        s = rs.mask_to_rle_string(m)
        segs.append(seg_list(m) if kind == "list" else {"counts": s.decode("ascii") if kind == "str" else s, "size": [H, W]})
    data, byte_offsets, counts, offsets = rs.pack_rle_any(segs, H, W)
    assert data.dtype == np.uint8 and byte_offsets.dtype == np.int32 and counts.dtype == np.int32 and offsets.dtype == np.int32
    assert byte_offsets.shape == offsets.shape == (6,) and byte_offsets[0] == 0 and offsets[0] == 0
    assert byte_offsets[-1] == len(data) and offsets[-1] == len(counts)
    for d, (m, kind) in enumerate(zip(masks, kinds)):
        want = ingest.mask_to_rle_counts(m)
        mine = data[byte_offsets[d]:byte_offsets[d + 1]].tobytes()
        assert offsets[d + 1] - offsets[d] == len(want)              # a string's slots: its number of terminators
        if kind == "list":
            assert mine == b""
            np.testing.assert_array_equal(counts[offsets[d]:offsets[d + 1]], want)
        else:
            assert mine == rs.mask_to_rle_string(m)
            assert not counts[offsets[d]:offsets[d + 1]].any()       # zero: the kernel fills them
    # all lists: pack_rle's counts and offsets, and no byte
    lists = [seg_list(m) for m in masks]
    data, byte_offsets, counts, offsets = rs.pack_rle_any(lists, H, W)
    c0, o0 = ingest.pack_rle(lists, H, W)
    assert data.shape == (0,) and byte_offsets.tolist() == [0] * 6
    np.testing.assert_array_equal(counts, c0)
    np.testing.assert_array_equal(offsets, o0)
    data, byte_offsets, counts, offsets = rs.pack_rle_any([], H, W)
    assert data.shape == (0,) and counts.shape == (0,) and byte_offsets.tolist() == [0] and offsets.tolist() == [0]


def test_pack_rle_any_rejections_name_the_detection():
    good = {"counts": rs.mask_to_rle_string(np.eye(6, 8, dtype=np.uint8)), "size": [6, 8]}
    with pytest.raises(ValueError, match=r"detection 1.*size"):
        rs.pack_rle_any([good, {"counts": good["counts"], "size": [8, 6]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 2.*empty"):
        rs.pack_rle_any([good, good, {"counts": "", "size": [6, 8]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 1.*not ASCII"):
        rs.pack_rle_any([good, {"counts": "5é7", "size": [6, 8]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 0.*not ASCII"):
        rs.pack_rle_any([{"counts": b"5\xe97", "size": [6, 8]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 0.*negative"):
        rs.pack_rle_any([{"counts": [50, -2], "size": [6, 8]}], 6, 8)
    with pytest.raises(ValueError, match=r"detection 1.*sum to 47"):
        rs.pack_rle_any([good, {"counts": [40, 7], "size": [6, 8]}], 6, 8)
    with pytest.raises(ValueError, match="not supported"):
        rs.pack_rle_any([], 65536, 65536)
    # what a string holds is the kernel's to check: a wrong total passes the host
    rs.pack_rle_any([{"counts": ref.encode_counts([40, 7]), "size": [6, 8]}], 6, 8)


# ---------------------------------------------------------------------------------------------- the kernel's two passes, in numpy
def two_pass_model(data, HW):
    """What gps_rle_string_scan does with one string, array-wise: (1) every terminator looks BACK over at most 6 continuation
    characters (never before the start) and assembles its token as a base-32 Horner sum from the last group down, the sign taken
    from the last group; its list position is the number of terminators before it.  (2) counts = running sums per parity (position
    0 alone, the even chain from 2, the odd chain from 1); cum = their inclusive sum."""
    v = np.frombuffer(data, np.uint8).astype(np.int64) - 48
    more = (v & 0x20) != 0
    term = np.flatnonzero(~more)
    m = np.arange(len(term))                                           # exclusive count of terminators
    x = (v[term] & 0x1f) - np.where(v[term] & 0x10, 32, 0)
    alive = np.ones(len(term), bool)
    for back in range(1, 7):
        p = term - back
        alive &= p >= 0
        alive[alive] &= more[p[alive]]
        x[alive] = x[alive] * 32 + (v[p[alive]] & 0x1f)
    counts = np.zeros(len(term), np.int64)
    counts[0] = x[0]
    counts[2::2] = np.cumsum(x[2::2])
    counts[1::2] = np.cumsum(x[1::2])
    return m, counts, np.minimum(np.cumsum(counts), HW)


def test_numpy_model_of_the_two_passes_equals_the_sequential_decoder():
    rng = np.random.RandomState(17)
    cases = [np.asarray(c) for c, _ in LIST_VECTORS] + random_lists(23, 60)
    cases.append(ingest.mask_to_rle_counts(rng.rand(37, 53) < 0.5))
    for c in cases:
        s = ref.encode_counts(c)
        m, counts, cum = two_pass_model(s, int(np.sum(c)))
        np.testing.assert_array_equal(m, np.arange(len(c)))
        np.testing.assert_array_equal(counts, ref.decode_counts(s))
        np.testing.assert_array_equal(cum, np.cumsum(np.asarray(c, np.int64)))


# ---------------------------------------------------------------------------------------------- the library and its header
def declared_symbols():
    src = open(os.path.join(ROOT, "include", "gigapose_rlestr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gps_[a-z0-9_]+)\s*\(", src)))


def test_rlestr_library_exports_exactly_its_header_and_no_other_librarys_symbol():
    names = declared_symbols()
    assert names == ["gps_abi_version", "gps_last_error", "gps_rle_string_scan"]
    exported = exported_symbols(rs.RLESTR_LIB_PATH)
    assert [n for n in exported if n.startswith("gps_")] == names
    assert not [n for n in exported if n.startswith(("gp_", "gpi_", "gpo_"))], "another library's symbol in the rlestr library"
    lib = rs.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.gps_abi_version() >= 1
    assert not [n for n in exported_symbols(ingest.INGEST_LIB_PATH) if n.startswith("gps_")]


def test_rlestr_argument_validation_needs_no_gpu():
    lib = rs.lib()
    null = ctypes.c_void_p(0)
    assert lib.gps_rle_string_scan(null, null, 4, null, 10, 1, 480, 640, null, null, null, null) == -1
    assert b"gps_rle_string_scan" in lib.gps_last_error() and b"null" in lib.gps_last_error()
    assert lib.gps_rle_string_scan(null, null, 4, null, 10, 1, 65536, 65536, null, null, null, null) == -1      # H*W >= 2^31
    assert b"bad sizes" in lib.gps_last_error()
    assert lib.gps_rle_string_scan(null, null, -1, null, 10, 1, 480, 640, null, null, null, null) == -1
    assert lib.gps_rle_string_scan(null, null, 4, null, 10, 65536, 480, 640, null, null, null, null) == -1
    assert lib.gps_rle_string_scan(null, null, 0, null, 0, 0, 480, 640, null, null, null, null) == 0            # D = 0: nothing to do
