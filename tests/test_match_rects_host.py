"""CPU: gigapose_amd/csrc/gp_match_rects.h -- the table of per-wave rectangles match_tiles_split_kernel reads, kMatchRect[nrb][ncb][wave] --
parsed as data (no compiler): every entry is a valid partition of the nrb x ncb live blocks into rectangles the kernel can run and whose
partial maxima it can merge, and the committed file is what tools/gen_match_rects.py prints.
The word layout (include of gp_match.hip: match_wave_tile_unpack): r0 bits 0-3, MI 4-5, c0 6-9, NI 10-12, row-maximum slot 13-14,
column-maximum slot 15-16, active 17."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "gigapose_amd", "csrc", "gp_match_rects.h")
FILLER = (1 << 4) | (1 << 10)            # an inactive wave: MI = NI = 1 at block (0, 0), no slots, not active


def unpack(w):
    return dict(r0=w & 15, mi=(w >> 4) & 3, c0=(w >> 6) & 15, ni=(w >> 10) & 7, rslot=(w >> 13) & 3, cslot=(w >> 15) & 3, active=(w >> 17) & 1)


@pytest.fixture(scope="module")
def table():
    text = open(HEADER).read()
    assert "kMatchRect[9][9][8]" in text
    body = re.sub(r"//[^\n]*", "", text)
    words = [int(w, 16) for w in re.findall(r"0x([0-9a-fA-F]+)u", body)]
    assert len(words) == 9 * 9 * 8
    assert len(re.findall(r"\{", body)) == 1 + 9 + 81                         # the nesting is [9][9][8]
    return [[words[(r * 9 + c) * 8:(r * 9 + c) * 8 + 8] for c in range(9)] for r in range(9)]


def test_every_entry_is_a_partition_the_kernel_can_run(table):
    for nrb in range(9):
        for ncb in range(9):
            words = table[nrb][ncb]
            rects = [unpack(w) for w in words]
            active = [r for r in rects if r["active"]]
            assert all(w == FILLER for w, r in zip(words, rects) if not r["active"]), (nrb, ncb)
            assert len(active) <= 8
            if nrb == 0 or ncb == 0:
                assert not active
                continue
            cover = {}
            for i, r in enumerate(active):
                assert 1 <= r["mi"] <= 2 and 1 <= r["ni"] <= 4, (nrb, ncb, r)              # the instantiations of match_split_kloop
                assert r["r0"] + r["mi"] <= nrb and r["c0"] + r["ni"] <= ncb, (nrb, ncb, r)
                for rb in range(r["r0"], r["r0"] + r["mi"]):
                    for cb in range(r["c0"], r["c0"] + r["ni"]):
                        assert (rb, cb) not in cover, (nrb, ncb, "block multiplied twice", rb, cb)
                        cover[(rb, cb)] = i
            assert set(cover) == {(rb, cb) for rb in range(nrb) for cb in range(ncb)}, (nrb, ncb)
            # row groups: the distinct (r0, MI) ranges are disjoint -- a rectangle lies inside ONE of them -- and there are at most 4
            groups = sorted({(r["r0"], r["mi"]) for r in active})
            assert len(groups) <= 4
            rows_seen = [rb for r0, mi in groups for rb in range(r0, r0 + mi)]
            assert sorted(rows_seen) == list(range(nrb)), (nrb, ncb, groups)
            for g in groups:
                mine = [r for r in active if (r["r0"], r["mi"]) == g]
                slots = [r["rslot"] for r in mine]
                assert len(set(slots)) == len(slots) and max(slots) < 4, (nrb, ncb, g, slots)   # partial row maxima: one slot each
                assert sorted(cb for r in mine for cb in range(r["c0"], r["c0"] + r["ni"])) == list(range(ncb))
            for cb in range(ncb):
                over = [r for r in active if r["c0"] <= cb < r["c0"] + r["ni"]]
                slots = [r["cslot"] for r in over]
                assert len(set(slots)) == len(slots) and max(slots) < 4, (nrb, ncb, cb, slots)  # partial column maxima likewise


def test_nothing_masked_out_is_the_plain_grid(table):
    """8 x 8: four row groups of 2 x two column groups of 4, row slot = the column group, column slot = the row group."""
    rects = [unpack(w) for w in table[8][8]]
    assert all(r["active"] and r["mi"] == 2 and r["ni"] == 4 for r in rects)
    assert sorted((r["r0"], r["c0"]) for r in rects) == [(r0, c0) for r0 in (0, 2, 4, 6) for c0 in (0, 4)]
    assert all(r["rslot"] == r["c0"] // 4 and r["cslot"] == r["r0"] // 2 for r in rects)


def test_committed_header_is_what_the_generator_prints():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_match_rects.py")], capture_output=True, check=True).stdout
    assert out == open(HEADER, "rb").read()
