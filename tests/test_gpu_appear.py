"""GPU: libgigapose_appear.so (gpp_patch_descriptors, gpp_patch_valid, gpp_appearance) and gigapose_amd/appearance.py against the
restatement of include/gigapose_appear.h (gigapose_testing/appear_ref.py, which tests/test_appear_host.py holds to independent
readings), BIT FOR BIT: every comparison is equality of integers -- the int8 MFMA kernel included, whose sums are exact.  Then the
whole route on a randomly initialised ViT-S/14 -- which proves plumbing, not accuracy: no checkpoint is available."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
import torch

from gigapose_amd import appearance, ingest, proposals
from gigapose_testing import appear_cases as cases
from gigapose_testing import appear_ref as ref
from gigapose_testing import synthetic as syn
from gigapose_testing.gpu_cases import DEV, K_SMALL, ZNEAR, assert_bits, pose, rotation
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. gpp_patch_descriptors
def device_patch_descriptors(x, gamma, beta, layout):
    store, offset, crop_stride, token_stride, channel_stride = cases.token_layouts(x)[layout]
    return appearance.patch_descriptors(_t(store), crop_stride, token_stride, channel_stride, _t(gamma), _t(beta), cases.EPS, x.shape[0], x.shape[2], offset=offset)


@functools.lru_cache(maxsize=None)
def token_case(C, B):
    """Tokens of every kind (B * 256 of them, the kinds in turn), the LayerNorm's parameters and the restatement's answer, made once."""
    gamma, beta = cases.label_cases.norm_parameters(C, C)
    x, kinds = cases.patch_tokens(7 * C + B, B, C, first_kind=B % 5)
    want_a, want_s = ref.patch_descriptors(x, gamma, beta, cases.EPS)
    for arr in (x, gamma, beta, want_a, want_s):
        arr.setflags(write=False)
    return x, kinds, gamma, beta, want_a, want_s


@pytest.mark.parametrize("B", (1, 3, 65))
@pytest.mark.parametrize("C", (64, 128, 1024))
@pytest.mark.parametrize("layout", ("contiguous", "workspace"))
def test_patch_descriptors_equal_the_restatement_on_tokens_of_every_kind(C, B, layout):
    """NaN stands in the class tokens and in the padding, which must not be read; a NaN or an infinity inside a token flags that
    token alone."""
    x, kinds, gamma, beta, want_a, want_s = token_case(C, B)
    got_a, got_s = device_patch_descriptors(x, gamma, beta, layout)
    assert_bits(got_s, want_s, f"C {C}, B {B}: status")
    assert_bits(got_a, want_a, f"C {C}, B {B}: limbs")
    flat_s, flat_a = want_s.reshape(-1), want_a.reshape(3, -1, C)
    for n, kind in enumerate(kinds[:40]):            # the restatement reads the tokens as named
        assert flat_s[n] == (ref.NON_FINITE if kind in ("nan", "inf") else 0), (n, kind)
        assert (flat_a[:, n] != 0).any() == (flat_s[n] == 0)


def test_patch_descriptors_flag_a_constant_token_without_beta_and_permute_with_the_crops():
    C, B = 128, 3
    gamma, beta = cases.label_cases.norm_parameters(5, C, zero_beta=True)
    x, kinds = cases.patch_tokens(11, B, C)
    want_a, want_s = ref.patch_descriptors(x, gamma, beta, cases.EPS)
    flat = want_s.reshape(-1)
    assert all(flat[n] == ref.ZERO_NORM for n, k in enumerate(kinds) if k == "constant") and (flat == ref.ZERO_NORM).sum() >= 150
    assert all(flat[n] == ref.NON_FINITE for n, k in enumerate(kinds) if k == "inf") and not want_a.reshape(3, -1, C)[:, flat != 0].any()
    got_a, got_s = device_patch_descriptors(x, gamma, beta, "workspace")
    assert_bits(got_s, want_s, "status") or assert_bits(got_a, want_a, "limbs")
    order = np.asarray([2, 0, 1])
    got_a, got_s = device_patch_descriptors(x[order], gamma, beta, "contiguous")
    assert_bits(got_s, want_s[order], "permuted: status") or assert_bits(got_a, want_a[:, order], "permuted: limbs")


# ---------------------------------------------------------------------------------------------- 2. gpp_patch_valid
@pytest.mark.parametrize("B", (1, 5))
def test_patch_valid_equals_the_restatement_at_the_planted_counts(B):
    mask, planted = cases.planted_masks(B, seed=B)
    assert {0, 97, 98, 99, 196} == set(planted.values()) if B == 5 else len(planted) == 5
    mask_d = _t(mask)
    for num, den in ((0, 1), (1, 2), (1, 1)):
        want_valid, want_count, want_set = ref.patch_valid(mask, num, den)
        valid, count, pixels = appearance.patch_valid(mask_d, num, den, want_set=True)
        assert_bits(valid, want_valid, f"valid at {num}/{den}") or assert_bits(count, want_count, "count") or assert_bits(pixels, want_set, "set")
        valid, count = appearance.patch_valid(mask_d, num, den)                                  # set = NULL
        assert_bits(valid, want_valid, f"valid at {num}/{den}, no set") or assert_bits(count, want_count, "count, no set")
        for (b, patch), k in planted.items():
            assert want_set[b, patch] == k and want_valid[b, patch] == {(0, 1): k >= 1, (1, 2): k >= 99, (1, 1): False}[(num, den)]


# ---------------------------------------------------------------------------------------------- 3. gpp_appearance
FIELDS = ("status", "n", "sum", "best", "arg")


def device_appearance(case, qi, ti, want=("best", "arg")):
    return appearance.appearance(_t(case["qa"]), _t(case["q_valid"]), _t(case["ta"]), _t(case["t_valid"]), _t(qi), _t(ti), want=want)


def check_appearance(what, case, qi, ti):
    want = ref.appearance(case["qa"], case["q_valid"], case["ta"], case["t_valid"], qi, ti)
    got = device_appearance(case, qi, ti)
    for name in FIELDS:
        assert_bits(got[name], want[name], f"{what}: {name}")
    return want


@functools.lru_cache(maxsize=None)
def planted(C):
    case = cases.planted_pairs(20 + C, C)
    for v in case.values():
        v.setflags(write=False)
    return case


@pytest.mark.parametrize("C", (64, 128))
def test_appearance_equals_the_restatement_on_the_planted_pairs(C):
    """Maxima at j = 0, 15, 16, 255; equal maxima in two tiles and in two lanes of one tile; an all-negative pair; an invalid template
    patch with the largest dot; one valid patch on either side and none; bad indices among good pairs.  Query and bank differ, so a
    transposed read cannot pass."""
    case = planted(C)
    qi, ti = cases.all_pairs_with_bad(4, 4)
    want = check_appearance(f"C {C}", case, qi, ti)
    i = case["plants"]
    assert [int(want["arg"][0, i[k]]) for k in range(4)] == list(cases.PLANTED_MAX_AT)
    assert want["arg"][0, i[4]] == cases.TIE_TILES[0] and want["arg"][0, i[5]] == cases.TIE_LANES[0] and want["arg"][0, i[6]] != cases.INVALID_WINNER
    status = {(int(q), int(t)): int(s) for q, t, s in zip(qi, ti, want["status"])}
    assert status[(2, 0)] == ref.NO_QUERY_PATCH and status[(0, 2)] == ref.NO_TEMPLATE_PATCH and status[(2, 2)] == ref.NO_QUERY_PATCH | ref.NO_TEMPLATE_PATCH
    assert (want["status"] == ref.BAD_INDEX).sum() == 4 and status[(1, 1)] == 0
    p33 = int(np.flatnonzero((qi == 3) & (ti == 3))[0])
    assert (want["best"][p33] < 0).all() and want["n"][p33] == 256
    swapped = ref.appearance(case["ta"], case["t_valid"], case["qa"], case["q_valid"], ti[:1], qi[:1])
    assert swapped["sum"][0] != want["sum"][0]                                                   # asymmetric operands


def test_appearance_at_the_extremes_of_the_limbs_fills_the_accumulators():
    """C = 2048, every limb at an extreme of either sign: patch 0 of row 0 against itself reaches 3 * 2^23 in the accumulator of weight 2."""
    C = 2048
    a = cases.extreme_limbs(5, 2, C)
    assert max(abs(v) for v in ref.limb_sums(a[:, 0, 0], a[:, 0, 0])) == 3 << 23
    rs = np.random.RandomState(6)
    valid = (rs.uniform(size=(2, 256)) < 0.7).astype(np.uint8)
    valid[:, :2] = 1
    case = dict(qa=a, q_valid=valid, ta=a[:, ::-1].copy(), t_valid=valid[::-1].copy())
    want = check_appearance("extremes", case, np.asarray([0, 1], np.int32), np.asarray([1, 1], np.int32))     # (row 0 against itself, row 1 against row 0)
    assert want["best"][0, 0] == int((ref.limbs_to_q(a[:, 0, 0]).astype(np.int64) ** 2).sum()) == 2048 * 1056832 ** 2 and want["arg"][0, 0] == 0


@pytest.mark.parametrize("P", (0, 1, 3))
def test_appearance_for_any_number_of_pairs_without_best_and_arg(P):
    case = planted(64)
    qi, ti = np.asarray([0, 3, 1][:P], np.int32), np.asarray([0, 3, 0][:P], np.int32)
    want = ref.appearance(case["qa"], case["q_valid"], case["ta"], case["t_valid"], qi, ti)
    for fields in ((), ("best",), ("arg",)):                                                     # best / arg NULL
        got = device_appearance(case, qi, ti, want=fields)
        assert sorted(got) == sorted(("sum", "n", "status") + fields)
        for name in got:
            assert_bits(got[name], want[name], f"P {P}, want {fields}: {name}")


def test_appearance_permutes_with_the_pairs_and_repeats_a_pair():
    case = planted(128)
    qi, ti = cases.all_pairs_with_bad(4, 4)
    want = ref.appearance(case["qa"], case["q_valid"], case["ta"], case["t_valid"], qi, ti)
    order = np.random.RandomState(3).permutation(len(qi))
    order = np.concatenate([order, order[:5], [0, 0, 0]])                                        # several pairs name one crop and one row
    got = device_appearance(case, qi[order], ti[order])
    for name in FIELDS:
        assert_bits(got[name], want[name][order], f"permuted: {name}")


def test_one_call_of_65535_pairs_over_a_few_rows():
    case = planted(64)
    uq, ut = cases.all_pairs_with_bad(4, 4)
    want = ref.appearance(case["qa"], case["q_valid"], case["ta"], case["t_valid"], uq, ut)
    pick = np.random.RandomState(8).randint(len(uq), size=appearance.MAX_PAIRS)
    got = device_appearance(case, uq[pick], ut[pick], want=("arg",))
    for name in ("status", "n", "sum", "arg"):
        assert_bits(got[name], want[name][pick], f"65535 pairs: {name}")


# ---------------------------------------------------------------------------------------------- 4. self-match
def test_a_template_against_itself_scores_one_to_the_quantisation():
    """|q . q - 2^40| <= 2^20 sqrt(C) + C / 4 for a quantised unit vector q (|e_c| <= 1/2: 2 * 2^20 |u . e| <= 2^20 sqrt(C), |e|^2 <= C / 4),
    and a patch's best match is at least its match with itself: score >= 1 - 2^-14, and no cosine of unit vectors exceeds
    1 + the same bound."""
    C, R = 128, 3
    rs = np.random.RandomState(9)
    a = ref.q_to_limbs(cases.quantised_units(rs, (R, 256), C))
    valid = (rs.uniform(size=(R, 256)) < 0.5).astype(np.uint8)
    case = dict(qa=a, q_valid=valid, ta=a, t_valid=valid)
    t = np.arange(R, dtype=np.int32)
    got = device_appearance(case, t, t)
    q = ref.limbs_to_q(a).astype(np.int64)
    own = np.where(valid != 0, (q * q).sum(axis=2), 0).sum(axis=1)
    total, n = got["sum"].cpu().numpy(), got["n"].cpu().numpy()
    assert (total >= own).all() and (n == (valid != 0).sum(axis=1)).all()
    score = appearance.float_appearance(got["sum"], got["n"]).cpu().numpy()
    assert (np.abs(score - 1.0) <= 2.0 ** -14).all(), score
    assert (2.0 ** 20 * np.sqrt(2048) + 2048 / 4) / 2.0 ** 40 <= 2.0 ** -14                      # the bound covers every C the library takes


# ---------------------------------------------------------------------------------------------- 5. end to end
H, W, ROWS, COLS = 240, 320, 3, 4
O, T = 2, 6


@pytest.fixture(scope="module")
def scene(golden_dir):
    """tests/test_gpu_label.py's small scene: two meshes of tests/golden/label_meshes.npz at 6 seeded template poses each, a frame of
    3 x 4 tiles holding the 12 renders, proposals = the renders' masks -- with a PatchBank beside the DescriptorBank.  The model is
    RANDOMLY INITIALISED: plumbing, not accuracy."""
    from gigapose_amd import render
    from gigapose_amd.vit import Dinov2ViT

    with np.load(os.path.join(golden_dir, "label_meshes.npz")) as z:
        objs = [(z[f"{n}_vertices"], z[f"{n}_faces"], z[f"{n}_colours"]) for n in ("boxes", "ball")]
    rs = np.random.RandomState(2121)
    poses = [np.stack([pose(rotation(rs), (rs.uniform(-.3, .3), rs.uniform(-.2, .2), rs.uniform(4.6, 5.4))) for _ in range(T)]).astype(np.float32)
             for _ in range(O)]
    templates = render.MeshTemplates(list(zip(objs, poses)), K=K_SMALL, device=DEV, H=H, W=W, znear=ZNEAR)
    vit = syn.fill_state_dict(Dinov2ViT(384, 12, 6), 31).eval().to(DEV)
    bank, patches = proposals.DescriptorBank(vit), appearance.PatchBank(vit)
    frame = np.zeros((3, ROWS * H, COLS * W), np.uint8)
    props = []
    for o in range(O):
        bank.add(o + 1, templates[o])
        patches.add(o + 1, templates[o])
        rgba = templates.render(o)["rgba"].cpu().numpy()
        for t in range(T):
            n = o * T + t
            y0, x0 = (n // COLS) * H, (n % COLS) * W
            frame[:, y0:y0 + H, x0:x0 + W] = rgba[t, ..., :3].transpose(2, 0, 1)
            mask = np.zeros((ROWS * H, COLS * W), bool)
            mask[y0:y0 + H, x0:x0 + W] = rgba[t, ..., 3] > 0
            props.append(dict(segmentation=dict(counts=ingest.mask_to_rle_counts(mask).tolist(), size=[ROWS * H, COLS * W])))
    return dict(templates=templates, vit=vit, bank=bank, patches=patches, frame=frame[None], props=props)


def norm_of(vit):
    return vit.norm.weight.detach().cpu().numpy(), vit.norm.bias.detach().cpu().numpy(), vit.norm.eps


def test_the_patch_bank_equals_the_restatement_fed_the_devices_tokens(scene, tmp_path):
    s = scene
    assert s["patches"].labels == [1, 2] and s["patches"].a.shape == (3, O * T, 256, 384) and s["patches"].valid.shape == (O * T, 256)
    item = s["templates"][1]
    tokens = s["vit"].forward_features(item.rgb)["x_prenorm"][:, 1:].cpu().numpy()
    want_a, want_s = ref.patch_descriptors(tokens, *norm_of(s["vit"]))
    assert not want_s.any()
    assert_bits(s["patches"].a[:, T:2 * T], want_a, "the limbs of object 2")
    assert_bits(s["patches"].valid[T:2 * T], ref.patch_valid(item.mask.cpu().numpy(), 1, 2)[0], "the valid patches of object 2")
    both = s["vit"].cls_and_patch_descriptors(item.rgb, item.mask, chunk=4)                      # two chunks: one forward each serves both libraries
    q, status = s["vit"].cls_descriptors(item.rgb)
    assert_bits(both["q"], q, "q beside the patches") or assert_bits(both["status"], status, "status") or assert_bits(both["a"], want_a, "limbs in chunks")
    s["patches"].save(tmp_path / "patches.npz")
    loaded = appearance.PatchBank.load(tmp_path / "patches.npz", device=DEV)
    assert loaded.labels == [1, 2] and torch.equal(loaded.a, s["patches"].a) and torch.equal(loaded.valid, s["patches"].valid)


def test_without_a_patch_bank_the_labeller_returns_what_it_returned(scene):
    s = scene
    kw = dict(top_k=3, min_score=0.2, per_label=True, max_dets=9)
    a, b = proposals.ProposalLabeller(s["vit"], s["bank"], appearance=None, **kw), proposals.ProposalLabeller(s["vit"], s["bank"], **kw)
    da, db = a.label(s["frame"], [s["props"]]), b.label(s["frame"], [s["props"]])
    assert da == db and a.report == b.report and "no_patch" not in a.report and len(da[0]) == 9
    assert all("appearance_score" not in d and "semantic_score" not in d for d in da[0])


def make_test_list(labels, view_id):
    from gigapose_amd.tensor_collection import PandasTensorCollection

    objs = sorted(set(int(v) for v in labels))
    return PandasTensorCollection(infos=pd.DataFrame(dict(
        im_id=[view_id] * len(objs), scene_id=[2] * len(objs), obj_id=objs, inst_count=[sum(int(v) == o for v in labels) for o in objs],
        detection_time=[0.05] * len(objs))))


def test_with_a_patch_bank_the_scores_equal_the_restatement_and_order_the_output(scene):
    s = scene
    size = s["props"][0]["segmentation"]["size"]
    off_mask = dict(s["props"][2], bbox=[3 * W + 10, 2 * H + 10, 60, 60])                        # the mask of tile 2, the box inside tile 11's background corner
    props = s["props"] + [s["props"][4], off_mask]                                               # 12: a duplicate of 4;  13: a crop whose mask is all zero
    plain = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=-1.0, nms_iou=(1, 1))
    both = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=-1.0, nms_iou=(1, 1), appearance=s["patches"])
    old = {d["proposal"]: d for d in plain.label(s["frame"], [props])[0]}
    dets = both.label(s["frame"], [props])[0]
    d = both.describe(s["frame"], [props])
    assert size == [ROWS * H, COLS * W] and both.report["no_patch"] == 1 and both.report["kept"] == 13 == len(dets) and 13 not in {x["proposal"] for x in dets}
    assert both.report == dict(plain.report, no_patch=1, kept=13) and plain.report["kept"] == 14
    # the restatement on the device's own tokens and crop masks
    tokens = s["vit"].forward_features(d["crops"])["x_prenorm"][:, 1:].cpu().numpy()
    want_a, want_s = ref.patch_descriptors(tokens, *norm_of(s["vit"]))
    want_valid, want_count, _ = ref.patch_valid(d["tar_mask"].cpu().numpy(), 1, 2)
    assert_bits(d["a"], want_a, "limbs of the crops") or assert_bits(d["pstatus"], want_s, "pstatus") or assert_bits(d["pvalid"], want_valid, "valid")
    assert want_count[13] == 0 and (want_count[:13] > 0).all()
    pair_t = d["label"].astype(np.int32) * T + d["best_template"]
    assert_bits(d["pair_t"], pair_t, "the bank rows of the pairs")
    want = ref.appearance(want_a, want_valid, s["patches"].a.cpu().numpy(), s["patches"].valid.cpu().numpy(), np.arange(14), pair_t)
    for name, key in (("sum", "app_sum"), ("n", "app_n"), ("status", "app_status")):
        assert_bits(d[key], want[name], name)
    assert want["status"].tolist() == [0] * 13 + [ref.NO_QUERY_PATCH]
    appear = ref.float_appearance(want["sum"], want["n"])
    for x in dets:
        p = x["proposal"]
        assert x["semantic_score"] == old[p]["score"] and x["appearance_score"] == appear[p]
        assert x["score"] == (np.float64(x["semantic_score"]) + np.float64(x["appearance_score"])) / 2
        assert (x["category_id"], x["best_template"], x["bbox"]) == (old[p]["category_id"], old[p]["best_template"], old[p]["bbox"])
    assert abs(dets[0]["appearance_score"] - 1.0) <= 2.0 ** -14                                  # a render against its own template
    combined = {x["proposal"]: x["score"] for x in dets}
    assert [x["proposal"] for x in dets] == sorted(combined, key=lambda p: (-combined[p], p))    # the stable sort of the combined score
    assert combined[4] == combined[12] and [x["proposal"] for x in dets].index(4) < [x["proposal"] for x in dets].index(12)
    # ingest.FrameIngest takes the dicts unchanged
    batch = ingest.FrameIngest(target_size=224)(torch.from_numpy(s["frame"]), K_SMALL[None], [dict(scene_id=2, view_id=7)], [dets],
                                                test_list=make_test_list([x["category_id"] for x in dets], 7))
    assert len(batch) == 13 and batch.infos.label.tolist() == [str(x["category_id"]) for x in dets]
    # min_score and max_dets go by the combined score
    cut = sorted(combined.values(), reverse=True)[5]
    few = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=cut, nms_iou=(1, 1), max_dets=4, appearance=s["patches"])
    out = few.label(s["frame"], [props])[0]
    assert [x["proposal"] for x in out] == [x["proposal"] for x in dets][:4]
    assert few.report["low_score"] == sum(v < cut for v in combined.values()) and few.report["over_max_dets"] == few.report["proposals"] - 1 - few.report["low_score"] - 4
