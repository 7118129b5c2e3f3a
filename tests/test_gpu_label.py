"""GPU: libgigapose_label.so (gpa_descriptors, gpa_scores, gpa_run_boxes, gpa_nms_matrix, gpa_nms_keep) and
gigapose_amd/proposals.py against the restatement of include/gigapose_label.h (gigapose_testing/label_ref.py, which
tests/test_label_host.py holds to independent readings), BIT FOR BIT: every comparison is equality of integers.  Then the whole
route on a randomly initialised ViT-S/14 -- which proves plumbing, not accuracy: no checkpoint is available."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import dropin_flow as df
from gigapose_amd import ingest, proposals
from gigapose_testing import factory
from gigapose_testing import label_cases as cases
from gigapose_testing import label_ref as ref
from gigapose_testing import synthetic as syn
from gigapose_testing.gpu_cases import DEV, K_SMALL, ZNEAR, assert_bits, pose, rotation
from gigapose_testing.gpu_cases import on_gpu as _t

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1. gpa_descriptors
def device_descriptors(x, gamma, beta, layout):
    store, crop_stride, channel_stride = cases.token_layouts(x)[layout]
    return proposals.descriptors(_t(store), crop_stride, channel_stride, _t(gamma), _t(beta), cases.EPS, *x.shape)


@pytest.mark.parametrize("C", (64, 384, 768, 1024, 2048))
@pytest.mark.parametrize("layout", ("contiguous", "workspace"))
def test_descriptors_equal_the_restatement_on_rows_of_every_kind(C, layout):
    """B = 65 with every row kind 13 times, B = 1 and 2 starting at every kind; NaN stands in every element that must not be read."""
    gamma, beta = cases.norm_parameters(C, C)
    for B, first in [(65, 0)] + [(B, k) for B in (1, 2) for k in range(5)]:
        x, kinds = cases.token_rows(7 * C + B + first, B, C, first)
        want_q, want_s = ref.descriptors(x, gamma, beta, cases.EPS)
        got_q, got_s = device_descriptors(x, gamma, beta, layout)
        assert_bits(got_s, want_s, f"C {C}, B {B}: status")
        assert_bits(got_q, want_q, f"C {C}, B {B}: q")
        for b, kind in enumerate(kinds):            # the restatement reads the rows as named
            assert want_s[b] == (ref.NON_FINITE if kind in ("nan", "inf") else 0), (b, kind)
            assert (want_q[b] != 0).any() == (want_s[b] == 0)


def test_descriptors_flag_a_constant_row_without_beta_and_permute_with_the_crops():
    C, B = 384, 65
    gamma, beta = cases.norm_parameters(5, C, zero_beta=True)
    x, kinds = cases.token_rows(11, B, C)
    want_q, want_s = ref.descriptors(x, gamma, beta, cases.EPS)
    assert all(want_s[b] == ref.ZERO_NORM for b, k in enumerate(kinds) if k == "constant") and (want_s == ref.ZERO_NORM).sum() == 13
    got_q, got_s = device_descriptors(x, gamma, beta, "workspace")
    assert_bits(got_s, want_s, "status") or assert_bits(got_q, want_q, "q")
    order = np.random.RandomState(3).permutation(B)
    got_q, got_s = device_descriptors(x[order], gamma, beta, "contiguous")
    assert_bits(got_s, want_s[order], "permuted: status") or assert_bits(got_q, want_q[order], "permuted: q")


# ---------------------------------------------------------------------------------------------- 2. gpa_scores
FIELDS = ("dot", "obj", "label", "score", "best_template")


def check_scores(what, q, bank, k):
    want = ref.scores(q, bank, k)
    got = proposals.scores(_t(q), _t(bank), k, want=("obj", "dot"))
    assert got["kk"] == want["kk"]
    for name in FIELDS:
        assert_bits(got[name], want[name], f"{what}: {name}")
    return want


@pytest.mark.parametrize("plant", cases.SCORE_PLANTS)
def test_scores_equal_the_restatement_at_every_size(plant):
    """P = 0 .. 65, O = 1 .. 41, T = 1 .. 65, k = 1, 5, 7 (and 64 > T), C = 64 .. 1024; O * T from 1 to 2 665 bank rows (42 tiles)."""
    for n, (P, O, T, C, k) in enumerate(cases.SCORE_SHAPES):
        q, bank = cases.score_case(100 + n, P, O, T, C, plant)
        want = check_scores(f"{plant} {(P, O, T, C, k)}", q, bank, k)
        if plant == "extreme" and P:
            assert want["dot"][0, O - 1, T - 1] == C << 40 and (O * T == 1 or want["dot"][0, 0, 0] == -(C << 40))
        if plant == "negative" and P:
            assert (want["dot"] < 0).all()
        if plant == "ties" and O >= 2 and P:
            assert (want["label"] < O - O // 2).all()                                     # of two equal objects the first wins
        if plant == "ties" and T >= 2 and P:
            assert (want["best_template"] < T - T // 2).all()


def test_scores_permute_with_the_proposals_and_with_the_bank():
    P, O, T, C, k = 65, 7, 42, 384, 5
    q, bank = cases.score_case(9, P, O, T, C, "random")
    want = check_scores("base", q, bank, k)
    rs = np.random.RandomState(4)
    order = rs.permutation(P)
    got = proposals.scores(_t(q[order]), _t(bank), k)
    for name in ("label", "score", "best_template"):
        assert_bits(got[name], want[name][order], f"proposals permuted: {name}")
    po, pt = rs.permutation(O), rs.permutation(T)
    got = proposals.scores(_t(q), _t(np.ascontiguousarray(bank[po][:, pt])), k)
    assert_bits(got["score"], want["score"], "bank permuted: score")
    assert po[got["label"].cpu().numpy()].tolist() == want["label"].tolist()                # random dots: no ties between objects
    assert pt[got["best_template"].cpu().numpy()].tolist() == want["best_template"].tolist()


def test_scores_in_chunks_of_proposals_equal_one_call(monkeypatch):
    q, bank = cases.score_case(12, 65, 3, 11, 64, "random")
    want = ref.scores(q, bank, 5)
    monkeypatch.setattr(proposals, "DOT_BYTES_PER_CALL", 8 * 3 * 11 * 7)                   # 7 proposals per call
    got = proposals.scores(_t(q), _t(bank), 5, want=("obj", "dot"))
    for name in FIELDS:
        assert_bits(got[name], want[name], name)


# ---------------------------------------------------------------------------------------------- 3. gpa_run_boxes
@pytest.mark.parametrize("H,W", ((1, 37), (41, 1), (23, 37), (96, 128), (16384, 256)))
def test_run_boxes_equal_the_restatement_and_the_dense_reading(H, W):
    names, masks = cases.planted_masks(H, W)
    lists = cases.mask_lists(masks)
    lists.append(np.asarray([0, H * W], np.int32))                                          # a first run of length 0: the whole frame
    lists.append(np.asarray([H * W], np.int32))                                             # one run: empty
    counts, offsets = cases.pack(lists)
    box, area, status = proposals.mask_boxes(counts, offsets, H, W)                          # through gpi_rle_scan
    cum = np.concatenate([np.cumsum(c) for c in lists]).astype(np.int32)
    want = ref.run_boxes(cum, offsets, len(cum), H, W)
    for name, g, w in zip(("box", "area", "status"), (box, area, status), want):
        assert_bits(g, w, name)
    dense_box, dense_area = cases.dense_boxes(masks)
    assert (want[0][:len(masks)] == dense_box).all() and (want[1][:len(masks)] == dense_area).all(), names
    assert want[2].tolist() == [ref.EMPTY_MASK if not m.any() else 0 for m in masks] + [0, ref.EMPTY_MASK]
    assert want[0][-2].tolist() == [0, 0, W, H] and want[1][-2] == H * W


@pytest.mark.parametrize("D", (0, 1, 65))
def test_run_boxes_for_any_number_of_masks_and_bad_lists(D):
    H, W = 23, 37
    rs = np.random.RandomState(D)
    masks = rs.uniform(size=(D, H, W)) < rs.uniform(0.0, 0.2, size=(D, 1, 1))
    lists = cases.mask_lists(masks)
    counts, offsets = cases.pack(lists)
    got = proposals.mask_boxes(counts, offsets, H, W)
    dense_box, dense_area = cases.dense_boxes(masks)
    assert_bits(got[0], dense_box, "box") or assert_bits(got[1], dense_area, "area")
    if D:                                                                                   # a slice that is not a list: flagged, never read
        cum = np.concatenate([np.cumsum(c) for c in lists]).astype(np.int32)
        cum[offsets[1] - 1] = -1
        bad_offsets = offsets.copy()
        want = ref.run_boxes(cum, bad_offsets, len(cum), H, W)
        got = proposals.run_boxes(_t(cum), _t(bad_offsets), H, W)
        assert want[2][0] == ref.BAD_MASK and not want[0][0].any()
        for name, g, w in zip(("box", "area", "status"), got, want):
            assert_bits(g, w, f"bad: {name}")
        with pytest.raises(ValueError, match="mask 0 has a bad run-length list"):
            proposals.mask_boxes(np.concatenate([[1], counts]).astype(np.int32), offsets + np.asarray([0] + [1] * D, np.int32), H, W)


# ---------------------------------------------------------------------------------------------- 4. gpa_nms_matrix / gpa_nms_keep
def device_nms_matrix(box, label, num, den, per_label):
    P = len(box)
    sup = torch.full((P, (P + 63) // 64), -1, dtype=torch.int64, device=DEV)
    b, lab = _t(box), _t(label)
    proposals._call("gpa_nms_matrix", proposals._lib.ptr(b), proposals._lib.ptr(lab), P, num, den, int(per_label), proposals._lib.ptr(sup),
                    proposals._lib.stream_ptr())
    return sup.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("P", (0, 1, 63, 64, 65, 129))
@pytest.mark.parametrize("per_label", (False, True))
def test_nms_equals_the_restatement(P, per_label):
    box, label = cases.nms_case(P, P)
    for num, den in ((1, 4), (0, 1), (3, 3), (30000, 65536)):
        want_sup = ref.nms_matrix(box, label, num, den, per_label)
        assert_bits(device_nms_matrix(box, label, num, den, per_label), want_sup, f"sup at {num}/{den}")
        want = ref.nms_keep(want_sup, P)
        assert_bits(proposals.nms(_t(box), _t(label), num, den, per_label), want, f"keep at {num}/{den}")
        if num == den:
            assert want.all()                                                               # IoU > 1 never holds


def test_nms_at_the_threshold_on_degenerate_boxes_and_along_chains():
    A = (0, 0, 5, 1)
    for name, expect in (("at", 1), ("above", 0), ("below", 1)):
        box = np.asarray([A, cases.THRESHOLD_PAIRS[name]], np.int32)
        keep = proposals.nms(_t(box), None, 1, 4)
        assert keep.cpu().tolist() == [1, expect] == ref.nms(box, None, 1, 4, False).tolist(), name
    empty = np.asarray([(0, 0, 10, 10), (3, 3, 3, 9), (8, 8, 2, 2), (0, 0, 0, 0), (0, 0, 10, 10)], np.int32)
    assert proposals.nms(_t(empty), None, 0, 1).cpu().tolist() == [1, 1, 1, 1, 0]            # empty boxes overlap nothing, even at IoU > 0
    for P in (3, 130, 1025):                                                                # A > B > C: C stays when B goes; 16 word boundaries
        box = cases.chain(P)
        keep = proposals.nms(_t(box), None, 1, 4)
        assert_bits(keep, ref.nms(box, None, 1, 4, False), f"chain of {P}")
        assert keep.cpu().tolist() == [1 - (i & 1) for i in range(P)]
    box, label = cases.nms_case(1025, 1025)
    assert_bits(proposals.nms(_t(box), _t(label), 1, 4, True), ref.nms(box, label, 1, 4, True), "1025 boxes per label")
    far = np.asarray([(-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (0, 0, 2 ** 22, 2 ** 22), (5, 5, 6, 6)], np.int32)
    assert_bits(proposals.nms(_t(far), None, 1, 4), ref.nms(far, None, 1, 4, False), "coordinates beyond the clamp")


# ---------------------------------------------------------------------------------------------- 5. end to end
H, W, ROWS, COLS = 240, 320, 3, 4
O, T = 2, 6


@pytest.fixture(scope="module")
def scene(golden_dir):
    """Two meshes of tests/golden/label_meshes.npz at 6 seeded template poses each, drawn by MeshTemplates; a frame of 3 x 4 tiles
    holding the 12 renders; proposals = the renders' masks (no box given).  The model is RANDOMLY INITIALISED: plumbing, not accuracy."""
    from gigapose_amd import render
    from gigapose_amd.vit import Dinov2ViT

    with np.load(os.path.join(golden_dir, "label_meshes.npz")) as z:
        objs = [(z[f"{n}_vertices"], z[f"{n}_faces"], z[f"{n}_colours"]) for n in ("boxes", "ball")]
    rs = np.random.RandomState(2121)
    poses = [np.stack([pose(rotation(rs), (rs.uniform(-.3, .3), rs.uniform(-.2, .2), rs.uniform(4.6, 5.4))) for _ in range(T)]).astype(np.float32)
             for _ in range(O)]
    templates = render.MeshTemplates(list(zip(objs, poses)), K=K_SMALL, device=DEV, H=H, W=W, znear=ZNEAR)
    vit = syn.fill_state_dict(Dinov2ViT(384, 12, 6), 31).eval().to(DEV)
    bank = proposals.DescriptorBank(vit)
    frame = np.zeros((3, ROWS * H, COLS * W), np.uint8)
    props = []
    for o in range(O):
        bank.add(o + 1, templates[o])
        rgba = templates.render(o)["rgba"].cpu().numpy()
        for t in range(T):
            n = o * T + t
            y0, x0 = (n // COLS) * H, (n % COLS) * W
            frame[:, y0:y0 + H, x0:x0 + W] = rgba[t, ..., :3].transpose(2, 0, 1)
            mask = np.zeros((ROWS * H, COLS * W), bool)
            mask[y0:y0 + H, x0:x0 + W] = rgba[t, ..., 3] > 0
            props.append(dict(segmentation=dict(counts=ingest.mask_to_rle_counts(mask).tolist(), size=[ROWS * H, COLS * W])))
    return dict(templates=templates, vit=vit, bank=bank, frame=frame[None], props=props)


def test_every_render_is_labelled_with_its_object_and_its_view(scene, tmp_path):
    s = scene
    assert s["bank"].q.shape == (O, T, 384) and s["bank"].labels == [1, 2]
    labeller = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1, min_score=0.5)
    dets = labeller.label(s["frame"], [s["props"]])[0]
    assert labeller.report == dict(proposals=12, empty_mask=0, flagged_descriptor=0, low_score=0, suppressed=0, over_max_dets=0, kept=12)
    by_proposal = {d["proposal"]: d for d in dets}
    bound = 384 * 2.0 ** -20                            # |q . q / 2^40 - 1| <= (2 * 2^20 * 0.5 * sqrt(C) + C / 4) / 2^40 < C * 2^-20
    for n in range(12):
        d = by_proposal[n]
        assert (d["category_id"], d["best_template"]) == (n // T + 1, n % T), (n, d)
        assert abs(d["score"] - 1.0) <= bound, (n, d["score"])
        assert d["segmentation"] is s["props"][n]["segmentation"]
        x, y, w, h = d["bbox"]
        assert (n % COLS) * W <= x < x + w <= (n % COLS + 1) * W and (n // COLS) * H <= y < y + h <= (n // COLS + 1) * H
    assert [d["score"] for d in dets] == sorted((d["score"] for d in dets), reverse=True)
    # the bank survives a round trip, and the loaded one labels alike
    s["bank"].save(tmp_path / "bank.npz")
    loaded = proposals.DescriptorBank.load(tmp_path / "bank.npz", device=DEV)
    assert loaded.labels == [1, 2] and torch.equal(loaded.q, s["bank"].q)
    again = proposals.ProposalLabeller(s["vit"], loaded, top_k=1).label(s["frame"], [s["props"]])[0]
    assert [(d["proposal"], d["category_id"], d["score"]) for d in again] == [(d["proposal"], d["category_id"], d["score"]) for d in dets]


def test_duplicates_are_suppressed_empty_masks_reported_and_the_decisions_equal_the_restatement(scene):
    s = scene
    size = s["props"][0]["segmentation"]["size"]
    empty = dict(segmentation=dict(counts=[size[0] * size[1]], size=size))
    props = s["props"][:5] + [empty] + s["props"][5:] + [s["props"][3], s["props"][9], empty]       # 3 -> 13, 9 -> 14 (one shifted by the empty one)
    frames = np.concatenate([s["frame"], s["frame"]])
    for kw in (dict(top_k=1), dict(top_k=5, min_score=0.0, per_label=True, max_dets=9), dict(top_k=3, min_score=0.2, nms_iou=(0, 1))):
        labeller = proposals.ProposalLabeller(s["vit"], s["bank"], **kw)
        dets = labeller.label(frames, [props, s["props"][:4]])
        d = labeller.describe(frames, [props, s["props"][:4]])
        assert d["mstatus"].tolist() == [ref.EMPTY_MASK if p is empty else 0 for p in props] + [0] * 4
        # the restatement on the device's own crops: descriptors from the tokens the ViT computed, then every decision
        tokens = s["vit"].forward_features(d["crops"])["x_prenorm"][:, 0].cpu().numpy()
        q, dstatus = ref.descriptors(tokens, s["vit"].norm.weight.detach().cpu().numpy(), s["vit"].norm.bias.detach().cpu().numpy(), s["vit"].norm.eps)
        assert_bits(d["q"], q, "descriptors of the labeller's crops")
        sc = ref.scores(q, s["bank"].q.cpu().numpy(), labeller.top_k)
        want, report = ref.label_proposals(d["image"], sc, dstatus, d["mstatus"], d["box"], sc["kk"], labeller.min_score, labeller.nms_iou,
                                           labeller.per_label, labeller.max_dets, 2)
        assert report == labeller.report and report["empty_mask"] == 2
        first = [0, len(props)]
        for im in range(2):
            assert [first[im] + x["proposal"] for x in dets[im]] == want[im], (kw, im)
            for x, p in zip(dets[im], want[im]):
                assert x["category_id"] == s["bank"].labels[sc["label"][p]] and x["best_template"] == sc["best_template"][p]
                assert x["score"] == ref.float_score(sc["score"][p], sc["kk"])
        if kw == dict(top_k=1):
            kept = sorted(x["proposal"] for x in dets[0])
            assert kept == [0, 1, 2, 3, 4] + list(range(6, 13)) and labeller.report["suppressed"] == 2       # 13 and 14 go, 3 and 10 (the lower indices) stay


def make_test_list(labels, view_id):
    from gigapose_amd.tensor_collection import PandasTensorCollection

    objs = sorted(set(int(v) for v in labels))
    return PandasTensorCollection(infos=pd.DataFrame(dict(
        im_id=[view_id] * len(objs), scene_id=[2] * len(objs), obj_id=objs, inst_count=[sum(int(v) == o for v in labels) for o in objs],
        detection_time=[0.05] * len(objs))))


def read_predictions(log_dir):
    pred_dir = os.path.join(str(log_dir), "predictions")
    with np.load(os.path.join(pred_dir, "0.npz")) as z:
        files = {k: z[k] for k in z.files}
    return files, {f: pd.read_csv(os.path.join(pred_dir, f)) for f in sorted(os.listdir(pred_dir)) if f.endswith(".csv")}


def test_labelled_proposals_go_through_frame_ingest_into_test_step(scene, tmp_path):
    """ProposalLabeller -> FrameIngest -> GigaPose.test_step writes what the same detections, written down by hand, write."""
    s = scene
    dets = proposals.ProposalLabeller(s["vit"], s["bank"], top_k=1).label(s["frame"], [s["props"]])
    by_hand = [[dict(bbox=list(d["bbox"]), category_id=int(d["category_id"]), score=float(d["score"]), segmentation=d["segmentation"]) for d in dets[0]]]
    assert len(by_hand[0]) == 12
    model = factory.build_model("dinov2_vits14", k=5, device=DEV, seed=70, numerics="chain")
    syn.condition_ist(model.ist_net)
    model.template_datasets = {"mesh": s["templates"]}
    model.test_dataset_name, model.run_id, model.accumulate_crops = "mesh", "r0", 0
    out = {}
    for name, source in (("labeller", dets), ("hand", by_hand)):
        model.log_dir = str(tmp_path / name)
        os.makedirs(os.path.join(model.log_dir, "predictions"), exist_ok=True)
        batch = ingest.FrameIngest(target_size=224)(torch.from_numpy(s["frame"]), K_SMALL[None], [dict(scene_id=2, view_id=7)], source,
                                                    test_list=make_test_list([d["category_id"] for d in source[0]], 7))
        assert len(batch) == 12 and batch.infos.label.tolist() == [str(d["category_id"]) for d in source[0]]
        df.trainer_test(model, [batch])
        out[name] = read_predictions(model.log_dir)
    (a_files, a_csv), (b_files, b_csv) = out["labeller"], out["hand"]
    assert sorted(a_files) == sorted(b_files) and a_files["poses"].shape[0] == 12
    for key in a_files:
        if key != "time":
            assert a_files[key].tobytes() == b_files[key].tobytes(), key
    assert list(a_csv) == list(b_csv) and len(a_csv) >= 1
    for name in a_csv:
        for col in a_csv[name].columns:
            if col != "time":
                assert a_csv[name][col].tolist() == b_csv[name][col].tolist(), f"{name}: {col}"
