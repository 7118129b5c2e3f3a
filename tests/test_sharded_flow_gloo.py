"""CPU, world_size 2 / 3 (gloo): `GigaPose.test_step` with a template-SHARDED bank (gigapose_amd/sharded_flow.py) -- host logic only.

The reference's test.py feeds one image per test_step (reference test.py:55-60) with as many detections as the image has; ranks
see different images.  The sharded step's exchanges are fixed-size collectives, so the product runs flushes of exactly
`accumulate_crops` crop rows on every rank and lets the ranks agree INSIDE the flushes on when everybody is done.  Here the device
half of a flush (`GigaPose._run_rows`: predict + downloads) is replaced by a CPU double that computes every crop's rows from the
crop alone and performs the flush's two cross-rank facts -- all ranks' "done" words (they travel with exchange #1) and all ranks'
status words -- as REAL gloo collectives.  A rank whose sequence of collectives differs from its peers' therefore hangs (the group
has a 60 s timeout) or reads words of the wrong shape: what runs as shipped is the crop-granular queue, the cut through images, the
padding, L(j+1)-then-F(j) pipelining, the collectively agreed end, the symmetric range recovery and the file writer.

The second half of the file holds the cases in which ONE rank's data would decide between "raise" and "go on to the next collective":
a crop that trips the range guard whenever it runs (giving up), the crop-transform flag on one rank, a re-pointed model.  There the
double trips per CROP (a planted pixel) and sets its crop-transform flag per crop (the real kernel's test on tar_M) or on a chosen
launch, its `_recover_range` always answers "recalibrated" after its all-reduces, so that only the flow's own rule can end the run, and
the workers RECORD each rank's outcome: the assertion is that all ranks end alike.  Their group times out after 20 s, so a divergence
fails in bounded time."""
import os
import socket
from datetime import timedelta

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gigapose_amd import _lib
from gigapose_amd.gigaPose import GigaPose
from gigapose_amd.tensor_collection import PandasTensorCollection

from test_accumulate_host import K_HYP, _Ev, crop_result, image, load


TRIP_MARK = 4096.0   # a planted pixel: a live row that holds it trips the range guard (status 4) whenever it runs


class _Metric:
    k = K_HYP


class _ShardedModel(GigaPose):
    def __init__(self, log_dir, rows, rank, world, ownership=None):
        torch.nn.Module.__init__(self)
        self.log_dir, self.test_setting, self.test_dataset_name = log_dir, "localization", "syn"
        os.makedirs(os.path.join(log_dir, "predictions"), exist_ok=True)
        self.template_datas, self.template_shard = {"syn": object(), "syn2": object()}, (rank, world, None)
        self.accumulate_crops, self._pending, self._pending_crops, self._in_flight = rows, [], 0, None
        self.image_ownership, self._sharded_flow = ownership, None
        self.testing_metric = _Metric()
        self.launched, self.live_rows, self.trip_on, self.recoveries, self.clock = 0, [], None, 0, 0.0
        self.model_name, self.run_id, self.global_rank = "large", "r0", rank
        self.runs = []                  # (dataset_name, live_rows) per launch
        self.recover_answer = None      # None: two remedies, then none left (the first half of the file); else what _recover_range answers
        self.flag_on = None             # launches on which the crop-transform flag is set whatever the rows hold
        self.crop_flag, self.flag_cleared = 0, 0   # the pose recovery's device flag: persistent until _clear_crop_flag

    def _flushable(self, batch):
        return getattr(batch, "test_list", None) is not None

    def _drain_device(self):
        pass

    def _recover_range(self, bits, images):
        # the product's remedy is collective (plane maxima all-reduced, once per tensor of `images`): the double all-reduces too,
        # so ranks that disagree on the number of calls do not pass
        assert len(images) == 2
        for x in images:
            t = torch.tensor([float(x.shape[0])])
            dist.all_reduce(t)
        self.recoveries += 1
        if self.recover_answer is not None:
            return self.recover_answer
        return "recalibrated" if self.recoveries <= 2 else False

    def _clear_crop_flag(self, dataset_name):
        self.crop_flag = 0
        self.flag_cleared += 1

    def _run_rows(self, inputs, labels_np, dataset_name, aux=None, live_rows=None):
        rank, world, _ = self.template_shard
        assert live_rows is not None and 0 <= live_rows <= len(labels_np)
        imgs = inputs["tar_img"]
        assert imgs.shape[0] == self.accumulate_crops == len(labels_np), "a sharded flush is exactly accumulate_crops rows"
        res = [crop_result(i) for i in imgs]
        status = 4 if ((self.trip_on is not None and self.launched in self.trip_on) or bool((imgs[:live_rows] == TRIP_MARK).any())) else 0
        M = inputs["tar_M"]             # gp_recover_poses' test of the crop transform (csrc/gp_pose.hip), over all rows as there
        if (self.flag_on is not None and self.launched in self.flag_on) or bool(((M[:, 1, 0] != 0) | (M[:, 0, 1] != 0) | (M[:, 0, 0] != M[:, 1, 1])).any()):
            self.crop_flag = 1
        status |= self.crop_flag * _lib.CROP_TRANSFORM_BIT   # the same bit, in the same word, as the real _run_rows
        self.runs.append((dataset_name, live_rows))
        self.launched += 1
        self.live_rows.append(int((imgs.reshape(imgs.shape[0], -1).abs().sum(1) > 0).sum()))
        assert self.live_rows[-1] == live_rows, "the flow tells the device half how many of its rows are real"
        words = torch.zeros(world, dtype=torch.int32)
        dist.all_gather_into_tensor(words, torch.tensor([status], dtype=torch.int32))                 # the flush's status all-gather
        aux_all = torch.zeros(world * len(labels_np), dtype=torch.int32)
        dist.all_gather_into_tensor(aux_all, torch.full((len(labels_np),), int(aux or 0), dtype=torch.int32))   # rides on exchange #1
        t0 = self.clock
        self.clock += 10.0
        host = dict(scores=torch.from_numpy(np.stack([r[0] for r in res])), pred_poses=torch.from_numpy(np.stack([r[1] for r in res])),
                    status=words, aux_all=aux_all, bad_crop_M=torch.full((1,), self.crop_flag, dtype=torch.int32))
        return dict(inputs=inputs, labels=labels_np, pred=None, host=host, ev=(_Ev(t0), _Ev(self.clock)), dataset_name=dataset_name, device="cpu")


def full_image(seed, n, view_id):
    """test_accumulate_host.image with the other tensors the flow slices and pads."""
    b = image(seed, max(n, 1), view_id)
    if n == 0:
        b = PandasTensorCollection(infos=b.infos.iloc[:0], tar_img=b.tar_img[:0])
        b.test_list = PandasTensorCollection(infos=pd.DataFrame(dict(im_id=[], scene_id=[], obj_id=[], inst_count=[], detection_time=[])))
    tl = b.test_list
    b.register_tensor("tar_mask", torch.ones(n, 4, 4))
    b.register_tensor("tar_K", torch.eye(3).expand(n, 3, 3).contiguous())
    b.register_tensor("tar_M", torch.eye(3).expand(n, 3, 3).contiguous())
    b.test_list = tl
    return b


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, tmp, rows, sizes_by_rank, trip_on, ownership, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=60))
    try:
        m = _ShardedModel(os.path.join(tmp, "sharded" if ownership is None else "owned"), rows, rank, world, ownership)
        m.trip_on = trip_on.get(rank)
        if ownership is None:
            feed = [(1000 * rank + i, full_image(5000 + 100 * rank + i, n, view_id=100 * rank + i)) for i, n in enumerate(sizes_by_rank[rank])]
        else:   # every rank replays every image (the reference's loader has no split_by_node); ownership picks
            feed = [(i, full_image(7000 + i, n, view_id=i)) for i, n in enumerate(sizes_by_rank[0])]
        for idx, b in feed:
            assert m.test_step(b, idx) == 0
        m.on_test_epoch_end() if ownership is not None else m.flush_pending()
        flow = m._flow()
        assert not flow.queue and flow.queued == 0 and flow.in_flight is None
        ret[rank] = dict(launched=m.launched, live=m.live_rows, recoveries=m.recoveries)
    finally:
        dist.destroy_process_group()


def _spawn(world, tmp, rows, sizes_by_rank, trip_on=None, ownership=None):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), str(tmp), rows, sizes_by_rank, trip_on or {}, ownership, ret), nprocs=world, join=True)
    return dict(ret)


def _expected(seed, n, view_id, tmp, idx):
    """The per-image flow's file for the same image (single process, accumulate_crops = 0: tests/test_accumulate_host.py)."""
    from test_accumulate_host import _Model

    m = _Model(str(tmp), 0)
    m.test_step(image(seed, n, view_id), idx)
    return load(tmp, idx)


def _check_files(tmp, sub, sizes_by_rank, ref_dir):
    for rank, sizes in enumerate(sizes_by_rank):
        for i, n in enumerate(sizes):
            idx = 1000 * rank + i
            got = load(os.path.join(tmp, sub), idx)
            if n == 0:
                assert got["poses"].shape == (0, K_HYP, 4, 4) and got["scores"].shape == (0, K_HYP) and len(got["object_id"]) == 0
                continue
            want = _expected(5000 + 100 * rank + i, n, 100 * rank + i, ref_dir, idx)
            assert sorted(got) == sorted(want)
            for key in want:
                assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (idx, key)
                if key != "time":
                    np.testing.assert_array_equal(got[key], want[key], err_msg=f"rank {rank} image {i}: {key}")
            assert (got["time"] > 0).all()


def test_ranks_with_different_detection_counts_flush_fixed_rows_and_agree_on_the_end(tmp_path):
    """The review's case: rank 0 sees images of 5 / 9 / 0 detections, rank 1 of 7 / 3 / 12; flushes of 8 rows.  Nobody raises, both ranks
    launch the same number of flushes, every file equals the per-image flow's."""
    sizes = [[5, 9, 0], [7, 3, 12]]
    ret = _spawn(2, tmp_path, 8, sizes)
    # rank 0: 14 crops -> 8 + 6(+2 dummies); rank 1: 22 -> 8 + 8 + 6(+2).  The end is seen in the third flush (both done), one
    # all-dummy flush was already queued behind it: 4 launches on BOTH ranks
    assert ret[0]["launched"] == ret[1]["launched"] == 4
    assert ret[0]["live"] == [8, 6, 0, 0] and ret[1]["live"] == [8, 8, 6, 0]
    _check_files(str(tmp_path), "sharded", sizes, tmp_path / "ref")


def test_a_rank_without_any_image_and_an_image_larger_than_a_flush(tmp_path):
    sizes = [[], [40, 3], [16]]
    ret = _spawn(3, tmp_path, 16, sizes)
    assert len({r["launched"] for r in ret.values()}) == 1
    assert ret[0]["live"] == [0] * ret[0]["launched"]                       # all-dummy flushes only
    assert ret[1]["live"][:3] == [16, 16, 11] and ret[2]["live"][0] == 16   # 40 crops cut 16 + 16 + 8, the 3-crop image joins the third flush
    _check_files(str(tmp_path), "sharded", sizes, tmp_path / "ref")


def test_a_range_trip_on_one_rank_is_recovered_by_all_ranks_together(tmp_path):
    """Flush 1 of rank 0 trips the split range guard.  The status words are shared, so BOTH ranks drop flushes 1 and 2, recover (a
    collective) and run the crops again; a later second trip (flush 4 of rank 1) is recovered the same way.  Files unchanged."""
    sizes = [[8, 8, 8, 5], [8, 3, 8, 8, 2]]
    clean = _spawn(2, tmp_path / "clean", 8, sizes)
    ret = _spawn(2, tmp_path / "trip", 8, sizes, trip_on={0: [1], 1: [4]})
    assert ret[0]["recoveries"] == ret[1]["recoveries"] == 2
    assert ret[0]["launched"] == ret[1]["launched"] > clean[0]["launched"] == clean[1]["launched"]
    _check_files(str(tmp_path / "trip"), "sharded", sizes, tmp_path / "ref")


def test_round_robin_image_ownership_splits_the_replayed_images(tmp_path):
    """Every rank is fed every image (the reference's loader does not split them); `image_ownership: round_robin` makes rank r
    compute idx % world == r only, and on_test_epoch_end merges after a barrier: all files exist exactly once, the csv holds them all."""
    sizes = [[5, 9, 3, 7, 12, 4, 8]]
    ret = _spawn(2, tmp_path, 8, sizes, ownership="round_robin")
    assert sum(sum(r["live"]) for r in ret.values()) == sum(sizes[0])        # every crop computed once over the two ranks
    pred = os.path.join(str(tmp_path), "owned", "predictions")
    assert sorted(f for f in os.listdir(pred) if f.endswith(".npz")) == sorted(f"{i}.npz" for i in range(len(sizes[0])))
    csvs = sorted(f for f in os.listdir(pred) if f.endswith(".csv"))
    assert len(csvs) == 2
    top1 = pd.read_csv(os.path.join(pred, csvs[0]))
    assert len(top1) == sum(sizes[0]) and set(top1.im_id) == set(range(len(sizes[0])))


# ------------------------------------------------------------------------------------------ decisions no rank may take on its own
OUTCOME_S = 20   # a condition, not a measurement: a rank left alone in a collective fails the test after this long


def _outcome_worker(rank, world, port, tmp, rows, case, ret):
    """One rank of a case; records how it ended instead of raising.  case[rank]: sizes, and optionally trip_crops / flag_crops
    [(image, crop)], trip_on / flag_on [launch], repoint (see test_a_repoint_with_crops_queued...)."""
    import time

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=OUTCOME_S))
    mine = case[rank]
    m = _ShardedModel(os.path.join(tmp, "sharded"), rows, rank, world)
    m.recover_answer, m.trip_on, m.flag_on = "recalibrated", mine.get("trip_on"), mine.get("flag_on")
    out, t0 = dict(exc=None, msg=None), time.monotonic()
    try:
        feed = [(1000 * rank + i, full_image(5000 + 100 * rank + i, n, view_id=100 * rank + i)) for i, n in enumerate(mine["sizes"])]
        for i, c in mine.get("trip_crops", []):
            feed[i][1].tar_img[c, 0, 0, 0] = TRIP_MARK
        for i, c in mine.get("flag_crops", []):
            feed[i][1].tar_M[c, 0, 0] *= 1.5          # no longer an isotropic scale
        if "repoint" in mine:
            _repoint(m, feed, mine["repoint"], tmp, out)
        else:
            for idx, b in feed:
                assert m.test_step(b, idx) == 0
            m.flush_pending()
            flow = m._flow()
            assert not flow.queue and flow.queued == 0 and flow.in_flight is None
    except BaseException as e:   # recorded, compared across the ranks by the test
        out.update(exc=type(e).__name__, msg=str(e))
    finally:
        dist.destroy_process_group()
    out.update(launched=m.launched, recoveries=m.recoveries, runs=list(m.runs), flag_cleared=m.flag_cleared, seconds=time.monotonic() - t0)
    ret[rank] = out


def _outcomes(tmp, case, rows=8):
    world = len(case)
    ret = mp.Manager().dict()
    mp.spawn(_outcome_worker, args=(world, _free_port(), str(tmp), rows, case, ret), nprocs=world, join=True)
    ret = dict(ret)
    for r in range(world):
        print(f"rank {r}: {ret[r]['exc']} {ret[r]['msg']!r} launched {ret[r]['launched']} recoveries {ret[r]['recoveries']} "
              f"flag_cleared {ret[r]['flag_cleared']} {ret[r]['seconds']:.2f} s")
    return ret


def _assert_all_ranks_end_alike(ret, exc):
    """Every rank ends with the same exception (None: none), after the same number of launches and recoveries -- in particular no rank
    with the process group's error of one whose peer has left (a timeout, a closed connection)."""
    for r, o in ret.items():
        assert o["exc"] == exc, f"rank {r} ended with {o['exc']}: {o['msg']}"
    assert len({o["msg"] for o in ret.values()}) == 1
    assert len({o["launched"] for o in ret.values()}) == 1, {r: o["launched"] for r, o in ret.items()}
    assert len({o["recoveries"] for o in ret.values()}) == 1, {r: o["recoveries"] for r, o in ret.items()}


def _assert_gave_up_together(ret):
    _assert_all_ranks_end_alike(ret, "GigaPoseHipError")
    assert ret[0]["msg"].startswith("device status 0x4:")
    assert ret[0]["recoveries"] == 2              # the trip that would start the third recovery in a row raises


def test_a_persistent_trip_makes_a_draining_peer_give_up_in_the_same_flush(tmp_path):
    """Rank 0: images of 8 and 8 crops, one crop of the second trips whenever it runs.  Rank 1 is fed nothing: all-dummy flushes, no
    image of its own to count attempts on.  Both give up at the third trip in a row.
    (Before: rank 0 raised after 7 launches and 2 recoveries, rank 1 died in the third recovery's all-reduce.)"""
    _assert_gave_up_together(_outcomes(tmp_path, [dict(sizes=[8, 8], trip_crops=[(1, 5)]), dict(sizes=[])]))


def test_a_persistent_trip_makes_a_peer_cycling_short_images_give_up_in_the_same_flush(tmp_path):
    """As above with rank 1 fed eight images of 3 crops: every redo meets other images there."""
    _assert_gave_up_together(_outcomes(tmp_path, [dict(sizes=[8, 8], trip_crops=[(1, 5)]), dict(sizes=[3] * 8)]))


def test_trips_separated_by_a_clean_flush_do_not_add_up(tmp_path):
    """Rank 0 holds ONE image of 40 crops, cut over flushes 0..4; rank 1 images of 8.  Launches (the same numbering on both ranks):
    1 trips (rank 0) with 2 in flight -> 3, 4 redo them, F(3) and F(4) clean; 5 trips (rank 1) with 6 in flight -> 7, 8 redo them, F(7)
    clean; 8 trips (rank 0) with 9 in flight.  Never two recoveries in a row: all three are recovered, on both ranks, and the files are
    those of the per-image flow.  (Before: the 40-crop image had been in all three, rank 0 gave up alone.)"""
    sizes = [[40], [8] * 5]
    ret = _outcomes(tmp_path, [dict(sizes=sizes[0], trip_on=[1, 8]), dict(sizes=sizes[1], trip_on=[5])])
    _assert_all_ranks_end_alike(ret, None)
    assert ret[0]["recoveries"] == 3
    _check_files(str(tmp_path), "sharded", sizes, tmp_path / "ref")


def test_a_clean_flush_resets_the_count_of_recoveries(tmp_path):
    """Launch 1 trips, its redo (3) trips again: two in a row.  Its second redo (5) is clean.  Then 6 and its redo 8 trip: two in a
    row again.  Four recoveries, nobody raises."""
    sizes = [[8] * 4, [8] * 4]
    ret = _outcomes(tmp_path, [dict(sizes=sizes[0], trip_on=[1, 3]), dict(sizes=sizes[1], trip_on=[6, 8])])
    _assert_all_ranks_end_alike(ret, None)
    assert ret[0]["recoveries"] == 4
    _check_files(str(tmp_path), "sharded", sizes, tmp_path / "ref")


CROP_ASSERT = "tar_M must be an isotropic scale + translation"   # reference lib3d/torch.py:54-55


def test_the_crop_transform_flag_of_one_rank_raises_on_every_rank(tmp_path):
    """The flag is set on rank 0's launch 1 only.  It travels in the gathered word: both ranks raise in F(1), after 3 launches, and both
    clear their flag.  (Before: rank 0 raised, rank 1 went on to launch 4 and died in its collective.)"""
    sizes = [[8] * 4, [8] * 4]
    ret = _outcomes(tmp_path, [dict(sizes=sizes[0], flag_on=[1]), dict(sizes=sizes[1])])
    _assert_all_ranks_end_alike(ret, "AssertionError")
    assert ret[0]["msg"] == CROP_ASSERT and ret[0]["launched"] == 3 and ret[0]["recoveries"] == 0
    assert ret[0]["flag_cleared"] >= 1 and ret[1]["flag_cleared"] >= 1
    for rank in (0, 1):                             # F(0) was clean: its image is on disk
        assert os.path.exists(os.path.join(str(tmp_path), "sharded", "predictions", f"{1000 * rank}.npz"))


def test_a_flush_with_the_flag_and_a_range_trip_is_recovered_first_and_raises_on_its_rerun(tmp_path):
    """Rank 0's image 1 has a crop with an anisotropic tar_M (launch 1), and launch 1 trips the range guard.  The range check comes
    first: launches 1 and 2 are dropped and recovered, 3 redoes 1, and F(3) raises the assert -- on both ranks, after 5 launches."""
    sizes = [[8] * 4, [8] * 4]
    ret = _outcomes(tmp_path, [dict(sizes=sizes[0], flag_crops=[(1, 3)], trip_on=[1]), dict(sizes=sizes[1])])
    _assert_all_ranks_end_alike(ret, "AssertionError")
    assert ret[0]["msg"] == CROP_ASSERT and ret[0]["launched"] == 5 and ret[0]["recoveries"] == 1
    assert ret[0]["flag_cleared"] >= 1 and ret[1]["flag_cleared"] >= 1


def _repoint(m, feed, spec, tmp, out):
    """Image 0 under "syn"; [the model re-pointed and image 1 pushed at once: must raise]; flush_pending on every rank; images 1..
    under "syn2" and another log directory; flush_pending."""
    (idx0, b0), rest = feed[0], feed[1:]
    assert m.test_step(b0, idx0) == 0
    launched = m.launched
    log2 = os.path.join(tmp, "second")
    os.makedirs(os.path.join(log2, "predictions"), exist_ok=True)
    if spec == "push_before_flush":
        log1, m.test_dataset_name, m.log_dir = m.log_dir, "syn2", log2
        try:
            m.test_step(rest[0][1], rest[0][0])
        except ValueError as e:
            out["early_push"] = str(e)
        assert m.launched == launched, "the refused push must not launch anything"
        m.test_dataset_name, m.log_dir = "syn2", log2      # stays re-pointed: what is queued runs under what it was queued under
    m.flush_pending()
    out["first_drain"] = m.launched
    m.test_dataset_name, m.log_dir = "syn2", log2
    for idx, b in rest:
        assert m.test_step(b, idx) == 0
    m.flush_pending()


def test_a_repoint_with_crops_queued_raises_until_every_rank_has_flushed(tmp_path):
    """5 crops queued under "syn"; rank 0 re-points its model to "syn2" and pushes again: ValueError, at once (rank 1 makes no such
    call, so no collective can be behind it).  After flush_pending() on both ranks the first image has run under "syn" and its file
    lies where it was queued for; the later images run under "syn2".  (Before: all launches ran under "syn2".)"""
    ret = _outcomes(tmp_path, [dict(sizes=[5, 5, 6], repoint="push_before_flush"), dict(sizes=[5, 5, 6], repoint="flush_first")])
    _assert_all_ranks_end_alike(ret, None)
    assert "flush_pending()" in ret[0].get("early_push", "") and "early_push" not in ret[1]
    for rank in (0, 1):
        o = ret[rank]
        first, second = o["runs"][:o["first_drain"]], o["runs"][o["first_drain"]:]
        assert {d for d, _ in first} == {"syn"} and sum(n for _, n in first) == 5
        assert {d for d, _ in second} == {"syn2"} and sum(n for _, n in second) == 11
        assert os.path.exists(os.path.join(str(tmp_path), "sharded", "predictions", f"{1000 * rank}.npz"))
        for i in (1, 2):
            assert os.path.exists(os.path.join(str(tmp_path), "second", "predictions", f"{1000 * rank + i}.npz"))
            assert not os.path.exists(os.path.join(str(tmp_path), "sharded", "predictions", f"{1000 * rank + i}.npz"))


def test_flush_pending_without_a_dataset_raises_instead_of_skipping_the_collective(tmp_path):
    """Single process, no collective is reached: a sharded model with no flow yet and no dataset cannot run its padding flushes."""
    m = _ShardedModel(str(tmp_path), 8, 0, 2)
    m.test_dataset_name = None
    with pytest.raises(RuntimeError, match="collective.*no dataset"):
        m.flush_pending()
    assert m.launched == 0
