"""-m gpu: the RGB network's upper-body crops (csrc/roi.hip through rgb_network/roi_extraction.py), bit-exact against the numpy
restatement tests/roi_ref.py: every crop width and height, upscaling, the largest and the fallback crop, img_dim 60 / 32 / 64 / 1,
saturation, batching, chunking and determinism, then AVI and .npy videos -> extract_body / RoiStore -> the RGB DataGenerator and
fit_generator."""
import os

import numpy as np
import pandas as pd
import pytest

from tests import roi_ref
from tests.avi_writer import write_avi

pytestmark = pytest.mark.gpu

H, W = 480, 640


def _roi():
    import mgr_amd  # noqa: F401
    from mgr_amd.rgb_network import roi_extraction
    return roi_extraction


def _pool(rng, n):
    """n frames: random BGR, 0/255 checkerboards of period 1 and 2 (saturation from the cubic's negative lobes), gradients."""
    out = np.empty((n, H, W, 3), np.uint8)
    yy, xx = np.indices((H, W))
    for i in range(n):
        kind = i % 4
        if kind == 0:
            out[i] = rng.randint(0, 256, (H, W, 3))
        elif kind == 1:
            out[i] = (((yy + xx) % 2) * 255)[..., None]
        elif kind == 2:
            out[i] = (((yy // 2 + xx // 2) % 2) * 255)[..., None]
        else:
            out[i, ..., 0], out[i, ..., 1], out[i, ..., 2] = xx % 256, yy % 256, (xx * yy) % 256
    return out


def _coverage_boxes(rng):
    """Every crop width 1..640 and every height 1..480 at least once (random positions), then upscaling crops of 1-4 rows / columns,
    the largest skeleton crop, the fallback crop and the whole frame."""
    boxes = []
    for i in range(W):
        w, h = i + 1, (i % H) + 1 if i < H else rng.randint(1, H + 1)
        y0, x0 = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
        boxes.append([y0, y0 + h, x0, x0 + w])
    for h in (1, 2, 3, 4, 478):
        for w in (1, 2, 3, 4, 638):
            boxes.append([1, 1 + h, 1, 1 + w])
    boxes += [[1, 479, 1, 639], [0, 330, 0, 640], [0, H, 0, W], [479, 480, 639, 640]]
    return np.array(boxes, np.int32)


def _check(got, frames, boxes, D, what):
    assert got.dtype == np.uint8 and got.shape == (len(boxes), D, D, 1), (what, got.shape)
    for i, b in enumerate(boxes):
        ref = roi_ref.roi(frames[i], b, D)
        if not np.array_equal(got[i, :, :, 0], ref):
            bad = np.argwhere(got[i, :, :, 0] != ref)
            raise AssertionError("%s: frame %d box %s: %d of %d bytes differ, first at %s: got %d ref %d"
                                 % (what, i, b.tolist(), len(bad), D * D, tuple(bad[0]), got[i, bad[0][0], bad[0][1], 0],
                                    ref[tuple(bad[0])]))


@pytest.mark.parametrize("D", [60, 32, 64, 1])
def test_every_crop_size_bit_exact(device, D):
    roi = _roi()
    rng = np.random.RandomState(D)
    boxes = _coverage_boxes(rng)
    widths, heights = set((boxes[:, 3] - boxes[:, 2]).tolist()), set((boxes[:, 1] - boxes[:, 0]).tolist())
    assert widths >= set(range(1, W + 1)) and heights >= set(range(1, H + 1))
    pool = _pool(rng, 16)
    step = 64
    for s in range(0, len(boxes), step):
        b = boxes[s:s + step]
        frames = pool[(np.arange(len(b)) + s // step) % len(pool)]
        got = roi.roi_frames(frames, b, img_dim=D, dev=device)
        _check(got, frames, b, D, "D=%d" % D)


def test_batch_chunks_and_repeats_agree(device):
    roi = _roi()
    rng = np.random.RandomState(11)
    frames = _pool(rng, 23)
    boxes = _coverage_boxes(rng)[rng.choice(600, 23, replace=False)]
    whole = roi.roi_frames(frames, boxes, img_dim=60, dev=device)
    _check(whole, frames, boxes, 60, "batch")
    single = np.concatenate([roi.roi_frames(frames[i:i + 1], boxes[i:i + 1], img_dim=60, dev=device) for i in range(len(frames))])
    assert np.array_equal(whole, single)
    chunked = roi.roi_frames(frames, boxes, img_dim=60, dev=device, chunk=5)       # a video longer than one upload chunk
    assert np.array_equal(whole, chunked)
    for _ in range(3):
        assert np.array_equal(roi.roi_frames(frames, boxes, img_dim=60, dev=device), whole)
    # odd img_dim: frames whose output bytes start off a dword boundary (head / tail byte stores)
    odd = roi.roi_frames(frames, boxes, img_dim=7, dev=device)
    _check(odd, frames, boxes, 7, "D=7")


def test_entry_point_edges(device):
    d_fr = device.array(np.full((2, H, W, 3), 200, np.uint8))
    d_out = device.empty((2, 5, 5), np.uint8)
    device.call("mgr_roi_crop", d_fr, 0, H, W, device.zeros((1, 4), np.int32), 5, d_out)      # n = 0: nothing to do
    d_out.upload(np.full((2, 5, 5), 7, np.uint8))
    # a box outside the stated bounds gives zeros, its neighbour (a 1 x 1 crop of gray 200) its own bytes
    boxes = device.array(np.array([[0, 0, 0, 10], [0, 1, 0, 1]], np.int32))
    device.call("mgr_roi_crop", d_fr, 2, H, W, boxes, 5, d_out)
    got = d_out.download()
    assert (got[0] == 0).all() and (got[1] == 200).all()
    from mgr_amd._capi import MgrError
    with pytest.raises(MgrError):
        device.call("mgr_roi_crop", d_fr, 1, H, W, boxes, 65, d_out)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, rng, nums_frames):
    """Videos (alternately AVI and .npy, one AVI with an AVIX continuation) and a skeletal CSV: file 1 has fewer skeleton rows than
    frames, file 3 none, the others one per frame with some joints out of range."""
    vdir = tmp_path / "video"
    vdir.mkdir()
    rows, truth = [], {}
    pool = _pool(rng, 8)
    for k, (num, n) in enumerate(nums_frames):
        frames = pool[rng.randint(0, len(pool), n)]
        frames[:, :8] = rng.randint(0, 256, (n, 8, W, 3))
        nrows = {1: max(n - 3, 0), 3: 0}.get(num, n)
        hx = rng.randint(-50, 700, nrows)
        hy = rng.randint(-150, 500, nrows)
        sy = rng.randint(-20, 600, nrows)
        for f in range(nrows):
            rows.append({"file_number": num, "frame": f, "lhX": 1, "lhY": 2, "rhX": 3, "rhY": 4, "leX": 5, "leY": 6, "reX": 7,
                         "reY": 8, "hipX": int(hx[f]), "hipY": int(hy[f]), "shcX": 9, "shcY": int(sy[f])})
        name = "Sample%05d_color" % num
        if k % 2 == 0:
            write_avi(str(vdir / (name + ".avi")), frames, avix_at=n // 2 if k == 2 else None)
        else:
            np.save(str(vdir / (name + ".npy")), frames)
        truth[name + ".npy"] = (frames, list(hx), list(hy), list(sy))
    csv = tmp_path / "skeletal.csv"
    pd.DataFrame(rows).to_csv(str(csv), index=False)
    return str(vdir), str(csv), truth


def test_extract_body_files_equal_the_reference(device, tmp_path, monkeypatch):
    roi = _roi()
    rng = np.random.RandomState(21)
    vdir, csv, truth = _dataset(tmp_path, rng, [(1, 9), (2, 70), (3, 4), (4, 0), (5, 6)])
    out = tmp_path / "out"
    written = roi.extract_body(csv, vdir, str(out), img_dim=60, dev=device)
    assert sorted(os.path.basename(p) for p in written) == sorted(truth)
    for name, (frames, hx, hy, sy) in truth.items():
        got = np.load(str(out / name))
        assert got.dtype == np.uint8 and got.shape == (len(frames), 60, 60, 1), (name, got.shape)
        assert np.array_equal(got, roi_ref.extract(frames, hx, hy, sy, 60)), name
    monkeypatch.setattr(roi, "_DEV", [device])    # the CLI's default device: this test's context
    assert roi.main(["--skeletal-csv", csv, "--video-dir", vdir, "--out-dir", str(tmp_path / "cli"), "--img-dim", "60"]) is None
    for name in truth:
        assert np.array_equal(np.load(str(tmp_path / "cli" / name)), np.load(str(out / name)))


def test_roi_store_feeds_the_rgb_generator_and_fit(device, tmp_path):
    roi = _roi()
    from mgr_amd.rgb_network import cnn_lstm
    rng = np.random.RandomState(22)
    D, maxlen, bs = 32, 40, 2
    vdir, csv, truth = _dataset(tmp_path, rng, [(1, 12), (2, 8), (3, 5), (5, 10)])
    lab = tmp_path / "labels.csv"
    lab.write_text("Id,Sequence\n1,3 4 5\n2,7\n3,1 2\n5,9 9 2\n")
    out = tmp_path / "rgb"
    roi.extract_body(csv, vdir, str(out), img_dim=D, dev=device)
    store = roi.RoiStore(vdir, csv, img_dim=D, dev=device)
    assert store.names() == sorted(truth)
    from_dir = cnn_lstm.DataGenerator(bs, D, maxlen, 0.5, data_path=str(out), lab_file=str(lab))
    from_store = cnn_lstm.DataGenerator(bs, D, maxlen, 0.5, lab_file=str(lab), store=store)
    assert from_dir.train_list == from_store.train_list and from_dir.val_list == from_store.val_list
    for train in (True, False):
        a, _ = from_dir.get_batch(train)
        b, _ = from_store.get_batch(train)
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    model = cnn_lstm.build_net(img_dim=D, maxlen=maxlen, h=32, device=device)
    hist = model.fit_generator(from_store.next_train(), steps_per_epoch=from_store.get_size(True) // bs, epochs=2, verbose=0,
                               callbacks=[from_store], validation_data=from_store.next_val(), validation_steps=1)
    assert len(hist.history["loss"]) == 2 and all(np.isfinite(v) for v in hist.history["loss"])
