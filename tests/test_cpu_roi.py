"""-m "not gpu": the host side of the RGB network's upper-body crops (rgb_network/roi_extraction.py) - the box rules against the
reference's own slicing, the uncompressed AVI reader, the refusals - and properties of the numpy restatement tests/roi_ref.py."""
import numpy as np
import pandas as pd
import pytest

import mgr_amd  # noqa: F401
from mgr_amd.rgb_network import cnn_lstm
from mgr_amd.rgb_network import roi_extraction as roi
from tests import roi_ref
from tests.avi_writer import write_avi

GRAY = np.zeros((480, 640), np.uint8)


def _ref_boxes(hx, hy, sy, n):
    return np.array([roi_ref.box(GRAY, hx, hy, sy, f) for f in range(n)], np.int32).reshape(n, 4)


def _check_boxes(hx, hy, sy, n):
    got = roi.crop_boxes(np.array(hx, np.int64), np.array(hy, np.int64), np.array(sy, np.int64), n)
    assert got.dtype == np.int32 and got.shape == (n, 4)
    np.testing.assert_array_equal(got, _ref_boxes(list(hx), list(hy), list(sy), n))
    return got


def test_box_centre_and_every_clamp():
    # centre; up <= 0; down >= 480; left <= 0; right >= 640; all four; exactly on each clamp's threshold and one past it
    hx = [320, 320, 320, 100, 500, 0, 180, 181, 460, 459]
    hy = [300, 300, 400, 300, 300, 470, 300, 300, 360, 359]
    sy = [150, 50, 150, 150, 150, 10, 120, 121, 150, 150]
    b = _check_boxes(hx, hy, sy, len(hx))
    assert b[0].tolist() == [30, 420, 140, 500]
    assert b[1, 0] == 1 and b[2, 1] == 479 and b[3, 2] == 1 and b[4, 3] == 639
    assert b[5].tolist() == [1, 479, 1, 180]
    assert b[6, 0] == 1 and b[7, 0] == 1 and b[6, 2] == 1 and b[7, 2] == 1   # up == 0 -> 1, up == 1 stays; left likewise
    assert b[8, 1] == 479 and b[9, 1] == 479 and b[8, 3] == 639 and b[9, 3] == 639
    assert (b[:, 0] >= 1).all() and (b[:, 1] <= 479).all() and (b[:, 2] >= 1).all() and (b[:, 3] <= 639).all()


def test_box_negative_down_and_right_count_from_the_end():
    # hipY + 120 < 0 -> gray[up:down] with down from the end; hipX + 180 < 0 likewise (left clamps to 1)
    hx = [320, -200, -500, -820, 320]
    hy = [-130, 300, 300, 300, -600]
    sy = [-300, 150, 150, 150, -300]
    b = _check_boxes(hx, hy, sy, len(hx))
    assert b[0].tolist() == [1, 470, 140, 500]           # down = -10 -> 470
    assert b[1].tolist() == [30, 420, 1, 620]            # right = -20 -> 620
    assert b[2].tolist() == [30, 420, 1, 320]            # right = -320 -> 320
    assert b[3].tolist() == [0, 330, 0, 640]             # right = -640 -> 0: empty -> fallback
    assert b[4].tolist() == [0, 330, 0, 640]             # down = -480 -> 0: empty -> fallback


def test_box_empty_crop_falls_back():
    # up >= down, up past the frame, left past the frame, left >= right
    hx = [320, 320, 900, 320]
    hy = [100, 300, 300, 300]
    sy = [400, 700, 150, 150]
    b = _check_boxes(hx, hy, sy, len(hx))
    assert (b[:3] == [0, 330, 0, 640]).all()
    assert b[3].tolist() == [30, 420, 140, 500]


def test_box_frames_past_the_skeleton_and_no_rows():
    b = _check_boxes([320, 330], [300, 310], [150, 160], 5)
    assert b[0].tolist() == [30, 420, 140, 500] and b[1].tolist() == [40, 430, 150, 510]
    assert (b[2:] == [0, 330, 0, 640]).all()
    b = _check_boxes([], [], [], 3)
    assert (b == [0, 330, 0, 640]).all()
    assert roi.crop_boxes([], [], [], 0).shape == (0, 4)
    assert roi.crop_boxes([320] * 9, [300] * 9, [150] * 9, 4).shape == (4, 4)   # more rows than frames


def test_box_random_against_the_reference_slicing():
    rng = np.random.RandomState(3)
    n = 4000
    hx, hy, sy = rng.randint(-900, 1300, n), rng.randint(-900, 1000, n), rng.randint(-900, 1000, n)
    _check_boxes(hx, hy, sy, n + 7)


def test_float_or_nan_columns_are_refused():
    with pytest.raises(ValueError, match="integer-typed"):
        roi.crop_boxes(np.array([320.0]), np.array([300]), np.array([150]), 1)
    with pytest.raises(ValueError, match="integer-typed"):
        roi.crop_boxes([320], [300], [np.nan], 1)
    df = pd.DataFrame({"file_number": [1, 1], "hipX": [320, 321], "hipY": [300.0, np.nan], "shcY": [150, 150]})
    with pytest.raises(ValueError, match="hipY"):
        roi._read_skeletal(df)


def _frames(rng, n, h, w):
    return rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)


@pytest.mark.parametrize("bottom_up", [True, False])
@pytest.mark.parametrize("tag", [b"00db", b"00dc"])
def test_avi_reader_orientation_and_chunk_tags(tmp_path, bottom_up, tag):
    rng = np.random.RandomState(1)
    fr = _frames(rng, 5, 6, 7)             # 3 * 7 = 21 bytes per row: rows padded to 24
    p = write_avi(str(tmp_path / "Sample00001_color.avi"), fr, bottom_up=bottom_up, tag=tag)
    got = roi.read_avi(p)
    assert got.dtype == np.uint8 and got.shape == fr.shape
    np.testing.assert_array_equal(got, fr)
    chunks = list(roi.iter_avi(p, 2))
    assert [c.shape[0] for c in chunks] == [2, 2, 1]
    np.testing.assert_array_equal(np.concatenate(chunks), fr)


@pytest.mark.parametrize("junk", [b"odd", b"even", None])
def test_avi_reader_skips_junk_index_rec_lists_and_audio(tmp_path, junk):
    rng = np.random.RandomState(2)
    fr = _frames(rng, 4, 3, 5)
    p = write_avi(str(tmp_path / "a.avi"), fr, junk=junk, ix=True, rec=True, audio=True)
    np.testing.assert_array_equal(roi.read_avi(p), fr)


def test_avi_reader_follows_avix_continuations(tmp_path):
    rng = np.random.RandomState(4)
    fr = _frames(rng, 7, 4, 4)
    p = write_avi(str(tmp_path / "a.avi"), fr, avix_at=3, tag=b"00dc")
    np.testing.assert_array_equal(roi.read_avi(p), fr)
    p = write_avi(str(tmp_path / "b.avi"), fr, avix_at=0)
    np.testing.assert_array_equal(roi.read_avi(p), fr)


def test_avi_reader_zero_frames(tmp_path):
    p = write_avi(str(tmp_path / "a.avi"), np.zeros((0, 4, 4, 3), np.uint8))
    assert roi.read_avi(p).shape == (0, 4, 4, 3)
    assert list(roi.iter_avi(p)) == []


def test_avi_reader_refuses_compressed_and_32_bit(tmp_path):
    fr = np.zeros((2, 4, 4, 3), np.uint8)
    p = write_avi(str(tmp_path / "mjpg.avi"), fr, compression=struct_fourcc(b"MJPG"))
    with pytest.raises(ValueError, match="bgr24"):
        roi.read_avi(p)
    p = write_avi(str(tmp_path / "rgb32.avi"), fr, bits=32)
    with pytest.raises(ValueError, match="32 bits"):
        roi.read_avi(p)
    bad = tmp_path / "x.avi"
    bad.write_bytes(b"RIFF\4\0\0\0WAVE")
    with pytest.raises(ValueError, match="not an AVI"):
        roi.read_avi(str(bad))


def struct_fourcc(b):
    return int.from_bytes(b, "little")


def test_npy_stacks_are_read_and_checked(tmp_path):
    rng = np.random.RandomState(5)
    fr = _frames(rng, 3, 480, 640)
    p = str(tmp_path / "Sample00002_color.npy")
    np.save(p, fr)
    np.testing.assert_array_equal(roi.read_avi(p), fr)
    np.save(p, fr.astype(np.int16))
    with pytest.raises(ValueError, match="uint8"):
        roi.read_avi(p)


def test_mp4_and_wrong_frames_are_refused(tmp_path):
    (tmp_path / "Sample00001_color.mp4").write_bytes(b"\0" * 16)
    df = pd.DataFrame({"file_number": [1], "hipX": [320], "hipY": [300], "shcY": [150]})
    with pytest.raises(ValueError, match="bgr24"):
        roi.extract_body(df, str(tmp_path), str(tmp_path / "out"))
    with pytest.raises(ValueError, match="bgr24"):
        roi.read_avi(str(tmp_path / "Sample00001_color.mp4"))
    with pytest.raises(ValueError, match="480, 640, 3"):
        roi.roi_frames(np.zeros((2, 240, 320, 3), np.uint8), np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="480, 640, 3"):
        roi.roi_frames(np.zeros((2, 480, 640, 3), np.float32), np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="inside the frame"):
        roi.roi_frames(np.zeros((1, 480, 640, 3), np.uint8), np.array([[0, 0, 0, 10]], np.int32))


def test_video_listing_and_output_names(tmp_path):
    for name in ["Sample00003_color.avi", "Sample00001_color.npy", "Sample00002_audio.wav", "notes.avi", "Sample00004_data.csv"]:
        (tmp_path / name).write_bytes(b"")
    assert roi.video_files(str(tmp_path)) == ["Sample00001_color.npy", "Sample00003_color.avi"]
    assert roi.out_name("Sample00003_color.avi") == "Sample00003_color.npy"


# ---- properties of the restatement ----------------------------------------------------------------------------------------------
def test_same_size_is_the_identity():
    sx, w = roi_ref.cubic_table(60, 60)
    assert (sx == np.arange(60)).all() and (w == [0, 2048, 0, 0]).all()
    rng = np.random.RandomState(6)
    img = rng.randint(0, 256, (60, 60)).astype(np.uint8)
    np.testing.assert_array_equal(roi_ref.resize(img, 60), img)


def test_weights_sum_to_one_and_gray_of_primaries():
    for dst, src in [(60, 638), (60, 330), (32, 478), (64, 1), (64, 3), (1, 640), (60, 61)]:
        _, w = roi_ref.cubic_table(dst, src)
        assert (np.abs(w.sum(1) - 2048) <= 2).all(), (dst, src)
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
    assert roi_ref.gray(px).tolist() == [(1868 * 255 + 8192) >> 14, (9617 * 255 + 8192) >> 14, (4899 * 255 + 8192) >> 14, 255, 0]
    assert roi_ref.gray(px).tolist() == [29, 150, 76, 255, 0]


def test_one_row_crop_gives_identical_rows_and_constant_stays_constant():
    rng = np.random.RandomState(7)
    row = rng.randint(0, 256, (1, 300)).astype(np.uint8)
    out = roi_ref.resize(row, 60)
    assert (out == out[0]).all()
    col = rng.randint(0, 256, (300, 1)).astype(np.uint8)
    out = roi_ref.resize(col, 60)
    assert (out == out[:, :1]).all()
    for v in (0, 1, 128, 254, 255):
        assert (roi_ref.resize(np.full((123, 457), v, np.uint8), 60) == v).all()


def test_checkerboard_saturates():
    img = ((np.indices((40, 40)).sum(0) % 2) * 255).astype(np.uint8)
    out = roi_ref.resize(img, 64)      # upscaling a 0/255 checkerboard overshoots on both sides: clipped to 0 and 255
    assert out.min() == 0 and out.max() == 255


def test_extract_npy_files_are_read_back_by_the_rgb_generator(tmp_path):
    rng = np.random.RandomState(8)
    D = 12
    lab = tmp_path / "labels.csv"
    lab.write_text("Id,Sequence\n1,3 4 5\n2,7\n3,1 2\n4,9 9\n")
    data = tmp_path / "rgb"
    data.mkdir()
    lens = {}
    for num in (1, 2, 3, 4):
        fr = _frames(rng, 3 + num, 480, 640)
        hx, hy, sy = [320, 330, 340], [300, 310, 320], [150, 160, 170]
        crops = roi_ref.extract(fr, hx, hy, sy, D)
        assert crops.dtype == np.uint8 and crops.shape == (3 + num, D, D, 1)
        np.save(str(data / roi.out_name("Sample%05d_color.avi" % num)), crops)
        lens[num] = crops
    gen = cnn_lstm.DataGenerator(2, D, 10, 0.5, data_path=str(data), lab_file=str(lab))
    batch, _ = gen.get_batch(True)
    for i, f in enumerate(gen.train_list[:2]):
        num = int(f[6:11])
        n = lens[num].shape[0]
        np.testing.assert_allclose(batch["the_input"][i, :n], (lens[num].astype(np.float32) - 128) / 255, rtol=0, atol=1e-7)
        assert (batch["the_input"][i, n:] == -128 / 255).all()
