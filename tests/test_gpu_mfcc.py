"""-m gpu: the HTK MFCC_0_D_A front-end (csrc/mfcc.hip through audio_network/feature_extraction.py) against the fp64 restatement
tests/htk_ref.py, its padded / strided output, determinism, and WAV files -> WavStore -> the audio network's fit_generator.

Bound: the kernel computes in fp64 and rounds once to f32, so an output is within 1 f32 ulp of the exact value - except where the
exact value is so close to 0 that the fp64 rounding of its sums (|terms| up to ~1e3, errors ~1e-13) exceeds that ulp; there the
bound is 1e-10 absolute."""
import os

import numpy as np
import pytest

from tests import htk_ref

pytestmark = pytest.mark.gpu

ATOL = 1e-10


def _fe():
    import mgr_amd  # noqa: F401
    from mgr_amd.audio_network import feature_extraction as fe
    return fe


def _check(got, ref, what=""):
    assert got.dtype == np.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    err = np.abs(got.astype(np.float64) - ref)
    ok = (err <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)) | (err <= ATOL)
    if not ok.all():
        i = np.argwhere(~ok)[0]
        raise AssertionError("%s: %d of %d outside 1 ulp / %g, first at %s: got %r ref %r" % (what, (~ok).sum(), ok.size, ATOL,
                                                                                           tuple(i), got[tuple(i)], ref[tuple(i)]))


def _noise(rng, n, scale=8000):
    return np.clip(rng.standard_normal(n) * scale, -32768, 32767).astype(np.int16)


def test_lengths_and_delta_edges(device):
    fe = _fe()
    rng = np.random.RandomState(0)
    # N < frameSize, N = frameSize, N = frameSize + frameRate - 1, then 1, 2, 3 and 5 frames
    lens = [399, 400, 559, 400, 560, 720, 1040]
    waves = [_noise(rng, n) for n in lens]
    got = fe.mfcc(waves, 16000, dev=device)
    assert [g.shape[0] for g in got] == [0, 1, 1, 1, 2, 3, 5]
    for w, g, n in zip(waves, got, lens):
        _check(g, htk_ref.mfcc_0_d_a(w, 16000), "N=%d" % n)
    assert not got[1][:, 13:].any()          # one frame: deltas and accelerations are 0


def test_ragged_batch(device):
    fe = _fe()
    rng = np.random.RandomState(1)
    lens = rng.randint(0, 40000, 16)
    lens[3] = 0
    waves = [_noise(rng, n, scale=rng.uniform(10, 20000)) for n in lens]
    got = fe.mfcc(waves, 16000, dev=device)
    for w, g, n in zip(waves, got, lens):
        _check(g, htk_ref.mfcc_0_d_a(w, 16000), "N=%d" % n)
    # MFCC_0 and MFCC_0_D are the leading columns of the same rows
    for kind, cols in (("MFCC_0", 13), ("MFCC_0_D", 26)):
        part = fe.mfcc(waves[:4], 16000, kind=kind, dev=device)
        assert all(np.array_equal(p, g[:, :cols]) for p, g in zip(part, got[:4]))


def test_long_utterance(device):
    fe = _fe()
    w = _noise(np.random.RandomState(2), 1520240, scale=3000)      # 95 s at 16 kHz
    got = fe.mfcc([w], 16000, dev=device)[0]
    assert got.shape == (9500, 39)
    _check(got, htk_ref.mfcc_0_d_a(w, 16000), "95 s")
    assert fe.mfcc([w], 16000, dev=device, stride=5)[0].shape == (1900, 39)


def test_signals(device):
    fe = _fe()
    n = 16000
    t = np.arange(n)
    rng = np.random.RandomState(3)
    waves = {
        "white noise, full scale": rng.randint(-32768, 32768, n).astype(np.int16),
        "clipped square": np.where((t // 40) % 2, 32767, -32768).astype(np.int16),
        "tone on bin 32 centre": np.round(20000 * np.sin(2 * np.pi * (32 * 16000 / 512) * t / 16000)).astype(np.int16),
        "silence": np.zeros(n, np.int16),
        "DC": np.full(n, 1000, np.int16),
        "DC negative full scale": np.full(n, -32768, np.int16),
    }
    got = fe.mfcc(list(waves.values()), 16000, dev=device)
    for (name, w), g in zip(waves.items(), got):
        _check(g, htk_ref.mfcc_0_d_a(w, 16000), name)
    assert not got[3].any()


@pytest.mark.parametrize("rate", [8000, 16000, 48000])
def test_sample_rates(device, rate):
    fe = _fe()
    rng = np.random.RandomState(rate)
    waves = [_noise(rng, rate * s // 4) for s in (1, 3, 7)]
    got = fe.mfcc(waves, rate, dev=device)
    for w, g in zip(waves, got):
        _check(g, htk_ref.mfcc_0_d_a(w, rate), "%d Hz" % rate)


def test_deterministic(device):
    fe = _fe()
    rng = np.random.RandomState(4)
    waves = [_noise(rng, n) for n in (123456, 40000, 1000, 77777)]
    a = fe.mfcc(waves, 16000, dev=device)
    for _ in range(2):
        b = fe.mfcc(waves, 16000, dev=device)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_padded_strided_batch(device):
    fe = _fe()
    rng = np.random.RandomState(5)
    waves = [_noise(rng, n) for n in (96000, 5000, 0, 300000, 48000)]
    T = 100
    packed = fe.mfcc(waves, 16000, dev=device)
    padded = fe.mfcc_padded(waves, 16000, T, stride=5, dev=device)
    assert padded.shape == (5, T, 39) and padded.dtype == np.float32
    strided = fe.mfcc(waves, 16000, dev=device, stride=5)
    for b, p in enumerate(packed):
        sub = p[::5][:T]
        assert np.array_equal(strided[b], p[::5])
        assert np.array_equal(padded[b, :sub.shape[0]], sub)
        assert not padded[b, sub.shape[0]:].any()


def test_wavstore_feeds_audio_fit_generator(device, tmp_path, monkeypatch):
    fe = _fe()
    from mgr_amd.audio_network import speech_lstm_ctc_words as audio
    from mgr_amd.datagen import CsvStore, WavStore
    monkeypatch.chdir(tmp_path)
    rng = np.random.RandomState(6)
    wav_dir, csv_dir = tmp_path / "wav", tmp_path / "csv"
    wav_dir.mkdir()
    csv_dir.mkdir()
    ids = [401, 402, 405, 410, 411, 420]
    waves = {}
    for fid in ids:
        waves[fid] = _noise(rng, int(rng.randint(16000, 48000)), scale=rng.uniform(100, 10000))
        fe.write_wav(str(wav_dir / ("Sample%05d_audio.wav" % fid)), waves[fid], 16000)
    (wav_dir / "notes.txt").write_text("not audio")
    labels = tmp_path / "labels.csv"
    labels.write_text("Id,Sequence\n" + "".join("%d,%s\n" % (fid, " ".join(str(v) for v in rng.randint(1, 21, 3))) for fid in ids))
    full = fe.mfcc([waves[f] for f in ids], 16000, dev=device)
    for fid, f in zip(ids, full):
        fe.write_audio_csv(str(csv_dir / ("audio_%d.csv" % fid)), f, fid)

    wav_store = WavStore(str(wav_dir), label_csv=str(labels), dev=device)
    csv_store = CsvStore(str(csv_dir), None, str(labels))
    assert wav_store.file_ids() == csv_store.file_ids() == ids
    for fid, f in zip(ids, full):
        got = wav_store.features(fid, "audio")
        assert got.dtype == np.float64 and np.array_equal(got, f[::5].astype(np.float64))
        assert np.array_equal(csv_store.features(fid, "audio").astype(np.float32), f[::5])

    maxlen, bs = 40, 2
    kw = dict(minibatch_size=bs, numfeats=39, maxlen=maxlen, nb_classes=44, dataset='train', val_split=0.2)
    gen = audio.DataGenerator(store=wav_store, **kw)
    ref_gen = audio.DataGenerator(store=csv_store, **kw)
    assert gen.train_list == ref_gen.train_list and len(gen.train_list) == 4
    for train in (True, False):
        (x, _), (xr, _) = gen.get_batch(train), ref_gen.get_batch(train)
        assert np.array_equal(x["the_input"].astype(np.float32), xr["the_input"].astype(np.float32))
        for k in ("the_labels", "input_length", "label_length"):
            assert np.array_equal(x[k], xr[k])
    model = audio.build_model(maxlen, 39, 44, 150, 'no', units=16, device=device)
    hist = model.fit_generator(gen.next_train(), steps_per_epoch=2, epochs=1, verbose=0, callbacks=[gen])
    assert len(hist.history["loss"]) == 1 and np.all(np.isfinite(hist.history["loss"]))
    assert os.path.exists("sp_ctc_lstm_model.json")
