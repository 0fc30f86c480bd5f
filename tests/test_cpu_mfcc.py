"""-m "not gpu": the HTK MFCC front-end's host side (audio_network/feature_extraction.py) - config parsing, WAV reading, the
filterbank table, HTK parameter files, the CSV layout CsvStore reads - and properties of the fp64 reference tests/htk_ref.py."""
import struct

import numpy as np
import pytest

import mgr_amd  # noqa: F401
from mgr_amd.audio_network import feature_extraction as fe
from mgr_amd.datagen import CsvStore
from tests import htk_ref

# the reference's config_HCopy, verbatim
CONFIG_HCOPY = """# Coding parameters
TARGETKIND = MFCC_0
SOURCEFORMAT = WAV
TARGETRATE = 100000.0
SAVECOMPRESSED = T
SAVEWITHCRC = T
WINDOWSIZE = 250000.0
USEHAMMING = T
PREEMCOEF = 0.97
NUMCHANS = 26
CEPLIFTER = 22
NUMCEPS = 12
ENORMALISE = T
"""


def test_config_hcopy_is_accepted(tmp_path):
    p = tmp_path / "config_HCopy"
    p.write_text(CONFIG_HCOPY)
    cfg = fe.read_hcopy_config(str(p))
    assert (cfg["TARGETKIND"], cfg["TARGETRATE"], cfg["WINDOWSIZE"], cfg["USEHAMMING"], cfg["PREEMCOEF"], cfg["NUMCHANS"],
            cfg["CEPLIFTER"], cfg["NUMCEPS"]) == ("MFCC_0", 100000.0, 250000.0, True, 0.97, 26, 22, 12)
    assert sorted(n.split()[0] for n in cfg["notes"]) == ["ENORMALISE", "SAVECOMPRESSED", "SAVEWITHCRC"]
    assert fe.frame_params(16000, cfg) == (400, 160, 512)
    assert fe.frame_params(8000, cfg) == (200, 80, 256)
    assert fe.frame_params(48000, cfg) == (1200, 480, 2048)
    assert fe.parse_hcopy_config("HPARM: NUMCHANS = 24\nTARGETKIND = MFCC_D_A_0\n")["NUMCHANS"] == 24


@pytest.mark.parametrize("line", ["TARGETKIND = MFCC_0_E", "TARGETKIND = MFCC_0_N", "TARGETKIND = MFCC_0_Z", "TARGETKIND = MFCC_0_C",
                                  "TARGETKIND = MFCC_0_K", "TARGETKIND = MFCC_E", "TARGETKIND = FBANK", "TARGETKIND = PLP_0",
                                  "TARGETKIND = MFCC_0_A", "USEPOWER = T", "LOFREQ = 300", "HIFREQ = 3400", "ZMEANSOURCE = T",
                                  "ADDDITHER = 1.0", "USEHAMMING = F", "DELTAWINDOW = 3", "ACCWINDOW = 1", "SIMPLEDIFFS = T",
                                  "SOURCEFORMAT = NIST", "NUMCHANS = many", "NOSUCHKEY = 1", "PREEMCOEF = 1.5"])
def test_config_refuses_unsupported_options(line):
    with pytest.raises(ValueError):
        fe.parse_hcopy_config(CONFIG_HCOPY + line + "\n")


def test_frame_params_refuse_fractional_frames():
    cfg = fe.parse_hcopy_config(CONFIG_HCOPY)
    with pytest.raises(ValueError):
        fe.frame_params(44100, cfg)          # 1102.5 samples per window
    with pytest.raises(ValueError):
        fe.frame_params(16000, fe.parse_hcopy_config(CONFIG_HCOPY + "TARGETRATE = 100003.0\n"))


def _chunk(cid, body):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if len(body) % 2 else b"")


def _wav_bytes(samples, rate=16000, channels=1, bits=16, tag=1, extra=True, truncate=0):
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * channels * bits // 8, channels * bits // 8, bits)
    pcm = np.asarray(samples, "<i2").tobytes() if bits == 16 else bytes(np.asarray(samples, np.uint8))
    chunks = _chunk(b"fmt ", fmt)
    if extra:
        chunks += _chunk(b"LIST", b"INFOISFT" + struct.pack("<I", 5) + b"hello") + _chunk(b"odd ", b"abc")
    data = b"data" + struct.pack("<I", len(pcm)) + pcm
    body = b"WAVE" + chunks + data
    raw = b"RIFF" + struct.pack("<I", len(body)) + body
    return raw[:len(raw) - truncate] if truncate else raw


def test_read_wav_hand_built(tmp_path):
    s = np.array([0, 1, -1, 32767, -32768, 1234, -4321], np.int16)
    p = tmp_path / "a.wav"
    p.write_bytes(_wav_bytes(s, rate=48000))
    got, rate = fe.read_wav(str(p))
    assert rate == 48000 and got.dtype == np.int16 and np.array_equal(got, s)
    fe.write_wav(str(p), s, 8000)
    got, rate = fe.read_wav(str(p))
    assert rate == 8000 and np.array_equal(got, s)


@pytest.mark.parametrize("kw", [dict(bits=8), dict(channels=2), dict(tag=3), dict(truncate=3), dict(truncate=1)])
def test_read_wav_refuses(tmp_path, kw):
    s = np.arange(10, dtype=np.int16) if kw.get("bits", 16) == 16 else np.arange(10)
    if kw.get("channels") == 2:
        s = np.arange(20, dtype=np.int16)
    p = tmp_path / "bad.wav"
    p.write_bytes(_wav_bytes(s, **kw))
    with pytest.raises(ValueError):
        fe.read_wav(str(p))


@pytest.mark.parametrize("rate", [8000, 16000, 48000])
def test_filterbank_table_matches_reference(rate):
    _, _, fft_n = htk_ref.frame_params(rate)
    lo_chan, lo_wt = fe.filterbank_table(rate, fft_n, 26)
    rc, rw = htk_ref.filterbank(rate, fft_n, 26)
    assert np.array_equal(lo_chan, rc[1:])
    np.testing.assert_allclose(lo_wt, rw[1:], rtol=0, atol=1e-13)
    assert lo_chan[0] == -1 and lo_chan.min() == -1 and lo_chan[1:].min() >= 0 and lo_chan.max() == 26


def test_htk_file_round_trip_and_header(tmp_path):
    r = np.random.RandomState(0)
    feats = r.standard_normal((7, 39)).astype(np.float32)
    p = tmp_path / "a.mfc"
    fe.write_htk(str(p), feats, 100000, "MFCC_0_D_A")
    raw = p.read_bytes()
    # nSamples 7, sampPeriod 100000 (0x000186A0), sampSize 156 (0x009C), parmKind 6 | 0x2000 | 0x100 | 0x200 = 0x2306
    assert raw[:12] == bytes([0, 0, 0, 7, 0, 1, 0x86, 0xA0, 0, 0x9C, 0x23, 0x06])
    assert len(raw) == 12 + 7 * 39 * 4 and raw[12:16] == struct.pack(">f", feats[0, 0])
    back, period, kind = fe.read_htk(str(p))
    assert period == 100000 and fe.kind_code(kind) == 0x2306 and np.array_equal(back, feats)
    assert fe.kind_code("MFCC_0") == 0x2006
    for q in ("MFCC_0_D_A_C", "MFCC_0_D_A_K"):
        p2 = tmp_path / "c.mfc"
        p2.write_bytes(struct.pack(">iihh", 1, 100000, 156, fe.kind_code(q)) + b"\0" * 156)
        with pytest.raises(ValueError):
            fe.read_htk(str(p2))
    p.write_bytes(raw[:-4])
    with pytest.raises(ValueError):
        fe.read_htk(str(p))


def test_audio_csv_is_read_back_by_csvstore(tmp_path):
    r = np.random.RandomState(1)
    feats = {3: (r.standard_normal((23, 39)) * np.exp(r.uniform(-8, 4, (23, 39)))).astype(np.float32),
             11: r.standard_normal((4, 39)).astype(np.float32)}
    for fid, f in feats.items():
        fe.write_audio_csv(str(tmp_path / ("audio_%d.csv" % fid)), f, fid)
    for stride in (1, 5):
        store = CsvStore(str(tmp_path), audio_stride=stride)
        assert store.file_ids() == [3, 11]
        for fid, f in feats.items():
            got = store.features(fid, "audio")
            assert got.dtype == np.float64 and got.shape == f[::stride].shape
            assert np.array_equal(got.astype(np.float32), f[::stride])
            np.testing.assert_allclose(got, f[::stride].astype(np.float64), rtol=1e-9, atol=0)   # pandas parser: last bits only


# ---- properties of the reference itself -----------------------------------------------------------------------------------------

def test_ref_fft_magnitude_equals_numpy_rfft():
    r = np.random.RandomState(2)
    for n in (256, 512, 2048):
        x = r.standard_normal((3, n)) * 1000
        np.testing.assert_allclose(np.abs(htk_ref.fft(x)), np.abs(np.fft.fft(x)), rtol=0, atol=1e-9 * np.abs(x).sum())
        np.testing.assert_allclose(np.abs(htk_ref.fft(x))[:, :n // 2 + 1], np.abs(np.fft.rfft(x)), rtol=0, atol=1e-9 * np.abs(x).sum())


def test_ref_silence_gives_zeros():
    out = htk_ref.mfcc_0_d_a(np.zeros(16000, np.int16), 16000)
    assert out.shape == (98, 39) and not out.any()


def test_ref_ramp_statics_give_constant_deltas():
    st = np.outer(np.arange(20.0), np.linspace(-1, 2, 13)) + 3.0
    d = htk_ref.deltas(st)
    a = htk_ref.deltas(d)
    np.testing.assert_allclose(d[2:-2], np.broadcast_to(np.linspace(-1, 2, 13), (16, 13)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(a[4:-4], 0.0, atol=1e-12)


@pytest.mark.parametrize("rate", [8000, 16000, 48000])
def test_ref_interior_filter_weights_sum_to_one(rate):
    _, _, fft_n = htk_ref.frame_params(rate)
    lo_chan, lo_wt = htk_ref.filterbank(rate, fft_n, 26)
    w = np.zeros((fft_n // 2 + 1, 28))
    for k in range(2, fft_n // 2 + 1):
        c = lo_chan[k]
        if c > 0:
            w[k, c] += lo_wt[k]
        if c < 26:
            w[k, c + 1] += 1 - lo_wt[k]
    interior = [k for k in range(2, fft_n // 2 + 1) if 1 <= lo_chan[k] < 26]
    assert len(interior) > fft_n // 4
    np.testing.assert_allclose(w[interior].sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert (lo_wt[2:] >= 0).all() and (lo_wt[2:] <= 1).all()
