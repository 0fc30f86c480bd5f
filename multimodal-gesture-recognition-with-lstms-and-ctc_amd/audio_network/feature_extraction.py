"""The audio network's 39-d features from WAV files: an HTK HCopy-compatible MFCC_0_D_A front-end on the GPU.

The reference extracts them outside the repository with HTK's HCopy and its ``config_HCopy`` (README: "13 MFCC features as well
as the first and second order derivatives (total 39 features)") and ships only that config.  Here the host parses the config and
the WAV files and builds HTK's filterbank table; one ``mgr_mfcc`` launch sequence (csrc/mfcc.hip) computes a whole batch of
utterances.  DESIGN 9c restates the algorithm.  Arithmetic is fp64 and the output f32; HTK computes in float, so its own output
differs in the low bits (parity with the HTK binary is not pinned).

Rows are in HTK's column order: C1..C12, C0, then the 13 deltas, then the 13 accelerations.
"""
import fractions
import os
import struct

import numpy as np

from .. import _capi

#: the reference's config_HCopy
REFERENCE_CONFIG = """# Coding parameters
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

DEFAULTS = {"TARGETKIND": "MFCC_0", "TARGETRATE": 100000.0, "WINDOWSIZE": 250000.0, "USEHAMMING": True, "PREEMCOEF": 0.97,
            "NUMCHANS": 20, "CEPLIFTER": 22, "NUMCEPS": 12, "LOFREQ": -1.0, "HIFREQ": -1.0, "USEPOWER": False,
            "ZMEANSOURCE": False, "ADDDITHER": 0.0, "DELTAWINDOW": 2, "ACCWINDOW": 2, "SIMPLEDIFFS": False}
_BOOL = {"USEHAMMING", "USEPOWER", "ZMEANSOURCE", "SIMPLEDIFFS", "SAVECOMPRESSED", "SAVEWITHCRC", "ENORMALISE"}
_INT = {"NUMCHANS", "CEPLIFTER", "NUMCEPS", "DELTAWINDOW", "ACCWINDOW"}
_FLOAT = {"TARGETRATE", "WINDOWSIZE", "PREEMCOEF", "LOFREQ", "HIFREQ", "ADDDITHER"}
#: accepted and ignored: output compression / CRC are not written, ENORMALISE acts on _E only
IGNORED = {"SAVECOMPRESSED": "HTK output compression is not written", "SAVEWITHCRC": "HTK CRC is not written",
           "ENORMALISE": "acts on _E (log energy) only, which is not computed"}

# HTK parameter kinds (HParm): base kinds and qualifier bits
BASE_KINDS = {"WAVEFORM": 0, "LPC": 1, "LPREFC": 2, "LPCEPSTRA": 3, "LPDELCEP": 4, "IREFC": 5, "MFCC": 6, "FBANK": 7, "MELSPEC": 8,
              "USER": 9, "DISCRETE": 10, "PLP": 11}
QUALIFIERS = {"E": 0o100, "N": 0o200, "D": 0o400, "A": 0o1000, "C": 0o2000, "Z": 0o4000, "K": 0o10000, "0": 0o20000}


def _bool(v):
    t = v.strip().upper()
    if t in ("T", "TRUE"):
        return True
    if t in ("F", "FALSE"):
        return False
    raise ValueError("not a boolean: %r" % v)


def parse_hcopy_config(text):
    """config_HCopy-style text -> validated dict (keys as in DEFAULTS, plus "notes": what was accepted and ignored).

    Refuses what the front-end does not implement: target kinds other than MFCC_0 (qualifiers _E _N _Z _C _K), USEPOWER T,
    LOFREQ / HIFREQ other than -1, ZMEANSOURCE T, ADDDITHER != 0, USEHAMMING F, DELTAWINDOW / ACCWINDOW != 2, SIMPLEDIFFS T,
    source formats other than WAV and unknown keys.  The sample-rate-dependent checks (integer frame size and rate) are done by
    ``frame_params``."""
    cfg = dict(DEFAULTS)
    cfg["notes"] = []
    for lineno, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        if not line:
            continue
        if "=" not in line:
            raise ValueError("config line %d: expected KEY = VALUE: %r" % (lineno, raw))
        key, val = (p.strip() for p in line.split("=", 1))
        key = key.split(":")[-1].strip().upper()   # an HTK module prefix ("HPARM: NUMCHANS") is allowed
        val = val.strip().strip('"').strip("'")
        try:
            if key in _BOOL:
                v = _bool(val)
            elif key in _INT:
                v = int(val)
            elif key in _FLOAT:
                v = float(val)
            elif key == "TARGETKIND":
                v = val.upper()
            elif key in ("SOURCEFORMAT", "SOURCEKIND"):
                v = val.upper()
                if v not in (("WAV",) if key == "SOURCEFORMAT" else ("WAVEFORM",)):
                    raise ValueError("only %s = %s is supported" % (key, "WAV" if key == "SOURCEFORMAT" else "WAVEFORM"))
                continue
            else:
                raise ValueError("unsupported config key %s" % key)
        except ValueError as e:
            raise ValueError("config line %d (%s): %s" % (lineno, key, e)) from None
        if key in IGNORED:
            cfg["notes"].append("%s = %s accepted and ignored: %s" % (key, val, IGNORED[key]))
            continue
        cfg[key] = v
    parse_kind(cfg["TARGETKIND"])
    if cfg["USEPOWER"]:
        raise ValueError("USEPOWER T is not supported (the filterbank runs on the magnitude spectrum)")
    if cfg["LOFREQ"] != -1.0 or cfg["HIFREQ"] != -1.0:
        raise ValueError("LOFREQ / HIFREQ other than -1 are not supported")
    if cfg["ZMEANSOURCE"]:
        raise ValueError("ZMEANSOURCE T is not supported")
    if cfg["ADDDITHER"] != 0.0:
        raise ValueError("ADDDITHER is not supported")
    if not cfg["USEHAMMING"]:
        raise ValueError("USEHAMMING F is not supported")
    if cfg["DELTAWINDOW"] != 2 or cfg["ACCWINDOW"] != 2 or cfg["SIMPLEDIFFS"]:
        raise ValueError("only DELTAWINDOW 2, ACCWINDOW 2, SIMPLEDIFFS F are supported")
    if not (0.0 <= cfg["PREEMCOEF"] < 1.0):
        raise ValueError("PREEMCOEF must be in [0, 1)")
    if not (2 <= cfg["NUMCHANS"] <= 128 and 1 <= cfg["NUMCEPS"] <= min(cfg["NUMCHANS"], 63) and cfg["CEPLIFTER"] >= 0):
        raise ValueError("need 2 <= NUMCHANS <= 128, 1 <= NUMCEPS <= min(NUMCHANS, 63), CEPLIFTER >= 0")
    return cfg


def read_hcopy_config(path):
    """Parse and validate a config_HCopy file (see parse_hcopy_config)."""
    with open(path) as f:
        return parse_hcopy_config(f.read())


def parse_kind(kind):
    """'MFCC_0_D_A' -> (deltas, accs).  Only MFCC_0, MFCC_0_D and MFCC_0_D_A (qualifiers in any order) are computed."""
    parts = str(kind).upper().split("_")
    quals = parts[1:]
    if parts[0] != "MFCC" or "0" not in quals:
        raise ValueError("target kind %s is not supported (only MFCC_0[_D[_A]])" % kind)
    bad = [q for q in quals if q not in ("0", "D", "A")]
    if bad or len(set(quals)) != len(quals):
        raise ValueError("target kind %s: qualifiers %s are not supported" % (kind, "_".join(bad) or "repeated"))
    if "A" in quals and "D" not in quals:
        raise ValueError("target kind %s: _A needs _D" % kind)
    return "D" in quals, "A" in quals


def frame_params(sample_rate, cfg):
    """(frameSize, frameRate, fftN) in samples at sample_rate; refuses a window or a frame shift that is not whole samples."""
    rate = fractions.Fraction(int(sample_rate))
    fs = fractions.Fraction(cfg["WINDOWSIZE"]) * rate / 10 ** 7
    fr = fractions.Fraction(cfg["TARGETRATE"]) * rate / 10 ** 7
    if fs.denominator != 1 or fr.denominator != 1:
        raise ValueError("WINDOWSIZE %g / TARGETRATE %g are not whole samples at %d Hz" % (cfg["WINDOWSIZE"], cfg["TARGETRATE"],
                                                                                           sample_rate))
    frame_size, frame_rate = int(fs), int(fr)
    fft_n = 2
    while fft_n < frame_size:
        fft_n *= 2
    if frame_size < 2 or frame_rate < 1 or not 256 <= fft_n <= 2048:
        raise ValueError("frame size %d samples is outside what the front-end supports (FFT sizes 256..2048)" % frame_size)
    return frame_size, frame_rate, fft_n


def filterbank_table(sample_rate, fft_n, num_chans):
    """HTK's mel filterbank (HSigP InitFBank, default LOFREQ / HIFREQ) as (loChan int32 [fftN/2], loWt float64 [fftN/2]), 0-based:
    entry k is HTK's bin k + 1 (k = 0 is DC)."""
    half = fft_n // 2
    fres = float(sample_rate) / (fft_n * 700.0)        # 1e7 / (sampPeriod * fftN * 700)
    mel = lambda k: 1127.0 * np.log(1.0 + (k - 1) * fres)   # noqa: E731  HTK bin k (1-based)
    klo, khi = 2, half
    mlo, mhi = 0.0, mel(half + 1)
    max_chan = num_chans + 1
    cf = np.zeros(max_chan + 2)
    for c in range(1, max_chan + 1):
        cf[c] = c / max_chan * (mhi - mlo) + mlo
    lo_chan = np.full(half, -1, np.int32)
    lo_wt = np.zeros(half, np.float64)
    chan = 1
    for k in range(1, half + 1):
        if k < klo or k > khi:
            continue
        mk = mel(k)
        while chan <= max_chan and cf[chan] < mk:
            chan += 1
        c = chan - 1
        lo_chan[k - 1] = c
        lo_wt[k - 1] = (cf[c + 1] - mk) / (cf[c + 1] - cf[c]) if c > 0 else (cf[1] - mk) / (cf[1] - mlo)
    return lo_chan, lo_wt


def read_wav(path):
    """RIFF/WAVE PCM, 16-bit, mono -> (int16 samples, sample rate).  Unknown chunks are skipped; stereo, other sample widths,
    compressed formats and truncated files are refused."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError("%s: not a RIFF/WAVE file" % path)
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        body = data[pos + 8:pos + 8 + size]
        if len(body) < size:
            raise ValueError("%s: truncated %r chunk (%d of %d bytes)" % (path, cid.decode("latin-1"), len(body), size))
        if cid == b"fmt ":
            if size < 16:
                raise ValueError("%s: fmt chunk too short" % path)
            tag, channels, rate, _, _, bits = struct.unpack("<HHIIHH", body[:16])
            if tag == 0xFFFE and size >= 40:          # WAVE_FORMAT_EXTENSIBLE: the sub-format's first two bytes are the tag
                tag = struct.unpack("<H", body[24:26])[0]
            fmt = (tag, channels, rate, bits)
        elif cid == b"data":
            pcm = body
        pos += 8 + size + (size & 1)                  # chunks are padded to an even size
    if fmt is None or pcm is None:
        raise ValueError("%s: missing %s chunk" % (path, "fmt" if fmt is None else "data"))
    tag, channels, rate, bits = fmt
    if tag != 1:
        raise ValueError("%s: compressed WAV (format tag %d) is not supported, only PCM" % (path, tag))
    if channels != 1:
        raise ValueError("%s: %d channels, only mono is supported" % (path, channels))
    if bits != 16:
        raise ValueError("%s: %d-bit samples, only 16-bit is supported" % (path, bits))
    if len(pcm) % 2:
        raise ValueError("%s: truncated data chunk (odd byte count)" % path)
    return np.frombuffer(pcm, "<i2").astype(np.int16), int(rate)


def write_wav(path, samples, sample_rate):
    """16-bit mono PCM WAV (used to make test inputs)."""
    pcm = np.asarray(samples, np.int16).astype("<i2").tobytes()
    fmt = struct.pack("<HHIIHH", 1, 1, int(sample_rate), 2 * int(sample_rate), 2, 16)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + 8 + len(fmt) + 8 + len(pcm)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(pcm)) + pcm)


_DEV = [None]


def _device():
    if _DEV[0] is None:
        _DEV[0] = _capi.Device(0)
    return _DEV[0]


def _config(config):
    if config is None:
        return parse_hcopy_config(REFERENCE_CONFIG)
    if isinstance(config, (str, os.PathLike)):
        return read_hcopy_config(config)
    return config


def _launch(waves, sample_rate, config, kind, dev, stride, rows_of):
    """One mgr_mfcc launch sequence over the batch; rows_of(u, n_out) -> capacity of utterance u's rows.  Returns (out, offsets,
    n_out per utterance, ncols)."""
    cfg = _config(config)
    deltas, accs = parse_kind(kind)
    frame_size, frame_rate, fft_n = frame_params(sample_rate, cfg)
    nchan, nceps = cfg["NUMCHANS"], cfg["NUMCEPS"]
    ncols = (nceps + 1) * (1 + deltas + accs)
    waves = [np.ascontiguousarray(w, np.int16).reshape(-1) for w in waves]
    if not waves:
        return np.zeros((0, ncols), np.float32), np.zeros(1, np.int64), [], ncols
    lens = np.array([w.size for w in waves], np.int64)
    nfr = np.where(lens >= frame_size, (lens - frame_size) // frame_rate + 1, 0)
    n_out = [int(-(-n // stride)) for n in nfr]
    offs = np.zeros(len(waves) + 1, np.int64)
    offs[1:] = np.cumsum([rows_of(u, n) for u, n in enumerate(n_out)])
    s_offs = np.zeros(len(waves) + 1, np.int64)
    s_offs[1:] = np.cumsum(lens)
    lo_chan, lo_wt = filterbank_table(sample_rate, fft_n, nchan)
    dev = dev or _device()
    n_frames = int(nfr.sum())
    total_rows = int(offs[-1])
    ws_bytes = dev.lib.mgr_mfcc_ws_bytes(len(waves), n_frames, frame_size, fft_n, nchan, nceps)
    arrays = [dev.array(np.concatenate(waves) if lens.sum() else np.zeros(1, np.int16)), dev.array(s_offs), dev.array(lo_chan),
              dev.array(lo_wt), dev.array(offs), dev.empty((max(total_rows, 1), ncols), np.float32), dev.bytes(ws_bytes)]
    d_s, d_so, d_lc, d_lw, d_oo, d_out, d_ws = arrays
    try:
        dev.call("mgr_mfcc", d_s, d_so, len(waves), n_frames, frame_size, frame_rate, fft_n, nchan, nceps, cfg["CEPLIFTER"],
                 float(cfg["PREEMCOEF"]), int(deltas), int(accs), int(stride), d_lc, d_lw, d_out, d_oo, d_ws, ws_bytes)
        out = d_out.download()[:total_rows]
    finally:
        for a in arrays:
            a.free()
        dev._arrays = [a for a in dev._arrays if a.ptr]
    return out, offs, n_out, ncols


#: what datagen.WavStore puts into one launch sequence: mgr_mfcc takes at most 65535 utterances, and 2^28 samples keep the int16
#: upload and the fp64 statics under ~1.2 GB
MAX_SAMPLES_PER_LAUNCH = 1 << 28
MAX_UTTS_PER_LAUNCH = 4096


def mfcc(waves, sample_rate, config=None, kind="MFCC_0_D_A", dev=None, stride=1):
    """HTK MFCC features of a list of 1-D int16 sample arrays at sample_rate, all in one batched launch sequence.

    config: None (the reference's config_HCopy), a path or a dict from read_hcopy_config.  kind: MFCC_0, MFCC_0_D or MFCC_0_D_A
    (the default: the README's 39 columns).  stride keeps every stride-th frame (frames 0, stride, ...).
    Returns a list of (ceil(n_frames_i / stride), cols) float32 arrays."""
    out, offs, _, _ = _launch(waves, sample_rate, config, kind, dev, stride, lambda u, n: n)
    return [out[offs[u]:offs[u + 1]] for u in range(len(offs) - 1)]


def mfcc_padded(waves, sample_rate, maxlen, stride=5, config=None, kind="MFCC_0_D_A", dev=None):
    """The features of every stride-th frame straight into a zero-padded (B, maxlen, cols) float32 batch (longer utterances are
    truncated), as pad_sequences(padding='post', truncating='post') would make of mfcc(..., stride=stride)."""
    out, _, _, ncols = _launch(waves, sample_rate, config, kind, dev, stride, lambda u, n: maxlen)
    return out.reshape(len(waves), maxlen, ncols)


def kind_code(kind):
    """'MFCC_0_D_A' -> HTK parmKind (6 | 0x2000 | 0x100 | 0x200)."""
    parts = str(kind).upper().split("_")
    if parts[0] not in BASE_KINDS:
        raise ValueError("unknown parameter kind %s" % kind)
    code = BASE_KINDS[parts[0]]
    for q in parts[1:]:
        if q not in QUALIFIERS:
            raise ValueError("unknown qualifier _%s in %s" % (q, kind))
        code |= QUALIFIERS[q]
    return code


def kind_name(code):
    names = {v: k for k, v in BASE_KINDS.items()}
    base = code & 0o77
    if base not in names:
        raise ValueError("unknown parameter kind code %d" % code)
    return "_".join([names[base]] + [q for q, bit in QUALIFIERS.items() if code & bit])


def write_htk(path, feats, samp_period, kind="MFCC_0_D_A"):
    """HTK parameter file (big-endian, uncompressed, no CRC): 12-byte header nSamples, sampPeriod (100 ns units), sampSize (bytes
    per frame), parmKind, then the frames as float32."""
    feats = np.asarray(feats, np.float32)
    if feats.ndim != 2:
        raise ValueError("feats must be (n_frames, cols)")
    code = kind_code(kind) if isinstance(kind, str) else int(kind)
    if code & (QUALIFIERS["C"] | QUALIFIERS["K"]):
        raise ValueError("compressed (_C) / CRC (_K) HTK files are not written")
    with open(path, "wb") as f:
        f.write(struct.pack(">iihh", feats.shape[0], int(samp_period), 4 * feats.shape[1], code))
        f.write(feats.astype(">f4").tobytes())


def read_htk(path):
    """An uncompressed HTK parameter file -> (feats float32 (n, cols), sampPeriod, kind name).  _C / _K files are refused."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12:
        raise ValueError("%s: shorter than an HTK header" % path)
    n, period, size, code = struct.unpack(">iihh", data[:12])
    code &= 0xFFFF
    if code & (QUALIFIERS["C"] | QUALIFIERS["K"]):
        raise ValueError("%s: compressed (_C) or CRC (_K) HTK files are not supported" % path)
    if n < 0 or size <= 0 or size % 4 or len(data) - 12 < n * size:
        raise ValueError("%s: bad or truncated HTK file (nSamples %d, sampSize %d, %d data bytes)" % (path, n, size, len(data) - 12))
    feats = np.frombuffer(data[12:12 + n * size], ">f4").astype(np.float32).reshape(n, size // 4)
    return feats, period, kind_name(code)


def write_audio_csv(path, feats, file_number):
    """The per-file CSV datagen.CsvStore reads (columns '0'..'38' and file_number).  Values are written as the shortest decimal
    of the f32 value's float64: a correctly rounded parser gives it back exactly, pandas' default parser to within its last bit,
    which rounds back to the same f32 value."""
    feats = np.asarray(feats, np.float32)
    cols = feats.shape[1]
    with open(path, "w") as f:
        f.write(",".join([str(i) for i in range(cols)] + ["file_number"]) + "\n")
        for row in feats.astype(np.float64):
            f.write(",".join(repr(float(v)) for v in row) + ",%d\n" % int(file_number))
