"""fp64 numpy restatement of HTK HCopy's MFCC_0_D_A front-end, independent of the product: its own filterbank table,
its own radix-2 FFT (a full complex transform of the zero-padded real frame), plain loops in HTK's order where order matters."""
import numpy as np


def frame_params(sample_rate, window=250000, target=100000):
    frame_size = window * sample_rate // 10 ** 7
    frame_rate = target * sample_rate // 10 ** 7
    assert frame_size * 10 ** 7 == window * sample_rate and frame_rate * 10 ** 7 == target * sample_rate
    fft_n = 1
    while fft_n < frame_size:
        fft_n *= 2
    return frame_size, frame_rate, fft_n


def fft(x):
    """Radix-2 decimation-in-time FFT along the last axis (length a power of two), fp64 complex."""
    x = np.asarray(x, np.complex128)
    n = x.shape[-1]
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(n)]) if bits else np.zeros(1, int)
    a = x[..., rev].copy()
    span = 1
    while span < n:
        w = np.exp(-2j * np.pi * np.arange(span) / (2 * span))
        a = a.reshape(a.shape[:-1] + (n // (2 * span), 2, span))
        even, odd = a[..., 0, :], a[..., 1, :] * w
        a = np.concatenate([even + odd, even - odd], axis=-1).reshape(x.shape)
        span *= 2
    return a


def filterbank(sample_rate, fft_n, num_chans):
    """HTK's (loChan, loWt) per bin, 1-based arrays of length fftN/2 + 1 as in HSigP (index 0 unused)."""
    half = fft_n // 2
    fres = 1e7 / ((1e7 / sample_rate) * fft_n * 700.0)

    def mel(k):
        return 1127.0 * np.log(1.0 + (k - 1) * fres)

    klo, khi, mlo, mhi = 2, half, 0.0, mel(half + 1)
    max_chan = num_chans + 1
    cf = [0.0] + [c / max_chan * (mhi - mlo) + mlo for c in range(1, max_chan + 1)]
    lo_chan = [-1] * (half + 1)
    lo_wt = [0.0] * (half + 1)
    chan = 1
    for k in range(1, half + 1):
        if klo <= k <= khi:
            while chan <= max_chan and cf[chan] < mel(k):
                chan += 1
            lo_chan[k] = chan - 1
    for k in range(1, half + 1):
        c = lo_chan[k]
        if klo <= k <= khi:
            lo_wt[k] = (cf[c + 1] - mel(k)) / (cf[c + 1] - cf[c]) if c > 0 else (cf[1] - mel(k)) / (cf[1] - mlo)
    return np.array(lo_chan), np.array(lo_wt)


def magnitudes(samples, sample_rate, preemph=0.97):
    """(n_frames, fftN/2) |X_k| of the pre-emphasised, Hamming-windowed, zero-padded frames (bins 1..fftN/2 of HTK)."""
    frame_size, frame_rate, fft_n = frame_params(sample_rate)
    s = np.asarray(samples, np.float64)
    n = (s.size - frame_size) // frame_rate + 1 if s.size >= frame_size else 0
    fr = np.stack([s[t * frame_rate:t * frame_rate + frame_size] for t in range(n)]) if n else np.zeros((0, frame_size))
    pe = fr.copy()
    pe[:, 1:] = fr[:, 1:] - preemph * fr[:, :-1]
    pe[:, 0] = fr[:, 0] * (1.0 - preemph)
    i = np.arange(frame_size)
    pe *= 0.54 - 0.46 * np.cos(2 * np.pi * i / (frame_size - 1))
    pad = np.zeros((n, fft_n))
    pad[:, :frame_size] = pe
    return np.abs(fft(pad))[:, :fft_n // 2]


def statics(samples, sample_rate, num_chans=26, num_ceps=12, lifter=22, preemph=0.97):
    """(n_frames, num_ceps + 1) fp64: C1..C12, C0."""
    mag = magnitudes(samples, sample_rate, preemph)
    _, _, fft_n = frame_params(sample_rate)
    lo_chan, lo_wt = filterbank(sample_rate, fft_n, num_chans)
    fb = np.zeros((mag.shape[0], num_chans + 1))
    for k in range(2, fft_n // 2 + 1):          # HTK's accumulation order: ascending bins
        c, ek = lo_chan[k], mag[:, k - 1]
        if c > 0:
            fb[:, c] += lo_wt[k] * ek
        if c < num_chans:
            fb[:, c + 1] += (1.0 - lo_wt[k]) * ek
    fb = np.log(np.maximum(fb[:, 1:], 1.0))
    norm = np.sqrt(2.0 / num_chans)
    k = np.arange(1, num_chans + 1)
    out = np.zeros((mag.shape[0], num_ceps + 1))
    for j in range(1, num_ceps + 1):
        c = (fb * np.cos(j * np.pi * (k - 0.5) / num_chans)).sum(axis=1) * norm
        out[:, j - 1] = c * (1.0 + lifter / 2.0 * np.sin(j * np.pi / lifter)) if lifter > 0 else c
    out[:, num_ceps] = fb.sum(axis=1) * norm
    return out


def deltas(x, window=2):
    """HTK regression deltas along frames, first / last frame replicated at the ends."""
    n = x.shape[0]
    if n == 0:
        return np.zeros_like(x)
    t = np.arange(n)
    den = 2.0 * sum(th * th for th in range(1, window + 1))
    acc = 0.0
    for th in range(1, window + 1):
        acc = acc + th * (x[np.minimum(t + th, n - 1)] - x[np.maximum(t - th, 0)])
    return acc / den


def mfcc_0_d_a(samples, sample_rate, **kw):
    """(n_frames, 39) fp64 in HTK column order."""
    st = statics(samples, sample_rate, **kw)
    d = deltas(st)
    return np.concatenate([st, d, deltas(d)], axis=1)
