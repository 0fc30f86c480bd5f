"""Writes tests/golden/ws_bytes.json: what every mgr_*_ws_bytes query with scalar arguments returns over a grid of shapes.

    python tests/golden/make_ws_bytes.py <libmgr.so of the commit that is the reference> <its commit id>

The queries are pure host functions: the library answers them without a GPU.  tests/test_cpu_ws_layout.py asserts that the library of
the tree returns the recorded values - so the fixture is made from the library of the commit BEFORE a change of the workspace
layouts, never from the code under test.

The grid holds every padding case of the 256-byte blocks (odd sizes, sizes one off a multiple of a tile, the limits) and the shapes
of configs.py at their own batch and length.  The cross product is thinned with a fixed seed: per query, every value of every
dimension is kept at least once, then rows drawn at random up to ROWS_PER_QUERY.
"""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ROWS_PER_QUERY = 28

Bs = [1, 2, 3, 16, 17]
Ts = [1, 31, 32, 33, 40, 1900]
Fs = [16, 20, 39, 64, 65, 72, 127, 128, 130, 2048]
Hs = [4, 20, 32, 64, 100, 128, 250]
Cs = [2, 21, 48, 64]
Ls = [1, 7, 63, 255]
BEAMS = [1, 10, 34]
PADS = [32, 64, 128]          # ldt = T rounded up to one of these
TOPS = [0, 1]                 # top_paths = 1 or beam


def ldt_of(T, pad):
    return (T + pad - 1) // pad * pad


def with_ldt(rows):           # (..., T at index 1, ..., pad) -> (..., ldt)
    return [r[:-1] + (ldt_of(r[1], r[-1]),) for r in rows]


def thin(dims, rng):
    """Rows of the cross product of dims: a cover of every value of every dimension, then random rows up to ROWS_PER_QUERY."""
    rows = []
    for k, vals in enumerate(dims):
        for v in vals:
            r = [d[rng.integers(len(d))] for d in dims]
            r[k] = v
            rows.append(tuple(r))
    full = list(itertools.product(*dims))
    for i in rng.permutation(len(full)):
        if len(rows) >= ROWS_PER_QUERY:
            break
        rows.append(full[i])
    return sorted(set(rows))


def config_rows():
    """(B, T, Lmax, C, D, [(F, H) of every LSTM layer]) of the named configurations."""
    sys.path.insert(0, ROOT)
    import mgr_amd  # noqa: F401
    from mgr_amd.configs import baseline_config
    out = []
    for key in ("A", "A_ref", "S", "S_ref", "F", "E", "F128"):
        spec, B, T, Lmax = baseline_config(key)
        out.append((B, T, Lmax, spec.num_classes, spec.head_width, sorted({(F, H) for _, F, H, _, _ in spec.lstm_layers()})))
    return out


def grid():
    rng = np.random.default_rng(20260256)
    cfg = config_rows()
    layers = sorted({(B, T, F, H) for B, T, _, _, _, fh in cfg for F, H in fh})
    heads = sorted({(B, T, D, C, L) for B, T, L, C, D, _ in cfg})
    q = {}
    q["mgr_lstm_input_proj_dropout_ws_bytes"] = thin([Bs, Fs, Hs], rng) + sorted({(B, F, H) for B, _, F, H in layers})
    q["mgr_lstm_input_proj_dropout_ts_ws_bytes"] = thin([Bs, Fs, Hs], rng) + sorted({(B, F, H) for B, _, F, H in layers}) + [(2, 130, 20)]
    q["mgr_lstm_scan_ws_bytes"] = thin([Bs, Ts, Hs], rng) + sorted({(B, T, H) for B, T, _, H in layers})
    q["mgr_lstm_param_grads_ws_bytes"] = thin([Bs, Ts, Fs, Hs], rng) + layers
    q["mgr_lstm_param_grads_dropout_ws_bytes"] = thin([Bs, Ts, Fs, Hs], rng) + layers
    lay_ldt = [(B, T, F, H, p) for B, T, F, H in layers for p in PADS]
    q["mgr_lstm_param_grads_dropout_t_ws_bytes"] = with_ldt(thin([Bs, Ts, Fs, Hs, PADS], rng) + lay_ldt)
    q["mgr_lstm_param_grads_dropout_ts_ws_bytes"] = with_ldt(thin([Bs, Ts, Fs, Hs, PADS], rng) + lay_ldt) + [(2, 40, 130, 20, 64)]
    q["mgr_dense_bwd_ws_bytes"] = [(B, T, 2 * H, C) for B, T, H, C in thin([Bs, Ts, Hs, Cs], rng)] + [h[:4] for h in heads]
    q["mgr_head_ws_bytes"] = [(B, T, 2 * H, C, L) for B, T, H, C, L in thin([Bs, Ts, Hs, Cs, Ls], rng)] + heads
    btcl = sorted({(B, T, C, L) for B, T, _, C, L in heads})
    q["mgr_ctc_ws_bytes"] = thin([Bs, Ts, Cs, Ls], rng) + btcl
    q["mgr_ctc_align_ws_bytes"] = thin([Bs, Ts, Cs, Ls], rng) + btcl
    btc = sorted({(B, T, C) for B, T, C, _ in btcl})
    q["mgr_ctc_beam_ws_bytes"] = thin([Bs, Ts, Cs, BEAMS], rng) + [r + (w,) for r in btc for w in BEAMS]
    q["mgr_ctc_beam_lm_ws_bytes"] = [(B, T, C, w, w if top else 1) for B, T, C, w, top in
                                     thin([Bs, Ts, Cs, BEAMS, TOPS], rng) + [r + (w, t) for r in btc for w in BEAMS for t in TOPS]]
    q["mgr_edit_distance_ws_bytes"] = thin([[1, 3, 17, 640], [1, 7, 63, 255], [1, 7, 63, 255], [0, 1]], rng)
    q["mgr_conv_pool_bwd_weights_ws_bytes"] = thin([[1, 3, 40, 1900], [60, 28, 12], [60, 28, 12], [1, 16, 32], [4, 5], [16, 32, 48]], rng)
    q["mgr_mfcc_ws_bytes"] = thin([[1, 3, 17], [1, 40, 1900, 100000], [200, 400], [256, 512, 2048], [2, 26, 128], [0, 12, 13]], rng)
    return q


def main(lib_path, commit):
    lib = C.CDLL(os.path.abspath(lib_path))
    rows = []
    for name, argsets in grid().items():
        fn = getattr(lib, name)
        fn.restype = C.c_size_t
        for args in sorted(set(argsets)):
            fn.argtypes = [C.c_longlong if (name == "mgr_mfcc_ws_bytes" and k == 1) else C.c_int for k in range(len(args))]
            rows.append([name, [int(a) for a in args], int(fn(*args))])
    path = os.path.join(HERE, "ws_bytes.json")
    with open(path, "w") as f:
        f.write('{"commit": %s, "rows": [\n' % json.dumps(commit))
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print("wrote", path, len(rows), "rows,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
