"""TEST INFRASTRUCTURE ONLY - numpy restatement of the reference's activity step (skeletal_network/load_skeleton.py, velocity.py,
r_position.py, extract_activity_feats.py, gather_skeletal.py), independent of the product: a per-cell Python parse, exact integer
square roots, numpy's float64 mean and median as pandas computes them, int() truncation."""
import csv
import io
import math
import re

import numpy as np

RAW_COLS = ['hip_center', 'shoulder_center', 'left_shoulder', 'left_elbow', 'left_wrist', 'left_hand', 'right_shoulder',
            'right_elbow', 'right_wrist', 'right_hand']
JOINT_COLS = ['hipX', 'hipY', 'shcX', 'shcY', 'lsX', 'lsY', 'leX', 'leY', 'lwX', 'lwY', 'lhX', 'lhY', 'rsX', 'rsY', 'reX', 'reY',
              'rwX', 'rwY', 'rhX', 'rhY']
FRAME_COLS = ['frame'] + JOINT_COLS
ACTIVITY_COLS = ['lh_v', 'rh_v', 'low_velocity', 'lh_dist_rp', 'rh_dist_rp']
LH, RH = JOINT_COLS.index('lhX'), JOINT_COLS.index('rhX')


def parse_text(text):
    """import_data on the CSV text -> (n, 21) int64 in FRAME_COLS order."""
    rows = list(csv.reader(io.StringIO(text)))
    head = rows[0]
    idx = [head.index(c) for c in RAW_COLS]
    out = np.zeros((len(rows) - 1, len(FRAME_COLS)), np.int64)
    for r, row in enumerate(rows[1:]):
        out[r, 0] = int(row[0])
        for j, c in enumerate(idx):
            t = row[c].strip('[').strip(']').split()
            x, y = int(t[0]), int(t[1])
            out[r, 1 + 2 * j] = 320 if x >= 640 else x
            out[r, 2 + 2 * j] = 240 if y >= 480 else y
    return out


def isqrt_rows(d2):
    return np.array([math.isqrt(int(v)) for v in d2], np.int64)


def velocities(J):
    """(n, 20) joints -> (n, 2) int64 lh_v, rh_v (rows 0..3 zero)."""
    J = np.asarray(J, np.int64)
    v = np.zeros((J.shape[0], 2), np.int64)
    if J.shape[0] > 4:
        for k, c in enumerate((LH, RH)):
            d = J[4:, c:c + 2] - J[3:-1, c:c + 2]
            v[4:, k] = isqrt_rows((d * d).sum(axis=1))
    return v


def rest_position(J, v):
    """-> (low (n,) bool, rp (16,) int64 or None when no frame is low)."""
    J = np.asarray(J, np.int64)
    if J.shape[0] == 0:
        return np.zeros(0, bool), None
    low = (v[:, 0] < v[:, 0].astype(np.float64).mean()) & (v[:, 1] < v[:, 1].astype(np.float64).mean())
    if not low.any():
        return low, None
    return low, np.array([int(np.median(J[low, c].astype(np.float64))) for c in range(4, 20)], np.int64)


def distances(J, rp):
    J = np.asarray(J, np.int64)
    d = np.zeros((J.shape[0], 2), np.int64)
    if J.shape[0] > 4:
        for k, c in enumerate((LH, RH)):
            e = J[4:, c:c + 2] - np.asarray(rp, np.int64)[c - 4:c - 2]
            d[4:, k] = isqrt_rows((e * e).sum(axis=1))
    return d


def activity(J, rest=None):
    """One file: (out (n, 5) int64 lh_v rh_v low lh_dist_rp rh_dist_rp, rp, status) as mgr_skeletal_activity defines them."""
    v = velocities(J)
    low, rp = rest_position(J, v)
    status = 0 if rp is not None else 1
    if rest is not None:
        rp = np.asarray(rest, np.int64)
    d = distances(J, rp) if rp is not None else np.zeros((len(v), 2), np.int64)
    out = np.concatenate([v, low.astype(np.int64)[:, None], d], axis=1)
    return out, (rp if rp is not None else np.zeros(16, np.int64)), status


def gather(tables, split=403):
    """gather_skeletal.load_data over {file name: DataFrame}: sorted by name, int file_number, train <= split < val."""
    import pandas as pd
    parts = []
    for name in sorted(tables):
        n = int(re.fullmatch(r'Sample(\d+)_data\.csv', name).group(1))
        df = tables[name].copy()
        df['file_number'] = n
        parts.append((n, df))
    sel = [[df for n, df in parts if split is None or n <= split], [df for n, df in parts if split is not None and n > split]]
    cat = [pd.concat(s, ignore_index=True) if s else None for s in sel]
    return cat[0] if split is None else tuple(cat)


def activity_table(frames, out):
    """The per-file activity table (FRAME_COLS + ACTIVITY_COLS) of a parsed file and its activity outputs."""
    import pandas as pd
    df = pd.DataFrame({c: frames[:, k] for k, c in enumerate(FRAME_COLS)}, columns=FRAME_COLS)
    for k, c in enumerate(ACTIVITY_COLS):
        df[c] = out[:, k].astype(bool) if c == 'low_velocity' else out[:, k]
    return df
