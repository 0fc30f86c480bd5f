"""The skeletal network's inputs from the raw Kinect joint files (reference skeletal_network/load_skeleton.py, velocity.py,
r_position.py, extract_activity_feats.py, gather_skeletal.py).

The reference's activity step parses one ``SampleNNNNN_data.csv`` per video, adds the integer hand velocities ``lh_v`` / ``rh_v``,
the ``low_velocity`` flag, a per-file hand rest position (the medians of the low-velocity frames) and each hand's distance from it
(``lh_dist_rp`` / ``rh_dist_rp``), and skips a file without low-velocity frames; gather_skeletal concatenates the files into the train
(file number <= 403) and validation tables that skeletal_feature_extraction turns into ``Training_set_skeletal.csv`` /
``Validation_set_skeletal.csv``.  Here the parse is vectorised on the host and the arithmetic is one HIP launch over a ragged batch
of files (``mgr_skeletal_activity``, integer exact).  Where the parse differs from the reference: a cell with more than two numbers
is refused (the reference silently ignores the third), as are NaN cells, non-integers and fewer than two numbers (the reference
raises an unnamed TypeError / ValueError / IndexError), and coordinates outside +-2^20 after the clamps.
"""
import argparse
import os
import re

import numpy as np

from .. import _capi

RAW_COLS = ['hip_center', 'shoulder_center', 'left_shoulder', 'left_elbow', 'left_wrist', 'left_hand', 'right_shoulder',
            'right_elbow', 'right_wrist', 'right_hand']
JOINT_COLS = ['hipX', 'hipY', 'shcX', 'shcY', 'lsX', 'lsY', 'leX', 'leY', 'lwX', 'lwY', 'lhX', 'lhY', 'rsX', 'rsY', 'reX', 'reY',
              'rwX', 'rwY', 'rhX', 'rhY']
FRAME_COLS = ['frame'] + JOINT_COLS
REST_COLS = JOINT_COLS[4:]                  # the rest position rp: ls, le, lw, lh, rs, re, rw, rh x X / Y
ACTIVITY_COLS = ['lh_v', 'rh_v', 'low_velocity', 'lh_dist_rp', 'rh_dist_rp']
FILE_PATTERN = r'Sample(\d+)_data\.csv'
SPLIT = 403                                 # gather_skeletal: file number <= 403 is the training set
COORD_LIMIT = 1 << 20                       # |coordinate| bound: squares and sums stay exact in int64 and fp64
MAX_FILES_PER_LAUNCH = 65536                # include/mgr.h MGR_ACTIVITY_MAX_FILES
MAX_FRAMES_PER_LAUNCH = 1 << 26             # include/mgr.h MGR_ACTIVITY_MAX_FRAMES

# a cell the reference reads: strip('[') then strip(']') leave two whitespace-separated integers (ASCII digits, at most 12)
_CELL = r'\[*\]*[ \t]*([+-]?[0-9]{1,12})[ \t]+([+-]?[0-9]{1,12})[ \t]*\]*\[*'
_CELLS = re.compile('^' + _CELL + '$', re.M)
_ONE = re.compile(_CELL)
_DEV = [None]


def _device():
    if _DEV[0] is None:
        _DEV[0] = _capi.Device(0)
    return _DEV[0]


# -- parsing ------------------------------------------------------------------------------------------------------------------------
def _parse_cells(cells):
    """cells (sequence of str) -> ((n, 2) int64 raw x / y, None), or (None, index of the first malformed cell).  One regex pass
    over the joined cells; the per-cell check runs only to name a malformed cell."""
    cells = list(cells)
    if not cells:
        return np.zeros((0, 2), np.int64), None
    if all(isinstance(c, str) for c in cells):
        m = _CELLS.findall('\n'.join(cells))
        if len(m) == len(cells):
            return np.array(m, dtype=np.int64).reshape(-1, 2), None
    for k, c in enumerate(cells):
        if not isinstance(c, str) or not _ONE.fullmatch(c):
            return None, k
    return None, 0   # a cell spanning lines (a quoted newline): the joined pass miscounts


def _clamp(xy, where, cells, rows):
    x, y = xy[:, 0].copy(), xy[:, 1].copy()
    x[x >= 640] = 320
    y[y >= 480] = 240
    out = (np.abs(x) > COORD_LIMIT) | (np.abs(y) > COORD_LIMIT)
    if out.any():
        k = int(np.flatnonzero(out)[0])
        raise ValueError("%s, row %d: coordinate %r outside +-2^20" % (where(k), k % rows, cells[k]))
    return x, y


def modify_array(arr, where="cells"):
    """(load_skeleton.py:5-19) the joint cells "[x y]" -> (x, y) int64 arrays with x >= 640 -> 320 and y >= 480 -> 240 (each axis on
    its own; negative values kept).  A malformed cell raises ValueError naming ``where`` and its row."""
    cells = list(arr)
    xy, bad = _parse_cells(cells)
    if xy is None:
        raise ValueError("%s, row %d: malformed joint cell %r (need exactly two integers, \"[x y]\")" % (where, bad, cells[bad]))
    return _clamp(xy, lambda k: where, cells, max(len(cells), 1))


def import_data(sk_data_path, data_file):
    """(load_skeleton.py:28-59) one raw joint file -> DataFrame frame, hipX .. rhY (FRAME_COLS, int64)."""
    import pandas as pd
    path = os.path.join(sk_data_path, data_file)
    raw = pd.read_csv(path, dtype={c: object for c in RAW_COLS})
    missing = [c for c in ['Unnamed: 0'] + RAW_COLS if c not in raw.columns]
    if missing:
        raise ValueError("%s: no column %s" % (path, ", ".join(missing)))
    frame = pd.to_numeric(raw['Unnamed: 0'], errors='coerce')
    bad = (frame.isna() | (frame != np.floor(frame))).to_numpy()
    if bad.any():
        raise ValueError("%s, row %d, column 'Unnamed: 0': not an integer frame number" % (path, int(np.flatnonzero(bad)[0])))
    n = len(raw)
    cells = raw[RAW_COLS].to_numpy().T.ravel()           # column by column
    xy, k = _parse_cells(cells)
    if xy is None:
        raise ValueError("%s, row %d, column %s: malformed joint cell %r (need exactly two integers, \"[x y]\")"
                         % (path, k % n, RAW_COLS[k // n], cells[k]))
    x, y = _clamp(xy, lambda k: "%s, column %s" % (path, RAW_COLS[k // n]), cells, max(n, 1))
    cols = {'frame': frame.to_numpy().astype(np.int64)}
    for j in range(len(RAW_COLS)):
        cols[JOINT_COLS[2 * j]], cols[JOINT_COLS[2 * j + 1]] = x[j * n:(j + 1) * n], y[j * n:(j + 1) * n]
    return pd.DataFrame(cols, columns=FRAME_COLS)


# -- the kernel ---------------------------------------------------------------------------------------------------------------------
def activity_arrays(joints, rest=None, dev=None):
    """joints: list of (n_i, 20) integer arrays in JOINT_COLS order (clamped, within +-2^20).  Returns (out, rp, status): out a list
    of (n_i, 5) int32 = lh_v rh_v low lh_dist_rp rh_dist_rp, rp (files, 16) int32 (REST_COLS order), status (files,) int32 (0 ok,
    1 no low-velocity frame: rest and distances 0 unless ``rest`` was given).  rest (files, 16): use it instead of estimating it.
    All files go through the GPU in launches of at most MAX_FILES_PER_LAUNCH files / MAX_FRAMES_PER_LAUNCH frames."""
    dev = dev or _device()
    mats = []
    for k, j in enumerate(joints):
        j = np.asarray(j)
        if j.ndim != 2 or j.shape[1] != len(JOINT_COLS):
            raise ValueError("file %d: joints must be (frames, %d)" % (k, len(JOINT_COLS)))
        if j.size and (not np.issubdtype(j.dtype, np.integer) or np.abs(j.astype(np.int64)).max() > COORD_LIMIT):
            raise ValueError("file %d: joints must be integers within +-2^20" % k)
        if j.shape[0] > MAX_FRAMES_PER_LAUNCH:
            raise ValueError("file %d: %d frames, more than %d" % (k, j.shape[0], MAX_FRAMES_PER_LAUNCH))
        mats.append(np.ascontiguousarray(j, dtype=np.int32))
    nf = len(mats)
    if rest is not None:
        rest = np.ascontiguousarray(rest, dtype=np.int64)
        if rest.shape != (nf, len(REST_COLS)):
            raise ValueError("rest must be (%d, %d)" % (nf, len(REST_COLS)))
        if nf and np.abs(rest).max() > COORD_LIMIT:
            raise ValueError("rest position outside +-2^20")
        rest = rest.astype(np.int32)
    outs, rp, status = [None] * nf, np.zeros((nf, len(REST_COLS)), np.int32), np.zeros(nf, np.int32)
    start = 0
    while start < nf:
        end, total = start, 0
        while end < nf and end - start < MAX_FILES_PER_LAUNCH and total + mats[end].shape[0] <= MAX_FRAMES_PER_LAUNCH:
            total += mats[end].shape[0]
            end += 1
        offs = np.zeros(end - start + 1, np.int64)
        offs[1:] = np.cumsum([m.shape[0] for m in mats[start:end]])
        J = np.concatenate(mats[start:end]) if total else np.zeros((0, len(JOINT_COLS)), np.int32)
        dJ = dev.array(J)
        dO = dev.empty((total, len(ACTIVITY_COLS)), np.int32)
        dOff = dev.array(offs)
        dR = dev.array(rest[start:end]) if rest is not None else dev.empty((end - start, len(REST_COLS)), np.int32)
        dS = dev.empty((end - start,), np.int32)
        try:
            dev.call("mgr_skeletal_activity", dJ, dOff, end - start, total, 1 if rest is not None else 0, dR, dO, dS)
            O, R, S = dO.download(), dR.download(), dS.download()
        finally:
            for a in (dJ, dO, dOff, dR, dS):
                a.free()
        for k in range(start, end):
            outs[k] = O[offs[k - start]:offs[k - start + 1]]
        rp[start:end], status[start:end] = R, S
        start = end
    return outs, rp, status


def _joints(df):
    return np.stack([np.asarray(df[c]) for c in JOINT_COLS], axis=1) if len(df) else np.zeros((0, len(JOINT_COLS)), np.int64)


def _one(df, rest=None):
    out, rp, st = activity_arrays([_joints(df)], None if rest is None else np.asarray(rest).reshape(1, -1))
    return out[0], rp[0], int(st[0])


# -- the reference's per-file functions ---------------------------------------------------------------------------------------------
def calculate_hand_velocities(df):
    """(velocity.py:7-27) lh_v, rh_v: int(euclidean(previous, current)) of the hands, 0 in rows 0..3 (by position)."""
    out, _, _ = _one(df)
    df['lh_v'] = out[:, 0].astype(np.int64)
    df['rh_v'] = out[:, 1].astype(np.int64)
    return df


def estimate_rest_position(df):
    """(r_position.py:8-21) -> (df with low_velocity, rp): rp the 16 int(median) of lsX .. rhY over the frames where both hands are
    slower than their mean.  No such frame: ValueError, as int(NaN) raises in the reference (whose caller then skips the file).
    The velocities are the kernel's; df's own lh_v / rh_v, if present, must equal them."""
    out, rp, st = _one(df)
    for k, c in enumerate(('lh_v', 'rh_v')):
        if c in df.columns and not np.array_equal(np.asarray(df[c]), out[:, k]):
            raise ValueError("%s differs from calculate_hand_velocities' values" % c)
    df['low_velocity'] = out[:, 2].astype(bool)
    if st != 0:
        raise ValueError("no low-velocity frame: the rest position is undefined (cannot convert float NaN to integer)")
    return df, tuple(int(v) for v in rp)


def calc_distance_from_rp(df, rp):
    """(r_position.py:27-46) lh_dist_rp, rh_dist_rp: int(euclidean(rp hand, hand)), 0 in rows 0..3; rp any 16 integers."""
    rp = np.asarray(rp, np.int64).reshape(-1)
    if rp.shape != (len(REST_COLS),):
        raise ValueError("rp must hold 16 values")
    out, _, _ = _one(df, rest=rp)
    df['lh_dist_rp'] = out[:, 3].astype(np.int64)
    df['rh_dist_rp'] = out[:, 4].astype(np.int64)
    return df


# -- whole directories --------------------------------------------------------------------------------------------------------------
def joint_files(sk_data_path):
    """The raw joint files of a directory, sorted by name (the reference's order)."""
    return [n for n in sorted(os.listdir(sk_data_path)) if re.fullmatch(FILE_PATTERN, n)]


def extract_activity(sk_data_path, out_path=None, dev=None):
    """extract_activity_feats.py for every SampleNNNNN_data.csv of sk_data_path in one batch: returns (tables, skipped), tables a
    dict file name -> DataFrame (FRAME_COLS + ACTIVITY_COLS, sorted by name) and skipped the names of the files without a
    low-velocity frame (the reference's bare ``except: continue``).  out_path: also write each table there as <name>, index=False."""
    names = joint_files(sk_data_path)
    frames = [import_data(sk_data_path, n) for n in names]
    out, _, status = activity_arrays([_joints(df) for df in frames], dev=dev)
    tables, skipped = {}, []
    for name, df, o, st in zip(names, frames, out, status):
        if st != 0:
            skipped.append(name)
            continue
        df['lh_v'] = o[:, 0].astype(np.int64)
        df['rh_v'] = o[:, 1].astype(np.int64)
        df['low_velocity'] = o[:, 2].astype(bool)
        df['lh_dist_rp'] = o[:, 3].astype(np.int64)
        df['rh_dist_rp'] = o[:, 4].astype(np.int64)
        tables[name] = df
    if out_path is not None:
        os.makedirs(out_path, exist_ok=True)
        for name, df in tables.items():
            df.to_csv(os.path.join(out_path, name), index=False)
    return tables, skipped


def load_data(path_or_tables, split=SPLIT):
    """(gather_skeletal.py:10-43) concatenate the per-file activity tables in file-name order with an int64 ``file_number`` column:
    (train, val) = (file number <= split, > split), or one table when split is None (the reference's final_data.csv).
    path_or_tables: a directory of activity CSVs or extract_activity's dict."""
    import pandas as pd
    if isinstance(path_or_tables, (str, os.PathLike)):
        tables = {n: pd.read_csv(os.path.join(path_or_tables, n)) for n in joint_files(path_or_tables)}
    else:
        tables = dict(path_or_tables)
    parts = []
    for name in sorted(tables):
        m = re.fullmatch(FILE_PATTERN, name)
        if not m:
            raise ValueError("%s is not a SampleNNNNN_data.csv name" % name)
        df = tables[name].copy()
        df['file_number'] = np.int64(int(m.group(1)))
        parts.append((int(m.group(1)), df))

    def cat(sel):
        if not sel:
            return pd.DataFrame({c: pd.Series(dtype=(bool if c == 'low_velocity' else np.int64))
                                 for c in FRAME_COLS + ACTIVITY_COLS + ['file_number']})
        return pd.concat(sel, ignore_index=True)
    if split is None:
        return cat([df for _, df in parts])
    return cat([df for n, df in parts if n <= split]), cat([df for n, df in parts if n > split])


def skeletal_tables(sk_data_path, split=SPLIT, dev=None):
    """Raw joint files -> the reference's final skeletal tables: extract_activity, load_data, then skeletal_feature_extraction's
    extract_features on each gathered table (its previous-frame shift crosses file boundaries; it overwrites lh_v / rh_v in place
    with its own velocities).  Returns (train, val), or one table when split is None."""
    from . import skeletal_feature_extraction as sfe
    tables, _ = extract_activity(sk_data_path, dev=dev)
    got = load_data(tables, split)
    if split is None:
        return sfe.extract_features(got)
    return tuple(sfe.extract_features(t) for t in got)


def main(argv=None):
    ap = argparse.ArgumentParser(description="raw Kinect joint files -> Training_set_skeletal.csv / Validation_set_skeletal.csv")
    ap.add_argument("--in", dest="inp", required=True, help="directory of SampleNNNNN_data.csv joint files")
    ap.add_argument("--out", required=True, help="output directory")
    ap.add_argument("--split", type=int, default=SPLIT, help="last file number of the training set (default 403)")
    ap.add_argument("--activity-dir", default=None, help="also write the per-file activity CSVs here")
    a = ap.parse_args(argv)
    from . import skeletal_feature_extraction as sfe
    tables, skipped = extract_activity(a.inp, a.activity_dir)
    for name in skipped:
        print("skipped %s: no low-velocity frame" % name)
    train, val = load_data(tables, a.split)
    os.makedirs(a.out, exist_ok=True)
    written = []
    for df, name in ((train, "Training_set_skeletal.csv"), (val, "Validation_set_skeletal.csv")):
        path = os.path.join(a.out, name)
        sfe.extract_features(df).to_csv(path, index=False)
        written.append(path)
        print(path)
    return written
