"""Writes tests/golden/activity_small.npz: a few raw Kinect joint files (their CSV text) and what the reference's activity step makes
of them - load_skeleton.import_data, velocity.calculate_hand_velocities, r_position.estimate_rest_position and calc_distance_from_rp,
called as its extract_activity_feats.py calls them (a file whose rest position raises is skipped).

    python tests/golden/make_activity_fixture.py <directory holding the reference's load_skeleton.py, velocity.py, r_position.py>

The reference modules are imported from that directory (they parse under Python 3; pandas >= 1 needs the one shim below, for
load_skeleton's Series.as_matrix).  Nothing of them is copied; the fixture holds the inputs and their recorded outputs only.
"""
import os
import sys
import tempfile

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
RAW_COLS = ['hip_center', 'shoulder_center', 'left_shoulder', 'left_elbow', 'left_wrist', 'left_hand', 'right_shoulder',
            'right_elbow', 'right_wrist', 'right_hand']
FRAME_COLS = ['frame', 'hipX', 'hipY', 'shcX', 'shcY', 'lsX', 'lsY', 'leX', 'leY', 'lwX', 'lwY', 'lhX', 'lhY', 'rsX', 'rsY', 'reX',
              'reY', 'rwX', 'rwY', 'rhX', 'rhY']
LH, RH = 5, 9      # joint index of left_hand / right_hand in RAW_COLS


def csv_text(P):
    """P (n, 10, 2) int: the raw layout (an unnamed index column, "[x y]" cells)."""
    lines = [',' + ','.join(RAW_COLS)]
    for i, row in enumerate(P):
        lines.append('%d,' % i + ','.join('[%d %d]' % (x, y) for x, y in row))
    return '\n'.join(lines) + '\n'


def walk(rng, n, step=6, base=(300, 200)):
    P = np.zeros((n, 10, 2), np.int64)
    P[:] = np.array(base) + rng.integers(-40, 40, (1, 10, 2))
    P[:, LH] += np.cumsum(rng.integers(-step, step + 1, (n, 2)), axis=0)
    P[:, RH] += np.cumsum(rng.integers(-step, step + 1, (n, 2)), axis=0)
    return P


def cases():
    rng = np.random.default_rng(20131904)
    out = {}
    out['Sample00398_data.csv'] = np.zeros((0, 10, 2), np.int64)              # empty: skipped
    out['Sample00399_data.csv'] = walk(rng, 3)                                 # <= 4 frames: every velocity 0, skipped
    out['Sample00400_data.csv'] = walk(rng, 4)
    P = walk(rng, 5)                                                           # 5 frames: rows 0..3 low, an even count
    P[:4, 2] = [[-3, 7], [-4, 8], [-5, 9], [-2, 10]]                           # left shoulder X: median of -3, -4 -> -3.5 -> -3
    P[4, LH] = P[3, LH] + [3, 4]                                               # a 3-4-5 step: lh_v = 5 exactly
    P[4, RH] = P[3, RH] + [6, 8]
    out['Sample00401_data.csv'] = P
    P = walk(rng, 6)                                                           # 6 frames with a perfect-square step and clamps
    P[5, LH] = P[4, LH] + [-3, -4]
    P[2:, 0] = [[700, 500], [640, 479], [639, 480], [-20, 900]]                # hip: x >= 640 -> 320, y >= 480 -> 240, each on its own
    out['Sample00403_data.csv'] = P
    P = walk(rng, 9, step=0)                                                   # hands never move: constant velocity 0, skipped
    out['Sample00405_data.csv'] = P
    P = walk(rng, 12)                                                          # right hand still: no frame below its mean, skipped
    P[:, RH] = P[0, RH]
    out['Sample00406_data.csv'] = P
    P = walk(rng, 41, step=9, base=(40, 30))                                   # negative coordinates, clamped hands, odd / even counts
    P[10:14, LH] = [[650, 100], [-7, 481], [700, 700], [-12, -9]]
    out['Sample00404_data.csv'] = P
    P = walk(rng, 30, step=4)
    P[:, 4] -= 400                                                             # left wrist at negative x
    out['Sample00410_data.csv'] = P
    return out


def main(ref_dir):
    sys.path.insert(0, ref_dir)
    if not hasattr(pd.Series, 'as_matrix'):
        pd.Series.as_matrix = pd.Series.to_numpy
    import load_skeleton
    import r_position
    import velocity
    z = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, (name, P) in enumerate(sorted(cases().items())):
            text = csv_text(P)
            with open(os.path.join(tmp, name), 'w') as f:
                f.write(text)
            z['name_%d' % k] = np.array(name)
            z['raw_%d' % k] = np.array(text)
            df = load_skeleton.import_data(tmp, name)
            assert list(df.columns) == FRAME_COLS, list(df.columns)
            z['frames_%d' % k] = df[FRAME_COLS].to_numpy(dtype=np.int64).reshape(-1, len(FRAME_COLS))
            df = velocity.calculate_hand_velocities(df)
            z['vel_%d' % k] = df[['lh_v', 'rh_v']].to_numpy(dtype=np.int64).reshape(-1, 2)
            try:
                df, rp = r_position.estimate_rest_position(df)
            except ValueError:
                z['status_%d' % k] = np.int32(1)
                continue
            z['status_%d' % k] = np.int32(0)
            z['low_%d' % k] = df['low_velocity'].to_numpy(dtype=bool)
            z['rp_%d' % k] = np.array(rp, np.int64)
            df = r_position.calc_distance_from_rp(df, rp)
            z['dist_%d' % k] = df[['lh_dist_rp', 'rh_dist_rp']].to_numpy(dtype=np.int64).reshape(-1, 2)
            print(name, len(P), 'skipped' if z['status_%d' % k] else rp)
    z['n_files'] = np.int32(len(cases()))
    path = os.path.join(HERE, 'activity_small.npz')
    np.savez_compressed(path, **z)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
