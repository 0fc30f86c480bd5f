"""-m "not gpu": the skeletal activity step's host side - the numpy restatement against the reference's recorded outputs, the
vectorised joint-file parser, gather_skeletal.load_data and CsvStore on a DataFrame."""
import os

import numpy as np
import pandas as pd
import pytest

from tests import activity_ref as ar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activity_small.npz")


def fixture_files():
    z = np.load(GOLDEN)
    return z, [(str(z['name_%d' % k]), str(z['raw_%d' % k])) for k in range(int(z['n_files']))]


def write_raw(tmp_path, files):
    for name, text in files:
        (tmp_path / name).write_text(text)
    return str(tmp_path)


def test_restatement_equals_reference_outputs():
    z, files = fixture_files()
    kinds = {'skipped': 0, 'odd': 0, 'even': 0, 'neg_even_median': 0}
    for k, (name, text) in enumerate(files):
        J = ar.parse_text(text)
        np.testing.assert_array_equal(J, z['frames_%d' % k], err_msg=name)
        out, rp, st = ar.activity(J[:, 1:])
        np.testing.assert_array_equal(out[:, :2], z['vel_%d' % k], err_msg=name)
        assert st == int(z['status_%d' % k]), name
        if st:
            kinds['skipped'] += 1
            continue
        np.testing.assert_array_equal(out[:, 2].astype(bool), z['low_%d' % k], err_msg=name)
        np.testing.assert_array_equal(rp, z['rp_%d' % k], err_msg=name)
        np.testing.assert_array_equal(out[:, 3:], z['dist_%d' % k], err_msg=name)
        cnt = int(out[:, 2].sum())
        kinds['odd' if cnt % 2 else 'even'] += 1
        low = J[out[:, 2].astype(bool), 1:]
        mid = np.sort(low, axis=0)[[(cnt - 1) // 2, cnt // 2]]
        kinds['neg_even_median'] += int(cnt % 2 == 0 and np.any((mid.sum(axis=0) < 0) & (mid.sum(axis=0) % 2 != 0)))
    # the fixture covers what it is for: skipped files of every kind, odd and even low counts, a negative half-integer median
    assert kinds['skipped'] == 5 and kinds['odd'] >= 1 and kinds['even'] >= 1 and kinds['neg_even_median'] >= 1, kinds
    assert any(int(z['vel_%d' % k][:, 0].tolist().count(5)) for k in range(len(files)))   # the 3-4-5 step


def test_parser_equals_reference_parse(tmp_path):
    import mgr_amd  # noqa: F401
    from mgr_amd.skeletal_network import load_skeleton
    z, files = fixture_files()
    d = write_raw(tmp_path, files)
    for k, (name, _) in enumerate(files):
        df = load_skeleton.import_data(d, name)
        assert list(df.columns) == ar.FRAME_COLS
        assert all(df[c].dtype == np.int64 for c in df.columns), df.dtypes
        np.testing.assert_array_equal(df.to_numpy().reshape(-1, 21), z['frames_%d' % k], err_msg=name)
    # the clamps act on each axis on their own; negative values are kept
    x, y = load_skeleton.modify_array(np.array(['[640 479]', '[639 480]', '[700 900]', '[-5 -1048576]', '[[12  7]]'], dtype=object))
    assert x.tolist() == [320, 639, 320, -5, 12] and y.tolist() == [479, 240, 240, -1048576, 7]


@pytest.mark.parametrize("cell,why", [("[1 2 3]", "three numbers"), ("[1]", "one number"), ("[1.5 2]", "not an integer"),
                                      ("", "NaN"), ("[a b]", "not numbers"), ("[-1048577 0]", "outside +-2^20"),
                                      (" [1 2]", "the reference's strip leaves '[1'")])
def test_parser_refuses_malformed_cells(tmp_path, cell, why):
    import mgr_amd  # noqa: F401
    from mgr_amd.skeletal_network import load_skeleton
    cells = ['[%d %d]' % (10 + j, 20 + j) for j in range(10)]
    rows = [',' + ','.join(ar.RAW_COLS)] + ['%d,' % i + ','.join(cells) for i in range(3)]
    bad = cells[:]
    bad[4] = '"%s"' % cell if cell else ''
    rows.append('3,' + ','.join(bad))
    (tmp_path / 'Sample00001_data.csv').write_text('\n'.join(rows) + '\n')
    with pytest.raises(ValueError) as e:
        load_skeleton.import_data(str(tmp_path), 'Sample00001_data.csv')
    msg = str(e.value)
    assert 'Sample00001_data.csv' in msg and 'row 3' in msg and 'left_wrist' in msg, (why, msg)


def test_restated_rest_position_semantics():
    # pandas' median of an even count is the mean of the two middle values, int() truncates toward zero
    J = np.zeros((6, 20), np.int64)
    J[:, 4] = [-3, -4, 9, 9, 0, 0]
    J[5, ar.LH:ar.LH + 2] = [3, 4]
    J[5, ar.RH:ar.RH + 2] = [6, 8]
    out, rp, st = ar.activity(J)
    assert st == 0 and out[:, 2].tolist() == [1, 1, 1, 1, 1, 0] and out[5, :2].tolist() == [5, 10]
    assert rp[0] == 0     # median of -4 -3 0 9 9 -> 0
    J[4, 4] = 9
    J[:5, 4] = [-3, -4, -5, -2, -7]
    _, rp, _ = ar.activity(J)
    assert rp[0] == -4    # odd count: -4 exactly
    J[:, 4] = [-3, -4, -5, -2, 100, 100]
    J[4, ar.LH] = 50      # row 4 moves: 4 low frames
    out, rp, _ = ar.activity(J)
    assert out[:, 2].sum() == 4 and rp[0] == -3     # (-4 + -3) / 2 = -3.5 -> -3


def test_gather_order_split_and_dtypes(tmp_path):
    import mgr_amd  # noqa: F401
    from mgr_amd.skeletal_network import gather_skeletal
    z, files = fixture_files()
    tables = {}
    for k, (name, text) in enumerate(files):
        if int(z['status_%d' % k]):
            continue
        J = ar.parse_text(text)
        out, _, _ = ar.activity(J[:, 1:])
        tables[name] = ar.activity_table(J, out)
    names = sorted(tables)
    # the directory form reads the per-file activity CSVs the reference writes; the dict form takes the tables themselves
    d = tmp_path / 'act'
    d.mkdir()
    for name in reversed(names):
        tables[name].to_csv(d / name, index=False)
    (d / 'notes.txt').write_text('not a joint file')
    for src in (str(d), tables):
        train, val = gather_skeletal.load_data(src)
        assert list(train.columns) == ar.FRAME_COLS + ar.ACTIVITY_COLS + ['file_number']
        assert list(val.columns) == list(train.columns)
        for df in (train, val):
            assert df['low_velocity'].dtype == bool
            assert all(df[c].dtype == np.int64 for c in df.columns if c != 'low_velocity'), df.dtypes
        # file number <= 403 is the training set; files in sorted name order; skipped files are absent
        assert train['file_number'].unique().tolist() == [401, 403]
        assert val['file_number'].unique().tolist() == [404, 410]
        ref_train, ref_val = ar.gather(tables)
        pd.testing.assert_frame_equal(train, ref_train)
        pd.testing.assert_frame_equal(val, ref_val)
        # the split point is a parameter; None gives one table (the reference's final_data.csv)
        tr, va = gather_skeletal.load_data(src, split=404)
        assert tr['file_number'].unique().tolist() == [401, 403, 404] and va['file_number'].unique().tolist() == [410]
        pd.testing.assert_frame_equal(tr, ar.gather(tables, 404)[0])
        pd.testing.assert_frame_equal(va, ar.gather(tables, 404)[1])
        one = gather_skeletal.load_data(src, split=None)
        pd.testing.assert_frame_equal(one, ar.gather(tables, None))
        assert not set(one['file_number']) & {398, 399, 400, 405, 406}


def test_csvstore_takes_a_dataframe(tmp_path):
    import mgr_amd  # noqa: F401
    from mgr_amd import datagen
    rng = np.random.default_rng(7)
    n = 120
    df = pd.DataFrame({c: rng.integers(-50, 600, n) / 4.0 for c in datagen.SKELETAL_COLUMNS})
    df['low_velocity'] = rng.random(n) < 0.5
    df['file_number'] = np.repeat([3, 5, 9], 40)
    p = tmp_path / 'skel.csv'
    df.to_csv(p, index=False)
    labs = tmp_path / 'labs.csv'
    pd.DataFrame({'Id': [3, 5, 9], 'Sequence': ['1 2', '3', '4 5 6']}).to_csv(labs, index=False)
    a = datagen.CsvStore(None, df, str(labs))
    b = datagen.CsvStore(None, str(p), str(labs))
    assert a.file_ids() == b.file_ids() == [3, 5, 9]
    for f in (3, 5, 9):
        np.testing.assert_array_equal(a.features(f, 'skeletal'), b.features(f, 'skeletal'))
        np.testing.assert_array_equal(a.labels(f), b.labels(f))
