"""-m gpu: the skeletal activity kernel (mgr_skeletal_activity) bit-exact against the reference's recorded outputs and the numpy
restatement tests/activity_ref.py, skeletal_tables against the restatement chained with the skeletal feature restatement, and the
gathered table feeding the skeletal, fusion and RGB paths end to end."""
import os

import numpy as np
import pandas as pd
import pytest

from oracle import skeletal_ref as sr
from tests import activity_ref as ar

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "activity_small.npz")


def _act():
    import mgr_amd  # noqa: F401
    from mgr_amd.skeletal_network import activity
    return activity


def _walk(rng, n, step=6, lo=-(1 << 20), hi=1 << 20, base=None):
    J = np.empty((n, 20), np.int64)
    J[:] = rng.integers(-300, 300, (1, 20)) + (0 if base is None else base)
    J += np.cumsum(rng.integers(-step, step + 1, (n, 20)), axis=0) * (rng.random((n, 20)) < 0.7)
    return np.clip(J, lo, hi)


def _check(got, J, rest=None):
    out, rp, st = got
    for k, j in enumerate(J):
        r_out, r_rp, r_st = ar.activity(j, None if rest is None else rest[k])
        assert st[k] == r_st, k
        np.testing.assert_array_equal(out[k], r_out, err_msg="file %d" % k)
        if rest is None:
            np.testing.assert_array_equal(rp[k], r_rp, err_msg="file %d" % k)
        else:
            np.testing.assert_array_equal(rp[k], rest[k])


def test_kernel_equals_reference_outputs(device):
    act = _act()
    z = np.load(GOLDEN)
    n = int(z['n_files'])
    frames = [z['frames_%d' % k] for k in range(n)]
    out, rp, st = act.activity_arrays([f[:, 1:] for f in frames], dev=device)
    for k in range(n):
        np.testing.assert_array_equal(out[k][:, :2], z['vel_%d' % k])
        assert st[k] == z['status_%d' % k], k
        if st[k] == 0:
            np.testing.assert_array_equal(out[k][:, 2].astype(bool), z['low_%d' % k])
            np.testing.assert_array_equal(rp[k], z['rp_%d' % k])
            np.testing.assert_array_equal(out[k][:, 3:], z['dist_%d' % k])
        else:
            assert not out[k][:, 2:].any() and not rp[k].any()


def test_kernel_equals_restatement_on_random_batches(device):
    act = _act()
    rng = np.random.default_rng(11)
    J = [_walk(rng, n) for n in (0, 1, 3, 4, 5, 6, 7)]
    J += [_walk(rng, int(rng.integers(5, 2500)), step=int(rng.integers(0, 12))) for _ in range(300)]
    J[10][:, 10:12] = J[10][0, 10:12]                     # a still left hand: skipped
    J[11][:, 18] = 3 * np.arange(len(J[11]))              # 3-4-5 steps of the right hand: rh_v = 5 exactly
    J[11][:, 19] = 4 * np.arange(len(J[11]))
    # coordinates at the +-2^20 bound: the largest radicands (2^21)^2 + (2^21)^2
    big = _walk(rng, 64, step=0)
    big[::2] = 1 << 20
    big[1::2] = -(1 << 20)
    J.append(big)
    J.append(_walk(rng, 200_000, step=5))                 # one long file: many strided passes per thread
    got = act.activity_arrays(J, dev=device)
    _check(got, J)
    assert sorted(set(got[2].tolist())) == [0, 1]
    # a caller-supplied rest position (r_position.calc_distance_from_rp(df, rp) with any rp)
    rest = rng.integers(-(1 << 20), 1 << 20, (len(J), 16))
    got2 = act.activity_arrays(J, rest=rest, dev=device)
    _check(got2, J, rest)


def test_repeated_launches_are_identical(device):
    act = _act()
    rng = np.random.default_rng(5)
    J = [_walk(rng, int(rng.integers(0, 3000))) for _ in range(120)]
    a = act.activity_arrays(J, dev=device)
    b = act.activity_arrays(J, dev=device)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_reference_named_functions_on_one_file(device, tmp_path):
    act = _act()
    act._DEV[0] = device
    from mgr_amd.skeletal_network import load_skeleton, r_position, velocity
    z = np.load(GOLDEN)
    for k in range(int(z['n_files'])):
        name = str(z['name_%d' % k])
        (tmp_path / name).write_text(str(z['raw_%d' % k]))
        df = velocity.calculate_hand_velocities(load_skeleton.import_data(str(tmp_path), name))
        np.testing.assert_array_equal(df[['lh_v', 'rh_v']].to_numpy().reshape(-1, 2), z['vel_%d' % k])
        if z['status_%d' % k]:
            with pytest.raises(ValueError):
                r_position.estimate_rest_position(df)
            continue
        df, rp = r_position.estimate_rest_position(df)
        assert rp == tuple(z['rp_%d' % k].tolist()) and all(type(v) is int for v in rp)
        np.testing.assert_array_equal(df['low_velocity'].to_numpy(), z['low_%d' % k])
        df = r_position.calc_distance_from_rp(df, rp)
        np.testing.assert_array_equal(df[['lh_dist_rp', 'rh_dist_rp']].to_numpy(), z['dist_%d' % k])
        assert list(df.columns) == ar.FRAME_COLS + ar.ACTIVITY_COLS


def _raw_dir(path, rng, ids, n_lo=30, n_hi=90, skip=()):
    path.mkdir(exist_ok=True)
    for fid in ids:
        n = int(rng.integers(n_lo, n_hi))
        J = _walk(rng, n, step=0 if fid in skip else 7, lo=-50, hi=700, base=300)
        lines = [',' + ','.join(ar.RAW_COLS)]
        lines += ['%d,' % i + ','.join('[%d %d]' % (J[i, 2 * j], J[i, 2 * j + 1]) for j in range(10)) for i in range(n)]
        (path / ('Sample%05d_data.csv' % fid)).write_text('\n'.join(lines) + '\n')
    return str(path)


def _restated_tables(d, split=403):
    tables = {}
    for name in sorted(os.listdir(d)):
        if not name.endswith('_data.csv'):
            continue
        with open(os.path.join(d, name)) as f:
            F = ar.parse_text(f.read())
        out, _, st = ar.activity(F[:, 1:])
        if st == 0:
            tables[name] = ar.activity_table(F, out)
    return ar.gather(tables, split)


def test_skeletal_tables_equal_restatement_chain(device, tmp_path):
    act = _act()
    act._DEV[0] = device
    from mgr_amd.skeletal_network import skeletal_feature_extraction as sfe
    sfe._DEV[0] = device
    rng = np.random.default_rng(23)
    ids = [397, 399, 400, 402, 403, 404, 407, 415]
    d = _raw_dir(tmp_path / 'raw', rng, ids, skip=(400, 407))
    tables, skipped = act.extract_activity(d, out_path=str(tmp_path / 'act'))
    assert skipped == ['Sample00400_data.csv', 'Sample00407_data.csv']
    assert sorted(os.listdir(tmp_path / 'act')) == sorted(tables)
    got = act.skeletal_tables(d)
    refs = _restated_tables(d)
    for g, r in zip(got, refs):
        cols = list(r.columns)
        feats = sr.extract_features({c: r[c].to_numpy(np.float64) for c in sr.JOINT_COLS})
        pre = {}
        for j in ('lh', 'rh', 'le', 're'):
            for ax in ('X', 'Y'):
                pre['pre_' + j + ax] = sr._prev(r[j + ax].to_numpy())
        order = cols + list(pre) + ['le_v', 're_v', 'pre_lh_v', 'pre_rh_v', 'pre_le_v', 'pre_re_v'] + sr.FEATURE_COLS[4:]
        assert list(g.columns) == order
        # integer and boolean columns exact, with the reference's dtypes
        for c in ar.FRAME_COLS + ['low_velocity', 'lh_dist_rp', 'rh_dist_rp', 'file_number'] + list(pre):
            assert g[c].dtype == r[c].dtype if c in r.columns else g[c].dtype == np.int64, c
            np.testing.assert_array_equal(g[c].to_numpy(), r[c].to_numpy() if c in r.columns else pre[c], err_msg=c)
        # float columns: the tolerances of tests/test_gpu_skeletal.py (coordinates < 1024)
        for c in sr.FEATURE_COLS:
            tol = 4e-16 * np.pi if c.endswith('_ang') else (2 if c.endswith('_a') else 1) * 2.0 ** -43
            np.testing.assert_allclose(g[c].to_numpy(), feats[c], rtol=0, atol=tol, err_msg=c)
        for j in ('lh', 'rh', 'le', 're'):
            np.testing.assert_array_equal(g['pre_%s_v' % j].to_numpy(), sr._prev(g['%s_v' % j].to_numpy()))
    assert got[0]['file_number'].unique().tolist() == [397, 399, 402, 403]
    assert got[1]['file_number'].unique().tolist() == [404, 415]
    # the CLI writes the two tables
    written = act.main(['--in', d, '--out', str(tmp_path / 'out')])
    for p, g in zip(written, got):
        back = pd.read_csv(p)
        assert list(back.columns) == list(g.columns)
        assert back['low_velocity'].dtype == bool and back['lh_dist_rp'].dtype == np.int64 and back['hipX'].dtype == np.int64


def test_raw_joints_train_skeletal_fusion_and_rgb_paths(device, tmp_path, monkeypatch):
    act = _act()
    act._DEV[0] = device
    import mgr_amd  # noqa: F401
    from mgr_amd import datagen
    from mgr_amd.audio_network import feature_extraction as fe
    from mgr_amd.multimodal_fusion import data_generator as fdg
    from mgr_amd.multimodal_fusion import multimodal
    from mgr_amd.rgb_network import roi_extraction as roi
    from mgr_amd.skeletal_network import skeletal_feature_extraction as sfe
    from mgr_amd.skeletal_network import skeletal_lstm_ctc as sk
    sfe._DEV[0] = device
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(31)
    ids = [396, 397, 398, 399, 400, 401, 402, 403, 404]
    d = _raw_dir(tmp_path / 'raw', rng, ids, n_lo=40, n_hi=60)
    train, val = act.skeletal_tables(d)
    assert sorted(train['file_number'].unique()) == ids[:-1] and val['file_number'].unique().tolist() == [404]
    labels = tmp_path / 'labels.csv'
    labels.write_text("Id,Sequence\n" + "".join("%d,%s\n" % (f, " ".join(str(v) for v in rng.integers(1, 21, 3))) for f in ids))

    # skeletal network: raw joint files -> gathered table -> CsvStore -> DataGenerator(store=) -> fit_generator
    store = datagen.CsvStore(None, train, str(labels))
    assert store.file_ids() == ids[:-1]
    maxlen, bs = 40, 2
    gen = sk.DataGenerator(bs, 20, maxlen, 0.25, 22, store=store)
    assert gen.store is store and gen.train_size == 6
    x, _ = gen.get_batch(True)
    assert x['the_input'].shape == (bs, maxlen, 20) and np.isfinite(x['the_input']).all()
    model = sk.build_model(maxlen, 20, 22, 28, 'no', units=16, device=device)
    hist = model.fit_generator(gen.next_train(), steps_per_epoch=2, epochs=1, verbose=0, callbacks=[gen])
    assert np.all(np.isfinite(hist.history['loss']))

    # fusion network: WAV files + the gathered table
    wav_dir = tmp_path / 'wav'
    wav_dir.mkdir()
    for f in ids[:-1]:
        fe.write_wav(str(wav_dir / ('Sample%05d_audio.wav' % f)), (rng.standard_normal(24000) * 2000).astype(np.int16), 16000)
    wstore = datagen.WavStore(str(wav_dir), skeletal_csv=train, label_csv=str(labels), dev=device)
    assert wstore.file_ids() == ids[:-1] and sorted(wstore.skel) == ids[:-1]
    fgen = fdg.DataGenerator(bs, 20, 39, maxlen, 22, 'train', val_split=0.25, store=wstore)
    fmodel = multimodal.build_model(maxlen, 39, 20, 22, 35, device=device)
    hist = fmodel.fit_generator(fgen.next_train(), steps_per_epoch=2, epochs=1, verbose=0, callbacks=[fgen])
    assert np.all(np.isfinite(hist.history['loss']))

    # RGB network: extract_body takes the gathered table for its hipX / hipY / shcY
    vid = tmp_path / 'video'
    vid.mkdir()
    for f in ids[:2]:
        n = int((train['file_number'] == f).sum())
        np.save(vid / ('Sample%05d_color.npy' % f), rng.integers(0, 256, (n, 480, 640, 3), dtype=np.uint8))
    written = roi.extract_body(train, str(vid), str(tmp_path / 'crops'), img_dim=16, dev=device)
    assert len(written) == 2
    for p, f in zip(written, ids[:2]):
        c = np.load(p)
        assert c.shape == (int((train['file_number'] == f).sum()), 16, 16, 1) and c.dtype == np.uint8
