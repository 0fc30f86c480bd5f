"""-m gpu: the RGB network (rgb_network/cnn_lstm.py) on the MI355X - the CNN front-end kernels through the C ABI against torch fp64,
a BiLSTM(512) layer on F = 768 inputs, whole RGB train steps against the fp64 oracle, determinism and the inference path."""
import numpy as np
import pytest

from tests.conv_harness import run_layer as _run_layer      # (guarded outputs, NaN-filled workspace: shared with test_gpu_conv_edges.py)
from tests.helpers import rel_err
from tests.rgb_ref import conv_layer, conv_layer_routed, loss_and_grads, reference_code

pytestmark = pytest.mark.gpu

# (Hin, Cin, ks, Cout) of conv_1 / conv_3 / conv_5 at img_dim = 60
LAYERS = {"conv_1": (60, 1, 5, 16), "conv_3": (28, 16, 5, 32), "conv_5": (12, 32, 4, 48)}


def _layer_case(layer, N, seed, constant=False):
    Hin, Cin, ks, Cout = LAYERS[layer]
    rng = np.random.RandomState(seed)
    if constant:   # constant frames: every window of a channel ties (or is a ReLU zero)
        x = np.repeat(rng.uniform(0, 1, (N, 1, 1, Cin)), Hin, 1).repeat(Hin, 2).astype(np.float32)
    else:
        x = rng.uniform(0 if Cin > 1 else -0.5, 1, (N, Hin, Hin, Cin)).astype(np.float32)
    W = rng.uniform(-0.05, 0.05, (ks, ks, Cin, Cout)).astype(np.float32)
    b = rng.uniform(-0.02, 0.02, Cout).astype(np.float32)
    Hp = (Hin - ks + 1) // 2
    dY = rng.standard_normal((N, Hp, Hp, Cout)).astype(np.float32)
    return x, W, b, dY, ks


@pytest.mark.parametrize("layer", sorted(LAYERS))
@pytest.mark.parametrize("N,constant", [(37, False), (1000, False), (37, True)])
def test_conv_layer_matches_fp64(device, layer, N, constant):
    x, W, b, dY, ks = _layer_case(layer, N, 7 + N, constant)
    Y, dX, gW, gb, code, rep = _run_layer(device, x, W, b, dY, ks)
    rY = conv_layer(x, W, b, dY)[0]
    assert rel_err(Y, rY) < 1e-5
    # routing: the f32 forward's window choice is the fp64 one wherever the two largest values are apart by more than f32 rounding
    code = code.reshape(Y.shape)
    pre, rdX, rW, rb = conv_layer_routed(x, W, b, dY, code)
    rcode, gap = reference_code(pre)
    tol = 1e-5 * np.abs(pre).max()
    clear = gap > tol
    assert np.array_equal(code[clear], rcode[clear])
    dead = pre.max(-1) < -tol                     # every value of the window a ReLU zero: no gradient at all
    assert (code[dead] == 255).all()
    assert (clear | dead).mean() > 0.99 or constant
    # gradients through that routing
    if layer != "conv_1":            # (conv_1's input is data: the engine never asks for its dX; the kernel computes it anyway)
        assert rel_err(dX, rdX) < 1e-5
    assert rel_err(gW, rW) < 1e-5, rel_err(gW, rW)
    assert rel_err(gb, rb) < 1e-5
    assert np.array_equal(gW, rep)   # the weight gradient is deterministic: a second launch gives the same bits
    if constant:
        assert set(np.unique(code)) <= {0, 255}        # ties go to the first position; ReLU-zero windows route nothing
        assert (code == 0).any() and (code == 255).any()


def _train_engine(device, spec, B, T, Lmax, seed=3):
    from mgr_amd.engine import Engine
    from mgr_amd.keras_like import Model
    eng = Engine(spec, B, T, Lmax, device=device)
    eng.set_weights(Model(spec, device=device).get_weights_dict())
    rng = np.random.RandomState(seed)
    w = eng.get_weights()
    for k in w:                       # (non-zero biases: every gradient path is exercised)
        if k.endswith("/b"):
            w[k] = rng.uniform(-0.05, 0.05, w[k].shape).astype(np.float32)
    eng.set_weights(w)
    return eng, eng.get_weights()


def _batch(spec, B, T, Lmax, seed):
    s = spec.streams[0]
    rng = np.random.RandomState(seed)
    if s.get("frontend"):
        x = rng.uniform(0, 1, (B, T) + tuple(s["frontend"]["input_shape"]))
        x = ((x * 255 - 128) / 255).astype(np.float32)
    else:
        x = rng.standard_normal((B, T, s["F"])).astype(np.float32)
    L = rng.randint(3, Lmax + 1, B)
    labels = np.full((B, Lmax), -1, np.int32)
    for i in range(B):
        labels[i, :L[i]] = rng.randint(0, spec.num_classes - 1, L[i])
    return x, labels, np.full(B, T - 2, np.int32), L.astype(np.int32)


def _check_step(eng, spec, x, labels, il, ll, wref):
    eng.enqueue_train_step({spec.streams[0]["name"]: x}, labels, il, ll, rand={}, apply_update=False)
    loss = float(eng.loss_mean.download()[0])
    w64 = {k: v.astype(np.float64) for k, v in wref.items()}
    if spec.streams[0].get("frontend"):
        fe = eng.fe[spec.streams[0]["name"]]["layers"]
        codes = {c["name"]: c["code"].download().reshape(-1, c["Hp"], c["Wp"], c["Cout"]) for c in fe}
        rloss, rloss_b, rg, rP = loss_and_grads(spec.to_dict(), w64, x, labels, il, ll, codes=codes)
    else:
        from oracle import network_ref as nr
        rloss, rloss_b, rg, rP = nr.loss_and_grads(spec.to_dict(), w64, {spec.streams[0]["name"]: x.astype(np.float64)}, labels, il, ll)
    assert abs(loss - rloss) <= 1e-4 * abs(rloss), (loss, rloss)
    assert rel_err(eng.P.download(), rP) < 1e-4
    g = eng.get_grads()
    assert set(g) == set(rg)
    bad = {k: rel_err(g[k], rg[k]) for k in rg if rel_err(g[k], rg[k]) >= 1e-4}
    assert not bad, bad


def test_bilstm512_on_768_features_matches_fp64(device):
    """One BiLSTM(512) on F = 768 inputs (the RGB network's first LSTM layer alone): H = 512 exactly, which no other test runs."""
    from mgr_amd.spec import NetworkSpec
    spec = NetworkSpec([{"name": "the_input", "F": 768, "layers": [{"H": 512, "dropout": 0.0, "name": "blstm_1"}]}], None,
                       {"dropout": 0.0, "C": 22}, optimizer={"lr": 1e-4, "decay": 0.0, "clipvalue": 0.5, "maxnorm": 3.0})
    B, T, Lmax = 2, 24, 6
    eng, w = _train_engine(device, spec, B, T, Lmax)
    _check_step(eng, spec, *_batch(spec, B, T, Lmax, 11), w)
    eng.close()


def test_rgb_train_step_matches_fp64(device):
    from mgr_amd import configs
    spec = configs.rgb_spec(h=64)
    B, T, Lmax = 2, 64, 12
    eng, w = _train_engine(device, spec, B, T, Lmax)
    _check_step(eng, spec, *_batch(spec, B, T, Lmax, 5), w)
    eng.close()


def test_rgb_train_step_reference_size_matches_fp64(device):
    """H = 512, T = 1900, B = 2: the reference's sizes."""
    from mgr_amd import configs
    spec = configs.rgb_spec()
    B, T, Lmax = 2, 1900, 35
    eng, w = _train_engine(device, spec, B, T, Lmax)
    _check_step(eng, spec, *_batch(spec, B, T, Lmax, 9), w)
    eng.close()


def test_rgb_three_steps_twice_are_bit_identical(device):
    from mgr_amd import configs
    spec = configs.rgb_spec(h=64)
    B, T, Lmax = 2, 48, 10
    finals = []
    for _ in range(2):
        eng, _w = _train_engine(device, spec, B, T, Lmax)
        losses = []
        for s in range(3):
            x, labels, il, ll = _batch(spec, B, T, Lmax, 100 + s)
            losses.append(eng.train_step({"the_input": x}, labels, il, ll))
        assert np.all(np.isfinite(losses))
        finals.append(eng.get_weights())
        eng.close()
    for k in finals[0]:
        assert np.array_equal(finals[0][k], finals[1][k]), k


def test_rgb_predict_equals_training_phase_forward(device):
    """Every dropout rate of the network is 0 and it has no noise: learning phase 0 and 1 run the same kernels on the same
    inputs, so the posteriors agree bit for bit."""
    from mgr_amd import configs
    spec = configs.rgb_spec(h=64)
    B, T, Lmax = 2, 40, 8
    eng, _w = _train_engine(device, spec, B, T, Lmax)
    x = _batch(spec, B, T, Lmax, 21)[0]
    p0 = eng.predict({"the_input": x})
    p1 = eng.forward_train_phase({"the_input": x})
    assert np.array_equal(p0, p1)
    streamed = list(eng.predict_stream([{"the_input": x}, {"the_input": x}]))
    assert all(np.array_equal(p, p0) for p in streamed)
    eng.close()


def test_rgb_fit_generator_checkpoint_and_decode(device, tmp_path):
    from mgr_amd.keras_like import ModelCheckpoint
    from mgr_amd.rgb_network import cnn_lstm, decode_rgb
    maxlen, bs = 40, 2
    gen = cnn_lstm.DataGenerator(minibatch_size=bs, img_dim=32, maxlen=maxlen, synthetic_files=8, val_split=0.25)
    model = cnn_lstm.build_net(img_dim=32, maxlen=maxlen, h=32, device=device)
    ck = str(tmp_path / "rgb_weights.h5")
    hist = model.fit_generator(gen.next_train(), steps_per_epoch=gen.get_size(True) // bs, epochs=2, verbose=0,
                               callbacks=[ModelCheckpoint(ck, monitor="loss", save_weights_only=True), gen],
                               validation_data=gen.next_val(), validation_steps=1)
    assert all(np.isfinite(v) for v in hist.history["loss"])
    back = cnn_lstm.build_net(img_dim=32, maxlen=maxlen, h=32, device=device)
    back.load_weights(ck)
    w0, w1 = model.get_weights_dict(), back.get_weights_dict()
    assert all(np.array_equal(w0[k], w1[k]) for k in w0)
    pred = decode_rgb.prediction_model(back)
    files = gen.val_list
    out = pred.predict_generator(gen.predict_batches(files), steps=(len(files) + bs - 1) // bs)
    seqs = decode_rgb.decode_batch(out[:len(files)], files, out_file=str(tmp_path / "rec.mlf"))
    assert len(seqs) == len(files) and all(isinstance(s, list) for s in seqs)
