"""-m gpu: the BASELINE.json configs that are parity cases rather than bench lines.
 A  audio plumbing  : 2-layer BiLSTM(128)+CTC, B=8,  T=200,  39-d, full size, loss + softmax + gradients vs oracle (the step runs
                      with apply_update=False: the update kernels have their own tests, test_gpu_update_kernels.py elementwise against fp64, and
                      the weight movement of the golden and max-norm trajectories of test_gpu_network.py)
 S  skeletal        : BiLSTM(128)+CTC,         B=32, T=1000, 22-d, full size, loss vs oracle (1e-4 relative)
 F  fusion (ref sizes 500/300/100) at B=4, T=96 and at the full T=1900 with B=2: loss + trainable grads
 E  early fusion: 2x BiLSTM(500) on the 59-d concatenated input, all trainable, B=4, T=64
 D  decode          : beam=10 and thresholded best-path on T=1900 sequences, label sequences bit-exact vs the oracle
The all-trainable networks at the reference's own sizes and lengths (A_ref, S_ref, E at T = 1000 / 1900): test_gpu_reference_shapes.py.
"""
import numpy as np
import pytest

from oracle import keras_ref as kr
from oracle import network_ref as nr
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu


def _run_case(device, key, B=None, T=None, lmin=3, lmax=10, check_grads=True, seed=0, wscale=2.0):
    import mgr_amd  # noqa: F401
    from mgr_amd.configs import baseline_config
    from mgr_amd.engine import Engine
    from mgr_amd.synthetic import synthetic_arrays, synthetic_weights
    spec, B0, T0, Lmax = baseline_config(key)
    B, T = B or B0, T or T0
    eng = Engine(spec, B, T, Lmax, device=device, seed=seed)
    w = synthetic_weights(spec, 100 + seed)
    # stronger recurrent / input weights than the init recipe so that gates leave their linear region
    for k in w:
        if k.endswith("/W") or k.endswith("/U"):
            w[k] = w[k] * wscale
    eng.set_weights(w)
    xs, labels, il, ll = synthetic_arrays(spec, B, T, Lmax, 200 + seed, lmin=lmin, lmax=lmax)
    sd = spec.to_dict()
    rand = nr.draw_rand(sd, B, T, np.random.default_rng(300 + seed))
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    ref_loss, ref_lb, ref_g, ref_P = nr.loss_and_grads(sd, w64, xs, labels, il, ll, rand)
    eng.enqueue_train_step(xs, labels, il, ll, rand=rand, apply_update=False)
    loss = float(eng.loss_mean.download()[0])
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss), (key, loss, ref_loss)
    assert np.allclose(eng.loss_b.download(), ref_lb, rtol=1e-4)
    # What bounds the activations and gradients is fp32 arithmetic itself, not the kernels: the SAME oracle run in float32 (numpy /
    # OpenBLAS, yet another summation order) sits at a comparable distance from the fp64 run.  The GPU figures are held to a small
    # multiple of that distance (the error model) and, as an outer limit, to the absolute caps used since round 1: softmax 3e-4,
    # gradients 5e-3 of the tensor maximum (fp32 BPTT through 200-1900 steps x 2 layers amplifies rounding; with doubled weights
    # the recurrence amplifies it further: 1.8e-4 .. 2.2e-4 at config A depending on the scan kernel's summation order).
    f32 = lambda d: {k: np.asarray(v, np.float32) for k, v in d.items()}
    rand32 = {k: (None if v is None else np.asarray(v, np.float32)) for k, v in rand.items()}
    _, _, g32, P32 = nr.loss_and_grads(sd, f32(w), f32(xs), labels, il, ll, rand32)
    eP, eP32 = rel_err(eng.P.download(), ref_P), rel_err(P32, ref_P)
    print("%s B=%d T=%d wscale=%g: softmax err gpu %.2e, numpy-f32 %.2e" % (key, B, T, wscale, eP, eP32))
    assert eP < 3e-4 and eP < max(4.0 * eP32, 2e-5), (key, "softmax", eP, eP32)
    if check_grads:
        g = eng.get_grads()
        assert set(g) == set(ref_g)
        for k in ref_g:
            eg, eg32 = rel_err(g[k], ref_g[k]), rel_err(g32[k], ref_g[k])
            print("   grad %-28s gpu %.2e, numpy-f32 %.2e" % (k, eg, eg32))
            assert eg < 5e-3 and eg < max(4.0 * eg32, 1e-4), (key, k, eg, eg32)
    eng.close()
    return loss


def test_config_A_audio_plumbing_full_size(device):
    _run_case(device, "A")


def test_config_S_skeletal_full_size(device):
    # the SURVEY 8(d) weight recipe as is: with doubled weights the T=1000 recurrence is chaotic enough that fp32 and
    # fp64 forward passes drift apart by ~1e-3 in the loss (a property of the dynamics, not of the kernels: the same
    # doubled-weight network matches to 1e-4 at T=200, test A)
    _run_case(device, "S", lmin=8, lmax=20, wscale=1.0)


def test_config_S_short_T_strong_weights(device):
    _run_case(device, "S", B=32, T=120, lmin=3, lmax=10, wscale=2.0)


def test_config_F_reference_sizes_short_T(device):
    _run_case(device, "F", B=4, T=96)


def test_config_F_reference_sizes_full_T(device):
    """The metric's own sequence length: T = 1900 through 500/300/100-unit BiLSTMs and the CTC, B = 2, loss and softmax
    and trainable gradients against the fp64 oracle (recipe weights: with doubled weights a 1900-step recurrence is chaotic, see config S)."""
    _run_case(device, "F", B=2, T=1900, lmin=8, lmax=20, check_grads=True, wscale=1.0)


def test_config_F_ragged_batch_not_multiple_of_16(device):
    _run_case(device, "F", B=19, T=40, seed=1)


def test_config_E_early_fusion_short_T(device):
    _run_case(device, "E", B=4, T=64)


def test_config_D_decode_long_sequences(device):
    from mgr_amd import decoding
    rng = np.random.default_rng(5)
    N, T, C = 3, 1900, 22
    # run-structured, peaky posteriors like a trained CTC network produces
    z = rng.standard_normal((N, T, C)) * 1.5
    z[:, :, C - 1] += 3.0
    for n in range(N):
        t = 20
        while t < T - 40:
            c = int(rng.integers(0, C - 1))
            run = int(rng.integers(5, 40))
            z[n, t:t + run, c] += rng.uniform(3.0, 9.0)
            t += run + int(rng.integers(10, 90))
    P = np.exp(z - z.max(-1, keepdims=True))
    P = (P / P.sum(-1, keepdims=True)).astype(np.float32)
    assert decoding.greedy_decode(P, 0.5, dev=device) == kr.greedy_decode_quirk(P, 0.5)
    il = np.full(N, T - 2)
    ref, rs = kr.ctc_beam_search(P, il, beam_width=10)
    got, gs = decoding.beam_search_decode(P, il, beam_width=10, dev=device)
    assert got == ref
    assert np.allclose(gs, rs, rtol=1e-10)
    # LER helper: identical hypotheses -> 0
    assert decoding.label_error_rate(got, ref) == 0.0
