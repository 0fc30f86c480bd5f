"""The randomness a device-RNG pass of the engine consumes, restated on the CPU (test infrastructure, NOT product code).

With rand=None the engine draws nothing on the host: every input-dropout mask is filled by mgr_dropout_mask, the Gaussian noise is
added by mgr_add_gaussian_noise and the head's Dropout is decided inside the Dense kernels, each from one 64-bit seed.  The
generator is stateless (tests/update_ref.py restates it bit for bit), so the `rand` dict that oracle.network_ref takes can be
rebuilt from (spec, B, T, engine seed, step counter) alone: replay() does that.  Nothing here is imported from the engine; this
is the one place where the test suite writes the engine's order of seeds down.

Seed of a site (Engine._seed):  (seed * 1000003 + rng_step * 131 + slot) mod 2^64.

rng_step (Engine.rng_step) starts at 0 and advances by one per training-phase forward pass - a training step
(Engine._enqueue_trainable_part), loss_on_batch / forward_train_phase with the learning phase on (Engine._forward); predict draws
nothing and leaves it alone.  ALL sites of one pass use the same rng_step, whichever call of the pipelined schedule enqueues them.

Slots:
  1, 2, ...   the encoder layers' input-dropout masks (Engine._encoder_phases): depth-major - every stream's layer 0, then every
              stream's layer 1 -, within a depth the streams in spec order, within a layer fwd then bwd.  A stream with fewer
              layers is skipped at the deeper depths; a layer with dropout 0 takes its two slots all the same and draws nothing.
              fusion_tiny: audio/l0 1, 2; skeletal/l0 3, 4; audio/l1 5, 6; skeletal/l1 7, 8.
  500, 501    the fusion layer's fwd / bwd mask (Engine._enqueue_fusion_head).
  900 + i     the Gaussian noise of stream i in spec order (Engine._encoder_phases); streams without noise keep their number.
  999         the head's Dropout (Engine._enqueue_fusion_head; read by mgr_head_fwd_bwd / mgr_dense_softmax_fwd / mgr_dense_bwd).

Values:
  mask [4, B, fin]   element i of the flat buffer is drop_scale(seed, i, p): 0 or the float32 1 / (1 - p) (Engine._prep_mask).
  head (B, T, D)     element f * D + d of frame f = b * T + t, the same function (csrc/dense.hip: drop_factor).
  noise (B, T, F)    the additive tensor: noise_ref(zeros, B T F, stddev, seed) - pairs of elements share one Box-Muller draw.
Keys, shapes and dtype (float64) are oracle.network_ref.draw_rand's; a site with p <= 0 (noise <= 0) has no key."""
import numpy as np

from tests import update_ref as ur

M64 = (1 << 64) - 1
SEED_MUL, STEP_MUL = 1000003, 131
FUSION_SLOTS = (500, 501)
NOISE_SLOT = 900
HEAD_SLOT = 999


def site_seed(seed, rng_step, slot):
    return (int(seed) * SEED_MUL + int(rng_step) * STEP_MUL + int(slot)) & M64


def sites(spec, B, T):
    """Every place of a training-phase pass that owns a slot, drawn from or not: [(key, slot, shape, rate, kind)] with kind
    "mask" (rate: dropout p) or "noise" (rate: stddev)."""
    out = []
    streams = spec["streams"]
    for i, s in enumerate(streams):
        out.append((s["name"] + "/noise", NOISE_SLOT + i, (B, T, s["F"]), float(s.get("noise", 0.0)), "noise"))
    slot = 0
    for k in range(max(len(s["layers"]) for s in streams)):
        for s in streams:
            if k >= len(s["layers"]):
                continue
            fin = s["F"] if k == 0 else 2 * s["layers"][k - 1]["H"]
            for d in ("fwd", "bwd"):
                slot += 1
                out.append(("%s/l%d/%s/mask" % (s["name"], k, d), slot, (4, B, fin), float(s["layers"][k].get("dropout", 0.0)), "mask"))
    width = sum(2 * s["layers"][-1]["H"] for s in streams)
    if spec.get("fusion"):
        for d, slot in zip(("fwd", "bwd"), FUSION_SLOTS):
            out.append(("fusion/%s/mask" % d, slot, (4, B, width), float(spec["fusion"].get("dropout", 0.0)), "mask"))
        width = 2 * spec["fusion"]["H"]
    out.append(("head/mask", HEAD_SLOT, (B, T, width), float(spec["head"].get("dropout", 0.0)), "mask"))
    return out


def replay(spec, B, T, seed, rng_step):
    """The `rand` dict of the pass that engine `seed` runs at step counter `rng_step`."""
    r = {}
    for key, slot, shape, rate, kind in sites(spec, B, T):
        if rate <= 0:
            continue
        n = int(np.prod(shape))
        sd = site_seed(seed, rng_step, slot)
        if kind == "noise":
            if any(s.get("frontend") for s in spec["streams"] if s["name"] + "/noise" == key):
                raise NotImplementedError("a CNN front-end takes no GaussianNoise")
            v = ur.noise_ref(np.zeros(n), n, rate, sd)
        else:
            v = ur.drop_scale(sd, np.arange(n, dtype=np.uint64), rate)
        r[key] = np.asarray(v, np.float64).reshape(shape)
    return r
