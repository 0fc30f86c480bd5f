"""-m gpu: `bench.py --gpus 1` end to end, in a process of its own (started from the fork server tests/conftest.py starts before
anything touches the GPU: a process that has initialised the GPU must not exec).  A plain run prints the headline and takes no leg
beside it; --full adds the f32 MFMA leg, the CTC parity against the fp64 oracle and the CPU baseline."""
import json
import multiprocessing as mp
import os

import pytest

from tests import dp_worker

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "16", "--maxlen", "96"]


def _bench_line(tmp_path, argv, timeout=240):
    from multiprocessing import forkserver
    if getattr(forkserver._forkserver, "_forkserver_pid", None) is None:
        pytest.skip("the fork server must be started before the GPU is initialised: run through `pytest -m gpu` (tests/conftest.py)")
    out = str(tmp_path / "bench.json")
    p = mp.get_context("forkserver").Process(target=dp_worker.run_bench, args=(out, argv, timeout))
    p.start()
    p.join(timeout + 30)
    assert not p.is_alive() and os.path.exists(out)
    rec = json.load(open(out))
    assert rec["rc"] == 0, rec
    lines = [l for l in rec["stdout"].splitlines() if l.startswith("{")]
    assert len(lines) == 1, rec
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_takes_no_leg_beside_it(device, tmp_path):
    d = _bench_line(tmp_path, SMALL + ["--dump-outputs", str(tmp_path / "dump")])
    assert d["metric"] == "train frames/sec, fusion BiLSTM+CTC" and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert abs(d["value"] - 16 * 96 * 1e3 / d["ms_per_step"]) <= 2e-3 * d["value"]     # frames of one step over its time
    assert d["f32_mfma_path"] is None and d["ctc_loss_parity"] is None and d["cpu_baseline"] is None and d["speedup_vs_cpu"] is None
    assert os.path.exists(tmp_path / "dump" / "loss.npy")


def test_full_run_adds_the_f32_leg_the_oracle_parity_and_the_cpu_baseline(device, tmp_path):
    d = _bench_line(tmp_path, SMALL + ["--full", "--cpu-T", "48"])
    assert d["f32_mfma_path"]["steps"] == 3 and d["f32_mfma_path"]["ms_per_step"] > 0
    p = d["ctc_loss_parity"]
    assert p["shape"] == "B=2,T=96" and p["rel_delta"] < 1e-4 and p["f32_mfma_path"]["rel_delta"] < 1e-4
    assert p["grad_max_rel_err"] < 1e-3 and p["f32_mfma_path"]["grad_max_rel_err"] < 1e-3
    assert d["cpu_baseline"]["value"] > 0 and "B=16 T=48" in d["cpu_baseline"]["sample"] and d["speedup_vs_cpu"] > 0
