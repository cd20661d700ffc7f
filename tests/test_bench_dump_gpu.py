"""`bench.py --dump-outputs DIR`: what the LAST timed step handed its caller (y, grad_x and every parameter gradient),
against the oracle on the same seeded inputs; and a plain run's line carries the headline without what --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, TOL_ACT, TOL_PARAM, rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(600)
def test_dump_outputs_are_the_last_timed_step(gpu, tmp_path):
    B, N, D = 2, 1024, 64
    # 5 steps at 2 per hipGraph: two replays of one graph, then the remainder graph runs the last step
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--steps-per-graph", "2", "--preheat-ms", "0", "--batch", str(B), "--seq", str(N), "--dim", str(D),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=550)
    assert p.returncode == 0, p.stderr[-3000:]
    js = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(js) == 1, p.stdout
    out = json.loads(js[0])
    assert out["steps"] == 5 and out["ms_per_step"] > 0 and out["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in out
    for k in ("roofline", "box", "cpu_baseline", "other_configs"):
        assert k not in out, k                                   # --full only

    import bench
    import tensor_cuda_fft_amd as pkg
    from oracle import spectral_oracle as so
    cfg = dict(B=B, N=N, D=D, F=D // 2, api="layer")
    _, _, (wr, wi, b) = bench.make_unit(pkg, cfg, gpu, seed=1234)
    gen = torch.Generator(device=gpu).manual_seed(1234)
    x = torch.randn(B, N, D, device=gpu, generator=gen).cpu().numpy()
    g = torch.randn(B, N, D, device=gpu, generator=gen).cpu().numpy()
    wr, wi, b = (t.detach().cpu().numpy() for t in (wr, wi, b))
    y_ref, _ = so.forward_closed(x, wr, wi, b)
    gx_ref, gwr_ref, gwi_ref, gb_ref = so.backward_closed(x, wr, wi, g)

    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["grad_bias", "grad_weight_imag", "grad_weight_real", "grad_x", "y"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert rel_err(got["y"], y_ref) <= TOL_ACT
    assert rel_err(got["grad_x"], gx_ref) <= TOL_ACT
    assert rel_err(got["grad_weight_real"], gwr_ref) <= TOL_PARAM
    assert rel_err(got["grad_weight_imag"], gwi_ref) <= TOL_PARAM
    assert rel_err(got["grad_bias"], gb_ref) <= TOL_PARAM
