"""GPU: a plain `python bench.py --gpus 1` run prints the headline line and nothing that takes runs of its own (those need
--full), and `--dump-outputs` writes what the last timed step handed its caller: the oracle's update of the same increment."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,K", [(50_000, 7), (200_000, 8)])
def test_plain_run_prints_the_headline_and_dumps_the_last_step(gpu_available, tmp_path, n, K):
    """K = 7 ends on the handle of increment 2 (the one of step 0), K = 8 on that of increment 3; n = 200 000 > DUMP_ROWS
    dumps the seeded sample of rows."""
    if not gpu_available:
        pytest.skip("no GPU")
    import bench
    from oracle import constitutive_np as onp

    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--points", str(n), "--steps", str(K),
                        "--warmup", "2", "--settle-seconds", "0.1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"].startswith("M quadrature-point updates/s") and out["unit"] == "Mpoints/s" and out["higher_is_better"] is True
    assert out["dtype"] == "f64" and out["steps"] == K and out["warmup"] == 2 and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(n / (out["value"] * 1e3) - out["ms_per_step"]) <= 6e-5   # value = n / ms_per_step, to the 4 decimals of ms_per_step
    for k in ("box", "cpu_baseline", "other_laws", "host_path", "gather_inclusive", "cfg3", "process_group"):
        assert k not in out, k
    assert out["roofline"]["stream_probe"] is None and out["roofline"]["measured_copy_GBs"] is None and out["roofline"]["kernel_ms"] > 0

    # step i integrates strain increment i % 3 + 1 (0-based) from the state converged after the increments before it
    hist = bench.history(n, 1234)
    last = (K - 1) % 3 + 1
    hard = onp.LinearHardening(bench.SIG0, bench.H)
    epsp, p = np.zeros((n, 6)), np.zeros(n)
    for eps in hist[:last]:
        ref = onp.j2_update(eps, epsp, p, bench.E, bench.NU, hard)
        epsp, p = ref["epsp"], ref["p"]
    ref = onp.j2_update(hist[last], epsp, p, bench.E, bench.NU, hard)
    rows = np.arange(n) if n <= bench.DUMP_ROWS else np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, bench.DUMP_ROWS, replace=False))
    assert len(rows) == min(n, bench.DUMP_ROWS) and len(np.unique(rows)) == len(rows)
    ref = {k: v[rows] for k, v in ref.items()}
    got = {name: np.load(os.path.join(tmp_path, f"{name}.npy")) for name in ("stress", "tangent", "p", "epsp")}
    assert sorted(os.listdir(tmp_path)) == ["epsp.npy", "p.npy", "stress.npy", "tangent.npy"]
    assert all(a.dtype == np.float64 and a.shape[0] == len(rows) for a in got.values())
    assert ref["plastic"].mean() > 0.3   # (increments 2 and 3 load)
    safe = np.abs(ref["f_trial"]) > 1e-9 * bench.SIG0
    for a, b in ((got["stress"], ref["sig"]), (got["tangent"], ref["Ct"].reshape(-1, 36)), (got["p"][:, 0], ref["p"]), (got["epsp"], ref["epsp"])):
        err = np.abs(a[safe] - b[safe]).max() / max(np.abs(b).max(), 1e-300)
        assert err < 1e-12, err
