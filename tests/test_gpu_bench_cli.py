"""bench.py's command line, as a fresh process at a reduced size.

A plain run (`--gpus 1 --steps K --warmup W`) reports the headline fields and
none of what `--full` adds; `--dump-outputs DIR` writes what the last timed
step computed -- `y` (here 70000 rows of 512 B, over half of
bench.DUMP_BUDGET, so the seeded row sample is exercised) and every weight and
bias gradient -- as float32 .npy files of at most DUMP_BUDGET bytes together.
The dumped arrays are checked against the same step run in this process:
the forward is deterministic, so `y` bit for bit; the gradients within fp32
summation order (1e-5 of each gradient's largest entry).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODES, PAIRS, FEAT, LAYERS = 70_000, 350_000, 128, 3
FULL_ONLY = ("kernels", "kernel_templates", "roofline", "cpu_baseline")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--nodes", str(NODES), "--pairs", str(PAIRS), *extra]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_last_step(cuda, tmp_path):
    import bench
    d = str(tmp_path / "dump")
    r = _bench("--dump-outputs", d)
    assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["unit"] == "edges/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["ms_per_step"] > 0
    assert r["value"] == pytest.approx(2 * PAIRS * LAYERS / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert not any(k in r for k in FULL_ONLY)

    names = ["y"] + [f"grad_{p}{i}" for i in range(LAYERS) for p in "Wb"]
    assert sorted(os.listdir(d)) == sorted(n + ".npy" for n in names)
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET
    assert r["dumped_outputs"] == {n: list(a.shape) for n, a in got.items()}

    ei, N = bench.make_er_graph(NODES, PAIRS)
    X, Ws, bs, dY = bench.make_inputs(N, FEAT, LAYERS)
    step, params = bench.build_stack(cuda, ei, X, Ws, bs, dY)
    y = step()
    keep = (bench.DUMP_BUDGET // 2) // (4 * FEAT)
    assert keep < N
    rows = torch.randperm(N, generator=torch.Generator().manual_seed(bench.DUMP_SEED))[:keep]
    rows = rows.sort().values
    np.testing.assert_array_equal(got["y"], y.detach()[rows.to(cuda)].cpu().numpy())
    for i, p in enumerate(params):  # W0, b0, W1, b1, ...
        g = p.grad.cpu().numpy()
        np.testing.assert_allclose(got[f"grad_{'Wb'[i % 2]}{i // 2}"], g, rtol=1e-5,
                                   atol=1e-5 * float(np.abs(g).max()))


def test_full_run_adds_kernel_figures(cuda):
    r = _bench("--full")
    assert r["ms_per_step"] > 0 and r["cpu_baseline"]["value"] > 0
    assert r["roofline"]["frac"] > 0 and r["roofline"]["kernel"].startswith("spmm_xw")
    assert set(r["kernel_templates"]) and set(r["kernels"])
