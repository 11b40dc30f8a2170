"""bench.py --dump-outputs on CPU: what dump_outputs writes (names, float32, the byte limit, the seeded sample of positions and the
values at them) and the options a plain run is driven by; the GPU run itself is in test_gpu_bench.py."""
import os
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import bench  # noqa: E402


def _outputs(rows, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g).to(torch.bfloat16) for _ in range(rows)]


def test_small_outputs_are_written_whole_as_float32(tmp_path):
    dq, gv = _outputs(3, 1000, 1), _outputs(3, 64, 2)
    written = bench.dump_outputs(str(tmp_path), {"dequant_out": dq, "gemv_out": gv})
    assert sorted(written) == sorted(os.listdir(tmp_path)) == ["dequant_out.npy", "gemv_out.npy"]
    for name, src in (("dequant_out.npy", dq), ("gemv_out.npy", gv)):
        arr = np.load(tmp_path / name)
        assert arr.dtype == np.float32 and arr.shape == (3, src[0].numel())
        assert np.array_equal(arr, torch.stack(src).float().numpy())  # bf16 -> f32 is exact
        assert written[name] == os.path.getsize(tmp_path / name)


def test_outputs_above_the_limit_are_a_fixed_sample_of_positions(tmp_path):
    limit = 200_000
    dq, gv = _outputs(4, 100_000, 3), _outputs(4, 256, 4)
    written = bench.dump_outputs(str(tmp_path / "a"), {"dequant_out": dq, "gemv_out": gv}, limit=limit)
    assert sorted(written) == ["dequant_out_sample.npy", "gemv_out.npy"] and sum(written.values()) <= limit
    arr = np.load(tmp_path / "a" / "dequant_out_sample.npy")
    count = arr.shape[1]
    assert arr.dtype == np.float32 and arr.shape[0] == 4 and 0 < count < 100_000
    pos = bench.sample_positions(100_000, count)
    assert len(np.unique(pos)) == count and (np.diff(pos) > 0).all() and pos[-1] < 100_000
    assert np.array_equal(arr, torch.stack(dq).float().numpy()[:, pos])
    # the same call writes the same file: the sample does not depend on the run
    bench.dump_outputs(str(tmp_path / "b"), {"dequant_out": dq, "gemv_out": gv}, limit=limit)
    assert np.array_equal(np.load(tmp_path / "b" / "dequant_out_sample.npy"), arr)


def test_ranks_share_the_limit_and_name_their_files(tmp_path):
    limit, world = 400_000, 4
    total = 0
    for rank in range(world):
        written = bench.dump_outputs(str(tmp_path), {"dequant_out": _outputs(2, 200_000, rank), "gemv_out": _outputs(2, 128, rank)},
                                     rank, world, limit=limit)
        suffix = "" if rank == 0 else f"_rank{rank}"
        assert sorted(written) == [f"dequant_out_sample{suffix}.npy", f"gemv_out{suffix}.npy"], written
        total += sum(written.values())
    assert total <= limit and len(os.listdir(tmp_path)) == 2 * world


def test_the_default_limit_is_64_mb():
    assert bench.DUMP_LIMIT_BYTES == 64 * 10**6


def test_the_options_of_a_plain_and_a_full_run():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-1500:]
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs", "--no-cpu"):
        assert opt in p.stdout, opt
