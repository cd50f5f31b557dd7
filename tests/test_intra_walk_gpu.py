"""The pictures of tests/intra_walk_cases.py on the device: a batch per sample format through
the lanes parse, k_transform and k_intra, and one picture through k_intra_stream, every
reconstructed, deblocked and SAO-filtered plane against the oracle; each batch is decoded
twice.  Once with the luma / chroma wave split forced off and once forced on: a child process
each, as in test_lanes_culist_gpu.py (the library reads HEIFGPU_INTRA_SPLIT once per process)."""
import os
import pathlib
import subprocess
import sys

import pytest

pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["0", "1"])
def test_gpu_intra_walk_pictures(split):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    env = {**os.environ, "HEIFGPU_INTRA_SPLIT": split}
    for k in ("HEIFGPU_INTRA_WAVES", "HEIFGPU_STREAM", "HEIFGPU_STREAM_PATIENCE_US", "HEIFGPU_LANES_VARIANT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "intra_walk_cases.py")], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=120)
    out = r.stdout + r.stderr
    print(out[-3000:])
    assert r.returncode == 0 and f"INTRA WALK GPU OK split={split}" in out, out[-3000:]
