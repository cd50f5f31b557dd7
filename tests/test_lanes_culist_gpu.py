"""The pictures of tests/lanes_culist_cases.py on the device: the 4:2:0 geometries in one
batch and a 4:2:2 picture in another (a batch shares one chroma format), forced to the lanes
parse, every deblocked and SAO-filtered plane against the oracle (the deblocking reads the
QpY map that k_paint_flags painted from the CU lists).  Each batch is decoded four times, so
the last decode reuses the first one's parse-output set.  A child process, as in
test_lanes_tbhdr_gpu.py (the library reads its lanes knobs once per process)."""
import os
import pathlib
import subprocess
import sys

import pytest

pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.mark.gpu
def test_gpu_culist_pictures():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    env = {**os.environ}
    env.pop("HEIFGPU_LANES_VARIANT", None)
    env.pop("HEIFGPU_LANES_PPW", None)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "lanes_culist_cases.py")], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=120)
    out = r.stdout + r.stderr
    print(out[-3000:])
    assert r.returncode == 0 and "LANES CULIST GPU OK" in out, out[-3000:]
