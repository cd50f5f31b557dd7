"""The small pictures of tests/lanes_tbhdr_cases.py on the device: batches forced to the
lanes parse, at one and at three pictures per wave, in the lean and the general body,
every deblocked and SAO-filtered plane against the oracle (the deblocking reads the
flag map that k_paint_flags painted from the TB records).  The library reads
HEIFGPU_LANES_PPW once per process, so each setting is a child process
(tests/lanes_tbhdr_cases.py run as a program)."""
import os
import pathlib
import subprocess
import sys

import pytest

pytest.importorskip("heif_amd.synth_encoder")

ROOT = pathlib.Path(__file__).resolve().parents[1]


@pytest.mark.gpu
@pytest.mark.parametrize("ppw", [1, 3])
def test_gpu_tbhdr_pictures(ppw):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    env = {**os.environ, "HEIFGPU_LANES_PPW": str(ppw)}
    env.pop("HEIFGPU_LANES_VARIANT", None)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "lanes_tbhdr_cases.py")], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=120)
    out = r.stdout + r.stderr
    print(out[-3000:])
    assert r.returncode == 0 and "LANES TBHDR GPU OK" in out, out[-3000:]
